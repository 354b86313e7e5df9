// The run machine that the walks along the listed rows share (kgx_kernels_roh.h: one genome, a het closes; kgx_kernels_pair_runs.h: a
// pair of genomes, a mismatch closes): the open run, the report rule and the walk over one 64-position word of events and called
// sites.  What a fold and a close DO differs between the two (where the positions come from, what a closed run is added to), so the
// walk takes them as callables; the order in which it calls them is the semantics of include/kgx.h and exists once, here.
#ifndef KGX_KERNELS_RUNS_H
#define KGX_KERNELS_RUNS_H

#include "kgx_kernels_common.h"

namespace kgx {

struct RohRun { uint32_t first, last, sites; };             // list positions of the first and last called site; sites == 0: no run

__device__ __forceinline__ bool roh_reported(uint32_t sites, unsigned long long length, uint32_t min_sites, uint32_t min_length) {
  return sites >= min_sites && length >= min_length;
}

// One tile of one walker.  events: the bits that close the open run (a het or a mismatch, and the tile's break word); called: the
// bits that extend or open one; the two are disjoint except at a break, whose own cell belongs to the piece that follows it.
// fold(piece): the piece's called sites join the open run, or open one (piece may be 0: nothing).  close(): the open run, if any,
// closes.  The called bits below the first event fold into the open run, which closes; the called bits from the last event up open
// the next run; a piece between two events of the tile is a whole run of at most 63 sites (62 after a het or mismatch, 63 from a
// break at bit 0 to an event at bit 63) -- skipped unseen where min_sites is above that (the usual filter: the tile then costs the
// same whatever its events), else tested by its popcount before anything else is done with it.  Without an event the whole word
// folds in one step.
template <typename Fold, typename Close>
__device__ __forceinline__ void roh_walk_word(unsigned long long events, unsigned long long called, uint32_t min_sites, Fold&& fold, Close&& close) {
  if (events == 0) {
    fold(called);                                             // inside a long run: one merge, no loop
  } else {
    const uint32_t first_event = static_cast<uint32_t>(__builtin_ctzll(events)), last_event = 63u - static_cast<uint32_t>(__builtin_clzll(events));
    fold(called & ((1ull << first_event) - 1ull));
    close();
    if (min_sites <= 63u) {
      unsigned long long pending = events & (events - 1ull);
      uint32_t from = first_event;
      while (pending) {
        const uint32_t to = static_cast<uint32_t>(__builtin_ctzll(pending));
        pending &= pending - 1ull;
        const unsigned long long piece = called & ((1ull << to) - 1ull) & ~((1ull << from) - 1ull);
        from = to;
        if (static_cast<uint32_t>(__builtin_popcountll(piece)) < min_sites) continue;
        fold(piece);
        close();
      }
    }
    fold(called & ~((1ull << last_event) - 1ull));
  }
}

}  // namespace kgx

#endif  // KGX_KERNELS_RUNS_H
