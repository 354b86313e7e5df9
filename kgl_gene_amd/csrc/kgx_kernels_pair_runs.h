// Shared runs between genome pairs (driven from kgx_pair_runs.hip: kgx_pair_runs): for every unordered pair of genomes the unbroken
// stretches of listed rows in which the two do not mismatch, summarised like the runs of homozygosity.  It is k_roh's walk
// (kgx_kernels_runs.h) with "het" replaced by "mismatch between two genomes", over k_pair_counts' genome-major panel
// (kgx_kernels_panel.h): G^2 / 2 walkers instead of G, each reading two genomes' rows, so the words of a genome are prepared once
// and met by many partners out of LDS.
//
// k_pair_runs: a workgroup of 256 threads owns a pair (A <= B) of 32-genome tiles for the WHOLE list (one launch per row batch;
//   no row slicing, no atomics, no stitch).  Thread t walks genome t & 31 of A against the four genomes 4 (t >> 5) .. + 3 of B: four
//   run machines whose open run {first site's position, last site's list index, sites} and summary {runs, total, longest, sites}
//   stay in registers over the batch; the device table carries both from batch to batch (48 bytes a pair), so batching changes
//   nothing.  Per step the workgroup stages a chunk of kRunChunk 64-row tiles of its 64 genomes: thread t takes 32 bytes of the
//   panel (genome t >> 2, tiles 2 (t & 3) and + 1) and de-interleaves each tile's four dwords ONCE into lo (bit 0 of the codes), hi
//   (bit 1) and nc = lo & hi, 64 rows a word, [tile][word][genome] in LDS; position[] of the chunk's 512 rows goes into a strip
//   beside them.  Two buffers: the next chunk's bytes are in flight in registers while this one is walked; one barrier a chunk.
//   In the walk a thread reads its A genome's three words (consecutive lanes, consecutive words) and each B genome's by broadcast
//   (the 32 lanes of a half wave ask for the same word); the tile's break word is one uniform load.  Per pair and tile
//     nocall = nc_a | nc_b;  mism = ~(lo_a | lo_b) & (hi_a ^ hi_b)  (IBS0: codes {0, 2})  or  ((lo_a ^ lo_b) | (hi_a ^ hi_b)) & ~nocall;
//     events = mism | brk;  called = ~(mism | nocall) & valid
//   and the rest is roh_walk_word.  valid clears the positions past the list's end in its last tile, where the panel holds code 0
//   -- a shared site here; a genome the mask leaves out (code 0 in the panel as well) is kept out by the keep bytes: its pairs are
//   not walked and read zero.  A run's first position is kept as a value when the run opens; its last site's position is fetched
//   at the close, from the strip -- or from position[] itself where no-calls have carried the open run past its chunk.
//   On a diagonal tile pair the B side IS the A side, staged once, and only a <= b is walked and stored.
#pragma once

#include <cstdint>

#include "kgx_kernels_runs.h"

namespace kgx {

constexpr uint32_t kRunTile = 32;                                             // genomes of a tile side
constexpr uint32_t kRunChunk = 8;                                             // 64-row tiles staged per step
constexpr uint32_t kRunPerLane = 4;                                           // B genomes a thread walks its A genome against
// words of a tile in LDS: lo, hi, nc of 64 genomes, padded so that the four tiles a quarter wave stages fall into different banks
constexpr uint32_t kRunStride = 3 * 64 + 4;
static_assert(kBlock == 2 * kRunTile * 4 && kBlock / kRunTile * kRunPerLane == kRunTile && kRunChunk == 8, "k_pair_runs' thread maps");

// the even bits of x, packed into bits 0 .. 15
__device__ __forceinline__ uint32_t run_even_bits(uint32_t x) {
  x &= 0x55555555u;
  x = (x | (x >> 1)) & 0x33333333u;
  x = (x | (x >> 2)) & 0x0F0F0F0Fu;
  x = (x | (x >> 4)) & 0x00FF00FFu;
  return (x | (x >> 8)) & 0x0000FFFFu;
}

// One genome's 64 rows of the panel (dword u: rows 16 u .. 16 u + 15, two bits a row) as one bit plane: bit i = bit `plane` of row i.
__device__ __forceinline__ unsigned long long run_plane(kgx_v4u x, uint32_t plane) {
  const uint32_t low = run_even_bits(x[0] >> plane) | (run_even_bits(x[1] >> plane) << 16);
  const uint32_t high = run_even_bits(x[2] >> plane) | (run_even_bits(x[3] >> plane) << 16);
  return static_cast<unsigned long long>(low) | (static_cast<unsigned long long>(high) << 32);
}

// One walker: RohRun with `first` holding the POSITION of the first site (the run may outlive the chunk it opened in), and the
// summary of its reported runs.
struct PairRun {
  RohRun open;
  unsigned long long runs, total, longest, in_runs;
};

// panel: [32 n_tiles genomes or more][panel_pitch], the batch's n_steps = ceil(batch_rows / 64) tiles of 16 bytes; keep: one byte a
// genome, [32 n_tiles], or null; position / breaks: the WHOLE list's; first_row: the batch's first list position, a multiple of 64;
// summary: [G (G + 1) / 2][4]; open_runs: [G (G + 1) / 2] {first position, last list index, sites, 0}; blockIdx.x: the tile pair,
// row-major over A <= B.  first_batch: start from nothing; last_batch: the list's end closes the open runs.
template <bool IDENTICAL>
__global__ void __launch_bounds__(kBlock)
k_pair_runs(const uint8_t* __restrict__ panel, uint64_t panel_pitch, uint32_t n_tiles, uint64_t n_genomes, const uint8_t* __restrict__ keep,
            const uint32_t* __restrict__ position, const unsigned long long* __restrict__ breaks, uint32_t first_row, uint32_t batch_rows,
            uint32_t min_sites, uint32_t min_length, bool first_batch, bool last_batch, unsigned long long* __restrict__ summary,
            kgx_v4u* __restrict__ open_runs) {
  __shared__ unsigned long long words[2][kRunChunk][kRunStride];              // [buffer][tile][word x 64 + genome of A then B]
  __shared__ uint32_t strips[2][kRunChunk * 64];                              // [buffer][row of the chunk]: position[]
  uint32_t tile_a = 0, rest = blockIdx.x;
  while (rest >= n_tiles - tile_a) { rest -= n_tiles - tile_a; ++tile_a; }
  const uint32_t tile_b = tile_a + rest;
  const bool diagonal = tile_a == tile_b;
  const uint32_t t = threadIdx.x, n_steps = (batch_rows + 63u) / 64u;

  // ---- staging: genome of the 64, side, the two tiles of the chunk
  const uint32_t s_genome = t >> 2, s_side = s_genome >> 5, s_tile = 2u * (t & 3u);
  const bool stages = !(diagonal && s_side == 1u);
  const uint8_t* src = panel + (static_cast<uint64_t>(s_side ? tile_b : tile_a) * kRunTile + (s_genome & 31u)) * panel_pitch;
  kgx_v4u in[2];
  uint32_t pos_in[2];
  auto fetch = [&](uint32_t c0) {                                             // the chunk that starts at tile c0 of the batch
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
      const uint32_t tile = c0 + s_tile + k, row = c0 * 64u + t + kBlock * k;
      in[k] = kgx_v4u{0u, 0u, 0u, 0u};
      if (stages && tile < n_steps) in[k] = *reinterpret_cast<const kgx_v4u*>(src + 16ull * tile);
      pos_in[k] = row < batch_rows ? position[static_cast<uint64_t>(first_row) + row] : 0u;
    }
  };
  auto stage = [&](uint32_t buffer) {
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
      if (stages) {
        const unsigned long long lo = run_plane(in[k], 0u), hi = run_plane(in[k], 1u);
        unsigned long long* w = &words[buffer][s_tile + k][s_genome];
        w[0] = lo;
        w[64] = hi;
        w[128] = lo & hi;
      }
      strips[buffer][t + kBlock * k] = pos_in[k];
    }
  };
  fetch(0u);
  stage(0u);

  // ---- the thread's four walkers
  const uint32_t a_local = t & 31u, b_local = (t >> 5) * kRunPerLane, b_side = diagonal ? 0u : 32u;
  const uint64_t ga = static_cast<uint64_t>(tile_a) * kRunTile + a_local, gb0 = static_cast<uint64_t>(tile_b) * kRunTile + b_local;
  PairRun st[kRunPerLane];
  bool stored[kRunPerLane], walked[kRunPerLane];                              // a pair of the table; ... both of whose genomes take part
  uint64_t at[kRunPerLane];
#pragma unroll
  for (uint32_t j = 0; j < kRunPerLane; ++j) {
    const uint64_t gb = gb0 + j;
    st[j] = PairRun{{0u, 0u, 0u}, 0ull, 0ull, 0ull, 0ull};
    stored[j] = ga < n_genomes && gb < n_genomes && ga <= gb;
    walked[j] = stored[j] && (keep == nullptr || (keep[ga] != 0 && keep[gb] != 0));
    at[j] = stored[j] ? ga * n_genomes - ga * (ga - 1u) / 2u + (gb - ga) : 0u;
    if (walked[j] && !first_batch) {
      const kgx_v4u o = open_runs[at[j]];
      st[j].open = RohRun{o.x, o.y, o.z};
      st[j].runs = summary[4u * at[j]];
      st[j].total = summary[4u * at[j] + 1u];
      st[j].longest = summary[4u * at[j] + 2u];
      st[j].in_runs = summary[4u * at[j] + 3u];
    }
  }
  __syncthreads();

  const uint32_t* strip = strips[0];
  uint32_t chunk_r0 = first_row;                                              // the list position of strip[0]
  auto close = [&](PairRun& p) {
    if (p.open.sites == 0) return;
    if (p.open.sites >= min_sites) {                                          // positions are read only for a run that has the sites
      const unsigned long long last = p.open.last >= chunk_r0 ? strip[p.open.last - chunk_r0] : position[p.open.last];
      const unsigned long long length = last - p.open.first + 1ull;
      if (roh_reported(p.open.sites, length, min_sites, min_length)) {
        ++p.runs;
        p.total += length;
        p.longest = length > p.longest ? length : p.longest;
        p.in_runs += p.open.sites;
      }
    }
    p.open.sites = 0;
  };

  for (uint32_t c0 = 0; c0 < n_steps; c0 += kRunChunk) {
    const uint32_t buffer = (c0 / kRunChunk) & 1u;
    const bool more = c0 + kRunChunk < n_steps;
    if (more) fetch(c0 + kRunChunk);
    strip = strips[buffer];
    chunk_r0 = first_row + c0 * 64u;
    const uint32_t tiles = n_steps - c0 < kRunChunk ? n_steps - c0 : kRunChunk;
    for (uint32_t s = 0; s < tiles; ++s) {
      const uint32_t r0 = chunk_r0 + 64u * s, left = batch_rows - (c0 + s) * 64u;
      const unsigned long long valid = left >= 64u ? ~0ull : (1ull << left) - 1ull;
      const unsigned long long brk = breaks[r0 >> 6] & valid;
      const unsigned long long* w = words[buffer][s];
      const unsigned long long lo_a = w[a_local], hi_a = w[64u + a_local], nc_a = w[128u + a_local];
#pragma unroll
      for (uint32_t j = 0; j < kRunPerLane; ++j) {
        if (!walked[j]) continue;
        const uint32_t b = b_side + b_local + j;
        const unsigned long long lo_b = w[b], hi_b = w[64u + b], nc_b = w[128u + b];
        const unsigned long long nocall = nc_a | nc_b;
        const unsigned long long mism = (IDENTICAL ? ((lo_a ^ lo_b) | (hi_a ^ hi_b)) & ~nocall : ~(lo_a | lo_b) & (hi_a ^ hi_b)) & valid;
        const unsigned long long called = ~(mism | nocall) & valid;
        RohRun& open = st[j].open;
        auto fold = [&](unsigned long long piece) {           // the piece's shared sites join the open run, or open one
          if (piece == 0) return;
          if (open.sites == 0) open.first = strip[64u * s + static_cast<uint32_t>(__builtin_ctzll(piece))];
          open.last = r0 + 63u - static_cast<uint32_t>(__builtin_clzll(piece));
          open.sites += static_cast<uint32_t>(__builtin_popcountll(piece));
        };
        roh_walk_word(mism | brk, called, min_sites, fold, [&]() { close(st[j]); });
      }
    }
    if (more) stage(buffer ^ 1u);
    __syncthreads();                                                          // the other buffer is staged; this one is free
  }

#pragma unroll
  for (uint32_t j = 0; j < kRunPerLane; ++j) {
    if (!stored[j]) continue;
    if (last_batch) close(st[j]);                                             // the list's end (the strip still holds the last chunk)
    summary[4u * at[j]] = st[j].runs;
    summary[4u * at[j] + 1u] = st[j].total;
    summary[4u * at[j] + 2u] = st[j].longest;
    summary[4u * at[j] + 3u] = st[j].in_runs;
    open_runs[at[j]] = kgx_v4u{st[j].open.first, st[j].open.last, st[j].open.sites, 0u};
  }
}

}  // namespace kgx
