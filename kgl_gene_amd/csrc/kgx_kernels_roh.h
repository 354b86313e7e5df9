// Runs of homozygosity per genome (kgx_roh, include/kgx.h): the one reduction of the 2-bit matrix that walks a genome ALONG the
// listed rows IN ORDER and carries state -- an open run {first, last, sites} that a het or a break closes, a called homozygous site
// extends and a no-call leaves alone.  The access shape is the row lists' (k_genome_row_lists): a wave owns four adjacent chunk
// columns (one 64-byte line of a row, 256 genomes) and a slice of whole 64-position tiles; lane i loads the line of list position
// r0 + i, two bit planes per chunk (het, no-call) are turned around by one six-stage butterfly, and lane j then holds its genome's
// 64 positions of both planes.  What is new is what happens to those words: a run machine per lane, its state carried in registers
// from tile to tile, and a fixed-size record per (slice, genome) -- head piece, tail piece, sums of the runs in between -- that
// k_roh_stitch folds over the slices in order, one thread per genome.  Integers throughout: the same bits whatever the slicing.
#ifndef KGX_KERNELS_ROH_H
#define KGX_KERNELS_ROH_H

#include "kgx_kernels_runs.h"

namespace kgx {

constexpr int kRohChunks = 4;              // chunk columns per wave: one 64-byte line of a row
constexpr int kRohPlanes = 4;              // 16-byte planes of a slice record, [plane][slice][genome]:
//   0: head {first, last, sites} (sites == 0: none) and flags: bit 0 = an event (het, break, the list's end) fell into the slice
//   1: tail {first, last, sites} -- the run open at the slice's end (only with an event; without one the whole slice is the head)
//      and the number of reported interior runs
//   2: the interior runs' total length and longest length (64 bits each)
//   3: the interior runs' sites (64 bits)
// Interior: opened after the slice's first event and closed inside the slice.
constexpr uint64_t kRohBytesPerCell = kRohPlanes * 16 + 4 + 8;   // ... plus the (slice, genome) count and cursor

// The chunk's 2-bit codes as two rows of 64 bits: w[0], w[1] = het (code 1), low and high dword; w[2], w[3] = no-call (code 3).
// The shift / mask ladder of carried_bits, once per plane.
__device__ __forceinline__ void roh_planes(kgx_v4u x, uint32_t (&w)[4]) {
  uint32_t het[4], nocall[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const uint32_t lo = x[d] & 0x55555555u, hi = (x[d] >> 1) & 0x55555555u;
    uint32_t h = lo & ~hi, n = lo & hi;                     // bit 2j: genome 16 d + j
    h = (h | (h >> 1)) & 0x33333333u;
    n = (n | (n >> 1)) & 0x33333333u;
    h = (h | (h >> 2)) & 0x0F0F0F0Fu;
    n = (n | (n >> 2)) & 0x0F0F0F0Fu;
    h = (h | (h >> 4)) & 0x00FF00FFu;
    n = (n | (n >> 4)) & 0x00FF00FFu;
    het[d] = (h | (h >> 8)) & 0x0000FFFFu;
    nocall[d] = (n | (n >> 8)) & 0x0000FFFFu;
  }
  w[0] = het[0] | (het[1] << 16);
  w[1] = het[2] | (het[3] << 16);
  w[2] = nocall[0] | (nocall[1] << 16);
  w[3] = nocall[2] | (nocall[3] << 16);
}

// (a & mask) | (b & ~mask): one v_bfi_b32.
__device__ __forceinline__ uint32_t roh_pick(uint32_t mask, uint32_t a, uint32_t b) { return (a & mask) | (b & ~mask); }

// All ones in the lanes whose number has bit S set (the upper lane of every pair i, i ^ S), zero in the others.
template <int S>
__device__ __forceinline__ uint32_t roh_upper(uint32_t lane) { return 0u - ((lane / S) & 1u); }

// One exchange stage of the butterfly at block size S < 32, without a branch or a select: every lane shifts what its partner takes
// into place before it sends -- the upper lane its low columns up, the lower lane its high columns down, by shift counts that are S
// or 0 by the lane -- and keeps its own half under `keep`.  The shift counts and masks are worked out once for the four dwords.
template <int S, uint32_t LOW>
__device__ __forceinline__ void roh_stage(uint32_t (&w)[4], uint32_t lane) {
  const uint32_t upper = roh_upper<S>(lane), up = S & upper, down = S & ~upper, keep = LOW ^ upper;
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = roh_pick(keep, w[i], __shfl_xor((w[i] << up) >> down, S));
}

// Both planes' 64 x 64 tiles turned around across the wave (transpose_tile's butterfly, kgx_kernels_dosage.h): lane i comes in with
// list position i (bit j = genome j) and leaves with genome i (bit j = position j).  At block size 32 whole dwords change hands: a
// lane sends only the dword its partner takes.
__device__ __forceinline__ void roh_transpose(uint32_t (&w)[4], uint32_t lane) {
  {
    const uint32_t upper = roh_upper<32>(lane);
    const uint32_t het = __shfl_xor(roh_pick(upper, w[0], w[1]), 32), nocall = __shfl_xor(roh_pick(upper, w[2], w[3]), 32);
    w[0] = roh_pick(upper, het, w[0]);
    w[1] = roh_pick(upper, w[1], het);
    w[2] = roh_pick(upper, nocall, w[2]);
    w[3] = roh_pick(upper, w[3], nocall);
  }
  roh_stage<16, 0x0000FFFFu>(w, lane);
  roh_stage<8, 0x00FF00FFu>(w, lane);
  roh_stage<4, 0x0F0F0F0Fu>(w, lane);
  roh_stage<2, 0x33333333u>(w, lane);
  roh_stage<1, 0x55555555u>(w, lane);
}

// A lane's state for one chunk column: the open run, carried from tile to tile, and what the slice's record is made of.
struct RohLane {
  RohRun open, head;                       // head: the run the slice's first event closed
  bool seen;                               // an event so far in the slice
  uint32_t runs;                           // reported interior runs ...
  unsigned long long total, longest, in_runs;   // ... their lengths' sum and maximum, their sites
  unsigned long long cursor;               // FILL: where the next interior run goes
};

// An event: the open run, if any, closes.  Closed by the slice's first event it is the head, which the stitch owns; later it is
// an interior run, tested and counted (or written) here.  strip: position[r0 ..] of the current tile.
template <bool FILL>
__device__ __forceinline__ void roh_close(RohLane& st, const uint32_t* strip, uint64_t r0, const uint32_t* __restrict__ position, uint32_t min_sites,
                                          uint32_t min_length, uint32_t* __restrict__ segments) {
  if (st.open.sites != 0) {
    if (!st.seen) {
      st.head = st.open;
    } else {
      unsigned long long length = 0;
      if (st.open.sites >= min_sites) {                       // positions are read only for a run that has the sites
        const unsigned long long first = st.open.first >= r0 ? strip[st.open.first - r0] : position[st.open.first];
        const unsigned long long last = st.open.last >= r0 ? strip[st.open.last - r0] : position[st.open.last];
        length = last - first + 1ull;
      }
      if (roh_reported(st.open.sites, length, min_sites, min_length)) {
        if constexpr (FILL) {
          segments[3 * st.cursor] = st.open.first;
          segments[3 * st.cursor + 1] = st.open.last;
          segments[3 * st.cursor + 2] = st.open.sites;
          ++st.cursor;
        } else {
          ++st.runs;
          st.total += length;
          st.longest = length > st.longest ? length : st.longest;
          st.in_runs += st.open.sites;
        }
      }
    }
    st.open.sites = 0;
  }
  st.seen = true;
}

// ---------------------------------------------------------------------------------------------
// The walk.  grid (column waves / 4, slices); FILL = false leaves the records, FILL = true walks the same way and writes the
// reported interior runs' {first, last, sites} from cursors[slice][genome] on (k_roh_stitch<true> put the cursor behind the one
// stitched run that may close in the slice).
// Events of a tile: events = het | brk (brk: the tile's break word, one uniform load).  A het is never a called site and a break
// before position b leaves b's own cell to the piece that follows, so both are handled alike, by roh_walk_word
// (kgx_kernels_runs.h, shared with the walk over genome pairs).
// The list's end closes the open run in the last slice, as one more event.
// Positions: lane i parks position[r0 + i] in the wave's own 256-byte strip of LDS, because the lanes ask for positions by a
// divergent bit number from a divergent loop.  One wave writes and reads its strip, LDS serves a wave's accesses in order, so a
// wave-scope fence is all the ordering there is -- no workgroup barrier (the waves of a workgroup walk different columns and may
// have left already).  A run's ends that lie before the tile are read from global memory.
// ---------------------------------------------------------------------------------------------
template <bool FILL>
__global__ void __launch_bounds__(kBlock)
k_roh(const kgx_v4u* __restrict__ rows, uint32_t chunks_per_row, uint64_t n_genomes, const kgx_v4u* __restrict__ keep /* the genome mask's row, or null */,
      const uint32_t* __restrict__ row_list /* or null: list position = row */, uint64_t n_rows, const uint32_t* __restrict__ position,
      const unsigned long long* __restrict__ breaks, uint64_t rows_per_slice, uint32_t min_sites, uint32_t min_length,
      kgx_v4u* __restrict__ records /* [kRohPlanes][slices][genomes padded to 256] */, uint64_t genomes_padded,
      const unsigned long long* __restrict__ cursors /* [slices][genomes padded] */, uint32_t* __restrict__ segments /* [..][3] */) {
  __shared__ uint32_t strips[kBlock];
  const uint32_t lane = threadIdx.x & (kWave - 1);
  uint32_t* strip = strips + (threadIdx.x - lane);
  const uint32_t c0 = (blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave) * kRohChunks;
  if (c0 >= chunks_per_row) return;
  const uint64_t slice = blockIdx.y, n_slices = gridDim.y;
  const uint64_t r_begin = slice * rows_per_slice;
  const uint64_t r_end = r_begin + rows_per_slice < n_rows ? r_begin + rows_per_slice : n_rows;

  RohLane st[kRohChunks];
  bool listed[kRohChunks];                                   // the lane's genome of chunk k takes part
#pragma unroll
  for (int k = 0; k < kRohChunks; ++k) {
    st[k] = RohLane{{0u, 0u, 0u}, {0u, 0u, 0u}, false, 0u, 0ull, 0ull, 0ull, 0ull};
    const uint64_t genome = (static_cast<uint64_t>(c0) + k) * 64u + lane;
    listed[k] = genome < n_genomes;
    if (keep != nullptr && c0 + k < chunks_per_row) {
      const kgx_v4u m = keep[c0 + k];
      listed[k] = listed[k] && ((m[lane >> 4] >> (2 * (lane & 15))) & 1u);
    }
    if constexpr (FILL) st[k].cursor = cursors[slice * genomes_padded + genome];
  }

  for (uint64_t r0 = r_begin; r0 < r_end; r0 += kWave) {
    const uint64_t p = r0 + lane;
    const bool live = p < r_end;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the last tile's reads of the strip come before these writes ...
    if (live) strip[lane] = position[p];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // ... and these writes before this tile's reads
    const uint64_t row = live ? (row_list != nullptr ? row_list[p] : p) : 0;
    kgx_v4u x[kRohChunks];
#pragma unroll
    for (int k = 0; k < kRohChunks; ++k) {
      x[k] = kgx_v4u{0u, 0u, 0u, 0u};
      if (live && c0 + k < chunks_per_row) x[k] = rows[row * chunks_per_row + c0 + k];
    }
    const uint64_t left = r_end - r0;
    const unsigned long long in_tile = left >= kWave ? ~0ull : (1ull << left) - 1ull;
    const unsigned long long brk = breaks[r0 >> 6] & in_tile;                 // slices are whole tiles: r0 is a multiple of 64
#pragma unroll
    for (int k = 0; k < kRohChunks; ++k) {
      uint32_t w[4];
      roh_planes(x[k], w);
      roh_transpose(w, lane);
      const unsigned long long het = (static_cast<unsigned long long>(w[0]) | (static_cast<unsigned long long>(w[1]) << 32)) & in_tile;
      const unsigned long long nocall = static_cast<unsigned long long>(w[2]) | (static_cast<unsigned long long>(w[3]) << 32);
      const unsigned long long events = (listed[k] ? het : 0ull) | brk;
      unsigned long long called = listed[k] ? ~(het | nocall) & in_tile : 0ull;
      RohRun& open = st[k].open;
      auto fold = [&](unsigned long long piece) {             // the piece's called sites join the open run, or open one
        if (piece == 0) return;
        if (open.sites == 0) open.first = static_cast<uint32_t>(r0) + static_cast<uint32_t>(__builtin_ctzll(piece));
        open.last = static_cast<uint32_t>(r0) + 63u - static_cast<uint32_t>(__builtin_clzll(piece));
        open.sites += static_cast<uint32_t>(__builtin_popcountll(piece));
      };
      roh_walk_word(events, called, min_sites, fold, [&]() { roh_close<FILL>(st[k], strip, r0, position, min_sites, min_length, segments); });
    }
  }

  const uint64_t last_r0 = (r_end - 1) & ~static_cast<uint64_t>(kWave - 1);     // the strip still holds the last tile
#pragma unroll
  for (int k = 0; k < kRohChunks; ++k) {
    // the list's end is the last slice's last event
    if (r_end == n_rows) roh_close<FILL>(st[k], strip, last_r0, position, min_sites, min_length, segments);
    if constexpr (!FILL) {
      const uint64_t at = slice * genomes_padded + (static_cast<uint64_t>(c0) + k) * 64u + lane;
      const uint64_t plane = n_slices * genomes_padded;
      const RohLane& l = st[k];
      const RohRun first_piece = l.seen ? l.head : l.open;
      const RohRun last_piece = l.seen ? l.open : RohRun{0u, 0u, 0u};
      records[at] = kgx_v4u{first_piece.first, first_piece.last, first_piece.sites, l.seen ? 1u : 0u};
      records[plane + at] = kgx_v4u{last_piece.first, last_piece.last, last_piece.sites, l.runs};
      records[2 * plane + at] = kgx_v4u{static_cast<uint32_t>(l.total), static_cast<uint32_t>(l.total >> 32), static_cast<uint32_t>(l.longest),
                                        static_cast<uint32_t>(l.longest >> 32)};
      records[3 * plane + at] = kgx_v4u{static_cast<uint32_t>(l.in_runs), static_cast<uint32_t>(l.in_runs >> 32), 0u, 0u};
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The stitch: one thread per genome folds its slice records in order.  carry = the run open at the previous slice's end; it is
// folded with the slice's head; where the slice has an event the folded run closes there -- the slice that owns it -- and the
// carry becomes the slice's tail.  The last slice always has an event (the list's end), so nothing is open afterwards.
//   FILL = false: counts[slice][genome] = the slice's reported runs (its interior ones plus the stitched one), summary[genome]
//                 and totals[genome] (the genome's runs: what k_roh_scan turns into begin[]).
//   FILL = true : the stitched runs' triples at their cursors, and cursors[slice][genome] for k_roh<true>: where the slice's
//                 interior runs start.
// ---------------------------------------------------------------------------------------------
template <bool FILL>
__global__ void __launch_bounds__(kBlock)
k_roh_stitch(const kgx_v4u* __restrict__ records, uint64_t n_slices, uint64_t genomes_padded, uint64_t n_genomes, const uint32_t* __restrict__ position,
             uint32_t min_sites, uint32_t min_length, uint32_t* __restrict__ counts /* [slices][genomes padded] */,
             unsigned long long* __restrict__ summary /* [n_genomes][4] */, unsigned long long* __restrict__ totals,
             const unsigned long long* __restrict__ begin, unsigned long long* __restrict__ cursors, uint32_t* __restrict__ segments) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= n_genomes) return;
  const uint64_t plane = n_slices * genomes_padded;
  RohRun carry{0u, 0u, 0u};
  unsigned long long n_runs = 0, total = 0, longest = 0, in_runs = 0, at = 0;
  if constexpr (FILL) at = begin[g];
  for (uint64_t s = 0; s < n_slices; ++s) {
    const uint64_t cell = s * genomes_padded + g;
    const kgx_v4u first_piece = records[cell], last_piece = records[plane + cell];
    if (first_piece.z != 0) {
      if (carry.sites == 0) carry.first = first_piece.x;
      carry.last = first_piece.y;
      carry.sites += first_piece.z;
    }
    uint32_t stitched = 0;
    if (first_piece.w & 1u) {
      if (carry.sites != 0) {
        const unsigned long long length = static_cast<unsigned long long>(position[carry.last]) - position[carry.first] + 1ull;
        if (roh_reported(carry.sites, length, min_sites, min_length)) {
          stitched = 1;
          if constexpr (FILL) {
            segments[3 * at] = carry.first;
            segments[3 * at + 1] = carry.last;
            segments[3 * at + 2] = carry.sites;
          } else {
            total += length;
            longest = length > longest ? length : longest;
            in_runs += carry.sites;
          }
        }
      }
      carry = RohRun{last_piece.x, last_piece.y, last_piece.z};
    }
    if constexpr (FILL) {
      cursors[cell] = at + stitched;
      at += counts[cell];
    } else {
      const kgx_v4u lengths = records[2 * plane + cell], sites = records[3 * plane + cell];
      const unsigned long long slice_longest = static_cast<unsigned long long>(lengths.z) | (static_cast<unsigned long long>(lengths.w) << 32);
      counts[cell] = last_piece.w + stitched;
      n_runs += last_piece.w + stitched;
      total += static_cast<unsigned long long>(lengths.x) | (static_cast<unsigned long long>(lengths.y) << 32);
      longest = slice_longest > longest ? slice_longest : longest;
      in_runs += static_cast<unsigned long long>(sites.x) | (static_cast<unsigned long long>(sites.y) << 32);
    }
  }
  if constexpr (!FILL) {
    summary[4 * g] = n_runs;
    summary[4 * g + 1] = total;
    summary[4 * g + 2] = longest;
    summary[4 * g + 3] = in_runs;
    totals[g] = n_runs;
  }
}

// Exclusive scan of the genomes' run counts into begin[] (one workgroup; the grand total lands in begin[n_genomes]): the shape of
// k_row_list_scan.
__global__ void __launch_bounds__(kBlock)
k_roh_scan(const unsigned long long* __restrict__ totals, uint64_t n_genomes, unsigned long long* __restrict__ begin) {
  __shared__ unsigned long long piece[kBlock];
  __shared__ unsigned long long carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint64_t base = 0; base < n_genomes; base += kBlock) {
    const uint64_t g = base + threadIdx.x;
    const unsigned long long mine = g < n_genomes ? totals[g] : 0ull;
    piece[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {              // inclusive scan of the piece (Hillis-Steele)
      const unsigned long long v = threadIdx.x >= static_cast<uint32_t>(off) ? piece[threadIdx.x - off] : 0ull;
      __syncthreads();
      piece[threadIdx.x] += v;
      __syncthreads();
    }
    if (g < n_genomes) begin[g] = carry + piece[threadIdx.x] - mine;
    __syncthreads();
    if (threadIdx.x == kBlock - 1) carry += piece[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) begin[n_genomes] = carry;
}

}  // namespace kgx

#endif  // KGX_KERNELS_ROH_H
