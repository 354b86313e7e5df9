// Windowed joint genotype counts between the listed ROWS of a 2-bit population (driven from kgx_ld.hip: kgx_ld_counts).
//
// With I_p[r][g] the 0 / 1 indicator "listed row r has kind p in genome g" (kinds H = code 1, M = code 2, O = code 3),
//     n[p][q](i, j) = sum over g of  I_p[i][g] * I_q[j][g]
// is the mirror of kgx_kernels_pairs.h: it contracts over GENOMES, which the variant-major matrix keeps together.  A 16-byte chunk
// of a row is 64 genomes = one K step of v_mfma_i32_16x16x64_i8 and dword u of the chunk is the 16 codes lane (c, u) of an operand
// needs, so there is no panel and no transposition: one kernel, straight from the shard's rows.
//
// k_ld_counts: a workgroup of 256 threads owns a pair (I, J = I + blockIdx.x % (band + 1)) of 64-row blocks of the list and walks
//   the segments (8 chunks = 512 genomes = 128 bytes a row) of its slice of the shard's genomes.
//   Staging: thread t fetches chunk t & 7 of the segment for the rows (t >> 3) + 32 k of the pair's 128 (A block, then B block):
//   8 lanes per row, 16 bytes a lane -- whole 128-byte lines where the pitch is a multiple of 128.  The row comes from the list;
//   positions past the list's end and chunks >= chunks_per_row are not read and are code 0.  The NEXT segment waits in REGISTERS
//   (16 VGPRs of rows + 4 of the mask's chunk) while this segment's steps run: a second raw buffer would cost 16 KiB of LDS and put
//   two workgroups at the 160 KiB a compute unit has, and it would not save the registers -- a global load lands in them first
//   either way.  Before the step that needs it the segment goes to LDS (raw[row][chunk ^ (row & 7)], so that the 8-byte reads of
//   one chunk of 8 adjacent rows spread over all banks) with the genome mask's chunk ANDed in and the codes past the shard's
//   genomes cleared (the rule of k_pair_panel).
//   Operands: per 64-genome step all threads build the step's 24 operands ONCE, thread t = (side t >> 7, row (t & 127) >> 1, half
//   t & 1) from 8 bytes of raw: pair_indicators per dword, written in the operand layout of kgx_kernels_hall.h / _census.h / _pairs.h
//   -- operand (16 rows, kind), lane (c, u) = row c, k = genomes 16 u .. 16 u + 15.  Two operand buffers: the next step's are
//   built while this step's products issue; one barrier a step, and one more where a segment ends (raw is rewritten, then read).
//   Products: wave w multiplies A rows 16 w .. 16 w + 15 x three kinds with the four B sub-tiles x three kinds: 36 accumulator
//   tiles, 15 ds_read_b128 and 36 products a step.  On J == I the B side IS the A side, staged once.
//   C: lane (c, u) holds B row c, A rows 4 u + reg -- all nine words of a row pair sit in one lane.  Stored where
//   0 <= j - i <= window and j < n_rows, at out[(i - batch_first) (window + 1) + (j - i)]: for one A row the 16 lanes c write one
//   contiguous run.  mode: 0 = store (the first shard of the device), 1 = add to what the earlier shards stored (the same owner,
//   no atomics), 2 = atomicAdd into a zeroed table (segments split over gridDim.z when there are few block pairs: integer sums,
//   exact in any order).  Entries past the list's end are nobody's: the driver zeroes them.
#pragma once

#include <cstdint>

#include "kgx_kernels_indicators.h"

namespace kgx {

constexpr uint32_t kLdBlock = 64;                                             // listed rows of a block
constexpr uint32_t kLdSegment = 8;                                            // chunks of a segment: 128 bytes of a row
constexpr uint32_t kLdNoRow = 0xFFFFFFFFu;

// rows: the shard's rows (chunks_per_row 16-byte chunks each, n_genomes genomes); keep: the genome mask's row or null; row_list:
// the WHOLE list on the device (null: position = row); first_block: the batch's first 64-row block of the list; gridDim.x =
// batch blocks x (band + 1); out: the batch's table [64 batch blocks][window + 1][9].
__global__ void __launch_bounds__(kBlock, 2)
k_ld_counts(const kgx_v4u* __restrict__ rows, uint32_t chunks_per_row, uint64_t n_genomes, const kgx_v4u* __restrict__ keep,
            const uint32_t* __restrict__ row_list, uint64_t n_rows, uint32_t window, uint32_t band, uint64_t first_block,
            uint32_t segments_per_slice, int mode, uint32_t* __restrict__ out) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  __shared__ kgx_v4u operands[2][2][kPairOperands][kWave];                    // [buffer][side][16-row tile x kind][lane]: 48 KiB
  __shared__ kgx_v4u raw[2 * kLdBlock][kLdSegment];                           // [side x row][chunk ^ (row & 7)]: 16 KiB
  const uint64_t block_a = first_block + blockIdx.x / (band + 1u), block_b = block_a + blockIdx.x % (band + 1u);
  if (block_b * kLdBlock >= n_rows) return;                                   // (the whole workgroup) the band is clipped to the list
  const bool diagonal = block_a == block_b;
  const uint32_t n_chunks = static_cast<uint32_t>((n_genomes + 63u) / 64u);   // <= chunks_per_row
  const uint32_t n_segments = (n_chunks + kLdSegment - 1u) / kLdSegment;
  const uint32_t seg_begin = blockIdx.z * segments_per_slice;
  const uint32_t seg_end = seg_begin + segments_per_slice < n_segments ? seg_begin + segments_per_slice : n_segments;
  if (seg_begin >= seg_end) return;                                           // (the whole workgroup)
  const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, c = lane & 15u, u = lane >> 4;

  // ---- fetching: chunk `piece` of the segment for the rows fetch_row + 32 k of the pair's 128
  const uint32_t piece = threadIdx.x & 7u, fetch_row = threadIdx.x >> 3;
  const int fetched = diagonal ? 2 : 4;                                       // k < 2: the A block, k >= 2: the B block
  uint32_t row_of[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint64_t at = (k < 2 ? block_a : block_b) * kLdBlock + ((fetch_row + 32u * k) & 63u);
    row_of[k] = at < n_rows && k < fetched ? (row_list ? row_list[at] : static_cast<uint32_t>(at)) : kLdNoRow;
  }
  kgx_v4u next[4], next_keep;
  auto fetch = [&](uint32_t segment) {
    const uint32_t chunk = segment * kLdSegment + piece;
    const bool inside = chunk < chunks_per_row;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      next[k] = kgx_v4u{0u, 0u, 0u, 0u};
      if (inside && row_of[k] != kLdNoRow) next[k] = rows[static_cast<uint64_t>(row_of[k]) * chunks_per_row + chunk];
    }
    next_keep = kgx_v4u{~0u, ~0u, ~0u, ~0u};
    if (inside && keep != nullptr) next_keep = keep[chunk];
  };
  auto land = [&](uint32_t segment) {                                         // registers -> raw, masked
    kgx_v4u mask = next_keep;
    const uint64_t g0 = (static_cast<uint64_t>(segment) * kLdSegment + piece) * 64u;
#pragma unroll
    for (int d = 0; d < 4; ++d) {                                             // the codes past the shard's genomes are nobody's
      const uint64_t g = g0 + 16u * d;
      const uint32_t valid = n_genomes >= g + 16u ? 16u : (n_genomes > g ? static_cast<uint32_t>(n_genomes - g) : 0u);
      if (valid < 16u) mask[d] &= (1u << (2u * valid)) - 1u;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < fetched) raw[fetch_row + 32u * k][piece ^ (fetch_row & 7u)] = next[k] & mask;
  };

  // ---- building: side, row of the side's block, which half of the step's 64 genomes
  const uint32_t side = threadIdx.x >> 7, row = (threadIdx.x & 127u) >> 1, half = threadIdx.x & 1u;
  const bool builds = !(diagonal && side == 1u);
  auto build = [&](uint32_t buffer, uint32_t step) {
    if (!builds) return;
    const uint2 codes = reinterpret_cast<const uint2*>(&raw[side * kLdBlock + row][step ^ (row & 7u)])[half];
    kgx_v4u* dst = &operands[buffer][side][(row >> 4) * kPairKinds][(row & 15u) + 32u * half];
    kgx_v4u h, m, o;
    pair_indicators(codes.x, h, m, o);
    dst[0] = h; dst[kWave] = m; dst[2 * kWave] = o;
    pair_indicators(codes.y, h, m, o);
    dst[16] = h; dst[kWave + 16] = m; dst[2 * kWave + 16] = o;
  };

  fetch(seg_begin);
  land(seg_begin);
  __syncthreads();
  build(0u, 0u);
  __syncthreads();

  v4i acc[kPairKinds][4][kPairKinds];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int q = 0; q < 3; ++q) acc[p][t][q] = v4i{0, 0, 0, 0};
  const uint32_t b_side = diagonal ? 0u : 1u;
  uint32_t buffer = 0;
  for (uint32_t segment = seg_begin; segment < seg_end; ++segment) {
    const uint32_t left = n_chunks - segment * kLdSegment, steps = left < kLdSegment ? left : kLdSegment;
    const bool more = segment + 1 < seg_end;
    if (more) fetch(segment + 1);                                             // in flight over this segment's steps
    for (uint32_t step = 0; step < steps; ++step, buffer ^= 1u) {
      v4i a[kPairKinds];
#pragma unroll
      for (int p = 0; p < 3; ++p) a[p] = __builtin_bit_cast(v4i, operands[buffer][0][wave * kPairKinds + p][lane]);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const v4i b = __builtin_bit_cast(v4i, operands[buffer][b_side][t * kPairKinds + q][lane]);
#pragma unroll
          for (int p = 0; p < 3; ++p) acc[p][t][q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[p], b, acc[p][t][q], 0, 0, 0);
        }
      if (step + 1 < steps) build(buffer ^ 1u, step + 1);
      __syncthreads();                                                        // the other buffer is built; this one is free
    }
    if (more) {                                                               // every build from raw lies before the last barrier
      land(segment + 1);
      __syncthreads();
      build(buffer, 0u);
      __syncthreads();
    }
  }

  // lane (c, u): B row c of each B sub-tile, A rows 4 u + reg of the wave's sub-tile
  const uint64_t batch_first = first_block * kLdBlock;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const uint64_t i = block_a * kLdBlock + 16u * wave + 4u * u + reg;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint64_t j = block_b * kLdBlock + 16u * t + c;
      if (j >= n_rows || j < i || j - i > window) continue;                   // (i <= j < n_rows)
      uint32_t* words = out + ((i - batch_first) * (static_cast<uint64_t>(window) + 1u) + (j - i)) * kPairWords;
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const uint32_t v = static_cast<uint32_t>(acc[p][t][q][reg]);
          if (mode == 0) words[3 * p + q] = v;
          else if (mode == 1) words[3 * p + q] += v;
          else if (v) atomicAdd(&words[3 * p + q], v);
        }
    }
  }
}

// table += other (a table another device filled, copied over)
__global__ void __launch_bounds__(kBlock)
k_ld_add(uint32_t* __restrict__ table, const uint32_t* __restrict__ other, uint64_t n_words) {
  for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; w < n_words; w += static_cast<uint64_t>(gridDim.x) * kBlock) table[w] += other[w];
}

// table[0 .. n_words) = 0
__global__ void __launch_bounds__(kBlock)
k_ld_clear(uint32_t* __restrict__ table, uint64_t n_words) {
  for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; w < n_words; w += static_cast<uint64_t>(gridDim.x) * kBlock) table[w] = 0u;
}

}  // namespace kgx
