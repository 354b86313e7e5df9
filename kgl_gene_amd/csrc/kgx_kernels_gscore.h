// Per-genome class sums of per-row weights of a 2-bit population (driven from kgx_gscore.hip: kgx_genome_scores).
//
// With I_k[i][g] the 0 / 1 indicator "list position i has kind k in genome g" (kinds H = code 1, M = code 2, O = code 3) and
// w[j][i] the caller's weight of column j at list position i (|w| <= KGX_SCORE_MAX),
//     S[k](g, j) = sum over i of  I_k[i][g] * w[j][i]
// is the transpose of kgx_kernels_assoc.h: it contracts over ROWS, the direction the rows are NOT packed in.  A lane of the A
// operand of v_mfma_i32_16x16x64_i8 needs 16 consecutive rows of one genome, a loaded dword holds 16 genomes of one row: the codes
// are transposed in registers on the way (gscore_transpose), no panel and no LDS for the genotypes.
//
// Digits.  Columns are taken in groups of 16, one group a pass (blockIdx.y).  A group has D = 1 or 2 signed base-128 digits:
// lo = ((v + 64) & 127) - 64 in [-64, 63], hi = (v - lo) / 128 with |hi| <= 64 for |v| <= 8128; D = 1 where every value of the group
// lies in [-64, 63].  Tile (group, k) is digit k of the group's 16 columns; group g's tiles are group_first[g] .. group_first[g + 1].
// With indicators 0 / 1 an int32 accumulator gains at most 64 a row: KGX_GSCORE_ACC_ROWS rows stay below 2^30.
//
// k_weight_operands (once per batch and device): the weights as digit bytes in MFMA B-operand order, 1 KiB per (64-row step, tile):
//   operands[(step * n_tiles + tile) * 64 + lane], lane (c, u) = column 16 group + c, bytes j = 0 .. 15 = the list positions
//   batch_first + 64 step + 16 u + j.  A position past the list's end and a column past n_columns are ZERO bytes: the product needs
//   no tail handling along K.
//
// k_genome_scores: a workgroup of 256 threads owns 256 adjacent genomes of the shard (wave w the 16-byte chunk 4 blockIdx.x + w of
//   every row: rows are read in 64-byte runs), one column group (blockIdx.y) and a slice of the batch's 256-row segments (blockIdx.z).
//   Rows: for a 64-row step lane (i, u) loads the wave's chunk of list position 16 u + i of the step; dword t of it holds the genomes
//   16 t .. 16 t + 15 of that ONE row.  Four exchange stages inside each 16-lane row (lane xor 8, 4, 2, 1; 2-bit elements move by
//   16, 8, 4, 2 bits) transpose the 16 x 16 codes of each dword: afterwards dword t of lane (i, u) holds genome 16 t + i for the rows
//   16 u .. 16 u + 15 of the step -- the A operand's K slots of M tile t -- and pair_indicators gives the H / M / O operands straight
//   from registers.  The genome mask's chunk is ANDed into the loaded chunk first: a masked genome is code 0 and adds nowhere.
//   A segment is 4 steps; the next segment's four chunks (16 VGPRs) are in flight while this segment's steps issue, and the list
//   entries of the segment after that, so that no load waits for the one before it.
//   Guards: a chunk >= chunks_per_row is never read (the whole wave idles but takes part in the barriers and in the staging); a
//   position past the list's end loads nothing and counts as zero; genomes past the shard's end are computed (the padding of the
//   pitch may hold anything) and never stored.
//   Weights: the group's operands of a segment (4 steps x D tiles x 1 KiB) are shared by the four waves through two LDS buffers,
//   one barrier a segment: wave w fetches step w's tiles.
//   Products: 4 M tiles x 3 kinds x D MFMAs a step and wave into 4 x 3 x D accumulator tiles: 96 accumulator VGPRs at D = 2.
//   Store: lane (c, u) holds column c for the genomes 16 t + 4 u + reg of the wave's 64; acc_lo + 128 acc_hi is formed in int64 in
//   registers and ADDED into the table (zeroed once per call by k_gscore_clear; later batches add): a plain += when the list is not
//   split (every word has one owner per launch), a 64-bit atomicAdd when it is split over gridDim.z.
#pragma once

#include <cstdint>

#include "kgx_kernels_indicators.h"

namespace kgx {

constexpr uint32_t kGscoreGenomes = 256;                                      // genomes of a workgroup: one 64-genome chunk a wave
constexpr uint32_t kGscoreSegment = 4;                                        // steps of a segment
constexpr uint32_t kGscoreSegmentRows = kGscoreSegment * kPairTile;           // 256 list positions
constexpr uint32_t kGscoreDigits = 2;                                         // digits of a group at most
constexpr uint32_t kGscoreNoRow = 0xFFFFFFFFu;

// Digit `digit` (0 or 1) of v in signed base 128: lo in [-64, 63], hi = (v - lo) / 128 (exact: the difference is a multiple of 128).
__host__ __device__ inline int32_t gscore_digit(int32_t v, uint32_t digit) {
  const int32_t lo = ((v + 64) & 127) - 64;
  return digit == 0 ? lo : (v - lo) / 128;
}

// x of lane ^ S inside a 16-lane row.  8 is a rotation of the row by 8 (DPP row_ror:8), 2 and 1 are quad permutations (DPP
// quad_perm [2,3,0,1] and [1,0,3,2]); 4 has no DPP pattern and goes through __shfl_xor.
template <int S>
__device__ __forceinline__ uint32_t gscore_from_xor(uint32_t x) {
  if constexpr (S == 8) return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x128, 0xF, 0xF, true));
  else if constexpr (S == 2) return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x4E, 0xF, 0xF, true));
  else if constexpr (S == 1) return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0xB1, 0xF, 0xF, true));
  else return static_cast<uint32_t>(__shfl_xor(static_cast<int>(x), S));
}

// One stage of the 16 x 16 transpose of 2-bit elements (lane i of a 16-lane row = row i, element j of the dword = column j): the
// lanes i and i ^ S swap their off-diagonal S x S blocks.  pair_transpose_stage's shape with 2-bit elements: shift 2 S.  Without
// a branch: the upper lane takes (other >> 2 S) & LOW, the lower (other << 2 S) & ~LOW -- one rotation by a per-lane amount (what
// wraps around falls under the mask) and one bit select; the amounts and masks are the lane's constants.
template <int S, uint32_t LOW>
__device__ __forceinline__ uint32_t gscore_stage(uint32_t x, uint32_t lane) {
  const bool upper = (lane & static_cast<uint32_t>(S)) != 0;
  const uint32_t other = gscore_from_xor<S>(x), keep = upper ? ~LOW : LOW;
  const uint32_t moved = __builtin_amdgcn_alignbit(other, other, upper ? 2u * S : 32u - 2u * S);   // rotate right
  return (x & keep) | (moved & ~keep);
}

// In: element j of lane i = the code of (row i, genome j).  Out: element j of lane i = the code of (row j, genome i).
__device__ __forceinline__ uint32_t gscore_transpose(uint32_t x, uint32_t lane) {
  x = gscore_stage<8, 0x0000FFFFu>(x, lane);
  x = gscore_stage<4, 0x00FF00FFu>(x, lane);
  x = gscore_stage<2, 0x0F0F0F0Fu>(x, lane);
  return gscore_stage<1, 0x33333333u>(x, lane);
}

// weights: [n_columns][n_rows] by list position; group_first: [n_groups + 1] the groups' first tiles; operands: [steps * n_tiles * 64]
// 16-byte units of the batch that begins at list position batch_first; n_units = steps * n_groups * kGscoreDigits * 64 are walked.
__global__ void __launch_bounds__(kBlock)
k_weight_operands(const int16_t* __restrict__ weights, uint64_t n_rows, uint32_t n_columns, uint64_t batch_first, const uint32_t* __restrict__ group_first,
                  uint32_t n_groups, uint32_t n_tiles, uint64_t n_units, kgx_v4u* __restrict__ operands) {
  for (uint64_t unit = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; unit < n_units; unit += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const uint32_t lane = static_cast<uint32_t>(unit & 63u), c = lane & 15u, u = lane >> 4;
    const uint64_t at = unit >> 6, step = at / (n_groups * kGscoreDigits);
    const uint32_t slot = static_cast<uint32_t>(at % (n_groups * kGscoreDigits)), group = slot / kGscoreDigits, digit = slot % kGscoreDigits;
    const uint32_t first_tile = group_first[group];
    if (digit >= group_first[group + 1] - first_tile) continue;               // a one-digit group has no second tile
    const uint64_t column = static_cast<uint64_t>(group) * 16u + c, p0 = batch_first + step * kPairTile + 16u * u;
    kgx_v4u bytes = {0u, 0u, 0u, 0u};
    if (column < n_columns) {
#pragma unroll
      for (uint32_t j = 0; j < 16; ++j)
        if (p0 + j < n_rows) bytes[j >> 2] |= (static_cast<uint32_t>(gscore_digit(weights[column * n_rows + p0 + j], digit)) & 0xFFu) << (8u * (j & 3u));
    }
    operands[(step * n_tiles + first_tile + digit) * kWave + lane] = bytes;
  }
}

// rows: the shard's rows (chunks_per_row 16-byte chunks each) of n_genomes genomes; keep: the genome mask's row or null; row_list:
// the WHOLE list on the device (null: position = row) of n_rows positions; the batch begins at list position batch_first and has
// n_segments 256-row segments, segments_per_slice of them per blockIdx.z; operands, group_first as above; out: the shard's table
// [n_genomes][n_columns][3].
__global__ void __launch_bounds__(kBlock, 2)
k_genome_scores(const kgx_v4u* __restrict__ rows, uint32_t chunks_per_row, uint64_t n_genomes, const kgx_v4u* __restrict__ keep,
                const uint32_t* __restrict__ row_list, uint64_t n_rows, uint64_t batch_first, const kgx_v4u* __restrict__ operands,
                const uint32_t* __restrict__ group_first, uint32_t n_tiles, uint32_t n_columns, uint32_t n_segments, uint32_t segments_per_slice, int atomic,
                long long* __restrict__ out) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  __shared__ kgx_v4u staged[2][kGscoreSegment][kGscoreDigits][kWave];         // [buffer][step][digit][lane]: 16 KiB
  const uint32_t seg_begin = blockIdx.z * segments_per_slice;
  const uint32_t seg_end = seg_begin + segments_per_slice < n_segments ? seg_begin + segments_per_slice : n_segments;
  if (seg_begin >= seg_end) return;                                           // (the whole workgroup)
  const uint32_t first_tile = group_first[blockIdx.y], digits = group_first[blockIdx.y + 1] - first_tile;   // 1 or 2
  const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, i = lane & 15u, u = lane >> 4;
  const uint32_t chunk = blockIdx.x * (kGscoreGenomes / kPairTile) + wave;
  const bool active = chunk < chunks_per_row;                                 // (the whole wave)
  const kgx_v4u mask = keep != nullptr && active ? keep[chunk] : kgx_v4u{~0u, ~0u, ~0u, ~0u};

  // ---- fetching: the rows of the lane's four list positions of a segment (their list entries a segment earlier); step `wave` of
  // the segment's weight operands
  uint32_t next_index[kGscoreSegment];
  kgx_v4u next_rows[kGscoreSegment], next_ops[kGscoreDigits];
  auto fetch_index = [&](uint32_t segment) {
    const uint64_t p0 = batch_first + static_cast<uint64_t>(segment) * kGscoreSegmentRows + 16u * u + i;
#pragma unroll
    for (uint32_t d = 0; d < kGscoreSegment; ++d) {
      const uint64_t position = p0 + kPairTile * d;
      next_index[d] = kGscoreNoRow;
      if (active && segment < seg_end && position < n_rows) next_index[d] = row_list ? row_list[position] : static_cast<uint32_t>(position);
    }
  };
  auto fetch = [&](uint32_t segment) {                                        // after fetch_index(segment)
#pragma unroll
    for (uint32_t d = 0; d < kGscoreSegment; ++d) {
      next_rows[d] = kgx_v4u{0u, 0u, 0u, 0u};
      if (next_index[d] != kGscoreNoRow) next_rows[d] = rows[static_cast<uint64_t>(next_index[d]) * chunks_per_row + chunk];
    }
    const kgx_v4u* src = operands + ((static_cast<uint64_t>(segment) * kGscoreSegment + wave) * n_tiles + first_tile) * kWave + lane;
    next_ops[0] = src[0];
    if (digits > 1) next_ops[1] = src[kWave];
  };
  auto land = [&](uint32_t buffer) {
    staged[buffer][wave][0][lane] = next_ops[0];
    if (digits > 1) staged[buffer][wave][1][lane] = next_ops[1];
  };

  v4i acc[kPairTile / 16][kPairKinds][kGscoreDigits];
#pragma unroll
  for (uint32_t t = 0; t < kPairTile / 16; ++t)
#pragma unroll
    for (uint32_t k = 0; k < kPairKinds; ++k)
#pragma unroll
      for (uint32_t e = 0; e < kGscoreDigits; ++e) acc[t][k][e] = v4i{0, 0, 0, 0};

  fetch_index(seg_begin);
  fetch(seg_begin);
  fetch_index(seg_begin + 1);
  land(0u);
  __syncthreads();
  for (uint32_t segment = seg_begin; segment < seg_end; ++segment) {
    const uint32_t buffer = (segment - seg_begin) & 1u;
    const bool more = segment + 1 < seg_end;
    kgx_v4u codes[kGscoreSegment];
#pragma unroll
    for (uint32_t d = 0; d < kGscoreSegment; ++d) codes[d] = next_rows[d] & mask;
    if (more) {                                                               // in flight over this segment's steps
      fetch(segment + 1);
      fetch_index(segment + 2);
    }
    if (active) {
#pragma unroll
      for (uint32_t d = 0; d < kGscoreSegment; ++d) {
        const v4i b_lo = __builtin_bit_cast(v4i, staged[buffer][d][0][lane]);
        v4i b_hi = {0, 0, 0, 0};
        if (digits > 1) b_hi = __builtin_bit_cast(v4i, staged[buffer][d][1][lane]);
#pragma unroll
        for (uint32_t t = 0; t < kPairTile / 16; ++t) {
          kgx_v4u h, m, o;
          pair_indicators(gscore_transpose(codes[d][t], lane), h, m, o);
          const v4i a_h = __builtin_bit_cast(v4i, h), a_m = __builtin_bit_cast(v4i, m), a_o = __builtin_bit_cast(v4i, o);
          acc[t][0][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_h, b_lo, acc[t][0][0], 0, 0, 0);
          acc[t][1][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_m, b_lo, acc[t][1][0], 0, 0, 0);
          acc[t][2][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_o, b_lo, acc[t][2][0], 0, 0, 0);
          if (digits > 1) {
            acc[t][0][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_h, b_hi, acc[t][0][1], 0, 0, 0);
            acc[t][1][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_m, b_hi, acc[t][1][1], 0, 0, 0);
            acc[t][2][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_o, b_hi, acc[t][2][1], 0, 0, 0);
          }
        }
      }
    }
    if (more) land(buffer ^ 1u);                                              // its readers passed the last barrier
    __syncthreads();
  }
  if (!active) return;

  // lane (c = i, u): column c of the group for the genomes 16 t + 4 u + reg of the wave's chunk
  const uint64_t column = static_cast<uint64_t>(blockIdx.y) * 16u + i;
  if (column >= n_columns) return;
#pragma unroll
  for (uint32_t t = 0; t < kPairTile / 16; ++t)
#pragma unroll
    for (uint32_t reg = 0; reg < 4; ++reg) {
      const uint64_t g = static_cast<uint64_t>(chunk) * kPairTile + 16u * t + 4u * u + reg;
      if (g >= n_genomes) continue;
      long long* words = out + (g * n_columns + column) * kPairKinds;
#pragma unroll
      for (uint32_t k = 0; k < kPairKinds; ++k) {
        long long sum = acc[t][k][0][reg];
        if (digits > 1) sum += 128ll * acc[t][k][1][reg];
        if (!atomic) words[k] += sum;
        else if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(&words[k]), static_cast<unsigned long long>(sum));
      }
    }
}

// table[0 .. n_words) = 0
__global__ void __launch_bounds__(kBlock)
k_gscore_clear(long long* __restrict__ table, uint64_t n_words) {
  for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; w < n_words; w += static_cast<uint64_t>(gridDim.x) * kBlock) table[w] = 0;
}

}  // namespace kgx
