// Per-row class sums of per-genome columns of a 2-bit population (driven from kgx_assoc.hip: kgx_column_sums).
//
// With I_k[r][g] the 0 / 1 indicator "listed row r has kind k in genome g" (kinds H = code 1, M = code 2, O = code 3) and w[j][g] the
// caller's column j (|w| <= KGX_COLUMN_MAX),
//     S[k](i, j) = sum over g of  I_k[i][g] * w[j][g]
// contracts over GENOMES like kgx_kernels_ld.h, but one side is a dense signed integer, not an indicator.  Exact on
// v_mfma_i32_16x16x64_i8 by signed base-128 digits: w = sum_k d_k 128^k, every d_k in [-64, 63], so that an int32 accumulator holds
// 2^25 genomes (64 * 2^25 = 2^31, reached only from below).
//
// Tiles.  Columns are taken in groups of 16.  A group has D in 1 .. 4 digits, the fewest that hold its largest and smallest value
// (D digits hold -64 S .. 63 S, S = (128^D - 1) / 127); tile (group, k) is digit k of the group's 16 columns.  The tiles of a
// group are adjacent and a PASS is up to 8 tiles of whole groups (the driver packs them; a group is never cut).  With the columns
// on the B side of the product lane (c, u) of the result holds column c of the tile for the wave's rows 4 u + reg -- EVERY digit of
// that column for those rows sits in the one lane, so the store puts sum_k acc_k 128^k together in int64 in registers: no int32
// scratch table and no combine pass.
//
// k_column_operands (once per call and shard): the shard's slice of the columns as digit bytes in MFMA operand order, 1 KiB per
//   (64-genome step, tile): operands[(step * n_tiles + tile) * 64 + lane], lane (c, u) = column 16 group + c, bytes j = 0 .. 15 =
//   the genomes 256 (step / 4) + 64 u + 16 (step % 4) + j -- the PERMUTED order of k_column_sums below.  A masked genome, a genome
//   past the shard's end and a column past n_columns are ZERO bytes: a zero column byte kills whatever the row holds there, so the
//   row side needs no mask, no tail handling and may hold anything in the padding of its pitch.
//
// k_column_sums: a workgroup of 256 threads owns 64 listed rows (wave w the rows 16 w .. 16 w + 15), one pass of tiles
//   (blockIdx.y) and a slice of the shard's 256-genome segments (blockIdx.z).
//   Rows: no LDS and no transposition.  For a segment (4 chunks of 16 bytes a row) lane (c, u) loads chunk u of row c with ONE
//   16-byte load; its dword d holds the genomes 64 u + 16 d .. + 15 of the segment.  Step d of the segment runs pair_indicators on
//   dword d and feeds the H / M / O operands straight from registers: k slots 16 u .. 16 u + 15 of step d ARE the genomes 64 u +
//   16 d ..  -- a contraction does not care about the order of K as long as both sides agree, and k_column_operands agrees.  The
//   next segment's chunk is in flight while this one's four steps issue.  A chunk >= chunks_per_row is never read (past the last
//   row it is past the allocation) and counts as zero; so does a list position past the list's end.
//   Columns: the pass's operands of the segment (4 steps x tiles x 1 KiB, 32 KiB at 8 tiles) are shared by the four waves through
//   double-buffered LDS: wave w fetches step w's tiles into registers while the current segment's products issue, then writes them
//   to the other buffer; one barrier a segment.
//   Products: 3 kinds x tiles MFMAs a step, 96 accumulator VGPRs at 8 tiles.
//   Store: mode 0 = store (the first shard of the device), 1 = add (later shards, same owner), 2 = 64-bit atomicAdd into a zeroed
//   table (the segments split over gridDim.z where few row blocks would leave the device idle: integer sums, exact in any order).
#pragma once

#include <cstdint>

#include "kgx_kernels_indicators.h"

namespace kgx {

constexpr uint32_t kAssocBlock = 64;                                          // listed rows of a workgroup
constexpr uint32_t kAssocSegment = 4;                                         // chunks of a segment: 256 genomes, one 16-byte load a lane
constexpr uint32_t kAssocTiles = 8;                                           // tiles of a pass
constexpr uint32_t kAssocDigits = 4;                                          // digits of a group at most
constexpr uint32_t kAssocGroupMask = 0x0FFFFFFFu;                             // a tile word: group | digit << 28
constexpr uint32_t kAssocNoRow = 0xFFFFFFFFu;

// Digit `digit` of w in signed base 128, every digit in [-64, 63].
__host__ __device__ inline int32_t assoc_digit(int32_t w, uint32_t digit) {
  for (uint32_t k = 0; k < digit; ++k) w = (w - (((w + 64) & 127) - 64)) >> 7;    // exact: the difference is a multiple of 128
  return ((w + 64) & 127) - 64;
}

// columns: [n_columns][total_genomes], the shard's genomes at genome_base ..; keep: the genome mask's row (2 bits a genome) or null;
// tiles: [n_tiles] tile words; operands: [n_units = steps * n_tiles * 64] 16-byte units, steps = 4 * segments of the shard.
__global__ void __launch_bounds__(kBlock)
k_column_operands(const int32_t* __restrict__ columns, uint64_t total_genomes, uint64_t genome_base, uint64_t n_genomes, uint32_t n_columns,
                  const uint8_t* __restrict__ keep, const uint32_t* __restrict__ tiles, uint32_t n_tiles, uint64_t n_units, kgx_v4u* __restrict__ operands) {
  for (uint64_t unit = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; unit < n_units; unit += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const uint32_t lane = static_cast<uint32_t>(unit & 63u), c = lane & 15u, u = lane >> 4;
    const uint64_t at = unit >> 6, step = at / n_tiles;
    const uint32_t word = tiles[at % n_tiles], digit = word >> 28;
    const uint64_t column = static_cast<uint64_t>(word & kAssocGroupMask) * 16u + c;
    const uint64_t g0 = (step >> 2) * (64u * kAssocSegment) + 64u * u + 16u * (step & 3u);
    kgx_v4u bytes = {0u, 0u, 0u, 0u};
    if (column < n_columns && g0 < n_genomes) {
      const int32_t* src = columns + column * total_genomes + genome_base + g0;
      const uint32_t kept = keep ? *reinterpret_cast<const uint32_t*>(keep + g0 / 4u) : ~0u;   // the 16 genomes' mask bits (g0 / 4 < pitch)
#pragma unroll
      for (uint32_t j = 0; j < 16; ++j)
        if (g0 + j < n_genomes && ((kept >> (2u * j)) & 1u))
          bytes[j >> 2] |= (static_cast<uint32_t>(assoc_digit(src[j], digit)) & 0xFFu) << (8u * (j & 3u));
    }
    operands[unit] = bytes;
  }
}

// rows: the shard's rows (chunks_per_row 16-byte chunks each); row_list: the WHOLE list on the device (null: position = row);
// first_block: the batch's first 64-row block of the list; operands, tiles as above; pass_first: [gridDim.y + 1] the passes' first
// tiles; n_segments 256-genome segments of the shard, segments_per_slice of them per blockIdx.z; out: the batch's table
// [64 gridDim.x][n_columns][3].
__global__ void __launch_bounds__(kBlock, 2)
k_column_sums(const kgx_v4u* __restrict__ rows, uint32_t chunks_per_row, const uint32_t* __restrict__ row_list, uint64_t n_rows, uint64_t first_block,
              const kgx_v4u* __restrict__ operands, const uint32_t* __restrict__ tiles, uint32_t n_tiles, const uint32_t* __restrict__ pass_first,
              uint32_t n_columns, uint32_t n_segments, uint32_t segments_per_slice, int mode, long long* __restrict__ out) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  __shared__ kgx_v4u staged[2][kAssocSegment][kAssocTiles][kWave];            // [buffer][step][tile of the pass][lane]: 64 KiB
  const uint64_t block = first_block + blockIdx.x;
  if (block * kAssocBlock >= n_rows) return;                                  // (the whole workgroup)
  const uint32_t seg_begin = blockIdx.z * segments_per_slice;
  const uint32_t seg_end = seg_begin + segments_per_slice < n_segments ? seg_begin + segments_per_slice : n_segments;
  if (seg_begin >= seg_end) return;                                           // (the whole workgroup)
  const uint32_t first_tile = pass_first[blockIdx.y], pass_tiles = pass_first[blockIdx.y + 1] - first_tile;   // 1 .. kAssocTiles
  const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, c = lane & 15u, u = lane >> 4;

  // ---- fetching: chunk u of the segment for the wave's row c; step `wave` of the segment's column operands
  const uint64_t position = block * kAssocBlock + 16u * wave + c;
  const uint32_t row = position < n_rows ? (row_list ? row_list[position] : static_cast<uint32_t>(position)) : kAssocNoRow;
  const kgx_v4u* row_chunks = rows + static_cast<uint64_t>(row == kAssocNoRow ? 0u : row) * chunks_per_row;
  kgx_v4u next_row, next_ops[kAssocTiles];
  auto fetch = [&](uint32_t segment) {
    const uint32_t chunk = segment * kAssocSegment + u;
    next_row = kgx_v4u{0u, 0u, 0u, 0u};
    if (row != kAssocNoRow && chunk < chunks_per_row) next_row = row_chunks[chunk];
    const kgx_v4u* src = operands + ((static_cast<uint64_t>(segment) * kAssocSegment + wave) * n_tiles + first_tile) * kWave + lane;
#pragma unroll
    for (uint32_t t = 0; t < kAssocTiles; ++t)
      if (t < pass_tiles) next_ops[t] = src[static_cast<uint64_t>(t) * kWave];
  };
  auto land = [&](uint32_t buffer) {
#pragma unroll
    for (uint32_t t = 0; t < kAssocTiles; ++t)
      if (t < pass_tiles) staged[buffer][wave][t][lane] = next_ops[t];
  };

  v4i acc[kPairKinds][kAssocTiles];
#pragma unroll
  for (uint32_t k = 0; k < kPairKinds; ++k)
#pragma unroll
    for (uint32_t t = 0; t < kAssocTiles; ++t) acc[k][t] = v4i{0, 0, 0, 0};

  fetch(seg_begin);
  land(0u);
  __syncthreads();
  for (uint32_t segment = seg_begin; segment < seg_end; ++segment) {
    const uint32_t buffer = (segment - seg_begin) & 1u;
    const bool more = segment + 1 < seg_end;
    const kgx_v4u codes = next_row;
    if (more) fetch(segment + 1);                                             // in flight over this segment's steps
#pragma unroll
    for (uint32_t d = 0; d < kAssocSegment; ++d) {
      kgx_v4u h, m, o;
      pair_indicators(codes[d], h, m, o);
      const v4i a_h = __builtin_bit_cast(v4i, h), a_m = __builtin_bit_cast(v4i, m), a_o = __builtin_bit_cast(v4i, o);
#pragma unroll
      for (uint32_t t = 0; t < kAssocTiles; ++t)
        if (t < pass_tiles) {
          const v4i b = __builtin_bit_cast(v4i, staged[buffer][d][t][lane]);
          acc[0][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_h, b, acc[0][t], 0, 0, 0);
          acc[1][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_m, b, acc[1][t], 0, 0, 0);
          acc[2][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_o, b, acc[2][t], 0, 0, 0);
        }
    }
    if (more) land(buffer ^ 1u);                                              // its readers passed the last barrier
    __syncthreads();
  }

  // lane (c, u): column c of each tile, rows 4 u + reg of the wave's 16; the digits of a group are adjacent tiles of the pass
  const uint64_t batch_first = first_block * kAssocBlock;
#pragma unroll
  for (uint32_t reg = 0; reg < 4; ++reg) {
    const uint64_t i = block * kAssocBlock + 16u * wave + 4u * u + reg;
    long long sum[kPairKinds] = {0, 0, 0};
#pragma unroll
    for (uint32_t t = 0; t < kAssocTiles; ++t)
      if (t < pass_tiles) {
        const uint32_t word = tiles[first_tile + t], group = word & kAssocGroupMask;
        const long long weight = 1ll << (7u * (word >> 28));
#pragma unroll
        for (uint32_t k = 0; k < kPairKinds; ++k) sum[k] += weight * acc[k][t][reg];
        if (t + 1 < pass_tiles && (tiles[first_tile + t + 1] & kAssocGroupMask) == group) continue;   // more digits of the group follow
        const uint64_t column = static_cast<uint64_t>(group) * 16u + c;
        if (i < n_rows && column < n_columns) {
          long long* words = out + ((i - batch_first) * n_columns + column) * kPairKinds;
#pragma unroll
          for (uint32_t k = 0; k < kPairKinds; ++k) {
            if (mode == 0) words[k] = sum[k];
            else if (mode == 1) words[k] += sum[k];
            else if (sum[k]) atomicAdd(reinterpret_cast<unsigned long long*>(&words[k]), static_cast<unsigned long long>(sum[k]));
          }
        }
        sum[0] = sum[1] = sum[2] = 0;
      }
  }
}

// table += other (a table another device filled, copied over)
__global__ void __launch_bounds__(kBlock)
k_assoc_add(long long* __restrict__ table, const long long* __restrict__ other, uint64_t n_words) {
  for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; w < n_words; w += static_cast<uint64_t>(gridDim.x) * kBlock) table[w] += other[w];
}

// table[0 .. n_words) = 0
__global__ void __launch_bounds__(kBlock)
k_assoc_clear(long long* __restrict__ table, uint64_t n_words) {
  for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; w < n_words; w += static_cast<uint64_t>(gridDim.x) * kBlock) table[w] = 0;
}

}  // namespace kgx
