// Per-row score tables between the genomes of a 2-bit population (driven from kgx_pair_scores.hip: kgx_pair_scores).
//
// With v[g][i] = tables[i][code(g, rows[i])] the score of a pair is  S(a, b) = sum over i of v[a][i] * v[b][i]:  V V^T of a matrix of
// 14-bit integers -- a product with reuse like kgx_kernels_pairs.h, but WEIGHTED: what a genome contributes in a row is looked up in
// the row's own table.  Exact on v_mfma_i32_16x16x64_i8 by two signed base-128 digits, v = 128 hi + lo, lo in [-64, 63], |hi| <= 64
// for |v| <= KGX_SCORE_MAX:
//     S = LL + 128 X + 16384 HH,   LL = sum lo_a lo_b,   HH = sum hi_a hi_b,   X = sum (lo_a hi_b + hi_a lo_b) = [lo_a | hi_a] . [hi_b | lo_b]
// -- three accumulator tiles and four products per (16 A genomes, 16 B genomes, 64 rows), X being one product of twice the depth.
//
// Stage 1 is k_pair_panel (kgx_kernels_panel.h), unchanged.  k_pair_scores (slot 0): a workgroup owns a pair (A <= B) of 64-genome
// tiles and walks the batch's rows 64 at a time.
//   Digit tables: the host splits the values and lays a step's 64 rows x 2 digits x 4 codes out as 128 dwords, one dword = the four
//   codes' bytes of one (row, digit), in the order the build reads them: [u][j][digit][i] for row 16 u + j + 4 i of the step.  Rows
//   past the batch's end are all zero (the panel pads them with code 0, whose value is not 0).  The step's 512 bytes are staged in
//   LDS two steps ahead and read by broadcast.
//   Operand build: wave w of the four takes side w >> 1 and rows 32 (w & 1) .. of the step, lane = genome of the side's tile: 8
//   panel bytes = 32 codes.  A dword of 16 codes shifted right by 2 j has the codes of rows j, j + 4, j + 8, j + 12 in bits 0, 1 of
//   its four bytes -- masked, these ARE the selectors of v_perm_b32, which picks a byte out of two table dwords: selector c takes
//   code c's byte of the first row's table, 4 + c of the second's, 0x0C is a zero byte.  So two rows a v_perm_b32, and one dword of
//   four operand bytes = shift, two v_and_or, then per digit two v_perm and an or: 9 instructions for 8 bytes.  The k slots of a
//   lane are therefore rows 16 u + j + 4 i at byte 4 j + i -- any order serves a contraction, as long as every operand has it.
//   LDS operand layout as in kgx_kernels_pairs.h: operand (16 genomes, digit), lane (c, u) = genome c, 16 bytes of rows 16 u ..
//   16 u + 15.  Two operand buffers, one barrier a step; on a diagonal pair the B side IS the A side.
//   Products: wave w multiplies A tile w's two digits with the four B tiles' two digits: 12 accumulator tiles (48 VGPRs), 10
//   ds_read_b128 and 16 products a step.  With 33 KiB of LDS and under 128 registers four workgroups share a compute unit, so one
//   wave's build runs beside another's products: the freed registers went into occupancy, not into a larger tile.
//   Store: lane (c, u) holds B genome c, A genomes 4 u + reg; LL + 128 X + 16384 HH in int64; a pair with a genome the mask leaves
//   out is ZERO (from the keep bytes, here, not from the panel).  mode: 0 = store, 1 = add (later batches, same owner), 2 = 64-bit
//   atomicAdd into a zeroed table (the steps split over gridDim.z).
#pragma once

#include <cstdint>

#include "../../include/kgx.h"
#include "kgx_kernels_panel.h"

namespace kgx {

constexpr uint32_t kScoreDigits = 2;
constexpr uint32_t kScoreStepDwords = kPairTile * kScoreDigits;               // a step's digit tables: 512 bytes
// The steps one workgroup may walk in one launch.  Per row an accumulator of X gains at most 2 * 64 * 64 = 2^13 in magnitude (LL and
// HH: 2^12), so 2^17 rows stay within 2^30 < 2^31.
constexpr uint32_t kScoreSteps = KGX_SCORE_ACC_ROWS / kPairTile;
static_assert(static_cast<uint64_t>(KGX_SCORE_ACC_ROWS) * 2u * 64u * 64u < (1ull << 31), "an int32 accumulator of X must hold KGX_SCORE_ACC_ROWS rows");

// Where the table dword of (row of the step, digit) sits among the step's 128: the order k_pair_scores' build reads them in.
__host__ __device__ constexpr uint32_t score_table_slot(uint32_t row, uint32_t digit) {
  return (((row >> 4) * 4u + (row & 3u)) * kScoreDigits + digit) * 4u + ((row >> 2) & 3u);
}

// panel: [64 n_tiles genomes][panel_pitch]; digits: [n_steps][128] table dwords; keep: one byte a genome or null (no mask);
// n_steps 64-row steps of the batch, steps_per_slice <= kScoreSteps of them per blockIdx.z; out: [G (G + 1) / 2];
// blockIdx.x: the tile pair, row-major over A <= B.
__global__ void __launch_bounds__(kBlock)
k_pair_scores(const uint8_t* __restrict__ panel, uint64_t panel_pitch, const uint32_t* __restrict__ digits, const uint8_t* __restrict__ keep, uint32_t n_tiles,
              uint64_t n_genomes, uint32_t n_steps, uint32_t steps_per_slice, int mode, long long* __restrict__ out) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  __shared__ kgx_v4u operands[2][2][kPairTile / 16][kScoreDigits][kWave];     // [buffer][side][16-genome tile][digit][lane]: 32 KiB
  __shared__ kgx_v4u tables[2][kScoreStepDwords / 4];                         // [step parity][(u, j, digit)]: the four rows i
  uint32_t tile_a = 0, rest = blockIdx.x;
  while (rest >= n_tiles - tile_a) { rest -= n_tiles - tile_a; ++tile_a; }
  const uint32_t tile_b = tile_a + rest;
  const bool diagonal = tile_a == tile_b;
  const uint32_t s_begin = blockIdx.z * steps_per_slice;
  const uint32_t s_end = s_begin + steps_per_slice < n_steps ? s_begin + steps_per_slice : n_steps;
  if (s_begin >= s_end) return;                                               // (the whole workgroup)
  const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, c = lane & 15u, u = lane >> 4;

  // staging: the wave's side and half of the step's 64 rows, the lane's genome of the side's tile
  const uint32_t side = wave >> 1, half = wave & 1u;
  const bool stages = !(diagonal && side == 1u);
  const uint8_t* src = panel + (static_cast<uint64_t>(side ? tile_b : tile_a) * kPairTile + lane) * panel_pitch + 8u * half;
  auto build = [&](uint32_t buffer, uint2 codes) {
    if (!stages) return;
#pragma unroll
    for (uint32_t uu = 0; uu < 2; ++uu) {
      const uint32_t w = uu ? codes.y : codes.x, group = 2u * half + uu;     // rows 16 group .. 16 group + 15
      kgx_v4u digit[kScoreDigits];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t x = w >> (2u * j);                                     // bits 0, 1 of byte i: the code of row 16 group + j + 4 i
        const uint32_t first = (x & 0x00000303u) | 0x0C0C0400u, second = (x & 0x03030000u) | 0x04000C0Cu;
#pragma unroll
        for (uint32_t d = 0; d < kScoreDigits; ++d) {
          const kgx_v4u t = tables[buffer][(group * 4u + j) * kScoreDigits + d];
          digit[d][j] = __builtin_amdgcn_perm(t[1], t[0], first) | __builtin_amdgcn_perm(t[3], t[2], second);
        }
      }
#pragma unroll
      for (uint32_t d = 0; d < kScoreDigits; ++d) operands[buffer][side][lane >> 4][d][c + 16u * group] = digit[d];
    }
  };
  // the digit tables of steps s_begin and s_begin + 1, then the first operands
  const bool carries = threadIdx.x < kScoreStepDwords;
  uint32_t* table_words = reinterpret_cast<uint32_t*>(tables);
  if (carries) {
    table_words[threadIdx.x] = digits[static_cast<uint64_t>(s_begin) * kScoreStepDwords + threadIdx.x];
    if (s_begin + 1 < s_end) table_words[kScoreStepDwords + threadIdx.x] = digits[static_cast<uint64_t>(s_begin + 1) * kScoreStepDwords + threadIdx.x];
  }
  uint2 next = {0u, 0u};
  if (stages) next = *reinterpret_cast<const uint2*>(src + 16ull * s_begin);
  __syncthreads();
  build(0u, next);
  __syncthreads();

  v4i ll[4], hh[4], xx[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) ll[t] = hh[t] = xx[t] = v4i{0, 0, 0, 0};
  const uint32_t b_side = diagonal ? 0u : 1u;
  for (uint32_t s = s_begin; s < s_end; ++s) {
    const uint32_t buffer = (s - s_begin) & 1u;
    const bool more = s + 1 < s_end, more_tables = carries && s + 2 < s_end;
    if (more && stages) next = *reinterpret_cast<const uint2*>(src + 16ull * (s + 1));
    uint32_t next_table = 0u;
    if (more_tables) next_table = digits[static_cast<uint64_t>(s + 2) * kScoreStepDwords + threadIdx.x];
    const v4i a_lo = __builtin_bit_cast(v4i, operands[buffer][0][wave][0][lane]), a_hi = __builtin_bit_cast(v4i, operands[buffer][0][wave][1][lane]);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const v4i b_lo = __builtin_bit_cast(v4i, operands[buffer][b_side][t][0][lane]), b_hi = __builtin_bit_cast(v4i, operands[buffer][b_side][t][1][lane]);
      xx[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_lo, b_hi, xx[t], 0, 0, 0);
      ll[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_lo, b_lo, ll[t], 0, 0, 0);
      hh[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_hi, b_hi, hh[t], 0, 0, 0);
      xx[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_hi, b_lo, xx[t], 0, 0, 0);
    }
    // step s + 1's operands from its tables (staged a step ago); step s + 2's tables take the place of step s's, read a step ago
    if (more) build(buffer ^ 1u, next);
    if (more_tables) table_words[buffer * kScoreStepDwords + threadIdx.x] = next_table;
    __syncthreads();                                                          // the other buffer is built; this one is free
  }

  // lane (c, u): B genome c of each B tile, A genomes 4 u + reg of the wave's tile
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const uint64_t ga = static_cast<uint64_t>(tile_a) * kPairTile + 16u * wave + 4u * u + reg;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint64_t gb = static_cast<uint64_t>(tile_b) * kPairTile + 16u * t + c;
      if (ga >= n_genomes || gb >= n_genomes || ga > gb) continue;
      long long v = static_cast<long long>(ll[t][reg]) + 128ll * xx[t][reg] + 16384ll * hh[t][reg];
      if (keep != nullptr && !(keep[ga] && keep[gb])) v = 0;                  // a masked genome reads as code 0, whose value is not 0
      long long* word = out + (ga * n_genomes - ga * (ga - 1) / 2 + (gb - ga));
      if (mode == 0) *word = v;
      else if (mode == 1) *word += v;
      else if (v) atomicAdd(reinterpret_cast<unsigned long long*>(word), static_cast<unsigned long long>(v));
    }
  }
}

}  // namespace kgx
