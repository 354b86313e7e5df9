// The allele census of the genotype matrix by genome group (driven from kgx_census.hip: kgx_gt8_allele_census).
//
// Per selected locus and genome group the census counts KINDS of cell: reference cells, copies of alts the call cannot name,
// crowded cells, and per alt a = 1..amax the cells holding one copy and the cells holding two (kgx.h).  With ind[kind][g] the
// 0 / 1 / 2 a cell adds to a kind and member[g][group] the 0 / 1 membership of its genome,
//     count[locus][kind][group] = sum over g of  ind[locus][kind][g] * member[g][group]
// is an exact int8 -> int32 matrix product: v_mfma_i32_16x16x64_i8 sums 64 genomes x 16 (locus, kind) rows x 16 groups per
// instruction, and the group axis costs the vector unit nothing -- it builds the indicator bytes once per (locus, kind, genome),
// whatever the number of groups (a second product per tile above 16 groups).
//
// Operands (lane l of a wave: c = l & 15, u = l >> 4; both sides take 16 k per lane with the same k map -- kgx_kernels_hall.h --
// so genome 64 * chunk + 16 * u + j only has to sit in byte j of lane (., u) on BOTH sides):
//   A[row c][k]     the indicator bytes of the lane's (locus, kind) row: from ONE 16-byte load of the locus's row, by SWAR
//   B[k][col c]     the membership of those 16 genomes in group c (16 + c for the second product): from 16 bytes of the
//                   per-genome group ids; id 0xFF and the ids past the shard's genomes (0xFF too) match no group, so the pad
//                   bytes of a row's pitch cannot count
//   C[row][col]     lane l holds group c, rows 4 * u + reg
// A wave owns three tiles of 16 rows and a few loci (census_loci_per_wave): two ALLELE tiles -- rows (locus, alt a, one copy | two
// copies), 2 * amax per locus -- and one tile of the three FIXED kinds per locus.  A tile's lanes then all run the same
// instructions (a wave pays for every branch any of its lanes takes: with the kinds of one locus dealt over one tile every lane
// paid for the unknown-copies arithmetic: 21.4 ms instead of 11.4 ms at 10,000 genomes x 10^6 loci, amax 3, profiles/gt8_census.md);
// rows left over count something nobody stores.  The wave walks
// its loci's rows 64 genomes at a time, all genomes of the shard: every word of the result is written once, by one lane, with a
// plain store -- no atomics, the same bits on every run.
#pragma once

#include <cstdint>

#include "kgx_kernels_common.h"

namespace kgx {

constexpr uint32_t kCensusAlleleRows = 32;                                    // (locus, alt, copies) rows of a wave: two 16-row tiles
constexpr uint32_t kCensusFixedRows = 16;                                     // (locus, fixed kind) rows: one tile
constexpr uint32_t kCensusWaves = kBlock / kWave;
constexpr uint32_t kCensusFixedKinds = 3;                                     // reference cells, unknown copies, crowded cells

__host__ __device__ inline uint32_t census_kinds(uint32_t amax) { return kCensusFixedKinds + 2u * amax; }
// loci a wave takes at a time: what its fixed tile (5) and its allele tiles (32 / (2 amax), at least 1: amax <= 14) hold
__host__ __device__ inline uint32_t census_loci_per_wave(uint32_t amax) {
  const uint32_t fixed = kCensusFixedRows / kCensusFixedKinds, allele = kCensusAlleleRows / (2u * amax);
  return fixed < allele ? fixed : allele;
}

// Four cells of one locus -> the four bytes they add to a row.  The nibble tests leave their answer in bit 4 of each byte:
// 0x10 - x has it set iff x == 0 (x <= 15: no borrow), x + 15 - amax iff x > amax (at most 29: no carry into the next byte).
// An allele row: alt4 = the alt in every byte; two_copies: the row counts the cells holding the alt twice, not once.
__device__ __forceinline__ uint32_t census_allele_indicator(uint32_t w, uint32_t alt4, bool two_copies) {
  const uint32_t lo = w & 0x0F0F0F0Fu, hi = (w >> 4) & 0x0F0F0F0Fu;
  const uint32_t lo_none = 0x10101010u - lo;                                  // the first nibble is 0
  const uint32_t lo_is = 0x10101010u - (lo ^ alt4), hi_is = 0x10101010u - (hi ^ alt4);
  const uint32_t twice = hi_is & (lo_is | lo_none);                           // (a, a) and the repeated-record pair (0, a)
  const uint32_t once = (lo_is ^ hi_is) & ~(hi_is & lo_none);
  return ((two_copies ? twice : once) >> 4) & 0x01010101u;
}
// A fixed row: kind 0 = reference cells (byte 0x00), 1 = the copies of alts past amax (15 among them) of a cell that is not
// crowded, 2 = crowded cells (byte 0xFF).  q4: (15 - amax) in every byte.
__device__ __forceinline__ uint32_t census_fixed_indicator(uint32_t w, uint32_t kind, uint32_t q4) {
  const uint32_t lo = w & 0x0F0F0F0Fu, hi = (w >> 4) & 0x0F0F0F0Fu;
  const uint32_t lo_none = 0x10101010u - lo, hi_none = 0x10101010u - hi;
  const uint32_t crowded = 0x10101010u - ((lo & hi) ^ 0x0F0F0F0Fu);           // both nibbles 15
  const uint32_t flag = ((kind == 2u ? crowded : lo_none & hi_none) >> 4) & 0x01010101u;
  const uint32_t first = (((lo + q4) & ~crowded) >> 4) & 0x01010101u;
  const uint32_t second = (((hi + q4) & ~crowded) >> 4) & 0x01010101u;
  const uint32_t unknown = first + second + ((lo_none >> 4) & second);        // (0, a): that alt twice
  return kind == 1u ? unknown : flag;
}

// 1 in the bytes of `ids` that equal `group`
__device__ __forceinline__ uint32_t census_member(uint32_t ids, uint32_t group4) {
  const uint32_t x = ids ^ group4;
  const uint32_t nonzero = ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x;
  return (~nonzero >> 7) & 0x01010101u;
}

// gt: the shard's rows (pitch a multiple of 128 bytes); group_of: one id per byte of a row's pitch, 0xFF past the shard's genomes;
// n_chunks = ceil(shard genomes / 64) (64 * n_chunks <= pitch: every 16-byte load stays inside its row);
// locus_index: the batch's rows or null (rows first, first + 1, ..); out[n_sel][n_groups][3 + 2 * amax].
__global__ void __launch_bounds__(kBlock)
k_allele_census(const uint8_t* __restrict__ gt, uint64_t pitch, uint32_t n_chunks, const uint8_t* __restrict__ group_of,
                const uint32_t* __restrict__ locus_index, uint64_t first, uint64_t n_sel, uint32_t amax, uint32_t n_groups,
                uint32_t* __restrict__ out) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, c = lane & 15u, u = lane >> 4;
  const uint32_t kinds = census_kinds(amax), loci_per_wave = census_loci_per_wave(amax), allele_rows = 2u * amax;
  const uint32_t q4 = (15u - amax) * 0x01010101u;
  const bool upper = n_groups > 16u;                                          // (the same for the whole grid)
  const uint32_t low4 = c * 0x01010101u, high4 = (16u + c) * 0x01010101u;
  const uint64_t units = (n_sel + loci_per_wave - 1) / loci_per_wave;
  // the lane's row of each tile: tiles 0 and 1 allele rows 16 t + c, tile 2 fixed row c
  uint32_t slot_of[3], alt4[2];
  bool two_copies[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const uint32_t r = 16u * t + c, k = r % allele_rows;
    slot_of[t] = r / allele_rows;
    alt4[t] = (1u + k / 2u) * 0x01010101u;
    two_copies[t] = (k & 1u) != 0u;
  }
  slot_of[2] = c / kCensusFixedKinds;
  const uint32_t fixed_kind = c % kCensusFixedKinds;
  for (uint64_t unit = static_cast<uint64_t>(blockIdx.x) * kCensusWaves + wave; unit < units; unit += static_cast<uint64_t>(gridDim.x) * kCensusWaves) {
    const uint64_t unit_first = unit * loci_per_wave;
    const uint64_t unit_last = (unit_first + loci_per_wave <= n_sel ? unit_first + loci_per_wave : n_sel) - 1;
    // where the locus of each of the lane's rows begins (a row past the unit's loci reads the unit's last locus: nobody stores
    // what it counts)
    const uint8_t* bytes[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      uint64_t s = unit_first + slot_of[t];
      if (slot_of[t] >= loci_per_wave || s > unit_last) s = unit_last;
      const uint64_t locus = locus_index ? static_cast<uint64_t>(locus_index[s]) : first + s;
      bytes[t] = gt + locus * pitch + 16u * u;
    }
    const uint8_t* ids = group_of + 16u * u;
    v4i acc[3][2];
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t][0] = acc[t][1] = v4i{0, 0, 0, 0};
    for (uint32_t chunk = 0; chunk < n_chunks; ++chunk) {
      const kgx_v4u w0 = __builtin_nontemporal_load(reinterpret_cast<const kgx_v4u*>(bytes[0] + 64ull * chunk));
      const kgx_v4u w1 = __builtin_nontemporal_load(reinterpret_cast<const kgx_v4u*>(bytes[1] + 64ull * chunk));
      const kgx_v4u w2 = __builtin_nontemporal_load(reinterpret_cast<const kgx_v4u*>(bytes[2] + 64ull * chunk));
      const kgx_v4u g = *reinterpret_cast<const kgx_v4u*>(ids + 64ull * chunk);
      v4i a[3], b_low, b_high;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        a[0][d] = static_cast<int>(census_allele_indicator(w0[d], alt4[0], two_copies[0]));
        a[1][d] = static_cast<int>(census_allele_indicator(w1[d], alt4[1], two_copies[1]));
        a[2][d] = static_cast<int>(census_fixed_indicator(w2[d], fixed_kind, q4));
        b_low[d] = static_cast<int>(census_member(g[d], low4));
      }
#pragma unroll
      for (int t = 0; t < 3; ++t) acc[t][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], b_low, acc[t][0], 0, 0, 0);
      if (upper) {
#pragma unroll
        for (int d = 0; d < 4; ++d) b_high[d] = static_cast<int>(census_member(g[d], high4));
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[t][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], b_high, acc[t][1], 0, 0, 0);
      }
    }
    // lane (c, u) holds group c (16 + c) of each tile's rows 4 u + reg
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const uint32_t r = (t < 2 ? 16u * t : 0u) + 4u * u + reg;
        const uint32_t slot = t < 2 ? r / allele_rows : r / kCensusFixedKinds;
        const uint32_t kind = t < 2 ? kCensusFixedKinds + r % allele_rows : r % kCensusFixedKinds;
        const uint64_t s = unit_first + slot;
        if (slot >= loci_per_wave || s > unit_last) continue;
        uint32_t* words = out + (s * n_groups) * kinds + kind;
        if (c < n_groups) words[static_cast<uint64_t>(c) * kinds] = static_cast<uint32_t>(acc[t][0][reg]);
        if (16u + c < n_groups) words[static_cast<uint64_t>(16u + c) * kinds] = static_cast<uint32_t>(acc[t][1][reg]);
      }
  }
}

}  // namespace kgx
