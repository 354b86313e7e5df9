// Pairwise joint genotype counts between the genomes of a 2-bit population (driven from kgx_pairs.hip: kgx_pair_counts).
//
// With I_p[g][r] the 0 / 1 indicator "genome g has kind p in listed row r" (kinds H = code 1, M = code 2, O = code 3),
//     n[p][q](a, b) = sum over r of  I_p[a][r] * I_q[b][r]
// is Z Z^T of a 0 / 1 matrix: exact in int8 -> int32 on v_mfma_i32_16x16x64_i8, the unit of the Hall moments and the allele
// census.  Unlike those two this is a product WITH reuse -- every 64-genome tile meets every other one -- and it contracts over
// ROWS, which the variant-major matrix keeps apart.  Two stages:
//
// k_pair_panel (every shard on its own device): gathers the listed rows of a row batch and turns them around into a genome-major
//   panel[genome][64-row tile][16 bytes]: dword u of a tile holds rows 16 u .. 16 u + 15 of that genome, row 16 u + k in bits
//   2 k, 2 k + 1.  A wave takes one 16-byte chunk (64 genomes) of 64 rows, lane i the chunk of row i; each half of the chunk is a
//   64 x 64 bit matrix (32 genomes x 2 bit planes), turned around by the six-stage butterfly of the row lists (lane j then holds
//   the 64 rows of plane j & 1 of genome j >> 1); the two lanes of a genome swap a dword and interleave the planes again, the even
//   lane rows 0 .. 31, the odd lane rows 32 .. 63.  The genome mask is ANDed in here; rows past the batch's end and genomes past
//   the shard's end are code 0, and every byte of the panel is written, so padding can never count.
//
// k_pair_counts (slot 0): a workgroup owns a pair (A <= B) of 64-genome tiles and walks the batch's rows 64 at a time.  Per step
//   all 256 threads build the step's 24 operands ONCE: thread t takes 8 bytes of the panel (side t >> 7, genome (t & 127) >> 1,
//   rows 32 (t & 1) ..) and turns each dword of 16 codes into 16 indicator bytes per kind -- the two bit planes spread to bytes by
//   a 24-bit multiply per four codes, then O = lo & hi, H = lo ^ O, M = hi ^ O -- written to LDS in the operand layout of
//   kgx_kernels_hall.h / kgx_kernels_census.h: operand (16 genomes, kind), lane (c, u) = genome c, k = rows 16 u .. 16 u + 15,
//   16 bytes a lane.  Two LDS buffers: the next step's panel bytes are in flight and its operands are built while this step's
//   products issue; one barrier a step.  Wave w multiplies A-side tile w x its three kinds with the four B-side tiles x three
//   kinds: 36 accumulator tiles (144 VGPRs), 15 ds_read_b128 and 36 products a step.  On a diagonal pair the B side IS the A
//   side, staged once.  C: lane (c, u) holds B genome c, A genomes 4 u + reg -- all nine words of a genome pair sit in one
//   lane and leave by plain stores (a <= b only).  mode: 0 = store (first row batch), 1 = add to what the earlier batches stored
//   (the same owner, no atomics), 2 = atomicAdd into a zeroed table (rows split over gridDim.z when there are few tile pairs:
//   integer sums, exact in any order).
#pragma once

#include <cstdint>

#include "kgx_kernels_panel.h"

namespace kgx {

// panel: [64 n_tiles genomes][panel_pitch]; n_steps 64-row steps of the batch, steps_per_slice of them per blockIdx.z;
// out: [G (G + 1) / 2][9]; blockIdx.x: the tile pair, row-major over A <= B.
__global__ void __launch_bounds__(kBlock)
k_pair_counts(const uint8_t* __restrict__ panel, uint64_t panel_pitch, uint32_t n_tiles, uint64_t n_genomes, uint32_t n_steps,
              uint32_t steps_per_slice, int mode, uint32_t* __restrict__ out) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  __shared__ kgx_v4u operands[2][2][kPairOperands][kWave];                    // [buffer][side][16-genome tile x kind][lane]: 48 KiB
  uint32_t tile_a = 0, rest = blockIdx.x;
  while (rest >= n_tiles - tile_a) { rest -= n_tiles - tile_a; ++tile_a; }
  const uint32_t tile_b = tile_a + rest;
  const bool diagonal = tile_a == tile_b;
  const uint32_t s_begin = blockIdx.z * steps_per_slice;
  const uint32_t s_end = s_begin + steps_per_slice < n_steps ? s_begin + steps_per_slice : n_steps;
  if (s_begin >= s_end) return;                                               // (the whole workgroup)
  const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, c = lane & 15u, u = lane >> 4;

  // staging: side, genome of the side's tile, which half of the step's 64 rows
  const uint32_t side = threadIdx.x >> 7, genome = (threadIdx.x & 127u) >> 1, half = threadIdx.x & 1u;
  const bool stages = !(diagonal && side == 1u);
  const uint8_t* src = panel + (static_cast<uint64_t>(side ? tile_b : tile_a) * kPairTile + genome) * panel_pitch + 8u * half;
  auto build = [&](uint32_t buffer, uint2 codes) {
    if (!stages) return;
    kgx_v4u* dst = &operands[buffer][side][(genome >> 4) * kPairKinds][(genome & 15u) + 32u * half];
    kgx_v4u h, m, o;
    pair_indicators(codes.x, h, m, o);
    dst[0] = h; dst[kWave] = m; dst[2 * kWave] = o;
    pair_indicators(codes.y, h, m, o);
    dst[16] = h; dst[kWave + 16] = m; dst[2 * kWave + 16] = o;
  };
  uint2 next = {0u, 0u};
  if (stages) next = *reinterpret_cast<const uint2*>(src + 16ull * s_begin);
  build(0u, next);
  __syncthreads();

  v4i acc[kPairKinds][4][kPairKinds];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int q = 0; q < 3; ++q) acc[p][t][q] = v4i{0, 0, 0, 0};
  const uint32_t b_side = diagonal ? 0u : 1u;
  for (uint32_t s = s_begin; s < s_end; ++s) {
    const uint32_t buffer = (s - s_begin) & 1u;
    const bool more = s + 1 < s_end;
    if (more && stages) next = *reinterpret_cast<const uint2*>(src + 16ull * (s + 1));
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
    if (more) build(buffer ^ 1u, next);
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
      uint32_t* words = out + (ga * n_genomes - ga * (ga - 1) / 2 + (gb - ga)) * kPairWords;
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

}  // namespace kgx
