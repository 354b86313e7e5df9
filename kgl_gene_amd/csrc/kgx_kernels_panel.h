// The genome-major 2-bit panel of a row batch: what the walks and products that take a genome ALONG the listed rows start from
// (kgx_kernels_pairs.h: the pair counts; kgx_kernels_pair_runs.h: the shared runs of genome pairs).  k_pair_panel is described at
// the top of kgx_kernels_pairs.h; it is `inline` because more than one translation unit launches it.
#pragma once

#include <cstdint>

#include "kgx_kernels_indicators.h"

namespace kgx {

template <int S, uint32_t LOW>
__device__ __forceinline__ void pair_transpose_stage(uint32_t& lo, uint32_t& hi, uint32_t lane) {
  const uint32_t other_lo = __shfl_xor(lo, S), other_hi = __shfl_xor(hi, S);
  if (lane & static_cast<uint32_t>(S)) {
    lo = ((other_lo >> S) & LOW) | (lo & ~LOW);
    hi = ((other_hi >> S) & LOW) | (hi & ~LOW);
  } else {
    lo = (lo & LOW) | ((other_lo & LOW) << S);
    hi = (hi & LOW) | ((other_hi & LOW) << S);
  }
}

// 64 x 64 bit transpose across a wave: lane i comes in with row i (bit j = column j) and leaves with column i (bit j = row j);
// at block size s the lanes i and i ^ s swap their off-diagonal s x s blocks.
__device__ __forceinline__ void pair_transpose_tile(uint32_t& lo, uint32_t& hi, uint32_t lane) {
  const uint32_t other_lo = __shfl_xor(lo, 32), other_hi = __shfl_xor(hi, 32);
  if (lane & 32u) lo = other_hi; else hi = other_lo;
  pair_transpose_stage<16, 0x0000FFFFu>(lo, hi, lane);
  pair_transpose_stage<8, 0x00FF00FFu>(lo, hi, lane);
  pair_transpose_stage<4, 0x0F0F0F0Fu>(lo, hi, lane);
  pair_transpose_stage<2, 0x33333333u>(lo, hi, lane);
  pair_transpose_stage<1, 0x55555555u>(lo, hi, lane);
}

// bits 0 .. 15 of x to the even bits of a dword
__device__ __forceinline__ uint32_t pair_spread16(uint32_t x) {
  x &= 0x0000FFFFu;
  x = (x | (x << 8)) & 0x00FF00FFu;
  x = (x | (x << 4)) & 0x0F0F0F0Fu;
  x = (x | (x << 2)) & 0x33333333u;
  return (x | (x << 1)) & 0x55555555u;
}

// rows: the shard's rows (chunks_per_row 16-byte chunks each); keep: the genome mask's row or null; row_list: the batch's rows
// (null: first_row, first_row + 1, ..); panel: the shard's first genome, [64 gridDim.y genomes][panel_pitch = 16 n_tiles bytes].
// gridDim.y = ceil(shard genomes / 64) <= chunks_per_row.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wcuda-compat"                              // clang honours `inline` on a kernel; the warning is about nvcc
inline __global__ void __launch_bounds__(kBlock)
k_pair_panel(const kgx_v4u* __restrict__ rows, uint32_t chunks_per_row, uint64_t n_genomes, const kgx_v4u* __restrict__ keep,
             const uint32_t* __restrict__ row_list, uint64_t first_row, uint64_t batch_rows, uint8_t* __restrict__ panel, uint64_t panel_pitch) {
  const uint32_t lane = threadIdx.x % kWave, odd = lane & 1u;
  const uint64_t tile = static_cast<uint64_t>(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;
  if (tile * 16u >= panel_pitch) return;                                      // (the whole wave)
  const uint32_t chunk = blockIdx.y;
  const uint64_t r = tile * kPairTile + lane;
  kgx_v4u x = {0u, 0u, 0u, 0u};
  if (r < batch_rows) {
    const uint64_t row = row_list ? static_cast<uint64_t>(row_list[r]) : first_row + r;
    x = rows[row * chunks_per_row + chunk];
  }
  if (keep != nullptr) x &= keep[chunk];
#pragma unroll
  for (int d = 0; d < 4; ++d) {                                               // the bytes past the shard's genomes are nobody's
    const uint64_t g0 = static_cast<uint64_t>(chunk) * 64u + 16u * d;
    const uint32_t valid = n_genomes >= g0 + 16u ? 16u : (n_genomes > g0 ? static_cast<uint32_t>(n_genomes - g0) : 0u);
    if (valid < 16u) x[d] &= (1u << (2u * valid)) - 1u;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint32_t lo = x[2 * h], hi = x[2 * h + 1];
    pair_transpose_tile(lo, hi, lane);                                        // lane: plane (lane & 1) of genome 32 h + (lane >> 1), bit i = row i
    const uint32_t other = __shfl_xor(odd ? lo : hi, 1), mine = odd ? hi : lo;  // the even lane takes rows 0 .. 31, the odd one 32 .. 63
    const uint32_t plane0 = odd ? other : mine, plane1 = odd ? mine : other;
    uint2 w;
    w.x = pair_spread16(plane0) | (pair_spread16(plane1) << 1);
    w.y = pair_spread16(plane0 >> 16) | (pair_spread16(plane1 >> 16) << 1);
    const uint64_t genome = static_cast<uint64_t>(chunk) * 64u + 32u * h + (lane >> 1);
    *reinterpret_cast<uint2*>(panel + genome * panel_pitch + tile * 16u + 8u * odd) = w;
  }
}
#pragma clang diagnostic pop

}  // namespace kgx
