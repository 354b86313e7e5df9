// What the two Z Z^T products of the 2-bit population share (kgx_kernels_pairs.h: genome x genome over rows; kgx_kernels_ld.h: row x
// row over genomes): the tile constants and the step from 16 codes to a lane's 16 indicator bytes per kind.
#pragma once

#include <cstdint>

#include "kgx_kernels_common.h"

namespace kgx {

constexpr uint32_t kPairTile = 64;                                            // genomes of a tile = rows of a step
constexpr uint32_t kPairKinds = 3;                                            // H, M, O
constexpr uint32_t kPairWords = kPairKinds * kPairKinds;                      // words per genome pair
constexpr uint32_t kPairOperands = (kPairTile / 16) * kPairKinds;             // operands a side and step: 12 of 1 KiB

// One dword of 16 codes -> the lane's 16 bytes of the H, M and O operands.  (b * 0x41041) moves bit 2 i of a byte to bit 8 i:
// the partial products that meet (bits 6, 12, 18) carry into odd bits nobody reads.
__device__ __forceinline__ void pair_indicators(uint32_t w, kgx_v4u& h, kgx_v4u& m, kgx_v4u& o) {
  const uint32_t lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const uint32_t lb = __umul24((lo >> (8 * d)) & 0xFFu, 0x41041u) & 0x01010101u;
    const uint32_t hb = __umul24((hi >> (8 * d)) & 0xFFu, 0x41041u) & 0x01010101u;
    o[d] = lb & hb;
    h[d] = lb ^ o[d];
    m[d] = hb ^ o[d];
  }
}

}  // namespace kgx
