// The bit-sliced counters of the by-genome sweep (k_count_by_genome, kgx_kernels_dosage.h) on their own: plain integer
// code without HIP includes, so that tests/tools/sliced_counters_check.cpp can drive the very structure the kernel uses
// with plain g++ (tests/test_sliced_counters_cpu.py).  The qualifier is the only difference between the two builds.
#ifndef KGX_SLICED_COUNTERS_H
#define KGX_SLICED_COUNTERS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define KGX_COUNTERS_FN __host__ __device__ __forceinline__
#else
#define KGX_COUNTERS_FN inline
#endif

namespace kgx {

constexpr int kHiPlanes = 8;                 // weights 16 .. 2048
constexpr int kBlocksPerFlush = 510;         // blocks of 8 rows: 510*8 + 15 < 16 * 2^kHiPlanes

KGX_COUNTERS_FN void csa(uint32_t& carry, uint32_t& sum, uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t u = a ^ b;
  carry = (a & b) | (u & c);
  sum = u ^ c;
}

template <int NW>
struct SlicedCounters {
  // bit planes of weight 1, 2, 4, 8 and 16 << p; pending = the weight-8 carry of an odd block, waiting for its partner
  uint32_t ones[NW], twos[NW], fours[NW], eights[NW], hi[NW][kHiPlanes], pending[NW];
  KGX_COUNTERS_FN void clear() {
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      ones[i] = twos[i] = fours[i] = eights[i] = pending[i] = 0;
#pragma unroll
      for (int p = 0; p < kHiPlanes; ++p) hi[i][p] = 0;
    }
  }
  // Fold 8 input words of stream-word i; returns the carry of weight 8.
  KGX_COUNTERS_FN uint32_t add8(int i, const uint32_t x[8]) {
    uint32_t t2a, t2b, f4a, f4b, e8;
    csa(t2a, ones[i], ones[i], x[0], x[1]);
    csa(t2b, ones[i], ones[i], x[2], x[3]);
    csa(f4a, twos[i], twos[i], t2a, t2b);
    csa(t2a, ones[i], ones[i], x[4], x[5]);
    csa(t2b, ones[i], ones[i], x[6], x[7]);
    csa(f4b, twos[i], twos[i], t2a, t2b);
    csa(e8, fours[i], fours[i], f4a, f4b);
    return e8;
  }
  // Two weight-8 carries (of two blocks of 8 rows) into the weight-8 plane; its carry ripples through the planes above --
  // once per 16 rows instead of once per 8.
  KGX_COUNTERS_FN void add_eights(int i, uint32_t a, uint32_t b) {
    uint32_t c16;
    csa(c16, eights[i], eights[i], a, b);
#pragma unroll
    for (int p = 0; p < kHiPlanes; ++p) {
      const uint32_t t = hi[i][p] & c16;
      hi[i][p] ^= c16;
      c16 = t;
    }
  }
  // Integer count of bit position b of stream-word i.
  KGX_COUNTERS_FN uint32_t value(int i, int b) const {
    uint32_t v = ((ones[i] >> b) & 1u) | (((twos[i] >> b) & 1u) << 1) | (((fours[i] >> b) & 1u) << 2) | (((eights[i] >> b) & 1u) << 3);
#pragma unroll
    for (int p = 0; p < kHiPlanes; ++p) v |= ((hi[i][p] >> b) & 1u) << (4 + p);
    return v;
  }
};

}  // namespace kgx

#endif  // KGX_SLICED_COUNTERS_H
