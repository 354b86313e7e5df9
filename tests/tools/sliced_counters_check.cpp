// The bit-sliced counters of the by-genome sweep (kgl_gene_amd/csrc/kgx_sliced_counters.h) on their own, without a device:
// driven exactly as by_genome_pass (kgx_kernels_dosage.h) drives them -- blocks of 8 words per stream word, the weight-8
// carries of two blocks going up together, `pending` holding an odd block's, a flush every kBlocksPerFlush blocks and at the
// end -- against plain per-bit counts.  Built and run by tests/test_sliced_counters_cpu.py:  g++ -std=c++20 -I kgl_gene_amd/csrc
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <random>
#include <vector>

#include "kgx_sliced_counters.h"

using namespace kgx;

namespace {

long long checks = 0, failures = 0;

void expect(bool ok, const char* what, long long a = 0, long long b = 0) {
  ++checks;
  if (ok) return;
  if (++failures <= 20) std::fprintf(stderr, "FAILED: %s (%lld, %lld)\n", what, a, b);
}

// by_genome_pass without the loads: feed() is one step of its loop, flush() its lambda; totals[i][b] stands for the LDS counters.
template <int NW>
struct Pass {
  SlicedCounters<NW> cnt;
  int blocks = 0, flushes = 0;
  int period;                                  // kBlocksPerFlush, or another number to show what a wrong one does
  uint64_t totals[NW][32] = {};
  explicit Pass(int flush_period = kBlocksPerFlush) : period(flush_period) { cnt.clear(); }
  void flush() {
    if (blocks & 1)
      for (int i = 0; i < NW; ++i) cnt.add_eights(i, cnt.pending[i], 0u);
    for (int i = 0; i < NW; ++i)
      for (int b = 0; b < 32; ++b) totals[i][b] += cnt.value(i, b);
    cnt.clear();
    blocks = 0;
    ++flushes;
  }
  void feed(const uint32_t w[NW][8]) {
    uint32_t e8[NW];
    for (int i = 0; i < NW; ++i) e8[i] = cnt.add8(i, w[i]);
    if (blocks & 1) {
      for (int i = 0; i < NW; ++i) cnt.add_eights(i, cnt.pending[i], e8[i]);
    } else {
      for (int i = 0; i < NW; ++i) cnt.pending[i] = e8[i];
    }
    if (++blocks == period) flush();
  }
};

// n_blocks blocks of words with every bit set with probability `density` (1.0: all ones); are all NW * 32 counts right?
template <int NW>
bool run(int n_blocks, double density, uint64_t seed, int period = kBlocksPerFlush, int* flushes = nullptr) {
  std::mt19937_64 rng(seed);
  std::bernoulli_distribution bit(density);
  Pass<NW> pass(period);
  uint64_t want[NW][32] = {};
  for (int k = 0; k < n_blocks; ++k) {
    uint32_t w[NW][8];
    for (int i = 0; i < NW; ++i)
      for (int j = 0; j < 8; ++j) {
        uint32_t x = 0;
        if (density >= 1.0) x = 0xFFFFFFFFu;
        else
          for (int b = 0; b < 32; ++b) x |= static_cast<uint32_t>(bit(rng)) << b;
        w[i][j] = x;
        for (int b = 0; b < 32; ++b) want[i][b] += (x >> b) & 1u;     // the reference: one add per bit
      }
    pass.feed(w);
  }
  pass.flush();
  if (flushes) *flushes = pass.flushes;
  bool ok = true;
  for (int i = 0; i < NW; ++i)
    for (int b = 0; b < 32; ++b) ok = ok && pass.totals[i][b] == want[i][b];
  return ok;
}

template <int NW>
void check_all() {
  // every bit position reads 8 * blocks: up to one full period without a flush in between, the last case with every one of
  // the eight high planes set (510 * 8 = 4080 = 0xFF0)
  for (int n : {1, 2, 3, 509, 510}) {
    int flushes = 0;
    expect(run<NW>(n, 1.0, 1, kBlocksPerFlush, &flushes), "all-ones input within one period", NW, n);
    expect(flushes == (n == kBlocksPerFlush ? 2 : 1), "one flush at the end (and the period's own at 510 blocks)", n, flushes);
  }
  // ... and across periods: the flush in the middle neither loses nor doubles a carry, whatever the parity of the tail
  for (int n : {511, 512, 1019, 1020, 1021, 1100, 1533}) expect(run<NW>(n, 1.0, 2), "all-ones input across flush periods", NW, n);
  // an odd block count at the flush: the last block's weight-8 carries sit in `pending`
  for (int n : {1, 3, 7, 509}) {
    Pass<NW> pass;
    uint32_t w[NW][8];
    for (int i = 0; i < NW; ++i)
      for (int j = 0; j < 8; ++j) w[i][j] = 0xFFFFFFFFu;
    for (int k = 0; k < n; ++k) pass.feed(w);
    bool waiting = true;
    for (int i = 0; i < NW; ++i) waiting = waiting && pass.cnt.pending[i] == 0xFFFFFFFFu;
    expect(waiting, "an odd block's carries wait in pending", NW, n);
    pass.flush();
    bool ok = true;
    for (int i = 0; i < NW; ++i)
      for (int b = 0; b < 32; ++b) ok = ok && pass.totals[i][b] == 8ull * n;
    expect(ok, "odd block count at the flush", NW, n);
  }
  // random words, dense enough for the top plane
  uint64_t seed = 100;
  for (double density : {0.5, 0.7, 0.8, 0.9, 0.95})
    for (int n : {1, 2, 7, 16, 255, 509, 510, 511, 1021, 1533}) expect(run<NW>(n, density, ++seed), "random words", n, static_cast<long long>(density * 100));
  // the bound is real, not slack: without a flush 511 blocks still fit (4088 + the weight-1..4 planes), 512 lose the carry out
  // of the top plane (4096 = 16 << kHiPlanes reads as 0)
  expect(run<NW>(511, 1.0, 3, 1 << 30), "511 blocks without a flush are still exact", NW);
  expect(!run<NW>(512, 1.0, 3, 1 << 30), "512 blocks without a flush lose a carry", NW);
}

}  // namespace

int main() {
  expect(kBlocksPerFlush * 8 + 15 < (16 << kHiPlanes), "kBlocksPerFlush * 8 + 15 < 16 << kHiPlanes", kBlocksPerFlush, kHiPlanes);
  expect(kBlocksPerFlush >= 2, "a period holds at least one pair of blocks", kBlocksPerFlush);
  check_all<4>();          // MODE 0: the chunk's four dwords
  check_all<2>();          // MODE 1: the two words of non-diploid indicators
  std::printf("sliced counters: %lld checks, %lld failed\n", checks, failures);
  return failures == 0 ? 0 : 1;
}
