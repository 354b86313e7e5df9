// The plan of a kgx_inbreed call (kgl_gene_amd/csrc/kgx_inbreed_plan.h) on its own, without a device: the segment cuts over a
// grid of shapes, the invariant that Loglikelihood on moments has a writer of the hits' words, and the table of which path a
// call takes.  Built and run by tests/test_inbreed_plan_cpu.py:  g++ -std=c++20 -I kgl_gene_amd/csrc
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "kgx_inbreed_plan.h"

using namespace kgx;

namespace {

long long checks = 0, failures = 0;
InbreedShape current;

void expect(bool ok, const char* what) {
  ++checks;
  if (ok) return;
  if (++failures <= 20)
    std::fprintf(stderr, "FAILED: %s  (genomes %llu, g0 %llu, loci %llu, amax %u, phased %d, algorithm %d, compute units %d)\n", what,
                 (unsigned long long)current.n, (unsigned long long)current.g0, (unsigned long long)current.n_sel, current.amax, (int)current.phased,
                 current.algorithm, current.compute_units);
}

enum Path { kOneLaunch, kMomentsCandidate, kPasses, kFrequencySweepOnly };

Path path_of(const InbreedShape& s, const InbreedPlan& p) {
  if (s.algorithm != kAlgoHallME && s.algorithm != kAlgoLoglikelihood) return kFrequencySweepOnly;
  if (p.wave_sized) return kOneLaunch;
  return (s.algorithm == kAlgoHallME ? p.hall_candidate : p.loglik_candidate) ? kMomentsCandidate : kPasses;
}

InbreedShape shape(uint64_t n, uint64_t g0, uint64_t n_sel, uint32_t amax, bool phased, int algorithm, int compute_units) {
  InbreedShape s;
  s.n = n; s.g0 = g0; s.n_sel = n_sel; s.amax = amax; s.phased = phased; s.algorithm = algorithm; s.compute_units = compute_units;
  return s;
}

void check_cuts(const InbreedShape& s, const InbreedSwitches& sw) {
  current = s;
  const InbreedPlan p = plan_inbreed(s, sw);
  // the segments cover the selection, and none of them is empty
  expect(p.n_seg * p.per_seg >= s.n_sel, "n_seg * per_seg covers n_sel");
  expect(p.eval_n_seg * p.eval_per_seg >= s.n_sel, "eval_n_seg * eval_per_seg covers n_sel");
  expect(p.n_seg >= 1 && p.eval_n_seg >= 1 && p.pass_n_seg >= 1, "at least one segment");
  expect(s.n_sel == 0 || (p.n_seg - 1) * p.per_seg < s.n_sel, "no empty segment");
  expect(s.n_sel == 0 || (p.eval_n_seg - 1) * p.eval_per_seg < s.n_sel, "no empty table-pass segment");
  expect(p.per_seg % 8 == 0, "per_seg is whole batches of 8");
  expect(p.eval_per_seg % 8 == 0, "eval_per_seg is whole batches of 8");
  expect(p.n_seg <= 65535 && p.eval_n_seg <= 65535 && p.pass_n_seg <= 65535 && p.max_seg <= 65535, "segment counts fit a grid dimension");
  expect(p.pass_n_seg == (p.eval_lut ? p.eval_n_seg : p.n_seg) && p.max_seg == (p.eval_n_seg > p.n_seg ? p.eval_n_seg : p.n_seg), "pass_n_seg, max_seg");
  if (p.table_sweep) expect(p.per_seg <= kRitlandSegment, "per_seg within the 12-bit class counters on the table sweep");
  else expect(p.per_seg <= 65535, "per_seg within the 16-bit class counters off the table sweep");
  // (off the tables no table pass runs and eval_per_seg is per_seg itself)
  if (p.eval_lut || p.table_sweep) expect(p.eval_per_seg >= 64, "eval_per_seg >= 64");
  else expect(p.eval_per_seg == p.per_seg && p.eval_n_seg == p.n_seg, "off the tables the table passes' cut is the sweep's");
  expect(p.eval_gpl == 4 || p.eval_gpl == 8, "eval_gpl is 4 or 8");
  expect(s.g0 % static_cast<uint64_t>(p.eval_gpl) == 0, "eval_gpl divides g0");
  // Loglikelihood on moments: somebody writes the hits' words
  expect(!p.loglik_candidate || (p.hit_words_planned && (p.hall_mfma || p.eval_gpl == 8)), "loglik_candidate implies a hit-word writer");
  expect(!(p.hall_candidate && p.loglik_candidate), "one estimator a call");
  expect(!p.by_moments() || !p.wave_sized, "the moments are for calls past the one-launch size");
  expect(p.by_moments() == (p.moments_extra_bytes != 0) && p.by_moments() == (p.hall_items != 0), "the moments' sizes are planned with them");
  expect(!p.hall_bits_planned || p.hall_mfma, "bit rows feed the matrix-core pass alone");
  InbreedPlan q = p;
  q.take_the_passes();
  expect(!q.by_moments() && !q.hall_mfma && !q.hall_bits_planned && !q.hit_words_planned, "take_the_passes drops every moments decision");
}

void check_decision(const InbreedShape& s, const InbreedSwitches& sw, Path want, const char* what) {
  current = s;
  expect(path_of(s, plan_inbreed(s, sw)) == want, what);
}

}  // namespace

int main() {
  const uint64_t genomes[] = {1, 4, 5, 64, 777, 2504, 10000};
  const uint64_t loci[] = {0, 1, 8, 63, 8192, 8193, 65536, 5000000};
  const uint32_t amaxes[] = {1, 4, 7, 8, 14, 15};
  const uint64_t starts[] = {0, 4, 8, 16};
  const int units[] = {8, 256};
  const InbreedSwitches defaults;
  InbreedSwitches gpl4;
  gpl4.eval_gpl = 4;
  for (uint64_t n : genomes)
    for (uint64_t n_sel : loci)
      for (uint32_t amax : amaxes)
        for (uint64_t g0 : starts)
          for (int phased = 0; phased < 2; ++phased)
            for (int algorithm = 0; algorithm < 4; ++algorithm)
              for (int cu : units) {
                check_cuts(shape(n, g0, n_sel, amax, phased != 0, algorithm, cu), defaults);
                check_cuts(shape(n, g0, n_sel, amax, phased != 0, algorithm, cu), gpl4);
              }

  // The decisions, with default switches unless named
  for (uint64_t n : genomes)
    for (int cu : units) {
      for (int algorithm : {kAlgoHallME, kAlgoLoglikelihood})
        for (uint32_t amax : {1u, 4u, 7u, 8u, 14u})
          for (int phased = 0; phased < 2; ++phased)
            for (uint64_t g0 : starts)
              check_decision(shape(n, g0, 8192, amax, phased != 0, algorithm, cu), defaults, kOneLaunch, "8192 loci, amax <= 14: one launch");
      for (uint32_t amax : {1u, 4u, 7u, 8u, 14u})
        for (int phased = 0; phased < 2; ++phased)
          for (uint64_t g0 : starts)
            check_decision(shape(n, g0, 8193, amax, phased != 0, kAlgoHallME, cu), defaults, kMomentsCandidate, "HallME at 8193 loci: moments candidate");
      check_decision(shape(n, 0, 9000, 15, true, kAlgoHallME, cu), defaults, kPasses, "HallME at 9000 loci, amax 15: passes");
      check_decision(shape(n, 0, 9000, 15, false, kAlgoHallME, cu), defaults, kPasses, "HallME at 9000 loci, amax 15, unphased: passes");
      for (uint32_t amax : {1u, 4u, 7u}) {
        for (uint64_t g0 : {0ull, 8ull, 16ull}) {
          const InbreedShape s = shape(n, g0, 8193, amax, true, kAlgoLoglikelihood, cu);
          check_decision(s, defaults, kMomentsCandidate, "Loglikelihood at 8193 loci, phased, g0 % 8 == 0, amax <= 7: moments candidate");
          InbreedSwitches sw;
          sw.search_brent = true;
          check_decision(s, sw, kPasses, "KGX_K7_SEARCH=brent: passes");
          sw = InbreedSwitches(); sw.golden = true;
          check_decision(s, sw, kPasses, "KGX_K7_GOLDEN: passes");
          sw = InbreedSwitches(); sw.estimate_start = 1;
          check_decision(s, sw, kPasses, "KGX_K7_ESTIMATE_START: passes");
          sw = InbreedSwitches(); sw.ll_passes = true;
          check_decision(s, sw, kPasses, "KGX_K7_LL_PASSES: passes");
          sw = InbreedSwitches(); sw.generic = true;
          check_decision(s, sw, kPasses, "KGX_K5_GENERIC: passes");
          sw = InbreedSwitches(); sw.no_eval_lut = true;
          check_decision(s, sw, kPasses, "KGX_K5_NO_EVAL_LUT: passes");
          check_decision(s, gpl4, kPasses, "KGX_K5_EVAL_GPL=4: passes (the search would read words nobody wrote)");
          // ... while HallME, which reads no words, keeps its moments under that switch
          check_decision(shape(n, g0, 8193, amax, true, kAlgoHallME, cu), gpl4, kMomentsCandidate, "HallME under KGX_K5_EVAL_GPL=4: moments candidate");
        }
        check_decision(shape(n, 4, 8193, amax, true, kAlgoLoglikelihood, cu), defaults, kPasses, "Loglikelihood with g0 = 4: passes");
        check_decision(shape(n, 0, 8193, amax, false, kAlgoLoglikelihood, cu), defaults, kPasses, "Loglikelihood unphased: passes");
      }
      check_decision(shape(n, 0, 8193, 8, true, kAlgoLoglikelihood, cu), defaults, kPasses, "Loglikelihood with amax = 8: passes");
    }
  std::printf("inbreed_plan_check: %lld checks, %lld failed\n", checks, failures);
  return failures ? 1 : 0;
}
