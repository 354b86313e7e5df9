// What one kgx_inbreed / kgx_inbreed_objective call over one shard WILL do, decided in one place from the call's shape and a
// snapshot of the KGX_* switches, before anything touches the device: the flavour of the frequency sweep, how the loci are cut
// into segments, which of the estimators' paths is a candidate, what the moments would need beyond the arena.  Host-only and
// pure (no HIP runtime, no environment): kgx_inbreed.hip fills the two inputs and drives the stages the plan names; the
// one decision that needs the device -- is there room for the moments -- stays there (InbreedPlan::take_the_passes).
#ifndef KGX_INBREED_PLAN_H
#define KGX_INBREED_PLAN_H

#include <cassert>
#include <cstddef>
#include <stdint.h>

#include "kgx_inbreed_constants.h"

namespace kgx {

// The algorithms of include/kgx.h (KGX_ALGO_*), which this header does not include: checked against it in kgx_inbreed.hip.
constexpr int kAlgoRitlandLocus = 0, kAlgoSimple = 1, kAlgoHallME = 2, kAlgoLoglikelihood = 3;

// Every KGX_K5_* / KGX_K7_* / KGX_KEEP_SCRATCH_GB / KGX_TIME_SMALL_CALLS switch the driver reads, with its default: read once, at
// the top of a call (read_switches in kgx_inbreed.hip), clamped as the driver always clamped them.
struct InbreedSwitches {
  bool generic = false;              // KGX_K5_GENERIC: the per-cell kernels everywhere
  bool no_eval_lut = false;          // KGX_K5_NO_EVAL_LUT
  bool no_table_sweep = false;       // KGX_K5_NO_TABLE_SWEEP (not for RitlandLocus)
  bool no_swar16 = false;            // KGX_K5_NO_SWAR16
  int eval_gpl = 8;                  // KGX_K5_EVAL_GPL, forced to 4 or 8: genomes per lane of the table passes
  int blocks_per_cu = 8;             // KGX_K5_BLOCKS_PER_CU
  int eval_resident = 2;             // KGX_K5_EVAL_RESIDENT
  int eval_rounds = 8;               // KGX_K5_EVAL_ROUNDS
  int sequential_min = 1 << 16;      // KGX_K5_SEQUENTIAL_MIN
  bool always_guard = false;         // KGX_K5_ALWAYS_GUARD
  uint32_t xcds = 1;                 // KGX_K5_XCDS, at least 1
  bool time_small_calls = false;     // KGX_TIME_SMALL_CALLS
  int keep_scratch_gb = -1;          // KGX_KEEP_SCRATCH_GB; negative: a quarter of the device's memory
  bool no_wave = false;              // KGX_K7_NO_WAVE
  int wave_loci = 1024;              // KGX_K7_WAVE_LOCI, in [1, kGenomeWaveLoci]
  int wave_genomes = 1024;           // KGX_K7_WAVE_GENOMES, at least 1 (default: 1024 for HallME, 512 for Loglikelihood)
  bool search_brent = false;         // KGX_K7_SEARCH=brent
  bool hall_passes = false;          // KGX_K7_HALL_PASSES
  bool golden = false;               // KGX_K7_GOLDEN
  int estimate_start = 0;            // KGX_K7_ESTIMATE_START (handed to k_brent_init as it is)
  bool ll_passes = false;            // KGX_K7_LL_PASSES
  bool ll_het_terms = false;         // KGX_K7_LL_HET_TERMS
  int ll_dense_per_1024 = 0;         // KGX_K7_LL_DENSE_PER_1024; <= 0: kLoglikDense
  bool class_sweeps = false;         // KGX_K7_CLASS_SWEEPS
  bool class_bytes = false;          // KGX_K7_CLASS_BYTES
  bool order_one_lane = false;       // KGX_K7_ORDER_ONE_LANE
  bool no_pair = false;              // KGX_K7_NO_PAIR
  bool no_compact = false;           // KGX_K7_NO_COMPACT
  int compact_min_genomes = 2048;    // KGX_K7_COMPACT_MIN_GENOMES
  int compact_min_cells = 1 << 26;   // KGX_K7_COMPACT_MIN_CELLS
  bool trace = false;                // KGX_K7_TRACE
};

struct InbreedShape {
  uint64_t n = 0;                    // genomes of the call (of this shard)
  uint64_t g0 = 0;                   // the first of them, shard-local
  uint64_t n_sel = 0;                // selected loci
  uint32_t amax = 1;
  int phased = 0;                    // as the caller gave it (the kernels take it so): non-zero = a phased population
  int algorithm = kAlgoSimple;
  int objective_method = 0;          // kgx_inbreed_objective: 1 by the moments, 2 by a table pass
  bool has_locus_index = false;
  int compute_units = 0;
};

struct InbreedPlan {
  // the frequency sweep's flavour
  bool ritland = false, table_sweep = false, swar16 = false, generic_sweep = false, eval_lut = false;
  int eval_gpl = 8;                  // as the group's alignment allows
  uint32_t gx = 0, gx16 = 0;         // workgroups across the genomes: 4 / 16 of them per lane
  // the three cuts of the loci: the frequency sweep's, the table passes', an estimator pass's (modes 1, 2)
  uint64_t n_seg = 1, per_seg = 8, eval_n_seg = 1, eval_per_seg = 8, max_seg = 1, pass_n_seg = 1;
  bool sequential_defaults = false, wave_sized = false, table_passes = false;
  // the estimators' paths.  A candidate runs on the moments if the device has the room (the driver's test: take_the_passes if not)
  int search = kSearchNelderMead, pass_search = kSearchNelderMead;
  uint64_t planes = 1;               // values of F per genome and pass
  bool hall_candidate = false, loglik_candidate = false;
  uint32_t hall_classes = 1;
  uint64_t hall_items = 0, hall_blocks = 0;   // per class, at most
  uint64_t words_per_block = 0;
  bool hall_mfma = false, hall_bits_planned = false;
  bool hit_words_planned = false;    // a class pass that writes the hits' words runs: what k_loglik_search reads
  uint64_t sel_pitch = 0, bit_row_bytes = 0;
  uint64_t moments_extra_bytes = 0;  // what the moments take beyond the arena's plain part, at most

  bool by_moments() const { return hall_candidate || loglik_candidate; }
  // No room for the moments (or no bin for a frequency): the passes, which need none of it.
  void take_the_passes() {
    hall_candidate = loglik_candidate = hall_mfma = hall_bits_planned = hit_words_planned = false;
    hall_items = hall_blocks = 0;
  }
};

inline InbreedPlan plan_inbreed(const InbreedShape& s, const InbreedSwitches& sw) {
  InbreedPlan p;
  const uint64_t n = s.n, g0 = s.g0, n_sel = s.n_sel;
  const uint32_t amax = s.amax;
  const uint64_t compute_units = static_cast<uint64_t>(s.compute_units);
  // Frequency pass flavour.  With allele indices that fit the tables (amax <= 7): ONE table pass that yields the class
  // counts and the class-frequency sums (k_inbreed_eval_lut<4>) and, for RitlandLocus, the Ritland terms with them
  // (k_inbreed_eval_lut<3>).  KGX_K5_NO_TABLE_SWEEP=1 (not for RitlandLocus): the SWAR sweeps instead -- 16 genomes per
  // lane (16-byte loads) when the group starts on a 16-genome boundary, otherwise 4 genomes per lane (amax <= 4).
  p.ritland = s.algorithm == kAlgoRitlandLocus;
  const bool no_tables = sw.generic || sw.no_eval_lut;
  p.table_sweep = !no_tables && amax <= 7 && n_sel <= 65535ull * kRitlandSegment && (p.ritland || !sw.no_table_sweep);
  p.swar16 = !p.table_sweep && !sw.generic && !sw.no_swar16 && amax <= 4 && (g0 & 15u) == 0 && !p.ritland;
  p.generic_sweep = !p.table_sweep && !p.swar16 && (sw.generic || amax > 4 || p.ritland);
  // The evaluation passes of HallME / Loglikelihood go through the per-batch LDS tables when the allele indices fit them.
  p.eval_lut = !no_tables && amax <= 7;
  p.eval_gpl = sw.eval_gpl;                                  // genomes per lane: the widest load the group's alignment allows
  if (p.eval_gpl != 4 && p.eval_gpl != 8) p.eval_gpl = 8;
  while (p.eval_gpl > 4 && (g0 % static_cast<uint64_t>(p.eval_gpl)) != 0) p.eval_gpl /= 2;
  p.gx = static_cast<uint32_t>(((n + 3) / 4 + kBlock - 1) / kBlock);
  p.gx16 = static_cast<uint32_t>(((n + 15) / 16 + kBlock - 1) / kBlock);
  const uint32_t sweep_gx = p.swar16 ? p.gx16 : p.gx;
  uint64_t n_seg = (compute_units * sw.blocks_per_cu + sweep_gx - 1) / sweep_gx;
  if (n_seg > (n_sel + 63) / 64) n_seg = (n_sel + 63) / 64;
  if (n_seg < (n_sel + 65534) / 65535) n_seg = (n_sel + 65534) / 65535;   // 16-bit class counters per segment
  if (n_seg < 1) n_seg = 1;
  if (n_seg > 65535) n_seg = 65535;
  uint64_t per_seg = n_sel ? (n_sel + n_seg - 1) / n_seg : 8;
  per_seg = (per_seg + 7) / 8 * 8;                                          // whole 8-locus batches per segment
  n_seg = n_sel ? (n_sel + per_seg - 1) / per_seg : 1;
  // The table passes cut the loci for their own launch shape: 256-thread workgroups of eval_gpl genomes per lane, two or
  // three resident per CU (registers), about eight rounds of them and never a workgroup more than that (one more, nearly
  // empty round costs an eighth of the pass).
  uint64_t eval_n_seg = n_seg, eval_per_seg = per_seg;
  if (p.eval_lut || p.table_sweep) {
    const uint64_t eval_gx = ((n + p.eval_gpl - 1) / p.eval_gpl + kBlock - 1) / kBlock;
    const uint64_t resident = compute_units * static_cast<uint64_t>(sw.eval_resident);
    uint64_t want = resident * static_cast<uint64_t>(sw.eval_rounds) / eval_gx;
    if (want < 1) want = 1;
    if (want > 65535) want = 65535;
    eval_per_seg = n_sel ? (n_sel + want - 1) / want : kEvalBatch;
    eval_per_seg = (eval_per_seg + 7) / 8 * 8;
    if (eval_per_seg < 64) eval_per_seg = 64;
    eval_n_seg = n_sel ? (n_sel + eval_per_seg - 1) / eval_per_seg : 1;
    if (p.table_sweep) {                                     // the frequency sweep's own cut: 12-bit class counters per segment
      per_seg = eval_per_seg > kRitlandSegment ? kRitlandSegment : eval_per_seg;
      n_seg = n_sel ? (n_sel + per_seg - 1) / per_seg : 1;
    }
  }
  p.n_seg = n_seg; p.per_seg = per_seg; p.eval_n_seg = eval_n_seg; p.eval_per_seg = eval_per_seg;
  p.max_seg = eval_n_seg > n_seg ? eval_n_seg : n_seg;
  p.pass_n_seg = p.eval_lut ? eval_n_seg : n_seg;                           // segments of an estimator pass (modes 1, 2)

  // The class-frequency sums of the defaults in the reference's own (sequential) summation order (k_seq_* kernels): from
  // the size at which a tree reduction and a sequential sum part by more than a tenth of the tolerance.
  const bool swar_family = p.table_sweep || (!sw.generic && amax <= 4 && !p.ritland);
  p.sequential_defaults = swar_family && n_sel >= static_cast<uint64_t>(sw.sequential_min);
  // The table passes' entries (k_eval_entries): 64 / 256 / 1024 bytes per selected locus, only where such a pass will run.
  // (amax > 14: a selection with offsets of more than 14 reference alts -- their cells are in the matrix's wide rows, which the
  // generic per-cell kernels alone read: no one-launch iteration, no moments; the table passes and SWAR sweeps stop at amax 7 / 4 anyway)
  const bool iterative = s.algorithm == kAlgoHallME || s.algorithm == kAlgoLoglikelihood;
  p.wave_sized = n_sel > 0 && n_sel <= static_cast<uint64_t>(kGenomeLoci) && !sw.no_wave && s.objective_method == 0 && amax <= 14;
  p.table_passes = n_sel > 0 && (p.table_sweep || (p.eval_lut && iterative && !p.wave_sized));

  // HallME and Loglikelihood over a large call: per-genome moments of the homozygous cells' frequencies instead of 50 / 38
  // passes (kgx_kernels_hall.h, kgx_kernels_loglik.h)
  // (any amax for HallME: the class passes compare bytes, no table; the generic / no-table flavours keep the passes they are there to test)
  p.search = sw.search_brent ? kSearchBrent : kSearchNelderMead;
  p.hall_candidate = s.algorithm == kAlgoHallME && n_sel > 0 && n_sel < (1ull << 31) && !p.wave_sized && !no_tables && amax <= 14 &&
                     !sw.hall_passes;                                       // (the radix sort counts its items in an int)
  // Loglikelihood: the reference optimiser's path alone, a phased population (unphased: every alt homozygote is a heterozygous
  // cell that can meet the upper bound -- every genome would be handed to the passes), the frequency sweep as a table pass
  // (it carries the heterozygous cells' term), positions in 28 bits -- and eight genomes per lane: the search reads the hits'
  // words, a lane of eight genomes' (k_hall_mfma<true, *>, k_hall_sweep<8, true>); the four-genome class pass
  // (k_hall_sweep<4, false>, under KGX_K5_EVAL_GPL=4 or a group that starts off an 8-genome boundary) writes none.
  p.loglik_candidate = s.algorithm == kAlgoLoglikelihood && n_sel > 0 && n_sel < (1ull << 28) && !p.wave_sized && !no_tables &&
                       p.table_sweep && s.phased && (g0 & 7u) == 0 && p.eval_gpl == 8 && p.search == kSearchNelderMead && !sw.golden &&
                       !sw.estimate_start && !sw.ll_passes;
  p.hall_classes = 1u + (s.phased ? amax : 0u);                             // byte 0x00, and a | a << 4 of a phased population (classify_cell)
  p.hall_items = p.by_moments() ? n_sel / kHallItemLoci + kHallBins + 1 : 0;        // per class, at most
  p.hall_blocks = p.by_moments() ? n_sel / kHallBlockLoci + p.hall_items : 0;        // per class, at most: blocks of 64 slots
  p.words_per_block = (n + 7) / 8 * 8;                                       // one word per genome, whole lanes of 8
  p.bit_row_bytes = hall_bit_row_bytes(n);                                   // whole spans of 2048 genomes
  p.sel_pitch = (n_sel + 7) / 8 * 8;
  // the matrix-core class pass (k_hall_mfma): per slot 32 digit bytes and its row
  p.hall_mfma = p.by_moments() && p.eval_gpl == 8 && !sw.class_sweeps;
  // ... fed by ONE pass over the bytes that leaves every class's hits as bits (k_class_bits): where each selected locus sits in
  // each class's blocks, and the bit rows themselves (a grow-only buffer of their own: an eighth of the bytes the classes cover)
  p.hall_bits_planned = p.hall_mfma && !sw.class_bytes;
  p.hit_words_planned = p.loglik_candidate && (p.hall_mfma || p.eval_gpl == 8);
  assert(!p.loglik_candidate || p.hit_words_planned);        // Loglikelihood on moments searches on words somebody wrote
  if (p.by_moments()) {
    // the moments' buffers (40 B per item and genome, 100 KB of bins per genome; Loglikelihood: a bit per homozygous-capable
    // cell of the bins its floor can reach)
    p.moments_extra_bytes = p.hall_items * kHallMoments * n * sizeof(double) + static_cast<uint64_t>(kHallBins) * kHallMoments * n * sizeof(double) +
                            p.hall_classes * (p.hall_blocks + 1) * kHallBlockLoci * (sizeof(HallRecord) + 36) + n_sel * (sizeof(HallRecord) + 4 * sizeof(uint32_t)) +
                            (p.loglik_candidate ? p.hall_classes * p.hall_blocks * p.words_per_block * sizeof(unsigned long long) : 0) +
                            p.hall_classes * p.hall_blocks * kHallBlockLoci * p.bit_row_bytes;     // (the hits' bit rows, at most)
  }
  // Loglikelihood's search: the reference optimiser's own path (Nelder-Mead, see nm_advance) unless KGX_K7_SEARCH=brent
  // ... two evaluations per pass where a pass is a sweep over the matrix (the table passes): same path, half the passes
  p.pass_search = (p.search == kSearchNelderMead && p.eval_lut && !sw.no_pair) ? kSearchNelderMeadPair : p.search;
  p.planes = p.pass_search == kSearchNelderMeadPair ? 2 : 1;
  return p;
}

}  // namespace kgx

#endif  // KGX_INBREED_PLAN_H
