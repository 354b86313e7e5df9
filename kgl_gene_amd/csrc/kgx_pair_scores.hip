// C ABI (include/kgx.h) of the per-row score tables between genome pairs: kgx_pair_scores (per unordered genome pair the sum over
// the listed rows of the product of the two genomes' table values: kgx_pair_counts' genome-major panel per row batch, then V V^T by
// two base-128 digits on the matrix cores, kgx_kernels_pair_scores.h), kgx_pair_scores_last, and the genomic relationship matrix
// as such tables: kgx_grm_tables / kgx_grm_finish (host only).  No CPU fallback exists for the device part.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

#include "kgx_kernels_pair_scores.h"
#include "kgx_internal.h"

namespace kgx {
namespace {

std::atomic<double> g_last_scores_ms{0.0};
std::atomic<uint64_t> g_last_scores_batches{0}, g_last_scores_splits{0};

// v = 128 hi + lo with lo in [-64, 63]; |v| <= KGX_SCORE_MAX gives |hi| <= 64.
void score_digits(int v, int& lo, int& hi) {
  lo = ((v + 64) & 127) - 64;
  hi = (v - lo) / 128;
}

// The digit tables of list positions [b0, b0 + B) as the kernel reads them: whole steps, the rows past B all zero.
void fill_digit_tables(const int16_t* tables, uint64_t b0, uint64_t B, std::vector<uint32_t>& words) {
  std::fill(words.begin(), words.end(), 0u);
  for (uint64_t r = 0; r < B; ++r) {
    uint32_t word[kScoreDigits] = {0u, 0u};
    for (int c = 0; c < 4; ++c) {
      int lo, hi;
      score_digits(tables[(b0 + r) * 4 + c], lo, hi);
      word[0] |= (static_cast<uint32_t>(lo) & 0xFFu) << (8 * c);
      word[1] |= (static_cast<uint32_t>(hi) & 0xFFu) << (8 * c);
    }
    uint32_t* step = words.data() + r / kPairTile * kScoreStepDwords;
    for (uint32_t d = 0; d < kScoreDigits; ++d) step[score_table_slot(static_cast<uint32_t>(r % kPairTile), d)] = word[d];
  }
}

int pair_scores_impl(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, const int16_t* tables, int64_t* out) {
  const uint64_t G = pop->n_genomes, T = (G + kPairTile - 1) / kPairTile, padded = T * kPairTile;
  const uint64_t pairs = G * (G + 1) / 2, list_bytes = rows ? n_rows * sizeof(uint32_t) : 0, keep_bytes = pop->keep.empty() ? 0 : G;
  const uint64_t step_bytes = kScoreStepDwords * sizeof(uint32_t);
  for (const auto& sh : pop->shards)
    if (sh.n_genomes && sh.genome_base % kPairTile) return fail(KGX_ESTATE, "pair_scores: a shard does not start at a whole 64-genome tile");

  // ---- devices: the product runs on the first shard's; shards on the same HIP device share its stream and arena
  Device& cdev = *pop->shards[0].dev;
  PanelShards shards(pop);
  std::vector<PanelShard>& sb = shards.sb;

  // ---- rows per batch, in whole 64-row steps: the panel and the steps' digit tables within a quarter of (free + arena) on every
  //      device; the pairs' table, the list and the keep bytes beside them on the first
  if (int rc = use_device(cdev)) return rc;
  const uint64_t available = available_bytes(cdev), fixed = pairs * sizeof(int64_t) + list_bytes + keep_bytes + 5 * 256;
  if (fixed + padded * 16 + step_bytes > available)
    return fail(KGX_ENOMEM, "pair_scores: the %llu-byte table of %llu genomes' pairs does not fit beside one 64-row panel into the %llu bytes free on the first device",
                (unsigned long long)(pairs * sizeof(int64_t)), (unsigned long long)G, (unsigned long long)available);
  uint64_t batch_tiles = std::min(available / 4, available - fixed) / (padded * 16 + step_bytes);
  if (int rc = shards.fit_elsewhere(pop, kPairTile, list_bytes, batch_tiles)) return rc;
  batch_tiles = std::max<uint64_t>(1, std::min(batch_tiles, (n_rows + kPairTile - 1) / kPairTile));
  const int row_cap = env_int("KGX_SCORES_ROWS", 0);          // only ever lowers the count
  if (row_cap > 0) batch_tiles = std::min(batch_tiles, (static_cast<uint64_t>(row_cap) + kPairTile - 1) / kPairTile);

  // ---- how the product is cut: tile pairs, and the batch's steps over gridDim.z where the pairs alone leave the device idle.  A
  //      workgroup walks at most kScoreSteps steps in one launch (its int32 accumulators): a longer batch is cut down to that.
  const uint64_t tile_pairs = T * (T + 1) / 2;
  if (tile_pairs > 0x7FFFFFFFull) return fail(KGX_EINVAL, "pair_scores: %llu genomes make more tile pairs than a grid holds", (unsigned long long)G);
  const uint64_t wanted = 2ull * static_cast<uint64_t>(std::max(cdev.compute_units, 1));
  uint64_t slices = tile_pairs < wanted ? std::min<uint64_t>({(wanted + tile_pairs - 1) / tile_pairs, batch_tiles, 65535}) : 1;
  const int slice_cap = env_int("KGX_SCORES_SPLITS", 0);     // only ever lowers the count: the tests walk several steps in one workgroup with it
  if (slice_cap > 0) slices = std::min(slices, static_cast<uint64_t>(slice_cap));
  uint64_t steps_per_slice = (batch_tiles + slices - 1) / slices;
  if (steps_per_slice > kScoreSteps) {
    steps_per_slice = kScoreSteps;
    batch_tiles = slices * kScoreSteps;
  }
  slices = (batch_tiles + steps_per_slice - 1) / steps_per_slice;
  const bool split = slices > 1;
  const uint64_t batch_rows = batch_tiles * kPairTile, panel_pitch = batch_tiles * 16;

  // ---- buffers
  if (int rc = use_device(cdev)) return rc;
  ScratchPlan plan;
  const size_t o_out = plan.add(pairs * sizeof(int64_t)), o_list = plan.add(list_bytes), o_keep = plan.add(keep_bytes);
  const size_t o_digits = plan.add(batch_tiles * step_bytes), o_panel = plan.add(padded * panel_pitch);
  char* arena = nullptr;
  if (int rc = scratch_reserve(cdev, plan.total, &arena)) return rc;
  long long* d_out = reinterpret_cast<long long*>(arena + o_out);
  uint8_t* d_panel = reinterpret_cast<uint8_t*>(arena + o_panel);
  uint32_t* d_digits = reinterpret_cast<uint32_t*>(arena + o_digits);
  const uint32_t* d_list = rows ? reinterpret_cast<const uint32_t*>(arena + o_list) : nullptr;
  const uint8_t* d_keep = keep_bytes ? reinterpret_cast<const uint8_t*>(arena + o_keep) : nullptr;
  if (rows) KGX_HIP(hipMemcpyAsync(arena + o_list, rows, list_bytes, hipMemcpyHostToDevice, cdev.stream));
  if (keep_bytes) KGX_HIP(hipMemcpyAsync(arena + o_keep, pop->keep.data(), keep_bytes, hipMemcpyHostToDevice, cdev.stream));
  KGX_HIP(hipStreamSynchronize(cdev.stream));                 // the sources are pageable host memory
  if (int rc = shards.reserve(pop, kPairTile, rows, list_bytes, d_list, d_panel, panel_pitch)) return rc;

  if (int rc = use_device(cdev)) return rc;
  if (split) KGX_HIP(hipMemsetAsync(d_out, 0, pairs * sizeof(int64_t), cdev.stream));
  EventPair product_time;
  if (int rc = product_time.create()) return rc;
  std::vector<uint32_t> digit_words(batch_tiles * kScoreStepDwords);

  uint64_t batches = 0;
  for (uint64_t b0 = 0; b0 < n_rows; b0 += batch_rows, ++batches) {
    const uint64_t B = std::min(batch_rows, n_rows - b0), steps = (B + kPairTile - 1) / kPairTile;
    // ---- stage 1: every shard turns its genomes' part of the batch around (k_pair_panel)
    for (size_t s = 0; s < pop->shards.size(); ++s) {
      const kgx_pop_shard& sh = pop->shards[s];
      if (sh.n_genomes == 0) continue;
      Device& dev = *sb[s].dev;
      if (int rc = use_device(dev)) return rc;
      const uint32_t chunks = static_cast<uint32_t>((sh.n_genomes + kPairTile - 1) / kPairTile);
      const dim3 grid(static_cast<uint32_t>((batch_tiles + kBlock / kWave - 1) / (kBlock / kWave)), chunks);
      hipLaunchKernelGGL(k_pair_panel, grid, dim3(kBlock), 0, dev.stream, reinterpret_cast<const kgx_v4u*>(sh.d_rows), sh.chunks_per_row, sh.n_genomes,
                         reinterpret_cast<const kgx_v4u*>(sh.d_keep), sb[s].d_list ? sb[s].d_list + b0 : nullptr, b0, B, sb[s].d_panel, panel_pitch);
      KGX_HIP(hipGetLastError());
      if (sb[s].foreign)
        KGX_HIP(hipMemcpyAsync(d_panel + sh.genome_base * panel_pitch, sb[s].d_panel, static_cast<uint64_t>(chunks) * kPairTile * panel_pitch, hipMemcpyDefault,
                               dev.stream));
    }
    for (Device* d : shards.foreign) {
      if (int rc = use_device(*d)) return rc;
      KGX_HIP(hipStreamSynchronize(d->stream));
    }
    // ---- the batch's digit tables, then stage 2: the product, on the first device
    if (int rc = use_device(cdev)) return rc;
    fill_digit_tables(tables, b0, B, digit_words);
    KGX_HIP(hipMemcpyAsync(d_digits, digit_words.data(), steps * step_bytes, hipMemcpyHostToDevice, cdev.stream));
    KGX_HIP(hipStreamSynchronize(cdev.stream));               // pageable source, rewritten for the next batch
    KGX_HIP(hipEventRecord(product_time.begin, cdev.stream));
    const uint64_t z = (steps + steps_per_slice - 1) / steps_per_slice;
    hipLaunchKernelGGL(k_pair_scores, dim3(static_cast<uint32_t>(tile_pairs), 1, static_cast<uint32_t>(z)), dim3(kBlock), 0, cdev.stream, d_panel, panel_pitch,
                       d_digits, d_keep, static_cast<uint32_t>(T), G, static_cast<uint32_t>(steps), static_cast<uint32_t>(steps_per_slice),
                       split ? 2 : (b0 ? 1 : 0), d_out);
    KGX_HIP(hipGetLastError());
    KGX_HIP(hipEventRecord(product_time.end, cdev.stream));
    KGX_HIP(hipStreamSynchronize(cdev.stream));               // the next batch overwrites the panel and the tables
    product_time.collect();
  }
  KGX_HIP(hipMemcpyAsync(out, d_out, pairs * sizeof(int64_t), hipMemcpyDeviceToHost, cdev.stream));
  KGX_HIP(hipStreamSynchronize(cdev.stream));
  g_last_scores_ms = product_time.ms;
  g_last_scores_batches = batches;
  g_last_scores_splits = slices;
  return KGX_OK;
}

// z(d) * 2^s of a used row for d = 0, 1, 2; false = the row is not used.
bool grm_row(const uint32_t* c, double min_maf, double z[3]) {
  const uint64_t called = static_cast<uint64_t>(c[0]) + c[1] + c[2];
  if (called == 0) return false;
  const double p = static_cast<double>(static_cast<uint64_t>(c[1]) + 2ull * c[2]) / static_cast<double>(2 * called);
  const double maf = std::min(p, 1.0 - p);
  if (!(maf > 0.0) || !(maf >= min_maf)) return false;
  const double sd = std::sqrt(2.0 * p * (1.0 - p));
  for (int d = 0; d < 3; ++d) z[d] = (static_cast<double>(d) - 2.0 * p) / sd;
  return true;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" {

int kgx_pair_scores(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, const int16_t* tables, int64_t* out) {
  return guarded([&]() -> int {
    if (int bound = require_bound()) return bound;
    if (!pop || !out) return fail(KGX_EINVAL, "pair_scores: null argument (pop and out are required)");
    if (n_rows > 0xFFFFFFFFull) return fail(KGX_EINVAL, "pair_scores: n_rows %llu is not below 2^32 (the int64 sums)", (unsigned long long)n_rows);
    if (n_rows && !tables) return fail(KGX_EINVAL, "pair_scores: null tables");
    if (!rows && n_rows > pop->n_variants)
      return fail(KGX_EINVAL, "pair_scores: n_rows %llu exceeds the population's %llu rows", (unsigned long long)n_rows, (unsigned long long)pop->n_variants);
    for (uint64_t i = 0; rows && i < n_rows; ++i)
      if (rows[i] >= pop->n_variants)
        return fail(KGX_EINVAL, "pair_scores: rows[%llu] = %u is not a row of the population's %llu", (unsigned long long)i, rows[i],
                    (unsigned long long)pop->n_variants);
    for (uint64_t i = 0; i < n_rows; ++i)
      for (int c = 0; c < 4; ++c)
        if (tables[4 * i + c] > KGX_SCORE_MAX || tables[4 * i + c] < -KGX_SCORE_MAX)
          return fail(KGX_EINVAL, "pair_scores: tables[%llu][%d] = %d is not within +-%d", (unsigned long long)i, c, (int)tables[4 * i + c], KGX_SCORE_MAX);
    g_last_scores_ms = 0.0;
    g_last_scores_batches = 0;
    g_last_scores_splits = 0;
    if (n_rows == 0) {
      std::memset(out, 0, pop->n_genomes * (pop->n_genomes + 1) / 2 * sizeof(int64_t));
      return KGX_OK;
    }
    const int rc = pair_scores_impl(pop, rows, n_rows, tables, out);
    (void)use_device(*pop->shards[0].dev);
    return rc;
  });
}

int kgx_pair_scores_last(double* kernel_ms, uint64_t* row_batches, uint64_t* row_splits) {
  if (kernel_ms) *kernel_ms = g_last_scores_ms.load();
  if (row_batches) *row_batches = g_last_scores_batches.load();
  if (row_splits) *row_splits = g_last_scores_splits.load();
  return KGX_OK;
}

// This translation unit is built with floating contraction off: p, sqrt, the division and the scaling are one IEEE operation each.
int kgx_grm_tables(const uint32_t* row_counts, uint64_t n_rows, double min_maf, int* scale_bits, int16_t* tables, uint64_t* rows_used) {
  return guarded([&]() -> int {
    if (!scale_bits || !rows_used || (n_rows && (!row_counts || !tables))) return fail(KGX_EINVAL, "grm_tables: null argument");
    if (*scale_bits > 12) return fail(KGX_EINVAL, "grm_tables: scale_bits %d is above 12", *scale_bits);
    // the largest |z| and the row that has it decide whether a scale fits
    double largest = 0.0;
    uint64_t largest_row = 0, used = 0;
    for (uint64_t i = 0; i < n_rows; ++i) {
      double z[3];
      if (!grm_row(row_counts + 4 * i, min_maf, z)) continue;
      ++used;
      const double here = std::max(std::fabs(z[0]), std::fabs(z[2]));
      if (here > largest) { largest = here; largest_row = i; }
    }
    auto fits = [&](int s) { return std::llrint(std::ldexp(largest, s)) <= KGX_SCORE_MAX; };
    int s = *scale_bits;
    if (s < 0) {
      s = 12;
      while (s > 0 && !fits(s)) --s;
      if (!fits(s)) return fail(KGX_EINVAL, "grm_tables: row %llu has |z| = %g, beyond %d at any scale", (unsigned long long)largest_row, largest, KGX_SCORE_MAX);
    } else if (!fits(s)) {
      return fail(KGX_EINVAL, "grm_tables: row %llu has |z| = %g, which at scale_bits %d exceeds %d", (unsigned long long)largest_row, largest, s, KGX_SCORE_MAX);
    }
    for (uint64_t i = 0; i < n_rows; ++i) {
      double z[3];
      int16_t* t = tables + 4 * i;
      t[0] = t[1] = t[2] = t[3] = 0;
      if (!grm_row(row_counts + 4 * i, min_maf, z)) continue;
      for (int d = 0; d < 3; ++d) t[d] = static_cast<int16_t>(std::llrint(std::ldexp(z[d], s)));
    }
    *scale_bits = s;
    *rows_used = used;
    return KGX_OK;
  });
}

int kgx_grm_finish(const int64_t* scores, uint64_t n_genomes, int scale_bits, uint64_t rows_used, double* out) {
  return guarded([&]() -> int {
    if (scale_bits < 0 || scale_bits > 12) return fail(KGX_EINVAL, "grm_finish: scale_bits %d is not in 0 .. 12", scale_bits);
    if (n_genomes && (!scores || !out)) return fail(KGX_EINVAL, "grm_finish: null argument");
    if (rows_used > (1ull << 32)) return fail(KGX_EINVAL, "grm_finish: rows_used %llu is above 2^32", (unsigned long long)rows_used);
    const double denominator = static_cast<double>(rows_used << (2 * scale_bits));     // exact: rows_used <= 2^32 times a power of two
    const uint64_t pairs = n_genomes * (n_genomes + 1) / 2;
    for (uint64_t i = 0; i < pairs; ++i)
      out[i] = rows_used == 0 ? std::numeric_limits<double>::quiet_NaN() : static_cast<double>(scores[i]) / denominator;
    return KGX_OK;
  });
}

}  // extern "C"
