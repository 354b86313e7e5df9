// C ABI (include/kgx.h) of the per-genome scores: kgx_genome_scores (per genome and per caller-supplied column of per-row weights
// the sum of the weights over the listed rows of each kind H / M / O: the indicators, transposed in registers straight from the
// shards' rows, times signed base-128 digits of the weights on the matrix cores, kgx_kernels_gscore.h), kgx_genome_scores_last, and
// the host-only companions kgx_score_weights (effect sizes to fixed-point weights) and kgx_score_finish (the dosage score from the
// sums).  No CPU fallback exists for the device part.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

#include "kgx_kernels_gscore.h"
#include "kgx_internal.h"

static_assert(64ull * KGX_GSCORE_ACC_ROWS <= (1ull << 30), "a digit adds at most 64 a row: KGX_GSCORE_ACC_ROWS rows must stay within an int32 accumulator");
static_assert(KGX_GSCORE_ACC_ROWS % kgx::kGscoreSegmentRows == 0, "a slice is whole segments");

namespace kgx {
namespace {

std::atomic<double> g_last_gscore_ms{0.0};
std::atomic<uint64_t> g_last_gscore_batches{0}, g_last_gscore_splits{0};

int genome_scores_impl(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, const int16_t* weights, uint32_t n_columns, const std::vector<uint32_t>& group_first,
                       int64_t* out) {
  const uint32_t n_groups = static_cast<uint32_t>(group_first.size() - 1), n_tiles = group_first.back();
  const uint64_t row_words = static_cast<uint64_t>(n_columns) * kPairKinds;   // of a genome
  const uint64_t list_bytes = rows ? n_rows * sizeof(uint32_t) : 0, weight_bytes = static_cast<uint64_t>(n_columns) * n_rows * sizeof(int16_t);
  const uint64_t plan_bytes = (n_groups + 1ull) * sizeof(uint32_t);
  const uint64_t n_segments = (n_rows + kGscoreSegmentRows - 1) / kGscoreSegmentRows;
  const uint64_t segment_bytes = static_cast<uint64_t>(kGscoreSegment) * n_tiles * kWave * sizeof(kgx_v4u);

  // ---- devices: every shard scores its own genomes on its own device into its own table; shards of one HIP device share the
  // stream, the arena and everything but the table
  struct ShardBuffers { size_t device = 0; long long* d_table = nullptr; uint64_t table_bytes = 0; };
  struct DeviceBuffers { const uint32_t *d_list = nullptr, *d_group_first = nullptr; const int16_t* d_weights = nullptr; kgx_v4u* d_operands = nullptr; uint64_t table_bytes = 0; };
  std::vector<ShardBuffers> sb(pop->shards.size());
  std::vector<Device*> devices;
  for (size_t s = 0; s < pop->shards.size(); ++s) {
    const kgx_pop_shard& sh = pop->shards[s];
    if (sh.n_genomes == 0) continue;
    auto same = std::find_if(devices.begin(), devices.end(), [&](const Device* f) { return f->id == sh.dev->id; });
    sb[s].device = static_cast<size_t>(same - devices.begin());
    if (same == devices.end()) devices.push_back(sh.dev);
    sb[s].table_bytes = sh.n_genomes * row_words * sizeof(int64_t);
  }
  std::vector<DeviceBuffers> db(devices.size());
  std::vector<std::unique_lock<std::mutex>> locks;
  for (Device* d : devices) locks.emplace_back(d->mutex);
  for (size_t s = 0; s < sb.size(); ++s)
    if (sb[s].table_bytes) db[sb[s].device].table_bytes += (sb[s].table_bytes + 255u) & ~255ull;

  // ---- segments per batch: the batch's operands within a quarter of (free + arena) on every device, beside the tables, the list,
  // the weights and the plan; never more rows than one int32 accumulation holds, so that no slice can
  uint64_t batch_segments = std::min<uint64_t>(n_segments, KGX_GSCORE_ACC_ROWS / kGscoreSegmentRows);
  for (size_t k = 0; k < devices.size(); ++k) {
    if (int rc = use_device(*devices[k])) return rc;
    const uint64_t quarter = available_bytes(*devices[k]) / 4, fixed = db[k].table_bytes + list_bytes + weight_bytes + plan_bytes + 1024;
    batch_segments = std::min(batch_segments, (quarter > fixed ? quarter - fixed : 0) / segment_bytes);
  }
  const int row_cap = env_int("KGX_GSCORE_ROWS", 0);
  if (row_cap > 0) batch_segments = std::min(batch_segments, (static_cast<uint64_t>(row_cap) + kGscoreSegmentRows - 1) / kGscoreSegmentRows);
  batch_segments = std::max<uint64_t>(1, batch_segments);
  const int slice_cap = env_int("KGX_GSCORE_SPLITS", 0);      // only ever lowers the count: the tests walk several segments in one workgroup with it

  // ---- buffers; every table is zeroed once, the batches add into it
  std::vector<EventPair> product_time(devices.size());
  for (size_t k = 0; k < devices.size(); ++k) {
    Device& dev = *devices[k];
    if (int rc = use_device(dev)) return rc;
    if (int rc = product_time[k].create()) return rc;
    ScratchPlan plan;
    const size_t o_tables = plan.add(db[k].table_bytes), o_list = plan.add(list_bytes), o_weights = plan.add(weight_bytes), o_plan = plan.add(plan_bytes);
    const size_t o_operands = plan.add(batch_segments * segment_bytes);
    char* arena = nullptr;
    if (int rc = scratch_reserve(dev, plan.total, &arena)) return rc;
    db[k].d_list = rows ? reinterpret_cast<const uint32_t*>(arena + o_list) : nullptr;
    db[k].d_weights = reinterpret_cast<const int16_t*>(arena + o_weights);
    db[k].d_group_first = reinterpret_cast<const uint32_t*>(arena + o_plan);
    db[k].d_operands = reinterpret_cast<kgx_v4u*>(arena + o_operands);
    if (rows) KGX_HIP(hipMemcpyAsync(arena + o_list, rows, list_bytes, hipMemcpyHostToDevice, dev.stream));
    KGX_HIP(hipMemcpyAsync(arena + o_weights, weights, weight_bytes, hipMemcpyHostToDevice, dev.stream));
    KGX_HIP(hipMemcpyAsync(arena + o_plan, group_first.data(), plan_bytes, hipMemcpyHostToDevice, dev.stream));
    KGX_HIP(hipStreamSynchronize(dev.stream));                 // the sources are pageable host memory
    size_t at = o_tables;
    for (size_t s = 0; s < sb.size(); ++s) {
      if (sb[s].table_bytes == 0 || sb[s].device != k) continue;
      sb[s].d_table = reinterpret_cast<long long*>(arena + at);
      at += (sb[s].table_bytes + 255u) & ~static_cast<size_t>(255u);
    }
    const uint64_t words = db[k].table_bytes / sizeof(int64_t);
    hipLaunchKernelGGL(k_gscore_clear, dim3(stream_grid(dev, words, kBlock)), dim3(kBlock), 0, dev.stream, reinterpret_cast<long long*>(arena + o_tables), words);
    KGX_HIP(hipGetLastError());
  }

  // ---- the batches: the operands of the batch's weights once per device, then every shard's product; the list is split over
  // gridDim.z where (genome blocks x groups) alone is below two workgroups a compute unit
  uint64_t batches = 0, widest = 1;
  for (uint64_t segment0 = 0; segment0 < n_segments; segment0 += batch_segments, ++batches) {
    const uint32_t segments = static_cast<uint32_t>(std::min(batch_segments, n_segments - segment0));
    const uint64_t batch_first = segment0 * kGscoreSegmentRows, units = static_cast<uint64_t>(segments) * kGscoreSegment * n_groups * kGscoreDigits * kWave;
    for (size_t k = 0; k < devices.size(); ++k) {
      Device& dev = *devices[k];
      if (int rc = use_device(dev)) return rc;
      hipLaunchKernelGGL(k_weight_operands, dim3(stream_grid(dev, units, kBlock)), dim3(kBlock), 0, dev.stream, db[k].d_weights, n_rows, n_columns, batch_first,
                         db[k].d_group_first, n_groups, n_tiles, units, db[k].d_operands);
      KGX_HIP(hipGetLastError());
      KGX_HIP(hipEventRecord(product_time[k].begin, dev.stream));
      for (size_t s = 0; s < sb.size(); ++s) {
        const kgx_pop_shard& sh = pop->shards[s];
        if (sb[s].table_bytes == 0 || sb[s].device != k) continue;
        const uint64_t blocks = (sh.n_genomes + kGscoreGenomes - 1) / kGscoreGenomes, work = blocks * n_groups;
        const uint64_t wanted = 2ull * static_cast<uint64_t>(std::max(dev.compute_units, 1));
        uint64_t slices = work < wanted ? std::min<uint64_t>({(wanted + work - 1) / work, segments, 65535}) : 1;
        if (slice_cap > 0) slices = std::min(slices, static_cast<uint64_t>(slice_cap));
        const uint32_t per_slice = static_cast<uint32_t>((segments + slices - 1) / slices), z = (segments + per_slice - 1) / per_slice;
        widest = std::max<uint64_t>(widest, z);
        hipLaunchKernelGGL(k_genome_scores, dim3(static_cast<uint32_t>(blocks), n_groups, z), dim3(kBlock), 0, dev.stream, reinterpret_cast<const kgx_v4u*>(sh.d_rows),
                           sh.chunks_per_row, sh.n_genomes, reinterpret_cast<const kgx_v4u*>(sh.d_keep), db[k].d_list, n_rows, batch_first, db[k].d_operands,
                           db[k].d_group_first, n_tiles, n_columns, segments, per_slice, z > 1 ? 1 : 0, sb[s].d_table);
        KGX_HIP(hipGetLastError());
      }
      KGX_HIP(hipEventRecord(product_time[k].end, dev.stream));
    }
    for (size_t k = 0; k < devices.size(); ++k) {               // the next batch overwrites the operands and records the events again
      if (int rc = use_device(*devices[k])) return rc;
      KGX_HIP(hipStreamSynchronize(devices[k]->stream));
      product_time[k].collect();
    }
  }

  // ---- every shard's table to the host at its first genome
  for (size_t s = 0; s < sb.size(); ++s) {
    if (sb[s].table_bytes == 0) continue;
    Device& dev = *devices[sb[s].device];
    if (int rc = use_device(dev)) return rc;
    KGX_HIP(hipMemcpyAsync(out + pop->shards[s].genome_base * row_words, sb[s].d_table, sb[s].table_bytes, hipMemcpyDeviceToHost, dev.stream));
  }
  double slowest = 0.0;
  for (size_t k = 0; k < devices.size(); ++k) {
    if (int rc = use_device(*devices[k])) return rc;
    KGX_HIP(hipStreamSynchronize(devices[k]->stream));
    slowest = std::max(slowest, product_time[k].ms);
  }
  g_last_gscore_ms = slowest;
  g_last_gscore_batches = batches;
  g_last_gscore_splits = widest;
  return KGX_OK;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" {

int kgx_genome_scores(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, const int16_t* weights, uint32_t n_columns, int64_t* out) {
  return guarded([&]() -> int {
    if (int bound = require_bound()) return bound;
    if (!pop || !out || (n_rows && !weights)) return fail(KGX_EINVAL, "genome_scores: null argument (pop and out are required, weights with n_rows > 0)");
    if (n_rows && n_columns == 0) return fail(KGX_EINVAL, "genome_scores: no columns");
    if (n_rows >= (1ull << 32)) return fail(KGX_EINVAL, "genome_scores: n_rows %llu is not below 2^32", (unsigned long long)n_rows);
    uint64_t bytes = 0, weight_bytes = 0;                      // before the list is walked: a size that overflows is no list's
    if (__builtin_mul_overflow(pop->n_genomes, static_cast<uint64_t>(n_columns) * kPairKinds * sizeof(int64_t), &bytes) ||
        __builtin_mul_overflow(n_rows, static_cast<uint64_t>(n_columns) * sizeof(int16_t), &weight_bytes))
      return fail(KGX_EINVAL, "genome_scores: the tables of %llu genomes and %llu rows x %u columns overflow 64 bits", (unsigned long long)pop->n_genomes,
                  (unsigned long long)n_rows, n_columns);
    if (!rows && n_rows > pop->n_variants)
      return fail(KGX_EINVAL, "genome_scores: n_rows %llu exceeds the population's %llu rows", (unsigned long long)n_rows, (unsigned long long)pop->n_variants);
    for (uint64_t i = 0; rows && i < n_rows; ++i)
      if (rows[i] >= pop->n_variants)
        return fail(KGX_EINVAL, "genome_scores: rows[%llu] = %u is not a row of the population's %llu", (unsigned long long)i, rows[i],
                    (unsigned long long)pop->n_variants);
    g_last_gscore_ms = 0.0;
    g_last_gscore_batches = 0;
    g_last_gscore_splits = 0;
    // the weights' range, and the groups' digits on the way: one where every value of the group lies in [-64, 63]
    const uint64_t n_groups = n_rows ? (static_cast<uint64_t>(n_columns) + 15) / 16 : 0;
    if (n_groups > 65535) return fail(KGX_EINVAL, "genome_scores: %u columns make %llu groups, more than a grid holds", n_columns, (unsigned long long)n_groups);
    std::vector<uint32_t> group_first(1, 0u);
    for (uint64_t group = 0; group < n_groups; ++group) {
      bool one = true;
      const uint64_t j_end = std::min<uint64_t>(group * 16 + 16, n_columns);
      for (uint64_t j = group * 16; j < j_end; ++j)
        for (uint64_t i = 0; i < n_rows; ++i) {
          const int32_t w = weights[j * n_rows + i];
          if (w > KGX_SCORE_MAX || w < -KGX_SCORE_MAX)
            return fail(KGX_EINVAL, "genome_scores: weights[%llu][%llu] = %d is not within +-%d", (unsigned long long)j, (unsigned long long)i, w, KGX_SCORE_MAX);
          one = one && w >= -64 && w <= 63;
        }
      group_first.push_back(group_first.back() + (one ? 1u : kGscoreDigits));
    }
    bool any = false;
    for (const auto& sh : pop->shards) any = any || sh.n_genomes != 0;
    if (n_rows == 0 || !any) {
      std::memset(out, 0, bytes);
      return KGX_OK;
    }
    const int rc = genome_scores_impl(pop, rows, n_rows, weights, n_columns, group_first, out);
    (void)use_device(*pop->shards[0].dev);
    return rc;
  });
}

int kgx_genome_scores_last(double* kernel_ms, uint64_t* row_batches, uint64_t* row_splits) {
  if (kernel_ms) *kernel_ms = g_last_gscore_ms.load();
  if (row_batches) *row_batches = g_last_gscore_batches.load();
  if (row_splits) *row_splits = g_last_gscore_splits.load();
  return KGX_OK;
}

// This translation unit is built with floating contraction off: x = beta, or (c1 + 2 c2) / called * beta -- one division and one
// multiplication --, then an exact scaling, and llrint rounds to nearest even.
int kgx_score_weights(const double* beta, const uint32_t* row_counts, uint64_t n_rows, uint32_t n_scores, int* scale_bits, int16_t* weights) {
  return guarded([&]() -> int {
    const uint64_t n = static_cast<uint64_t>(n_scores) * n_rows;
    if (!scale_bits || (n && (!beta || !weights))) return fail(KGX_EINVAL, "score_weights: null argument");
    if (*scale_bits > 12) return fail(KGX_EINVAL, "score_weights: scale_bits %d is above 12", *scale_bits);
    auto twice_p = [&](uint64_t i) {                           // 2 p of the row: the mean dosage of its called genomes (none: 0)
      const uint32_t* c = row_counts + 4 * i;
      const uint64_t called = static_cast<uint64_t>(c[0]) + c[1] + c[2];
      return called ? static_cast<double>(static_cast<uint64_t>(c[1]) + 2ull * c[2]) / static_cast<double>(called) : 0.0;
    };
    // the largest |x| decides whether a scale fits: rounding is monotonic
    double largest = 0.0;
    uint64_t largest_at = 0;
    for (uint64_t at = 0; at < n; ++at) {
      if (!std::isfinite(beta[at]))
        return fail(KGX_EINVAL, "score_weights: beta[%llu][%llu] is not finite", (unsigned long long)(at / n_rows), (unsigned long long)(at % n_rows));
      const double x = std::max(std::fabs(beta[at]), row_counts ? std::fabs(twice_p(at % n_rows) * beta[at]) : 0.0);
      if (x > largest) { largest = x; largest_at = at; }
    }
    auto fits = [&](int s) {
      const double scaled = std::ldexp(largest, s);
      return scaled < 8129.0 && std::llrint(scaled) <= KGX_SCORE_MAX;
    };
    int s = *scale_bits;
    if (s < 0) {
      s = 12;
      while (s > 0 && !fits(s)) --s;
    }
    if (!fits(s))
      return fail(KGX_EINVAL, "score_weights: beta[%llu][%llu] = %g at scale_bits %d exceeds %d", (unsigned long long)(n_rows ? largest_at / n_rows : 0),
                  (unsigned long long)(n_rows ? largest_at % n_rows : 0), beta[largest_at], s, KGX_SCORE_MAX);
    for (uint64_t at = 0; at < n; ++at) {
      weights[at] = static_cast<int16_t>(std::llrint(std::ldexp(beta[at], s)));
      if (row_counts) weights[n + at] = static_cast<int16_t>(std::llrint(std::ldexp(twice_p(at % n_rows) * beta[at], s)));
    }
    *scale_bits = s;
    return KGX_OK;
  });
}

// One conversion and one exact scaling: |S_H + 2 S_M + S_O| < 2^32 * 3 * 8128 is far inside an int64.
int kgx_score_finish(const int64_t* sums, uint64_t n_genomes, uint32_t n_scores, int imputed, int scale_bits, double* out) {
  return guarded([&]() -> int {
    if (scale_bits < 0 || scale_bits > 12) return fail(KGX_EINVAL, "score_finish: scale_bits %d is not in 0 .. 12", scale_bits);
    if (n_genomes && n_scores && (!sums || !out)) return fail(KGX_EINVAL, "score_finish: null argument");
    const uint64_t columns = static_cast<uint64_t>(n_scores) * (imputed ? 2 : 1);
    for (uint64_t g = 0; g < n_genomes; ++g)
      for (uint64_t j = 0; j < n_scores; ++j) {
        const int64_t* q = sums + (g * columns + j) * kPairKinds;             // {H, M, O} of q; of m, n_scores columns on
        const int64_t score = q[0] + 2 * q[1] + (imputed ? q[n_scores * kPairKinds + 2] : 0);
        out[g * n_scores + j] = std::ldexp(static_cast<double>(score), -scale_bits);
      }
    return KGX_OK;
  });
}

}  // extern "C"
