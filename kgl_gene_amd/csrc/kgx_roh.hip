// C ABI (include/kgx.h) of the runs of homozygosity: kgx_roh (per genome the unbroken stretches of called homozygous sites along a
// row list, their summary and optionally the runs themselves; the walk and its stitch are kgx_kernels_roh.h), kgx_roh_last and
// kgx_roh_coefficients (F_ROH from the summaries, host only).  No CPU fallback exists for the device part.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <deque>
#include <limits>
#include <mutex>
#include <vector>

#include "kgx_kernels_roh.h"
#include "kgx_internal.h"

namespace kgx {
namespace {

static_assert(sizeof(kgx_roh_summary) == 4 * sizeof(unsigned long long), "k_roh_stitch writes the summary as four 64-bit words");

std::atomic<double> g_last_roh_ms{0.0};
std::atomic<uint64_t> g_last_roh_slices{0};

// One shard's part of its device's arena.
struct ShardPlan {
  uint64_t genomes_padded = 0, slices = 0, rows_per_slice = 0;
  size_t o_records = 0, o_counts = 0, o_cursors = 0, o_summary = 0, o_totals = 0, o_begin = 0, o_segments = 0;
  std::vector<unsigned long long> begin;     // the shard's own begin[], starting at 0
  uint64_t entries() const { return begin.empty() ? 0 : begin.back(); }
};

// The shards of one HIP device share its first slot's stream and arena (a device may be bound more than once).
struct DeviceGroup {
  Device* dev = nullptr;
  std::vector<size_t> shards;
  hipEvent_t count_begin = nullptr, count_end = nullptr;
  size_t o_breaks = 0, o_list = 0, o_position = 0;
  char* arena = nullptr;
  DeviceGroup() = default;
  DeviceGroup(const DeviceGroup&) = delete;
  ~DeviceGroup() {
    if (count_begin) (void)hipEventDestroy(count_begin);
    if (count_end) (void)hipEventDestroy(count_end);
  }
};

struct RohCall {
  kgx_pop* pop;
  const uint32_t *rows, *position;
  uint64_t n_rows;
  const std::vector<unsigned long long>& breaks;
  uint32_t min_sites, min_length;
  std::vector<ShardPlan> plans;
};

uint32_t column_blocks(const kgx_pop_shard& sh) {
  const uint32_t column_waves = (sh.chunks_per_row + kRohChunks - 1) / kRohChunks;
  return (column_waves + (kBlock / kWave) - 1) / (kBlock / kWave);
}

// How the shards of a device cut the list: enough (column waves x slices) for two waves on every SIMD, whole 64-position tiles, the
// records of the device's shards within a quarter of (free + arena).
int plan_slices(RohCall& call, DeviceGroup& group) {
  if (int rc = use_device(*group.dev)) return rc;
  size_t free_bytes = 0, total_bytes = 0;
  if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) { (void)hipGetLastError(); free_bytes = 0; }
  uint64_t cells = 0;
  for (size_t s : group.shards) {
    const kgx_pop_shard& sh = call.pop->shards[s];
    call.plans[s].genomes_padded = (static_cast<uint64_t>(sh.chunks_per_row) + kRohChunks - 1) / kRohChunks * kRohChunks * 64u;
    cells += call.plans[s].genomes_padded;
  }
  const uint64_t fitting = (static_cast<uint64_t>(free_bytes) + group.dev->scratch_bytes) / 4 / (kRohBytesPerCell * cells);
  const uint64_t tiles = (call.n_rows + kWave - 1) / kWave;
  const int cap = env_int("KGX_ROH_SLICES", 0);              // only ever lowers the count: the tests walk several tiles a slice with it
  for (size_t s : group.shards) {
    const kgx_pop_shard& sh = call.pop->shards[s];
    const uint64_t column_waves = (sh.chunks_per_row + kRohChunks - 1) / kRohChunks;
    const uint64_t wanted = 2ull * 4ull * static_cast<uint64_t>(std::max(group.dev->compute_units, 1));   // four SIMDs a compute unit
    uint64_t slices = std::min<uint64_t>({(wanted + column_waves - 1) / column_waves, tiles, 65535, std::max<uint64_t>(fitting, 1)});
    if (cap > 0) slices = std::min(slices, static_cast<uint64_t>(cap));
    ShardPlan& plan = call.plans[s];
    plan.rows_per_slice = (tiles + slices - 1) / slices * kWave;
    plan.slices = (call.n_rows + plan.rows_per_slice - 1) / plan.rows_per_slice;
  }
  return KGX_OK;
}

// Reserve the device's arena (with room for every shard's runs behind its buffers where asked), upload the list's tables and queue
// the count pass of every shard of the device: k_roh<false>, bracketed by the events, then the stitch and the scan.
int queue_count_pass(RohCall& call, DeviceGroup& group, bool with_segments) {
  Device& dev = *group.dev;
  if (int rc = use_device(dev)) return rc;
  const uint64_t n_rows = call.n_rows;
  const size_t list_bytes = call.rows ? n_rows * sizeof(uint32_t) : 0;
  ScratchPlan layout;
  group.o_breaks = layout.add(call.breaks.size() * sizeof(unsigned long long));
  group.o_list = layout.add(list_bytes);
  group.o_position = layout.add(n_rows * sizeof(uint32_t));
  for (size_t s : group.shards) {
    const kgx_pop_shard& sh = call.pop->shards[s];
    ShardPlan& plan = call.plans[s];
    const uint64_t cells = plan.slices * plan.genomes_padded;
    plan.o_records = layout.add(cells * kRohPlanes * sizeof(kgx_v4u));
    plan.o_counts = layout.add(cells * sizeof(uint32_t));
    plan.o_cursors = layout.add(cells * sizeof(unsigned long long));
    plan.o_summary = layout.add(sh.n_genomes * sizeof(kgx_roh_summary));
    plan.o_totals = layout.add(sh.n_genomes * sizeof(unsigned long long));
    plan.o_begin = layout.add((sh.n_genomes + 1) * sizeof(unsigned long long));
    plan.o_segments = layout.add(with_segments ? plan.entries() * 3 * sizeof(uint32_t) : 0);
  }
  if (int rc = scratch_reserve(dev, layout.total, &group.arena)) return rc;
  char* arena = group.arena;
  KGX_HIP(hipMemcpyAsync(arena + group.o_breaks, call.breaks.data(), call.breaks.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, dev.stream));
  if (call.rows) KGX_HIP(hipMemcpyAsync(arena + group.o_list, call.rows, list_bytes, hipMemcpyHostToDevice, dev.stream));
  KGX_HIP(hipMemcpyAsync(arena + group.o_position, call.position, n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, dev.stream));
  KGX_HIP(hipStreamSynchronize(dev.stream));                  // the sources are pageable host memory
  const uint32_t* d_list = call.rows ? reinterpret_cast<const uint32_t*>(arena + group.o_list) : nullptr;
  const uint32_t* d_position = reinterpret_cast<const uint32_t*>(arena + group.o_position);
  const unsigned long long* d_breaks = reinterpret_cast<const unsigned long long*>(arena + group.o_breaks);

  KGX_HIP(hipEventRecord(group.count_begin, dev.stream));
  for (size_t s : group.shards) {
    const kgx_pop_shard& sh = call.pop->shards[s];
    const ShardPlan& plan = call.plans[s];
    hipLaunchKernelGGL((k_roh<false>), dim3(column_blocks(sh), static_cast<uint32_t>(plan.slices)), dim3(kBlock), 0, dev.stream,
                       reinterpret_cast<const kgx_v4u*>(sh.d_rows), sh.chunks_per_row, sh.n_genomes, reinterpret_cast<const kgx_v4u*>(sh.d_keep), d_list, n_rows,
                       d_position, d_breaks, plan.rows_per_slice, call.min_sites, call.min_length, reinterpret_cast<kgx_v4u*>(arena + plan.o_records),
                       plan.genomes_padded, nullptr, nullptr);
    KGX_HIP(hipGetLastError());
  }
  KGX_HIP(hipEventRecord(group.count_end, dev.stream));
  for (size_t s : group.shards) {
    const kgx_pop_shard& sh = call.pop->shards[s];
    const ShardPlan& plan = call.plans[s];
    const uint32_t by_genome = static_cast<uint32_t>((sh.n_genomes + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((k_roh_stitch<false>), dim3(by_genome), dim3(kBlock), 0, dev.stream, reinterpret_cast<const kgx_v4u*>(arena + plan.o_records),
                       plan.slices, plan.genomes_padded, sh.n_genomes, d_position, call.min_sites, call.min_length,
                       reinterpret_cast<uint32_t*>(arena + plan.o_counts), reinterpret_cast<unsigned long long*>(arena + plan.o_summary),
                       reinterpret_cast<unsigned long long*>(arena + plan.o_totals), nullptr, nullptr, nullptr);
    KGX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_roh_scan, dim3(1), dim3(kBlock), 0, dev.stream, reinterpret_cast<const unsigned long long*>(arena + plan.o_totals), sh.n_genomes,
                       reinterpret_cast<unsigned long long*>(arena + plan.o_begin));
    KGX_HIP(hipGetLastError());
  }
  return KGX_OK;
}

// The summaries to the caller (the shards' genomes are contiguous: concatenated in genome order) and every shard's begin[].
int collect_counts(RohCall& call, DeviceGroup& group, kgx_roh_summary* summary) {
  Device& dev = *group.dev;
  if (int rc = use_device(dev)) return rc;
  for (size_t s : group.shards) {
    const kgx_pop_shard& sh = call.pop->shards[s];
    ShardPlan& plan = call.plans[s];
    plan.begin.assign(sh.n_genomes + 1, 0);
    KGX_HIP(hipMemcpyAsync(summary + sh.genome_base, group.arena + plan.o_summary, sh.n_genomes * sizeof(kgx_roh_summary), hipMemcpyDeviceToHost, dev.stream));
    KGX_HIP(hipMemcpyAsync(plan.begin.data(), group.arena + plan.o_begin, (sh.n_genomes + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, dev.stream));
  }
  KGX_HIP(hipStreamSynchronize(dev.stream));
  return KGX_OK;
}

int roh_impl(RohCall& call, kgx_roh_summary* summary, uint64_t* begin, uint32_t* segments, uint64_t capacity) {
  kgx_pop* pop = call.pop;
  // ---- devices, in the order of their first shard
  std::deque<DeviceGroup> groups;
  for (size_t s = 0; s < pop->shards.size(); ++s) {
    if (pop->shards[s].n_genomes == 0) continue;
    Device* d = pop->shards[s].dev;
    auto same = std::find_if(groups.begin(), groups.end(), [&](const DeviceGroup& g) { return g.dev->id == d->id; });
    if (same == groups.end()) {
      groups.emplace_back();
      groups.back().dev = d;
      same = groups.end() - 1;
    }
    same->shards.push_back(s);
  }
  if (groups.empty()) return KGX_OK;                          // no genome anywhere: the zeros the caller already has
  std::vector<std::unique_lock<std::mutex>> locks;
  for (DeviceGroup& g : groups) locks.emplace_back(g.dev->mutex);
  call.plans.assign(pop->shards.size(), ShardPlan());

  // ---- the count pass: every device at the same time, no exchange
  for (DeviceGroup& g : groups) {
    if (int rc = plan_slices(call, g)) return rc;
    KGX_HIP(hipEventCreate(&g.count_begin));
    KGX_HIP(hipEventCreate(&g.count_end));
    if (int rc = queue_count_pass(call, g, false)) return rc;
  }
  double slowest = 0.0;
  for (DeviceGroup& g : groups) {
    if (int rc = collect_counts(call, g, summary)) return rc;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g.count_begin, g.count_end) == hipSuccess) slowest = std::max(slowest, static_cast<double>(ms));
    else (void)hipGetLastError();
  }
  g_last_roh_ms = slowest;
  g_last_roh_slices = call.plans[groups[0].shards[0]].slices;
  if (!begin) return KGX_OK;

  // ---- begin[]: the shards' own, offset on the host
  uint64_t needed = 0;
  for (size_t s = 0; s < pop->shards.size(); ++s) {
    const kgx_pop_shard& sh = pop->shards[s];
    if (sh.n_genomes == 0) continue;
    for (uint64_t g = 0; g < sh.n_genomes; ++g) begin[sh.genome_base + g] = needed + call.plans[s].begin[g];
    needed += call.plans[s].entries();
  }
  begin[pop->n_genomes] = needed;
  if (!segments) return KGX_OK;
  if (capacity < needed)
    return fail(KGX_EINVAL, "roh: capacity %llu is below the %llu runs to write", (unsigned long long)capacity, (unsigned long long)needed);

  // ---- the fill pass: the stitched runs and the cursors, then the same walk again
  for (DeviceGroup& g : groups) {
    Device& dev = *g.dev;
    uint64_t entries = 0, room = 0;
    for (size_t s : g.shards) {
      entries += call.plans[s].entries();
      room += (call.plans[s].entries() * 3 * sizeof(uint32_t) + 255u) & ~static_cast<uint64_t>(255u);
    }
    if (entries == 0) continue;
    // the arena is laid out with the segments last: where they fit behind the count pass's buffers nothing moves; where the arena has
    // to grow, its contents go and the count pass runs once more
    const size_t without = call.plans[g.shards.back()].o_segments;
    const bool regrow = without + room > dev.scratch_bytes;
    if (int rc = regrow ? queue_count_pass(call, g, true) : use_device(dev)) return rc;
    if (!regrow) {
      size_t at = without;
      for (size_t s : g.shards) {
        call.plans[s].o_segments = at;
        at += (call.plans[s].entries() * 3 * sizeof(uint32_t) + 255u) & ~static_cast<size_t>(255u);
      }
    }
    char* arena = g.arena;
    const uint32_t* d_list = call.rows ? reinterpret_cast<const uint32_t*>(arena + g.o_list) : nullptr;
    const uint32_t* d_position = reinterpret_cast<const uint32_t*>(arena + g.o_position);
    for (size_t s : g.shards) {
      const kgx_pop_shard& sh = pop->shards[s];
      const ShardPlan& plan = call.plans[s];
      if (plan.entries() == 0) continue;
      uint32_t* d_segments = reinterpret_cast<uint32_t*>(arena + plan.o_segments);
      const uint32_t by_genome = static_cast<uint32_t>((sh.n_genomes + kBlock - 1) / kBlock);
      hipLaunchKernelGGL((k_roh_stitch<true>), dim3(by_genome), dim3(kBlock), 0, dev.stream, reinterpret_cast<const kgx_v4u*>(arena + plan.o_records),
                         plan.slices, plan.genomes_padded, sh.n_genomes, d_position, call.min_sites, call.min_length,
                         reinterpret_cast<uint32_t*>(arena + plan.o_counts), nullptr, nullptr, reinterpret_cast<const unsigned long long*>(arena + plan.o_begin),
                         reinterpret_cast<unsigned long long*>(arena + plan.o_cursors), d_segments);
      KGX_HIP(hipGetLastError());
      hipLaunchKernelGGL((k_roh<true>), dim3(column_blocks(sh), static_cast<uint32_t>(plan.slices)), dim3(kBlock), 0, dev.stream,
                         reinterpret_cast<const kgx_v4u*>(sh.d_rows), sh.chunks_per_row, sh.n_genomes, reinterpret_cast<const kgx_v4u*>(sh.d_keep), d_list,
                         call.n_rows, d_position, reinterpret_cast<const unsigned long long*>(arena + g.o_breaks), plan.rows_per_slice, call.min_sites,
                         call.min_length, nullptr, plan.genomes_padded, reinterpret_cast<const unsigned long long*>(arena + plan.o_cursors), d_segments);
      KGX_HIP(hipGetLastError());
    }
  }
  for (DeviceGroup& g : groups) {
    if (int rc = use_device(*g.dev)) return rc;
    for (size_t s : g.shards) {
      const ShardPlan& plan = call.plans[s];
      if (plan.entries() == 0) continue;
      KGX_HIP(hipMemcpyAsync(segments + 3 * begin[pop->shards[s].genome_base], g.arena + plan.o_segments, plan.entries() * 3 * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, g.dev->stream));
    }
    KGX_HIP(hipStreamSynchronize(g.dev->stream));
  }
  return KGX_OK;
}

}  // namespace

int run_breaks(const char* who, const kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, const uint32_t* position, const uint8_t* contig_start,
               uint32_t max_gap, std::vector<unsigned long long>& breaks) {
  breaks.assign((n_rows + 63) / 64, 0ull);
  for (uint64_t i = 0; i < n_rows; ++i) {
    if (rows && rows[i] >= pop->n_variants)
      return fail(KGX_EINVAL, "%s: rows[%llu] = %u is not a row of the population's %llu", who, (unsigned long long)i, rows[i], (unsigned long long)pop->n_variants);
    if (i == 0) continue;                                     // position 0 begins the first contig: no break before it
    const bool contig = contig_start && contig_start[i] != 0;
    if (!contig && position[i] < position[i - 1])
      return fail(KGX_EINVAL, "%s: position[%llu] = %u is below position[%llu] = %u without a contig start", who, (unsigned long long)i, position[i],
                  (unsigned long long)(i - 1), position[i - 1]);
    if (contig || (max_gap != 0 && position[i] - position[i - 1] > max_gap)) breaks[i >> 6] |= 1ull << (i & 63);
  }
  return KGX_OK;
}

}  // namespace kgx

using namespace kgx;

extern "C" {

int kgx_roh(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, const uint32_t* position, const uint8_t* contig_start, const kgx_roh_params* params,
            kgx_roh_summary* summary, uint64_t* begin, uint32_t* segments, uint64_t capacity) {
  return guarded([&]() -> int {
    if (int bound = require_bound()) return bound;
    if (!pop) return fail(KGX_EINVAL, "roh: null argument (pop is required)");
    if (n_rows && (!position || !summary)) return fail(KGX_EINVAL, "roh: null argument (position and summary are required)");
    if (segments && !begin) return fail(KGX_EINVAL, "roh: segments without begin");
    if (n_rows >= (1ull << 32)) return fail(KGX_EINVAL, "roh: n_rows %llu exceeds the 32-bit list positions of the runs", (unsigned long long)n_rows);
    if (!rows && n_rows > pop->n_variants)
      return fail(KGX_EINVAL, "roh: n_rows %llu exceeds the population's %llu rows", (unsigned long long)n_rows, (unsigned long long)pop->n_variants);
    std::vector<unsigned long long> breaks;
    if (int rc = run_breaks("roh", pop, rows, n_rows, position, contig_start, params ? params->max_gap : 0, breaks)) return rc;
    g_last_roh_ms = 0.0;
    g_last_roh_slices = 0;
    if (summary) std::memset(summary, 0, pop->n_genomes * sizeof(kgx_roh_summary));
    if (begin) std::memset(begin, 0, (pop->n_genomes + 1) * sizeof(uint64_t));
    if (n_rows == 0) return KGX_OK;
    RohCall call{pop, rows, position, n_rows, breaks, params && params->min_sites ? params->min_sites : 1u, params && params->min_length ? params->min_length : 1u, {}};
    const int rc = roh_impl(call, summary, begin, segments, capacity);
    (void)use_device(*pop->shards[0].dev);
    return rc;
  });
}

int kgx_roh_last(double* kernel_ms, uint64_t* row_slices) {
  if (kernel_ms) *kernel_ms = g_last_roh_ms.load();
  if (row_slices) *row_slices = g_last_roh_slices.load();
  return KGX_OK;
}

// Each value is one conversion of each integer and ONE division.
int kgx_roh_coefficients(const kgx_roh_summary* summary, uint64_t n_genomes, uint64_t denominator, double* out) {
  return guarded([&]() -> int {
    if (n_genomes && (!summary || !out)) return fail(KGX_EINVAL, "roh_coefficients: null argument");
    for (uint64_t g = 0; g < n_genomes; ++g)
      out[g] = denominator ? static_cast<double>(summary[g].total_length) / static_cast<double>(denominator) : std::numeric_limits<double>::quiet_NaN();
    return KGX_OK;
  });
}

}  // extern "C"
