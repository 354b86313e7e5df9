// C ABI (include/kgx.h) of the shared runs between genome pairs: kgx_pair_runs (per unordered genome pair the summary of the
// unbroken stretches of listed rows without a mismatch: kgx_pair_counts' genome-major panel per row batch, then the walk of
// kgx_kernels_pair_runs.h), kgx_pair_runs_last and kgx_pair_run_fractions (host only).  No CPU fallback exists for the device part.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

#include "kgx_kernels_panel.h"
#include "kgx_kernels_pair_runs.h"
#include "kgx_internal.h"

namespace kgx {
namespace {

static_assert(sizeof(kgx_roh_summary) == 4 * sizeof(unsigned long long), "k_pair_runs writes the summary as four 64-bit words");

std::atomic<double> g_last_pair_runs_ms{0.0};
std::atomic<uint64_t> g_last_pair_runs_batches{0};

struct PairRunsCall {
  kgx_pop* pop;
  const uint32_t *rows, *position;
  uint64_t n_rows;
  const std::vector<unsigned long long>& breaks;
  uint32_t min_sites, min_length, mode;
};

int pair_runs_impl(const PairRunsCall& call, kgx_roh_summary* out) {
  kgx_pop* pop = call.pop;
  const uint64_t n_rows = call.n_rows, G = pop->n_genomes, padded = (G + kPairTile - 1) / kPairTile * kPairTile, T = (G + kRunTile - 1) / kRunTile;
  const uint64_t pairs = G * (G + 1) / 2, list_bytes = call.rows ? n_rows * sizeof(uint32_t) : 0;
  for (const auto& sh : pop->shards)
    if (sh.n_genomes && sh.genome_base % kPairTile) return fail(KGX_ESTATE, "pair_runs: a shard does not start at a whole 64-genome tile");

  // ---- devices: the walk runs on the first shard's; shards on the same HIP device share its stream and arena
  Device& cdev = *pop->shards[0].dev;
  struct ShardBuffers { Device* dev = nullptr; bool foreign = false; const uint32_t* d_list = nullptr; uint8_t* d_panel = nullptr; };
  std::vector<ShardBuffers> sb(pop->shards.size());
  std::vector<Device*> foreign;
  for (size_t s = 0; s < pop->shards.size(); ++s) {
    Device* d = pop->shards[s].dev;
    sb[s].foreign = d->id != cdev.id;
    sb[s].dev = sb[s].foreign ? d : &cdev;
    if (sb[s].foreign && pop->shards[s].n_genomes && std::find(foreign.begin(), foreign.end(), d) == foreign.end()) foreign.push_back(d);
  }
  std::vector<std::unique_lock<std::mutex>> locks;
  locks.emplace_back(cdev.mutex);
  for (Device* d : foreign) locks.emplace_back(d->mutex);

  // ---- rows per batch, in whole 64-row tiles: the panel within a quarter of (free + arena) on every device; the pairs' table
  //      (summary and open run), the list's tables and the keep bytes beside it on the first
  if (int rc = use_device(cdev)) return rc;
  const uint64_t tiles = (n_rows + kPairTile - 1) / kPairTile, table_bytes = pairs * (sizeof(kgx_roh_summary) + sizeof(kgx_v4u));
  const uint64_t available = available_bytes(cdev), fixed = table_bytes + list_bytes + n_rows * sizeof(uint32_t) + tiles * 8 + T * kRunTile + 7 * 256;
  if (fixed + padded * 16 > available)
    return fail(KGX_ENOMEM, "pair_runs: the %llu-byte table of %llu genomes' pairs does not fit beside one 64-row panel into the %llu bytes free on the first device",
                (unsigned long long)table_bytes, (unsigned long long)G, (unsigned long long)available);
  uint64_t batch_tiles = std::min(available / 4, available - fixed) / (padded * 16);
  for (size_t s = 0; s < pop->shards.size(); ++s) {
    if (!sb[s].foreign || pop->shards[s].n_genomes == 0) continue;
    if (int rc = use_device(*sb[s].dev)) return rc;
    const uint64_t shard_padded = (pop->shards[s].n_genomes + kPairTile - 1) / kPairTile * kPairTile, there = available_bytes(*sb[s].dev);
    batch_tiles = std::min(batch_tiles, (there / 4 > list_bytes ? there / 4 - list_bytes : 0) / (shard_padded * 16));
  }
  batch_tiles = std::max<uint64_t>(1, std::min(batch_tiles, tiles));
  const int cap = env_int("KGX_PAIR_RUNS_ROWS", 0);           // only ever lowers the count: the tests carry open runs over batch edges with it
  if (cap > 0) batch_tiles = std::min(batch_tiles, (static_cast<uint64_t>(cap) + kPairTile - 1) / kPairTile);
  const uint64_t batch_rows = batch_tiles * kPairTile, panel_pitch = batch_tiles * 16;

  // ---- buffers
  if (int rc = use_device(cdev)) return rc;
  ScratchPlan plan;
  const size_t o_summary = plan.add(pairs * sizeof(kgx_roh_summary)), o_open = plan.add(pairs * sizeof(kgx_v4u)), o_list = plan.add(list_bytes);
  const size_t o_position = plan.add(n_rows * sizeof(uint32_t)), o_breaks = plan.add(tiles * 8), o_keep = plan.add(pop->keep.empty() ? 0 : T * kRunTile);
  const size_t o_panel = plan.add(padded * panel_pitch);
  char* arena = nullptr;
  if (int rc = scratch_reserve(cdev, plan.total, &arena)) return rc;
  uint8_t* d_panel = reinterpret_cast<uint8_t*>(arena + o_panel);
  const uint32_t* d_list = call.rows ? reinterpret_cast<const uint32_t*>(arena + o_list) : nullptr;
  std::vector<uint8_t> keep;                                  // the mask, one byte a genome, zero past the last
  if (!pop->keep.empty()) {
    keep.assign(T * kRunTile, 0);
    std::copy(pop->keep.begin(), pop->keep.end(), keep.begin());
    KGX_HIP(hipMemcpyAsync(arena + o_keep, keep.data(), keep.size(), hipMemcpyHostToDevice, cdev.stream));
  }
  if (call.rows) KGX_HIP(hipMemcpyAsync(arena + o_list, call.rows, list_bytes, hipMemcpyHostToDevice, cdev.stream));
  KGX_HIP(hipMemcpyAsync(arena + o_position, call.position, n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, cdev.stream));
  KGX_HIP(hipMemcpyAsync(arena + o_breaks, call.breaks.data(), tiles * 8, hipMemcpyHostToDevice, cdev.stream));
  KGX_HIP(hipStreamSynchronize(cdev.stream));                 // the sources are pageable host memory
  for (size_t s = 0; s < pop->shards.size(); ++s) {
    const kgx_pop_shard& sh = pop->shards[s];
    sb[s].d_list = d_list;
    sb[s].d_panel = d_panel + sh.genome_base * panel_pitch;   // results go straight into the first device's panel
    if (!sb[s].foreign || sh.n_genomes == 0) continue;
    // a shard elsewhere: its own copy of the row list and its own panel in that device's arena, copied over per batch
    Device& dev = *sh.dev;
    if (int rc = use_device(dev)) return rc;
    ScratchPlan fplan;
    const size_t f_list = fplan.add(list_bytes), f_panel = fplan.add((sh.n_genomes + kPairTile - 1) / kPairTile * kPairTile * panel_pitch);
    char* farena = nullptr;
    if (int rc = scratch_reserve(dev, fplan.total, &farena)) return rc;
    if (call.rows) {
      KGX_HIP(hipMemcpyAsync(farena + f_list, call.rows, list_bytes, hipMemcpyHostToDevice, dev.stream));
      KGX_HIP(hipStreamSynchronize(dev.stream));
      sb[s].d_list = reinterpret_cast<const uint32_t*>(farena + f_list);
    }
    sb[s].d_panel = reinterpret_cast<uint8_t*>(farena + f_panel);
  }

  if (int rc = use_device(cdev)) return rc;
  const uint64_t tile_pairs = T * (T + 1) / 2;
  if (tile_pairs > 0x7FFFFFFFull) return fail(KGX_EINVAL, "pair_runs: %llu genomes make more tile pairs than a grid holds", (unsigned long long)G);
  EventPair walk_time;
  if (int rc = walk_time.create()) return rc;

  uint64_t batches = 0;
  for (uint64_t b0 = 0; b0 < n_rows; b0 += batch_rows, ++batches) {
    const uint64_t B = std::min(batch_rows, n_rows - b0);
    // ---- stage 1: every shard turns its genomes' part of the batch around (k_pair_panel: rows past B and masked genomes are code 0)
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
    for (Device* d : foreign) {
      if (int rc = use_device(*d)) return rc;
      KGX_HIP(hipStreamSynchronize(d->stream));
    }
    // ---- stage 2: the batch's part of every pair's walk, on the first device; the table carries the open runs to the next batch
    if (int rc = use_device(cdev)) return rc;
    KGX_HIP(hipEventRecord(walk_time.begin, cdev.stream));
    const auto kernel = call.mode == KGX_SHARE_IDENTICAL ? k_pair_runs<true> : k_pair_runs<false>;
    hipLaunchKernelGGL(kernel, dim3(static_cast<uint32_t>(tile_pairs)), dim3(kBlock), 0, cdev.stream, d_panel, panel_pitch, static_cast<uint32_t>(T), G,
                       pop->keep.empty() ? nullptr : reinterpret_cast<const uint8_t*>(arena + o_keep), reinterpret_cast<const uint32_t*>(arena + o_position),
                       reinterpret_cast<const unsigned long long*>(arena + o_breaks), static_cast<uint32_t>(b0), static_cast<uint32_t>(B), call.min_sites,
                       call.min_length, b0 == 0, b0 + B == n_rows, reinterpret_cast<unsigned long long*>(arena + o_summary),
                       reinterpret_cast<kgx_v4u*>(arena + o_open));
    KGX_HIP(hipGetLastError());
    KGX_HIP(hipEventRecord(walk_time.end, cdev.stream));
    KGX_HIP(hipStreamSynchronize(cdev.stream));               // the next batch overwrites the panel
    walk_time.collect();
  }
  KGX_HIP(hipMemcpyAsync(out, arena + o_summary, pairs * sizeof(kgx_roh_summary), hipMemcpyDeviceToHost, cdev.stream));
  KGX_HIP(hipStreamSynchronize(cdev.stream));
  g_last_pair_runs_ms = walk_time.ms;
  g_last_pair_runs_batches = batches;
  return KGX_OK;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" {

int kgx_pair_runs(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, const uint32_t* position, const uint8_t* contig_start,
                  const kgx_pair_runs_params* params, kgx_roh_summary* out) {
  return guarded([&]() -> int {
    if (int bound = require_bound()) return bound;
    if (!pop) return fail(KGX_EINVAL, "pair_runs: null argument (pop is required)");
    if (n_rows && (!position || !out)) return fail(KGX_EINVAL, "pair_runs: null argument (position and out are required)");
    const uint32_t mode = params ? params->mode : static_cast<uint32_t>(KGX_SHARE_IBS0);
    if (mode != KGX_SHARE_IBS0 && mode != KGX_SHARE_IDENTICAL)
      return fail(KGX_EINVAL, "pair_runs: mode %u is neither KGX_SHARE_IBS0 (0) nor KGX_SHARE_IDENTICAL (1)", mode);
    if (n_rows >= (1ull << 32)) return fail(KGX_EINVAL, "pair_runs: n_rows %llu exceeds the 32-bit list positions of the runs", (unsigned long long)n_rows);
    if (!rows && n_rows > pop->n_variants)
      return fail(KGX_EINVAL, "pair_runs: n_rows %llu exceeds the population's %llu rows", (unsigned long long)n_rows, (unsigned long long)pop->n_variants);
    std::vector<unsigned long long> breaks;
    if (int rc = run_breaks("pair_runs", pop, rows, n_rows, position, contig_start, params ? params->max_gap : 0, breaks)) return rc;
    g_last_pair_runs_ms = 0.0;
    g_last_pair_runs_batches = 0;
    if (out) std::memset(out, 0, pop->n_genomes * (pop->n_genomes + 1) / 2 * sizeof(kgx_roh_summary));
    if (n_rows == 0 || pop->n_genomes == 0) return KGX_OK;
    const PairRunsCall call{pop, rows, position, n_rows, breaks, params && params->min_sites ? params->min_sites : 1u,
                            params && params->min_length ? params->min_length : 1u, mode};
    const int rc = pair_runs_impl(call, out);
    (void)use_device(*pop->shards[0].dev);
    return rc;
  });
}

int kgx_pair_runs_last(double* kernel_ms, uint64_t* row_batches) {
  if (kernel_ms) *kernel_ms = g_last_pair_runs_ms.load();
  if (row_batches) *row_batches = g_last_pair_runs_batches.load();
  return KGX_OK;
}

// Each value is one conversion of each integer and ONE division.
int kgx_pair_run_fractions(const kgx_roh_summary* summary, uint64_t n_genomes, uint64_t denominator, double* out) {
  return guarded([&]() -> int {
    if (n_genomes && (!summary || !out)) return fail(KGX_EINVAL, "pair_run_fractions: null argument");
    const uint64_t pairs = n_genomes * (n_genomes + 1) / 2;
    for (uint64_t p = 0; p < pairs; ++p)
      out[p] = denominator ? static_cast<double>(summary[p].total_length) / static_cast<double>(denominator) : std::numeric_limits<double>::quiet_NaN();
    return KGX_OK;
  });
}

}  // extern "C"
