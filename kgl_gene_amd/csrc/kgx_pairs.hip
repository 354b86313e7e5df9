// C ABI (include/kgx.h) of the pairwise joint genotype counts: kgx_pair_counts (per unordered genome pair the nine joint counts of
// the kinds H / M / O over the listed rows: a genome-major panel per row batch, then Z Z^T on the matrix cores,
// kgx_kernels_pairs.h), kgx_pair_counts_last / kgx_pair_counts_last_panel_ms and kgx_pair_distances (the library's two distances
// from those counts, host only).  No CPU fallback exists for the device part.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

#include "kgx_kernels_pairs.h"
#include "kgx_internal.h"

namespace kgx {
namespace {

std::atomic<double> g_last_pairs_ms{0.0}, g_last_panel_ms{0.0};
std::atomic<uint64_t> g_last_pairs_batches{0}, g_last_pairs_splits{0};

int pair_counts_impl(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, uint32_t* out) {
  const uint64_t G = pop->n_genomes, T = (G + kPairTile - 1) / kPairTile, padded = T * kPairTile;
  const uint64_t words = G * (G + 1) / 2 * kPairWords, list_bytes = rows ? n_rows * sizeof(uint32_t) : 0;
  for (const auto& sh : pop->shards)
    if (sh.n_genomes && sh.genome_base % kPairTile) return fail(KGX_ESTATE, "pair_counts: a shard does not start at a whole 64-genome tile");

  // ---- devices: the product runs on the first shard's; shards on the same HIP device share its stream and arena
  Device& cdev = *pop->shards[0].dev;
  PanelShards shards(pop);
  std::vector<PanelShard>& sb = shards.sb;
  const std::vector<Device*>& foreign = shards.foreign;

  // ---- rows per batch: the panel within a quarter of (free + arena) on every device; the triangle beside it on the first
  if (int rc = use_device(cdev)) return rc;
  const uint64_t available = available_bytes(cdev), fixed = words * sizeof(uint32_t) + list_bytes + 3 * 256;
  if (fixed + padded * 16 > available)
    return fail(KGX_ENOMEM, "pair_counts: the %llu-byte table of %llu genomes' pairs does not fit beside one 64-row panel into the %llu bytes free on the first device",
                (unsigned long long)(words * sizeof(uint32_t)), (unsigned long long)G, (unsigned long long)available);
  uint64_t batch_tiles = std::min(available / 4, available - fixed) / (padded * 16);
  if (int rc = shards.fit_elsewhere(pop, kPairTile, list_bytes, batch_tiles)) return rc;
  batch_tiles = std::max<uint64_t>(1, std::min(batch_tiles, (n_rows + kPairTile - 1) / kPairTile));
  uint64_t batch_rows = std::min(batch_tiles * kPairTile, n_rows);
  const int forced = env_int("KGX_PAIRS_ROWS", 0);
  if (forced > 0) batch_rows = std::min(batch_rows, static_cast<uint64_t>(forced));
  batch_tiles = (batch_rows + kPairTile - 1) / kPairTile;
  const uint64_t panel_pitch = batch_tiles * 16;

  // ---- buffers
  if (int rc = use_device(cdev)) return rc;
  ScratchPlan plan;
  const size_t o_out = plan.add(words * sizeof(uint32_t)), o_list = plan.add(list_bytes), o_panel = plan.add(padded * panel_pitch);
  char* arena = nullptr;
  if (int rc = scratch_reserve(cdev, plan.total, &arena)) return rc;
  uint32_t* d_out = reinterpret_cast<uint32_t*>(arena + o_out);
  uint8_t* d_panel = reinterpret_cast<uint8_t*>(arena + o_panel);
  const uint32_t* d_list = rows ? reinterpret_cast<const uint32_t*>(arena + o_list) : nullptr;
  if (rows) {
    KGX_HIP(hipMemcpyAsync(arena + o_list, rows, list_bytes, hipMemcpyHostToDevice, cdev.stream));
    KGX_HIP(hipStreamSynchronize(cdev.stream));               // the source is pageable host memory
  }
  if (int rc = shards.reserve(pop, kPairTile, rows, list_bytes, d_list, d_panel, panel_pitch)) return rc;

  // ---- how the product is cut: tile pairs, and the batch's steps over gridDim.z where the pairs alone leave the device idle
  if (int rc = use_device(cdev)) return rc;
  const uint64_t tile_pairs = T * (T + 1) / 2;
  if (tile_pairs > 0x7FFFFFFFull) return fail(KGX_EINVAL, "pair_counts: %llu genomes make more tile pairs than a grid holds", (unsigned long long)G);
  const uint64_t wanted = 2ull * static_cast<uint64_t>(std::max(cdev.compute_units, 1));
  uint64_t slices = tile_pairs < wanted ? std::min<uint64_t>({(wanted + tile_pairs - 1) / tile_pairs, batch_tiles, 65535}) : 1;
  const int slice_cap = env_int("KGX_PAIRS_SPLITS", 0);      // only ever lowers the count: the tests walk several steps in one workgroup with it
  if (slice_cap > 0) slices = std::min(slices, static_cast<uint64_t>(slice_cap));
  const uint64_t steps_per_slice = (batch_tiles + slices - 1) / slices;
  slices = (batch_tiles + steps_per_slice - 1) / steps_per_slice;
  const bool split = slices > 1;
  if (split) KGX_HIP(hipMemsetAsync(d_out, 0, words * sizeof(uint32_t), cdev.stream));
  EventPair panel_time, product_time;
  if (int rc = panel_time.create()) return rc;
  if (int rc = product_time.create()) return rc;

  uint64_t batches = 0;
  for (uint64_t b0 = 0; b0 < n_rows; b0 += batch_rows, ++batches) {
    const uint64_t B = std::min(batch_rows, n_rows - b0), steps = (B + kPairTile - 1) / kPairTile;
    // ---- stage 1: every shard turns its genomes' part of the batch around
    KGX_HIP(hipEventRecord(panel_time.begin, cdev.stream));
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
    // ---- stage 2: the product of the batch, on the first device
    if (int rc = use_device(cdev)) return rc;
    KGX_HIP(hipEventRecord(panel_time.end, cdev.stream));
    KGX_HIP(hipEventRecord(product_time.begin, cdev.stream));
    const uint64_t z = (steps + steps_per_slice - 1) / steps_per_slice;
    hipLaunchKernelGGL(k_pair_counts, dim3(static_cast<uint32_t>(tile_pairs), 1, static_cast<uint32_t>(z)), dim3(kBlock), 0, cdev.stream, d_panel, panel_pitch,
                       static_cast<uint32_t>(T), G, static_cast<uint32_t>(steps), static_cast<uint32_t>(steps_per_slice), split ? 2 : (b0 ? 1 : 0), d_out);
    KGX_HIP(hipGetLastError());
    KGX_HIP(hipEventRecord(product_time.end, cdev.stream));
    KGX_HIP(hipStreamSynchronize(cdev.stream));               // the next batch overwrites the panel
    panel_time.collect();
    product_time.collect();
  }
  KGX_HIP(hipMemcpyAsync(out, d_out, words * sizeof(uint32_t), hipMemcpyDeviceToHost, cdev.stream));
  KGX_HIP(hipStreamSynchronize(cdev.stream));
  g_last_pairs_ms = product_time.ms;
  g_last_panel_ms = panel_time.ms;
  g_last_pairs_batches = batches;
  g_last_pairs_splits = slices;
  return KGX_OK;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" {

int kgx_pair_counts(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, uint32_t* out) {
  return guarded([&]() -> int {
    if (int bound = require_bound()) return bound;
    if (!pop || !out) return fail(KGX_EINVAL, "pair_counts: null argument (pop and out are required)");
    if (n_rows > 0xFFFFFFFFull) return fail(KGX_EINVAL, "pair_counts: n_rows %llu does not fit the 32-bit counts", (unsigned long long)n_rows);
    if (!rows && n_rows > pop->n_variants)
      return fail(KGX_EINVAL, "pair_counts: n_rows %llu exceeds the population's %llu rows", (unsigned long long)n_rows, (unsigned long long)pop->n_variants);
    for (uint64_t i = 0; rows && i < n_rows; ++i)
      if (rows[i] >= pop->n_variants)
        return fail(KGX_EINVAL, "pair_counts: rows[%llu] = %u is not a row of the population's %llu", (unsigned long long)i, rows[i],
                    (unsigned long long)pop->n_variants);
    g_last_pairs_ms = 0.0;
    g_last_panel_ms = 0.0;
    g_last_pairs_batches = 0;
    g_last_pairs_splits = 0;
    if (n_rows == 0) {
      std::memset(out, 0, pop->n_genomes * (pop->n_genomes + 1) / 2 * kPairWords * sizeof(uint32_t));
      return KGX_OK;
    }
    const int rc = pair_counts_impl(pop, rows, n_rows, out);
    (void)use_device(*pop->shards[0].dev);
    return rc;
  });
}

int kgx_pair_counts_last(double* kernel_ms, uint64_t* row_batches, uint64_t* row_splits) {
  if (kernel_ms) *kernel_ms = g_last_pairs_ms.load();
  if (row_batches) *row_batches = g_last_pairs_batches.load();
  if (row_splits) *row_splits = g_last_pairs_splits.load();
  return KGX_OK;
}

double kgx_pair_counts_last_panel_ms(void) { return g_last_panel_ms.load(); }

// This translation unit is built with floating contraction off; each value is one fp64 division of two integers below 2^53.
int kgx_pair_distances(const uint32_t* counts, uint64_t n_genomes, uint64_t n_rows, int kind, double* out) {
  return guarded([&]() -> int {
    if (kind != 0 && kind != 1) return fail(KGX_EINVAL, "pair_distances: kind %d is neither 0 (IBS) nor 1 (within-sample frequency)", kind);
    if (n_genomes && (!counts || !out)) return fail(KGX_EINVAL, "pair_distances: null argument");
    const uint64_t G = n_genomes;
    for (uint64_t a = 0; a < G; ++a) {
      const uint32_t* own_a = counts + pair_index(a, a, G) * kPairWords;
      for (uint64_t b = a; b < G; ++b) {
        const uint64_t at = pair_index(a, b, G);
        const uint32_t *own_b = counts + pair_index(b, b, G) * kPairWords, *n = counts + at * kPairWords;   // n[3 p + q]: a has kind p, b kind q
        const int64_t called = static_cast<int64_t>(n_rows) - own_a[8] - own_b[8] + n[8];
        const int64_t x_a = (static_cast<int64_t>(own_a[0]) - n[2]) + 2 * (static_cast<int64_t>(own_a[4]) - n[5]);
        const int64_t x_b = (static_cast<int64_t>(own_b[0]) - n[6]) + 2 * (static_cast<int64_t>(own_b[4]) - n[7]);
        const int64_t shared = kind == 0 ? 2 * (static_cast<int64_t>(n[0]) + n[1] + n[3] + 2 * static_cast<int64_t>(n[4]))
                                         : static_cast<int64_t>(n[0]) + 2 * static_cast<int64_t>(n[1]) + 2 * static_cast<int64_t>(n[3]) + 4 * static_cast<int64_t>(n[4]);
        out[at] = called == 0 ? std::numeric_limits<double>::quiet_NaN() : static_cast<double>(x_a + x_b - shared) / static_cast<double>(2 * called);
      }
    }
    return KGX_OK;
  });
}

}  // extern "C"
