// C ABI (include/kgx.h) of the pairwise identity by descent: kgx_pair_hmm (per unordered genome pair the log-likelihood and the
// smoothed IBD weight of a two-state hidden Markov model along the listed rows: kgx_pair_counts' genome-major panel per row batch,
// then the forward walk of kgx_kernels_pair_hmm.h), kgx_pair_hmm_last, and the model's inputs from counts and positions:
// kgx_ibd_tables / kgx_ibd_carry (host only).  No CPU fallback exists for the device part.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "kgx_kernels_panel.h"
#include "kgx_kernels_pair_hmm.h"
#include "kgx_internal.h"

namespace kgx {
namespace {

static_assert(sizeof(kgx_pair_hmm_result) == 2 * sizeof(double), "k_pair_hmm writes the result as two doubles");
static_assert(sizeof(HmmRow) == 4 * sizeof(double), "k_pair_hmm reads a row's constants as 32 bytes");

std::atomic<double> g_last_pair_hmm_ms{0.0};
std::atomic<uint64_t> g_last_pair_hmm_batches{0};

constexpr double kEmitLow = 0x1p-30, kEmitHigh = 0x1p30, kWeightHigh = 0x1p32;

struct PairHmmCall {
  kgx_pop* pop;
  const uint32_t* rows;
  uint64_t n_rows;
  const float* emit;
  const double *carry, *weight;
  double pi;
};

int pair_hmm_impl(const PairHmmCall& call, kgx_pair_hmm_result* out) {
  kgx_pop* pop = call.pop;
  const uint64_t n_rows = call.n_rows, G = pop->n_genomes, padded = (G + kPairTile - 1) / kPairTile * kPairTile, T = (G + kHmmTile - 1) / kHmmTile;
  const uint64_t pairs = G * (G + 1) / 2, list_bytes = call.rows ? n_rows * sizeof(uint32_t) : 0, keep_bytes = pop->keep.empty() ? 0 : T * kHmmTile;
  const uint64_t tiles = (n_rows + kPairTile - 1) / kPairTile, list_rows = tiles * kPairTile;
  for (const auto& sh : pop->shards)
    if (sh.n_genomes && sh.genome_base % kPairTile) return fail(KGX_ESTATE, "pair_hmm: a shard does not start at a whole 64-genome tile");

  // ---- the list's tables as the kernel reads them: whole 64-row tiles, the positions past the end identities of the recursion
  std::vector<float> emit(list_rows * 12, 1.0f);
  std::copy(call.emit, call.emit + n_rows * 12, emit.begin());
  std::vector<HmmRow> row_constants(list_rows, HmmRow{1.0, 0.0, 0.0, 0.0});
  for (uint64_t i = 0; i < n_rows; ++i) {
    const double rho = i == 0 ? 0.0 : call.carry[i], jump = 1.0 - rho;
    row_constants[i] = HmmRow{rho, jump * (1.0 - call.pi), jump * call.pi, call.weight ? call.weight[i] : 1.0};
  }

  // ---- devices: the walk runs on the first shard's; shards on the same HIP device share its stream and arena
  Device& cdev = *pop->shards[0].dev;
  PanelShards shards(pop);
  std::vector<PanelShard>& sb = shards.sb;

  // ---- rows per batch, in whole 64-row tiles: the panel within a quarter of (free + arena) on every device; the pairs' table
  //      (state and result), the list's tables and the keep bytes beside it on the first
  if (int rc = use_device(cdev)) return rc;
  const uint64_t table_bytes = pairs * (kHmmState * sizeof(double) + sizeof(kgx_pair_hmm_result));
  const uint64_t available = available_bytes(cdev), fixed = table_bytes + list_bytes + keep_bytes + list_rows * (12 * sizeof(float) + sizeof(HmmRow)) + 7 * 256;
  if (fixed + padded * 16 > available)
    return fail(KGX_ENOMEM, "pair_hmm: the %llu-byte table of %llu genomes' pairs does not fit beside one 64-row panel into the %llu bytes free on the first device",
                (unsigned long long)table_bytes, (unsigned long long)G, (unsigned long long)available);
  uint64_t batch_tiles = std::min(available / 4, available - fixed) / (padded * 16);
  if (int rc = shards.fit_elsewhere(pop, kPairTile, list_bytes, batch_tiles)) return rc;
  batch_tiles = std::max<uint64_t>(1, std::min(batch_tiles, tiles));
  const int cap = env_int("KGX_PAIR_HMM_ROWS", 0);            // only ever lowers the count: the tests carry the state over batch edges with it
  if (cap > 0) batch_tiles = std::min(batch_tiles, (static_cast<uint64_t>(cap) + kPairTile - 1) / kPairTile);
  const uint64_t batch_rows = batch_tiles * kPairTile, panel_pitch = batch_tiles * 16;

  // ---- buffers
  if (int rc = use_device(cdev)) return rc;
  ScratchPlan plan;
  const size_t o_state = plan.add(pairs * kHmmState * sizeof(double)), o_result = plan.add(pairs * sizeof(kgx_pair_hmm_result)), o_list = plan.add(list_bytes);
  const size_t o_keep = plan.add(keep_bytes), o_emit = plan.add(emit.size() * sizeof(float)), o_rows = plan.add(row_constants.size() * sizeof(HmmRow));
  const size_t o_panel = plan.add(padded * panel_pitch);
  char* arena = nullptr;
  if (int rc = scratch_reserve(cdev, plan.total, &arena)) return rc;
  uint8_t* d_panel = reinterpret_cast<uint8_t*>(arena + o_panel);
  const uint32_t* d_list = call.rows ? reinterpret_cast<const uint32_t*>(arena + o_list) : nullptr;
  std::vector<uint8_t> keep;                                  // the mask, one byte a genome, zero past the last
  if (keep_bytes) {
    keep.assign(keep_bytes, 0);
    std::copy(pop->keep.begin(), pop->keep.end(), keep.begin());
    KGX_HIP(hipMemcpyAsync(arena + o_keep, keep.data(), keep_bytes, hipMemcpyHostToDevice, cdev.stream));
  }
  if (call.rows) KGX_HIP(hipMemcpyAsync(arena + o_list, call.rows, list_bytes, hipMemcpyHostToDevice, cdev.stream));
  KGX_HIP(hipMemcpyAsync(arena + o_emit, emit.data(), emit.size() * sizeof(float), hipMemcpyHostToDevice, cdev.stream));
  KGX_HIP(hipMemcpyAsync(arena + o_rows, row_constants.data(), row_constants.size() * sizeof(HmmRow), hipMemcpyHostToDevice, cdev.stream));
  KGX_HIP(hipStreamSynchronize(cdev.stream));                 // the sources are pageable host memory
  if (int rc = shards.reserve(pop, kPairTile, call.rows, list_bytes, d_list, d_panel, panel_pitch)) return rc;

  if (int rc = use_device(cdev)) return rc;
  const uint64_t tile_pairs = T * (T + 1) / 2;
  if (tile_pairs > 0x7FFFFFFFull) return fail(KGX_EINVAL, "pair_hmm: %llu genomes make more tile pairs than a grid holds", (unsigned long long)G);
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
    for (Device* d : shards.foreign) {
      if (int rc = use_device(*d)) return rc;
      KGX_HIP(hipStreamSynchronize(d->stream));
    }
    // ---- stage 2: the batch's part of every pair's walk, on the first device; the table carries the state to the next batch
    if (int rc = use_device(cdev)) return rc;
    KGX_HIP(hipEventRecord(walk_time.begin, cdev.stream));
    hipLaunchKernelGGL(k_pair_hmm, dim3(static_cast<uint32_t>(tile_pairs)), dim3(kBlock), 0, cdev.stream, d_panel, panel_pitch, static_cast<uint32_t>(T), G,
                       keep_bytes ? reinterpret_cast<const uint8_t*>(arena + o_keep) : nullptr, reinterpret_cast<const float*>(arena + o_emit),
                       reinterpret_cast<const HmmRow*>(arena + o_rows), static_cast<uint32_t>(b0), static_cast<uint32_t>(B), 1.0 - call.pi, call.pi, b0 == 0,
                       b0 + B == n_rows, reinterpret_cast<double*>(arena + o_state), reinterpret_cast<double*>(arena + o_result));
    KGX_HIP(hipGetLastError());
    KGX_HIP(hipEventRecord(walk_time.end, cdev.stream));
    KGX_HIP(hipStreamSynchronize(cdev.stream));               // the next batch overwrites the panel
    walk_time.collect();
  }
  KGX_HIP(hipMemcpyAsync(out, arena + o_result, pairs * sizeof(kgx_pair_hmm_result), hipMemcpyDeviceToHost, cdev.stream));
  KGX_HIP(hipStreamSynchronize(cdev.stream));
  g_last_pair_hmm_ms = walk_time.ms;
  g_last_pair_hmm_batches = batches;
  return KGX_OK;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" {

int kgx_pair_hmm(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, const float* emit, const double* carry, const double* weight,
                 const kgx_pair_hmm_params* params, kgx_pair_hmm_result* out) {
  return guarded([&]() -> int {
    if (int bound = require_bound()) return bound;
    if (!pop || !params) return fail(KGX_EINVAL, "pair_hmm: null argument (pop and params are required)");
    if (n_rows && (!emit || !carry || !out)) return fail(KGX_EINVAL, "pair_hmm: null argument (emit, carry and out are required)");
    if (!(params->pi > 0.0 && params->pi < 1.0)) return fail(KGX_EINVAL, "pair_hmm: pi = %g is not inside (0, 1)", params->pi);
    if (n_rows >= (1ull << 32)) return fail(KGX_EINVAL, "pair_hmm: n_rows %llu exceeds the 32-bit list positions", (unsigned long long)n_rows);
    if (!rows && n_rows > pop->n_variants)
      return fail(KGX_EINVAL, "pair_hmm: n_rows %llu exceeds the population's %llu rows", (unsigned long long)n_rows, (unsigned long long)pop->n_variants);
    for (uint64_t i = 0; i < n_rows; ++i) {
      if (rows && rows[i] >= pop->n_variants)
        return fail(KGX_EINVAL, "pair_hmm: rows[%llu] = %u is not a row of the population's %llu", (unsigned long long)i, rows[i], (unsigned long long)pop->n_variants);
      for (int e = 0; e < 12; ++e) {
        const float v = emit[12 * i + e];
        if (!(v >= kEmitLow && v <= kEmitHigh))               // (a NaN fails both)
          return fail(KGX_EINVAL, "pair_hmm: emit[%llu][%d][%d] = %g is not within [2^-30, 2^30]", (unsigned long long)i, e / 6, e % 6, (double)v);
      }
      if (!(carry[i] >= 0.0 && carry[i] <= 1.0)) return fail(KGX_EINVAL, "pair_hmm: carry[%llu] = %g is not within [0, 1]", (unsigned long long)i, carry[i]);
      if (weight && !(weight[i] >= 0.0 && weight[i] <= kWeightHigh))
        return fail(KGX_EINVAL, "pair_hmm: weight[%llu] = %g is not within [0, 2^32]", (unsigned long long)i, weight[i]);
    }
    g_last_pair_hmm_ms = 0.0;
    g_last_pair_hmm_batches = 0;
    if (out) std::memset(out, 0, pop->n_genomes * (pop->n_genomes + 1) / 2 * sizeof(kgx_pair_hmm_result));
    if (n_rows == 0 || pop->n_genomes == 0) return KGX_OK;
    const PairHmmCall call{pop, rows, n_rows, emit, carry, weight, params->pi};
    const int rc = pair_hmm_impl(call, out);
    (void)use_device(*pop->shards[0].dev);
    return rc;
  });
}

int kgx_pair_hmm_last(double* kernel_ms, uint64_t* row_batches) {
  if (kernel_ms) *kernel_ms = g_last_pair_hmm_ms.load();
  if (row_batches) *row_batches = g_last_pair_hmm_batches.load();
  return KGX_OK;
}

// This translation unit is built with floating contraction off: every line below is the IEEE operations it shows, in double, and
// each entry is rounded to float once.
int kgx_ibd_tables(const uint32_t* row_counts, uint64_t n_rows, double eps, float* emit) {
  return guarded([&]() -> int {
    if (n_rows && (!row_counts || !emit)) return fail(KGX_EINVAL, "ibd_tables: null argument");
    if (!(eps > 0.0 && eps <= 0.5)) return fail(KGX_EINVAL, "ibd_tables: eps = %g is not within (0, 0.5]", eps);
    constexpr int kClass[2][2] = {{0, 2}, {2, 5}};            // of the alleles (x, y): codes 0 and 2
    for (uint64_t i = 0; i < n_rows; ++i) {
      float* e = emit + 12 * i;
      std::fill(e, e + 12, 1.0f);
      const uint64_t c0 = row_counts[4 * i], c2 = row_counts[4 * i + 2];
      if (c0 == 0 || c2 == 0) continue;                       // nothing called, or one allele only: the row says nothing
      const double p1 = static_cast<double>(c2) / static_cast<double>(c0 + c2), p[2] = {1.0 - p1, p1};
      const double g[2] = {p[0] * (1.0 - eps) + (1.0 - p[0]) * eps, p[1] * (1.0 - eps) + (1.0 - p[1]) * eps};
      for (int x = 0; x < 2; ++x)
        for (int y = x; y < 2; ++y) {
          double ibd = 0.0;
          for (int z = 0; z < 2; ++z) ibd += p[z] * (x == z ? 1.0 - eps : eps) * (y == z ? 1.0 - eps : eps);
          e[kClass[x][y]] = static_cast<float>(g[x] * g[y]);
          e[6 + kClass[x][y]] = static_cast<float>(ibd);
        }
    }
    return KGX_OK;
  });
}

int kgx_ibd_carry(const uint32_t* position, const uint8_t* contig_start, uint64_t n_rows, double rate, double* carry) {
  return guarded([&]() -> int {
    if (n_rows && (!position || !carry)) return fail(KGX_EINVAL, "ibd_carry: null argument (position and carry are required)");
    if (!(rate >= 0.0 && std::isfinite(rate))) return fail(KGX_EINVAL, "ibd_carry: rate = %g is not a finite rate >= 0", rate);
    for (uint64_t i = 0; i < n_rows; ++i) {
      const bool contig = i == 0 || (contig_start && contig_start[i] != 0);
      if (!contig && position[i] < position[i - 1])
        return fail(KGX_EINVAL, "ibd_carry: position[%llu] = %u is below position[%llu] = %u without a contig start", (unsigned long long)i, position[i],
                    (unsigned long long)(i - 1), position[i - 1]);
      carry[i] = contig ? 0.0 : std::exp(-rate * static_cast<double>(position[i] - position[i - 1]));
    }
    return KGX_OK;
  });
}

}  // extern "C"
