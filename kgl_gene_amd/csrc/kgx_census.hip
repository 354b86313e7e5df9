// C ABI (include/kgx.h) of the allele census of the genotype matrix: kgx_gt8_allele_census (per selected locus and genome group
// what the group's genomes carry there, one pass over the matrix bytes on the matrix cores: kgx_kernels_census.h),
// kgx_gt8_allele_census_last and kgx_census_allele_frequencies (the census as the INFO-style AC / AN frequencies the inbreeding
// estimators read, host only).  No CPU fallback exists for the device part.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

#include "kgx_kernels_census.h"
#include "kgx_internal.h"

namespace kgx {
namespace {

std::atomic<double> g_last_census_ms{0.0};
std::atomic<uint64_t> g_last_census_batches{0};

// HIP events of one call, destroyed with it.
struct EventPair {
  hipEvent_t begin = nullptr, end = nullptr;
  double ms = 0.0;
  bool recorded = false;
  ~EventPair() {
    if (begin) (void)hipEventDestroy(begin);
    if (end) (void)hipEventDestroy(end);
  }
};

int allele_census_impl(kgx_gt8* gt, const uint8_t* group_of_genome, uint32_t n_groups, const uint32_t* locus_index, uint64_t n_selected, uint32_t amax,
                       uint32_t* out) {
  const uint32_t kinds = census_kinds(amax);
  const uint64_t words_per_locus = static_cast<uint64_t>(kinds) * n_groups;
  const size_t n_shards = gt->shards.size();
  std::vector<std::unique_lock<std::mutex>> locks;
  for (auto& sh : gt->shards) locks.emplace_back(sh.dev->mutex);

  // ---- loci per batch: the result within a quarter of what is free on every device (the arena counts as free: it is re-used)
  uint64_t batch = n_selected;
  for (auto& sh : gt->shards) {
    if (int rc = use_device(*sh.dev)) return rc;
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) { (void)hipGetLastError(); free_bytes = 0; }
    const uint64_t budget = (static_cast<uint64_t>(free_bytes) + sh.dev->scratch_bytes) / 4;
    batch = std::min(batch, budget / (4 * words_per_locus));
  }
  const int forced = env_int("KGX_CENSUS_LOCI", 0);
  if (forced > 0) batch = std::min(batch, static_cast<uint64_t>(forced));
  if (batch < 1) batch = 1;

  // ---- per shard: the group ids in the rows' own layout, the locus list, the batch's counts
  struct ShardBuffers { const uint8_t* d_ids = nullptr; const uint32_t* d_index = nullptr; uint32_t* d_out = nullptr; };
  std::vector<ShardBuffers> sb(n_shards);
  std::vector<EventPair> events(n_shards);
  std::vector<void*> buffers(n_shards);
  std::vector<hipStream_t> streams(n_shards);
  std::vector<uint8_t> ids;
  for (size_t s = 0; s < n_shards; ++s) {
    kgx_gt8_shard& sh = gt->shards[s];
    Device& dev = *sh.dev;
    if (int rc = use_device(dev)) return rc;
    ScratchPlan plan;
    const size_t o_out = plan.add(batch * words_per_locus * sizeof(uint32_t));
    const size_t o_ids = plan.add(sh.pitch), o_index = plan.add(locus_index ? n_selected * sizeof(uint32_t) : 0);
    char* arena = nullptr;
    if (int rc = scratch_reserve(dev, plan.total, &arena)) return rc;
    sb[s].d_out = reinterpret_cast<uint32_t*>(arena + o_out);
    buffers[s] = sb[s].d_out;
    streams[s] = dev.stream;
    if (sh.n_genomes == 0) continue;
    ids.assign(sh.pitch, 0xFF);                                // past the shard's genomes: in no group
    std::memcpy(ids.data(), group_of_genome + sh.genome_base, sh.n_genomes);
    KGX_HIP(hipMemcpyAsync(arena + o_ids, ids.data(), sh.pitch, hipMemcpyHostToDevice, dev.stream));
    if (locus_index) KGX_HIP(hipMemcpyAsync(arena + o_index, locus_index, n_selected * sizeof(uint32_t), hipMemcpyHostToDevice, dev.stream));
    KGX_HIP(hipStreamSynchronize(dev.stream));                 // the sources are pageable host memory
    sb[s].d_ids = reinterpret_cast<const uint8_t*>(arena + o_ids);
    if (locus_index) sb[s].d_index = reinterpret_cast<const uint32_t*>(arena + o_index);
    KGX_HIP(hipEventCreate(&events[s].begin));
    KGX_HIP(hipEventCreate(&events[s].end));
  }

  const uint32_t loci_per_wave = census_loci_per_wave(amax);
  uint64_t batches = 0;
  for (uint64_t b0 = 0; b0 < n_selected; b0 += batch, ++batches) {
    const uint64_t B = std::min(batch, n_selected - b0);
    for (size_t s = 0; s < n_shards; ++s) {
      kgx_gt8_shard& sh = gt->shards[s];
      Device& dev = *sh.dev;
      if (int rc = use_device(dev)) return rc;
      if (sh.n_genomes == 0) {                                  // a slot without genomes adds nothing to the exchange
        KGX_HIP(hipMemsetAsync(sb[s].d_out, 0, B * words_per_locus * sizeof(uint32_t), dev.stream));
        continue;
      }
      const uint64_t units = (B + loci_per_wave - 1) / loci_per_wave;
      KGX_HIP(hipEventRecord(events[s].begin, dev.stream));
      hipLaunchKernelGGL(k_allele_census, dim3(stream_grid(dev, units, kCensusWaves)), dim3(kBlock), 0, dev.stream, sh.d_gt, sh.pitch,
                         static_cast<uint32_t>((sh.n_genomes + 63) / 64), sb[s].d_ids, sb[s].d_index ? sb[s].d_index + b0 : nullptr, b0, B, amax, n_groups,
                         sb[s].d_out);
      KGX_HIP(hipGetLastError());
      KGX_HIP(hipEventRecord(events[s].end, dev.stream));
      events[s].recorded = true;
    }
    if (n_shards > 1 || gt->rt->exchange != Exchange::None)
      if (int rc = exchange_counts(*gt->rt, buffers, B * words_per_locus, streams)) return rc;
    if (int rc = use_device(*gt->shards[0].dev)) return rc;
    KGX_HIP(hipMemcpyAsync(out + b0 * words_per_locus, sb[0].d_out, B * words_per_locus * sizeof(uint32_t), hipMemcpyDeviceToHost, streams[0]));
    for (size_t s = n_shards; s-- > 0;) {                       // every slot is done with its buffer before the next batch overwrites it
      if (int rc = use_device(*gt->shards[s].dev)) return rc;
      KGX_HIP(hipStreamSynchronize(streams[s]));
    }
    for (auto& p : events)
      if (p.recorded) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.begin, p.end) == hipSuccess) p.ms += ms;
        else (void)hipGetLastError();
        p.recorded = false;
      }
  }
  double slowest = 0.0;
  for (const auto& p : events) slowest = std::max(slowest, p.ms);
  g_last_census_ms = slowest;
  g_last_census_batches = batches;
  return KGX_OK;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" {

int kgx_gt8_allele_census(kgx_gt8* gt, const uint8_t* group_of_genome, uint32_t n_groups, const uint32_t* locus_index, uint64_t n_selected, uint32_t amax,
                          uint32_t* out) {
  return guarded([&]() -> int {
    if (int bound = require_bound()) return bound;
    if (!gt || !group_of_genome || !out) return fail(KGX_EINVAL, "allele_census: null argument (gt, group_of_genome and out are required)");
    if (n_groups == 0 || n_groups > 32) return fail(KGX_EINVAL, "allele_census: n_groups %u outside 1..32", n_groups);
    if (amax == 0 || amax > 14) return fail(KGX_EINVAL, "allele_census: amax %u outside 1..14", amax);
    for (uint64_t g = 0; g < gt->n_genomes; ++g)
      if (group_of_genome[g] >= n_groups && group_of_genome[g] != 0xFF)
        return fail(KGX_EINVAL, "allele_census: group_of_genome[%llu] = %u is neither a group below n_groups = %u nor 0xFF", (unsigned long long)g,
                    group_of_genome[g], n_groups);
    if (!locus_index && n_selected > gt->n_loci)
      return fail(KGX_EINVAL, "allele_census: n_selected %llu exceeds the matrix's %llu loci", (unsigned long long)n_selected, (unsigned long long)gt->n_loci);
    for (uint64_t i = 0; locus_index && i < n_selected; ++i) {
      if (locus_index[i] >= gt->n_loci)
        return fail(KGX_EINVAL, "allele_census: locus_index[%llu] = %u is not a row of the matrix's %llu", (unsigned long long)i, locus_index[i],
                    (unsigned long long)gt->n_loci);
      if (i && locus_index[i] <= locus_index[i - 1]) return fail(KGX_EINVAL, "allele_census: locus_index is not ascending at entry %llu", (unsigned long long)i);
    }
    // offsets with more than 14 alts keep their cells in a wide row: not the census' business
    for (uint64_t i = 0; i < n_selected && !gt->wide_loci.empty(); ++i) {
      const uint32_t locus = locus_index ? locus_index[i] : static_cast<uint32_t>(i);
      if (std::binary_search(gt->wide_loci.begin(), gt->wide_loci.end(), locus))
        return fail(KGX_EINVAL, "allele_census: selected locus %u has a wide row (more than 14 alts): leave it out of locus_index", locus);
    }
    g_last_census_ms = 0.0;
    g_last_census_batches = 0;
    if (n_selected == 0) return KGX_OK;
    const int rc = allele_census_impl(gt, group_of_genome, n_groups, locus_index, n_selected, amax, out);
    (void)use_device(*gt->shards[0].dev);
    return rc;
  });
}

int kgx_gt8_allele_census_last(double* kernel_ms, uint64_t* batches) {
  if (kernel_ms) *kernel_ms = g_last_census_ms.load();
  if (batches) *batches = g_last_census_batches.load();
  return KGX_OK;
}

// This translation unit is built with floating contraction off; the quotient is one fp64 division rounded once to float32, the
// storage type of a VCF INFO frequency.
int kgx_census_allele_frequencies(const uint32_t* census, uint64_t n_loci, uint32_t n_groups, uint32_t amax, const uint64_t* group_genomes,
                                  const uint32_t* pool, uint32_t n_pool, const uint8_t* n_alt, double* minor_af) {
  return guarded([&]() -> int {
    if (n_groups == 0 || n_groups > 32) return fail(KGX_EINVAL, "census_allele_frequencies: n_groups %u outside 1..32", n_groups);
    if (amax == 0 || amax > 14) return fail(KGX_EINVAL, "census_allele_frequencies: amax %u outside 1..14", amax);
    if (!group_genomes || (n_pool && !pool) || (n_loci && (!census || !minor_af))) return fail(KGX_EINVAL, "census_allele_frequencies: null argument");
    uint64_t genomes = 0;
    for (uint32_t p = 0; p < n_pool; ++p) {
      if (pool[p] >= n_groups) return fail(KGX_EINVAL, "census_allele_frequencies: pool[%u] = %u is not a group below n_groups = %u", p, pool[p], n_groups);
      genomes += group_genomes[pool[p]];
    }
    const double allele_number = static_cast<double>(2 * genomes);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const uint32_t kinds = census_kinds(amax);
    for (uint64_t l = 0; l < n_loci; ++l) {
      const uint32_t alts = n_alt ? std::min<uint32_t>(n_alt[l], amax) : amax;
      const uint32_t* locus = census + l * n_groups * kinds;
      for (uint32_t a = 0; a < amax; ++a) {
        if (genomes == 0 || a >= alts) { minor_af[l * amax + a] = nan; continue; }
        uint64_t copies = 0;
        for (uint32_t p = 0; p < n_pool; ++p) {
          const uint32_t* words = locus + static_cast<uint64_t>(pool[p]) * kinds + kCensusFixedKinds + 2u * a;
          copies += static_cast<uint64_t>(words[0]) + 2ull * words[1];
        }
        minor_af[l * amax + a] = static_cast<double>(static_cast<float>(static_cast<double>(copies) / allele_number));
      }
    }
    return KGX_OK;
  });
}

}  // extern "C"
