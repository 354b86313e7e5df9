// C ABI (include/kgx.h) of the gene genotype tables: kgx_gene_genotypes (per-(gene, genome) genotype hashes by one sweep over
// the 2-bit rows, then the per-gene census of those hashes on the device) and kgx_genotype_statistics (Gini / HRel / IQV of a
// genotype distribution, host only).  Replaces the std::map walks of GenotypeAnalysis / GeneGenomeAnalysis
// (kga_analytic/kga_PfEMP/kga_analysis_PfEMP_variant.cpp).  No CPU fallback exists for the device part.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "kgx_kernels_gene.h"
#include "kgx_internal.h"

namespace kgx {
namespace {

std::atomic<double> g_last_gene_ms{0.0};

// Device bytes the census keeps per (gene, genome) of a batch: hash 8 + counts 16 + compacted keys 8 + sorted keys 8 + the
// sort's own second buffer 8.  (The run lists reuse the compacted keys' and the counts' space.)
constexpr uint64_t kCensusBytesPerCell = 48;

// HIP events of one call, destroyed with it.
struct EventPair {
  hipEvent_t begin = nullptr, end = nullptr;
  double ms = 0.0;
  bool recorded = false;
};
struct CallEvents {
  std::vector<EventPair> pairs;
  ~CallEvents() {
    for (auto& p : pairs) {
      if (p.begin) (void)hipEventDestroy(p.begin);
      if (p.end) (void)hipEventDestroy(p.end);
    }
  }
};

// What one shard's sweep needs on the shard's device: the call's tables and, on a device other than the census', the shard's own
// [batch][shard genomes] results before they are copied over.
struct ShardBuffers {
  Device* dev = nullptr;         // whose stream the sweep runs on
  bool foreign = false;          // not the census' HIP device
  const uint32_t* d_list = nullptr;
  const unsigned long long* d_key = nullptr;
  const uint8_t* d_single = nullptr;
  const GeneSpan* d_spans = nullptr;
  unsigned long long* d_hash = nullptr;   // foreign only
  kgx_v4u* d_counts = nullptr;            // foreign only
};

struct Tables {
  size_t o_list, o_key, o_single, o_spans;
  void plan(ScratchPlan& p, uint64_t n_members, uint64_t V, uint64_t n_genes) {
    o_list = p.add((n_members + 1) * sizeof(uint32_t));
    o_key = p.add((V + 1) * sizeof(unsigned long long));
    o_single = p.add(V + 4);
    o_spans = p.add(n_genes * sizeof(GeneSpan));
  }
};

int upload_tables(Device& dev, char* arena, const Tables& t, const uint32_t* member_rows, uint64_t n_members, const uint64_t* row_key, uint64_t V,
                  const std::vector<uint8_t>& single, const std::vector<GeneSpan>& spans, ShardBuffers& b) {
  hipStream_t st = dev.stream;
  if (n_members) KGX_HIP(hipMemcpyAsync(arena + t.o_list, member_rows, n_members * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (V) {
    KGX_HIP(hipMemcpyAsync(arena + t.o_key, row_key, V * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    KGX_HIP(hipMemcpyAsync(arena + t.o_single, single.data(), V, hipMemcpyHostToDevice, st));
  }
  KGX_HIP(hipMemcpyAsync(arena + t.o_spans, spans.data(), spans.size() * sizeof(GeneSpan), hipMemcpyHostToDevice, st));
  KGX_HIP(hipStreamSynchronize(st));                         // the sources are pageable host memory
  b.d_list = reinterpret_cast<const uint32_t*>(arena + t.o_list);
  b.d_key = reinterpret_cast<const unsigned long long*>(arena + t.o_key);
  b.d_single = reinterpret_cast<const uint8_t*>(arena + t.o_single);
  b.d_spans = reinterpret_cast<const GeneSpan*>(arena + t.o_spans);
  return KGX_OK;
}

int gene_genotypes_impl(kgx_pop* pop, const uint64_t* row_key, const uint32_t* member_rows, uint64_t n_members, const uint32_t* first_member,
                        const uint32_t* n_rows, uint64_t n_genes, uint64_t* hash, uint32_t* counts, kgx_gene_census* census, uint64_t* run_begin,
                        uint64_t* run_hash, uint32_t* run_count, uint64_t capacity) {
  const uint64_t G = pop->n_genomes, V = pop->n_variants;
  const bool fill = run_hash != nullptr;
  run_begin[0] = 0;
  g_last_gene_ms = 0.0;
  if (n_genes == 0) return KGX_OK;
  if (G > 0xFFFFFFFFull || V > 0xFFFFFFFFull) return fail(KGX_EINVAL, "gene_genotypes: more than 2^32 genomes or rows");

  // ---- the genes: ranges, rows in range, no row twice in a gene
  std::vector<GeneSpan> spans(n_genes);
  {
    std::vector<uint64_t> seen_in(V, 0);                      // 1 + the last gene that listed the row
    for (uint64_t i = 0; i < n_genes; ++i) {
      if (static_cast<uint64_t>(first_member[i]) + n_rows[i] > n_members)
        return fail(KGX_EINVAL, "gene %llu: rows [%u, +%u) outside the %llu member rows", (unsigned long long)i, first_member[i], n_rows[i], (unsigned long long)n_members);
      spans[i] = GeneSpan{first_member[i], n_rows[i]};
      for (uint32_t r = 0; r < n_rows[i]; ++r) {
        const uint32_t row = member_rows[first_member[i] + r];
        if (row >= V) return fail(KGX_EINVAL, "gene %llu: member row %u past the population's %llu rows", (unsigned long long)i, row, (unsigned long long)V);
        if (seen_in[row] == i + 1) return fail(KGX_EINVAL, "gene %llu lists row %u more than once", (unsigned long long)i, row);
        seen_in[row] = i + 1;
      }
    }
  }

  // ---- which rows have a carrier, which exactly one: the population's K2 counts (under the genome mask, if one is set)
  std::vector<uint8_t> single(V, 0);
  std::vector<uint8_t> carried_row(V, 0);
  if (V && G) {
    std::vector<uint32_t> k2(V * 4);
    if (int rc = kgx_allele_count_by_locus(pop, k2.data())) return rc;
    for (uint64_t v = 0; v < V; ++v) {
      const uint64_t carriers = static_cast<uint64_t>(k2[v * 4 + 1]) + k2[v * 4 + 2] + k2[v * 4 + 3];
      carried_row[v] = carriers > 0;
      single[v] = carriers == 1;
    }
  }
  uint64_t kept = 0;
  for (const auto& sh : pop->shards) kept += sh.n_kept;
  for (uint64_t i = 0; i < n_genes; ++i) {
    kgx_gene_census c;
    std::memset(&c, 0, sizeof(c));
    c.genomes = kept;
    for (uint32_t r = 0; r < n_rows[i]; ++r) {
      const uint32_t row = member_rows[first_member[i] + r];
      c.unique_variants += carried_row[row];
      c.singleton_variants += single[row];
    }
    census[i] = c;
  }
  if (G == 0) {
    for (uint64_t i = 0; i < n_genes; ++i) run_begin[i + 1] = 0;
    return KGX_OK;
  }

  // ---- devices: the census runs on the first shard's; shards on the same HIP device share its stream, arena and tables
  Device& cdev = *pop->shards[0].dev;
  std::vector<ShardBuffers> sb(pop->shards.size());
  std::vector<Device*> foreign;                                // distinct Device objects on other HIP devices
  for (size_t s = 0; s < pop->shards.size(); ++s) {
    Device* d = pop->shards[s].dev;
    sb[s].foreign = d->id != cdev.id;
    sb[s].dev = sb[s].foreign ? d : &cdev;
    if (sb[s].foreign && std::find(foreign.begin(), foreign.end(), d) == foreign.end()) foreign.push_back(d);
  }
  std::vector<std::unique_lock<std::mutex>> locks;
  locks.emplace_back(cdev.mutex);
  for (Device* d : foreign) locks.emplace_back(d->mutex);
  if (int rc = use_device(cdev)) return rc;
  hipStream_t st = cdev.stream;

  // ---- batch size: the census' buffers within a quarter of what is free (the arena counts as free: it is re-used)
  size_t free_bytes = 0, total_bytes = 0;
  if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) { (void)hipGetLastError(); free_bytes = 0; }
  const uint64_t budget = (static_cast<uint64_t>(free_bytes) + cdev.scratch_bytes) / 4;
  uint64_t batch = budget / (kCensusBytesPerCell * G);
  if (batch > 0xFFFFFFFFull / G) batch = 0xFFFFFFFFull / G;   // the sort's 32-bit positions
  // KGX_GENE_SMALL=b or b,s: at most b genes per batch and exactly s (default b) genes per workgroup slice -- the tests cross
  // both boundaries at small sizes with it
  uint64_t forced_batch = 0, forced_slice = 0;
  {
    const std::string small = env_str("KGX_GENE_SMALL");
    if (!small.empty()) {
      const long b = std::atol(small.c_str());
      const size_t comma = small.find(',');
      const long s = comma == std::string::npos ? b : std::atol(small.c_str() + comma + 1);
      if (b > 0) forced_batch = static_cast<uint64_t>(b);
      if (s > 0) forced_slice = static_cast<uint64_t>(s);
    }
  }
  if (forced_batch && forced_batch < batch) batch = forced_batch;
  if (batch > n_genes) batch = n_genes;
  if (batch < 1) batch = 1;
  const uint64_t cells = batch * G;

  size_t sort_bytes = 0;
  KGX_HIP(rocprim::segmented_radix_sort_keys(nullptr, sort_bytes, static_cast<unsigned long long*>(nullptr), static_cast<unsigned long long*>(nullptr),
                                             static_cast<unsigned int>(cells), static_cast<unsigned int>(batch), static_cast<uint32_t*>(nullptr),
                                             static_cast<uint32_t*>(nullptr), 0, 64, st));
  ScratchPlan plan;
  Tables tables;
  tables.plan(plan, n_members, V, n_genes);
  const size_t o_hash = plan.add(cells * 8), o_counts = plan.add(cells * 16), o_keys = plan.add(cells * 8), o_sorted = plan.add(cells * 8);
  const size_t o_sort = plan.add(sort_bytes), o_begin = plan.add(batch * 4), o_end = plan.add(batch * 4), o_sums = plan.add(batch * sizeof(GeneSums));
  const size_t o_nruns = plan.add(batch * 4), o_runbegin = plan.add(batch * 8), o_top = plan.add(batch * 5 * 8);
  char* arena = nullptr;
  if (int rc = scratch_reserve(cdev, plan.total, &arena)) return rc;
  ShardBuffers central;
  central.dev = &cdev;
  if (int rc = upload_tables(cdev, arena, tables, member_rows, n_members, row_key, V, single, spans, central)) return rc;
  auto* d_hash = reinterpret_cast<unsigned long long*>(arena + o_hash);
  auto* d_counts = reinterpret_cast<kgx_v4u*>(arena + o_counts);
  auto* d_keys = reinterpret_cast<unsigned long long*>(arena + o_keys);
  auto* d_sorted = reinterpret_cast<unsigned long long*>(arena + o_sorted);
  auto* d_seg_begin = reinterpret_cast<uint32_t*>(arena + o_begin);
  auto* d_seg_end = reinterpret_cast<uint32_t*>(arena + o_end);
  auto* d_sums = reinterpret_cast<GeneSums*>(arena + o_sums);
  auto* d_nruns = reinterpret_cast<uint32_t*>(arena + o_nruns);
  auto* d_runbegin = reinterpret_cast<unsigned long long*>(arena + o_runbegin);
  auto* d_top = reinterpret_cast<unsigned long long*>(arena + o_top);
  unsigned long long* d_run_hash = d_keys;                                   // dead once sorted
  uint32_t* d_run_count = reinterpret_cast<uint32_t*>(d_counts);             // dead once compacted (and copied out, in stream order)

  CallEvents events;
  events.pairs.resize(pop->shards.size());
  for (size_t s = 0; s < pop->shards.size(); ++s) {
    const kgx_pop_shard& sh = pop->shards[s];
    if (!sb[s].foreign) {
      sb[s] = central;                                        // the census device's tables; results go straight into its buffers
    } else if (sh.n_genomes) {
      // a shard elsewhere: its own copy of the tables and its own [batch][shard genomes] results in that device's arena
      Device& dev = *sh.dev;
      if (int rc = use_device(dev)) return rc;
      ScratchPlan fplan;
      Tables ft;
      ft.plan(fplan, n_members, V, n_genes);
      const size_t f_hash = fplan.add(batch * sh.n_genomes * 8), f_counts = fplan.add(batch * sh.n_genomes * 16);
      char* farena = nullptr;
      if (int rc = scratch_reserve(dev, fplan.total, &farena)) return rc;
      if (int rc = upload_tables(dev, farena, ft, member_rows, n_members, row_key, V, single, spans, sb[s])) return rc;
      sb[s].d_hash = reinterpret_cast<unsigned long long*>(farena + f_hash);
      sb[s].d_counts = reinterpret_cast<kgx_v4u*>(farena + f_counts);
    }
    if (sh.n_genomes) {
      if (int rc = use_device(*sb[s].dev)) return rc;
      KGX_HIP(hipEventCreate(&events.pairs[s].begin));
      KGX_HIP(hipEventCreate(&events.pairs[s].end));
    }
  }

  std::vector<uint32_t> h_nruns(batch);
  std::vector<GeneSums> h_sums(batch);
  std::vector<unsigned long long> h_runbegin(batch), h_top(batch * 5);
  for (uint64_t b0 = 0; b0 < n_genes; b0 += batch) {
    const uint64_t B = std::min(batch, n_genes - b0);
    // ---- the hashing sweep, every shard on its own device
    for (size_t s = 0; s < pop->shards.size(); ++s) {
      const kgx_pop_shard& sh = pop->shards[s];
      if (sh.n_genomes == 0) continue;
      Device& dev = *sb[s].dev;
      if (int rc = use_device(dev)) return rc;
      const uint64_t cols = (sh.n_genomes + 15) / 16;
      const uint32_t gx = static_cast<uint32_t>((cols + kBlock - 1) / kBlock);
      uint64_t slices = (static_cast<uint64_t>(dev.compute_units) * 8 + gx - 1) / gx;
      if (slices > B) slices = B;
      if (slices > 65535) slices = 65535;
      uint64_t per_slice = (B + slices - 1) / slices;
      if (forced_slice) per_slice = forced_slice;
      const uint64_t gy = (B + per_slice - 1) / per_slice;
      if (gy > 65535) return fail(KGX_EINVAL, "gene_genotypes: %llu slices of %llu genes exceed the grid", (unsigned long long)gy, (unsigned long long)per_slice);
      unsigned long long* out_hash = sb[s].foreign ? sb[s].d_hash : d_hash;
      kgx_v4u* out_counts = sb[s].foreign ? sb[s].d_counts : d_counts;
      const uint64_t out_pitch = sb[s].foreign ? sh.n_genomes : G, out_col0 = sb[s].foreign ? 0 : sh.genome_base;
      KGX_HIP(hipEventRecord(events.pairs[s].begin, dev.stream));
      hipLaunchKernelGGL(k_gene_genotypes, dim3(gx, static_cast<uint32_t>(gy)), dim3(kBlock), 0, dev.stream, reinterpret_cast<const uint32_t*>(sh.d_rows),
                         sh.pitch / 4, sh.n_genomes, reinterpret_cast<const uint32_t*>(sh.d_keep), sb[s].d_spans + b0, B, per_slice, sb[s].d_list, sb[s].d_key,
                         sb[s].d_single, out_hash, out_counts, out_pitch, out_col0);
      KGX_HIP(hipGetLastError());
      KGX_HIP(hipEventRecord(events.pairs[s].end, dev.stream));
      events.pairs[s].recorded = true;
      if (sb[s].foreign) {
        KGX_HIP(hipMemcpy2DAsync(d_hash + sh.genome_base, G * 8, sb[s].d_hash, sh.n_genomes * 8, sh.n_genomes * 8, B, hipMemcpyDefault, dev.stream));
        KGX_HIP(hipMemcpy2DAsync(d_counts + sh.genome_base, G * 16, sb[s].d_counts, sh.n_genomes * 16, sh.n_genomes * 16, B, hipMemcpyDefault, dev.stream));
      }
    }
    for (Device* d : foreign) {
      if (int rc = use_device(*d)) return rc;
      KGX_HIP(hipStreamSynchronize(d->stream));
    }
    if (int rc = use_device(cdev)) return rc;
    if (hash) KGX_HIP(hipMemcpyAsync(hash + b0 * G, d_hash, B * G * 8, hipMemcpyDeviceToHost, st));
    if (counts) KGX_HIP(hipMemcpyAsync(counts + b0 * G * 4, d_counts, B * G * 16, hipMemcpyDeviceToHost, st));

    // ---- the census of the batch: compact, sort, count the runs
    hipLaunchKernelGGL(k_gene_compact, dim3(static_cast<uint32_t>(B)), dim3(kBlock), 0, st, d_hash, d_counts, G, d_keys, d_seg_begin, d_seg_end, d_sums);
    KGX_HIP(hipGetLastError());
    size_t need = 0;
    KGX_HIP(rocprim::segmented_radix_sort_keys(nullptr, need, d_keys, d_sorted, static_cast<unsigned int>(B * G), static_cast<unsigned int>(B), d_seg_begin,
                                               d_seg_end, 0, 64, st));
    if (need > sort_bytes) return fail(KGX_ESTATE, "gene_genotypes: the sort of %llu genes needs %zu bytes, %zu were planned", (unsigned long long)B, need, sort_bytes);
    KGX_HIP(rocprim::segmented_radix_sort_keys(arena + o_sort, need, d_keys, d_sorted, static_cast<unsigned int>(B * G), static_cast<unsigned int>(B), d_seg_begin,
                                               d_seg_end, 0, 64, st));
    hipLaunchKernelGGL((k_gene_runs<false>), dim3(static_cast<uint32_t>(B)), dim3(kBlock), 0, st, d_sorted, G, d_seg_begin, d_seg_end, d_nruns, nullptr, nullptr,
                       nullptr, nullptr);
    KGX_HIP(hipGetLastError());
    KGX_HIP(hipMemcpyAsync(h_nruns.data(), d_nruns, B * 4, hipMemcpyDeviceToHost, st));
    KGX_HIP(hipMemcpyAsync(h_sums.data(), d_sums, B * sizeof(GeneSums), hipMemcpyDeviceToHost, st));
    KGX_HIP(hipStreamSynchronize(st));

    // ---- offsets, then fill
    uint64_t batch_runs = 0;
    for (uint64_t i = 0; i < B; ++i) {
      h_runbegin[i] = batch_runs;
      batch_runs += h_nruns[i];
      run_begin[b0 + i + 1] = run_begin[b0] + batch_runs;
      kgx_gene_census& c = census[b0 + i];
      c.genotypes = h_nruns[i];
      c.zero_variant_genomes = kept - h_sums[i].genotype_genomes;
      c.variant_objects = h_sums[i].variant_objects;
      c.non_diploid_cells = h_sums[i].non_diploid_cells;
      c.singleton_genomes = h_sums[i].singleton_genomes;
    }
    if (fill && run_begin[b0] + batch_runs > capacity)
      return fail(KGX_EINVAL, "gene_genotypes: the run lists need more than %llu entries, capacity is %llu", (unsigned long long)(run_begin[b0] + batch_runs - 1),
                  (unsigned long long)capacity);
    KGX_HIP(hipMemcpyAsync(d_runbegin, h_runbegin.data(), B * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((k_gene_runs<true>), dim3(static_cast<uint32_t>(B)), dim3(kBlock), 0, st, d_sorted, G, d_seg_begin, d_seg_end, nullptr, d_runbegin, d_run_hash,
                       d_run_count, d_top);
    KGX_HIP(hipGetLastError());
    KGX_HIP(hipMemcpyAsync(h_top.data(), d_top, B * 5 * 8, hipMemcpyDeviceToHost, st));
    if (fill && batch_runs) {
      KGX_HIP(hipMemcpyAsync(run_hash + run_begin[b0], d_run_hash, batch_runs * 8, hipMemcpyDeviceToHost, st));
      KGX_HIP(hipMemcpyAsync(run_count + run_begin[b0], d_run_count, batch_runs * 4, hipMemcpyDeviceToHost, st));
    }
    KGX_HIP(hipStreamSynchronize(st));                       // h_runbegin is pageable; the results are the caller's now
    for (uint64_t i = 0; i < B; ++i)
      for (int k = 0; k < 5; ++k) census[b0 + i].top[k] = h_top[i * 5 + k];
    for (auto& p : events.pairs)
      if (p.recorded) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.begin, p.end) == hipSuccess) p.ms += ms;
        else (void)hipGetLastError();
        p.recorded = false;
      }
  }
  double slowest = 0.0;
  for (const auto& p : events.pairs) slowest = std::max(slowest, p.ms);
  g_last_gene_ms = slowest;
  return KGX_OK;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" {

int kgx_gene_genotypes(kgx_pop* pop, const uint64_t* row_key, const uint32_t* member_rows, uint64_t n_members, const uint32_t* first_member,
                       const uint32_t* n_rows, uint64_t n_genes, uint64_t* hash, uint32_t* counts, kgx_gene_census* census, uint64_t* run_begin,
                       uint64_t* run_hash, uint32_t* run_count, uint64_t capacity) {
  return guarded([&]() -> int {
    if (int bound = require_bound()) return bound;
    if (!pop || !run_begin || (n_genes && (!census || !first_member || !n_rows)) || (n_members && !member_rows) || (pop->n_variants && !row_key))
      return fail(KGX_EINVAL, "gene_genotypes: null argument");
    if ((run_hash == nullptr) != (run_count == nullptr)) return fail(KGX_EINVAL, "gene_genotypes: run_hash and run_count are given together or not at all");
    if (n_members > 0xFFFFFFFFull) return fail(KGX_EINVAL, "more than 2^32 member rows");
    const int rc = gene_genotypes_impl(pop, row_key, member_rows, n_members, first_member, n_rows, n_genes, hash, counts, census, run_begin, run_hash, run_count,
                                       capacity);
    (void)use_device(*pop->shards[0].dev);
    return rc;
  });
}

double kgx_gene_genotypes_last_ms(void) { return g_last_gene_ms.load(); }

// GenotypeAnalysis::Gini / HRel / IQV (kga_analysis_PfEMP_variant.cpp:499-628), quirks kept: one more category for the genomes
// without a variant even when there is none; IQV's proportions over total x 100.  This translation unit is built with floating
// contraction off, as the class-frequency code is.
int kgx_genotype_statistics(const uint32_t* run_count, uint64_t n_runs, uint64_t zero_variant_genomes, double out[3]) {
  return guarded([&]() -> int {
    if (!out || (n_runs && !run_count)) return fail(KGX_EINVAL, "genotype_statistics: null argument");
    const uint64_t categories = n_runs + 1;
    if (categories <= 1) {
      out[0] = 1.0;
      out[1] = 0.0;
      out[2] = 1.0;
      return KGX_OK;
    }
    uint64_t total = zero_variant_genomes;
    for (uint64_t i = 0; i < n_runs; ++i) total += run_count[i];
    // Gini: the reference's O(k^2) sum of |f_i - f_j| over i < j is an integer; over ascending counts it is
    // sum_i f_i (2 i - (k - 1)), computed exactly and converted once (the same double below 2^53)
    std::vector<uint64_t> sorted(categories);
    sorted[0] = zero_variant_genomes;
    for (uint64_t i = 0; i < n_runs; ++i) sorted[i + 1] = run_count[i];
    std::sort(sorted.begin(), sorted.end());
    __int128 pair_sum = 0;
    for (uint64_t i = 0; i < categories; ++i)
      pair_sum += static_cast<__int128>(sorted[i]) * (2 * static_cast<__int128>(i) - static_cast<__int128>(categories - 1));
    const double sum_abs = static_cast<double>(pair_sum);
    const double scaling = 1.0 / (static_cast<double>(total) * static_cast<double>(categories - 1));
    out[0] = 1.0 - (scaling * sum_abs);
    if (total == 0) {
      out[1] = 0.0;
      out[2] = 1.0;
      return KGX_OK;
    }
    // HRel: in the order given, the zero-variant term first
    double sum = 0.0;
    if (zero_variant_genomes != 0) {
      const double proportion = static_cast<double>(zero_variant_genomes) / static_cast<double>(total);
      sum = std::log2(proportion) * proportion;
    }
    for (uint64_t i = 0; i < n_runs; ++i) {
      if (run_count[i] == 0) continue;                         // "Unexpected empty genotype": skipped with a warning there
      const double proportion = static_cast<double>(run_count[i]) / static_cast<double>(total);
      sum += std::log2(proportion) * proportion;
    }
    out[1] = (-1.0 * sum) / std::log2(static_cast<double>(categories));
    // IQV
    double proportion = static_cast<double>(zero_variant_genomes) / (static_cast<double>(total) * 100.0);
    double squares = proportion * proportion;
    for (uint64_t i = 0; i < n_runs; ++i) {
      proportion = static_cast<double>(run_count[i]) / (static_cast<double>(total) * 100.0);
      squares += proportion * proportion;
    }
    const double scale = static_cast<double>(categories) / static_cast<double>(categories - 1);
    out[2] = scale * (1.0 - squares);
    return KGX_OK;
  });
}

}  // extern "C"
