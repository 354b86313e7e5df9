// C ABI (include/kgx.h) of the windowed joint genotype counts between variant rows: kgx_ld_counts (per list position and distance
// 0 .. window the nine joint counts of the kinds H / M / O over the genomes: Z Z^T on the matrix cores straight from the shards'
// rows, kgx_kernels_ld.h), kgx_ld_counts_last and kgx_ld_statistics (the library's genotype correlation r from those counts, host
// only).  No CPU fallback exists for the device part.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

#include "kgx_kernels_ld.h"
#include "kgx_internal.h"

namespace kgx {
namespace {

std::atomic<double> g_last_ld_ms{0.0};
std::atomic<uint64_t> g_last_ld_batches{0}, g_last_ld_splits{0};

uint32_t segments_of(uint64_t genomes) { return static_cast<uint32_t>((genomes + 64u * kLdSegment - 1) / (64u * kLdSegment)); }

int ld_counts_impl(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, uint32_t window, uint32_t* out) {
  const uint64_t entries = static_cast<uint64_t>(window) + 1, n_blocks = (n_rows + kLdBlock - 1) / kLdBlock;
  const uint64_t band = std::min<uint64_t>((static_cast<uint64_t>(window) + kLdBlock - 1) / kLdBlock, n_blocks - 1);
  const uint64_t block_bytes = kLdBlock * entries * kPairWords * sizeof(uint32_t), list_bytes = rows ? n_rows * sizeof(uint32_t) : 0;

  // ---- devices: shards on the first shard's HIP device share its stream, arena and table; a shard elsewhere fills a table there
  Device& cdev = *pop->shards[0].dev;
  struct ShardBuffers { Device* dev = nullptr; bool foreign = false; const uint32_t* d_list = nullptr; uint32_t* d_table = nullptr; };
  std::vector<ShardBuffers> sb(pop->shards.size());
  std::vector<Device*> foreign;
  uint32_t most_segments = 0;
  for (size_t s = 0; s < pop->shards.size(); ++s) {
    Device* d = pop->shards[s].dev;
    sb[s].foreign = d->id != cdev.id;
    sb[s].dev = sb[s].foreign ? d : &cdev;
    most_segments = std::max(most_segments, segments_of(pop->shards[s].n_genomes));
    if (!sb[s].foreign || pop->shards[s].n_genomes == 0) continue;
    auto same = std::find_if(foreign.begin(), foreign.end(), [&](const Device* f) { return f->id == d->id; });
    if (same == foreign.end()) foreign.push_back(d);
    else sb[s].dev = *same;                                    // one table, stream and arena per HIP device
  }
  std::vector<std::unique_lock<std::mutex>> locks;
  locks.emplace_back(cdev.mutex);
  for (Device* d : foreign) locks.emplace_back(d->mutex);

  // ---- blocks per batch: the batch's part of the table (and, with shards elsewhere, the copy of theirs) within a quarter of
  // (free + arena) on every device
  if (int rc = use_device(cdev)) return rc;
  const uint64_t tables_here = foreign.empty() ? 1 : 2, here = available_bytes(cdev) / 4;
  uint64_t batch_blocks = (here > list_bytes ? here - list_bytes : 0) / (block_bytes * tables_here);
  for (Device* d : foreign) {
    if (int rc = use_device(*d)) return rc;
    const uint64_t there = available_bytes(*d) / 4;
    batch_blocks = std::min(batch_blocks, (there > list_bytes ? there - list_bytes : 0) / block_bytes);
  }
  batch_blocks = std::min<uint64_t>(batch_blocks, 0x7FFFFFFFull / (band + 1));         // block pairs of a batch: gridDim.x
  const int row_cap = env_int("KGX_LD_ROWS", 0);
  if (row_cap > 0) batch_blocks = std::min(batch_blocks, (static_cast<uint64_t>(row_cap) + kLdBlock - 1) / kLdBlock);
  batch_blocks = std::max<uint64_t>(1, std::min(batch_blocks, n_blocks));
  const uint64_t table_bytes = batch_blocks * block_bytes;

  // ---- buffers
  if (int rc = use_device(cdev)) return rc;
  ScratchPlan plan;
  const size_t o_table = plan.add(table_bytes), o_list = plan.add(list_bytes), o_stage = plan.add(foreign.empty() ? 0 : table_bytes);
  char* arena = nullptr;
  if (int rc = scratch_reserve(cdev, plan.total, &arena)) return rc;
  uint32_t* d_table = reinterpret_cast<uint32_t*>(arena + o_table);
  uint32_t* d_stage = reinterpret_cast<uint32_t*>(arena + o_stage);
  const uint32_t* d_list = rows ? reinterpret_cast<const uint32_t*>(arena + o_list) : nullptr;
  if (rows) {
    KGX_HIP(hipMemcpyAsync(arena + o_list, rows, list_bytes, hipMemcpyHostToDevice, cdev.stream));
    KGX_HIP(hipStreamSynchronize(cdev.stream));               // the source is pageable host memory
  }
  for (size_t s = 0; s < pop->shards.size(); ++s) {
    sb[s].d_list = d_list;
    sb[s].d_table = d_table;
  }
  for (Device* d : foreign) {                                  // its own copy of the row list and its own table in that device's arena
    if (int rc = use_device(*d)) return rc;
    ScratchPlan fplan;
    const size_t f_table = fplan.add(table_bytes), f_list = fplan.add(list_bytes);
    char* farena = nullptr;
    if (int rc = scratch_reserve(*d, fplan.total, &farena)) return rc;
    if (rows) {
      KGX_HIP(hipMemcpyAsync(farena + f_list, rows, list_bytes, hipMemcpyHostToDevice, d->stream));
      KGX_HIP(hipStreamSynchronize(d->stream));
    }
    for (size_t s = 0; s < pop->shards.size(); ++s)
      if (sb[s].dev == d) {
        sb[s].d_list = rows ? reinterpret_cast<const uint32_t*>(farena + f_list) : nullptr;
        sb[s].d_table = reinterpret_cast<uint32_t*>(farena + f_table);
      }
  }

  // ---- how the product is cut: block pairs, and the genomes' segments over gridDim.z where the pairs alone leave the device idle
  const uint64_t block_pairs = batch_blocks * (band + 1), wanted = 2ull * static_cast<uint64_t>(std::max(cdev.compute_units, 1));
  uint64_t slices = block_pairs < wanted ? std::min<uint64_t>({(wanted + block_pairs - 1) / block_pairs, most_segments, 65535}) : 1;
  const int slice_cap = env_int("KGX_LD_SPLITS", 0);          // only ever lowers the count: the tests walk several segments in one workgroup with it
  if (slice_cap > 0) slices = std::min(slices, static_cast<uint64_t>(slice_cap));
  slices = std::max<uint64_t>(slices, 1);
  EventPair product_time;
  if (int rc = use_device(cdev)) return rc;
  if (int rc = product_time.create()) return rc;

  uint64_t batches = 0, widest = 1;
  // the shards of one device, in order: the first stores (or, split, all add atomically into a cleared table), the later ones add
  auto run_device = [&](Device& dev, uint64_t block0, uint64_t blocks, uint64_t b0, uint64_t B, EventPair* time) -> int {
    if (int rc = use_device(dev)) return rc;
    bool first = true;
    for (size_t s = 0; s < pop->shards.size(); ++s) {
      const kgx_pop_shard& sh = pop->shards[s];
      if (sb[s].dev != &dev || sh.n_genomes == 0) continue;
      const uint32_t segments = segments_of(sh.n_genomes), per_slice = static_cast<uint32_t>((segments + slices - 1) / slices);
      const uint32_t z = (segments + per_slice - 1) / per_slice;
      const bool split = slices > 1;                          // one rule for the device: a table is either stored into or added into atomically
      if (first) {
        // nobody owns the entries past the list's end; split, every word is added into
        const uint64_t tail0 = split ? b0 : std::max(b0, n_rows > window ? n_rows - window : 0);
        if (tail0 < b0 + B) {
          const uint64_t n_words = (b0 + B - tail0) * entries * kPairWords;
          hipLaunchKernelGGL(k_ld_clear, dim3(stream_grid(dev, n_words, kBlock)), dim3(kBlock), 0, dev.stream, sb[s].d_table + (tail0 - b0) * entries * kPairWords,
                             n_words);
          KGX_HIP(hipGetLastError());
        }
        if (time) KGX_HIP(hipEventRecord(time->begin, dev.stream));
      }
      widest = std::max<uint64_t>(widest, z);
      hipLaunchKernelGGL(k_ld_counts, dim3(static_cast<uint32_t>(blocks * (band + 1)), 1, z), dim3(kBlock), 0, dev.stream,
                         reinterpret_cast<const kgx_v4u*>(sh.d_rows), sh.chunks_per_row, sh.n_genomes, reinterpret_cast<const kgx_v4u*>(sh.d_keep), sb[s].d_list,
                         n_rows, window, static_cast<uint32_t>(band), block0, per_slice, split ? 2 : (first ? 0 : 1), sb[s].d_table);
      KGX_HIP(hipGetLastError());
      first = false;
    }
    if (time && !first) KGX_HIP(hipEventRecord(time->end, dev.stream));
    if (first && &dev == &cdev) {                             // no genome here: the other devices' tables are added into zeros
      hipLaunchKernelGGL(k_ld_clear, dim3(stream_grid(dev, B * entries * kPairWords, kBlock)), dim3(kBlock), 0, dev.stream, d_table, B * entries * kPairWords);
      KGX_HIP(hipGetLastError());
    }
    return KGX_OK;
  };
  for (uint64_t block0 = 0; block0 < n_blocks; block0 += batch_blocks, ++batches) {
    const uint64_t blocks = std::min(batch_blocks, n_blocks - block0), b0 = block0 * kLdBlock, B = std::min(blocks * kLdBlock, n_rows - b0);
    const uint64_t words = B * entries * kPairWords;
    for (Device* d : foreign)
      if (int rc = run_device(*d, block0, blocks, b0, B, nullptr)) return rc;
    if (int rc = run_device(cdev, block0, blocks, b0, B, &product_time)) return rc;
    for (Device* d : foreign) {                                // one staging table: a device at a time
      if (int rc = use_device(*d)) return rc;
      uint32_t* theirs = nullptr;
      for (size_t s = 0; s < pop->shards.size(); ++s)
        if (sb[s].dev == d) theirs = sb[s].d_table;
      KGX_HIP(hipMemcpyAsync(d_stage, theirs, words * sizeof(uint32_t), hipMemcpyDefault, d->stream));
      KGX_HIP(hipStreamSynchronize(d->stream));
      if (int rc = use_device(cdev)) return rc;
      hipLaunchKernelGGL(k_ld_add, dim3(stream_grid(cdev, words, kBlock)), dim3(kBlock), 0, cdev.stream, d_table, d_stage, words);
      KGX_HIP(hipGetLastError());
      KGX_HIP(hipStreamSynchronize(cdev.stream));
    }
    if (int rc = use_device(cdev)) return rc;
    KGX_HIP(hipMemcpyAsync(out + b0 * entries * kPairWords, d_table, words * sizeof(uint32_t), hipMemcpyDeviceToHost, cdev.stream));
    KGX_HIP(hipStreamSynchronize(cdev.stream));               // the next batch overwrites the table
    product_time.collect();
  }
  g_last_ld_ms = product_time.ms;
  g_last_ld_batches = batches;
  g_last_ld_splits = widest;
  return KGX_OK;
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" {

int kgx_ld_counts(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, uint32_t window, uint32_t* out) {
  return guarded([&]() -> int {
    if (int bound = require_bound()) return bound;
    if (!pop || (!out && n_rows)) return fail(KGX_EINVAL, "ld_counts: null argument (pop and out are required)");
    if (!rows && n_rows > pop->n_variants)
      return fail(KGX_EINVAL, "ld_counts: n_rows %llu exceeds the population's %llu rows", (unsigned long long)n_rows, (unsigned long long)pop->n_variants);
    for (uint64_t i = 0; rows && i < n_rows; ++i)
      if (rows[i] >= pop->n_variants)
        return fail(KGX_EINVAL, "ld_counts: rows[%llu] = %u is not a row of the population's %llu", (unsigned long long)i, rows[i],
                    (unsigned long long)pop->n_variants);
    uint64_t bytes = 0;
    if (__builtin_mul_overflow(n_rows, (static_cast<uint64_t>(window) + 1) * kPairWords * sizeof(uint32_t), &bytes) ||
        n_rows > std::numeric_limits<uint64_t>::max() - kLdBlock)
      return fail(KGX_EINVAL, "ld_counts: the table of %llu rows x %llu distances overflows 64 bits", (unsigned long long)n_rows, (unsigned long long)window + 1);
    g_last_ld_ms = 0.0;
    g_last_ld_batches = 0;
    g_last_ld_splits = 0;
    if (n_rows == 0) return KGX_OK;
    bool any = false;
    for (const auto& sh : pop->shards) any = any || sh.n_genomes != 0;
    if (!any) {
      std::memset(out, 0, bytes);
      return KGX_OK;
    }
    const int rc = ld_counts_impl(pop, rows, n_rows, window, out);
    (void)use_device(*pop->shards[0].dev);
    return rc;
  });
}

int kgx_ld_counts_last(double* kernel_ms, uint64_t* row_batches, uint64_t* genome_splits) {
  if (kernel_ms) *kernel_ms = g_last_ld_ms.load();
  if (row_batches) *row_batches = g_last_ld_batches.load();
  if (genome_splits) *genome_splits = g_last_ld_splits.load();
  return KGX_OK;
}

// This translation unit is built with floating contraction off.  cov, vx and vy are exact 128-bit integers; r is three
// conversions, one multiplication, one square root and one division in fp64.
int kgx_ld_statistics(const uint32_t* counts, uint64_t n_rows, uint32_t window, uint64_t n_genomes, double* r) {
  return guarded([&]() -> int {
    if (n_rows && (!counts || !r)) return fail(KGX_EINVAL, "ld_statistics: null argument");
    const uint64_t entries = static_cast<uint64_t>(window) + 1;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (uint64_t i = 0; i < n_rows; ++i) {
      const uint32_t* own_i = counts + i * entries * kPairWords;
      for (uint64_t d = 0; d < entries; ++d) {
        double& value = r[i * entries + d];
        value = nan;
        if (d >= n_rows - i) continue;                          // past the list's end
        const uint32_t *own_j = counts + (i + d) * entries * kPairWords, *n = own_i + d * kPairWords;   // n[3 p + q]: row i has kind p, row j kind q
        typedef __int128 wide;
        const wide N = static_cast<wide>(n_genomes) - own_i[8] - own_j[8] + n[8];
        const wide hx = static_cast<wide>(own_i[0]) - n[2], mx = static_cast<wide>(own_i[4]) - n[5];
        const wide hy = static_cast<wide>(own_j[0]) - n[6], my = static_cast<wide>(own_j[4]) - n[7];
        const wide Sx = hx + 2 * mx, Sxx = hx + 4 * mx, Sy = hy + 2 * my, Syy = hy + 4 * my;
        const wide Sxy = static_cast<wide>(n[0]) + 2 * static_cast<wide>(n[1]) + 2 * static_cast<wide>(n[3]) + 4 * static_cast<wide>(n[4]);
        const wide cov = N * Sxy - Sx * Sy, vx = N * Sxx - Sx * Sx, vy = N * Syy - Sy * Sy;
        if (N <= 0 || vx <= 0 || vy <= 0) continue;             // nobody jointly called, or a constant row (negative: not a table of kgx_ld_counts)
        value = static_cast<double>(cov) / std::sqrt(static_cast<double>(vx) * static_cast<double>(vy));
      }
    }
    return KGX_OK;
  });
}

}  // extern "C"
