// C ABI (include/kgx.h) of the association scan: kgx_column_sums (per listed row and per caller-supplied genome column the sum of
// the column over the genomes of each kind H / M / O: the indicator rows times signed base-128 digits of the columns on the matrix
// cores straight from the shards' rows, kgx_kernels_assoc.h), kgx_column_sums_last, and the host-only companions kgx_assoc_columns
// (traits to fixed-point columns) and kgx_assoc_statistics (the library's single-variant regression from the sums).  No CPU
// fallback exists for the device part.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <vector>

#include "kgx_kernels_assoc.h"
#include "kgx_internal.h"

namespace kgx {
namespace {

std::atomic<double> g_last_assoc_ms{0.0};
std::atomic<uint64_t> g_last_assoc_batches{0}, g_last_assoc_splits{0};

uint32_t segments_of(uint64_t genomes) { return static_cast<uint32_t>((genomes + 64u * kAssocSegment - 1) / (64u * kAssocSegment)); }

// The fewest digits in [-64, 63] that hold every value of lo .. hi: D digits hold -64 S .. 63 S, S = (128^D - 1) / 127.
uint32_t digits_for(int32_t lo, int32_t hi) {
  int64_t span = 1;
  for (uint32_t d = 1; d < kAssocDigits; ++d, span = span * 128 + 1)
    if (lo >= -64 * span && hi <= 63 * span) return d;
  return kAssocDigits;
}

// The tile words of the columns' groups of 16 and the passes' first tiles: whole groups, at most kAssocTiles tiles a pass.
void plan_tiles(const int32_t* columns, uint64_t G, uint32_t n_columns, std::vector<uint32_t>& tiles, std::vector<uint32_t>& pass_first) {
  pass_first.assign(1, 0u);
  for (uint32_t group = 0; static_cast<uint64_t>(group) * 16 < n_columns; ++group) {
    int32_t lo = 0, hi = 0;
    const uint64_t j_end = std::min<uint64_t>(static_cast<uint64_t>(group) * 16 + 16, n_columns);
    for (uint64_t j = static_cast<uint64_t>(group) * 16; j < j_end; ++j)
      for (uint64_t g = 0; g < G; ++g) {
        lo = std::min(lo, columns[j * G + g]);
        hi = std::max(hi, columns[j * G + g]);
      }
    const uint32_t digits = digits_for(lo, hi);
    if (tiles.size() + digits - pass_first.back() > kAssocTiles) pass_first.push_back(static_cast<uint32_t>(tiles.size()));
    for (uint32_t d = 0; d < digits; ++d) tiles.push_back(group | d << 28);
  }
  pass_first.push_back(static_cast<uint32_t>(tiles.size()));
}

int column_sums_impl(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, const int32_t* columns, uint32_t n_columns, int64_t* out) {
  const uint64_t G = pop->n_genomes, n_blocks = (n_rows + kAssocBlock - 1) / kAssocBlock;
  const uint64_t row_words = static_cast<uint64_t>(n_columns) * kPairKinds, block_bytes = kAssocBlock * row_words * sizeof(int64_t);
  const uint64_t list_bytes = rows ? n_rows * sizeof(uint32_t) : 0, column_bytes = static_cast<uint64_t>(n_columns) * G * sizeof(int32_t);
  std::vector<uint32_t> tiles, pass_first;
  plan_tiles(columns, G, n_columns, tiles, pass_first);
  const uint64_t n_tiles = tiles.size(), passes = pass_first.size() - 1;
  if (passes > 65535) return fail(KGX_EINVAL, "column_sums: %u columns make %llu passes of tiles, more than a grid holds", n_columns, (unsigned long long)passes);
  const uint64_t plan_bytes = (n_tiles + passes + 1) * sizeof(uint32_t) + 256;

  // ---- devices: shards on the first shard's HIP device share its stream, arena and table; a shard elsewhere fills a table there
  Device& cdev = *pop->shards[0].dev;
  struct ShardBuffers { Device* dev = nullptr; uint32_t segments = 0; uint64_t units = 0; kgx_v4u* d_operands = nullptr; };
  struct DeviceBuffers { const uint32_t *d_list = nullptr, *d_tiles = nullptr, *d_pass_first = nullptr; long long* d_table = nullptr; uint64_t operand_bytes = 0; };
  std::vector<ShardBuffers> sb(pop->shards.size());
  std::vector<Device*> devices(1, &cdev);                      // the first device, then the others that hold genomes
  uint32_t most_segments = 0;
  for (size_t s = 0; s < pop->shards.size(); ++s) {
    Device* d = pop->shards[s].dev;
    sb[s].dev = d->id == cdev.id ? &cdev : d;
    sb[s].segments = segments_of(pop->shards[s].n_genomes);
    sb[s].units = static_cast<uint64_t>(sb[s].segments) * kAssocSegment * n_tiles * kWave;
    most_segments = std::max(most_segments, sb[s].segments);
    if (pop->shards[s].n_genomes == 0) continue;
    auto same = std::find_if(devices.begin(), devices.end(), [&](const Device* f) { return f->id == d->id; });
    if (same == devices.end()) devices.push_back(d);
    else sb[s].dev = *same;                                    // one table, stream and arena per HIP device
  }
  std::vector<DeviceBuffers> db(devices.size());
  std::vector<std::unique_lock<std::mutex>> locks;
  for (Device* d : devices) locks.emplace_back(d->mutex);
  for (size_t s = 0; s < sb.size(); ++s)
    for (size_t k = 0; k < devices.size(); ++k)
      if (sb[s].dev == devices[k]) db[k].operand_bytes += (sb[s].units * sizeof(kgx_v4u) + 255u) & ~255ull;
  const bool elsewhere = devices.size() > 1;

  // ---- blocks per batch: the batch's part of the table (and, with shards elsewhere, the copy of theirs) within a quarter of
  // (free + arena) on every device, beside the list, the columns and their operands
  uint64_t batch_blocks = n_blocks;
  for (size_t k = 0; k < devices.size(); ++k) {
    if (int rc = use_device(*devices[k])) return rc;
    const uint64_t quarter = available_bytes(*devices[k]) / 4, fixed = list_bytes + column_bytes + db[k].operand_bytes + plan_bytes;
    batch_blocks = std::min(batch_blocks, (quarter > fixed ? quarter - fixed : 0) / (block_bytes * (k == 0 && elsewhere ? 2 : 1)));
  }
  batch_blocks = std::min<uint64_t>(batch_blocks, 0x7FFFFFFFull);                      // gridDim.x
  const int row_cap = env_int("KGX_ASSOC_ROWS", 0);
  if (row_cap > 0) batch_blocks = std::min(batch_blocks, (static_cast<uint64_t>(row_cap) + kAssocBlock - 1) / kAssocBlock);
  batch_blocks = std::max<uint64_t>(1, batch_blocks);
  const uint64_t table_bytes = batch_blocks * block_bytes;

  // ---- buffers, and every shard's column operands (once per call)
  long long* d_stage = nullptr;
  for (size_t k = 0; k < devices.size(); ++k) {
    Device& dev = *devices[k];
    if (int rc = use_device(dev)) return rc;
    ScratchPlan plan;
    const size_t o_table = plan.add(table_bytes), o_stage = plan.add(k == 0 && elsewhere ? table_bytes : 0), o_list = plan.add(list_bytes);
    const size_t o_tiles = plan.add(n_tiles * sizeof(uint32_t)), o_passes = plan.add((passes + 1) * sizeof(uint32_t)), o_columns = plan.add(column_bytes);
    const size_t o_operands = plan.add(db[k].operand_bytes);
    char* arena = nullptr;
    if (int rc = scratch_reserve(dev, plan.total, &arena)) return rc;
    db[k].d_table = reinterpret_cast<long long*>(arena + o_table);
    if (k == 0) d_stage = reinterpret_cast<long long*>(arena + o_stage);
    db[k].d_list = rows ? reinterpret_cast<const uint32_t*>(arena + o_list) : nullptr;
    db[k].d_tiles = reinterpret_cast<const uint32_t*>(arena + o_tiles);
    db[k].d_pass_first = reinterpret_cast<const uint32_t*>(arena + o_passes);
    if (rows) KGX_HIP(hipMemcpyAsync(arena + o_list, rows, list_bytes, hipMemcpyHostToDevice, dev.stream));
    KGX_HIP(hipMemcpyAsync(arena + o_tiles, tiles.data(), n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, dev.stream));
    KGX_HIP(hipMemcpyAsync(arena + o_passes, pass_first.data(), (passes + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, dev.stream));
    KGX_HIP(hipMemcpyAsync(arena + o_columns, columns, column_bytes, hipMemcpyHostToDevice, dev.stream));
    KGX_HIP(hipStreamSynchronize(dev.stream));                 // the sources are pageable host memory
    size_t at = o_operands;
    for (size_t s = 0; s < pop->shards.size(); ++s) {
      const kgx_pop_shard& sh = pop->shards[s];
      if (sb[s].dev != &dev || sh.n_genomes == 0) continue;
      sb[s].d_operands = reinterpret_cast<kgx_v4u*>(arena + at);
      at += (sb[s].units * sizeof(kgx_v4u) + 255u) & ~static_cast<size_t>(255u);
      hipLaunchKernelGGL(k_column_operands, dim3(stream_grid(dev, sb[s].units, kBlock)), dim3(kBlock), 0, dev.stream, reinterpret_cast<const int32_t*>(arena + o_columns), G,
                         sh.genome_base, sh.n_genomes, n_columns, sh.d_keep, db[k].d_tiles, static_cast<uint32_t>(n_tiles), sb[s].units, sb[s].d_operands);
      KGX_HIP(hipGetLastError());
    }
  }

  // ---- how the product is cut: row blocks x passes, and the genomes' segments over gridDim.z where those alone leave the device idle
  const uint64_t work = std::min(batch_blocks, n_blocks) * passes, wanted = 2ull * static_cast<uint64_t>(std::max(cdev.compute_units, 1));
  uint64_t slices = work < wanted ? std::min<uint64_t>({(wanted + work - 1) / work, most_segments, 65535}) : 1;
  const int slice_cap = env_int("KGX_ASSOC_SPLITS", 0);       // only ever lowers the count: the tests walk several segments in one workgroup with it
  if (slice_cap > 0) slices = std::min(slices, static_cast<uint64_t>(slice_cap));
  slices = std::max<uint64_t>(slices, 1);
  const bool split = slices > 1;                              // one rule for the call: a table is either stored into or added into atomically
  EventPair product_time;
  if (int rc = use_device(cdev)) return rc;
  if (int rc = product_time.create()) return rc;

  uint64_t batches = 0, widest = 1;
  // the shards of one device, in order: the first stores (or, split, all add atomically into a cleared table), the later ones add
  auto run_device = [&](size_t k, uint64_t block0, uint64_t blocks, uint64_t B) -> int {
    Device& dev = *devices[k];
    if (int rc = use_device(dev)) return rc;
    bool first = true;
    for (size_t s = 0; s < pop->shards.size(); ++s) {
      const kgx_pop_shard& sh = pop->shards[s];
      if (sb[s].dev != &dev || sh.n_genomes == 0) continue;
      const uint32_t per_slice = static_cast<uint32_t>((sb[s].segments + slices - 1) / slices), z = (sb[s].segments + per_slice - 1) / per_slice;
      if (first) {
        if (split) {
          hipLaunchKernelGGL(k_assoc_clear, dim3(stream_grid(dev, B * row_words, kBlock)), dim3(kBlock), 0, dev.stream, db[k].d_table, B * row_words);
          KGX_HIP(hipGetLastError());
        }
        if (k == 0) KGX_HIP(hipEventRecord(product_time.begin, dev.stream));
      }
      widest = std::max<uint64_t>(widest, z);
      hipLaunchKernelGGL(k_column_sums, dim3(static_cast<uint32_t>(blocks), static_cast<uint32_t>(passes), z), dim3(kBlock), 0, dev.stream,
                         reinterpret_cast<const kgx_v4u*>(sh.d_rows), sh.chunks_per_row, db[k].d_list, n_rows, block0, sb[s].d_operands, db[k].d_tiles,
                         static_cast<uint32_t>(n_tiles), db[k].d_pass_first, n_columns, sb[s].segments, per_slice, split ? 2 : (first ? 0 : 1), db[k].d_table);
      KGX_HIP(hipGetLastError());
      first = false;
    }
    if (k == 0 && !first) KGX_HIP(hipEventRecord(product_time.end, dev.stream));
    if (k == 0 && first) {                                    // no genome here: the other devices' tables are added into zeros
      hipLaunchKernelGGL(k_assoc_clear, dim3(stream_grid(dev, B * row_words, kBlock)), dim3(kBlock), 0, dev.stream, db[k].d_table, B * row_words);
      KGX_HIP(hipGetLastError());
    }
    return KGX_OK;
  };
  for (uint64_t block0 = 0; block0 < n_blocks; block0 += batch_blocks, ++batches) {
    const uint64_t blocks = std::min(batch_blocks, n_blocks - block0), b0 = block0 * kAssocBlock, B = std::min(blocks * kAssocBlock, n_rows - b0);
    const uint64_t words = B * row_words;
    for (size_t k = devices.size(); k-- > 0;)
      if (int rc = run_device(k, block0, blocks, B)) return rc;
    for (size_t k = 1; k < devices.size(); ++k) {              // one staging table: a device at a time
      if (int rc = use_device(*devices[k])) return rc;
      KGX_HIP(hipMemcpyAsync(d_stage, db[k].d_table, words * sizeof(int64_t), hipMemcpyDefault, devices[k]->stream));
      KGX_HIP(hipStreamSynchronize(devices[k]->stream));
      if (int rc = use_device(cdev)) return rc;
      hipLaunchKernelGGL(k_assoc_add, dim3(stream_grid(cdev, words, kBlock)), dim3(kBlock), 0, cdev.stream, db[0].d_table, d_stage, words);
      KGX_HIP(hipGetLastError());
      KGX_HIP(hipStreamSynchronize(cdev.stream));
    }
    if (int rc = use_device(cdev)) return rc;
    KGX_HIP(hipMemcpyAsync(out + b0 * row_words, db[0].d_table, words * sizeof(int64_t), hipMemcpyDeviceToHost, cdev.stream));
    KGX_HIP(hipStreamSynchronize(cdev.stream));               // the next batch overwrites the table
    product_time.collect();
  }
  g_last_assoc_ms = product_time.ms;
  g_last_assoc_batches = batches;
  g_last_assoc_splits = widest;
  return KGX_OK;
}

// ---- exact integers past 128 bits for kgx_assoc_statistics: a * b of two non-negative 128-bit values as four 64-bit limbs
typedef __int128 wide;
typedef unsigned __int128 uwide;
struct Limbs { uint64_t w[4]; };

Limbs product(uwide a, uwide b) {
  const uint64_t al = static_cast<uint64_t>(a), ah = static_cast<uint64_t>(a >> 64), bl = static_cast<uint64_t>(b), bh = static_cast<uint64_t>(b >> 64);
  const uwide ll = static_cast<uwide>(al) * bl, lh = static_cast<uwide>(al) * bh, hl = static_cast<uwide>(ah) * bl, hh = static_cast<uwide>(ah) * bh;
  Limbs r;
  r.w[0] = static_cast<uint64_t>(ll);
  const uwide mid = (ll >> 64) + static_cast<uint64_t>(lh) + static_cast<uint64_t>(hl);
  r.w[1] = static_cast<uint64_t>(mid);
  const uwide top = hh + (lh >> 64) + (hl >> 64) + (mid >> 64);
  r.w[2] = static_cast<uint64_t>(top);
  r.w[3] = static_cast<uint64_t>(top >> 64);
  return r;
}

// a - b for a >= b
Limbs difference(const Limbs& a, const Limbs& b) {
  Limbs r;
  uint64_t borrow = 0;
  for (int i = 0; i < 4; ++i) {
    const uint64_t d = a.w[i] - b.w[i], e = d - borrow;
    borrow = (a.w[i] < b.w[i]) || (d < borrow);
    r.w[i] = e;
  }
  return r;
}

// The nearest double: the value is cut to its top 128 bits with a sticky last bit, far below the place where a double rounds.
double to_double(const Limbs& v) {
  int top = 3;
  while (top > 1 && v.w[top] == 0) --top;
  uwide head = static_cast<uwide>(v.w[top]) << 64 | v.w[top - 1];
  for (int i = 0; i < top - 1; ++i)
    if (v.w[i]) head |= 1;
  return std::ldexp(static_cast<double>(head), 64 * (top - 1));
}

}  // namespace
}  // namespace kgx

using namespace kgx;

extern "C" {

int kgx_column_sums(kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, const int32_t* columns, uint32_t n_columns, int64_t* out) {
  return guarded([&]() -> int {
    if (int bound = require_bound()) return bound;
    if (!pop || (n_rows && (!out || !columns))) return fail(KGX_EINVAL, "column_sums: null argument (pop, columns and out are required)");
    if (n_rows && n_columns == 0) return fail(KGX_EINVAL, "column_sums: no columns");
    uint64_t bytes = 0, column_bytes = 0;                      // before the list is walked: a size that overflows is no list's
    if (__builtin_mul_overflow(n_rows, static_cast<uint64_t>(n_columns) * kPairKinds * sizeof(int64_t), &bytes) ||
        __builtin_mul_overflow(pop->n_genomes, static_cast<uint64_t>(n_columns) * sizeof(int32_t), &column_bytes) ||
        n_rows > std::numeric_limits<uint64_t>::max() - kAssocBlock)
      return fail(KGX_EINVAL, "column_sums: the table of %llu rows x %u columns overflows 64 bits", (unsigned long long)n_rows, n_columns);
    if (!rows && n_rows > pop->n_variants)
      return fail(KGX_EINVAL, "column_sums: n_rows %llu exceeds the population's %llu rows", (unsigned long long)n_rows, (unsigned long long)pop->n_variants);
    for (uint64_t i = 0; rows && i < n_rows; ++i)
      if (rows[i] >= pop->n_variants)
        return fail(KGX_EINVAL, "column_sums: rows[%llu] = %u is not a row of the population's %llu", (unsigned long long)i, rows[i],
                    (unsigned long long)pop->n_variants);
    g_last_assoc_ms = 0.0;
    g_last_assoc_batches = 0;
    g_last_assoc_splits = 0;
    if (n_rows == 0) return KGX_OK;
    for (const auto& sh : pop->shards)
      if (sh.n_genomes > (1ull << 25))
        return fail(KGX_EINVAL, "column_sums: a shard of %llu genomes is above the 2^25 one int32 accumulation holds", (unsigned long long)sh.n_genomes);
    for (uint32_t j = 0; j < n_columns; ++j)
      for (uint64_t g = 0; g < pop->n_genomes; ++g) {
        const int32_t w = columns[static_cast<uint64_t>(j) * pop->n_genomes + g];
        if (w > KGX_COLUMN_MAX || w < -KGX_COLUMN_MAX)
          return fail(KGX_EINVAL, "column_sums: columns[%u][%llu] = %d is not within +-%d", j, (unsigned long long)g, w, KGX_COLUMN_MAX);
      }
    bool any = false;
    for (const auto& sh : pop->shards) any = any || sh.n_genomes != 0;
    if (!any) {
      std::memset(out, 0, bytes);
      return KGX_OK;
    }
    const int rc = column_sums_impl(pop, rows, n_rows, columns, n_columns, out);
    (void)use_device(*pop->shards[0].dev);
    return rc;
  });
}

int kgx_column_sums_last(double* kernel_ms, uint64_t* row_batches, uint64_t* genome_splits) {
  if (kernel_ms) *kernel_ms = g_last_assoc_ms.load();
  if (row_batches) *row_batches = g_last_assoc_batches.load();
  if (genome_splits) *genome_splits = g_last_assoc_splits.load();
  return KGX_OK;
}

// This translation unit is built with floating contraction off: the scaling is exact and llrint rounds to nearest even.
int kgx_assoc_columns(const double* y, uint64_t n_genomes, uint32_t n_traits, int* scale_bits, int32_t* columns) {
  return guarded([&]() -> int {
    const uint64_t n = static_cast<uint64_t>(n_traits) * n_genomes;
    if (!scale_bits || (n && (!y || !columns))) return fail(KGX_EINVAL, "assoc_columns: null argument");
    if (*scale_bits > 12) return fail(KGX_EINVAL, "assoc_columns: scale_bits %d is above 12", *scale_bits);
    // the largest |y| decides whether a scale fits: rounding is monotonic
    double largest = 0.0;
    uint64_t largest_at = 0;
    for (uint64_t i = 0; i < n; ++i) {
      if (!std::isfinite(y[i]))
        return fail(KGX_EINVAL, "assoc_columns: y[%llu][%llu] is not finite", (unsigned long long)(i / n_genomes), (unsigned long long)(i % n_genomes));
      if (std::fabs(y[i]) > largest) { largest = std::fabs(y[i]); largest_at = i; }
    }
    auto fits = [&](int s) {
      const double scaled = std::ldexp(largest, s);
      return scaled < 8129.0 && std::llrint(scaled) <= 8128;
    };
    int s = *scale_bits;
    if (s < 0) {
      s = 12;
      while (s > 0 && !fits(s)) --s;
    }
    if (!fits(s))
      return fail(KGX_EINVAL, "assoc_columns: y[%llu][%llu] = %g at scale_bits %d exceeds 8128", (unsigned long long)(n_genomes ? largest_at / n_genomes : 0),
                  (unsigned long long)(n_genomes ? largest_at % n_genomes : 0), y[largest_at], s);
    for (uint64_t i = 0; i < n; ++i) {
      const int32_t q = static_cast<int32_t>(std::llrint(std::ldexp(y[i], s)));
      columns[i] = q;
      columns[n + i] = q * q;
    }
    *scale_bits = s;
    return KGX_OK;
  });
}

// Every moment is an exact integer; cov, vx, vy in 128 bits, vx vy - cov^2 in 256.  beta is two conversions, one division and an
// exact scaling; t is two conversions, two square roots, one division and one multiplication in fp64.
int kgx_assoc_statistics(const int64_t* sums, const uint32_t* row_counts, uint64_t n_rows, const int32_t* columns, const uint8_t* keep, uint64_t n_genomes,
                         uint32_t n_traits, int scale_bits, double* beta, double* t) {
  return guarded([&]() -> int {
    if (scale_bits < 0 || scale_bits > 12) return fail(KGX_EINVAL, "assoc_statistics: scale_bits %d is not in 0 .. 12", scale_bits);
    if (n_traits && n_genomes && !columns) return fail(KGX_EINVAL, "assoc_statistics: null columns");
    if (n_rows && n_traits && (!sums || !row_counts || !beta || !t)) return fail(KGX_EINVAL, "assoc_statistics: null argument");
    const uint64_t C = 2ull * n_traits;
    std::vector<wide> total(C, 0);                             // of every column over the kept genomes
    for (uint64_t j = 0; j < C; ++j)
      for (uint64_t g = 0; g < n_genomes; ++g)
        if (!keep || keep[g]) total[j] += columns[j * n_genomes + g];
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (uint64_t i = 0; i < n_rows; ++i) {
      const uint32_t* c = row_counts + 4 * i;
      const wide N = static_cast<wide>(c[0]) + c[1] + c[2], Sx = static_cast<wide>(c[1]) + 2 * static_cast<wide>(c[2]);
      const wide Sxx = static_cast<wide>(c[1]) + 4 * static_cast<wide>(c[2]), vx = N * Sxx - Sx * Sx;
      for (uint32_t k = 0; k < n_traits; ++k) {
        const int64_t *q = sums + (i * C + k) * kPairKinds, *qq = sums + (i * C + n_traits + k) * kPairKinds;   // {H, M, O} of q and of q^2
        double &b = beta[i * n_traits + k], &value = t[i * n_traits + k];
        b = value = nan;
        const wide Sy = total[k] - q[2], Sxy = static_cast<wide>(q[0]) + 2 * static_cast<wide>(q[1]), Syy = total[n_traits + k] - qq[2];
        const wide cov = N * Sxy - Sx * Sy, vy = N * Syy - Sy * Sy;
        if (N < 3 || vx <= 0 || vy <= 0) continue;              // too few called genomes, a monomorphic row or a constant trait (negative: not sums of these columns)
        b = std::ldexp(static_cast<double>(cov) / static_cast<double>(vx), -scale_bits);
        const uwide magnitude = cov < 0 ? static_cast<uwide>(-cov) : static_cast<uwide>(cov);
        const Limbs squares = product(static_cast<uwide>(vx), static_cast<uwide>(vy)), square = product(magnitude, magnitude);
        const Limbs rest = difference(squares, square);         // >= 0 (Cauchy-Schwarz)
        if ((rest.w[0] | rest.w[1] | rest.w[2] | rest.w[3]) == 0) value = cov < 0 ? -inf : inf;
        else value = static_cast<double>(cov) / std::sqrt(to_double(rest)) * std::sqrt(static_cast<double>(N - 2));
      }
    }
    return KGX_OK;
  });
}

}  // extern "C"
