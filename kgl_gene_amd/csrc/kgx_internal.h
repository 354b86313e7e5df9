// Internal declarations shared by the C-ABI translation units (kgx_runtime.hip, kgx_dosage.hip, kgx_inbreed.hip, ...), and at
// the end the small helpers that more than one driver uses (EventPair, available_bytes, pair_index, PanelShards).
//
// A Runtime is one binding of the library to a list of devices (kgx_init).  Every handle keeps the Runtime it was
// created under alive and owns one shard per device slot; nothing per-device lives in process globals -- the only
// global is the pointer to the binding new handles are created under.
#ifndef KGX_INTERNAL_H
#define KGX_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kgx.h"

namespace kgx {

// One device slot of a binding: its own stream, scratch arena and timing events.
struct Device {
  int slot = 0;                  // index in Runtime::devs
  int id = -1;                   // HIP ordinal
  int compute_units = 0;
  uint64_t hbm_bytes = 0;
  hipStream_t stream = nullptr;  // the library's stream on this device (non-blocking)
  hipStream_t side_stream = nullptr;   // small per-locus work that runs beside a sweep (the sequential-sum chain)
  hipEvent_t side_begin = nullptr, side_end = nullptr;
  hipEvent_t entries_end = nullptr;    // a large call's table entries, tabulated on the side stream beside the segment defaults
  char name[128] = {0};
  char arch[64] = {0};
  hipEvent_t sweep_begin = nullptr, sweep_end = nullptr;   // bracket the frequency sweep of the last kgx_inbreed call here
  hipEvent_t kernel_begin = nullptr, kernel_end = nullptr; // ... and the one kernel of it that walks the genotype bytes
  hipEvent_t moments_begin = nullptr, moments_end = nullptr;   // ... the class passes of a call that ran on moments (sweeps + merges)
  hipEvent_t search_begin = nullptr, search_end = nullptr;     // ... and the kernel that iterates / searches on them
  hipEvent_t ready = nullptr;                              // cross-stream ordering (kgx_allele_count_by_locus_dev)
  hipEvent_t by_genome_begin = nullptr, by_genome_end = nullptr;   // bracket the K3 kernel of the last by-genome sweep here
  // what the kgx_*_last_* getters report: written by the call that owns `mutex`, read by any thread without it
  std::atomic<double> last_by_genome_ms{0.0};
  std::atomic<double> last_sweep_ms{0.0}, last_kernel_ms{0.0}, last_moments_ms{0.0}, last_search_ms{0.0};
  std::atomic<int> last_evaluations{0};                    // objective evaluations of the last Loglikelihood call here
  std::atomic<int> last_path{0};                           // KGX_PATH_*: what the last kgx_inbreed call here ran on
  // kgx_dosage_last_work: [KGX_WORK_*] = { pieces launched, units in the longest piece, the kernel's period } of the last such launch here
  std::atomic<uint64_t> last_dosage_work[3][3] = {};
  char* scratch = nullptr;                                 // grow-only arena for kgx_inbreed's per-call buffers
  size_t scratch_bytes = 0;
  char* compact[2] = {nullptr, nullptr};                   // ping-pong buffers of the Loglikelihood search's compaction levels
  size_t compact_bytes[2] = {0, 0};
  char* pinned[2] = {nullptr, nullptr};                    // kgx_inbreed_batch: page-locked host images of a batch's inputs / results (grow-only)
  size_t pinned_bytes[2] = {0, 0};
  char* words = nullptr;                                   // Loglikelihood by moments: the class passes' hit bits, [block][genome] (grow-only, like the arena)
  size_t words_bytes = 0;
  char* bits = nullptr;                                    // both estimators by moments: every class's hits as bit rows, [slot][genome / 8] (k_class_bits; grow-only)
  size_t bits_bytes = 0;
  void* exchange_stage = nullptr;                          // "peer" exchange: staging for another shard's counts
  size_t exchange_stage_bytes = 0;
  std::mutex mutex;                                        // serialises the per-device state above between handles
  ~Device();
};

enum class Exchange { None, Rccl, Peer };

struct Runtime {
  std::vector<std::unique_ptr<Device>> devs;
  Exchange exchange = Exchange::None;
  std::vector<void*> comms;       // ncclComm_t per slot (Exchange::Rccl)
  ~Runtime();
};

// The binding new handles are created under (null before kgx_init).
std::shared_ptr<Runtime> current_runtime();
// KGX_ENODEVICE (with the "no CPU fallback" message) until kgx_init has succeeded: the first check of every compute entry point.
int require_bound();

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
const std::string& last_error();
void set_last_error(const std::string& message);
// The KGX_* switches, from the snapshot taken at kgx_init / kgx_reload_options (never from the environment itself).
int env_int(const char* name, int dflt);
std::string env_str(const char* name);
void reload_options();
uint32_t stream_grid(const Device& dev, uint64_t work_items, uint32_t items_per_block);

// Per-call device buffers come out of ONE grow-only arena per device (a window loop calls kgx_inbreed thousands of times, the
// FWS analysis the by-genome sweep once per population: a dozen hipMalloc / hipFree pairs per call cost more than some of
// the sweeps).  The caller holds the device's mutex; kgx_release_scratch frees the arena.
struct ScratchPlan {
  size_t total = 0;
  size_t add(size_t bytes) {
    const size_t at = total;
    total += (bytes + 255u) & ~static_cast<size_t>(255u);
    return at;
  }
};
int scratch_reserve(Device& dev, size_t bytes, char** out);
// A grow-only device buffer kept between calls beside the arena (the hits' words, the classes' bit rows, a compaction level): at
// least `want` bytes behind p afterwards.  Grown by freeing first and only where `want + headroom` bytes are free; where that
// fails p is null, bytes 0, HIP's error cleared and nothing reported (non-zero return): the caller has a path without the buffer.
int grow_device_buffer(char*& p, size_t& bytes, size_t want, size_t headroom);
// ... and a page-locked host buffer of the device (which: 0 inputs, 1 results), grown when needed; the caller holds the mutex.
int pinned_reserve(Device& dev, int which, size_t bytes, char** out);

// Makes `dev` the calling thread's current HIP device.
int use_device(const Device& dev);

// No exception crosses the C ABI (or leaves a worker thread): host containers sized from caller or device values may throw.
template <typename Fn>
int guarded(Fn&& fn) noexcept {
  try {
    return fn();
  } catch (const std::bad_alloc&) {
    return fail(KGX_ENOMEM, "host allocation failed");
  } catch (const std::length_error&) {
    return fail(KGX_ENOMEM, "host allocation failed (size beyond the container's limit)");
  } catch (const std::exception& e) {
    return fail(KGX_ESTATE, "unexpected exception: %s", e.what());
  }
}

// Run fn(i) for i in [0, n): inline when n == 1, otherwise one host thread per item (each shard drives its own device
// and blocks on its own stream).  Returns the first non-zero code; the failing worker's message becomes this thread's.
template <typename Fn>
int for_each_parallel(size_t n, Fn&& fn) {
  if (n == 0) return KGX_OK;
  if (n == 1) return guarded([&]() -> int { return fn(static_cast<size_t>(0)); });
  std::vector<int> codes(n, KGX_OK);
  std::vector<std::string> messages(n);
  std::vector<std::thread> workers;
  workers.reserve(n);
  for (size_t i = 0; i < n; ++i)
    workers.emplace_back([&, i]() {
      codes[i] = guarded([&]() -> int { return fn(i); });         // an exception leaving a thread would end the process
      if (codes[i] != KGX_OK) messages[i] = last_error();
    });
  for (auto& w : workers) w.join();
  for (size_t i = 0; i < n; ++i)
    if (codes[i] != KGX_OK) {
      set_last_error(messages[i]);
      return codes[i];
    }
  return KGX_OK;
}

// Sum d_counts[slot] (uint32 x n_words each, one buffer per slot, in place) over the slots; queued behind the work
// already on each slot's `streams[slot]`, complete on every slot's stream afterwards.
int exchange_counts(Runtime& rt, const std::vector<void*>& d_counts, uint64_t n_words, const std::vector<hipStream_t>& streams);

}  // namespace kgx

// One genome shard of a population on one device slot.
struct kgx_pop_shard {
  kgx::Device* dev = nullptr;
  uint64_t genome_base = 0;      // first genome of the shard (a multiple of 64)
  uint64_t n_genomes = 0;
  uint64_t n_variants = 0;
  uint64_t capacity = 0;         // rows allocated (>= n_variants; kgx_population_resize)
  uint64_t row_bytes = 0;        // ceil(n_genomes / 4): algorithmic bytes per row
  uint64_t pitch = 0;            // device row pitch, multiple of 16
  uint32_t chunks_per_row = 0;   // pitch / 16
  uint8_t* d_alloc = nullptr;    // the hipMalloc'd block holding d_rows
  uint8_t* d_rows = nullptr;     // [n_variants][pitch] dosage2
  float* d_af = nullptr;         // [n_variants] INFO allele frequency (float32, NaN = missing)
  void* d_counts = nullptr;      // [n_variants][4] u32 scratch for the host-returning entry points
  uint8_t* d_keep = nullptr;     // [pitch] genome mask in the rows' own layout: 0b11 where the genome takes part; null = all do
  uint64_t n_kept = 0;           // genomes of the shard taking part (n_genomes without a mask)
  // phase plane (kgx_population_load_phase_plane): one bit per (row, genome of the shard), rows of phase_pitch bytes
  // (a multiple of 16: 128-genome chunks), capacity rows like d_rows; null until a plane is loaded
  uint8_t* d_phase = nullptr;
  uint64_t phase_pitch = 0;
};

struct kgx_pop {
  std::shared_ptr<kgx::Runtime> rt;
  uint64_t n_genomes = 0;        // all shards
  uint64_t n_variants = 0;
  std::vector<kgx_pop_shard> shards;
  bool has_af = false;
  std::vector<uint8_t> keep;     // kgx_population_set_genome_mask: one byte per genome, empty = no mask
  bool counts_current = false;   // with a mask: every shard's d_counts holds the population's K2 counts under it
};

struct kgx_gt8_shard {
  kgx::Device* dev = nullptr;
  uint64_t genome_base = 0;      // first genome of the shard (a multiple of 128)
  uint64_t n_genomes = 0;
  uint64_t n_loci = 0;
  uint64_t pitch = 0;            // bytes per locus row, multiple of 128
  uint8_t* d_gt = nullptr;       // [n_loci][pitch]
  // Does any byte hold an allele index 8..14 (a nibble with bit 3 set that is not 15)?  0 = not looked at since the
  // bytes last changed, 1 = none, 2 = some.  Without them the SWAR sweeps need no guard against indexes past their
  // 8-entry tables (k_scan_wide_nibbles; every flattener output at <= 7 reference alts is such a matrix).
  int wide_nibbles = 0;
  // Offsets with more than 14 reference alts (kgx_gt8_set_wide_rows): their cells as 16-bit pairs of 8-bit indices.
  uint32_t* d_wide_of_row = nullptr;   // [n_loci]: the row's wide row, 0xFFFFFFFF = none; null = the matrix has none
  uint16_t* d_wide = nullptr;          // [n_wide][wide_pitch]
  uint64_t wide_pitch = 0, n_wide = 0;
};

struct kgx_gt8 {
  std::shared_ptr<kgx::Runtime> rt;
  uint64_t n_genomes = 0;
  uint64_t n_loci = 0;
  std::vector<kgx_gt8_shard> shards;
  std::vector<uint32_t> wide_loci;   // the rows that have a wide row (kgx_gt8_set_wide_rows), ascending: what the allele census refuses
};

namespace kgx {
// The row list of a walk along the rows (kgx_roh, kgx_pair_runs) checked, and its break words: bit i & 63 of breaks[i >> 6] = a
// break before list position i (a contig start, or a position step above max_gap != 0).  KGX_EINVAL names the index, after `who`.
int run_breaks(const char* who, const kgx_pop* pop, const uint32_t* rows, uint64_t n_rows, const uint32_t* position, const uint8_t* contig_start,
               uint32_t max_gap, std::vector<unsigned long long>& breaks);
}  // namespace kgx

#define KGX_HIP(call)                                                                             \
  do {                                                                                            \
    hipError_t kgx_err_ = (call);                                                                 \
    if (kgx_err_ != hipSuccess) {                                                                 \
      (void)hipGetLastError();                                                                    \
      return ::kgx::fail(KGX_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(kgx_err_),  \
                         __FILE__, __LINE__);                                                     \
    }                                                                                             \
  } while (0)

#define KGX_HIP_MEM(call)                                                                         \
  do {                                                                                            \
    hipError_t kgx_err_ = (call);                                                                 \
    if (kgx_err_ != hipSuccess) {                                                                 \
      (void)hipGetLastError();                                                                    \
      return ::kgx::fail(KGX_ENOMEM, "%s failed: %s (%s:%d)", #call, hipGetErrorString(kgx_err_), \
                         __FILE__, __LINE__);                                                     \
    }                                                                                             \
  } while (0)

namespace kgx {

// HIP events of one call, destroyed with it.
struct EventPair {
  hipEvent_t begin = nullptr, end = nullptr;
  double ms = 0.0;
  ~EventPair() {
    if (begin) (void)hipEventDestroy(begin);
    if (end) (void)hipEventDestroy(end);
  }
  int create() {
    KGX_HIP(hipEventCreate(&begin));
    KGX_HIP(hipEventCreate(&end));
    return KGX_OK;
  }
  void collect() {
    float t = 0.f;
    if (hipEventElapsedTime(&t, begin, end) == hipSuccess) ms += t;
    else (void)hipGetLastError();
  }
};

// What a call may plan with on the current device (= dev).
inline uint64_t available_bytes(const Device& dev) {
  size_t free_bytes = 0, total_bytes = 0;
  if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) { (void)hipGetLastError(); free_bytes = 0; }
  return static_cast<uint64_t>(free_bytes) + dev.scratch_bytes;          // the arena counts as free: it is re-used
}

// Where the pair a <= b of G genomes sits in a table of genome pairs.
inline uint64_t pair_index(uint64_t a, uint64_t b, uint64_t G) { return a * G - a * (a - 1) / 2 + (b - a); }

// The products over the genome-major panel (kgx_pair_counts, kgx_pair_scores) run on the first shard's device; shards on the same
// HIP device share its stream and arena and write straight into its panel, a shard elsewhere builds its part there (its own copy
// of the row list, its own panel in that device's arena) and copies it over per batch.
struct PanelShard { Device* dev = nullptr; bool foreign = false; const uint32_t* d_list = nullptr; uint8_t* d_panel = nullptr; };
struct PanelShards {
  std::vector<PanelShard> sb;                                 // one per shard of the population
  std::vector<Device*> foreign;                               // the other devices that hold genomes
  std::vector<std::unique_lock<std::mutex>> locks;            // the first device's mutex, then theirs

  explicit PanelShards(const kgx_pop* pop) : sb(pop->shards.size()) {
    Device& cdev = *pop->shards[0].dev;
    for (size_t s = 0; s < pop->shards.size(); ++s) {
      Device* d = pop->shards[s].dev;
      sb[s].foreign = d->id != cdev.id;
      sb[s].dev = sb[s].foreign ? d : &cdev;
      bool known = false;
      for (Device* f : foreign) known = known || f == d;
      if (sb[s].foreign && pop->shards[s].n_genomes && !known) foreign.push_back(d);
    }
    locks.emplace_back(cdev.mutex);
    for (Device* d : foreign) locks.emplace_back(d->mutex);
  }

  // The 64-row tiles of a batch that the other devices have room for: a panel of the shard's genomes (padded to `tile` of them)
  // and the row list within a quarter of (free + arena) there.  Lowers batch_tiles only.
  int fit_elsewhere(const kgx_pop* pop, uint64_t tile, uint64_t list_bytes, uint64_t& batch_tiles) const {
    for (size_t s = 0; s < pop->shards.size(); ++s) {
      if (!sb[s].foreign || pop->shards[s].n_genomes == 0) continue;
      if (int rc = use_device(*sb[s].dev)) return rc;
      const uint64_t shard_padded = (pop->shards[s].n_genomes + tile - 1) / tile * tile, there = available_bytes(*sb[s].dev);
      batch_tiles = std::min(batch_tiles, (there / 4 > list_bytes ? there / 4 - list_bytes : 0) / (shard_padded * 16));
    }
    return KGX_OK;
  }

  // Every shard's list and panel pointers: d_list / d_panel are the first device's (rows null: no list); a shard elsewhere gets
  // its own out of that device's arena, the list copied there.
  int reserve(const kgx_pop* pop, uint64_t tile, const uint32_t* rows, uint64_t list_bytes, const uint32_t* d_list, uint8_t* d_panel, uint64_t panel_pitch) {
    for (size_t s = 0; s < pop->shards.size(); ++s) {
      const kgx_pop_shard& sh = pop->shards[s];
      sb[s].d_list = d_list;
      sb[s].d_panel = d_panel + sh.genome_base * panel_pitch;   // results go straight into the first device's panel
      if (!sb[s].foreign || sh.n_genomes == 0) continue;
      Device& dev = *sh.dev;
      if (int rc = use_device(dev)) return rc;
      ScratchPlan fplan;
      const size_t f_list = fplan.add(list_bytes), f_panel = fplan.add((sh.n_genomes + tile - 1) / tile * tile * panel_pitch);
      char* farena = nullptr;
      if (int rc = scratch_reserve(dev, fplan.total, &farena)) return rc;
      if (rows) {
        KGX_HIP(hipMemcpyAsync(farena + f_list, rows, list_bytes, hipMemcpyHostToDevice, dev.stream));
        KGX_HIP(hipStreamSynchronize(dev.stream));
        sb[s].d_list = reinterpret_cast<const uint32_t*>(farena + f_list);
      }
      sb[s].d_panel = reinterpret_cast<uint8_t*>(farena + f_panel);
    }
    return KGX_OK;
  }
};

}  // namespace kgx

#endif  // KGX_INTERNAL_H
