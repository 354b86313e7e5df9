// The device buffers of one kgx_inbreed call, typed, and the ONE place that lays them out in the arena.  Host-only (no HIP call):
// included by kgx_inbreed.hip behind the kernel headers, whose structs the buffers hold.
#ifndef KGX_INBREED_BUFFERS_H
#define KGX_INBREED_BUFFERS_H

#include <type_traits>

#include "kgx_inbreed_plan.h"
#include "kgx_internal.h"
#include "kgx_kernels_loglik.h"

namespace kgx {

// A run-time value as a compile-time constant of a generic lambda: with_bool(b, [&](auto B) { k<decltype(B)::value> ... }),
// with_int<4, 8>(v, ...) for the listed values (any other: nothing is called).  Each call site instantiates exactly the
// combinations its lambdas name.
template <typename Fn>
void with_bool(bool value, Fn&& fn) {
  if (value) fn(std::true_type{}); else fn(std::false_type{});
}
template <int... Values, typename Fn>
void with_int(int value, Fn&& fn) {
  (void)((value == Values ? (fn(std::integral_constant<int, Values>{}), true) : false) || ...);
}

// Scratch comes out of one grow-only device arena kept by the library (a window loop calls this hundreds of times;
// fourteen hipMalloc/hipFree pairs per call cost more than the sweep).  The call is synchronous, so reuse is safe.
// A Carver hands the regions out in order: without a base it only adds up their sizes (what the arena must hold), with the
// arena it yields the pointers -- the same function lays the buffers out both times.
struct Carver {
  char* base = nullptr;
  ScratchPlan plan;
  template <typename T>
  T* take(size_t bytes) {
    const size_t at = plan.add(bytes);
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
};

// What every call has.
struct InbreedBuffers {
  double *d_af = nullptr, *d_table = nullptr;
  uint8_t* d_valid = nullptr;
  uint32_t* d_meta = nullptr;
  double *d_part = nullptr, *d_segdef = nullptr, *d_sums = nullptr;
  unsigned long long* d_counts = nullptr;   // counts | F | the flag/counter word | locus index: adjacent, cleared by one memset
  double* d_f = nullptr;
  unsigned int* d_running = nullptr;
  uint32_t* d_index_slot = nullptr;         // (the call's d_index if it has a locus index)
  char* cleared_end = nullptr;
  double* d_eval = nullptr;
  LocusResultsDev* d_out = nullptr;
  GoldenState* d_golden = nullptr;
  BrentState* d_brent = nullptr;
  double *d_start = nullptr, *d_keep = nullptr;
  double* d_seq_sum = nullptr;
  int* d_seq_e = nullptr;
  long long* d_seq_n = nullptr;
  double* d_seq_out = nullptr;
  EvalEntry* d_entries = nullptr;
  unsigned long long* d_segcnt = nullptr;
};

inline InbreedBuffers carve_buffers(Carver& c, const InbreedShape& s, const InbreedPlan& p) {
  const uint64_t n = s.n, n_sel = s.n_sel, n_tab = n_sel ? n_sel : 1;
  InbreedBuffers b;
  b.d_af = c.take<double>(n_tab * s.amax * sizeof(double));
  b.d_table = c.take<double>(n_tab * sweep_stride(s.amax) * sizeof(double));
  b.d_valid = c.take<uint8_t>(n_tab);
  b.d_meta = c.take<uint32_t>((n_tab + 8) * sizeof(uint32_t));
  b.d_part = c.take<double>(p.max_seg * n * kParts0 * sizeof(double));
  b.d_segdef = c.take<double>(p.max_seg * kSegDefaults * sizeof(double));
  b.d_sums = c.take<double>(n * kParts0 * sizeof(double));
  // counts | F | the flag/counter word | locus index, adjacent: one memset clears them all (a window-sized call is bound
  // by its API calls, not by its kernels)
  // (two planes of n values each for F and the objective: the paired Loglikelihood search evaluates two points per pass)
  b.d_counts = c.take<unsigned long long>(n * 6 * sizeof(unsigned long long));
  b.d_f = c.take<double>(2 * n * sizeof(double));
  b.d_running = c.take<unsigned int>(sizeof(unsigned int));
  b.d_index_slot = c.take<uint32_t>((n_sel + 8) * sizeof(uint32_t));
  b.cleared_end = c.take<char>(0);
  b.d_eval = c.take<double>(2 * n * sizeof(double));
  b.d_out = c.take<LocusResultsDev>(n * sizeof(LocusResultsDev));
  b.d_golden = c.take<GoldenState>(n * sizeof(GoldenState));
  b.d_brent = c.take<BrentState>(n * sizeof(BrentState));
  b.d_start = c.take<double>(n * sizeof(double));
  b.d_keep = c.take<double>(n * sizeof(double));
  const uint64_t n_seq_blocks = (n_sel + kSeqBlock - 1) / kSeqBlock;          // (the sequential sums of the defaults: k_seq_*)
  b.d_seq_sum = c.take<double>(n_seq_blocks * 4 * sizeof(double));
  b.d_seq_e = c.take<int>(n_seq_blocks * 4 * sizeof(int));
  b.d_seq_n = c.take<long long>(n_seq_blocks * 4 * sizeof(long long));
  b.d_seq_out = c.take<double>(kParts0 * sizeof(double));
  // The table passes' entries (k_eval_entries): 64 / 256 / 1024 bytes per selected locus, only where such a pass will run.
  b.d_entries = c.take<EvalEntry>(p.table_passes ? (n_sel << (2u * eval_bits(s.amax))) * sizeof(EvalEntry) : 0);
  b.d_segcnt = c.take<unsigned long long>(p.table_sweep ? p.max_seg * n * sizeof(unsigned long long) : sizeof(unsigned long long));
  return b;
}

// per class: bin_begin | bin_end | item_base | bin_block (kHallBins + 1 words each); then, for all: bin_used | used; then the counters:
// per class n_items, n_blocks, n_blocks of the bins a band can reach, 0; for all n_used, unsupported, handed over, 0
constexpr size_t kHallClassWords = 4 * (kHallBins + 1);                   // (and bin_block: the first block of each bin)

// What a call on moments has on top (empty regions otherwise: they come behind the others, so no offset of those moves).
struct MomentsBuffers {
  uint32_t classes = 0;                     // the plan's, or 0 off the moments
  uint64_t items_per_class = 0;
  size_t padded_records = 0;                // per class: its loci in blocks (+ a block of slack)
  size_t keys_bytes = 0, records_bytes = 0, sort_bytes = 0, sort_stride = 0;   // of one of the two sort lanes
  char* keys = nullptr;                     // per lane: keys, slots, sorted keys, sorted slots
  char* records = nullptr;                  // per lane: a class's loci in bin order, as sorted
  HallRecord* padded = nullptr;
  uint32_t* words = nullptr;
  size_t word_count = 0;
  HallItem* items = nullptr;
  uint32_t* item_blocks = nullptr;
  double* ys = nullptr;                     // per class: every slot's frequency (Loglikelihood alone)
  int8_t* digits = nullptr;                 // the matrix-core class pass (k_hall_mfma): per slot 32 digit bytes and its row
  uint32_t* rows = nullptr;
  uint32_t* slot_of_locus = nullptr;        // where each selected locus sits in each class's blocks (k_class_bits), or null
  char* sort = nullptr;                     // the radix sort's own scratch, per lane
  double* moments = nullptr;
  double* bins = nullptr;
  uint32_t* d_needs_passes = nullptr;
  unsigned long long *d_smallest_het = nullptr, *d_search_stats = nullptr;

  uint32_t* class_words(uint32_t k) const { return words + k * kHallClassWords; }
  uint32_t* bin_used() const { return words + classes * kHallClassWords; }
  uint32_t* used() const { return bin_used() + (kHallBins + 1); }
  uint32_t* counters() const { return used() + (kHallBins + 1); }           // [class][4]: n_items, n_blocks; then n_used, unsupported, handed over
  uint32_t* totals() const { return counters() + classes * 4; }
  HallRecord* padded_of(uint32_t k) const { return padded + static_cast<uint64_t>(k) * padded_records; }
  double* ys_of(uint32_t k) const { return ys ? ys + static_cast<uint64_t>(k) * padded_records : nullptr; }
  HallItem* items_of(uint32_t k) const { return items + static_cast<uint64_t>(k) * items_per_class; }
  uint32_t* item_blocks_of(uint32_t k) const { return item_blocks + static_cast<uint64_t>(k) * (items_per_class + 1); }
  int8_t* digits_of(uint32_t k) const { return digits + static_cast<uint64_t>(k) * padded_records * 32; }
  uint32_t* rows_of(uint32_t k) const { return rows + static_cast<uint64_t>(k) * padded_records; }
};

inline MomentsBuffers carve_moments(Carver& c, const InbreedShape& s, const InbreedPlan& p, size_t sort_bytes) {
  const uint64_t n = s.n, n_sel = s.n_sel;
  const bool planned = p.by_moments(), loglik = p.loglik_candidate;
  MomentsBuffers m;
  m.classes = planned ? p.hall_classes : 0;
  m.items_per_class = p.hall_items;
  m.padded_records = static_cast<size_t>(p.hall_blocks + 1) * kHallBlockLoci;
  // (two of each: the classes are put in order two at a time, on the call's stream and on the side stream)
  m.keys_bytes = (4 * n_sel * sizeof(uint32_t) + 255) / 256 * 256;
  m.records_bytes = (n_sel * sizeof(HallRecord) + 255) / 256 * 256;
  m.keys = c.take<char>(planned ? 2 * m.keys_bytes : 0);
  m.records = c.take<char>(planned ? 2 * m.records_bytes : 0);
  m.padded = c.take<HallRecord>(m.classes * m.padded_records * sizeof(HallRecord));
  m.word_count = m.classes * kHallClassWords + 2 * (kHallBins + 1) + (m.classes + 1) * 4;
  m.words = c.take<uint32_t>(planned ? m.word_count * sizeof(uint32_t) : 0);
  m.items = c.take<HallItem>(m.classes * m.items_per_class * sizeof(HallItem));
  m.item_blocks = c.take<uint32_t>(m.classes * (m.items_per_class + 1) * sizeof(uint32_t));
  m.ys = c.take<double>(loglik ? m.classes * m.padded_records * sizeof(double) : 0);
  if (!loglik) m.ys = nullptr;
  m.digits = c.take<int8_t>(p.hall_mfma ? m.classes * m.padded_records * 32 : 0);
  m.rows = c.take<uint32_t>(p.hall_mfma ? m.classes * m.padded_records * sizeof(uint32_t) : 0);
  m.slot_of_locus = c.take<uint32_t>(p.hall_bits_planned ? m.classes * p.sel_pitch * sizeof(uint32_t) : 0);
  if (!p.hall_bits_planned) m.slot_of_locus = nullptr;
  m.sort_bytes = sort_bytes;
  m.sort_stride = (sort_bytes + 255) / 256 * 256;
  m.sort = c.take<char>(2 * m.sort_stride);
  m.moments = c.take<double>(m.items_per_class * kHallMoments * n * sizeof(double));
  m.bins = c.take<double>(planned ? static_cast<size_t>(kHallBins) * kHallMoments * n * sizeof(double) : 0);
  m.d_needs_passes = c.take<uint32_t>(loglik ? n * sizeof(uint32_t) : 0);
  m.d_smallest_het = c.take<unsigned long long>(sizeof(unsigned long long));
  m.d_search_stats = c.take<unsigned long long>(8 * sizeof(unsigned long long));
  return m;
}

}  // namespace kgx

#endif  // KGX_INBREED_BUFFERS_H
