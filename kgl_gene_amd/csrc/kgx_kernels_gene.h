// Gene genotype tables (kgx_gene_genotypes): the per-(gene, genome) genotype hash of GenotypeAnalysis::genotypeHash
// (kga_analytic/kga_PfEMP/kga_analysis_PfEMP_variant.cpp:453-484) as a sweep over the 2-bit rows, and the per-gene census of
// those hashes (GenotypeAnalysis::analyzeGenePopulation, :401-450; the columns of writeGeneResults, :109-233).
#ifndef KGX_KERNELS_GENE_H
#define KGX_KERNELS_GENE_H

#include "kgx_kernels_common.h"

namespace kgx {

// A gene of the batch: its first position in the row list and its number of rows there.
struct GeneSpan {
  uint32_t first;
  uint32_t n_rows;
};

// What k_gene_compact leaves per gene: the genomes with a genotype and the sums over the gene's cells.
struct GeneSums {
  unsigned long long genotype_genomes;   // genomes carrying >= 1 row of the gene
  unsigned long long variant_objects;    // code 1 -> 1, code 2 -> 2
  unsigned long long non_diploid_cells;  // code 3
  unsigned long long singleton_genomes;  // genomes carrying >= 1 row nobody else carries
};

// ---------------------------------------------------------------------------------------------
// The hashing sweep.  Same access shape as k_compound_offsets: a lane owns one dword column (16 genomes) and walks the rows of
// a slice of WHOLE genes, so every (gene, genome) result is owned by one lane and leaves by plain stores -- no atomics, the
// same bits on every run.  Per row the key is wave-uniform; hash[g] += key where the genome carries the row (code != 0), in
// uint64: the reference's size_t sum, order-free.  A dword nobody of its 16 genomes carries anything in is skipped (real data
// is mostly reference-homozygous).  carried / twice (code 2) / more (code 3) / singleton rows carried are summed in 4-bit
// fields (even and odd genomes apart, as k_compound_offsets does) and drained into 32-bit counters after 15 counted rows.
// keep: the genome mask in the rows' own layout (0b11 = takes part), or null.  Genomes past n_genomes and masked-out genomes
// carry nothing: hash 0, counts 0.
// out_hash / out_counts: [n_genes][out_pitch], this shard's genomes from column out_col0.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_gene_genotypes(const uint32_t* __restrict__ rows, uint64_t dwords_per_row, uint64_t n_genomes, const uint32_t* __restrict__ keep,
                 const GeneSpan* __restrict__ genes, uint64_t n_genes, uint64_t genes_per_slice, const uint32_t* __restrict__ row_list,
                 const unsigned long long* __restrict__ row_key, const uint8_t* __restrict__ row_single,
                 unsigned long long* __restrict__ out_hash, kgx_v4u* __restrict__ out_counts, uint64_t out_pitch, uint64_t out_col0) {
  const uint64_t col = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;   // dword column = 16 genomes
  if (col * 16 >= n_genomes) return;
  const uint64_t left = n_genomes - col * 16;
  uint32_t live = left >= 16 ? 0xFFFFFFFFu : (1u << (2 * static_cast<uint32_t>(left))) - 1u;   // the column tail
  if (keep) live &= keep[col];
  live &= 0x55555555u;
  const uint64_t g_begin = static_cast<uint64_t>(blockIdx.y) * genes_per_slice;
  const uint64_t g_end = g_begin + genes_per_slice < n_genes ? g_begin + genes_per_slice : n_genes;

  for (uint64_t gi = g_begin; gi < g_end; ++gi) {
    const GeneSpan gene = genes[gi];
    unsigned long long h[16];
    uint32_t carried[16], twice[16], more[16], single[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      h[j] = 0;
      carried[j] = twice[j] = more[j] = single[j] = 0;
    }
    uint32_t present_e = 0, present_o = 0, two_e = 0, two_o = 0, three_e = 0, three_o = 0, single_e = 0, single_o = 0;
    uint32_t pending = 0;                                     // rows in the fields: at most 15
    auto drain = [&]() {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        // genome j of the dword sits in bits 2j..2j+1: even j -> nibble j/2 of *_e, odd j -> nibble j/2 of *_o
        const int s = 4 * (j >> 1);
        carried[j] += (((j & 1) ? present_o : present_e) >> s) & 0xFu;
        twice[j] += (((j & 1) ? two_o : two_e) >> s) & 0xFu;
        more[j] += (((j & 1) ? three_o : three_e) >> s) & 0xFu;
        single[j] += (((j & 1) ? single_o : single_e) >> s) & 0xFu;
      }
      present_e = present_o = two_e = two_o = three_e = three_o = single_e = single_o = 0;
      pending = 0;
    };
    for (uint32_t r = 0; r < gene.n_rows; ++r) {
      const uint64_t row = row_list[gene.first + r];          // gene-uniform, hence wave-uniform: scalar loads
      const unsigned long long key = row_key[row];
      const uint32_t is_single = row_single[row];
      const uint32_t w = rows[row * dwords_per_row + col];
      const uint32_t lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;
      const uint32_t present = (lo | hi) & live;
      if (present == 0) continue;
      const uint32_t two = hi & ~lo & live, three = hi & lo & live;
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if ((present >> (2 * j)) & 1u) h[j] += key;
      present_e += present & 0x11111111u;
      present_o += (present >> 2) & 0x11111111u;
      two_e += two & 0x11111111u;
      two_o += (two >> 2) & 0x11111111u;
      three_e += three & 0x11111111u;
      three_o += (three >> 2) & 0x11111111u;
      if (is_single) {
        single_e += present & 0x11111111u;
        single_o += (present >> 2) & 0x11111111u;
      }
      if (++pending == 15) drain();
    }
    if (pending) drain();
    const uint64_t base = gi * out_pitch + out_col0 + col * 16;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (static_cast<uint64_t>(j) < left) {
        out_hash[base + j] = h[j];
        kgx_v4u c;
        c.x = carried[j];
        c.y = twice[j];
        c.z = more[j];
        c.w = single[j];
        out_counts[base + j] = c;
      }
  }
}

// ---------------------------------------------------------------------------------------------
// Census, one workgroup per gene of the batch.
// ---------------------------------------------------------------------------------------------

// Exclusive scan of one flag per thread over the workgroup (kBlock threads, 4 waves): the number of set flags in the threads
// before this one; *total = the workgroup's count.  wave_sums: kBlock / kWave words of LDS.  Every thread must call it.
__device__ inline uint32_t block_flag_scan(bool flag, uint32_t* wave_sums, uint32_t* total) {
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const unsigned long long ballot = __ballot(flag);
  const uint32_t before = static_cast<uint32_t>(__popcll(ballot & ((1ull << lane) - 1ull)));
  __syncthreads();                                            // the previous round's readers are done with wave_sums
  if (lane == 0) wave_sums[wave] = static_cast<uint32_t>(__popcll(ballot));
  __syncthreads();
  uint32_t offset = 0, sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < kBlock / kWave; ++k) {
    const uint32_t s = wave_sums[k];
    if (k < wave) offset += s;
    sum += s;
  }
  *total = sum;
  return offset + before;
}

__device__ inline unsigned long long block_sum(unsigned long long v, unsigned long long* lds /* kBlock */) {
  __syncthreads();
  lds[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t s = kBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  return lds[0];
}

// The hashes of the genomes that HAVE a genotype (carried > 0 -- never hash != 0: a genotype may hash to 0), in genome order at
// the front of the gene's segment of `keys`; seg_begin / seg_end: the segment for the sort; sums: GeneSums.
__global__ void __launch_bounds__(kBlock)
k_gene_compact(const unsigned long long* __restrict__ hash, const kgx_v4u* __restrict__ counts, uint64_t n_genomes,
               unsigned long long* __restrict__ keys, uint32_t* __restrict__ seg_begin, uint32_t* __restrict__ seg_end, GeneSums* __restrict__ sums) {
  __shared__ uint32_t wave_sums[kBlock / kWave];
  __shared__ unsigned long long reduce[kBlock];
  const uint64_t gene = blockIdx.x, base = gene * n_genomes;
  unsigned long long objects = 0, non_diploid = 0, with_single = 0;
  uint32_t written = 0;
  for (uint64_t g0 = 0; g0 < n_genomes; g0 += kBlock) {
    const uint64_t g = g0 + threadIdx.x;
    bool has = false;
    unsigned long long hsh = 0;
    if (g < n_genomes) {
      const kgx_v4u c = counts[base + g];
      has = c.x > 0;
      if (has) {
        hsh = hash[base + g];
        objects += static_cast<unsigned long long>(c.x - c.y - c.z) + 2ull * c.y;
        non_diploid += c.z;
        with_single += c.w > 0 ? 1u : 0u;
      }
    }
    uint32_t total = 0;
    const uint32_t at = block_flag_scan(has, wave_sums, &total);
    if (has) keys[base + written + at] = hsh;
    written += total;
  }
  const unsigned long long o = block_sum(objects, reduce), n = block_sum(non_diploid, reduce), s = block_sum(with_single, reduce);
  if (threadIdx.x == 0) {
    seg_begin[gene] = static_cast<uint32_t>(base);
    seg_end[gene] = static_cast<uint32_t>(base) + written;
    GeneSums out;
    out.genotype_genomes = written;
    out.variant_objects = o;
    out.non_diploid_cells = n;
    out.singleton_genomes = s;
    sums[gene] = out;
  }
}

// Run-length encoding of a gene's sorted hashes, in the two passes of k_genome_row_lists<FILL>: count, (offsets on the host), fill.
//   FILL = false: n_runs[gene] = distinct hashes.
//   FILL = true : run_hash / run_count [run_begin[gene] ..) = the distinct hashes ascending and how many genomes hold each;
//                 top[gene][5] = the five largest counts, descending, 0-padded (GenotypeAnalysis::getTopCounts<5>).
template <bool FILL>
__global__ void __launch_bounds__(kBlock)
k_gene_runs(const unsigned long long* __restrict__ sorted, uint64_t n_genomes, const uint32_t* __restrict__ seg_begin, const uint32_t* __restrict__ seg_end,
            uint32_t* __restrict__ n_runs, const unsigned long long* __restrict__ run_begin, unsigned long long* __restrict__ run_hash,
            uint32_t* __restrict__ run_count, unsigned long long* __restrict__ top) {
  __shared__ uint32_t wave_sums[kBlock / kWave];
  __shared__ unsigned long long reduce[kBlock];
  const uint64_t gene = blockIdx.x;
  const uint64_t base = seg_begin[gene];
  const uint32_t n = seg_end[gene] - seg_begin[gene];
  uint32_t runs = 0;
  const unsigned long long out0 = FILL ? run_begin[gene] : 0;
  for (uint32_t i0 = 0; i0 < n; i0 += kBlock) {
    const uint32_t i = i0 + threadIdx.x;
    bool head = false;
    unsigned long long key = 0;
    if (i < n) {
      key = sorted[base + i];
      head = i == 0 || sorted[base + i - 1] != key;
    }
    uint32_t total = 0;
    const uint32_t at = block_flag_scan(head, wave_sums, &total);
    if (FILL && head) {
      run_hash[out0 + runs + at] = key;
      run_count[out0 + runs + at] = i;                        // the run's first position; its length follows below
    }
    runs += total;
  }
  if (!FILL) {
    if (threadIdx.x == 0) n_runs[gene] = runs;
    return;
  }
  // length of run r = first position of run r + 1 (or n) - its own; a chunk's reads are done before its writes, and the
  // one value a chunk reads beyond itself belongs to the next chunk, which has not written yet
  uint32_t best[5] = {0, 0, 0, 0, 0};
  for (uint32_t r0 = 0; r0 < runs; r0 += kBlock) {
    const uint32_t r = r0 + threadIdx.x;
    uint32_t length = 0;
    __syncthreads();                                          // the positions written above / the previous chunk's lengths
    if (r < runs) length = (r + 1 < runs ? run_count[out0 + r + 1] : n) - run_count[out0 + r];
    __syncthreads();
    if (r < runs) {
      run_count[out0 + r] = length;
      uint32_t v = length;
#pragma unroll
      for (int k = 0; k < 5; ++k)
        if (v > best[k]) {
          const uint32_t t = best[k];
          best[k] = v;
          v = t;
        }
    }
  }
  // five rounds of "largest head among the threads' lists"; the winning thread (the lowest on a tie) pops its head
  for (int k = 0; k < 5; ++k) {
    __syncthreads();
    reduce[threadIdx.x] = (static_cast<unsigned long long>(best[0]) << 32) | (kBlock - 1 - threadIdx.x);
    __syncthreads();
    for (uint32_t s = kBlock / 2; s > 0; s >>= 1) {
      if (threadIdx.x < s && reduce[threadIdx.x + s] > reduce[threadIdx.x]) reduce[threadIdx.x] = reduce[threadIdx.x + s];
      __syncthreads();
    }
    const unsigned long long winner = reduce[0];
    if (threadIdx.x == 0) top[gene * 5 + k] = winner >> 32;
    if (kBlock - 1 - static_cast<uint32_t>(winner & 0xFFFFFFFFull) == threadIdx.x) {
      best[0] = best[1];
      best[1] = best[2];
      best[2] = best[3];
      best[3] = best[4];
      best[4] = 0;
    }
  }
}

}  // namespace kgx

#endif  // KGX_KERNELS_GENE_H
