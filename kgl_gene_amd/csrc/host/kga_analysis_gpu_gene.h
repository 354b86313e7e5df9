// The gene-variant analysis of the PfEMP package (kga_analytic/kga_PfEMP/kga_analysis_PfEMP_variant.{h,cpp}) on the device:
// GenomeGeneVariantAnalysis::writeGeneResults writes one CSV line per gene from a walk of every genome and every gene through
// std::map<std::string, ...> lookups (GeneGenomeAnalysis, GenotypeAnalysis); here the same line comes from
// kgx_gene_genotypes (per-(gene, genome) genotype hashes + the per-gene census) and kgx_genotype_statistics.
//
// Out of scope: deciding WHICH rows belong to a gene.  That needs the GFF gene model and ContigModifyFilter's 500-base indel
// margin (getGeneVariants); the row lists are the caller's.  GpuAlleleAnalysis does not write these files by itself.
#ifndef KGA_ANALYSIS_GPU_GENE_H
#define KGA_ANALYSIS_GPU_GENE_H

#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/kgx.h"
#include "kgx_flatten.h"

namespace kellerberrin::genome::analysis::gpu {

// One gene as the analysis needs it: what the reference takes from the GeneFeature (id, coding length of the first
// transcript, featureText) and the population rows of the variants within it.
struct GeneRowList {
  std::string id;                  // gene_ptr->id()
  uint64_t coding_length{0};       // getTranscriptionSequences(gene)->getFirst()->codingNucleotides(), 0 without a transcript
  std::string detail;              // gene_ptr->featureText(CSV_DELIMITER_)
  std::vector<uint32_t> rows;      // device rows of the gene's variants, any order, no row twice
};

class GpuGeneGenotypes {
 public:
  // rows: the FlatPopulation's rows (HGVS per row), in device row order.
  GpuGeneGenotypes(const std::vector<VariantRow>& rows, std::vector<GeneRowList> genes);

  // Utility::hash(HGVS): the reference's crcStringHash is the standard reflected CRC-32 (kel_utility/kel_string_hash.h).
  [[nodiscard]] static uint64_t rowKey(const std::string& hgvs);

  // Runs kgx_gene_genotypes over `population` (whose rows are the rows given above, under whatever genome mask it has).
  // false + error() on failure.
  [[nodiscard]] bool analyze(kgx_pop* population);
  // The reference's file: header and column order of writeGeneResults (_variant.cpp:109-233), std::ofstream default formatting.
  [[nodiscard]] bool writeGeneResults(const std::string& file_name) const;

  [[nodiscard]] const std::vector<GeneRowList>& genes() const { return genes_; }
  [[nodiscard]] const std::vector<kgx_gene_census>& census() const { return census_; }
  [[nodiscard]] const std::vector<uint64_t>& runBegin() const { return run_begin_; }
  [[nodiscard]] const std::vector<uint32_t>& runCount() const { return run_count_; }
  [[nodiscard]] const std::string& error() const { return error_; }

  constexpr static const char CSV_DELIMITER_ = ',';

 private:
  std::vector<uint64_t> row_key_;
  std::vector<GeneRowList> genes_;
  std::vector<kgx_gene_census> census_;
  std::vector<uint64_t> run_begin_, run_hash_;
  std::vector<uint32_t> run_count_;
  std::string error_;
  bool analyzed_{false};
};

}  // namespace kellerberrin::genome::analysis::gpu

#endif  // KGA_ANALYSIS_GPU_GENE_H
