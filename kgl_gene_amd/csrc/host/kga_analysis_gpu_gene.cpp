#include "kga_analysis_gpu_gene.h"

#include <zlib.h>

#include <fstream>

namespace kellerberrin::genome::analysis::gpu {

GpuGeneGenotypes::GpuGeneGenotypes(const std::vector<VariantRow>& rows, std::vector<GeneRowList> genes) : genes_(std::move(genes)) {
  row_key_.reserve(rows.size());
  for (const auto& row : rows) row_key_.push_back(rowKey(row.hgvs));
}

uint64_t GpuGeneGenotypes::rowKey(const std::string& hgvs) {
  return static_cast<uint64_t>(::crc32(::crc32(0L, Z_NULL, 0), reinterpret_cast<const Bytef*>(hgvs.data()), static_cast<uInt>(hgvs.size())));
}

bool GpuGeneGenotypes::analyze(kgx_pop* population) {
  analyzed_ = false;
  error_.clear();
  if (!population || kgx_population_variants(population) != row_key_.size()) {
    error_ = "GpuGeneGenotypes::analyze; the population's rows are not the rows the keys were made from";
    return false;
  }
  std::vector<uint32_t> members, first(genes_.size()), count(genes_.size());
  for (size_t i = 0; i < genes_.size(); ++i) {
    first[i] = static_cast<uint32_t>(members.size());
    count[i] = static_cast<uint32_t>(genes_[i].rows.size());
    members.insert(members.end(), genes_[i].rows.begin(), genes_[i].rows.end());
  }
  census_.assign(genes_.size(), kgx_gene_census{});
  run_begin_.assign(genes_.size() + 1, 0);
  // the sizing call, then the filled one (the convention of kgx_genome_row_lists)
  int rc = kgx_gene_genotypes(population, row_key_.data(), members.data(), members.size(), first.data(), count.data(), genes_.size(), nullptr, nullptr,
                              census_.data(), run_begin_.data(), nullptr, nullptr, 0);
  if (rc == KGX_OK) {
    const uint64_t capacity = run_begin_.back();
    run_hash_.assign(capacity + 1, 0);
    run_count_.assign(capacity + 1, 0);
    rc = kgx_gene_genotypes(population, row_key_.data(), members.data(), members.size(), first.data(), count.data(), genes_.size(), nullptr, nullptr,
                            census_.data(), run_begin_.data(), run_hash_.data(), run_count_.data(), capacity);
    run_hash_.resize(capacity);
    run_count_.resize(capacity);
  }
  if (rc != KGX_OK) {
    error_ = std::string("GpuGeneGenotypes::analyze; kgx_gene_genotypes failed: ") + kgx_last_error();
    return false;
  }
  analyzed_ = true;
  return true;
}

bool GpuGeneGenotypes::writeGeneResults(const std::string& file_name) const {
  if (!analyzed_) return false;
  std::ofstream variant_file(file_name);
  if (not variant_file.good()) return false;
  const char d = CSV_DELIMITER_;
  variant_file << "Gene_ID" << d << "Coding Length" << d << "Variant Count" << d << "Variant Rate" << d << "Unique filter" << d << "Unique Variant Rate" << d
               << "Single Genome filter" << d << "Single Variant Genomes" << d << "No Variant Genomes" << d << "Genotypes" << d << "Gini" << d << "HRel" << d
               << "2-IQV" << d << "Top1 Genotype" << d << "Top2 Genotype" << d << "Top3 Genotype" << d << "Top4 Genotype" << d << "Top5 Genotype" << d
               << "Gene Detail" << '\n';
  for (size_t i = 0; i < genes_.size(); ++i) {
    const GeneRowList& gene = genes_[i];
    const kgx_gene_census& c = census_[i];
    double variant_rate{0.0};
    double unique_variant_rate{0.0};
    if (gene.coding_length > 0) {
      variant_rate = static_cast<double>(c.variant_objects) / static_cast<double>(gene.coding_length);
      unique_variant_rate = static_cast<double>(c.unique_variants) / static_cast<double>(gene.coding_length);
    }
    double stats[3] = {1.0, 0.0, 1.0};
    const uint64_t runs = run_begin_[i + 1] - run_begin_[i];
    if (kgx_genotype_statistics(runs ? run_count_.data() + run_begin_[i] : nullptr, runs, c.zero_variant_genomes, stats) != KGX_OK) return false;
    variant_file << gene.id << d << gene.coding_length << d << c.variant_objects << d << variant_rate << d << c.unique_variants << d << unique_variant_rate << d
                 << c.singleton_variants << d << c.singleton_genomes << d << c.zero_variant_genomes << d << c.genotypes << d << stats[0] << d << stats[1] << d
                 << (2.0 - stats[2]) << d << c.top[0] << d << c.top[1] << d << c.top[2] << d << c.top[3] << d << c.top[4] << d << gene.detail << '\n';
  }
  return variant_file.good();
}

}  // namespace kellerberrin::genome::analysis::gpu
