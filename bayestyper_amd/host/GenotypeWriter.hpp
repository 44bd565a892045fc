// Output VCF of the genotyping stage: GenotypeWriter (include/bayesTyper/GenotypeWriter.hpp, src/bayesTyper/GenotypeWriter.cpp:57-556).
// One line per genotyped variant: REF/ALT rebuilt from the cluster's variant records and the reference sequence, QUAL/FILTER and
// the call statistics (Genotypes.hpp), the cluster annotations (VCS, VCR, VCGS, VCGR, HC), ANC, ACO and the per-sample columns;
// lines sorted by contig (genome order) and position; the header names every non-decoy contig.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "Genotypes.hpp"
#include "TabixIndex.hpp"
#include "VariantFileParser.hpp"

namespace bthost {

struct VariantInfo {   // include/bayesTyper/VariantInfo.hpp:66-121
    uint32_t position = 0;   // 1-based
    std::string id;
    bool has_dependency = false;
    std::vector<AlleleInfo> alt_alleles;
    uint16_t numberOfAlleles() const { return (uint16_t)(1 + (has_dependency ? 1 : 0) + alt_alleles.size()); }
    uint32_t maxReferenceLength() const;
};
// variant_cluster_info of a cluster's graph (VariantClusterGraph.cpp:69-93) and the region getGenotypes reports (VariantClusterGenotyper.cpp:535-555)
std::vector<VariantInfo> variantClusterInfo(const VariantCluster &cluster);
std::string variantClusterRegion(const std::string &chrom_name, const std::vector<VariantInfo> &variant_cluster_info);

struct ClusterAnnotation {   // the Genotypes fields that describe where a variant was genotyped (Genotypes.hpp:47-58)
    std::string chrom_name;
    uint32_t variant_cluster_size = 0;
    std::string variant_cluster_region;
    uint32_t variant_cluster_group_size = 0;
    std::string variant_cluster_group_region;
    uint32_t num_candidates = 0;   // haplotype candidates of the cluster (HC)
};

class GenotypeWriter {
  public:
    GenotypeWriter(std::vector<std::string> sample_names, const Chromosomes &chromosomes);
    struct GenotypedVariant {
        uint32_t position, max_ref_length;
        std::string variant_id, genotypes;   // genotypes = everything after the REF column
    };
    // one genotyped variant (GenotypeWriter::writeGenotypes :84-128); sample_columns = formatSampleColumns(...) of that variant
    void addGenotypes(const ClusterAnnotation &where, const VariantInfo &variant_info, const VariantGenotypes &genotypes, const std::string &sample_columns);
    // the same in two steps, so that worker threads can format (const, thread-safe) and one thread appends in the order of a one-thread run
    GenotypedVariant formatGenotypes(const ClusterAnnotation &where, const VariantInfo &variant_info, const VariantGenotypes &genotypes, const std::string &sample_columns) const;
    // the same line from text formatted on the device (bt_gibbs_genotype_text): quality_and_filter = formatQualityAndFilter(...), stats = "AC=..;AF=..;AN=..;ACP=..",
    // cover = ";ANC=.." or empty, sample_columns = the samples piece with the GQs spliced in; the host adds ALT, the cluster annotations, ACO and FORMAT
    GenotypedVariant formatGenotypesFromText(const ClusterAnnotation &where, const VariantInfo &variant_info, const std::string &quality_and_filter, const char *stats, size_t stats_len,
                                             const char *cover, size_t cover_len, const std::string &sample_columns) const;
    void append(const std::string &chrom_name, GenotypedVariant &&variant) { genotyped_variants[chrom_name].push_back(std::move(variant)); }
    std::string generateHeader(const std::string &genome_filename, const std::string &graph_options_header, const std::string &genotype_options_header) const;   // :494-551
    // header + sorted lines (finalise :352-492); the file variant writes <output_prefix>.vcf or .vcf.gz and returns the number of variants
    // line_table (optional): what a tabix index is built from (TabixIndex.hpp) — the names of the contigs that have lines, in the text's order, and per data
    // line its contig, POS, len(REF), first byte in the text and length.  The text is the same with or without it.
    struct LineTable {
        std::vector<std::string> contigs;
        std::vector<TabixLine> lines;
    };
    std::string vcfText(const std::string &genome_filename, const std::string &graph_options_header, const std::string &genotype_options_header, LineTable *line_table = nullptr);
    uint32_t finalise(const std::string &output_prefix, bool gzip_output, const std::string &genome_filename, const std::string &graph_options_header,
                      const std::string &genotype_options_header);
    // the same with the .vcf.gz written by gz_writer(filename, text) instead of the single gzwrite stream (one thread, texts below 2 GiB): the device route
    // (writeGzFileOnDevice, 64-bit sizes).  An empty gz_writer, or gzip_output false, is the call above.
    using GzWriter = std::function<void(const std::string &filename, const std::string &text)>;
    uint32_t finalise(const std::string &output_prefix, bool gzip_output, const std::string &genome_filename, const std::string &graph_options_header,
                      const std::string &genotype_options_header, const GzWriter &gz_writer);
    // the same with the .vcf.gz and its index written by indexed_writer(filename, text, line_table): the BGZF route (writeBgzfVcfOnDevice)
    using IndexedGzWriter = std::function<void(const std::string &filename, const std::string &text, const LineTable &line_table)>;
    uint32_t finalise(const std::string &output_prefix, const std::string &genome_filename, const std::string &graph_options_header, const std::string &genotype_options_header,
                      const IndexedGzWriter &indexed_writer);

  private:
    GenotypedVariant formatLine(const ClusterAnnotation &where, const VariantInfo &variant_info, const char *quality_filter_stats, size_t qfs_len, const char *cover, size_t cover_len,
                                const std::string &sample_columns) const;
    std::vector<std::string> samples;
    const Chromosomes &chromosomes;
    std::unordered_map<std::string, std::vector<GenotypedVariant>> genotyped_variants;
};

}  // namespace bthost
