// Genotype summaries of one (variant, sample) cell and of one variant, as the host layer computes them (bayestyper_amd/host/Genotypes.cpp: getGenotypes,
// a restatement of VariantClusterGenotyper::getGenotypes, VariantClusterGenotyper.cpp:208-567), written once for the host and the device:
// geno_cell_kernel / geno_variant_kernel (bt_gibbs.hip) and bt_diag_genotype_cluster run this code.  Same floatCompare / floatLess, same float
// arithmetic (sums accumulated in float, divided by the number of collected sweeps afterwards), same running-maximum rule for the set of best genotypes.
// GQ is NOT computed here: (uint32_t)(-10 * log10f(1 - best)) truncates, and posteriors such as 0.9 sit on its integer boundaries, so one ulp between
// two log10f implementations flips the digit.  The record carries `best`; the host derives GQ with its own log10.
//
// The record layout of bt_gibbs_genotypes' word string (include/btgpu.h) is defined here as well, so that the kernels, the diagnostic entry and the
// readers agree on it by construction.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BTG_HD __host__ __device__
#else
#define BTG_HD
#endif

namespace btgeno {

constexpr uint16_t NONE = 0xFFFF;
constexpr float kFloatEps = 1.1920928955078125e-7f;   // std::numeric_limits<float>::epsilon()
// two DIFFERENT integer sums (exact in float up to 2^24) can only compare equal under float_compare once the smaller exceeds this: below it the set of
// best genotypes does not depend on the order the diplotype entries are visited in (bt_gibbs.hip: geno_cell_kernel)
constexpr uint32_t kOrderFreeBelow = 83887;

// Utils::floatCompare / floatLess (include/bayesTyper/Utils.hpp:89-103)
BTG_HD inline bool float_compare(float a, float b) { return a == b || __builtin_fabsf(a - b) < __builtin_fabsf(b < a ? b : a) * kFloatEps * 100; }
BTG_HD inline bool float_less(float a, float b) { return a < b && !float_compare(a, b); }

// ---- record layout (32-bit words; every record starts on an even word and has an even length, so doubles are 8-byte aligned) -------------------
//   variant record:  [0] A  [1] total_count  [2] max_alt_allele_call_probability (f32)  [3] has_dependency
//                    per allele a < A, 4 words: allele call probability (f32), alt allele count, alt allele frequency (f32) (both of allele a, 0 for a = 0:
//                    the host's alt_allele_counts[a - 1]), 1 if the allele is not covered by a haplotype candidate
//                    then the S sample records
//   sample record:   [0] ploidy  [1] estimate: first | second << 16 (0xFFFF = no call / unused)  [2] best genotype posterior (f32)  [3] 0
//                    genotype posteriors f32 [G]: G = A (A + 1) / 2 for ploidy 2 (index second (second + 1) / 2 + first), A for ploidy 1, 0 for ploidy 0
//                    allele posteriors f32 [A'], allele filter bits [A'] (1 = NAK, 2 = FAK): A' = A, or 0 for ploidy 0
//                    one pad word if the count so far is odd
//                    k-mer means f64 [A][3]: KmerStats::getMean of the count / fraction / mean statistics (-1 when nothing was added)
constexpr uint32_t kVariantHead = 4, kAlleleWords = 4, kSampleHead = 4;
BTG_HD inline uint64_t num_genotypes(uint32_t A, uint32_t ploidy) { return ploidy == 2 ? (uint64_t)A * (A - 1) / 2 + A : (ploidy == 1 ? A : 0u); }
BTG_HD inline uint64_t variant_head_words(uint32_t A) { return kVariantHead + (uint64_t)kAlleleWords * A; }
BTG_HD inline uint64_t sample_means_at(uint32_t A, uint32_t ploidy) {   // word offset of the k-mer means inside a sample record
    const uint64_t n = kSampleHead + num_genotypes(A, ploidy) + (ploidy ? 2ull * A : 0ull);
    return n + (n & 1u);
}
BTG_HD inline uint64_t sample_words(uint32_t A, uint32_t ploidy) { return sample_means_at(A, ploidy) + 6ull * A; }

// ---- one (variant, sample) cell: getGenotypeSampleStats (VariantClusterGenotyper.cpp:249-466; Genotypes.cpp:37-105) -----------------------------
struct Cell {
    uint32_t ploidy, A;
    float *gpp, *app;   // [num_genotypes], [A or 0]: zeroed by cell_begin, sums until cell_finish
    uint32_t num_iterations, best_n;
    uint16_t best_first, best_second;
    float best_value;
};
BTG_HD inline void cell_begin(Cell &c, uint32_t A, uint32_t ploidy, float *gpp, float *app) {
    c.ploidy = ploidy;
    c.A = A;
    c.gpp = gpp;
    c.app = app;
    c.num_iterations = c.best_n = 0;
    c.best_first = c.best_second = NONE;
    c.best_value = 0;
    const uint64_t G = num_genotypes(A, ploidy);
    for (uint64_t i = 0; i < G; ++i) gpp[i] = 0.f;
    for (uint32_t a = 0; a < (ploidy ? A : 0u); ++a) app[a] = 0.f;
}
// one diplotype entry (h1, h2) sampled f times; allele_of(h): haplotypeToAlleleIndex (the missing allele A - 1 for h = NONE)
template <class AlleleOf>
BTG_HD inline void cell_add(Cell &c, uint16_t h1, uint16_t h2, uint32_t f, AlleleOf allele_of) {
    if (!f) return;
    uint16_t g1 = NONE, g2 = NONE;
    uint64_t gi = 0;
    if (c.ploidy == 2) {
        g1 = allele_of(h1);
        g2 = allele_of(h2);
        if (g1 > g2) {
            const uint16_t t = g1;
            g1 = g2;
            g2 = t;
        }
        gi = (uint64_t)g2 * (g2 + 1u) / 2 + g1;
        c.gpp[gi] += f;
        c.app[g1] += f;
        if (g1 != g2) c.app[g2] += f;
    } else if (c.ploidy == 1) {
        g1 = allele_of(h1);
        gi = g1;
        c.gpp[gi] += f;
        c.app[g1] += f;
    }
    c.num_iterations += f;
    if (c.ploidy) {   // running maximum over the accumulating genotype sums (:334-346): a genotype may enter the set more than once
        if (float_compare(c.best_value, c.gpp[gi])) {
            if (!c.best_n) {
                c.best_first = g1;
                c.best_second = g2;
            }
            c.best_n++;
        } else if (c.best_value < c.gpp[gi]) {
            c.best_n = 1;
            c.best_first = g1;
            c.best_second = g2;
            c.best_value = c.gpp[gi];
        }
    }
}
// stat(a, i): element i of the twelve k-mer statistics of allele a for this sample ([stat * 4 + {count, fraction, mean, M2}]); filters: [A or 0];
// estimate[2] and *best receive the call (NONE = no call / unused) and the best posterior
template <class Stat>
BTG_HD inline void cell_finish(Cell &c, uint32_t *filters, float min_genotype_posterior, float min_number_of_kmers, float min_fraction_observed_kmers, Stat stat,
                               uint16_t *estimate, float *best) {
    c.best_value /= c.num_iterations;
    const uint64_t G = num_genotypes(c.A, c.ploidy);
    const uint32_t Ap = c.ploidy ? c.A : 0u;
    for (uint64_t i = 0; i < G; ++i) c.gpp[i] /= c.num_iterations;
    for (uint32_t a = 0; a < Ap; ++a) c.app[a] /= c.num_iterations;
    for (uint32_t a = 0; a < Ap; ++a) {
        filters[a] = 0;
        if (float_compare(c.app[a], 0)) continue;
        const float count_mean = (float)stat(a, 2u);
        if (float_less(count_mean, min_number_of_kmers)) filters[a] += 1;
        if (!float_compare(count_mean, 0)) {
            const float fraction_mean = (float)stat(a, 6u);
            if (float_less(fraction_mean, min_fraction_observed_kmers)) filters[a] += 2;
        }
    }
    estimate[0] = estimate[1] = NONE;
    if (c.ploidy == 2) {
        if (c.best_n == 1 && !float_less(c.best_value, min_genotype_posterior) && filters[c.best_first] == 0 && filters[c.best_second] == 0) {
            estimate[0] = c.best_first;
            estimate[1] = c.best_second;
        }
    } else if (c.ploidy == 1) {
        if (c.best_n == 1 && !float_less(c.best_value, min_genotype_posterior) && filters[c.best_first] == 0) estimate[0] = c.best_first;
    }
    *best = c.best_value;
}
// KmerStats::getMean (KmerStats.cpp:82-92) of the three statistics of allele a -> means[3]
template <class Stat>
BTG_HD inline void cell_kmer_means(uint32_t a, Stat stat, double *means) {
    for (uint32_t k = 0; k < 3; ++k) means[k] = stat(a, 4u * k) == 0 ? -1.0 : stat(a, 4u * k + 2u);
}

BTG_HD inline float word_as_float(uint32_t w) {
    float f;
    __builtin_memcpy(&f, &w, 4);
    return f;
}
BTG_HD inline uint32_t float_as_word(float f) {
    uint32_t w;
    __builtin_memcpy(&w, &f, 4);
    return w;
}

// the whole sample record of one cell; entries(add): calls add(h1, h2, f) for every diplotype entry of the cluster with its count for this sample, in
// the order bt_gibbs_result_fetch hands them out
template <class Entries, class AlleleOf, class Stat>
BTG_HD inline void sample_record(uint32_t *rec, uint32_t A, uint32_t ploidy, Entries entries, AlleleOf allele_of, Stat stat, float min_genotype_posterior,
                                 float min_number_of_kmers, float min_fraction_observed_kmers) {
    const uint64_t G = num_genotypes(A, ploidy);
    const uint32_t Ap = ploidy ? A : 0u;
    float *gpp = reinterpret_cast<float *>(rec + kSampleHead), *app = gpp + G;
    uint32_t *filters = rec + kSampleHead + G + Ap;
    Cell c;
    cell_begin(c, A, ploidy, gpp, app);
    entries([&](uint16_t h1, uint16_t h2, uint32_t f) { cell_add(c, h1, h2, f, allele_of); });
    uint16_t est[2];
    float best;
    cell_finish(c, filters, min_genotype_posterior, min_number_of_kmers, min_fraction_observed_kmers, stat, est, &best);
    rec[0] = ploidy;
    rec[1] = (uint32_t)est[0] | ((uint32_t)est[1] << 16);
    rec[2] = float_as_word(best);
    rec[3] = 0;
    const uint64_t at = sample_means_at(A, ploidy);
    if ((kSampleHead + G + 2ull * Ap) & 1u) rec[at - 1] = 0;
    double *means = reinterpret_cast<double *>(rec + at);
    for (uint32_t a = 0; a < A; ++a) cell_kmer_means(a, stat, means + 3u * a);
}

// ---- one variant: getNonCoveredAlleles (:221-247) and getGenotypeVariantStats (:468-527; Genotypes.cpp:29-34, 106-125) from its finished sample records --------
// rec: the variant record (its sample records filled); hap_allele_of(h): the variant's allele on haplotype candidate h < H
template <class HapAllele>
BTG_HD inline void variant_record(uint32_t *rec, uint32_t A, bool has_dependency, uint32_t S, uint32_t H, HapAllele hap_allele_of) {
    uint32_t *al = rec + kVariantHead;
    for (uint32_t a = 0; a < A; ++a) {
        al[4u * a] = float_as_word(0.f);
        al[4u * a + 1] = 0;
        al[4u * a + 2] = float_as_word(0.f);
        al[4u * a + 3] = 1;
    }
    for (uint32_t h = 0; h < H; ++h) al[4u * hap_allele_of(h) + 3] = 0;
    if (has_dependency) al[4u * (A - 1) + 3] = 0;
    uint32_t total_count = 0;
    const uint32_t *sr = rec + variant_head_words(A);
    for (uint32_t s = 0; s < S; ++s) {
        const uint32_t ploidy = sr[0];
        const uint16_t est[2] = {(uint16_t)(sr[1] & 0xFFFFu), (uint16_t)(sr[1] >> 16)};
        for (uint32_t i = 0; i < ploidy && i < 2; ++i)
            if (est[i] != NONE) {
                total_count++;
                if (est[i] > 0) al[4u * est[i] + 1]++;
            }
        const uint64_t G = num_genotypes(A, ploidy);
        const uint32_t Ap = ploidy ? A : 0u;
        const uint32_t *app = sr + kSampleHead + G, *filters = app + Ap;
        for (uint32_t a = 0; a < Ap; ++a)
            if (filters[a] == 0) {
                const float cur = word_as_float(al[4u * a]), p = word_as_float(app[a]);
                al[4u * a] = float_as_word(cur < p ? p : cur);   // std::max
            }
        sr += sample_words(A, ploidy);
    }
    float max_alt = 0;
    const uint32_t num_alt = A - 1 - (has_dependency ? 1u : 0u);   // the missing allele is not an alt allele
    for (uint32_t a = 0; a < num_alt; ++a) {
        const float p = word_as_float(al[4u * (a + 1)]);
        max_alt = max_alt < p ? p : max_alt;
    }
    if (total_count > 0)
        for (uint32_t a = 1; a < A; ++a) al[4u * a + 2] = float_as_word(al[4u * a + 1] / (float)total_count);
    rec[0] = A;
    rec[1] = total_count;
    rec[2] = float_as_word(max_alt);
    rec[3] = has_dependency ? 1u : 0u;
}

}  // namespace btgeno
