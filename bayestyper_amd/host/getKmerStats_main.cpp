// `getKmerStats` — the bayesTyperTools k-mer statistics script (src/bayesTyperTools/scripts/getKmerStats.cpp): every record of a sample's
// KMC table -> <output_prefix>_kmer_stats.txt, a histogram over (k-mer count, #A, #C, #G, #T).  Same command line, progress lines, header line
// and error messages; the histogram is built on the GPU while the .kmc_suf file streams through the staging slots of the count-table scan
// (bt_kmc_scan_kmer_stats_file).  There is no CPU path.
//
// Line order: the reference writes the lines in its unordered_map's iteration order, which is not part of its contract.  Here they are
// sorted by (count, A, C, G, T) — the order of the device histogram's bins — so two runs write byte-identical files.
//
// Checks that need no GPU (arguments, the table, k, the output file) all run before the GPU context is created.  A record whose count is
// above 255 (the reference asserts count <= 255, line 113) fails the run and no output file is written.
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/btgpu.h"
#include "KmcFile.hpp"
#include "Options.hpp"

using namespace bthost;

namespace {
const char *const BT_VERSION = "v1.5 (MI355X build)";
const uint64_t REPORT_EVERY = 10000000;   // getKmerStats.cpp:121-124

int error(const std::string &msg) {
    std::cerr << "\nERROR: " << msg << "\n" << std::endl;
    return 1;
}

bool readable(const std::string &path) { return ::access(path.c_str(), R_OK) == 0; }

// could the file be created or overwritten?  (checked without touching it: nothing is written before the histogram is complete)
bool writable(const std::string &path) {
    struct stat st;
    if (::stat(path.c_str(), &st) == 0) return S_ISREG(st.st_mode) && ::access(path.c_str(), W_OK) == 0;
    const size_t slash = path.find_last_of('/');
    const std::string dir = slash == std::string::npos ? "." : (slash == 0 ? "/" : path.substr(0, slash));
    return ::stat(dir.c_str(), &st) == 0 && S_ISDIR(st.st_mode) && ::access(dir.c_str(), W_OK | X_OK) == 0;
}

struct Progress {
    uint64_t next = REPORT_EVERY;
};

void report(uint64_t records_done, void *user) {   // after the chunk that crosses each multiple of 10^7 records
    Progress &p = *static_cast<Progress *>(user);
    while (records_done >= p.next) {
        std::cout << "[" << getLocalTime() << "] Parsed " << p.next << " kmers" << std::endl;
        p.next += REPORT_EVERY;
    }
}

void check(int rc, const char *what) {
    if (rc != BT_OK) throw std::runtime_error(std::string(what) + ": " + bt_last_error());
}

// the histogram of the whole table on the GPU; returns the number of records binned
uint64_t histogram(const KmcFile &db, std::vector<uint64_t> &hist, uint64_t &over255) {
    bt_ctx *ctx = nullptr;
    const char *dev = getenv("BT_DEVICE");
    check(bt_ctx_create(dev ? atoi(dev) : 0, &ctx), "bt_ctx_create");
    bt_kmc_scan *scan = nullptr;
    uint64_t binned = 0;
    Progress progress;
    try {
        check(bt_kmc_scan_create_bins(ctx, db.kmer_length, db.lut_prefix_length, db.counter_size, db.total_kmers, db.prefix_lut().data(), db.prefix_lut().size(), &scan),
              "bt_kmc_scan_create");
        check(bt_kmc_scan_set_count_range(scan, db.min_count, db.max_count), "bt_kmc_scan_set_count_range");   // ReadNextKmer's counter filter (kmc_file.cpp:496-511)
        const auto t0 = std::chrono::steady_clock::now();
        check(bt_kmc_scan_kmer_stats_file(scan, db.suffix_file().c_str(), 4, 0, db.total_kmers, 0, hist.data(), &binned, &over255, report, &progress),
              "bt_kmc_scan_kmer_stats_file");
        if (getenv("BT_STAGE_TIMES")) {
            const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            fprintf(stderr, "  kmer stats: %llu records in %.6f s = %g records/s (stream + histogram + histogram download)\n", (unsigned long long)db.total_kmers, s,
                    db.total_kmers / s);
        }
    } catch (...) {
        if (scan) bt_kmc_scan_destroy(scan);
        bt_ctx_destroy(ctx);
        throw;
    }
    bt_kmc_scan_destroy(scan);
    bt_ctx_destroy(ctx);
    return binned;
}
}  // namespace

int main(int argc, char const *argv[]) {
    if (argc != 3) {
        std::cout << "USAGE: getKmerStats <kmc_table_prefix> <output_prefix>" << std::endl;
        return 1;
    }
    const unsigned kmer_size = getenv("BT_KMER_SIZE") ? (unsigned)atoi(getenv("BT_KMER_SIZE")) : 55u;
    std::cout << "\n[" << getLocalTime() << "] Running BayesTyperTools (" << BT_VERSION << ") getKmerStats script ...\n" << std::endl;
    if (kmer_size < 1 || kmer_size > 64) return error("BT_KMER_SIZE must be between 1 and 64");
    const std::string prefix = argv[1];
    const std::string out_path = std::string(argv[2]) + "_kmer_stats.txt";
    if (!readable(prefix + ".kmc_pre") || !readable(prefix + ".kmc_suf")) return error("Unable to open KMC table " + prefix);   // OpenForListing failed
    try {
        KmcFile db(prefix);   // KMC1 and KMC2; refuses mode-1 (quality-weighted) tables
        if (db.kmer_length != kmer_size)
            return error("KMC table " + prefix + " holds " + std::to_string(db.kmer_length) + "-mers, not " + std::to_string(kmer_size) + "-mers (BT_KMER_SIZE)");
        if (!writable(out_path)) return error("Unable to write file " + out_path);
        std::cout << "[" << getLocalTime() << "] Parsing kmer table containing " << db.total_kmers << " unique kmers with a length of " << db.kmer_length << " nts ...\n"
                  << std::endl;
        std::vector<uint64_t> hist(bt_kmer_stats_num_bins(kmer_size), 0);
        uint64_t over255 = 0;
        const uint64_t num_kmers = histogram(db, hist, over255);
        if (over255)
            return error(std::to_string(over255) + " kmer(s) in KMC table " + prefix + " have a count above 255, the largest count getKmerStats supports; no statistics written");
        std::ofstream stats_outfile(out_path);
        if (!stats_outfile.is_open()) return error("Unable to write file " + out_path);
        stats_outfile << "NumberOfKmers\tKmerCount\tAdenineCount\tCytosineCount\tGuanineCount\tThymineCount\n";
        // bins in index order = lines sorted by (count, A, C, G, T) (include/btgpu.h: bt_kmer_stats_num_bins)
        uint64_t bin = 0;
        for (unsigned count = 0; count < 256; ++count)
            for (unsigned a = 0; a <= kmer_size; ++a)
                for (unsigned c = 0; a + c <= kmer_size; ++c)
                    for (unsigned g = 0; a + c + g <= kmer_size; ++g, ++bin)
                        if (hist[bin]) stats_outfile << hist[bin] << "\t" << count << "\t" << a << "\t" << c << "\t" << g << "\t" << kmer_size - a - c - g << "\n";
        stats_outfile.close();
        if (!stats_outfile) return error("Unable to write file " + out_path);
        std::cout << "\n[" << getLocalTime() << "] Wrote statistics for " << num_kmers << " kmers" << std::endl;
        std::cout << std::endl;
    } catch (const std::exception &e) {
        return error(e.what());
    }
    return 0;
}
