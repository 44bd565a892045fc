// The manifest of a k-mer table checkpoint (BT_TABLE_CHECKPOINT=<file>, include/btgpu.h: bt_table_save / bt_table_load): one "name=value" line per
// item that determines the table a genotype run holds after parseSampleKmers — and nothing that does not (the seed, the Gibbs options, the filters and
// --noise-genotyping only act after it).  Two runs with equal manifests build equal tables, so the second may load the first one's.
#pragma once
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

namespace bthost {

struct TableCheckpointInputs {
    struct SampleDb {   // a sample and its KMC database (KmcFile's header fields, the size of the .kmc_suf file)
        std::string name;
        bool present = true;   // false: the database is not there (a run that loads the checkpoint does not need it); the line then reads "absent"
        uint64_t total_kmers = 0, suf_bytes = 0, max_count = 0;
        uint32_t counter_size = 0, min_count = 0;
        std::string reads_identity;   // not empty: the sample has no database and is counted from its reads (ReadsFile.hpp: readsIdentity); the line carries this instead
    };
    struct InputFile {   // variant_clusters.bin, parameter_kmers.fa.gz, intercluster_regions.txt.gz
        std::string what;
        uint64_t bytes = 0;
        uint32_t crc = 0;
    };
    struct Chromosome {
        std::string name;
        uint64_t length = 0;
        bool is_decoy = false;
        unsigned female_ploidy = 0, male_ploidy = 0;   // the inter-cluster multiplicities are stored per gender
    };
    unsigned kmer_size = 0;
    std::vector<SampleDb> samples;   // in the samples file's order: sample s owns count byte s
    std::vector<InputFile> files;
    std::vector<Chromosome> chromosomes;
};

inline std::string sampleDbLine(size_t s, const TableCheckpointInputs::SampleDb &db) {
    const std::string name = "sample." + std::to_string(s) + ".kmc=";
    if (!db.reads_identity.empty()) return name + db.reads_identity;
    if (!db.present) return name + "absent";
    return name + "total_kmers:" + std::to_string(db.total_kmers) + " suf_bytes:" + std::to_string(db.suf_bytes) + " counter_size:" + std::to_string(db.counter_size) +
           " min_count:" + std::to_string(db.min_count) + " max_count:" + std::to_string(db.max_count);
}

inline std::string tableCheckpointManifest(const TableCheckpointInputs &in) {
    std::string m = "k=" + std::to_string(in.kmer_size) + "\nsamples=" + std::to_string(in.samples.size()) + "\n";
    for (size_t s = 0; s < in.samples.size(); s++) m += "sample." + std::to_string(s) + ".name=" + in.samples[s].name + "\n" + sampleDbLine(s, in.samples[s]) + "\n";
    char hex[16];
    for (auto &f : in.files) {
        std::snprintf(hex, sizeof hex, "%08x", f.crc);
        m += "file." + f.what + "=bytes:" + std::to_string(f.bytes) + " crc32:" + hex + "\n";
    }
    for (auto &c : in.chromosomes)
        m += "chromosome." + c.name + "=length:" + std::to_string(c.length) + " decoy:" + (c.is_decoy ? "1" : "0") + " ploidy:" + std::to_string(c.female_ploidy) + "/" +
             std::to_string(c.male_ploidy) + "\n";
    return m;
}

// A run that loads a checkpoint does not need the samples' KMC databases; where one is absent its line cannot be derived and the checkpoint's own is
// taken over (the sample's name and position are still compared).  Returns `expected` with every "...kmc=absent" line replaced by `stored`'s line of that name.
inline std::string adoptAbsentDatabases(const std::string &expected, const std::string &stored) {
    std::string out;
    for (size_t a = 0; a < expected.size();) {
        const size_t e = std::min(expected.find('\n', a), expected.size());
        std::string line = expected.substr(a, e - a);
        const size_t eq = line.find('=');
        if (eq != std::string::npos && line.compare(eq, std::string::npos, "=absent") == 0) {
            const std::string name = line.substr(0, eq + 1);
            for (size_t b = 0; b < stored.size();) {
                const size_t f = std::min(stored.find('\n', b), stored.size());
                if (stored.compare(b, name.size(), name) == 0) line = stored.substr(b, f - b);
                b = f + 1;
            }
        }
        out += line + "\n";
        a = e + 1;
    }
    return out;
}

// size and CRC32 of a file's bytes
inline TableCheckpointInputs::InputFile inputFileIdentity(const std::string &what, const std::string &path) {
    TableCheckpointInputs::InputFile id;
    id.what = what;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("Unable to open file " + path);
    std::vector<unsigned char> buf(1u << 20);
    uLong crc = crc32(0L, Z_NULL, 0);
    for (size_t n; (n = std::fread(buf.data(), 1, buf.size(), f)) > 0;) {
        crc = crc32(crc, buf.data(), (uInt)n);
        id.bytes += n;
    }
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    if (bad) throw std::runtime_error("Unable to read file " + path);
    id.crc = (uint32_t)crc;
    return id;
}

}  // namespace bthost
