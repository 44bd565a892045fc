#include "ReadsPack.hpp"

#include <sys/stat.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>
#include <set>
#include <stdexcept>

#include "BamFile.hpp"
#include "ReadsFile.hpp"

namespace bthost {

namespace {

const char *const BAM_LINE = "bam_skip_flags:";

bool envIs(const char *name, const char *value) {
    const char *v = getenv(name);
    return v && std::strcmp(v, value) == 0;
}

void warnOnce(const std::string &path, const std::string &what) {
    static std::mutex m;
    static std::set<std::string> warned;   // once per file and process: genotype reads a sample once per inference unit
    std::lock_guard<std::mutex> lock(m);
    if (warned.insert(path).second) std::cerr << "WARNING: " << what << std::endl;
}

void check(int rc, const std::string &what) {
    if (rc != BT_OK) throw std::runtime_error(what + ": " + bt_last_error());
}

}  // namespace

bool readsPackIgnored() { return envIs("BT_READS_PACK", "0"); }
bool readsPackWanted() { return envIs("BT_READS_PACK", "1"); }
std::string readsPackPath(const std::string &prefix) { return prefix + ".reads.pack"; }

std::string readsPackManifest(const std::string &prefix, unsigned kmer_size, bool names_bam) {
    std::string m = readsIdentity(prefix) + "\nk:" + std::to_string(kmer_size) + "\n";
    if (names_bam) m += BAM_LINE + std::to_string(bamSkipFlags()) + "\n";
    return m;
}

std::unique_ptr<ReadsPackReader> ReadsPackReader::openFor(const std::string &prefix, unsigned kmer_size) {
    if (readsPackIgnored()) return nullptr;
    const std::string path = readsPackPath(prefix);
    struct stat sb;
    if (stat(path.c_str(), &sb) != 0) return nullptr;
    bt_reads_pack_reader *r = nullptr;
    bt_reads_pack_info info;
    if (bt_reads_pack_reader_open(path.c_str(), &r, &info) != BT_OK) {
        warnOnce(path, std::string(bt_last_error()) + ": the read files are read instead");
        return nullptr;
    }
    std::string stored(info.manifest_bytes, '\0');
    uint64_t len = 0;
    if (bt_reads_pack_reader_manifest(r, stored.empty() ? nullptr : &stored[0], stored.size(), &len) != BT_OK) {
        bt_reads_pack_reader_close(r);
        throw std::runtime_error(std::string("reads pack ") + path + ": " + bt_last_error());
    }
    // (whether the list names a BAM is taken from the pack, so that no read file is opened to find out: with the same list and the same files it still does)
    const bool names_bam = stored.find(std::string("\n") + BAM_LINE) != std::string::npos;
    const std::string expected = readsPackManifest(prefix, kmer_size, names_bam);
    if (stored != expected) {
        bt_reads_pack_reader_close(r);
        size_t a = 0, b = 0;   // the first line that differs
        std::string la, lb;
        do {
            const size_t ea = std::min(stored.find('\n', a), stored.size()), eb = std::min(expected.find('\n', b), expected.size());
            la = stored.substr(a, ea - a), lb = expected.substr(b, eb - b);
            a = ea + 1, b = eb + 1;
        } while (la == lb && a < stored.size() && b < expected.size());
        warnOnce(path, "reads pack " + path + " is stale (it was made from \"" + la + "\", this run has \"" + lb + "\"): the read files are read instead");
        return nullptr;
    }
    return std::unique_ptr<ReadsPackReader>(new ReadsPackReader(r, info, path));
}

ReadsPackReader::~ReadsPackReader() { bt_reads_pack_reader_close(r_); }

ReadsPackTotals ReadsPackReader::forEachSection(const std::function<void(const uint8_t *, uint64_t)> &consume) {
    ReadsPackTotals totals;
    std::vector<uint32_t> buffer((size_t)(bt_reads_packed_bytes(info_.max_section_positions) / 4) + 1);   // 4-byte aligned
    uint8_t *bytes = reinterpret_cast<uint8_t *>(buffer.data());
    while (true) {
        uint64_t positions = 0, bases = 0, reads = 0;
        int end = 0;
        if (bt_reads_pack_reader_next(r_, bytes, buffer.size() * 4, &positions, &bases, &reads, &end) != BT_OK) throw std::runtime_error(bt_last_error());
        if (end) break;
        if (positions) consume(bytes, positions);
        totals.bases += bases;
        totals.reads += reads;
        totals.sections++;
    }
    if (totals.bases != info_.bases || totals.reads != info_.reads) throw std::runtime_error("reads pack " + path_ + ": the sections do not add up to the trailer's totals");
    return totals;
}

ReadsPackWriter::ReadsPackWriter(bt_ctx *ctx, const std::string &prefix, unsigned kmer_size, bool names_bam) : ctx_(ctx) {
    check(bt_reads_pack_writer_create(readsPackPath(prefix).c_str(), kmer_size, readsPackManifest(prefix, kmer_size, names_bam).c_str(), &w_), "reads pack");
}

ReadsPackWriter::~ReadsPackWriter() {
    if (w_) bt_reads_pack_writer_destroy(w_);
    if (d_packed_) bt_free(ctx_, d_packed_);
}

void ReadsPackWriter::packHost(const std::string &slab, std::vector<uint8_t> &packed) {
    packed.resize((size_t)bt_reads_packed_bytes(slab.size()));
    check(bt_diag_reads_pack(slab.data(), slab.size(), packed.data()), "bt_diag_reads_pack");
}

void ReadsPackWriter::addPacked(const std::vector<uint8_t> &packed, uint64_t positions, uint64_t bases, uint64_t reads) {
    check(bt_reads_pack_writer_add(w_, packed.data(), positions, bases, reads), "reads pack");
}

void ReadsPackWriter::addDeviceText(const char *d_text, uint64_t len, uint64_t bases, uint64_t reads) {
    const size_t bytes = (size_t)bt_reads_packed_bytes(len);
    if (bytes > d_capacity_) {
        if (d_packed_) bt_free(ctx_, d_packed_);
        d_packed_ = nullptr;
        d_capacity_ = 0;
        check(bt_malloc(ctx_, bytes + bytes / 4, &d_packed_), "bt_malloc");
        d_capacity_ = bytes + bytes / 4;
    }
    host_.resize(bytes);
    if (len) {
        check(bt_reads_pack(ctx_, d_text, len, (uint8_t *)d_packed_), "bt_reads_pack");
        check(bt_memcpy_d2h(ctx_, host_.data(), d_packed_, bytes), "bt_memcpy_d2h");   // (waits for the stream)
    }
    addPacked(host_, len, bases, reads);
}

void ReadsPackWriter::finish() {
    check(bt_reads_pack_writer_finish(w_), "reads pack");
}

}  // namespace bthost
