// The reads pack of a sample, <prefix>.reads.pack (include/btgpu.h: bt_reads_pack_writer_* / bt_reads_pack_reader_*): the sample's reads as 2-bit codes and
// validity bits, written by the first pass over the read files when BT_READS_PACK=1 asks for it and streamed by every later pass instead of the files (SampleReads.hpp:
// forEachSampleReads).  BT_READS_PACK=0 ignores a pack that is there.  Without the variable and without a pack nothing here runs.
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/btgpu.h"

namespace bthost {

bool readsPackIgnored();   // BT_READS_PACK=0
bool readsPackWanted();    // BT_READS_PACK=1
std::string readsPackPath(const std::string &prefix);   // <prefix>.reads.pack
// What a pack is made of: readsIdentity(prefix), k (a read longer than a slab is cut into pieces that overlap by k - 1 bases) and, when the list names a BAM, the
// value of BT_BAM_SKIP_FLAGS.  Slab sizes, -p and the device-route switches change no k-mer and stay out.
std::string readsPackManifest(const std::string &prefix, unsigned kmer_size, bool names_bam);
// for the BT_STAGE_TIMES rows of the reads route
inline std::string readsPackNote(bool from_pack) { return from_pack ? " (from the reads pack)" : ""; }

struct ReadsPackTotals {
    uint64_t bases = 0, reads = 0, sections = 0;
};

// A pack that is present, whole (header, section heads, trailer, size) and made from what this run names; null when there is none, when BT_READS_PACK=0, or — with
// one warning per file and process — when it is damaged or stale.
class ReadsPackReader {
   public:
    static std::unique_ptr<ReadsPackReader> openFor(const std::string &prefix, unsigned kmer_size);
    ~ReadsPackReader();
    ReadsPackReader(const ReadsPackReader &) = delete;
    ReadsPackReader &operator=(const ReadsPackReader &) = delete;
    // every section to consume(packed bytes, positions); a section whose CRC-32 fails throws (the message names the section and its file offset)
    ReadsPackTotals forEachSection(const std::function<void(const uint8_t *, uint64_t)> &consume);
    const std::string &path() const { return path_; }

   private:
    ReadsPackReader(bt_reads_pack_reader *r, const bt_reads_pack_info &info, const std::string &path) : r_(r), info_(info), path_(path) {}
    bt_reads_pack_reader *r_;
    bt_reads_pack_info info_;
    std::string path_;
};

// The writer of one pass: sections are appended by one thread at a time; finish() renames the temporary file, a writer destroyed before it leaves nothing.
class ReadsPackWriter {
   public:
    ReadsPackWriter(bt_ctx *ctx, const std::string &prefix, unsigned kmer_size, bool names_bam);
    ~ReadsPackWriter();
    ReadsPackWriter(const ReadsPackWriter &) = delete;
    ReadsPackWriter &operator=(const ReadsPackWriter &) = delete;
    static void packHost(const std::string &slab, std::vector<uint8_t> &packed);   // bt_diag_reads_pack: any thread
    void addPacked(const std::vector<uint8_t> &packed, uint64_t positions, uint64_t bases, uint64_t reads);
    void addDeviceText(const char *d_text, uint64_t len, uint64_t bases, uint64_t reads);   // bt_reads_pack, copied back at 3/8 of the text's size
    void finish();

   private:
    bt_ctx *ctx_;
    bt_reads_pack_writer *w_ = nullptr;
    void *d_packed_ = nullptr;
    size_t d_capacity_ = 0;
    std::vector<uint8_t> host_;
};

}  // namespace bthost
