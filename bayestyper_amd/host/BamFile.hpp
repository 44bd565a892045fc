// A BAM file (SAM specification sections 4.1, 4.2) as slabs of whole compressed BGZF blocks for the stream object of libbtgpu (include/btgpu.h:
// bt_bam_scan_text), which inflates them and turns the records into reads text on the device.  The host only finds the blocks' boundaries, and inflates the
// leading block(s) with zlib as far as it takes to step over the header (magic, text, reference list — it may span several blocks).  No GPU, no libbtgpu.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace bthost {

class BamFile {
   public:
    // true: the file starts with a BGZF block whose data starts with "BAM\1".  A FASTA / FASTQ compressed as BGZF is not a BAM (false: zlib reads it as the
    // gzip it is).  Throws std::runtime_error for CRAM magic (said so in the message) and for a file that cannot be read.
    static bool isBam(const std::string &path);

    // slab_bytes: the most compressed bytes per slab, at least one block (65536).  Reads the header; throws on a damaged one.
    BamFile(const std::string &path, size_t slab_bytes);
    ~BamFile();
    BamFile(const BamFile &) = delete;
    BamFile &operator=(const BamFile &) = delete;

    // the next slab of whole blocks (read with pread) -> out; false when the file is exhausted.  The first slab starts at the block that holds the header's
    // last byte (or the first record); skipFirstBytes() of its data belong to the header.  Throws on a damaged block header or a file that ends inside a block.
    bool next(std::vector<uint8_t> &out);
    uint64_t skipFirstBytes() const { return skip_first_; }
    uint64_t slabOffset() const { return slab_offset_; }   // file offset of the slab next() returned last
    uint64_t headerBytes() const { return header_bytes_; }
    uint32_t references() const { return n_ref_; }
    uint64_t fileBytes() const { return file_bytes_; }
    bool hasEofBlock() const { return has_eof_; }   // a missing one is worth a warning (a file cut at a block boundary looks like this), not an error

   private:
    [[noreturn]] void fail(const std::string &what) const;

    std::string path_;
    int fd_ = -1;
    size_t slab_bytes_;
    uint64_t file_bytes_ = 0, at_ = 0, slab_offset_ = 0, skip_first_ = 0, header_bytes_ = 0;
    uint32_t n_ref_ = 0;
    bool has_eof_ = false;
};

// BT_BAM_SKIP_FLAGS, or 0x900 (secondary and supplementary alignments: every read counts once).  Throws when the value is not a number below 65536.
uint32_t bamSkipFlags();

}  // namespace bthost
