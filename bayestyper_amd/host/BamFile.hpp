// A BAM file (SAM specification sections 4.1, 4.2) as slabs of whole compressed BGZF blocks for the stream object of libbtgpu (include/btgpu.h:
// bt_bam_scan_text), which inflates them and turns the records into reads text on the device.  The host only finds the blocks' boundaries, and inflates the
// leading block(s) with zlib as far as it takes to step over the header (magic, text, reference list — it may span several blocks).  No GPU, no libbtgpu.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "BgzfFile.hpp"

namespace bthost {

class BamFile : public BgzfFile {
   public:
    // true: the file starts with a BGZF block whose data starts with "BAM\1".  A FASTA / FASTQ compressed as BGZF is not a BAM (false: a FASTQ goes the
    // way of BgzfFastqFile when isBgzfFastq says so, a FASTA is read by zlib as the gzip it is).  Throws std::runtime_error for CRAM magic (said so in the message) and for a file that cannot be read.
    static bool isBam(const std::string &path);

    // slab_bytes: the most compressed bytes per slab, at least one block (65536).  Reads the header; throws on a damaged one.
    BamFile(const std::string &path, size_t slab_bytes);

    // next() (BgzfFile): the first slab starts at the block that holds the header's last byte (or the first record); skipFirstBytes() of its data belong
    // to the header.
    uint64_t skipFirstBytes() const { return skip_first_; }
    uint64_t headerBytes() const { return header_bytes_; }
    uint32_t references() const { return n_ref_; }

   private:
    uint64_t skip_first_ = 0, header_bytes_ = 0;
    uint32_t n_ref_ = 0;
};

// BT_BAM_SKIP_FLAGS, or 0x900 (secondary and supplementary alignments: every read counts once).  Throws when the value is not a number below 65536.
uint32_t bamSkipFlags();

}  // namespace bthost
