// A file of BGZF blocks (SAM specification section 4.1) as slabs of whole compressed blocks, read with pread, for the stream objects of libbtgpu
// (include/btgpu.h: bt_bam_scan_text, bt_fastq_scan_text), which inflate them on the device.  The host only finds the blocks' boundaries.  BamFile steps over
// the BAM header first; BgzfFastqFile delivers a BGZF-compressed FASTQ from its first block on.  No GPU.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace bthost {

class BgzfFile {
   public:
    BgzfFile(const BgzfFile &) = delete;
    BgzfFile &operator=(const BgzfFile &) = delete;

    // the next slab of whole blocks (read with pread) -> out; false when the file is exhausted.  Throws on a damaged block header or a file that ends inside a block.
    bool next(std::vector<uint8_t> &out);
    uint64_t slabOffset() const { return slab_offset_; }   // file offset of the slab next() returned last
    uint64_t fileBytes() const { return file_bytes_; }
    bool hasEofBlock() const { return has_eof_; }   // a missing one is worth a warning (a file cut at a block boundary looks like this), not an error

   protected:
    // slab_bytes: the most compressed bytes per slab, at least one block (65536).  Opens the file; the slabs start at offset 0 until a derived class moves at_.
    BgzfFile(const std::string &path, size_t slab_bytes);
    ~BgzfFile();
    [[noreturn]] void fail(const std::string &what) const;

    std::string path_;
    int fd_ = -1;
    size_t slab_bytes_;
    uint64_t file_bytes_ = 0, at_ = 0, slab_offset_ = 0;
    bool has_eof_ = false;
    std::string not_bgzf_advice_;   // appended to "not a BGZF block header" (what else the bytes may be, and what to do)
};

// A FASTQ file compressed as BGZF (what `bgzip` and the sequencers' converters write): its slabs, from the first block on.
class BgzfFastqFile : public BgzfFile {
   public:
    BgzfFastqFile(const std::string &path, size_t slab_bytes);
};

// true: the file starts with a BGZF block that passes every header check of bt_bgzf_scan_blocks, and the first data byte of the first block with ISIZE > 0 is
// '@'.  Throws std::runtime_error for a file that cannot be read.
bool isBgzfFastq(const std::string &path);
// BT_FASTQ_BGZF_ON_HOST set to anything but "" and "0": such files are read with zlib on the host, as every other FASTQ file
bool fastqBgzfOnHost();

namespace bgzf_detail {   // shared with BamFile.cpp
constexpr uint32_t kNeedMore = 0xFFFFFFFFu;
constexpr size_t kBlockMax = 65536;
uint32_t rd16(const uint8_t *p);
uint32_t rd32(const uint8_t *p);
uint32_t bgzfBlockSize(const uint8_t *head, size_t avail, uint32_t *payload_at);
size_t preadAll(int fd, uint8_t *buf, size_t n, uint64_t offset);
uint32_t inflateBlockAt(int fd, uint64_t offset, std::vector<uint8_t> &data, std::string &what);
}  // namespace bgzf_detail

}  // namespace bthost
