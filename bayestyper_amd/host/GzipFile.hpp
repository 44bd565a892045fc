// An ordinary gzip file (RFC 1952: one long member, or a few, as gzip, pigz and most archives write them) as slabs of raw compressed bytes, read with pread,
// for the stream object of libbtgpu that inflates them on the device (include/btgpu.h: bt_fastq_gz_scan_text).  The slabs are cut anywhere: the stream object
// carries what a slab leaves open.  The counterpart of BgzfFastqFile (BgzfFile.hpp) for a FASTQ that is gzip but not BGZF.  No GPU.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace bthost {

class GzipFastqFile {
   public:
    // slab_bytes: the compressed bytes per slab.  Throws std::runtime_error for a file that cannot be opened.
    GzipFastqFile(const std::string &path, size_t slab_bytes);
    ~GzipFastqFile();
    GzipFastqFile(const GzipFastqFile &) = delete;
    GzipFastqFile &operator=(const GzipFastqFile &) = delete;

    // the next slab -> out; false when the file is exhausted
    bool next(std::vector<uint8_t> &out);
    uint64_t slabOffset() const { return slab_offset_; }   // file offset of the slab next() returned last
    uint64_t fileBytes() const { return file_bytes_; }

   private:
    std::string path_;
    int fd_ = -1;
    size_t slab_bytes_;
    uint64_t file_bytes_ = 0, at_ = 0, slab_offset_ = 0;
};

// true: the file starts 1f 8b 08, is not BGZF by isBgzfFastq's own test of the header, and the first inflated byte (host zlib over the file's first bytes) is
// '@'.  A .fasta.gz, a gzip file whose first member is empty and a damaged header are false: they stay with zlib on the host.  Throws std::runtime_error for a
// file that cannot be read.
bool isGzipFastq(const std::string &path);
// BT_FASTQ_GZIP_ON_DEVICE set to anything but "" and "0": such files are inflated on the device; otherwise with zlib on the host, as before
bool fastqGzipOnDevice();
// BT_GUNZIP_CHUNK_BYTES: the chunk size handed to bt_fastq_gz_scan_create; unset or 0: the library's default
uint32_t gunzipChunkBytes();

}  // namespace bthost
