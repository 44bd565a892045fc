#include "GzipFile.hpp"

#include <zlib.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "BgzfFile.hpp"

namespace bthost {

using namespace bgzf_detail;

GzipFastqFile::GzipFastqFile(const std::string &path, size_t slab_bytes) : path_(path), slab_bytes_(std::max<size_t>(slab_bytes, 1)) {
    fd_ = open(path.c_str(), O_RDONLY);
    if (fd_ < 0) throw std::runtime_error("Unable to open read file " + path);
    struct stat sb;
    if (fstat(fd_, &sb) != 0) {
        close(fd_);
        fd_ = -1;
        throw std::runtime_error("read file " + path + ": cannot stat");
    }
    file_bytes_ = (uint64_t)sb.st_size;
}

GzipFastqFile::~GzipFastqFile() {
    if (fd_ >= 0) close(fd_);
}

bool GzipFastqFile::next(std::vector<uint8_t> &out) {
    out.clear();
    if (at_ >= file_bytes_) return false;
    out.resize((size_t)std::min<uint64_t>(slab_bytes_, file_bytes_ - at_));
    const size_t got = preadAll(fd_, out.data(), out.size(), at_);
    if (got == 0) throw std::runtime_error("read file " + path_ + ": the file ends at offset " + std::to_string(at_) + ", before its size");
    out.resize(got);
    slab_offset_ = at_;
    at_ += got;
    return true;
}

bool isGzipFastq(const std::string &path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) throw std::runtime_error("Unable to open read file " + path);
    uint8_t head[4096];
    size_t got = 0;
    try {
        got = preadAll(fd, head, sizeof head, 0);
    } catch (...) {
        close(fd);
        throw;
    }
    close(fd);
    if (got < 18 || head[0] != 0x1f || head[1] != 0x8b || head[2] != 8) return false;
    uint32_t payload_at = 0;
    if (bgzfBlockSize(head, got, &payload_at) != 0) return false;   // BGZF (or its extra field is not all there): isBgzfFastq's business
    z_stream z;
    std::memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 15 + 16) != Z_OK) throw std::runtime_error("inflateInit2 failed");
    uint8_t first[256];
    z.next_in = head;
    z.avail_in = (uInt)got;
    z.next_out = first;
    z.avail_out = sizeof first;
    const int rc = inflate(&z, Z_SYNC_FLUSH);
    const bool fastq = (rc == Z_OK || rc == Z_STREAM_END || rc == Z_BUF_ERROR) && z.total_out > 0 && first[0] == '@';
    inflateEnd(&z);
    return fastq;
}

bool fastqGzipOnDevice() {
    const char *v = getenv("BT_FASTQ_GZIP_ON_DEVICE");
    return v && *v && std::strcmp(v, "0") != 0;
}

uint32_t gunzipChunkBytes() {
    const char *v = getenv("BT_GUNZIP_CHUNK_BYTES");
    if (!v || !*v) return 0;
    char *end = nullptr;
    const unsigned long long n = std::strtoull(v, &end, 10);
    if (*end || n > 0xFFFFFFFFull) throw std::runtime_error(std::string("BT_GUNZIP_CHUNK_BYTES: not a number of bytes: ") + v);
    return (uint32_t)n;
}

}  // namespace bthost
