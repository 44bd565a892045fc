#include "BgzfFile.hpp"

#include <zlib.h>

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

namespace bthost {

namespace {
const uint8_t kEofBlock[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
}

namespace bgzf_detail {

uint32_t rd16(const uint8_t *p) { return p[0] | ((uint32_t)p[1] << 8); }
uint32_t rd32(const uint8_t *p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// SAM 4.1: head[0..avail) -> the block's size (BSIZE + 1) and where its payload starts; 0: not a BGZF header; kNeedMore: the extra field is not all there
uint32_t bgzfBlockSize(const uint8_t *head, size_t avail, uint32_t *payload_at) {
    if (avail < 12) return kNeedMore;
    if (head[0] != 0x1f || head[1] != 0x8b || head[2] != 8 || head[3] != 4) return 0;
    const uint32_t xlen = rd16(head + 10);
    if (12 + (size_t)xlen > avail) return kNeedMore;
    uint32_t size = 0;
    for (uint32_t at = 0; at + 4 <= xlen;) {
        const uint8_t *f = head + 12 + at;
        const uint32_t slen = rd16(f + 2);
        if (at + 4 + slen > xlen) return 0;
        if (f[0] == 'B' && f[1] == 'C') {
            if (slen != 2 || size) return 0;
            size = rd16(f + 4) + 1;
        }
        at += 4 + slen;
    }
    if (size < 12 + xlen + 8) return 0;
    *payload_at = 12 + xlen;
    return size;
}

size_t preadAll(int fd, uint8_t *buf, size_t n, uint64_t offset) {
    size_t got = 0;
    while (got < n) {
        const ssize_t r = pread(fd, buf + got, n - got, (off_t)(offset + got));
        if (r < 0) {
            if (errno == EINTR) continue;
            throw std::runtime_error(std::string("read error: ") + std::strerror(errno));
        }
        if (r == 0) break;
        got += (size_t)r;
    }
    return got;
}

// the block at `offset`, inflated with zlib and appended to data -> the block's size; 0 at the end of the file.  what: set to the fault for a damaged block.
uint32_t inflateBlockAt(int fd, uint64_t offset, std::vector<uint8_t> &data, std::string &what) {
    uint8_t block[kBlockMax];
    const size_t got = preadAll(fd, block, sizeof block, offset);
    if (got == 0) return 0;
    uint32_t payload_at = 0;
    const uint32_t size = bgzfBlockSize(block, got, &payload_at);
    if (size == 0 || size == kNeedMore || size > got) {
        what = size == 0 ? "not a BGZF block header" : "the file ends inside a BGZF block";
        return 0;
    }
    const uint32_t isize = rd32(block + size - 4);
    if (isize > kBlockMax) {
        what = "ISIZE above 65536";
        return 0;
    }
    const size_t before = data.size();
    data.resize(before + isize);
    z_stream z;
    std::memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) throw std::runtime_error("inflateInit2 failed");
    z.next_in = block + payload_at;
    z.avail_in = size - 8 - payload_at;
    uint8_t none = 0;
    z.next_out = isize ? data.data() + before : &none;
    z.avail_out = isize;
    const int rc = inflate(&z, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && z.total_out == isize && crc32(crc32(0L, Z_NULL, 0), data.data() + before, isize) == rd32(block + size - 8);
    inflateEnd(&z);
    if (!ok) {
        what = "damaged deflate data, length or CRC-32";
        return 0;
    }
    return size;
}

}  // namespace bgzf_detail

using namespace bgzf_detail;

BgzfFile::BgzfFile(const std::string &path, size_t slab_bytes) : path_(path), slab_bytes_(std::max<size_t>(slab_bytes, kBlockMax)) {
    fd_ = open(path.c_str(), O_RDONLY);
    if (fd_ < 0) throw std::runtime_error("Unable to open read file " + path);
    try {
        struct stat sb;
        if (fstat(fd_, &sb) != 0) fail("cannot stat");
        file_bytes_ = (uint64_t)sb.st_size;
        uint8_t tail[sizeof kEofBlock];
        has_eof_ = file_bytes_ >= sizeof tail && preadAll(fd_, tail, sizeof tail, file_bytes_ - sizeof tail) == sizeof tail && std::memcmp(tail, kEofBlock, sizeof tail) == 0;
    } catch (...) {   // (no destructor runs for a constructor that throws)
        close(fd_);
        fd_ = -1;
        throw;
    }
}

BgzfFile::~BgzfFile() {
    if (fd_ >= 0) close(fd_);
}

void BgzfFile::fail(const std::string &what) const { throw std::runtime_error("read file " + path_ + ": " + what); }

bool BgzfFile::next(std::vector<uint8_t> &out) {
    out.clear();
    if (at_ >= file_bytes_) return false;
    out.resize((size_t)std::min<uint64_t>(slab_bytes_, file_bytes_ - at_));
    const size_t got = preadAll(fd_, out.data(), out.size(), at_);
    size_t used = 0;
    while (used < got) {
        uint32_t payload_at = 0;
        const uint32_t size = bgzfBlockSize(out.data() + used, got - used, &payload_at);
        if (size == 0) fail("BGZF block at offset " + std::to_string(at_ + used) + ": not a BGZF block header" + not_bgzf_advice_);
        if (size == kNeedMore || size > got - used) break;
        used += size;
    }
    if (used == 0) fail("BGZF block at offset " + std::to_string(at_) + ": the file ends inside the block: truncated");
    out.resize(used);
    slab_offset_ = at_;
    at_ += used;
    return true;
}

BgzfFastqFile::BgzfFastqFile(const std::string &path, size_t slab_bytes) : BgzfFile(path, slab_bytes) {
    not_bgzf_advice_ = " (the file starts as BGZF and goes on as something else, a plain gzip member perhaps; BT_FASTQ_BGZF_ON_HOST=1 reads such a file with zlib on the host)";
}

bool isBgzfFastq(const std::string &path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) throw std::runtime_error("Unable to open read file " + path);
    bool fastq = false;
    try {
        std::vector<uint8_t> data;
        std::string what;
        for (uint64_t at = 0; data.empty();) {   // (the first block may be empty)
            const uint32_t size = inflateBlockAt(fd, at, data, what);
            if (!size) break;
            at += size;
        }
        fastq = !data.empty() && data[0] == '@';
    } catch (...) {
        close(fd);
        throw;
    }
    close(fd);
    return fastq;
}

bool fastqBgzfOnHost() {
    const char *v = getenv("BT_FASTQ_BGZF_ON_HOST");
    return v && *v && std::strcmp(v, "0") != 0;
}

}  // namespace bthost
