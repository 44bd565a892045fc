#include "BamFile.hpp"

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

using namespace bgzf_detail;

namespace {

// the header's length when data holds all of it (SAM 4.2: magic, l_text, text, n_ref, then l_name, name, l_ref per reference); 0: more data needed
uint64_t bamHeaderBytes(const std::vector<uint8_t> &data, uint32_t *n_ref, std::string &what) {
    if (data.size() >= 4 && std::memcmp(data.data(), "BAM\1", 4) != 0) {
        what = "no BAM magic";
        return 0;
    }
    if (data.size() < 12) return 0;
    const uint32_t l_text = rd32(data.data() + 4);
    if (l_text > 0x7FFFFFFFu) {
        what = "negative l_text";
        return 0;
    }
    uint64_t pos = 8 + (uint64_t)l_text;
    if (data.size() < pos + 4) return 0;
    const uint32_t refs = rd32(data.data() + pos);
    if (refs > 0x7FFFFFFFu) {
        what = "negative n_ref";
        return 0;
    }
    pos += 4;
    for (uint32_t i = 0; i < refs; i++) {
        if (data.size() < pos + 4) return 0;
        const uint32_t l_name = rd32(data.data() + pos);
        if (l_name > 0x7FFFFFFFu) {
            what = "negative l_name";
            return 0;
        }
        pos += 4 + (uint64_t)l_name + 4;
    }
    if (data.size() < pos) return 0;
    *n_ref = refs;
    return pos;
}

}  // namespace

bool BamFile::isBam(const std::string &path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) throw std::runtime_error("Unable to open read file " + path);
    bool bam = false;
    std::string cram;
    try {
        uint8_t magic[4] = {0, 0, 0, 0};
        const size_t got = preadAll(fd, magic, 4, 0);
        if (got == 4 && std::memcmp(magic, "CRAM", 4) == 0)
            cram = "read file " + path + ": CRAM is not supported (convert it with `samtools view -b`, or to FASTQ with `samtools fastq`)";
        else if (got == 4 && magic[0] == 0x1f && magic[1] == 0x8b) {
            std::vector<uint8_t> data;
            std::string what;
            for (uint64_t at = 0; data.size() < 4;) {   // (the first block may be empty)
                const uint32_t size = inflateBlockAt(fd, at, data, what);
                if (!size) break;
                at += size;
            }
            bam = data.size() >= 4 && std::memcmp(data.data(), "BAM\1", 4) == 0;
        }
    } catch (...) {
        close(fd);
        throw;
    }
    close(fd);
    if (!cram.empty()) throw std::runtime_error(cram);
    return bam;
}

BamFile::BamFile(const std::string &path, size_t slab_bytes) : BgzfFile(path, slab_bytes) {
    // the leading blocks, as far as the header reaches
    std::vector<uint8_t> data;
    std::vector<uint64_t> block_at, data_at;
    std::string what;
    uint64_t at = 0;
    while (!(header_bytes_ = bamHeaderBytes(data, &n_ref_, what))) {
        if (!what.empty()) fail("BAM header: " + what);
        block_at.push_back(at);
        data_at.push_back(data.size());
        const uint32_t size = inflateBlockAt(fd_, at, data, what);
        if (!size) fail(what.empty() ? "the file ends inside the BAM header: truncated" : "BGZF block at offset " + std::to_string(at) + ": " + what);
        at += size;
    }
    // the slabs start at the block that holds the first byte behind the header; when the header ends with its block, at the next block
    at_ = at;
    skip_first_ = 0;
    for (size_t b = 0; b < block_at.size(); b++) {
        const uint64_t end = b + 1 < data_at.size() ? data_at[b + 1] : data.size();
        if (end > header_bytes_) {
            at_ = block_at[b];
            skip_first_ = header_bytes_ - data_at[b];
            break;
        }
    }
}

uint32_t bamSkipFlags() {
    const char *v = getenv("BT_BAM_SKIP_FLAGS");
    if (!v) return 0x900;
    char *end = nullptr;
    errno = 0;
    const unsigned long long x = std::strtoull(v, &end, 0);
    if (!*v || *end || errno || x >= 65536 || *v == '-') throw std::runtime_error(std::string("BT_BAM_SKIP_FLAGS must be a number below 65536 (decimal, or hexadecimal with 0x), not '") + v + "'");
    return (uint32_t)x;
}

}  // namespace bthost
