// The reads pack file (<prefix>.reads.pack: bt_reads_pack_writer_* / bt_reads_pack_reader_* / bt_reads_pack_file_info): the packed form of a sample's reads
// (bt_reads_pack.hpp) slab by slab, so that a later pass streams it instead of inflating and parsing the read files again.  Plain host code, no HIP, modelled on
// the k-mer table checkpoint (bt_table_file.hpp).
//
// Everything is little endian and unaligned (fields are copied, never cast):
//   header    magic "BTAMDRPK1" (9) | u32 version | u32 k | u32 block positions (128) | u32 manifest_len | manifest text | u32 crc32 of every header byte before it
//   section   "SECT" | u64 positions | u64 bases | u64 reads | 48 * ceil(positions / 128) payload bytes | u32 crc32 of (the three fields, the payload)   — zero or more
//   trailer   "REND" | u64 sections | u64 positions | u64 bases | u64 reads (the totals) | u32 crc32 of (the four fields)                                — then the end
// `bases` and `reads` are what the source reader counted for the slab (the overlap of a read cut at a slab's end counts once), so they are stored, not derived.
// k is recorded because a read longer than a slab is cut into pieces that overlap by k - 1 bases: a pack made at one k is stale at another.
#pragma once
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <string>
#include <vector>

namespace btpack {

constexpr char MAGIC[] = "BTAMDRPK1";
constexpr size_t MAGIC_LEN = 9;
constexpr uint32_t VERSION = 1, BLOCK_POSITIONS = 128, BLOCK_BYTES = 48;
constexpr size_t FIXED_HEADER = MAGIC_LEN + 4 * 4, SECTION_HEAD = 4 + 3 * 8, TRAILER_BYTES = 4 + 4 * 8 + 4;
constexpr uint32_t MAX_MANIFEST = 1u << 24;
constexpr char SECTION_TAG[] = "SECT", TRAILER_TAG[] = "REND";

inline uint64_t packed_bytes(uint64_t positions) { return (positions / BLOCK_POSITIONS + (positions % BLOCK_POSITIONS != 0)) * BLOCK_BYTES; }

template <typename T>
inline void put(std::string &s, T v) {
    for (size_t i = 0; i < sizeof(T); ++i) s.push_back((char)((v >> (8 * i)) & 0xFFu));
}
template <typename T>
inline T get(const uint8_t *p) {
    T v = 0;
    for (size_t i = 0; i < sizeof(T); ++i) v |= (T)p[i] << (8 * i);
    return v;
}
inline uint32_t crc(uint32_t seed, const void *p, size_t n) {   // zlib's crc32 takes a 32-bit length
    const uint8_t *b = (const uint8_t *)p;
    while (n) {
        const size_t m = n < (1u << 30) ? n : (1u << 30);
        seed = (uint32_t)crc32(seed, b, (uInt)m);
        b += m;
        n -= m;
    }
    return seed;
}

struct Totals {
    uint64_t sections = 0, positions = 0, bases = 0, reads = 0;
};
struct Section {
    uint64_t offset = 0, positions = 0, bases = 0, reads = 0;   // offset: of the section's tag in the file
};

// open() validates the header, walks the section heads (28 bytes each: nothing of a payload is read), validates the trailer against them and the end of the file
// against the trailer, all before anything is handed out; next() then reads one section's payload with pread() into the caller's buffer and checks its CRC.
// Every function returns false with `error` set — the message names the file and the defect.
class Reader {
  public:
    uint32_t version = 0, k = 0;
    std::string manifest, error;
    Totals totals;
    std::vector<Section> sections;
    uint64_t max_positions = 0;   // of one section
    ~Reader() { close(); }
    void close() {
        if (fd >= 0) ::close(fd);
        fd = -1;
    }
    bool open(const char *p) {
        path = p;
        fd = ::open(p, O_RDONLY);
        if (fd < 0) return fail("cannot open");
        struct stat st;
        if (fstat(fd, &st) != 0) return fail("cannot stat");
        const uint64_t size = (uint64_t)st.st_size;
        uint8_t fixed[FIXED_HEADER];
        if (!read_at(fixed, FIXED_HEADER, 0)) return fail("truncated header");
        if (memcmp(fixed, MAGIC, MAGIC_LEN) != 0) return fail("bad magic (not a reads pack)");
        const uint8_t *q = fixed + MAGIC_LEN;
        version = get<uint32_t>(q);
        k = get<uint32_t>(q + 4);
        const uint32_t block = get<uint32_t>(q + 8), mlen = get<uint32_t>(q + 12);
        // (a damaged length must not become an allocation: the CRC is checked after the manifest has been read)
        if (mlen > MAX_MANIFEST || FIXED_HEADER + (uint64_t)mlen + 4 > size) return fail("header CRC mismatch (manifest length " + std::to_string(mlen) + ")");
        manifest.resize(mlen);
        uint8_t c[4];
        if ((mlen && !read_at(&manifest[0], mlen, FIXED_HEADER)) || !read_at(c, 4, FIXED_HEADER + mlen)) return fail("truncated header");
        if (crc(crc(0, fixed, FIXED_HEADER), manifest.data(), mlen) != get<uint32_t>(c)) return fail("header CRC mismatch");
        if (version != VERSION) return fail("unsupported version " + std::to_string(version));
        if (k < 1 || k > 64 || block != BLOCK_POSITIONS) return fail("inconsistent header (k " + std::to_string(k) + ", blocks of " + std::to_string(block) + " positions)");
        uint64_t at = FIXED_HEADER + mlen + 4;
        Totals sum;
        while (true) {
            uint8_t head[SECTION_HEAD];
            const std::string where = "section " + std::to_string(sections.size()) + " at offset " + std::to_string(at);
            if (at == size) return fail("missing trailer (the file ends after " + std::to_string(sections.size()) + " sections)");
            if (size - at < 4 || !read_at(head, 4, at)) return fail("truncated in " + where);
            if (memcmp(head, TRAILER_TAG, 4) == 0) break;
            if (memcmp(head, SECTION_TAG, 4) != 0) return fail("damaged head of " + where);
            if (size - at < SECTION_HEAD || !read_at(head, SECTION_HEAD, at)) return fail("truncated in " + where);
            Section s;
            s.offset = at;
            s.positions = get<uint64_t>(head + 4);
            s.bases = get<uint64_t>(head + 12);
            s.reads = get<uint64_t>(head + 20);
            if (s.positions > (1ull << 48)) return fail("damaged head of " + where);
            const uint64_t bytes = SECTION_HEAD + packed_bytes(s.positions) + 4;
            if (size - at < bytes) return fail("truncated in " + where + " (" + std::to_string(size - at) + " of " + std::to_string(bytes) + " bytes)");
            at += bytes;
            sections.push_back(s);
            sum.sections++, sum.positions += s.positions, sum.bases += s.bases, sum.reads += s.reads;
            if (s.positions > max_positions) max_positions = s.positions;
        }
        uint8_t t[TRAILER_BYTES];
        if (size - at < TRAILER_BYTES || !read_at(t, TRAILER_BYTES, at)) return fail("truncated trailer");
        if (crc(0, t + 4, 32) != get<uint32_t>(t + 36)) return fail("trailer CRC mismatch");
        totals.sections = get<uint64_t>(t + 4), totals.positions = get<uint64_t>(t + 12), totals.bases = get<uint64_t>(t + 20), totals.reads = get<uint64_t>(t + 28);
        if (totals.sections != sum.sections || totals.positions != sum.positions || totals.bases != sum.bases || totals.reads != sum.reads)
            return fail("totals mismatch: the trailer states " + std::to_string(totals.sections) + " sections and " + std::to_string(totals.positions) + " positions, the sections have " +
                        std::to_string(sum.sections) + " and " + std::to_string(sum.positions));
        if (size - at != TRAILER_BYTES) return fail("data after the trailer");
        return true;
    }
    // the next section's payload into dst (capacity bytes); *end = true (and nothing else) after the last one
    bool next(uint8_t *dst, uint64_t capacity, Section *out, bool *end) {
        *end = cursor >= sections.size();
        if (*end) return true;
        const Section &s = sections[cursor];
        const std::string where = "section " + std::to_string(cursor) + " at offset " + std::to_string(s.offset);
        const uint64_t bytes = packed_bytes(s.positions);
        if (bytes > capacity) return fail("internal: buffer too small for " + where);
        uint8_t head[SECTION_HEAD], c[4];
        if (!read_at(head, SECTION_HEAD, s.offset) || !read_at(dst, bytes, s.offset + SECTION_HEAD) || !read_at(c, 4, s.offset + SECTION_HEAD + bytes))
            return fail("cannot read " + where);
        if (crc(crc(0, head + 4, 24), dst, bytes) != get<uint32_t>(c)) return fail(where + ": CRC mismatch (the section is damaged)");
        *out = s;
        ++cursor;
        return true;
    }

  private:
    int fd = -1;
    std::string path;
    size_t cursor = 0;
    bool read_at(void *dst, uint64_t n, uint64_t at) {
        uint8_t *p = (uint8_t *)dst;
        while (n) {
            const ssize_t got = pread(fd, p, n < (1u << 30) ? n : (1u << 30), (off_t)at);
            if (got <= 0) return false;
            p += got, at += (uint64_t)got, n -= (uint64_t)got;
        }
        return true;
    }
    bool fail(const std::string &what) {
        error = "reads pack " + path + ": " + what;
        return false;
    }
};

// The writer's counterpart: open() (header), section() per slab, finish() (trailer, flush, rename of <path>.tmp.<pid> to <path>).  An object that is destroyed
// before finish() removes the temporary file, and an interrupted process leaves no file under the final name.
class Writer {
  public:
    std::string error;
    Totals totals;
    ~Writer() {
        if (f) {
            fclose(f);
            remove(tmp.c_str());
        }
    }
    bool open(const char *p, uint32_t k, const std::string &manifest) {
        path = p;
        tmp = path + ".tmp." + std::to_string((long)getpid());
        if (k < 1 || k > 64) return fail("k must lie in 1 .. 64");
        if (manifest.size() > MAX_MANIFEST) return fail("manifest too long");
        f = fopen(tmp.c_str(), "wb");
        if (!f) return fail("cannot create " + tmp);
        std::string s(MAGIC, MAGIC_LEN);
        put<uint32_t>(s, VERSION);
        put<uint32_t>(s, k);
        put<uint32_t>(s, BLOCK_POSITIONS);
        put<uint32_t>(s, (uint32_t)manifest.size());
        s += manifest;
        put<uint32_t>(s, crc(0, s.data(), s.size()));
        return out(s.data(), s.size());
    }
    bool section(const uint8_t *packed, uint64_t positions, uint64_t bases, uint64_t reads) {
        if (!f) return fail("internal: no open file");
        std::string head(SECTION_TAG, 4);
        put<uint64_t>(head, positions);
        put<uint64_t>(head, bases);
        put<uint64_t>(head, reads);
        const size_t bytes = (size_t)packed_bytes(positions);
        std::string tail;
        put<uint32_t>(tail, crc(crc(0, head.data() + 4, 24), packed, bytes));
        totals.sections++, totals.positions += positions, totals.bases += bases, totals.reads += reads;
        return out(head.data(), head.size()) && out(packed, bytes) && out(tail.data(), 4);
    }
    bool finish() {
        if (!f) return fail("internal: no open file");
        std::string s(TRAILER_TAG, 4);
        put<uint64_t>(s, totals.sections);
        put<uint64_t>(s, totals.positions);
        put<uint64_t>(s, totals.bases);
        put<uint64_t>(s, totals.reads);
        put<uint32_t>(s, crc(0, s.data() + 4, 32));
        const bool written = out(s.data(), s.size());
        const bool ok = fflush(f) == 0;
        const bool closed = fclose(f) == 0;
        f = nullptr;
        if (!written || !ok || !closed || rename(tmp.c_str(), path.c_str()) != 0) {
            remove(tmp.c_str());
            return fail("cannot complete " + path + " (disk full?)");
        }
        return true;
    }

  private:
    FILE *f = nullptr;
    std::string path, tmp;
    bool out(const void *p, size_t n) {
        if (n && fwrite(p, 1, n, f) != n) return fail("write to " + tmp + " failed (disk full?)");
        return true;
    }
    bool fail(const std::string &what) {
        error = "reads pack " + path + ": " + what;
        return false;
    }
};

}  // namespace btpack
