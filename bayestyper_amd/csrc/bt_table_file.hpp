// The k-mer table checkpoint file (bt_table_save / bt_table_load / bt_table_file_info, SURVEY §5 "Checkpoint / resume"): plain host code, no HIP.
//
// Everything is little endian and unaligned (fields are copied, never cast):
//   header   magic "BTAMDKTBL1" (10) | u32 version | u32 k | u32 num_samples | u32 record_bytes | u64 num_records | u64 max_chunk_records |
//            u32 manifest_len | manifest text | u32 crc32 of every header byte before it
//   chunk    "CHNK" | u64 n (1 .. max_chunk_records) | n packed records | u32 crc32 of (n, records)          — zero or more
//   trailer  "TEND" | u64 num_records | u32 crc32 of (the count)                                               — then the end of the file
// A packed record is 16 key bytes (lo, hi), the 4 meta bytes (flags, max haploid multiplicity, female and male inter-cluster multiplicity) and the
// samples' counts padded with zeros to a multiple of four: record_bytes = 20 + ((num_samples + 3) & ~3).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <string>

namespace btfile {

constexpr char MAGIC[] = "BTAMDKTBL1";
constexpr size_t MAGIC_LEN = 10;
constexpr uint32_t VERSION = 1;
constexpr size_t FIXED_HEADER = MAGIC_LEN + 4 * 4 + 8 + 8 + 4;
constexpr uint32_t MAX_MANIFEST = 1u << 24;
constexpr char CHUNK_TAG[] = "CHNK", TRAILER_TAG[] = "TEND";

struct Header {
    uint32_t version = 0, k = 0, num_samples = 0, record_bytes = 0;
    uint64_t num_records = 0, max_chunk_records = 0;
    std::string manifest;
};

inline uint32_t record_bytes_for(uint32_t num_samples) { return 20u + ((num_samples + 3u) & ~3u); }

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

inline std::string header_bytes(const Header &h) {
    std::string s(MAGIC, MAGIC_LEN);
    put<uint32_t>(s, VERSION);
    put<uint32_t>(s, h.k);
    put<uint32_t>(s, h.num_samples);
    put<uint32_t>(s, h.record_bytes);
    put<uint64_t>(s, h.num_records);
    put<uint64_t>(s, h.max_chunk_records);
    put<uint32_t>(s, (uint32_t)h.manifest.size());
    s += h.manifest;
    put<uint32_t>(s, crc(0, s.data(), s.size()));
    return s;
}

// "" when the texts are equal, else the first line that differs (1-based) with both versions
inline std::string manifest_difference(const std::string &stored, const std::string &expected) {
    if (stored == expected) return "";
    size_t a = 0, b = 0, line = 1;
    while (true) {
        const size_t ea = stored.find('\n', a), eb = expected.find('\n', b);
        const std::string la = a < stored.size() ? stored.substr(a, ea == std::string::npos ? ea : ea - a) : "<end of manifest>";
        const std::string lb = b < expected.size() ? expected.substr(b, eb == std::string::npos ? eb : eb - b) : "<end of manifest>";
        if (la != lb || a >= stored.size() || b >= expected.size())
            return "manifest line " + std::to_string(line) + " differs: the file has \"" + la + "\", this run has \"" + lb + "\"";
        a = ea == std::string::npos ? stored.size() : ea + 1;
        b = eb == std::string::npos ? expected.size() : eb + 1;
        ++line;
    }
}

// Sequential reader: open() verifies the header; next_chunk() + read_records() walk the chunks (the caller owns the buffer, so a chunk can land in pinned
// memory or be skimmed in pieces); next_chunk() verifies the trailer and the end of the file when no chunk is left.  Every function returns false with
// `error` set — the message names the file and the defect.
class Reader {
  public:
    Header header;
    std::string error;
    ~Reader() { close(); }
    void close() {
        if (f) fclose(f);
        f = nullptr;
    }
    bool open(const char *p) {
        path = p;
        f = fopen(p, "rb");
        if (!f) return fail("cannot open");
        uint8_t fixed[FIXED_HEADER];
        if (fread(fixed, 1, FIXED_HEADER, f) != FIXED_HEADER) return fail("truncated header");
        if (memcmp(fixed, MAGIC, MAGIC_LEN) != 0) return fail("bad magic (not a k-mer table checkpoint)");
        const uint8_t *q = fixed + MAGIC_LEN;
        header.version = get<uint32_t>(q);
        header.k = get<uint32_t>(q + 4);
        header.num_samples = get<uint32_t>(q + 8);
        header.record_bytes = get<uint32_t>(q + 12);
        header.num_records = get<uint64_t>(q + 16);
        header.max_chunk_records = get<uint64_t>(q + 24);
        const uint32_t mlen = get<uint32_t>(q + 32);
        // (a damaged length must not become an allocation: the CRC is checked after the manifest has been read)
        if (mlen > MAX_MANIFEST) return fail("header CRC mismatch (manifest length " + std::to_string(mlen) + ")");
        header.manifest.resize(mlen);
        uint8_t c[4];
        if ((mlen && fread(&header.manifest[0], 1, mlen, f) != mlen) || fread(c, 1, 4, f) != 4) return fail("truncated header");
        uint32_t sum = crc(0, fixed, FIXED_HEADER);
        sum = crc(sum, header.manifest.data(), mlen);
        if (sum != get<uint32_t>(c)) return fail("header CRC mismatch");
        if (header.version != VERSION) return fail("unsupported version " + std::to_string(header.version));
        if (header.k < 1 || header.k > 64 || header.num_samples < 1 || header.num_samples > 30 || header.record_bytes != record_bytes_for(header.num_samples))
            return fail("inconsistent header (k " + std::to_string(header.k) + ", " + std::to_string(header.num_samples) + " samples, " + std::to_string(header.record_bytes) + "-byte records)");
        if (header.max_chunk_records == 0 && header.num_records != 0) return fail("inconsistent header (records but no chunk size)");
        return true;
    }
    // *n = records of the next chunk, 0 after the (verified) trailer
    bool next_chunk(uint64_t *n) {
        uint8_t head[12];
        const size_t got = fread(head, 1, 12, f);
        if (got == 12 && memcmp(head, TRAILER_TAG, 4) == 0) {
            uint8_t c[4];
            if (fread(c, 1, 4, f) != 4) return fail("truncated trailer");
            if (crc(0, head + 4, 8) != get<uint32_t>(c)) return fail("trailer CRC mismatch");
            if (get<uint64_t>(head + 4) != header.num_records || seen != header.num_records)
                return fail("record count mismatch: header " + std::to_string(header.num_records) + ", chunks " + std::to_string(seen) + ", trailer " + std::to_string(get<uint64_t>(head + 4)));
            if (fgetc(f) != EOF) return fail("data after the trailer");
            *n = 0;
            return true;
        }
        if (got >= 4 && got < 12 && memcmp(head, TRAILER_TAG, 4) == 0) return fail("truncated trailer");
        if (got < 12) return fail(got == 0 ?"missing trailer (the file ends after " + std::to_string(seen) + " of " + std::to_string(header.num_records) + " records)" : "truncated chunk header");
        if (memcmp(head, CHUNK_TAG, 4) != 0) return fail("damaged chunk header after " + std::to_string(seen) + " records");
        pending = get<uint64_t>(head + 4);
        if (pending == 0 || pending > header.max_chunk_records || pending > header.num_records - seen) return fail("damaged chunk header after " + std::to_string(seen) + " records (chunk size " + std::to_string(pending) + ")");
        sum = crc(0, head + 4, 8);
        *n = pending;
        return true;
    }
    // the next m records of the current chunk (m <= what is left of it); the chunk's CRC is checked with its last record
    bool read_records(uint8_t *dst, uint64_t m) {
        const size_t bytes = (size_t)(m * header.record_bytes);
        if (m > pending) return fail("internal: read past the chunk");
        if (fread(dst, 1, bytes, f) != bytes) return fail("truncated in a chunk (after " + std::to_string(seen) + " of " + std::to_string(header.num_records) + " records)");
        sum = crc(sum, dst, bytes);
        pending -= m;
        seen += m;
        if (pending == 0) {
            uint8_t c[4];
            if (fread(c, 1, 4, f) != 4) return fail("truncated in a chunk (its CRC is missing)");
            if (sum != get<uint32_t>(c)) return fail("chunk CRC mismatch (records " + std::to_string(seen - m) + " .. " + std::to_string(seen) + " are damaged)");
        }
        return true;
    }

  private:
    FILE *f = nullptr;
    std::string path;
    uint64_t pending = 0, seen = 0;
    uint32_t sum = 0;
    bool fail(const std::string &what) {
        error = "k-mer table checkpoint " + path + ": " + what;
        return false;
    }
};

// The writer's counterpart: header(), then chunk() per non-empty range, then finish() (trailer, flush, rename of <path>.tmp to <path>).  An object that is
// destroyed before finish() removes the temporary file.
class Writer {
  public:
    std::string error;
    ~Writer() {
        if (f) {
            fclose(f);
            remove(tmp.c_str());
        }
    }
    bool open(const char *p, const Header &h) {
        path = p;
        tmp = path + ".tmp";
        total = h.num_records;
        f = fopen(tmp.c_str(), "wb");
        if (!f) return fail("cannot create " + tmp);
        const std::string s = header_bytes(h);
        return out(s.data(), s.size());
    }
    bool chunk(const uint8_t *records, uint64_t n, uint32_t record_bytes) {
        std::string head(CHUNK_TAG, 4);
        put<uint64_t>(head, n);
        const size_t bytes = (size_t)(n * record_bytes);
        std::string tail;
        put<uint32_t>(tail, crc(crc(0, head.data() + 4, 8), records, bytes));
        written += n;
        return out(head.data(), head.size()) && out(records, bytes) && out(tail.data(), 4);
    }
    bool finish() {
        if (written != total) return fail("internal: " + std::to_string(written) + " records written, " + std::to_string(total) + " announced");
        std::string s(TRAILER_TAG, 4);
        put<uint64_t>(s, total);
        put<uint32_t>(s, crc(0, s.data() + 4, 8));
        if (!out(s.data(), s.size())) return false;
        const bool ok = fflush(f) == 0;
        const bool closed = fclose(f) == 0;
        f = nullptr;
        if (!ok || !closed || rename(tmp.c_str(), path.c_str()) != 0) {
            remove(tmp.c_str());
            return fail("cannot complete " + path + " (disk full?)");
        }
        return true;
    }

  private:
    FILE *f = nullptr;
    std::string path, tmp;
    uint64_t total = 0, written = 0;
    bool out(const void *p, size_t n) {
        if (n && fwrite(p, 1, n, f) != n) return fail("write to " + tmp + " failed (disk full?)");
        return true;
    }
    bool fail(const std::string &what) {
        error = "k-mer table checkpoint: " + what;
        return false;
    }
};

}  // namespace btfile
