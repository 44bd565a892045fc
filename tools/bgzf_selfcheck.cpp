// Stand-alone host program for a sanitizer build (tools/bgzf_selfcheck.sh): bt_diag_bgzf and bt_diag_crc32 — the BGZF block code of
// bayestyper_amd/csrc/bt_bgzf.hpp run by a team of one thread — over the sizes of tests/test_bgzf_cpu.py (VCF-like text, random bytes, a run of one byte;
// built here again, in C++), every stream walked block by block, every payload inflated with zlib and compared with its slice, every CRC-32 compared with
// zlib's, the capacity rule at one byte short; then bthost::buildTabixIndex over a synthetic line table.  It uses no GPU.  Exit status 0: every call
// returned what it should.
#include <zlib.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../bayestyper_amd/csrc/bt_bgzf.hpp"
#include "../bayestyper_amd/host/TabixIndex.hpp"
#include "../include/btgpu.h"

namespace bt {   // what bt_bgzf.hip takes from bt_ctx.hip
static std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }
int fail(const std::string &msg) {
    set_error(msg);
    return BT_ERR;
}
}  // namespace bt

static int failures = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);      \
            ++failures;                                               \
        }                                                             \
    } while (0)

typedef std::vector<uint8_t> Bytes;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static Bytes random_bytes(size_t n) {
    Bytes b(n);
    for (auto &c : b) c = (uint8_t)rnd();
    return b;
}
static Bytes text(size_t n) {   // VCF-like lines
    std::string s;
    unsigned pos = 1000;
    while (s.size() < n) {
        pos += rnd() % 5000;
        char line[256];
        std::snprintf(line, sizeof line, "chr%u\t%u\t.\t%c\t%c\t%u.%02u\tPASS\tAC=%u;AF=0.%03u;AN=%u\tGT:GQ:GPP\t%u/%u:%u:0.%04u,0.%04u\n", 1 + rnd() % 22, pos, "ACGT"[rnd() % 4],
                      "ACGT"[rnd() % 4], rnd() % 100, rnd() % 100, rnd() % 7, rnd() % 1000, 2 * (1 + rnd() % 3), rnd() % 2, rnd() % 2, rnd() % 99, rnd() % 10000, rnd() % 10000);
        s += line;
    }
    s.resize(n);
    return Bytes(s.begin(), s.end());
}

static bool inflate_raw(const uint8_t *in, size_t n, size_t expect, Bytes &out) {
    z_stream zs;
    std::memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    out.assign(expect + 16, 0);
    zs.next_in = const_cast<Bytef *>(in);
    zs.avail_in = (uInt)n;
    zs.next_out = out.data();
    zs.avail_out = (uInt)out.size();
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.avail_in == 0;
    out.resize(out.size() - zs.avail_out);
    if (!ok) std::fprintf(stderr, "inflate: %d %s\n", rc, zs.msg ? zs.msg : "");
    inflateEnd(&zs);
    return ok;
}

static const uint8_t kEofBlock[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

static void check(const char *name, const Bytes &in) {
    uint64_t cap = 0, blocks = 0, n1 = 0;
    EXPECT(bt_bgzf_bound(in.size(), &cap, &blocks) == BT_OK && blocks == (in.size() + btbgzf::kBlock - 1) / btbgzf::kBlock);
    Bytes a(cap);
    std::vector<uint64_t> offsets(blocks + 1, 77);
    bt_deflate_stats st;
    EXPECT(bt_diag_bgzf(in.data(), in.size(), 1, a.data(), cap, &n1, offsets.data(), &st) == BT_OK && n1 <= cap && n1 >= 28);
    uint64_t at = 0;
    for (uint64_t b = 0; b < blocks; ++b) {   // the walk
        const size_t len = std::min<size_t>(btbgzf::kBlock, in.size() - b * btbgzf::kBlock);
        EXPECT(offsets[b] == at && at + 26 <= n1);
        EXPECT(std::memcmp(a.data() + at, kEofBlock, 16) == 0);   // (the first 16 bytes of every block are the EOF block's)
        const uint32_t size = (a[at + 16] | a[at + 17] << 8) + 1u;
        EXPECT(size <= 65536 && at + size + 28 <= n1);
        if (at + size > n1) break;
        Bytes back;
        EXPECT(inflate_raw(a.data() + at + 18, size - 26, len, back) && back.size() == len && std::memcmp(back.data(), in.data() + b * btbgzf::kBlock, len) == 0);
        uint32_t crc, isize;
        std::memcpy(&crc, a.data() + at + size - 8, 4);
        std::memcpy(&isize, a.data() + at + size - 4, 4);
        EXPECT(crc == (uint32_t)crc32(crc32(0L, Z_NULL, 0), in.data() + b * btbgzf::kBlock, (uInt)len) && isize == len);
        at += size;
    }
    EXPECT(offsets[blocks] == at && at + 28 == n1 && std::memcmp(a.data() + at, kEofBlock, 28) == 0);
    Bytes small(cap - 1, 0xAA);
    uint64_t n3 = 77;
    EXPECT(bt_diag_bgzf(in.data(), in.size(), 1, small.data(), cap - 1, &n3, nullptr, nullptr) != BT_OK && n3 == 77);
    for (auto c : small) EXPECT(c == 0xAA);
    uint32_t crc = 0;
    EXPECT(bt_diag_crc32(in.data(), in.size(), &crc) == BT_OK && crc == (uint32_t)crc32(crc32(0L, Z_NULL, 0), in.data(), (uInt)in.size()));
    std::printf("%-8s in %8zu  out %8llu  blocks %2llu stored %2llu\n", name, in.size(), (unsigned long long)n1, (unsigned long long)st.pieces, (unsigned long long)st.stored_pieces);
}

static void check_crc_lengths() {
    const Bytes r = random_bytes(btbgzf::kBlock), z(btbgzf::kBlock, 0), f(btbgzf::kBlock, 0xFF);
    std::vector<size_t> lengths;
    for (size_t n = 0; n <= 80; ++n) lengths.push_back(n);
    for (size_t n = 1019; n <= 1025; ++n) lengths.push_back(n);
    lengths.push_back(btbgzf::kBlock - 1);
    lengths.push_back(btbgzf::kBlock);
    for (const Bytes *b : {&r, &z, &f})
        for (size_t n : lengths) {
            const Bytes exact(b->end() - n, b->end());   // its own allocation: a read before or behind it is reported
            uint32_t crc = 1;
            EXPECT(bt_diag_crc32(exact.data(), n, &crc) == BT_OK && crc == (uint32_t)crc32(crc32(0L, Z_NULL, 0), exact.data(), (uInt)n));
        }
}

static uint32_t get32(const std::string &s, size_t at) {
    uint32_t v;
    std::memcpy(&v, s.data() + at, 4);
    return v;
}

static void check_tabix() {
    using bthost::TabixLine;
    const std::vector<std::string> contigs = {"chrA", "chrEmpty", "chrB"};
    const std::vector<uint64_t> block_offsets = {0, 20000, 41000, 60000};   // three blocks and the EOF block
    std::vector<TabixLine> lines;
    uint64_t off = 300;
    for (uint64_t pos : {100ull, 16380ull, 16384ull, 121072ull, 140000ull, 400000ull}) {
        const uint64_t ref = pos == 121072 ? 20000 : pos == 16380 ? 10 : 2, len = 40 + ref;
        lines.push_back(TabixLine{0, pos, ref, off, len});
        off += len;
    }
    lines.push_back(TabixLine{0, 400100, 1, off, btbgzf::kBlock - off});   // ends where the first block ends
    off = btbgzf::kBlock;
    for (uint64_t pos : {5ull, 70000ull, 300000000ull, (1ull << 29) - 1}) {
        lines.push_back(TabixLine{2, pos, 1, off, 30000});
        off += 30000;
    }
    EXPECT(off <= 3 * (uint64_t)btbgzf::kBlock);
    std::string tbi, warning;
    EXPECT(bthost::buildTabixIndex(contigs, block_offsets, lines, tbi, warning) && warning.empty());
    EXPECT(tbi.size() > 36 + 20 && std::memcmp(tbi.data(), "TBI\1", 4) == 0 && get32(tbi, 4) == 3 && get32(tbi, 8) == 2 && get32(tbi, 12) == 1 && get32(tbi, 16) == 2 &&
           get32(tbi, 20) == 0 && get32(tbi, 24) == '#' && get32(tbi, 28) == 0 && get32(tbi, 32) == 19);
    EXPECT(std::memcmp(tbi.data() + tbi.size() - 8, "\0\0\0\0\0\0\0\0", 8) == 0);
    EXPECT(bthost::tabixReg2bin(16383, 16385) == 585 && bthost::tabixReg2bin(16384, 16385) == 4682 && bthost::tabixReg2bin(121071, 141071) == 73 &&
           bthost::tabixReg2bin((1u << 29) - 2, (1u << 29) - 1) == 4681 + 32767);
    lines.push_back(TabixLine{2, 1ull << 29, 1, off, 10});
    EXPECT(!bthost::buildTabixIndex(contigs, block_offsets, lines, tbi, warning) && tbi.empty() && warning.find("2^29") != std::string::npos);
    lines.back() = TabixLine{2, 10, 1, off, 10};
    EXPECT(!bthost::buildTabixIndex(contigs, block_offsets, lines, tbi, warning) && warning.find("not sorted") != std::string::npos);
    lines.back() = TabixLine{2, (1ull << 29) - 1, 1, 4 * (uint64_t)btbgzf::kBlock, 10};
    EXPECT(!bthost::buildTabixIndex(contigs, block_offsets, lines, tbi, warning) && warning.find("outside the blocks") != std::string::npos);
    EXPECT(bthost::buildTabixIndex({}, {0}, {}, tbi, warning) && tbi.size() == 36 + 8);
}

int main() {
    const size_t B = btbgzf::kBlock;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)3, (size_t)4, B - 1, B, B + 1, 2 * B, 2 * B + 1, 3 * B + 17}) {
        check("text", text(n));
        check("random", random_bytes(n));
        check("run", Bytes(n, 'G'));
    }
    check_crc_lengths();
    check_tabix();
    std::printf("%s\n", failures ? "FAILED" : "bgzf selfcheck ok");
    return failures ? 1 : 0;
}
