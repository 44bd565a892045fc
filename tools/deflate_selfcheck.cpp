// Stand-alone host program for a sanitizer build (tools/deflate_selfcheck.sh): bt_diag_deflate — the compressor of bayestyper_amd/csrc/bt_deflate.hpp run by a
// team of one thread — over the inputs of tests/test_deflate_cpu.py (built here again, in C++), every result inflated with zlib and compared with its input,
// every call made twice, the capacity rule at one byte short.  It uses no GPU.  Exit status 0: every call returned what it should.
#include <zlib.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../bayestyper_amd/csrc/bt_deflate.hpp"
#include "../include/btgpu.h"

namespace bt {   // what bt_deflate.hip takes from bt_ctx.hip
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
static void de_bruijn(int t, int p, int k, int n, std::vector<int> &a, Bytes &out) {
    if (t > n) {
        if (n % p == 0)
            for (int i = 1; i <= p; ++i) out.push_back((uint8_t)('a' + a[i]));
    } else {
        a[t] = a[t - p];
        de_bruijn(t + 1, p, k, n, a, out);
        for (int j = a[t - p] + 1; j < k; ++j) {
            a[t] = j;
            de_bruijn(t + 1, t, k, n, a, out);
        }
    }
}

static bool inflate_raw(const Bytes &in, size_t expect, Bytes &out) {
    z_stream zs;
    std::memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    out.assign(expect + 16, 0);
    zs.next_in = const_cast<Bytef *>(in.data());
    zs.avail_in = (uInt)in.size();
    zs.next_out = out.data();
    zs.avail_out = (uInt)out.size();
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.avail_in == 0;
    out.resize(out.size() - zs.avail_out);
    if (!ok) std::fprintf(stderr, "inflate: %d %s\n", rc, zs.msg ? zs.msg : "");
    inflateEnd(&zs);
    return ok;
}

static void check(const char *name, const Bytes &in) {
    uint64_t cap = 0, n1 = 0, n2 = 0;
    EXPECT(bt_deflate_bound(in.size(), &cap) == BT_OK);
    Bytes a(cap), b(cap), back;
    bt_deflate_stats s1, s2;
    EXPECT(bt_diag_deflate(in.data(), in.size(), 1, a.data(), cap, &n1, &s1) == BT_OK);
    EXPECT(bt_diag_deflate(in.data(), in.size(), 1, b.data(), cap, &n2, &s2) == BT_OK);
    EXPECT(n1 == n2 && n1 <= cap && std::memcmp(a.data(), b.data(), n1) == 0);
    a.resize(n1);
    EXPECT(inflate_raw(a, in.size(), back) && back == in);
    EXPECT(s1.bytes_in == in.size() && s1.bytes_out == n1 && s1.literals + s1.matched_bytes == in.size());
    Bytes small(cap ? cap - 1 : 0, 0xAA);
    uint64_t n3 = 77;
    EXPECT(bt_diag_deflate(in.data(), in.size(), 1, small.data(), cap - 1, &n3, nullptr) != BT_OK && n3 == 77);
    for (auto c : small) EXPECT(c == 0xAA);
    std::printf("%-28s in %8zu  out %8llu  pieces %3llu stored %3llu  literals %8llu matches %7llu\n", name, in.size(), (unsigned long long)n1, (unsigned long long)s1.pieces,
                (unsigned long long)s1.stored_pieces, (unsigned long long)s1.literals, (unsigned long long)s1.matches);
}

int main() {
    const size_t P = btdeflate::kPiece;
    for (size_t n : {0, 1, 2, 3}) check("tiny", text(n));
    for (size_t n : {P - 1, P, P + 1, 2 * P + 17}) check("text", text(n));
    check("70000 equal bytes", Bytes(70000, 'A'));
    {
        Bytes b;   // a match of every length 3 .. 258: a fresh random block, 64 random bytes (a round or more between source and copy), the block again
        for (size_t L = 3; L <= 258; ++L) {
            const Bytes blk = random_bytes(L), gap = random_bytes(64);
            b.insert(b.end(), blk.begin(), blk.end());
            b.insert(b.end(), gap.begin(), gap.end());
            b.insert(b.end(), blk.begin(), blk.end());
            b.push_back((uint8_t)rnd());
        }
        check("every match length", b);
    }
    {
        Bytes b(4 * 256);
        for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)(i < 512 ? i : 255 - i % 256);
        check("all byte values", b);
    }
    check("random", random_bytes(3 * P + 1000));
    for (size_t dist : {32769, 32768, 2 * 32769, 2 * 32768}) {   // the doubled ones: zeros between the blocks instead of random bytes
        const bool zeros = dist > 40000;
        if (zeros) dist /= 2;
        Bytes b = zeros ? Bytes(40000, 0) : random_bytes(40000);
        const Bytes blk = random_bytes(300);
        std::copy(blk.begin(), blk.end(), b.begin() + 100);
        std::copy(blk.begin(), blk.end(), b.begin() + 100 + dist);
        check(dist == 32768 ? "block at distance 32768" : "block at distance 32769", b);
    }
    {
        Bytes b;
        std::vector<int> a(16 * 3 + 1, 0);
        de_bruijn(1, 1, 16, 3, a, b);
        EXPECT(b.size() == 4096);
        check("de Bruijn B(16,3)", b);
    }
    {
        Bytes b = text(P), r = random_bytes(P), t = text(P - 5);
        b.insert(b.end(), r.begin(), r.end());
        b.insert(b.end(), t.begin(), t.end());
        check("text, random, text", b);
    }
    std::printf("%s\n", failures ? "FAILED" : "deflate selfcheck ok");
    return failures ? 1 : 0;
}
