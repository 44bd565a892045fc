// Stand-alone host check of the packed reads' host code: pack, unpack and the packed front end (bayestyper_amd/csrc/bt_reads_pack.hpp, bt_reads_window.hpp) and the
// reads pack file's writer and reader (bayestyper_amd/csrc/bt_reads_pack_file.hpp), for a sanitizer build.  No GPU, no library.
//
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/reads_pack_host_check.cpp -lz -o reads_pack_host_check
//   ./reads_pack_host_check <scratch directory>
// The texts are those of the tests (tests/test_reads_pack_cpu.py): lengths 0 .. 257 and two host tiles, every byte value, lower and mixed case, runs of N, CRLF.
// Every input and output is an exactly sized heap block, so a load or store past it is an overflow the sanitizer sees.  Then the file: a round trip of 0, 1 and 5
// sections, and a reader on a truncated file, a flipped payload bit, a flipped header bit and a file without trailer.  Prints one line per stage; exit code 0
// when every comparison held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../bayestyper_amd/csrc/bt_reads_pack_file.hpp"
#include "../bayestyper_amd/csrc/bt_reads_window.hpp"

using namespace bt;

namespace {

int failures = 0;
void expect(bool ok, const std::string &what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what.c_str());
        failures++;
    }
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

std::string test_text(size_t n, unsigned flavour) {
    static const char alphabet[] = "ACGTacgtN\n";
    std::string s;
    if (flavour == 0)
        for (unsigned b = 0; b < 256; ++b) s.push_back((char)b);
    if (flavour == 1) s = "acgtACGTaCgTNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNACGT\r\nacgtn\r\n\r\n";
    while (s.size() < n) {
        if (flavour == 2 && rnd() % 150 == 0) s.push_back('\n');
        else s.push_back(flavour == 2 ? "ACGT"[rnd() & 3] : alphabet[rnd() % 10]);
    }
    s.resize(n);
    return s;
}

struct Window {
    uint64_t lo, hi, hash, end;
    bool operator==(const Window &o) const { return lo == o.lo && hi == o.hi && hash == o.hash && end == o.end; }
};

// pack into an exactly sized block, unpack into another, and run both front ends; returns the packed bytes
std::vector<uint32_t> check_text(const std::string &text, const unsigned *ks, size_t num_k) {
    const uint64_t n = text.size();
    const std::vector<char> exact(text.begin(), text.end());
    std::vector<uint32_t> packed((size_t)(reads_packed_bytes(n) / 4));
    reads_pack_host(exact.data(), n, packed.data());
    std::vector<char> back((size_t)n);
    reads_unpack_host(packed.data(), n, back.data());
    for (uint64_t i = 0; i < n; ++i) {
        const int code = nt_code(text[i]);
        expect(back[i] == (code < 0 ? '\n' : "ACGT"[code]), "unpack(pack) at " + std::to_string(i) + " of " + std::to_string(n));
    }
    // the padding of the last block is code 0, invalid; with garbage there the front end sees the same windows
    std::vector<uint32_t> dirty = packed;
    if (n % PACK_BLOCK_POSITIONS) {
        const uint64_t base = n / PACK_BLOCK_POSITIONS * PACK_BLOCK_WORDS;
        for (uint64_t j = n % PACK_BLOCK_POSITIONS; j < PACK_BLOCK_POSITIONS; ++j) {
            expect(((packed[base + j / 16] >> (2 * (j % 16))) & 3u) == 0 && ((packed[base + 8 + j / 32] >> (j % 32)) & 1u) == 0, "padding of a text of " + std::to_string(n));
            dirty[base + j / 16] |= 3u << (2 * (j % 16));
            dirty[base + 8 + j / 32] |= 1u << (j % 32);
        }
    }
    for (size_t q = 0; q < num_k; ++q) {
        const RollConst c = make_roll_const(ks[q]);
        std::vector<Window> want, got, got_dirty;
        auto into = [](std::vector<Window> &v) { return [&v](Kmer can, uint64_t h, uint64_t end) { v.push_back(Window{can.lo, can.hi, h, end}); }; };
        {
            HostTeam team;
            auto consume = into(want);
            reads_front_end(team, exact.data(), n, 0, c, consume);
        }
        {
            PackedHostTeam team;
            auto consume = into(got);
            reads_front_end_packed(team, packed.data(), n, 0, c, consume);
        }
        {
            PackedHostTeam team;
            auto consume = into(got_dirty);
            reads_front_end_packed(team, dirty.data(), n, 0, c, consume);
        }
        expect(want == got && want == got_dirty, "front ends at k " + std::to_string(ks[q]) + " over a text of " + std::to_string(n));
        // a later slab: only the windows that end at or behind first_end
        if (n > 300) {
            std::vector<Window> tail;
            PackedHostTeam team;
            auto consume = into(tail);
            reads_front_end_packed(team, packed.data(), n, n / 2, c, consume);
            size_t from = 0;
            while (from < want.size() && want[from].end < n / 2) from++;
            expect(std::vector<Window>(want.begin() + (long)from, want.end()) == tail, "first_end at k " + std::to_string(ks[q]));
        }
    }
    return packed;
}

std::string slurp(const std::string &path) {
    std::ifstream in(path, std::ios::binary);
    return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}
void spill(const std::string &path, const std::string &bytes) {
    std::ofstream out(path, std::ios::binary);
    out.write(bytes.data(), (std::streamsize)bytes.size());
}

// open + every section -> "" or the error
std::string read_all(const std::string &path, std::vector<std::vector<uint8_t>> *payloads = nullptr) {
    btpack::Reader r;
    if (!r.open(path.c_str())) return r.error;
    while (true) {
        std::vector<uint8_t> buf((size_t)btpack::packed_bytes(r.max_positions));   // exactly the largest section
        btpack::Section s;
        bool end = false;
        if (!r.next(buf.data(), buf.size(), &s, &end)) return r.error;
        if (end) break;
        buf.resize((size_t)btpack::packed_bytes(s.positions));
        if (payloads) payloads->push_back(buf);
    }
    return "";
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const unsigned ks[] = {1, 31, 32, 33, 55, 63, 64};
    const size_t lengths[] = {0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257, 4095, 4096, 4097, 2 * 4096 + 77};
    size_t texts = 0;
    for (size_t n : lengths)
        for (unsigned flavour = 0; flavour < 3; ++flavour) {
            check_text(test_text(n, flavour), ks, sizeof ks / sizeof *ks);
            texts++;
        }
    std::printf("pack, unpack and the packed front end: %zu texts at %zu k-mer sizes, %d failures\n", texts, sizeof ks / sizeof *ks, failures);

    const std::string manifest = "reads list_bytes:17 list_crc32:1a2b3c4d files:1 r.fq:117\nk:55\n";
    std::string five;
    for (size_t count : {(size_t)0, (size_t)1, (size_t)5}) {
        const std::string path = dir + "/check_" + std::to_string(count) + ".pack";
        std::vector<std::vector<uint32_t>> packed;
        std::vector<uint64_t> positions;
        std::remove(path.c_str());
        btpack::Writer w;
        expect(w.open(path.c_str(), 55, manifest), "writer open: " + w.error);
        for (size_t i = 0; i < count; ++i) {
            const std::string text = test_text(i == 2 ? 640 : 1 + rnd() % 3000, 2);
            packed.push_back(check_text(text, ks, 0));
            positions.push_back(text.size());
            expect(w.section(reinterpret_cast<const uint8_t *>(packed.back().data()), text.size(), text.size() / 2, i + 3), "writer section: " + w.error);
        }
        expect(slurp(path).empty(), "nothing under the final name before finish");
        expect(w.finish(), "writer finish: " + w.error);
        std::vector<std::vector<uint8_t>> payloads;
        const std::string err = read_all(path, &payloads);
        expect(err.empty(), "round trip of " + std::to_string(count) + " sections: " + err);
        expect(payloads.size() == count, "section count");
        for (size_t i = 0; i < payloads.size() && i < count; ++i)
            expect(payloads[i].size() == packed[i].size() * 4 && std::memcmp(payloads[i].data(), packed[i].data(), payloads[i].size()) == 0, "payload of section " + std::to_string(i));
        btpack::Reader r;
        expect(r.open(path.c_str()) && r.totals.sections == count && r.k == 55 && r.manifest == manifest, "header and trailer of " + std::to_string(count) + " sections");
        if (count == 5) five = slurp(path);
    }
    std::printf("file round trips of 0, 1 and 5 sections: %d failures\n", failures);

    const size_t header = btpack::FIXED_HEADER + manifest.size() + 4;
    struct Case {
        const char *name;
        std::string bytes;
        const char *words;
    };
    std::string payload_bit = five, header_bit = five;
    payload_bit[header + btpack::SECTION_HEAD + 7] ^= 0x08;
    header_bit[btpack::MAGIC_LEN + 5] ^= 0x01;
    const Case cases[] = {{"truncated", five.substr(0, header + 40), "truncated in section 0"},
                          {"payload_bit", payload_bit, "section 0 at offset"},
                          {"header_bit", header_bit, "header CRC mismatch"},
                          {"no_trailer", five.substr(0, five.size() - btpack::TRAILER_BYTES), "missing trailer"},
                          {"every_cut", "", ""}};
    for (const Case &c : cases) {
        const std::string path = dir + "/check_" + c.name + ".pack";
        if (std::string(c.name) == "every_cut") {   // a cut at every byte of the header and of the first section's head, and at every 97th byte behind: refused, never read past
            for (size_t cut = 0; cut < five.size(); cut += cut < header + 64 ? 1 : 97) {
                spill(path, five.substr(0, cut));
                expect(!read_all(path).empty(), "a file cut at " + std::to_string(cut) + " was accepted");
            }
            continue;
        }
        spill(path, c.bytes);
        const std::string err = read_all(path);
        expect(err.find(c.words) != std::string::npos, std::string(c.name) + ": \"" + err + "\"");
        std::printf("%s: %s\n", c.name, err.c_str());
    }
    std::printf("reads pack host check: %d failures\n", failures);
    return failures ? 1 : 0;
}
