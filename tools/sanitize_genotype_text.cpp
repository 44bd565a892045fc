// Stand-alone host program for a sanitizer build (tools/sanitize_genotype_text.sh): the number formatter of bayestyper_amd/csrc/bt_genotype_text.hpp and
// bt_diag_genotype_text over a record string read from a file (tests/_genotype_text.py: make_string(2, hand_written(2))), over every truncation of it, over
// copies with one word overwritten, and with every capacity from 0 to the exact one.  It uses no GPU.  Exit status 0: every call returned what it should.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../bayestyper_amd/csrc/bt_genotype_text.hpp"
#include "../include/btgpu.h"

namespace bt {   // what bt_genotype_text.hip takes from bt_ctx.hip
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

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    // 1. the formatter against printf's %g, through the header directly and through the diagnostic entry
    std::vector<double> values = {0.0, -0.0, 1.0, -1.0, 0.5, 1e-27, 999999.5, 999999.4, 9.9999949e-5, 9.9999951e-5, 1e-4, 123456.5, 0.1234565, 2.0 / 3, 1e6, 1e7, 1e-28, 5e-324,
                                  std::numeric_limits<double>::infinity(), std::nan(""), std::nextafter(1e-27, 0.0), 29.99999951};
    for (int N : {1, 3, 7, 64, 250, 7000})
        for (int k = 0; k <= N; ++k) values.push_back((double)((float)k / (float)N));
    std::vector<char> text16(values.size() * 16);
    std::vector<int32_t> lens(values.size());
    EXPECT(bt_diag_format_g6(values.data(), values.size(), text16.data(), lens.data()) == BT_OK);
    for (size_t i = 0; i < values.size(); ++i) {
        char want[64];
        std::snprintf(want, sizeof want, "%g", values[i]);
        const double av = std::fabs(values[i]);
        const bool covered = values[i] == 0 || (std::isnormal(values[i]) && av >= 1e-27 && av < 1e6);
        EXPECT(covered == (lens[i] >= 0));
        if (lens[i] >= 0) EXPECT(std::string(text16.data() + 16 * i, (size_t)lens[i]) == want);
        unsigned char buf[24];
        for (unsigned shift = 0; shift < 4; ++shift) {   // every alignment of the store sink
            std::memset(buf, 0xAA, sizeof buf);
            btgtext::StoreSink o(buf + 4 + shift);
            const bool ok = btgtext::format_g6(o, values[i]);
            o.finish();
            EXPECT(ok == covered && (!ok || std::string((const char *)buf + 4 + shift, (size_t)o.count()) == want));
            for (unsigned j = 0; j < sizeof buf; ++j)
                if (j < 4 + shift || j >= 4 + shift + o.count()) EXPECT(buf[j] == 0xAA);
        }
    }
    // 2. the record string
    std::vector<uint32_t> words;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        uint32_t w;
        while (std::fread(&w, 4, 1, f) == 1) words.push_back(w);
        std::fclose(f);
    }
    uint64_t nt = 0, ni = 0;
    uint32_t nc = 0;
    EXPECT(bt_diag_genotype_text(words.data(), words.size(), nullptr, 0, nullptr, 0, &nt, &ni, &nc) != BT_OK && nt > 0 && ni > 0 && nc == 2);
    const uint64_t text_bytes = nt, index_words = ni;
    std::vector<uint8_t> ref_text(text_bytes);
    std::vector<uint32_t> ref_index(index_words);
    EXPECT(bt_diag_genotype_text(words.data(), words.size(), ref_text.data(), text_bytes, ref_index.data(), index_words, &nt, &ni, &nc) == BT_OK);
    for (uint64_t cap = 0; cap < text_bytes; cap += 7) {   // exactly sized heap buffers: a byte past a too-small capacity is the sanitizer's to report
        std::vector<uint8_t> t(cap);
        std::vector<uint32_t> ix(index_words);
        EXPECT(bt_diag_genotype_text(words.data(), words.size(), t.data(), cap, ix.data(), index_words, &nt, &ni, &nc) != BT_OK);
    }
    for (uint64_t n = 0; n < words.size(); ++n) {   // every truncation, in a buffer of exactly that length
        std::vector<uint32_t> part(words.begin(), words.begin() + n);
        std::vector<uint8_t> t(text_bytes);
        std::vector<uint32_t> ix(index_words);
        (void)bt_diag_genotype_text(part.data(), n, t.data(), text_bytes, ix.data(), index_words, &nt, &ni, &nc);
    }
    const uint32_t pokes[] = {0u, 1u, 2u, 3u, 40u, 0xFFFFu, 0x10000u, 0x7FFFFFFFu, 0xFFFFFFFFu};
    for (uint64_t at = 0; at < words.size(); ++at)   // one word overwritten: refused, or formatted inside the counted size
        for (uint32_t poke : pokes) {
            std::vector<uint32_t> bad(words);
            bad[at] = poke;
            uint64_t t_bytes = 0, i_words = 0;
            (void)bt_diag_genotype_text(bad.data(), bad.size(), nullptr, 0, nullptr, 0, &t_bytes, &i_words, &nc);
            if (t_bytes > (1u << 24) || i_words > (1u << 24)) continue;
            std::vector<uint8_t> t(t_bytes);
            std::vector<uint32_t> ix(i_words);
            (void)bt_diag_genotype_text(bad.data(), bad.size(), t.data(), t_bytes, ix.data(), i_words, &nt, &ni, &nc);
        }
    std::printf("sanitize_genotype_text: %zu values, %zu words, %llu text bytes, %d failure(s)\n", values.size(), words.size(), (unsigned long long)text_bytes, failures);
    return failures ? 1 : 0;
}
