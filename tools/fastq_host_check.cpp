// Stand-alone host check of the BGZF FASTQ route's host code: the FASTQ line code (bayestyper_amd/csrc/bt_fastq.hpp) and the BGZF inflate
// (bayestyper_amd/csrc/bt_inflate.hpp) run by one thread, and the file classes (bayestyper_amd/host/BgzfFile.cpp), for a sanitizer build.  No GPU, no library.
//
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/fastq_host_check.cpp -x c++ bayestyper_amd/host/BgzfFile.cpp -lz -o fastq_host_check
//   ./fastq_host_check <slab bytes> <file>...
// Per file: a BGZF FASTQ (isBgzfFastq) goes through BgzfFastqFile's slabs, each inflated block by block behind the carried tail and turned into text, the
// tail judged as the file's end, as bt_fastq_scan_text and _finish do; any other file is taken as FASTQ text (sound or damaged) and walked whole, as the file's
// end and as a piece of it, and at every cut of its first 300 bytes.  Inputs and outputs are exactly sized heap blocks: a load or store past them is an
// overflow the sanitizer sees.  Errors are printed and are the expected end of a damaged file; the exit code is 0 unless a file cannot be opened.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../bayestyper_amd/csrc/bt_fastq.hpp"
#include "../bayestyper_amd/csrc/bt_inflate.hpp"
#include "../bayestyper_amd/host/BgzfFile.hpp"

namespace {

// whole blocks of in[0..n) appended to out (each exactly sized) -> the first failing block's status and offset
uint32_t inflate_blocks(btinflate::Shared &sh, btbgzf::CrcShared &cs, const uint8_t *in, size_t n, std::vector<uint8_t> &out, size_t *bad_at) {
    size_t at = 0;
    while (n - at >= btbgzf::kFrame) {
        uint32_t bsize = 0;
        const uint32_t payload = btinflate::parse_header(in + at, n - at, &bsize);
        *bad_at = at;
        if (!payload) return btinflate::kBadHeader;
        const size_t size = (size_t)bsize + 1;
        if (size > n - at || size < payload + btbgzf::kTrailer) break;
        const uint32_t isize = btinflate::load32(in + at + size - 4);
        std::vector<uint8_t> data(isize <= btinflate::kMaxIsize ? isize : 0);
        const uint32_t st = btinflate::inflate_block<btinflate::LaneTeam>(sh, cs, in + at, (uint32_t)size, data.data(), isize);
        if (st != btinflate::kOk) return st;
        out.insert(out.end(), data.begin(), data.end());
        at += size;
    }
    return btinflate::kOk;
}

// the walk over an exactly sized copy of data[0..n), into a text buffer of exactly the size the text takes
btfastq::HostText walk(const uint8_t *data, size_t n, bool final, unsigned long long *checksum) {
    const std::vector<uint8_t> exact(data, data + n);
    std::vector<char> roomy(n);
    const btfastq::HostText first = btfastq::reads_text_host(exact.data(), n, final, roomy.data(), roomy.size());
    if (first.verdict != btfastq::kLineOk) return first;
    std::vector<char> text(first.text_bytes);
    const btfastq::HostText t = btfastq::reads_text_host(exact.data(), n, final, text.data(), text.size());
    if (t.too_small || t.text_bytes != first.text_bytes) std::abort();
    for (size_t j = 0; j < t.text_bytes; j++) *checksum = *checksum * 1099511628211ull + (unsigned char)text[j];
    if (first.text_bytes) {   // one byte less is refused, and nothing is written past it
        std::vector<char> tight(first.text_bytes - 1);
        if (!btfastq::reads_text_host(exact.data(), n, final, tight.data(), tight.size()).too_small) std::abort();
    }
    return t;
}

std::string message(const btfastq::HostText &t, unsigned long long first_line) {
    return btfastq::error_text(t.verdict, first_line + t.err_line, t.err_bases, t.err_quals, t.lines_of_four);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <slab bytes> <file>...\n", argv[0]);
        return 2;
    }
    const size_t slab_bytes = (size_t)std::strtoull(argv[1], nullptr, 0);
    int unreadable = 0;
    std::unique_ptr<btinflate::Shared> sh(new btinflate::Shared);
    std::unique_ptr<btbgzf::CrcShared> cs(new btbgzf::CrcShared);
    for (int i = 2; i < argc; i++) {
        try {
            unsigned long long reads = 0, bases = 0, line = 1, checksum = 0;
            if (bthost::isBgzfFastq(argv[i])) {
                bthost::BgzfFastqFile file(argv[i], slab_bytes);
                std::vector<uint8_t> slab, raw;
                unsigned long long slabs = 0;
                bool failed = false;
                while (!failed && file.next(slab)) {
                    size_t bad_at = 0;
                    const uint32_t status = inflate_blocks(*sh, *cs, slab.data(), slab.size(), raw, &bad_at);
                    if (status != btinflate::kOk) {
                        std::printf("%s\terror: BGZF block at offset %llu: %s\n", argv[i], (unsigned long long)(file.slabOffset() + bad_at), btinflate::status_text(status));
                        failed = true;
                        break;
                    }
                    const btfastq::HostText t = walk(raw.data(), raw.size(), false, &checksum);
                    if (t.verdict != btfastq::kLineOk) {
                        std::printf("%s\terror: %s\n", argv[i], message(t, line).c_str());
                        failed = true;
                        break;
                    }
                    reads += t.reads, bases += t.bases, line += t.lines, slabs++;
                    raw.erase(raw.begin(), raw.begin() + (long)t.consumed);
                }
                if (!failed) {
                    const btfastq::HostText t = walk(raw.data(), raw.size(), true, &checksum);
                    if (t.verdict != btfastq::kLineOk)
                        std::printf("%s\terror: %s\n", argv[i], message(t, line).c_str());
                    else
                        std::printf("%s\tBGZF FASTQ\teof %d\tslabs %llu\treads %llu\tbases %llu\tlines %llu\ttext %016llx\n", argv[i], (int)file.hasEofBlock(), slabs, reads + t.reads,
                                    bases + t.bases, line - 1 + t.lines, checksum);
                }
            } else {
                std::ifstream in(argv[i], std::ios::binary);
                if (!in.is_open()) throw std::runtime_error("cannot open");
                const std::vector<char> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
                const uint8_t *data = reinterpret_cast<const uint8_t *>(bytes.data());
                for (size_t cut = 0; cut < bytes.size() && cut < 300; cut++) (void)walk(data, cut, cut % 2 == 0, &checksum);
                const btfastq::HostText piece = walk(data, bytes.size(), false, &checksum), t = walk(data, bytes.size(), true, &checksum);
                if (t.verdict != btfastq::kLineOk)
                    std::printf("%s\terror: %s\t(as a piece: %s)\n", argv[i], message(t, 1).c_str(), piece.verdict == btfastq::kLineOk ? "sound" : message(piece, 1).c_str());
                else
                    std::printf("%s\ttext\treads %llu\tbases %llu\tlines %llu\tas a piece: consumed %llu of %zu\n", argv[i], (unsigned long long)t.reads, (unsigned long long)t.bases,
                                (unsigned long long)t.lines, (unsigned long long)piece.consumed, bytes.size());
            }
        } catch (const std::exception &e) {
            std::printf("%s\terror: %s\n", argv[i], e.what());
            if (std::string(e.what()).find("cannot open") != std::string::npos || std::string(e.what()).find("Unable to open") != std::string::npos) unreadable++;
        }
    }
    return unreadable ? 1 : 0;
}
