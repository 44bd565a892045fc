// Stand-alone host check of the BAM route's host code: the BGZF reader and inflate (bayestyper_amd/csrc/bt_inflate.hpp) and the record code
// (bayestyper_amd/csrc/bt_bam.hpp) run by one thread, and the BAM file reader (bayestyper_amd/host/BamFile.cpp), for a sanitizer build.  No GPU, no library.
//
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/bam_host_check.cpp -x c++ bayestyper_amd/host/BamFile.cpp bayestyper_amd/host/BgzfFile.cpp -lz -o bam_host_check
//   ./bam_host_check <slab bytes> <file>...
// Per file: a BAM goes through BamFile's slabs, each inflated block by block behind the carried tail and turned into text, as bt_bam_scan_text does;
// any other file is taken as a run of BGZF blocks (sound or damaged) and inflated.  Errors are printed and are the expected end of a damaged file; the
// exit code is 0 unless a file cannot be opened.  What counts is that the sanitizers stay silent.
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../bayestyper_amd/csrc/bt_bam.hpp"
#include "../bayestyper_amd/csrc/bt_inflate.hpp"
#include "../bayestyper_amd/host/BamFile.hpp"

namespace {

struct Inflater {
    std::unique_ptr<btinflate::Shared> sh{new btinflate::Shared};
    std::unique_ptr<btbgzf::CrcShared> cs{new btbgzf::CrcShared};
    // whole blocks of in[0..n) appended to out (exactly sized: a write past a block's ISIZE is a heap overflow the sanitizer sees) -> bytes taken; the first
    // failing block's status in *status
    size_t run(const uint8_t *in, size_t n, std::vector<uint8_t> &out, uint32_t *status, size_t *bad_at) {
        size_t at = 0;
        *status = btinflate::kOk;
        while (n - at >= btbgzf::kFrame) {
            uint32_t bsize = 0;
            const uint32_t payload = btinflate::parse_header(in + at, n - at, &bsize);
            if (!payload) {
                *status = btinflate::kBadHeader, *bad_at = at;
                break;
            }
            const size_t size = (size_t)bsize + 1;
            if (size > n - at || size < payload + btbgzf::kTrailer) break;
            const uint32_t isize = btinflate::load32(in + at + size - 4);
            std::vector<uint8_t> data(isize <= btinflate::kMaxIsize ? isize : 0);
            const uint32_t st = btinflate::inflate_block<btinflate::LaneTeam>(*sh, *cs, in + at, (uint32_t)size, data.data(), isize);
            if (st != btinflate::kOk && *status == btinflate::kOk) *status = st, *bad_at = at;
            out.insert(out.end(), data.begin(), data.end());
            at += size;
        }
        return at;
    }
};

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <slab bytes> <file>...\n", argv[0]);
        return 2;
    }
    const size_t slab_bytes = (size_t)std::strtoull(argv[1], nullptr, 0);
    int unreadable = 0;
    Inflater inflater;
    for (int i = 2; i < argc; i++) {
        try {
            uint32_t status = 0;
            size_t bad_at = 0;
            if (bthost::BamFile::isBam(argv[i])) {
                bthost::BamFile file(argv[i], slab_bytes);
                std::vector<uint8_t> slab, raw;
                unsigned long long kept = 0, skipped = 0, bases = 0, slabs = 0, checksum = 0;
                size_t skip = file.skipFirstBytes();
                bool failed = false;
                while (!failed && file.next(slab)) {
                    inflater.run(slab.data(), slab.size(), raw, &status, &bad_at);
                    if (status != btinflate::kOk) {
                        std::printf("%s\terror: BGZF block at offset %llu: %s\n", argv[i], (unsigned long long)(file.slabOffset() + bad_at), btinflate::status_text(status));
                        failed = true;
                        break;
                    }
                    const size_t drop = skip < raw.size() ? skip : raw.size();
                    raw.erase(raw.begin(), raw.begin() + (long)drop);
                    skip -= drop;
                    std::vector<char> text(raw.size());
                    const btbam::HostText t = btbam::reads_text_host(raw.data(), raw.size(), bthost::bamSkipFlags(), text.data(), text.size());
                    if (t.err != btbam::kRecOk) {
                        std::printf("%s\terror: BAM record at offset %llu of the slab: %s\n", argv[i], (unsigned long long)t.err_offset, btbam::record_error_text(t.err));
                        failed = true;
                        break;
                    }
                    for (size_t j = 0; j < t.text_bytes; j++) checksum = checksum * 1099511628211ull + (unsigned char)text[j];
                    kept += t.kept, skipped += t.skipped, bases += t.bases, slabs++;
                    raw.erase(raw.begin(), raw.begin() + (long)t.consumed);
                }
                if (!failed)
                    std::printf("%s\tBAM\theader %llu\trefs %u\teof %d\tslabs %llu\tkept %llu\tskipped %llu\tbases %llu\tleft over %zu\ttext %016llx\n", argv[i],
                                (unsigned long long)file.headerBytes(), file.references(), (int)file.hasEofBlock(), slabs, kept, skipped, bases, raw.size() + skip, checksum);
            } else {
                std::ifstream in(argv[i], std::ios::binary);
                if (!in.is_open()) throw std::runtime_error("cannot open");
                const std::vector<char> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
                // an exactly sized copy: a load past the end of the input is a heap overflow the sanitizer sees
                const std::vector<uint8_t> exact(bytes.begin(), bytes.end());
                std::vector<uint8_t> raw;
                const size_t taken = inflater.run(exact.data(), exact.size(), raw, &status, &bad_at);
                if (status != btinflate::kOk)
                    std::printf("%s\terror: BGZF block at offset %zu: %s\n", argv[i], bad_at, btinflate::status_text(status));
                else {
                    std::vector<char> text(raw.size());   // records, when that is what the blocks hold: any bytes must be safe to walk
                    const btbam::HostText t = btbam::reads_text_host(raw.data(), raw.size(), 0, text.data(), text.size());
                    std::printf("%s\tBGZF\ttaken %zu of %zu\tdata %zu\tas records: kept %llu, error %u\n", argv[i], taken, exact.size(), raw.size(), (unsigned long long)t.kept, t.err);
                }
            }
        } catch (const std::exception &e) {
            std::printf("%s\terror: %s\n", argv[i], e.what());
            if (std::string(e.what()).find("cannot open") != std::string::npos) unreadable++;
        }
    }
    return unreadable ? 1 : 0;
}
