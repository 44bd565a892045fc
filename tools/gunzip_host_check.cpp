// Stand-alone host check of the parallel gunzip's code (bayestyper_amd/csrc/bt_gunzip.hpp: the header search, the teams' decoder with markers, the windows,
// the resolve and the rounds) run by one thread, for a sanitizer build.  No GPU, no library.
//
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/gunzip_host_check.cpp -lz -o gunzip_host_check
//   python tests/gunzip_data.py <directory>          (the corpus: sound streams and 200 single-bit flips of one)
//   ./gunzip_host_check <directory>/*.deflate
// Per file (a raw deflate stream, sound or damaged) and chunk size (1 KiB, 4 KiB, 16 KiB, 1 MiB): the stream is inflated from an exactly sized heap copy
// into an exactly sized output, so that a load or store past either is an overflow the sanitizer sees, and again in three calls with a third of the room
// each time.  zlib's inflate is the yardstick: where it ends the stream, the bytes, the end and the CRC-32 have to be its own; where it reports damage or
// runs out of input, the result here is an error or a stop short of the stream's end.  The four chunk sizes have to agree in everything.
// One line per file: "<file> ok <bytes> <crc32> <stream_end>" or "<file> error <message>": what the tests compare the library's results with.
// The exit code is 0 unless a file cannot be opened or a comparison fails.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../bayestyper_amd/csrc/bt_gunzip.hpp"

namespace {

using namespace btgunzip;

struct Outcome {
    bool error = false;
    std::string message;
    std::vector<uint8_t> data;
    uint32_t end_bit = 0, crc = 0;
    int stream_end = 0;
    Stats stats{0, 0, 0, 0, 0, 0};
};

// one call: in[0..n) from start_bit with the window, into exactly `capacity` bytes
Outcome run(const std::vector<uint8_t> &in, uint32_t start_bit, const std::vector<uint8_t> &window, uint32_t chunk, uint64_t capacity) {
    std::vector<uint8_t> out(capacity);
    HostBackend be(in.data(), (uint32_t)in.size(), chunk, window.data(), (uint32_t)window.size(), out.data(), capacity);
    RawResult r;
    Outcome o;
    if (inflate_rounds(be, RawJob{(uint32_t)in.size(), start_bit, chunk, (uint32_t)window.size(), capacity}, r)) std::abort();
    if (r.status != kOk) {
        o.error = true;
        o.message = block_error(r.end_bit >> 3, r.end_bit & 7u, r.status);
        return o;
    }
    if (r.out_bytes > capacity) std::abort();
    o.data.assign(out.begin(), out.begin() + (ptrdiff_t)r.out_bytes);
    o.end_bit = r.end_bit, o.crc = r.crc, o.stream_end = r.stream_end, o.stats = r.stats;
    return o;
}

// zlib's answer: the bytes, whether the stream ended, and where
bool zlib_inflate(const std::vector<uint8_t> &in, std::vector<uint8_t> &out, size_t *used) {
    z_stream z{};
    if (inflateInit2(&z, -15) != Z_OK) std::abort();
    out.resize(1 << 16);
    z.next_in = const_cast<Bytef *>(in.data());
    z.avail_in = (uInt)in.size();
    int rc = Z_OK;
    for (;;) {
        if (z.total_out == out.size()) out.resize(out.size() * 2);
        z.next_out = out.data() + z.total_out;
        z.avail_out = (uInt)(out.size() - z.total_out);
        rc = inflate(&z, Z_NO_FLUSH);
        if (rc != Z_OK) break;
    }
    out.resize(z.total_out);
    *used = z.total_in;
    inflateEnd(&z);
    return rc == Z_STREAM_END;
}

}  // namespace

int main(int argc, char **argv) {
    int failures = 0;
    for (int i = 1; i < argc; ++i) {
        std::ifstream f(argv[i], std::ios::binary);
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[i]);
            return 2;
        }
        const std::vector<uint8_t> in((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        std::vector<uint8_t> want;
        size_t used = 0;
        const bool sound = zlib_inflate(in, want, &used);
        const uint64_t room = want.size() + 70000;   // (a damaged stream may hold a block more than zlib got through)
        Outcome shown;
        for (uint32_t chunk : {1024u, 4096u, 16384u, 1048576u}) {
            const Outcome o = run(in, 0, {}, chunk, sound ? want.size() : room);
            if (sound) {
                const bool same = !o.error && o.stream_end && o.data == want && (o.end_bit + 7) / 8 == used && o.crc == (uint32_t)crc32(crc32(0L, Z_NULL, 0), want.data(), (uInt)want.size());
                if (!same) {
                    std::printf("%s MISMATCH at chunk %u: %s\n", argv[i], chunk, o.error ? o.message.c_str() : "bytes, end or CRC-32 differ from zlib's");
                    ++failures;
                }
                // again in calls with a third of the room: from end_bit with the last 32 KiB as the window
                std::vector<uint8_t> all, window;
                uint32_t at = 0;
                int ended = 0;
                for (int calls = 0; calls < 64 && !ended; ++calls) {
                    const Outcome p = run(in, at, window, chunk, want.size() / 3 + 1);
                    if (p.error || (!p.stream_end && p.data.empty())) break;
                    all.insert(all.end(), p.data.begin(), p.data.end());
                    window.assign(all.end() - (ptrdiff_t)std::min<size_t>(all.size(), kWindow), all.end());
                    at = p.end_bit;
                    ended = p.stream_end;
                }
                // (a block larger than a third of the output cannot be resumed into: then the pieces stop short, which is a result)
                if (ended ? all != want : all.size() > want.size() || !std::equal(all.begin(), all.end(), want.begin())) {
                    std::printf("%s MISMATCH at chunk %u: resumed calls differ from zlib's bytes\n", argv[i], chunk);
                    ++failures;
                }
            } else if (!o.error && o.stream_end) {   // zlib saw damage (or no end) where this decoder saw a stream's end: the two disagree about the format
                std::printf("%s MISMATCH at chunk %u: zlib reports damage, this decoder a stream's end\n", argv[i], chunk);
                ++failures;
            }
            if (chunk == 1024u) shown = o;
            else if (o.error != shown.error || o.message != shown.message || o.data != shown.data || o.end_bit != shown.end_bit || o.crc != shown.crc) {
                std::printf("%s MISMATCH: chunk %u and chunk 1024 differ\n", argv[i], chunk);
                ++failures;
            }
        }
        if (shown.error) std::printf("%s error %s\n", argv[i], shown.message.c_str());
        else std::printf("%s ok %zu %08x %d\n", argv[i], shown.data.size(), shown.crc, shown.stream_end);
    }
    return failures ? 1 : 0;
}
