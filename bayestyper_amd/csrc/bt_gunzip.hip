// libbtgpu: one long gzip member inflated on the device (bt_inflate_raw), the host run of the same code (bt_diag_inflate_raw) and the stream object over it
// (bt_fastq_gz_scan_*): an ordinary .fastq.gz -> reads text.  The algorithm, its verification argument and the rounds are bt_gunzip.hpp, one text for both.
// What zlib's inflate does under ReadsFile on one host thread per file.
//
// gunzip_find_kernel     a lane per bit offset behind the start's chunk: the 17-bit test, then plausible_header; the first hit of a chunk by atomic minimum
// gunzip_decode_kernel   a 64-thread workgroup = one wavefront per team (decode_team<WaveTeam>): 5.6 KiB of LDS for the decode tables.  No team waits on another.
// gunzip_windows_kernel  one workgroup of 1024 walks the chain with the window in LDS (32 KiB) and writes every team's window out
// gunzip_resolve_kernel  a thread per symbol: bytes to their place in the output, markers through the team's window
// gunzip_crc_kernel      a wavefront per 64 KiB of output (crc32_team); the pieces are joined on the host as zlib's crc32_combine does
// The kernels of a round follow each other on the stream; between rounds the host reads the teams' records (32 bytes each) and checks the links.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "bt_fastq_stream.hpp"
#include "bt_gunzip.hpp"
#include "bt_internal.hpp"

using namespace bt;
using namespace btgunzip;

namespace {

struct BlockTeam {   // the 1024 threads of the windows kernel's workgroup
    static constexpr uint32_t W = 1024;
    __device__ static uint32_t lane() { return threadIdx.x; }
    __device__ static void sync() { __syncthreads(); }
};

__global__ __launch_bounds__(256) void gunzip_find_kernel(const uint8_t *__restrict__ in, uint32_t n, uint32_t chunk, uint32_t first_chunk, uint32_t *__restrict__ cand) {
    const uint64_t at = (uint64_t)first_chunk * chunk * 8 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (uint64_t)n * 8) return;
    const uint32_t byte = (uint32_t)(at >> 3);
    // the cheap test first: BFINAL = 0, BTYPE = 2, HLIT and HDIST at most 29, from the 13 bits at the offset
    uint32_t w = 0;
    for (uint32_t k = 0; k < 3; ++k)
        if (byte + k < n) w |= (uint32_t)in[byte + k] << (8 * k);
    w >>= (uint32_t)at & 7u;
    if ((w & 7u) != 4u || ((w >> 3) & 31u) > 29u || ((w >> 8) & 31u) > 29u) return;
    if (plausible_header(in, n, (uint32_t)at)) atomicMin(&cand[byte / chunk], (uint32_t)at);
}

// workgroup 0 when first != 0: team 0, from p0 with the room and the known bytes of the arguments, at the symbol buffer's start; the others: the teams of the
// candidates starts[t], their records at recs[1 + t]
__global__ __launch_bounds__(64) void gunzip_decode_kernel(const uint8_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ starts, uint32_t n_starts, int first, uint32_t p0,
                                                           uint32_t limit0, uint32_t room, uint32_t known, uint64_t room0, uint16_t *syms, TeamRec *recs) {
    __shared__ Shared sh;
    uint32_t start = p0, limit = limit0;
    uint64_t at = 0;
    TeamRec *rec = recs;
    if (!first || blockIdx.x) {
        const uint32_t t = blockIdx.x - (first ? 1u : 0u);
        if (t >= n_starts) return;
        start = starts[t];
        limit = t + 1 < n_starts ? starts[t + 1] : kNone;
        const uint32_t byte = start >> 3, end_byte = t + 1 < n_starts ? limit >> 3 : n;
        if (byte >= n || end_byte > n || end_byte <= byte) return;   // (never: the starts ascend, a chunk apart, inside the input)
        at = room0 + (uint64_t)kExpand * byte;
        room = kExpand * (end_byte - byte);
        known = kWindow;
        rec = recs + 1 + t;
    }
    decode_team<WaveTeam>(sh, in, n, start, limit, syms + at, room, known, rec);
}

// windows [0]: the window in front of the chain -> windows [j + 1]: the window behind team j, which is team j + 1's
__global__ __launch_bounds__(1024) void gunzip_windows_kernel(const ChainEntry *__restrict__ chain, uint32_t n_teams, const uint16_t *__restrict__ syms, uint8_t *windows) {
    __shared__ uint8_t win[kWindow];
    for (uint32_t i = threadIdx.x; i < kWindow; i += 1024) win[i] = windows[i];
    __syncthreads();
    for (uint32_t j = 0; j < n_teams; ++j) window_step<BlockTeam>(win, syms + chain[j].sym_at, chain[j].n, windows + (uint64_t)(j + 1) * kWindow);
}

__global__ __launch_bounds__(256) void gunzip_resolve_kernel(const ChainEntry *__restrict__ chain, const uint16_t *__restrict__ syms, const uint8_t *__restrict__ windows,
                                                             uint8_t *__restrict__ out, uint64_t out_end) {
    const ChainEntry e = chain[blockIdx.x];
    const uint8_t *window = windows + (uint64_t)blockIdx.x * kWindow;
    const uint16_t *s = syms + e.sym_at;
    for (uint32_t k = blockIdx.y * 256 + threadIdx.x; k < e.n; k += gridDim.y * 256)
        if (e.out_at + k < out_end) out[e.out_at + k] = resolve_symbol(s[k], window);
}

__global__ __launch_bounds__(64) void gunzip_crc_kernel(const uint8_t *__restrict__ out, uint64_t bytes, uint32_t *__restrict__ crcs) {
    __shared__ btbgzf::CrcShared cs;
    const uint64_t at = (uint64_t)blockIdx.x * kCrcPiece;
    const uint32_t len = (uint32_t)std::min<uint64_t>(kCrcPiece, bytes - at);
    const uint32_t c = btbgzf::crc32_team<WaveTeam>(cs, out + at, len);
    if (threadIdx.x == 0) crcs[blockIdx.x] = c;
}

// Wall seconds per stage, summed over the calls of this process (bt_diag_gunzip_stage_seconds): find, decode, windows, resolve, crc.  Every stage ends with a
// synchronisation of its own except windows, which gets one only when BT_GUNZIP_STAGE_TIMES is set (the measurement of tools/gunzip_scan.py).
double g_stage_seconds[5] = {0, 0, 0, 0, 0};
struct StageClock {
    int stage;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit StageClock(int s) : stage(s) {}
    ~StageClock() { g_stage_seconds[stage] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
bool stage_times_wanted() {
    static const bool on = getenv("BT_GUNZIP_STAGE_TIMES") != nullptr;
    return on;
}

// The device's backend of inflate_rounds.  The buffers grow and stay: the stream object keeps one for its file.
struct DeviceBackend {
    bt_ctx *ctx = nullptr;
    const uint8_t *d_in = nullptr;
    uint32_t n = 0, chunk = 0;
    uint8_t *d_out = nullptr;
    uint64_t out_capacity = 0, room0 = 0;
    uint16_t *d_syms = nullptr;
    uint32_t *d_cand = nullptr, *d_starts = nullptr, *d_crcs = nullptr;
    TeamRec *d_recs = nullptr;
    ChainEntry *d_chain = nullptr;
    uint8_t *d_windows = nullptr;
    uint64_t cap_syms = 0, cap_cand = 0, cap_starts = 0, cap_crcs = 0, cap_recs = 0, cap_chain = 0, cap_windows = 0;
    uint32_t n_starts = 0;
    std::vector<uint32_t> h_crcs;

    template <class P>
    int reserve(P *&p, uint64_t &cap, uint64_t count) { return grow(reinterpret_cast<void **>(&p), &cap, count * sizeof(P)); }
    // the window slot 0 is kept from call to call; start_window: d_window [known] right-aligned into it (nullptr: left as it is)
    int begin(bt_ctx *c, const uint8_t *in, uint32_t n_, uint32_t chunk_, uint8_t *out, uint64_t capacity, const uint8_t *d_window, uint32_t known, bool keep_window) {
        ctx = c, d_in = in, n = n_, chunk = chunk_, d_out = out, out_capacity = capacity;
        room0 = std::min<uint64_t>(capacity, kMaxRun);
        n_starts = 0;
        if (!d_windows) {
            if (reserve(d_windows, cap_windows, 4 * (uint64_t)kWindow) != BT_OK) return BT_ERR;
            BT_HIP(hipMemsetAsync(d_windows, 0, kWindow, ctx->stream));
        }
        if (reserve(d_syms, cap_syms, symbol_count(n, room0) + 1) != BT_OK) return BT_ERR;
        if (!keep_window) {
            BT_HIP(hipMemsetAsync(d_windows, 0, kWindow, ctx->stream));
            if (known) BT_HIP(hipMemcpyAsync(d_windows + (kWindow - known), d_window, known, hipMemcpyDeviceToDevice, ctx->stream));
        }
        return BT_OK;
    }
    // the windows buffer for n_teams teams; slot 0 survives
    int reserve_windows(uint64_t n_teams) {
        const uint64_t need = (n_teams + 2) * kWindow;
        if (need <= cap_windows) return BT_OK;
        uint8_t *old = d_windows;
        d_windows = nullptr;
        cap_windows = 0;
        const int rc = reserve(d_windows, cap_windows, need);
        if (rc == BT_OK && hipMemcpyAsync(d_windows, old, kWindow, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) return fail("gunzip: window copy failed");
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(old);
        return rc;
    }
    int find(uint32_t first_chunk, std::vector<uint32_t> &cand) {
        StageClock clock(0);
        const uint32_t n_chunks = (uint32_t)(((uint64_t)n + chunk - 1) / chunk);
        cand.assign(n_chunks, kNone);
        if (reserve(d_cand, cap_cand, n_chunks) != BT_OK) return BT_ERR;
        BT_HIP(hipMemsetAsync(d_cand, 0xFF, (size_t)n_chunks * 4, ctx->stream));
        const uint64_t lanes = ((uint64_t)n - (uint64_t)first_chunk * chunk) * 8;
        hipLaunchKernelGGL(gunzip_find_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, d_in, n, chunk, first_chunk, d_cand);
        BT_CHECK_LAUNCH();
        BT_HIP(hipMemcpyAsync(cand.data(), d_cand, (size_t)n_chunks * 4, hipMemcpyDeviceToHost, ctx->stream));
        BT_HIP(hipStreamSynchronize(ctx->stream));
        return BT_OK;
    }
    int decode_all(const std::vector<uint32_t> &starts, std::vector<TeamRec> &recs, uint32_t p0, uint32_t limit, uint32_t room, uint32_t known, TeamRec *rec) {
        StageClock clock(1);
        n_starts = (uint32_t)starts.size();
        if (room > room0) return fail("gunzip: team 0's room exceeds the symbol buffer");
        if (reserve(d_starts, cap_starts, (uint64_t)n_starts + 1) != BT_OK || reserve(d_recs, cap_recs, (uint64_t)n_starts + 1) != BT_OK) return BT_ERR;
        if (n_starts) BT_HIP(hipMemcpyAsync(d_starts, starts.data(), (size_t)n_starts * 4, hipMemcpyHostToDevice, ctx->stream));
        BT_HIP(hipMemsetAsync(d_recs, 0, ((size_t)n_starts + 1) * sizeof(TeamRec), ctx->stream));
        hipLaunchKernelGGL(gunzip_decode_kernel, dim3(n_starts + 1), dim3(64), 0, ctx->stream, d_in, n, (const uint32_t *)d_starts, n_starts, 1, p0, limit, room, known, room0, d_syms, d_recs);
        BT_CHECK_LAUNCH();
        BT_HIP(hipMemcpyAsync(rec, d_recs, sizeof(TeamRec), hipMemcpyDeviceToHost, ctx->stream));
        if (n_starts) BT_HIP(hipMemcpyAsync(recs.data(), d_recs + 1, (size_t)n_starts * sizeof(TeamRec), hipMemcpyDeviceToHost, ctx->stream));
        BT_HIP(hipStreamSynchronize(ctx->stream));
        return BT_OK;
    }
    int decode_first(uint32_t p0, uint32_t limit, uint32_t room, uint32_t known, TeamRec *rec) {
        StageClock clock(1);
        if (reserve(d_recs, cap_recs, 1) != BT_OK) return BT_ERR;
        if (room > room0) return fail("gunzip: team 0's room exceeds the symbol buffer");
        hipLaunchKernelGGL(gunzip_decode_kernel, dim3(1), dim3(64), 0, ctx->stream, d_in, n, (const uint32_t *)d_starts, 0u, 1, p0, limit, room, known, room0, d_syms, d_recs);
        BT_CHECK_LAUNCH();
        BT_HIP(hipMemcpyAsync(rec, d_recs, sizeof(TeamRec), hipMemcpyDeviceToHost, ctx->stream));
        BT_HIP(hipStreamSynchronize(ctx->stream));
        return BT_OK;
    }
    int resolve(const std::vector<ChainEntry> &chain) {
        const uint32_t teams = (uint32_t)chain.size();
        if (reserve(d_chain, cap_chain, teams) != BT_OK || reserve_windows(teams) != BT_OK) return BT_ERR;
        BT_HIP(hipMemcpyAsync(d_chain, chain.data(), (size_t)teams * sizeof(ChainEntry), hipMemcpyHostToDevice, ctx->stream));
        {
            StageClock clock(2);
            hipLaunchKernelGGL(gunzip_windows_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const ChainEntry *)d_chain, teams, (const uint16_t *)d_syms, d_windows);
            BT_CHECK_LAUNCH();
            if (stage_times_wanted()) BT_HIP(hipStreamSynchronize(ctx->stream));
        }
        StageClock clock(3);
        hipLaunchKernelGGL(gunzip_resolve_kernel, dim3(teams, 16), dim3(256), 0, ctx->stream, (const ChainEntry *)d_chain, (const uint16_t *)d_syms, (const uint8_t *)d_windows, d_out,
                           out_capacity);
        BT_CHECK_LAUNCH();
        // the window behind the last team is the next round's, and the next call's
        BT_HIP(hipMemcpyAsync(d_windows, d_windows + (uint64_t)teams * kWindow, kWindow, hipMemcpyDeviceToDevice, ctx->stream));
        BT_HIP(hipStreamSynchronize(ctx->stream));   // (chain is the caller's vector)
        return BT_OK;
    }
    int crc(uint64_t bytes, uint32_t *crc_out) {
        StageClock clock(4);
        const uint64_t pieces = (bytes + kCrcPiece - 1) / kCrcPiece;
        uLong c = crc32(0L, Z_NULL, 0);
        if (pieces) {
            if (reserve(d_crcs, cap_crcs, pieces) != BT_OK) return BT_ERR;
            h_crcs.resize(pieces);
            hipLaunchKernelGGL(gunzip_crc_kernel, dim3((unsigned)pieces), dim3(64), 0, ctx->stream, (const uint8_t *)d_out, bytes, d_crcs);
            BT_CHECK_LAUNCH();
            BT_HIP(hipMemcpyAsync(h_crcs.data(), d_crcs, pieces * 4, hipMemcpyDeviceToHost, ctx->stream));
            BT_HIP(hipStreamSynchronize(ctx->stream));
            for (uint64_t i = 0; i < pieces; ++i) c = crc32_combine(c, h_crcs[i], (z_off_t)std::min<uint64_t>(kCrcPiece, bytes - i * kCrcPiece));
        }
        *crc_out = (uint32_t)c;
        return BT_OK;
    }
    void release() {
        if (!ctx) return;
        (void)hipStreamSynchronize(ctx->stream);
        for (void *p : {(void *)d_syms, (void *)d_cand, (void *)d_starts, (void *)d_crcs, (void *)d_recs, (void *)d_chain, (void *)d_windows})
            if (p) (void)hipFree(p);
        d_syms = nullptr, d_cand = d_starts = d_crcs = nullptr, d_recs = nullptr, d_chain = nullptr, d_windows = nullptr;
        cap_syms = cap_cand = cap_starts = cap_crcs = cap_recs = cap_chain = cap_windows = 0;
        ctx = nullptr;
    }
};

int check_raw_args(const char *who, uint64_t in_bytes, uint64_t start_bit, uint64_t window_bytes, uint32_t *chunk_bytes) {
    const std::string name(who);
    if (in_bytes > kMaxIn) return fail(name + ": at most " + std::to_string(kMaxIn) + " input bytes per call");
    if (start_bit > in_bytes * 8) return fail(name + ": start_bit lies behind the input");
    if (window_bytes > kWindow) return fail(name + ": a window holds at most 32768 bytes");
    if (*chunk_bytes == 0) *chunk_bytes = kDefaultChunk;
    if (*chunk_bytes < kMinChunk) return fail(name + ": chunk_bytes must be at least " + std::to_string(kMinChunk));
    return BT_OK;
}

void give_stats(const Stats &s, bt_gunzip_stats *out) {
    if (out) *out = bt_gunzip_stats{s.rounds, s.candidates, s.links_verified, s.links_broken, s.blocks, s.out_bytes};
}

}  // namespace

// ---- the stream object -------------------------------------------------------------------------------------------------------------------------------------
struct bt_fastq_gz_scan {
    BgzfStream st;                 // the buffers and the tail of the text half (bt_fastq_stream.hpp); no BGZF here
    FastqText *ft = nullptr;
    DeviceBackend be;
    uint32_t chunk = 0;
    enum State { kHeader, kDeflate, kTrailer } state = kHeader;
    std::vector<uint8_t> carry;    // the compressed bytes not consumed yet
    uint64_t carry_offset = 0;     // file offset of carry[0]
    uint32_t bit = 0;              // in kDeflate: the next block starts at this bit of carry[0]
    uint64_t member_offset = 0;    // file offset of the member under way
    uint32_t known = 0;            // bytes of the member's output in the window
    uLong crc = 0;
    uint64_t isize = 0;
    uint8_t *d_in = nullptr;
    uint64_t cap_in = 0;
    Stats total{0, 0, 0, 0, 0, 0};
};

namespace {

void drop_front(bt_fastq_gz_scan *s, uint64_t bytes) {
    s->carry.erase(s->carry.begin(), s->carry.begin() + (ptrdiff_t)bytes);
    s->carry_offset += bytes;
}

// d_raw keeps its first `used` bytes and gets room for `need`
int grow_raw(BgzfStream &st, uint64_t used, uint64_t need) {
    if (need <= st.cap_raw) return BT_OK;
    uint8_t *old = st.d_raw;
    st.d_raw = nullptr;
    st.cap_raw = 0;
    int rc = grow(reinterpret_cast<void **>(&st.d_raw), &st.cap_raw, need);
    if (rc == BT_OK && used && hipMemcpyAsync(st.d_raw, old, used, hipMemcpyDeviceToDevice, st.ctx->stream) != hipSuccess) rc = fail("bt_fastq_gz_scan_text: copy failed");
    (void)hipStreamSynchronize(st.ctx->stream);
    if (old) (void)hipFree(old);
    return rc;
}

// everything of the carried bytes that can be inflated now -> d_raw behind the tail; *raw = the tail and the new bytes
int gz_inflate(bt_fastq_gz_scan *s, uint64_t *raw) {
    const std::string who = "bt_fastq_gz_scan_text";
    BgzfStream &st = s->st;
    bt_ctx *ctx = st.ctx;
    uint64_t produced = 0;
    if (grow_raw(st, 0, st.tail + 65536) != BT_OK) return BT_ERR;
    if (st.tail) BT_HIP(hipMemcpyAsync(st.d_raw, st.d_tail, st.tail, hipMemcpyDeviceToDevice, ctx->stream));
    for (;;) {
        if (s->state == bt_fastq_gz_scan::kHeader) {
            if (s->carry.empty()) break;
            std::string what;
            const uint32_t at = gzip_header(s->carry.data(), s->carry.size(), &what);
            if (at == kNone) return fail(who + ": gzip member at offset " + std::to_string(s->carry_offset) + ": " + what);
            if (!at) {
                if (s->carry.size() > st.max_in_bytes) return fail(who + ": gzip member at offset " + std::to_string(s->carry_offset) + ": the header is not whole within max_in_bytes");
                break;
            }
            s->member_offset = s->carry_offset;
            drop_front(s, at);
            s->state = bt_fastq_gz_scan::kDeflate;
            s->bit = 0, s->known = 0, s->isize = 0;
            s->crc = crc32(0L, Z_NULL, 0);
        } else if (s->state == bt_fastq_gz_scan::kDeflate) {
            const uint64_t n = s->carry.size();
            if (!n) break;
            if (n > kMaxIn) return fail(who + ": more than " + std::to_string(kMaxIn) + " compressed bytes carried");
            if (grow(reinterpret_cast<void **>(&s->d_in), &s->cap_in, n + 16) != BT_OK) return BT_ERR;
            BT_HIP(hipMemcpyAsync(s->d_in, s->carry.data(), n, hipMemcpyHostToDevice, ctx->stream));
            BT_HIP(hipStreamSynchronize(ctx->stream));
            bool more_input = false;
            for (;;) {   // runs of at most run_cap bytes of output, until the carried bytes hold no further whole block
                const uint64_t run_cap = std::max<uint64_t>(8 * st.max_in_bytes, 1u << 20);
                uint64_t used = st.tail + produced;
                if (used + run_cap >= 0xFFFFFFFFull)
                    return fail(who + ": the bytes handed in at offset " + std::to_string(s->carry_offset) + " inflate to more than 4 GiB - 2 with the carried tail; hand in smaller slabs");
                if (st.cap_raw - used < run_cap && grow_raw(st, used, used + std::max<uint64_t>(run_cap, used)) != BT_OK) return BT_ERR;
                if (s->be.begin(ctx, s->d_in, (uint32_t)n, s->chunk, st.d_raw + used, run_cap, nullptr, 0, true) != BT_OK) return BT_ERR;
                RawResult r;
                if (inflate_rounds(s->be, RawJob{(uint32_t)n, s->bit, s->chunk, s->known, run_cap}, r) != BT_OK) return BT_ERR;
                const uint64_t block_at = s->carry_offset + (r.end_bit >> 3);
                if (r.status != kOk) return fail(who + ": gzip member at offset " + std::to_string(s->member_offset) + ": " + block_error(block_at, r.end_bit & 7u, r.status));
                produced += r.out_bytes;
                s->known = r.known;
                s->isize += r.out_bytes;
                s->crc = crc32_combine(s->crc, r.crc, (z_off_t)r.out_bytes);
                s->bit = r.end_bit;
                s->total.rounds += r.stats.rounds, s->total.candidates += r.stats.candidates, s->total.links_verified += r.stats.links_verified;
                s->total.links_broken += r.stats.links_broken, s->total.blocks += r.stats.blocks, s->total.out_bytes += r.stats.out_bytes;
                if (r.stream_end) break;
                if (r.stop == kStopRoom && r.out_bytes) continue;   // the run's room is used up: the next run goes on
                if (r.stop == kStopRoom)
                    return fail(who + ": gzip member at offset " + std::to_string(s->member_offset) + ": the deflate block at offset " + std::to_string(block_at) + " inflates to more than " +
                                std::to_string(run_cap) + " bytes (8 x max_in_bytes)");
                if (n - (r.end_bit >> 3) > st.max_in_bytes)
                    return fail(who + ": gzip member at offset " + std::to_string(s->member_offset) + ": the deflate block at offset " + std::to_string(block_at) +
                                " is not whole within max_in_bytes = " + std::to_string(st.max_in_bytes) + " of carried input");
                more_input = true;
                break;
            }
            if (more_input) {
                drop_front(s, s->bit >> 3);
                s->bit &= 7u;
                break;
            }
            drop_front(s, (s->bit + 7) >> 3);
            s->bit = 0;
            s->state = bt_fastq_gz_scan::kTrailer;
        } else {
            if (s->carry.size() < 8) break;
            const uint32_t want_crc = load32(s->carry.data()), want_isize = load32(s->carry.data() + 4);
            if (want_crc != (uint32_t)s->crc)
                return fail(who + ": gzip member at offset " + std::to_string(s->member_offset) + ": CRC-32 mismatch (trailer at offset " + std::to_string(s->carry_offset) + ")");
            if (want_isize != (uint32_t)(s->isize & 0xFFFFFFFFu))
                return fail(who + ": gzip member at offset " + std::to_string(s->member_offset) + ": output length differs from ISIZE (trailer at offset " + std::to_string(s->carry_offset) + ")");
            drop_front(s, 8);
            s->state = bt_fastq_gz_scan::kHeader;
        }
    }
    *raw = st.tail + produced;
    return BT_OK;
}

}  // namespace

extern "C" {

int bt_inflate_raw(bt_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes, uint64_t start_bit, const uint8_t *d_window, uint64_t window_bytes, uint32_t chunk_bytes, uint8_t *d_out,
                   uint64_t capacity, uint64_t *out_bytes, uint64_t *end_bit, int *stream_end, uint32_t *crc, bt_gunzip_stats *stats) {
    if (!ctx || (in_bytes && !d_in) || (window_bytes && !d_window) || (capacity && !d_out) || !out_bytes || !end_bit || !stream_end || !crc) return fail("bt_inflate_raw: null argument");
    if (check_raw_args("bt_inflate_raw", in_bytes, start_bit, window_bytes, &chunk_bytes) != BT_OK) return BT_ERR;
    BT_HIP(hipSetDevice(ctx->device));
    DeviceBackend be;
    RawResult r;
    int rc = be.begin(ctx, d_in, (uint32_t)in_bytes, chunk_bytes, d_out, capacity, d_window, (uint32_t)window_bytes, false);
    if (rc == BT_OK) rc = inflate_rounds(be, RawJob{(uint32_t)in_bytes, (uint32_t)start_bit, chunk_bytes, (uint32_t)window_bytes, capacity}, r) ? BT_ERR : BT_OK;
    be.release();
    if (rc != BT_OK) return rc;
    if (r.status != kOk) return fail("bt_inflate_raw: " + block_error(r.end_bit >> 3, r.end_bit & 7u, r.status));
    *out_bytes = r.out_bytes, *end_bit = r.end_bit, *stream_end = r.stream_end, *crc = r.crc;
    give_stats(r.stats, stats);
    return BT_OK;
}

int bt_diag_inflate_raw(const uint8_t *h_in, uint64_t in_bytes, uint64_t start_bit, const uint8_t *h_window, uint64_t window_bytes, uint32_t chunk_bytes, uint8_t *h_out, uint64_t capacity,
                        uint64_t *out_bytes, uint64_t *end_bit, int *stream_end, uint32_t *crc, bt_gunzip_stats *stats) {
    if ((in_bytes && !h_in) || (window_bytes && !h_window) || (capacity && !h_out) || !out_bytes || !end_bit || !stream_end || !crc) return fail("bt_diag_inflate_raw: null argument");
    if (check_raw_args("bt_diag_inflate_raw", in_bytes, start_bit, window_bytes, &chunk_bytes) != BT_OK) return BT_ERR;
    HostBackend be(h_in, (uint32_t)in_bytes, chunk_bytes, h_window, (uint32_t)window_bytes, h_out, capacity);
    RawResult r;
    if (inflate_rounds(be, RawJob{(uint32_t)in_bytes, (uint32_t)start_bit, chunk_bytes, (uint32_t)window_bytes, capacity}, r)) return BT_ERR;
    if (r.status != kOk) return fail("bt_diag_inflate_raw: " + block_error(r.end_bit >> 3, r.end_bit & 7u, r.status));
    *out_bytes = r.out_bytes, *end_bit = r.end_bit, *stream_end = r.stream_end, *crc = r.crc;
    give_stats(r.stats, stats);
    return BT_OK;
}

int bt_diag_gunzip_plausible(const uint8_t *h_in, uint64_t in_bytes, uint64_t first_bit, uint64_t n_bits, uint8_t *h_flags) {
    if ((in_bytes && !h_in) || (n_bits && !h_flags)) return fail("bt_diag_gunzip_plausible: null argument");
    if (in_bytes > kMaxIn) return fail("bt_diag_gunzip_plausible: at most " + std::to_string(kMaxIn) + " bytes of input");
    if (first_bit > 8 * in_bytes || n_bits > 8 * in_bytes - first_bit) return fail("bt_diag_gunzip_plausible: the bit offsets lie behind the input");
    for (uint64_t i = 0; i < n_bits; ++i) h_flags[i] = plausible_header(h_in, (uint32_t)in_bytes, (uint32_t)(first_bit + i)) ? 1 : 0;
    return BT_OK;
}

uint32_t bt_gunzip_default_chunk_bytes(void) { return kDefaultChunk; }
uint32_t bt_gunzip_expansion_budget(void) { return kExpand; }
void bt_diag_gunzip_stage_seconds(double *seconds5, int reset) {
    for (int i = 0; i < 5; ++i) {
        if (seconds5) seconds5[i] = g_stage_seconds[i];
        if (reset) g_stage_seconds[i] = 0;
    }
}

int bt_fastq_gz_scan_create(bt_ctx *ctx, uint64_t max_in_bytes, uint32_t chunk_bytes, bt_fastq_gz_scan **out) {
    if (!ctx || !out) return fail("bt_fastq_gz_scan_create: null argument");
    if (max_in_bytes < 65536 || max_in_bytes > (1ull << 26)) return fail("bt_fastq_gz_scan_create: max_in_bytes must lie in 64 KiB .. 64 MiB");
    if (chunk_bytes == 0) chunk_bytes = kDefaultChunk;
    if (chunk_bytes < kMinChunk) return fail("bt_fastq_gz_scan_create: chunk_bytes must be at least " + std::to_string(kMinChunk));
    BT_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<bt_fastq_gz_scan> s(new bt_fastq_gz_scan);
    s->st.ctx = ctx;
    s->st.max_in_bytes = max_in_bytes;
    s->chunk = chunk_bytes;
    s->ft = fastq_text_create();
    const int rc = s->be.begin(ctx, nullptr, 0, chunk_bytes, nullptr, 0, nullptr, 0, false);   // (the window slot)
    if (rc != BT_OK) {
        bt_fastq_gz_scan_destroy(s.release());
        return rc;
    }
    *out = s.release();
    return BT_OK;
}

int bt_fastq_gz_scan_text(bt_fastq_gz_scan *s, const uint8_t *h_bytes, uint64_t n_bytes, const char **d_text, uint64_t *text_len, bt_fastq_stats *stats) {
    const char *who = "bt_fastq_gz_scan_text";
    if (!s || (n_bytes && !h_bytes) || !d_text || !text_len) return fail("bt_fastq_gz_scan_text: null argument");
    *d_text = nullptr;
    *text_len = 0;
    if (stats) *stats = bt_fastq_stats{0, 0, 0};
    BgzfStream &st = s->st;
    if (n_bytes > st.max_in_bytes) return fail("bt_fastq_gz_scan_text: " + std::to_string(n_bytes) + " bytes handed in, the stream was created for " + std::to_string(st.max_in_bytes));
    BT_HIP(hipSetDevice(st.ctx->device));
    s->carry.insert(s->carry.end(), h_bytes, h_bytes + n_bytes);
    uint64_t raw = 0;
    if (gz_inflate(s, &raw) != BT_OK) return BT_ERR;
    if (grow(reinterpret_cast<void **>(&st.d_text), &st.cap_text, raw) != BT_OK) return BT_ERR;
    return fastq_text_slab(who, st, *s->ft, raw, d_text, text_len, stats);
}

int bt_fastq_gz_scan_finish(bt_fastq_gz_scan *s, const char **d_text, uint64_t *text_len, bt_fastq_stats *stats) {
    if (!s || !d_text || !text_len) return fail("bt_fastq_gz_scan_finish: null argument");
    *d_text = nullptr;
    *text_len = 0;
    if (stats) *stats = bt_fastq_stats{0, 0, 0};
    if (s->state != bt_fastq_gz_scan::kHeader || !s->carry.empty())
        return fail("bt_fastq_gz_scan_finish: truncated gzip file: it ends at offset " + std::to_string(s->carry_offset + s->carry.size()) + " inside the member at offset " +
                    std::to_string(s->state == bt_fastq_gz_scan::kHeader ? s->carry_offset : s->member_offset));
    BT_HIP(hipSetDevice(s->st.ctx->device));
    return fastq_text_finish("bt_fastq_gz_scan_finish", s->st, *s->ft, d_text, text_len, stats);
}

int bt_fastq_gz_scan_stats(const bt_fastq_gz_scan *s, bt_gunzip_stats *stats) {
    if (!s || !stats) return fail("bt_fastq_gz_scan_stats: null argument");
    give_stats(s->total, stats);
    return BT_OK;
}

void bt_fastq_gz_scan_destroy(bt_fastq_gz_scan *s) {
    if (!s) return;
    (void)hipSetDevice(s->st.ctx->device);
    s->be.ctx = s->st.ctx;
    s->be.release();
    if (s->d_in) (void)hipFree(s->d_in);
    if (s->ft) fastq_text_destroy(s->ft);
    s->st.release();
    delete s;
}

}  // extern "C"
