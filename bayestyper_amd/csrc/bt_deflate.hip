// libbtgpu: deflate on the device (bt_deflate), gzip files written through it (bt_gzip_save) and the host run of the same code (bt_diag_deflate).
// The compressor is bt_deflate.hpp, one text for both.  Replaces the host-side gzip streams of GenotypeWriter.cpp (the VCF) and main.cpp (the parameter
// k-mer FASTA, the intercluster regions) of the reference.
//
// deflate_piece_kernel: one 64-thread workgroup = one wavefront per 64 KiB piece, so the team's barrier is a wave barrier.  Its LDS is btdeflate::Shared,
//   21.6 KiB, of which the head table is 16 KiB: seven pieces would fit the 160 KiB of a CU, but what is resident is set by the grid — a batch of
//   kBatch = 1024 pieces is 4 per CU, a 32 MiB slab 2 per CU — so the LDS is not the limit.  The kernel waits on memory (the table in LDS, the
//   candidate's bytes in global memory) most of the time.  A larger table buys nothing: on the VCF text of
//   tests/_deflate_inputs.py tables of 2^11, 2^12, 2^13, 2^14 words give 0.4028, 0.4035, 0.4029, 0.4025 of the input (a 3-byte hash: 0.44).
//   Tokens go to a per-piece area of 64 Ki words, the piece's bytes to a staging slot of kPieceOut bytes.
// deflate_compact_kernel: one workgroup per piece sums the sizes of the batch's pieces before its own (an exclusive scan done by each workgroup for
//   itself: no workgroup waits for another) and copies its slot to its place; the workgroup of the batch's last piece leaves the running total for the
//   next batch.  A call runs batches of at most kBatch pieces so that the token areas stay at 256 MiB.
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "bt_deflate.hpp"
#include "bt_gz_staging.hpp"
#include "bt_internal.hpp"

using bt::fail;
using namespace btdeflate;
using btgz::GzStaging;
using btgz::since;
using btgz::TmpFile;

namespace {

constexpr uint32_t kBatch = 1024;   // pieces per launch
constexpr unsigned COPY_BLOCK = 256;

__global__ __launch_bounds__(64) void deflate_piece_kernel(const uint8_t *__restrict__ in, uint64_t n, uint64_t first_piece, uint64_t total_pieces, int last,
                                                           uint32_t *__restrict__ tokens, uint8_t *__restrict__ stage, uint32_t *__restrict__ recs, uint32_t *error) {
    __shared__ Shared sh;
    const uint64_t piece = first_piece + blockIdx.x, off = piece * kPiece;
    const uint32_t len = off >= n ? 0u : (uint32_t)std::min<uint64_t>(kPiece, n - off);
    deflate_piece<WaveTeam>(sh, in + off, len, last && piece + 1 == total_pieces, tokens + (uint64_t)blockIdx.x * kPiece, stage + (uint64_t)blockIdx.x * kPieceOut,
                            recs + piece * kRecWords, error);
}

// bases[batch]: where the batch's first piece goes; bases[batch + 1] is written for the next batch
__global__ __launch_bounds__(COPY_BLOCK) void deflate_compact_kernel(const uint8_t *__restrict__ stage, const uint32_t *__restrict__ recs, uint64_t first_piece, uint32_t batch_pieces,
                                                                     unsigned long long *bases, uint32_t batch, uint8_t *__restrict__ out, uint64_t capacity, uint32_t *error) {
    __shared__ unsigned long long part[COPY_BLOCK];
    const uint32_t b = blockIdx.x;
    unsigned long long s = 0;
    for (uint32_t j = threadIdx.x; j < b; j += COPY_BLOCK) s += recs[(first_piece + j) * kRecWords];
    part[threadIdx.x] = s;
    __syncthreads();
    for (unsigned w = COPY_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    const uint32_t size = recs[(first_piece + b) * kRecWords];
    const unsigned long long at = bases[batch] + part[0];
    if (size > kPieceOut || at + size > capacity) {   // never with a capacity of bt_deflate_bound: the guard that nothing is written past it
        if (threadIdx.x == 0) atomicOr(error, (uint32_t)kErrCapacity);
        return;
    }
    if (b + 1 == batch_pieces && threadIdx.x == 0) bases[batch + 1] = at + size;
    const uint8_t *src = stage + (uint64_t)b * kPieceOut;
    uint8_t *dst = out + at;
    // bytes up to the destination's first whole dword, whole dwords (the source is read at any alignment), the rest
    const uint32_t head = std::min<uint32_t>(size, (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3)), words = (size - head) / 4, tail = head + words * 4;
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    for (uint32_t w = threadIdx.x; w < words; w += COPY_BLOCK) *reinterpret_cast<uint32_t *>(dst + head + 4 * w) = load32(src + head + 4 * w);
    if (threadIdx.x < size - tail) dst[tail + threadIdx.x] = src[tail + threadIdx.x];
}

// the scratch of a call (or of all slabs of a bt_gzip_save): token areas and staging slots of one batch, the pieces' records, the batches' bases
struct Work {
    uint32_t *d_tokens = nullptr, *d_recs = nullptr, *d_error = nullptr;
    uint8_t *d_stage = nullptr;
    unsigned long long *d_bases = nullptr;
    uint64_t cap_pieces = 0, batches = 0;
    hipError_t alloc(uint64_t pieces) {
        cap_pieces = pieces;
        batches = (pieces + kBatch - 1) / kBatch;
        const uint64_t bp = std::min<uint64_t>(pieces, kBatch);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_tokens), bp * kPiece * 4);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_stage), bp * kPieceOut);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_recs), pieces * kRecWords * 4);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_bases), (batches + 1) * 8);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_error), 4);
        return e;
    }
    ~Work() {
        (void)hipFree(d_tokens);
        (void)hipFree(d_stage);
        (void)hipFree(d_recs);
        (void)hipFree(d_bases);
        (void)hipFree(d_error);
    }
};

// the kernels of one stream of n bytes, enqueued on st; the pieces' records, the total and the error word stay on the device
hipError_t enqueue(Work &w, hipStream_t st, const uint8_t *d_in, uint64_t n, int last, uint8_t *d_out, uint64_t capacity) {
    const uint64_t pieces = num_pieces(n);
    hipError_t e = hipMemsetAsync(w.d_bases, 0, 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(w.d_error, 0, 4, st);
    for (uint64_t first = 0, batch = 0; first < pieces && e == hipSuccess; first += kBatch, ++batch) {
        const uint32_t bp = (uint32_t)std::min<uint64_t>(kBatch, pieces - first);
        hipLaunchKernelGGL(deflate_piece_kernel, dim3(bp), dim3(64), 0, st, d_in, n, first, pieces, last, w.d_tokens, w.d_stage, w.d_recs, w.d_error);
        hipLaunchKernelGGL(deflate_compact_kernel, dim3(bp), dim3(COPY_BLOCK), 0, st, (const uint8_t *)w.d_stage, (const uint32_t *)w.d_recs, first, bp, w.d_bases, (uint32_t)batch, d_out,
                           capacity, w.d_error);
        e = hipGetLastError();
    }
    return e;
}

void add_records(const uint32_t *recs, uint64_t pieces, uint64_t n, bt_deflate_stats *stats) {
    if (!stats) return;
    stats->pieces += pieces;
    stats->bytes_in += n;
    for (uint64_t i = 0; i < pieces; ++i) {
        const uint32_t *r = recs + i * kRecWords;
        stats->bytes_out += r[0];
        stats->stored_pieces += r[1];
        stats->literals += r[2];
        stats->matches += r[3];
        stats->matched_bytes += r[4];
    }
}

int error_word(const char *who, uint32_t err) {
    if (!err) return BT_OK;
    std::string what;
    if (err & kErrKraft) what += " a code's lengths could not be limited;";
    if (err & kErrBlockEnd) what += " a block did not end where its size was computed;";
    if (err & kErrTokens) what += " a piece's tokens do not add up to its length;";
    if (err & kErrCapacity) what += " the output buffer is too small;";
    return fail(std::string(who) + ":" + what + " (error word " + std::to_string(err) + ")");
}

uint64_t slab_bytes() {
    uint64_t slab = 32ull << 20;
    if (const char *e = getenv("BT_GZIP_SLAB_BYTES")) {
        const uint64_t v = strtoull(e, nullptr, 10);
        if (v >= 1 && v <= (1ull << 30)) slab = v;
    }
    return (slab + kPiece - 1) / kPiece * kPiece;
}

// CRC-32 of p[0..n) on `threads` threads: per-part crc32, then crc32_combine in order (writeGzFile's pattern)
uint32_t crc_parallel(const uint8_t *p, uint64_t n, unsigned threads) {
    const uint64_t part = 4ull << 20, parts = (n + part - 1) / part;
    if (parts <= 1 || threads <= 1) {
        uLong c = crc32(0L, Z_NULL, 0);
        for (uint64_t at = 0; at < n; at += 1u << 30) c = crc32(c, p + at, (uInt)std::min<uint64_t>(1u << 30, n - at));
        return (uint32_t)c;
    }
    std::vector<uLong> crcs(parts);
    const unsigned nt = (unsigned)std::min<uint64_t>(threads, parts);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&, t] {
            for (uint64_t i = t; i < parts; i += nt) crcs[i] = crc32(crc32(0L, Z_NULL, 0), p + i * part, (uInt)std::min<uint64_t>(part, n - i * part));
        });
    for (auto &th : pool) th.join();
    uLong c = crc32(0L, Z_NULL, 0);
    for (uint64_t i = 0; i < parts; ++i) c = crc32_combine(c, crcs[i], (z_off_t)std::min<uint64_t>(part, n - i * part));
    return (uint32_t)c;
}

}  // namespace

extern "C" {

int bt_deflate_bound(uint64_t n, uint64_t *capacity) {
    if (!capacity) return fail("bt_deflate_bound: null argument");
    *capacity = stream_bound(n);
    return BT_OK;
}

int bt_deflate(bt_ctx *ctx, const uint8_t *d_in, uint64_t n, int last, uint8_t *d_out, uint64_t capacity, uint64_t *h_out_bytes, bt_deflate_stats *stats) {
    if (!ctx || (n && !d_in) || !d_out || !h_out_bytes) return fail("bt_deflate: null argument");
    if (capacity < stream_bound(n)) return fail("bt_deflate: buffer too small (" + std::to_string(capacity) + " bytes, bt_deflate_bound gives " + std::to_string(stream_bound(n)) + ")");
    BT_HIP(hipSetDevice(ctx->device));
    const uint64_t pieces = num_pieces(n);
    Work w;
    hipError_t e = w.alloc(pieces);
    if (e != hipSuccess) return fail(std::string("bt_deflate: scratch buffers: ") + hipGetErrorString(e));
    BT_HIP(enqueue(w, ctx->stream, d_in, n, last, d_out, capacity));
    std::vector<uint32_t> recs(pieces * kRecWords);
    unsigned long long total = 0;
    uint32_t err = 0;
    BT_HIP(hipMemcpyAsync(recs.data(), w.d_recs, recs.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipMemcpyAsync(&total, w.d_bases + w.batches, 8, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipMemcpyAsync(&err, w.d_error, 4, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipStreamSynchronize(ctx->stream));
    if (error_word("bt_deflate", err) != BT_OK) return BT_ERR;
    *h_out_bytes = total;
    if (stats) {
        *stats = bt_deflate_stats{};
        add_records(recs.data(), pieces, n, stats);
        if (stats->bytes_out != total) return fail("bt_deflate: the pieces' sizes do not add up to the stream's length");
    }
    return BT_OK;
}

int bt_gzip_save(bt_ctx *ctx, const char *path, const uint8_t *h_data, uint64_t n, uint32_t threads, bt_deflate_stats *stats) {
    if (!ctx || !path || (n && !h_data)) return fail("bt_gzip_save: null argument");
    BT_HIP(hipSetDevice(ctx->device));
    const uint64_t slab = std::min<uint64_t>(slab_bytes(), (n + kPiece - 1) / kPiece * kPiece), slabs = n ? (n + slab - 1) / slab : 1;
    const uint64_t bound = stream_bound(slab), slab_pieces = num_pieces(slab);
    hipStream_t st = ctx->stream;
    GzStaging g;
    Work w;
    hipError_t e = g.alloc(st, slab, bound, slab_pieces * kRecWords * 4, slabs > 1 ? 2 : 1);
    if (e == hipSuccess) e = w.alloc(slab_pieces);
    if (e != hipSuccess) return fail(std::string("bt_gzip_save: staging buffers: ") + hipGetErrorString(e));
    TmpFile file;
    if (!file.open(path)) return fail(std::string("bt_gzip_save: cannot create ") + path + ".tmp");
    const unsigned char header[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};   // deflate, no flags, no time stamp, unix (writeGzFile's)
    if (!file.write(header, 10)) return fail(std::string("bt_gzip_save: write to ") + path + ".tmp failed (disk full?)");
    bt_deflate_stats s{};
    uLong crc = crc32(0L, Z_NULL, 0);
    auto len_of = [&](uint64_t i) { return n ? std::min(slab, n - i * slab) : 0; };
    // slab i: staged, copied in, compressed (all enqueued at once); then slab i - 1's copy out is enqueued on a stream of its own, slab i's CRC-32 is
    // computed while the device works, and slab i - 1 is written
    for (uint64_t i = 0; i <= slabs; ++i) {
        const int b = (int)(i & 1), p = b ^ 1;
        if (i < slabs) {
            const uint64_t len = len_of(i);
            const auto t0 = std::chrono::steady_clock::now();
            if (len) std::memcpy(g.pin_in[b], h_data + i * slab, len);
            s.seconds_host += since(t0);
            e = hipEventRecord(g.ev[b][0], st);
            if (e == hipSuccess && len) e = hipMemcpyAsync(g.d_in[b], g.pin_in[b], len, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipEventRecord(g.ev[b][1], st);
            if (e == hipSuccess) e = enqueue(w, st, g.d_in[b], len, i + 1 == slabs, g.d_out[b], bound);
            if (e == hipSuccess) e = hipEventRecord(g.ev[b][2], st);
            if (e == hipSuccess) e = hipMemcpyAsync(g.pin_recs[b], w.d_recs, num_pieces(len) * kRecWords * 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(g.pin_total[b], w.d_bases + (num_pieces(len) + kBatch - 1) / kBatch, 8, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(g.pin_total[b] + 1, w.d_error, 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipEventRecord(g.ev[b][3], st);
            if (e != hipSuccess) return fail(std::string("bt_gzip_save: ") + hipGetErrorString(e));
        }
        uint64_t out_prev = 0;
        if (i > 0) {   // slab i - 1 is compressed: its length is known, its bytes start their way out
            e = hipEventSynchronize(g.ev[p][3]);
            if (e != hipSuccess) return fail(std::string("bt_gzip_save: ") + hipGetErrorString(e));
            if (error_word("bt_gzip_save", (uint32_t)g.pin_total[p][1]) != BT_OK) return BT_ERR;
            out_prev = g.pin_total[p][0];
            if (out_prev > bound) return fail("bt_gzip_save: a slab's stream is longer than its bound");
            add_records(g.pin_recs[p], num_pieces(len_of(i - 1)), len_of(i - 1), &s);
            e = hipEventRecord(g.ev[p][4], g.copy_out);
            if (e == hipSuccess) e = hipMemcpyAsync(g.pin_out[p], g.d_out[p], out_prev, hipMemcpyDeviceToHost, g.copy_out);
            if (e == hipSuccess) e = hipEventRecord(g.ev[p][5], g.copy_out);
            if (e != hipSuccess) return fail(std::string("bt_gzip_save: ") + hipGetErrorString(e));
        }
        if (i < slabs && len_of(i)) {
            const auto t0 = std::chrono::steady_clock::now();
            crc = crc32_combine(crc, crc_parallel(h_data + i * slab, len_of(i), std::max(1u, threads)), (z_off_t)len_of(i));
            s.seconds_host += since(t0);
        }
        if (i > 0) {
            e = hipEventSynchronize(g.ev[p][5]);
            if (e != hipSuccess) return fail(std::string("bt_gzip_save: ") + hipGetErrorString(e));
            const auto t0 = std::chrono::steady_clock::now();
            if (!file.write(g.pin_out[p], out_prev)) return fail(std::string("bt_gzip_save: write to ") + path + ".tmp failed (disk full?)");
            s.seconds_host += since(t0);
            float ms[3] = {0, 0, 0};
            (void)hipEventElapsedTime(&ms[0], g.ev[p][0], g.ev[p][1]);
            (void)hipEventElapsedTime(&ms[1], g.ev[p][1], g.ev[p][2]);
            (void)hipEventElapsedTime(&ms[2], g.ev[p][4], g.ev[p][5]);
            s.seconds_h2d += ms[0] * 1e-3;
            s.seconds_kernels += ms[1] * 1e-3;
            s.seconds_d2h += ms[2] * 1e-3;
        }
    }
    const uint32_t trailer[2] = {(uint32_t)crc, (uint32_t)(n & 0xFFFFFFFFu)};
    if (!file.write(trailer, 8) || !file.finish()) return fail(std::string("bt_gzip_save: cannot complete ") + path + " (disk full?)");
    if (stats) *stats = s;
    return BT_OK;
}

int bt_diag_deflate(const uint8_t *h_in, uint64_t n, int last, uint8_t *h_out, uint64_t capacity, uint64_t *out_bytes, bt_deflate_stats *stats) {
    if ((n && !h_in) || !h_out || !out_bytes) return fail("bt_diag_deflate: null argument");
    if (capacity < stream_bound(n)) return fail("bt_diag_deflate: buffer too small (" + std::to_string(capacity) + " bytes, bt_deflate_bound gives " + std::to_string(stream_bound(n)) + ")");
    const uint64_t pieces = num_pieces(n);
    std::unique_ptr<Shared> sh(new Shared);
    std::vector<uint32_t> tokens(kPiece), slot(kPieceOut / 4), recs(pieces * kRecWords);
    uint32_t err = 0;
    uint64_t at = 0;
    for (uint64_t piece = 0; piece < pieces; ++piece) {
        const uint64_t off = piece * kPiece;
        const uint32_t len = off >= n ? 0u : (uint32_t)std::min<uint64_t>(kPiece, n - off);
        uint32_t *rec = recs.data() + piece * kRecWords;
        deflate_piece<LaneTeam>(*sh, h_in + off, len, last && piece + 1 == pieces, tokens.data(), reinterpret_cast<uint8_t *>(slot.data()), rec, &err);
        if (rec[0] > kPieceOut || at + rec[0] > capacity) err |= kErrCapacity;
        if (err) break;
        std::memcpy(h_out + at, slot.data(), rec[0]);
        at += rec[0];
    }
    if (error_word("bt_diag_deflate", err) != BT_OK) return BT_ERR;
    *out_bytes = at;
    if (stats) {
        *stats = bt_deflate_stats{};
        add_records(recs.data(), pieces, n, stats);
    }
    return BT_OK;
}

}  // extern "C"
