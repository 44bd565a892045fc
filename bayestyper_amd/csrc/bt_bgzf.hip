// libbtgpu: BGZF on the device (bt_bgzf), BGZF files written through it (bt_bgzf_save) and the host runs of the same code (bt_diag_bgzf, bt_diag_crc32).
// The block's code is bt_bgzf.hpp over bt_deflate.hpp, one text for both.  Replaces the bgzip + tabix pass a user runs over the VCF of `genotype -z`.
//
// bgzf_block_kernel: one 64-thread workgroup = one wavefront per block of 65280 input bytes: deflate_piece as in deflate_piece_kernel, then the CRC-32 of
//   the block's input by the same wavefront while the block is still in the cache (1.25 KiB of LDS beside btdeflate::Shared).
// bgzf_frame_kernel: deflate_compact_kernel's scan over the batch's sizes, each plus the 26 bytes of framing; a workgroup writes its block's header,
//   payload, CRC-32 and length to its place and the block's offset into the offsets array.
// bgzf_end_kernel: one workgroup writes the last offset, the EOF block when asked for, and the stream's length.
// A call runs batches of at most kBatch blocks, as bt_deflate does.
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "bt_bgzf.hpp"
#include "bt_gz_staging.hpp"
#include "bt_internal.hpp"

using bt::fail;
using namespace btbgzf;

namespace {

constexpr uint32_t kBatch = 1024;   // blocks per launch
constexpr unsigned COPY_BLOCK = 256;

__global__ __launch_bounds__(64) void bgzf_block_kernel(const uint8_t *__restrict__ in, uint64_t n, uint64_t first_block, uint32_t *__restrict__ tokens, uint8_t *__restrict__ stage,
                                                        uint32_t *__restrict__ recs, uint32_t *error) {
    __shared__ Shared sh;
    __shared__ CrcShared cs;
    const uint64_t block = first_block + blockIdx.x, off = block * kBlock;
    if (off >= n) return;   // (the grid is the number of blocks: never)
    const uint32_t len = (uint32_t)std::min<uint64_t>(kBlock, n - off);
    bgzf_block<WaveTeam>(sh, cs, in + off, len, tokens + (uint64_t)blockIdx.x * kPiece, stage + (uint64_t)blockIdx.x * kPieceOut, recs + block * kBlockRecWords, error);
}

// bases[batch]: where the batch's first block goes; bases[batch + 1] is written for the next batch.  offsets[block]: where the block went.
__global__ __launch_bounds__(COPY_BLOCK) void bgzf_frame_kernel(const uint8_t *__restrict__ stage, const uint32_t *__restrict__ recs, uint64_t first_block, uint32_t batch_blocks,
                                                                unsigned long long *bases, uint32_t batch, uint8_t *__restrict__ out, uint64_t capacity,
                                                                unsigned long long *__restrict__ offsets, uint32_t *error) {
    __shared__ unsigned long long part[COPY_BLOCK];
    const uint32_t b = blockIdx.x;
    unsigned long long s = 0;
    for (uint32_t j = threadIdx.x; j < b; j += COPY_BLOCK) s += recs[(first_block + j) * kBlockRecWords] + kFrame;
    part[threadIdx.x] = s;
    __syncthreads();
    for (unsigned w = COPY_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    const uint32_t *rec = recs + (first_block + b) * kBlockRecWords;
    const uint32_t payload = rec[0], size = payload + kFrame;
    const unsigned long long at = bases[batch] + part[0];
    if (payload > kPieceOut || size > kBlockMax || at + size > capacity) {   // never with a capacity of bt_bgzf_bound: the guard that nothing is written past it
        if (threadIdx.x == 0) atomicOr(error, (uint32_t)kErrCapacity);
        return;
    }
    if (threadIdx.x == 0) {
        offsets[first_block + b] = at;
        if (b + 1 == batch_blocks) bases[batch + 1] = at + size;
    }
    const uint8_t *src = stage + (uint64_t)b * kPieceOut;
    uint8_t *dst = out + at;
    if (threadIdx.x < kHeader) dst[threadIdx.x] = frame_byte(threadIdx.x, size - 1);
    if (threadIdx.x >= 32 && threadIdx.x < 32 + kTrailer) {
        const uint32_t t = threadIdx.x - 32;
        dst[kHeader + payload + t] = (uint8_t)(rec[5 + t / 4] >> (8 * (t % 4)));
    }
    dst += kHeader;
    // bytes up to the destination's first whole dword, whole dwords (the source is read at any alignment), the rest
    const uint32_t head = std::min<uint32_t>(payload, (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3)), words = (payload - head) / 4, tail = head + words * 4;
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    for (uint32_t w = threadIdx.x; w < words; w += COPY_BLOCK) *reinterpret_cast<uint32_t *>(dst + head + 4 * w) = load32(src + head + 4 * w);
    if (threadIdx.x < payload - tail) dst[tail + threadIdx.x] = src[tail + threadIdx.x];
}

// offsets[blocks] = where the data blocks end (the EOF block's offset), offsets[blocks + 1] = the stream's length
__global__ __launch_bounds__(64) void bgzf_end_kernel(const unsigned long long *__restrict__ bases, uint32_t batches, uint64_t blocks, int eof, uint8_t *__restrict__ out, uint64_t capacity,
                                                      unsigned long long *__restrict__ offsets, uint32_t *error) {
    const unsigned long long at = bases[batches], tail = eof ? kEof : 0;
    if (at + tail > capacity) {
        if (threadIdx.x == 0) atomicOr(error, (uint32_t)kErrCapacity);
        return;
    }
    if (threadIdx.x < tail) out[at + threadIdx.x] = eof_byte(threadIdx.x);
    if (threadIdx.x == 0) {
        offsets[blocks] = at;
        offsets[blocks + 1] = at + tail;
    }
}

// the scratch of a call (or of all slabs of a bt_bgzf_save): token areas and staging slots of one batch, the blocks' records and offsets, the batches' bases
struct Work {
    uint32_t *d_tokens = nullptr, *d_recs = nullptr, *d_error = nullptr;
    uint8_t *d_stage = nullptr;
    unsigned long long *d_bases = nullptr, *d_offsets = nullptr;
    hipError_t alloc(uint64_t blocks) {
        const uint64_t batches = (blocks + kBatch - 1) / kBatch, bb = std::max<uint64_t>(1, std::min<uint64_t>(blocks, kBatch));
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_tokens), bb * kPiece * 4);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_stage), bb * kPieceOut);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_recs), std::max<uint64_t>(1, blocks) * kBlockRecWords * 4);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_bases), (batches + 1) * 8);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_offsets), (blocks + 2) * 8);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_error), 4);
        return e;
    }
    ~Work() {
        (void)hipFree(d_tokens);
        (void)hipFree(d_stage);
        (void)hipFree(d_recs);
        (void)hipFree(d_bases);
        (void)hipFree(d_offsets);
        (void)hipFree(d_error);
    }
};

// the kernels of one stream of n bytes, enqueued on st; the blocks' records and offsets, the stream's length and the error word stay on the device
hipError_t enqueue(Work &w, hipStream_t st, const uint8_t *d_in, uint64_t n, int eof, uint8_t *d_out, uint64_t capacity) {
    const uint64_t blocks = num_blocks(n);
    // (every base zeroed: a batch whose predecessor stopped at its guard must not read a stale one)
    hipError_t e = hipMemsetAsync(w.d_bases, 0, ((blocks + kBatch - 1) / kBatch + 1) * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(w.d_error, 0, 4, st);
    uint64_t batch = 0;
    for (uint64_t first = 0; first < blocks && e == hipSuccess; first += kBatch, ++batch) {
        const uint32_t bb = (uint32_t)std::min<uint64_t>(kBatch, blocks - first);
        hipLaunchKernelGGL(bgzf_block_kernel, dim3(bb), dim3(64), 0, st, d_in, n, first, w.d_tokens, w.d_stage, w.d_recs, w.d_error);
        hipLaunchKernelGGL(bgzf_frame_kernel, dim3(bb), dim3(COPY_BLOCK), 0, st, (const uint8_t *)w.d_stage, (const uint32_t *)w.d_recs, first, bb, w.d_bases, (uint32_t)batch, d_out, capacity,
                           w.d_offsets, w.d_error);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bgzf_end_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long *)w.d_bases, (uint32_t)batch, blocks, eof, d_out, capacity, w.d_offsets, w.d_error);
        e = hipGetLastError();
    }
    return e;
}

void add_records(const uint32_t *recs, uint64_t blocks, uint64_t n, bt_deflate_stats *stats) {
    stats->pieces += blocks;
    stats->bytes_in += n;
    for (uint64_t i = 0; i < blocks; ++i) {
        const uint32_t *r = recs + i * kBlockRecWords;
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
    if (err & kErrTokens) what += " a block's tokens do not add up to its length;";
    if (err & kErrCapacity) what += " the output buffer is too small;";
    return fail(std::string(who) + ":" + what + " (error word " + std::to_string(err) + ")");
}

uint64_t slab_bytes() {
    uint64_t slab = 32ull << 20;
    if (const char *e = getenv("BT_BGZF_SLAB_BYTES")) {
        const uint64_t v = strtoull(e, nullptr, 10);
        if (v >= 1 && v <= (1ull << 30)) slab = v;
    }
    return (slab + kBlock - 1) / kBlock * kBlock;
}

std::string too_small(const char *who, uint64_t capacity, uint64_t n) {
    return std::string(who) + ": buffer too small (" + std::to_string(capacity) + " bytes, bt_bgzf_bound gives " + std::to_string(bgzf_bound(n)) + ")";
}

}  // namespace

extern "C" {

int bt_bgzf_bound(uint64_t n, uint64_t *capacity, uint64_t *blocks) {
    if (!capacity || !blocks) return fail("bt_bgzf_bound: null argument");
    *capacity = bgzf_bound(n);
    *blocks = num_blocks(n);
    return BT_OK;
}

int bt_bgzf(bt_ctx *ctx, const uint8_t *d_in, uint64_t n, int eof, uint8_t *d_out, uint64_t capacity, uint64_t *h_out_bytes, uint64_t *h_block_offsets, bt_deflate_stats *stats) {
    if (!ctx || (n && !d_in) || !d_out || !h_out_bytes) return fail("bt_bgzf: null argument");
    if (capacity < bgzf_bound(n)) return fail(too_small("bt_bgzf", capacity, n));
    BT_HIP(hipSetDevice(ctx->device));
    const uint64_t blocks = num_blocks(n);
    Work w;
    hipError_t e = w.alloc(blocks);
    if (e != hipSuccess) return fail(std::string("bt_bgzf: scratch buffers: ") + hipGetErrorString(e));
    BT_HIP(enqueue(w, ctx->stream, d_in, n, eof, d_out, capacity));
    std::vector<uint32_t> recs(blocks * kBlockRecWords);
    std::vector<unsigned long long> offsets(blocks + 2);
    uint32_t err = 0;
    if (blocks) BT_HIP(hipMemcpyAsync(recs.data(), w.d_recs, recs.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipMemcpyAsync(offsets.data(), w.d_offsets, offsets.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipMemcpyAsync(&err, w.d_error, 4, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipStreamSynchronize(ctx->stream));
    if (error_word("bt_bgzf", err) != BT_OK) return BT_ERR;
    *h_out_bytes = offsets[blocks + 1];
    if (h_block_offsets)
        for (uint64_t i = 0; i <= blocks; ++i) h_block_offsets[i] = offsets[i];
    if (stats) {
        *stats = bt_deflate_stats{};
        add_records(recs.data(), blocks, n, stats);
        if (stats->bytes_out + blocks * kFrame != offsets[blocks]) return fail("bt_bgzf: the blocks' sizes do not add up to the stream's length");
    }
    return BT_OK;
}

int bt_bgzf_save(bt_ctx *ctx, const char *path, const uint8_t *h_data, uint64_t n, uint32_t threads, uint64_t *h_block_offsets, uint64_t offsets_capacity, bt_deflate_stats *stats) {
    (void)threads;   // no host CRC on this route: nothing here runs on a thread pool, and the bytes cannot depend on it
    if (!ctx || !path || (n && !h_data)) return fail("bt_bgzf_save: null argument");
    const uint64_t total_blocks = num_blocks(n);
    if (h_block_offsets && offsets_capacity < total_blocks + 1)
        return fail("bt_bgzf_save: room for " + std::to_string(offsets_capacity) + " block offsets, " + std::to_string(total_blocks + 1) + " needed");
    BT_HIP(hipSetDevice(ctx->device));
    const uint64_t slab = std::max<uint64_t>(kBlock, std::min<uint64_t>(slab_bytes(), total_blocks * kBlock)), slabs = n ? (n + slab - 1) / slab : 1;
    const uint64_t bound = bgzf_bound(slab), slab_blocks = slab / kBlock;
    hipStream_t st = ctx->stream;
    btgz::GzStaging g;
    Work w;
    // the records' pinned copy holds the slab's records and, behind them, its offsets
    hipError_t e = g.alloc(st, slab, bound, slab_blocks * kBlockRecWords * 4 + (slab_blocks + 2) * 8, slabs > 1 ? 2 : 1);
    if (e == hipSuccess) e = w.alloc(slab_blocks);
    if (e != hipSuccess) return fail(std::string("bt_bgzf_save: staging buffers: ") + hipGetErrorString(e));
    btgz::TmpFile file;
    if (!file.open(path)) return fail(std::string("bt_bgzf_save: cannot create ") + path + ".tmp");
    bt_deflate_stats s{};
    uint64_t file_at = 0, block_at = 0;
    auto len_of = [&](uint64_t i) { return n ? std::min(slab, n - i * slab) : 0; };
    auto offsets_of = [&](int b) { return reinterpret_cast<const unsigned long long *>(g.pin_recs[b] + slab_blocks * kBlockRecWords); };
    // slab i: staged, copied in, compressed (all enqueued at once); then slab i - 1's copy out is enqueued on a stream of its own and slab i - 1 is written.
    // Only the last slab carries the EOF block.
    for (uint64_t i = 0; i <= slabs; ++i) {
        const int b = (int)(i & 1), p = b ^ 1;
        if (i < slabs) {
            const uint64_t len = len_of(i), blocks = num_blocks(len);
            const auto t0 = std::chrono::steady_clock::now();
            if (len) std::memcpy(g.pin_in[b], h_data + i * slab, len);
            s.seconds_host += btgz::since(t0);
            e = hipEventRecord(g.ev[b][0], st);
            if (e == hipSuccess && len) e = hipMemcpyAsync(g.d_in[b], g.pin_in[b], len, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipEventRecord(g.ev[b][1], st);
            if (e == hipSuccess) e = enqueue(w, st, g.d_in[b], len, i + 1 == slabs, g.d_out[b], bound);
            if (e == hipSuccess) e = hipEventRecord(g.ev[b][2], st);
            if (e == hipSuccess && blocks) e = hipMemcpyAsync(g.pin_recs[b], w.d_recs, blocks * kBlockRecWords * 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(const_cast<unsigned long long *>(offsets_of(b)), w.d_offsets, (blocks + 2) * 8, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(g.pin_total[b] + 1, w.d_error, 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipEventRecord(g.ev[b][3], st);
            if (e != hipSuccess) return fail(std::string("bt_bgzf_save: ") + hipGetErrorString(e));
        }
        if (i > 0) {   // slab i - 1 is compressed: its length is known, its bytes go out and are written
            e = hipEventSynchronize(g.ev[p][3]);
            if (e != hipSuccess) return fail(std::string("bt_bgzf_save: ") + hipGetErrorString(e));
            if (error_word("bt_bgzf_save", (uint32_t)g.pin_total[p][1]) != BT_OK) return BT_ERR;
            const uint64_t len = len_of(i - 1), blocks = num_blocks(len);
            const unsigned long long *off = offsets_of(p);
            const uint64_t out_prev = off[blocks + 1];
            if (out_prev > bound) return fail("bt_bgzf_save: a slab's stream is longer than its bound");
            add_records(g.pin_recs[p], blocks, len, &s);
            if (h_block_offsets) {
                for (uint64_t k = 0; k < blocks; ++k) h_block_offsets[block_at + k] = file_at + off[k];
                if (i == slabs) h_block_offsets[block_at + blocks] = file_at + off[blocks];
            }
            block_at += blocks;
            e = hipEventRecord(g.ev[p][4], g.copy_out);
            if (e == hipSuccess) e = hipMemcpyAsync(g.pin_out[p], g.d_out[p], out_prev, hipMemcpyDeviceToHost, g.copy_out);
            if (e == hipSuccess) e = hipEventRecord(g.ev[p][5], g.copy_out);
            if (e == hipSuccess) e = hipEventSynchronize(g.ev[p][5]);
            if (e != hipSuccess) return fail(std::string("bt_bgzf_save: ") + hipGetErrorString(e));
            const auto t0 = std::chrono::steady_clock::now();
            if (!file.write(g.pin_out[p], out_prev)) return fail(std::string("bt_bgzf_save: write to ") + path + ".tmp failed (disk full?)");
            s.seconds_host += btgz::since(t0);
            file_at += out_prev;
            float ms[3] = {0, 0, 0};
            (void)hipEventElapsedTime(&ms[0], g.ev[p][0], g.ev[p][1]);
            (void)hipEventElapsedTime(&ms[1], g.ev[p][1], g.ev[p][2]);
            (void)hipEventElapsedTime(&ms[2], g.ev[p][4], g.ev[p][5]);
            s.seconds_h2d += ms[0] * 1e-3;
            s.seconds_kernels += ms[1] * 1e-3;
            s.seconds_d2h += ms[2] * 1e-3;
        }
    }
    if (!file.finish()) return fail(std::string("bt_bgzf_save: cannot complete ") + path + " (disk full?)");
    if (stats) *stats = s;
    return BT_OK;
}

int bt_diag_bgzf(const uint8_t *h_in, uint64_t n, int eof, uint8_t *h_out, uint64_t capacity, uint64_t *out_bytes, uint64_t *h_block_offsets, bt_deflate_stats *stats) {
    if ((n && !h_in) || !h_out || !out_bytes) return fail("bt_diag_bgzf: null argument");
    if (capacity < bgzf_bound(n)) return fail(too_small("bt_diag_bgzf", capacity, n));
    const uint64_t blocks = num_blocks(n);
    std::unique_ptr<Shared> sh(new Shared);
    std::unique_ptr<CrcShared> cs(new CrcShared);
    std::vector<uint32_t> tokens(kPiece), slot(kPieceOut / 4), recs(blocks * kBlockRecWords);
    std::vector<uint64_t> offsets(blocks + 1);
    uint32_t err = 0;
    uint64_t at = 0;
    for (uint64_t block = 0; block < blocks && !err; ++block) {
        const uint64_t off = block * kBlock;
        const uint32_t len = (uint32_t)std::min<uint64_t>(kBlock, n - off);
        uint32_t *rec = recs.data() + block * kBlockRecWords;
        bgzf_block<LaneTeam>(*sh, *cs, h_in + off, len, tokens.data(), reinterpret_cast<uint8_t *>(slot.data()), rec, &err);
        const uint32_t size = rec[0] + kFrame;
        if (rec[0] > kPieceOut || size > kBlockMax || at + size > capacity) err |= kErrCapacity;
        if (err) break;
        offsets[block] = at;
        for (uint32_t i = 0; i < kHeader; ++i) h_out[at + i] = frame_byte(i, size - 1);
        std::memcpy(h_out + at + kHeader, slot.data(), rec[0]);
        for (uint32_t t = 0; t < kTrailer; ++t) h_out[at + kHeader + rec[0] + t] = (uint8_t)(rec[5 + t / 4] >> (8 * (t % 4)));
        at += size;
    }
    if (!err && at + (eof ? kEof : 0) > capacity) err |= kErrCapacity;
    if (error_word("bt_diag_bgzf", err) != BT_OK) return BT_ERR;
    offsets[blocks] = at;
    if (eof)
        for (uint32_t i = 0; i < kEof; ++i) h_out[at++] = eof_byte(i);
    *out_bytes = at;
    if (h_block_offsets) std::copy(offsets.begin(), offsets.end(), h_block_offsets);
    if (stats) {
        *stats = bt_deflate_stats{};
        add_records(recs.data(), blocks, n, stats);
    }
    return BT_OK;
}

int bt_diag_crc32(const uint8_t *h_in, uint64_t n, uint32_t *crc) {
    if ((n && !h_in) || !crc) return fail("bt_diag_crc32: null argument");
    std::unique_ptr<CrcShared> cs(new CrcShared);
    uLong c = crc32(0L, Z_NULL, 0);   // blocks of at most kBlock bytes through the team's routine, joined as zlib joins two CRCs
    for (uint64_t at = 0; at < n; at += kBlock) {
        const uint32_t len = (uint32_t)std::min<uint64_t>(kBlock, n - at);
        c = crc32_combine(c, crc32_team<LaneTeam>(*cs, h_in + at, len), (z_off_t)len);
    }
    *crc = (uint32_t)c;
    return BT_OK;
}

}  // extern "C"
