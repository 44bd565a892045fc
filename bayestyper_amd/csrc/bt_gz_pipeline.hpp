// The gzip and the BGZF device pipelines, written once over a format policy.  bt_deflate.hip (RawDeflate) and bt_bgzf.hip (Bgzf) keep their kernels as thin
// __global__ wrappers and their extern "C" functions as argument checks; everything between is here:
//   place_unit   the placement kernels' body: scan over the batch's sizes, guard, hand-over of the running total, framing bytes, aligned copy
//   Work, enqueue, add_records, error_word, slab_bytes   the scratch of a call and the launches of one stream
//   run_once     bt_deflate / bt_bgzf: one stream from device memory to device memory
//   save         bt_gzip_save / bt_bgzf_save: the double-buffered slab pipeline into a file that keeps a temporary name until it is complete
//   replay       bt_diag_deflate / bt_diag_bgzf: the same units by a team of one thread on the host
// A policy states what differs between the formats and nothing else; a third format is a third policy.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bt_bgzf.hpp"
#include "bt_internal.hpp"

namespace btgz {

using bt::fail;
using namespace btbgzf;   // (and btdeflate with it)

constexpr uint32_t kBatch = 1024;   // units per launch: the token areas stay at 256 MiB
constexpr unsigned COPY_BLOCK = 256;

template <class F>
struct Work;
// one stream of n bytes; flag: `last` of bt_deflate, `eof` of bt_bgzf
struct Job {
    const uint8_t *d_in;
    uint64_t n;
    int flag;
    uint8_t *d_out;
    uint64_t capacity;
};

// ---- the formats ---------------------------------------------------------------------------------------------------------------------------------------
// kUnit: input bytes per unit.  kRecWords: words of a unit's record, [0] its payload's size.  kHeader / kTrailer: framing bytes around a payload.
// kIndexed: the units' offsets are kept and an end kernel closes them — offsets[units] where the data ends, offsets[units + 1] the stream's length, the EOF
// block between the two when asked for; otherwise the stream's length is the base after the last batch.  compress: one unit by team T (the host replay's
// call; the kernels make the same one).  launch_batch / launch_end: defined beside the kernels they launch.
struct RawDeflate {
    static constexpr uint32_t kUnit = kPiece, kRecWords = btdeflate::kRecWords, kHeader = 0, kTrailer = 0, kFrame = 0;
    static constexpr bool kIndexed = false;
    static constexpr const char *kNoun = "piece", *kSlabEnv = "BT_GZIP_SLAB_BYTES";
    struct Scratch {
        Shared sh;
    };
    static uint64_t units(uint64_t n) { return num_pieces(n); }
    static uint64_t bound(uint64_t n) { return stream_bound(n); }
    template <class T>
    BTD_HD static void compress(Scratch &s, const uint8_t *in, uint32_t len, bool final_unit, uint32_t *tokens, uint8_t *out, uint32_t *rec, uint32_t *error) {
        deflate_piece<T>(s.sh, in, len, final_unit, tokens, out, rec, error);
    }
    static void launch_batch(Work<RawDeflate> &w, hipStream_t st, const Job &job, uint64_t first, uint32_t count, uint32_t batch);
};

struct Bgzf {
    static constexpr uint32_t kUnit = kBlock, kRecWords = kBlockRecWords, kHeader = btbgzf::kHeader, kTrailer = btbgzf::kTrailer, kFrame = btbgzf::kFrame;
    static constexpr bool kIndexed = true;
    static constexpr const char *kNoun = "block", *kSlabEnv = "BT_BGZF_SLAB_BYTES";
    struct Scratch {
        Shared sh;
        CrcShared cs;
    };
    static uint64_t units(uint64_t n) { return num_blocks(n); }
    static uint64_t bound(uint64_t n) { return bgzf_bound(n); }
    template <class T>
    BTD_HD static void compress(Scratch &s, const uint8_t *in, uint32_t len, bool, uint32_t *tokens, uint8_t *out, uint32_t *rec, uint32_t *error) {
        bgzf_block<T>(s.sh, s.cs, in, len, tokens, out, rec, error);
    }
    BTD_HD static uint8_t header_byte(uint32_t i, uint32_t size) { return frame_byte(i, size - 1); }
    BTD_HD static uint8_t trailer_byte(uint32_t t, const uint32_t *rec) { return (uint8_t)(rec[5 + t / 4] >> (8 * (t % 4))); }   // CRC-32, length
    static void launch_batch(Work<Bgzf> &w, hipStream_t st, const Job &job, uint64_t first, uint32_t count, uint32_t batch);
    static void launch_end(Work<Bgzf> &w, hipStream_t st, const Job &job, uint64_t units, uint32_t batches);
};

// a payload that its staging slot or (framed) the format's 16-bit BSIZE cannot hold: never from the compressor, the guard of device and host placement
template <class F>
BTD_HD inline bool too_large(uint32_t payload) {
    return payload > kPieceOut || (F::kFrame && payload + F::kFrame > kBlockMax);
}

// ---- placement -----------------------------------------------------------------------------------------------------------------------------------------
// One workgroup of COPY_BLOCK threads per unit.  It sums the sizes of the batch's units before its own (an exclusive scan done by each workgroup for itself:
// no workgroup waits for another) and writes its unit — header, payload from its staging slot, trailer — to its place.  bases[batch]: where the batch's
// first unit goes; the workgroup of the batch's last unit writes bases[batch + 1] for the next batch.  offsets[unit] (indexed formats): where the unit went.
template <class F>
__device__ __forceinline__ void place_unit(const uint8_t *__restrict__ stage, const uint32_t *__restrict__ recs, uint64_t first, uint32_t count, unsigned long long *bases, uint32_t batch,
                                           uint8_t *__restrict__ out, uint64_t capacity, unsigned long long *__restrict__ offsets, uint32_t *error) {
    __shared__ unsigned long long part[COPY_BLOCK];
    const uint32_t b = blockIdx.x;
    unsigned long long s = 0;
    for (uint32_t j = threadIdx.x; j < b; j += COPY_BLOCK) s += recs[(first + j) * F::kRecWords] + F::kFrame;
    part[threadIdx.x] = s;
    __syncthreads();
    for (unsigned w = COPY_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    const uint32_t *rec = recs + (first + b) * F::kRecWords;
    const uint32_t payload = rec[0], size = payload + F::kFrame;
    const unsigned long long at = bases[batch] + part[0];
    if (too_large<F>(payload) || at + size > capacity) {   // never with a capacity of the format's bound: the guard that nothing is written past it
        if (threadIdx.x == 0) atomicOr(error, (uint32_t)kErrCapacity);
        return;
    }
    if (threadIdx.x == 0) {
        if constexpr (F::kIndexed) offsets[first + b] = at;
        if (b + 1 == count) bases[batch + 1] = at + size;
    }
    const uint8_t *src = stage + (uint64_t)b * kPieceOut;
    uint8_t *dst = out + at;
    if constexpr (F::kFrame != 0) {
        if (threadIdx.x < F::kHeader) dst[threadIdx.x] = F::header_byte(threadIdx.x, size);
        if (threadIdx.x >= 32 && threadIdx.x < 32 + F::kTrailer) dst[F::kHeader + payload + threadIdx.x - 32] = F::trailer_byte(threadIdx.x - 32, rec);
        dst += F::kHeader;
    }
    // bytes up to the destination's first whole dword, whole dwords (the source is read at any alignment), the rest
    const uint32_t head = std::min<uint32_t>(payload, (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3)), words = (payload - head) / 4, tail = head + words * 4;
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    for (uint32_t w = threadIdx.x; w < words; w += COPY_BLOCK) *reinterpret_cast<uint32_t *>(dst + head + 4 * w) = load32(src + head + 4 * w);
    if (threadIdx.x < payload - tail) dst[tail + threadIdx.x] = src[tail + threadIdx.x];
}

// ---- the scratch of a call and the launches of one stream ---------------------------------------------------------------------------------------------------
// the scratch of a call (or of all slabs of a save): token areas and staging slots of one batch, the units' records (and offsets), the batches' bases
template <class F>
struct Work {
    uint32_t *d_tokens = nullptr, *d_recs = nullptr, *d_error = nullptr;
    uint8_t *d_stage = nullptr;
    unsigned long long *d_bases = nullptr, *d_offsets = nullptr;   // d_offsets: indexed formats only
    static uint64_t batches(uint64_t units) { return (units + kBatch - 1) / kBatch; }
    hipError_t alloc(uint64_t units) {
        units = std::max<uint64_t>(1, units);   // (an empty content of a format without an empty unit)
        const uint64_t bu = std::min<uint64_t>(units, kBatch);
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_tokens), bu * kPiece * 4);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_stage), bu * kPieceOut);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_recs), units * F::kRecWords * 4);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_bases), (batches(units) + 1) * 8);
        if (e == hipSuccess && F::kIndexed) e = hipMalloc(reinterpret_cast<void **>(&d_offsets), (units + 2) * 8);
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
    // the words a stream of `units` units leaves for the host, the stream's length last: an indexed format's offsets, otherwise the length alone
    static uint64_t tail_words(uint64_t units) { return F::kIndexed ? units + 2 : 1; }
    const unsigned long long *d_tail(uint64_t units) const { return F::kIndexed ? d_offsets : d_bases + batches(units); }
};

// the kernels of one stream, enqueued on st; the units' records, the tail words and the error word stay on the device
template <class F>
hipError_t enqueue(Work<F> &w, hipStream_t st, const Job &job) {
    const uint64_t units = F::units(job.n);
    // (every base zeroed: a batch whose predecessor stopped at its guard must not read a stale one)
    hipError_t e = hipMemsetAsync(w.d_bases, 0, (Work<F>::batches(units) + 1) * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(w.d_error, 0, 4, st);
    uint32_t batch = 0;
    for (uint64_t first = 0; first < units && e == hipSuccess; first += kBatch, ++batch) {
        F::launch_batch(w, st, job, first, (uint32_t)std::min<uint64_t>(kBatch, units - first), batch);
        e = hipGetLastError();
    }
    if constexpr (F::kIndexed)
        if (e == hipSuccess) {
            F::launch_end(w, st, job, units, batch);
            e = hipGetLastError();
        }
    return e;
}

template <class F>
void add_records(const uint32_t *recs, uint64_t units, uint64_t n, bt_deflate_stats *stats) {
    if (!stats) return;
    stats->pieces += units;
    stats->bytes_in += n;
    for (uint64_t i = 0; i < units; ++i) {
        const uint32_t *r = recs + i * F::kRecWords;
        stats->bytes_out += r[0];
        stats->stored_pieces += r[1];
        stats->literals += r[2];
        stats->matches += r[3];
        stats->matched_bytes += r[4];
    }
}

template <class F>
int error_word(const char *who, uint32_t err) {
    if (!err) return BT_OK;
    std::string what;
    if (err & kErrKraft) what += " a code's lengths could not be limited;";
    if (err & kErrBlockEnd) what += " a block did not end where its size was computed;";
    if (err & kErrTokens) what += std::string(" a ") + F::kNoun + "'s tokens do not add up to its length;";
    if (err & kErrCapacity) what += " the output buffer is too small;";
    return fail(std::string(who) + ":" + what + " (error word " + std::to_string(err) + ")");
}

template <class F>
uint64_t slab_bytes() {
    uint64_t slab = 32ull << 20;
    if (const char *e = getenv(F::kSlabEnv)) {
        const uint64_t v = strtoull(e, nullptr, 10);
        if (v >= 1 && v <= (1ull << 30)) slab = v;
    }
    return (slab + F::kUnit - 1) / F::kUnit * F::kUnit;
}

inline int too_small(const char *who, uint64_t capacity, const char *bound_fn, uint64_t bound) {
    return fail(std::string(who) + ": buffer too small (" + std::to_string(capacity) + " bytes, " + bound_fn + " gives " + std::to_string(bound) + ")");
}

// ---- one stream, device memory to device memory ------------------------------------------------------------------------------------------------------------
template <class F>
int run_once(const char *who, bt_ctx *ctx, const Job &job, uint64_t *h_out_bytes, uint64_t *h_offsets, bt_deflate_stats *stats) {
    BT_HIP(hipSetDevice(ctx->device));
    const uint64_t units = F::units(job.n);
    Work<F> w;
    hipError_t e = w.alloc(units);
    if (e != hipSuccess) return fail(std::string(who) + ": scratch buffers: " + hipGetErrorString(e));
    BT_HIP(enqueue<F>(w, ctx->stream, job));
    std::vector<uint32_t> recs(units * F::kRecWords);
    std::vector<unsigned long long> tail(Work<F>::tail_words(units));
    uint32_t err = 0;
    if (units) BT_HIP(hipMemcpyAsync(recs.data(), w.d_recs, recs.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipMemcpyAsync(tail.data(), w.d_tail(units), tail.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipMemcpyAsync(&err, w.d_error, 4, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipStreamSynchronize(ctx->stream));
    if (error_word<F>(who, err) != BT_OK) return BT_ERR;
    *h_out_bytes = tail.back();
    if (F::kIndexed && h_offsets)
        for (uint64_t i = 0; i <= units; ++i) h_offsets[i] = tail[i];
    if (stats) {
        *stats = bt_deflate_stats{};
        add_records<F>(recs.data(), units, job.n, stats);
        if (stats->bytes_out + units * F::kFrame != (F::kIndexed ? tail[units] : tail.back()))
            return fail(std::string(who) + ": the " + F::kNoun + "s' sizes do not add up to the stream's length");
    }
    return BT_OK;
}

// ---- the slab pipeline ---------------------------------------------------------------------------------------------------------------------------------
// what a slab pipeline stages through: per slab parity a pinned input, a device input, a device output, a pinned output, the pinned copy of the records
// and the tail words
struct GzStaging {
    uint8_t *pin_in[2] = {}, *pin_out[2] = {}, *d_in[2] = {}, *d_out[2] = {};
    uint32_t *pin_recs[2] = {}, *pin_error[2] = {};
    hipEvent_t ev[2][6] = {};                // h2d begin / end, kernels end, results copied, d2h begin / end
    hipStream_t copy_out = nullptr;
    hipStream_t main = nullptr;
    hipError_t alloc(hipStream_t on, uint64_t slab, uint64_t bound, uint64_t rec_bytes, int n) {
        main = on;
        hipError_t e = hipStreamCreateWithFlags(&copy_out, hipStreamNonBlocking);
        for (int i = 0; i < n && e == hipSuccess; ++i) {
            e = hipHostMalloc(reinterpret_cast<void **>(&pin_in[i]), std::max<uint64_t>(slab, 1), hipHostMallocDefault);
            if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&pin_out[i]), bound, hipHostMallocDefault);
            if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&pin_recs[i]), rec_bytes, hipHostMallocDefault);
            if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&pin_error[i]), 4, hipHostMallocDefault);
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_in[i]), std::max<uint64_t>(slab, 1));
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_out[i]), bound);
            for (int k = 0; k < 6 && e == hipSuccess; ++k) e = hipEventCreate(&ev[i][k]);
        }
        return e;
    }
    ~GzStaging() {
        if (main) (void)hipStreamSynchronize(main);   // (an error path may leave work in flight)
        if (copy_out) {
            (void)hipStreamSynchronize(copy_out);
            (void)hipStreamDestroy(copy_out);
        }
        for (int i = 0; i < 2; ++i) {
            if (pin_in[i]) (void)hipHostFree(pin_in[i]);
            if (pin_out[i]) (void)hipHostFree(pin_out[i]);
            if (pin_recs[i]) (void)hipHostFree(pin_recs[i]);
            if (pin_error[i]) (void)hipHostFree(pin_error[i]);
            (void)hipFree(d_in[i]);
            (void)hipFree(d_out[i]);
            for (int k = 0; k < 6; ++k)
                if (ev[i][k]) (void)hipEventDestroy(ev[i][k]);
        }
    }
};

// the file under a temporary name until it is complete
struct TmpFile {
    FILE *f = nullptr;
    std::string path, tmp;
    ~TmpFile() {
        if (f) {
            fclose(f);
            remove(tmp.c_str());
        }
    }
    bool open(const char *p) {
        path = p;
        tmp = path + ".tmp";
        f = fopen(tmp.c_str(), "wb");
        return f != nullptr;
    }
    bool write(const void *p, size_t n) { return !n || fwrite(p, 1, n, f) == n; }
    bool finish() {
        const bool ok = fflush(f) == 0;
        const bool closed = fclose(f) == 0;
        f = nullptr;
        if (!ok || !closed || rename(tmp.c_str(), path.c_str()) != 0) {
            remove(tmp.c_str());
            return false;
        }
        return true;
    }
};

inline double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// what a caller of save adds to the slabs; these do nothing
struct NoExtras {
    bool before(TmpFile &) { return true; }           // written in front of the slabs' streams
    void overlap(const uint8_t *, uint64_t) {}        // the host's share of a slab, done while the device compresses it
    void drained(const unsigned long long *, uint64_t, uint64_t, bool) {}   // a compressed slab's tail words, units, place in the file; whether it is the last
    bool after(TmpFile &) { return true; }            // written behind them
};

// h_data[0..n) -> the file `path`.  Slab i: staged, copied in, compressed (all enqueued at once); then slab i - 1's copy out is enqueued on a stream of its
// own, the caller's share of slab i is done while the device works, and slab i - 1 is written.  Only the last slab carries the stream's end (flag).
template <class F, class Extras>
int save(const char *who, bt_ctx *ctx, const char *path, const uint8_t *h_data, uint64_t n, Extras &x, bt_deflate_stats *stats) {
    const std::string me = std::string(who) + ": ";
    BT_HIP(hipSetDevice(ctx->device));
    const uint64_t slab = std::max<uint64_t>(F::kUnit, std::min<uint64_t>(slab_bytes<F>(), (n + F::kUnit - 1) / F::kUnit * F::kUnit)), slabs = n ? (n + slab - 1) / slab : 1;
    const uint64_t bound = F::bound(slab), slab_units = slab / F::kUnit;
    const uint64_t tail_at = (slab_units * F::kRecWords + 1) / 2 * 2;   // the records' pinned copy holds the slab's records and, behind them on 8 bytes, its tail words
    hipStream_t st = ctx->stream;
    GzStaging g;
    Work<F> w;
    hipError_t e = g.alloc(st, slab, bound, tail_at * 4 + Work<F>::tail_words(slab_units) * 8, slabs > 1 ? 2 : 1);
    if (e == hipSuccess) e = w.alloc(slab_units);
    if (e != hipSuccess) return fail(me + "staging buffers: " + hipGetErrorString(e));
    TmpFile file;
    if (!file.open(path)) return fail(me + "cannot create " + path + ".tmp");
    const std::string write_failed = me + "write to " + path + ".tmp failed (disk full?)";
    if (!x.before(file)) return fail(write_failed);
    bt_deflate_stats s{};
    uint64_t file_at = 0;   // bytes of the slabs' streams written so far
    auto len_of = [&](uint64_t i) { return n ? std::min(slab, n - i * slab) : 0; };
    auto tail_of = [&](int b) { return reinterpret_cast<unsigned long long *>(g.pin_recs[b] + tail_at); };
    for (uint64_t i = 0; i <= slabs; ++i) {
        const int b = (int)(i & 1), p = b ^ 1;
        if (i < slabs) {
            const uint64_t len = len_of(i), units = F::units(len);
            const auto t0 = std::chrono::steady_clock::now();
            if (len) std::memcpy(g.pin_in[b], h_data + i * slab, len);
            s.seconds_host += since(t0);
            e = hipEventRecord(g.ev[b][0], st);
            if (e == hipSuccess && len) e = hipMemcpyAsync(g.d_in[b], g.pin_in[b], len, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipEventRecord(g.ev[b][1], st);
            if (e == hipSuccess) e = enqueue<F>(w, st, Job{g.d_in[b], len, i + 1 == slabs, g.d_out[b], bound});
            if (e == hipSuccess) e = hipEventRecord(g.ev[b][2], st);
            if (e == hipSuccess && units) e = hipMemcpyAsync(g.pin_recs[b], w.d_recs, units * F::kRecWords * 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(tail_of(b), w.d_tail(units), Work<F>::tail_words(units) * 8, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(g.pin_error[b], w.d_error, 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipEventRecord(g.ev[b][3], st);
            if (e != hipSuccess) return fail(me + hipGetErrorString(e));
        }
        uint64_t out_prev = 0;
        if (i > 0) {   // slab i - 1 is compressed: its length is known, its bytes start their way out
            e = hipEventSynchronize(g.ev[p][3]);
            if (e != hipSuccess) return fail(me + hipGetErrorString(e));
            if (error_word<F>(who, *g.pin_error[p]) != BT_OK) return BT_ERR;
            const uint64_t len = len_of(i - 1), units = F::units(len);
            const unsigned long long *tail = tail_of(p);
            out_prev = tail[Work<F>::tail_words(units) - 1];
            if (out_prev > bound) return fail(me + "a slab's stream is longer than its bound");
            add_records<F>(g.pin_recs[p], units, len, &s);
            x.drained(tail, units, file_at, i == slabs);
            e = hipEventRecord(g.ev[p][4], g.copy_out);
            if (e == hipSuccess) e = hipMemcpyAsync(g.pin_out[p], g.d_out[p], out_prev, hipMemcpyDeviceToHost, g.copy_out);
            if (e == hipSuccess) e = hipEventRecord(g.ev[p][5], g.copy_out);
            if (e != hipSuccess) return fail(me + hipGetErrorString(e));
        }
        if (i < slabs && len_of(i)) {
            const auto t0 = std::chrono::steady_clock::now();
            x.overlap(h_data + i * slab, len_of(i));
            s.seconds_host += since(t0);
        }
        if (i > 0) {
            e = hipEventSynchronize(g.ev[p][5]);
            if (e != hipSuccess) return fail(me + hipGetErrorString(e));
            const auto t0 = std::chrono::steady_clock::now();
            if (!file.write(g.pin_out[p], out_prev)) return fail(write_failed);
            s.seconds_host += since(t0);
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
    if (!x.after(file) || !file.finish()) return fail(me + "cannot complete " + path + " (disk full?)");
    if (stats) *stats = s;
    return BT_OK;
}

// ---- the host replay: the units of one stream, one at a time, by a team of one thread ---------------------------------------------------------------------
template <class F>
int replay(const char *who, const uint8_t *h_in, uint64_t n, int flag, uint8_t *h_out, uint64_t capacity, uint64_t *out_bytes, uint64_t *h_offsets, bt_deflate_stats *stats) {
    const uint64_t units = F::units(n);
    std::unique_ptr<typename F::Scratch> scratch(new typename F::Scratch);
    std::vector<uint32_t> tokens(kPiece), slot(kPieceOut / 4), recs(units * F::kRecWords);
    std::vector<uint64_t> offsets(units + 1);
    uint32_t err = 0;
    uint64_t at = 0;
    for (uint64_t unit = 0; unit < units; ++unit) {
        const uint64_t off = unit * F::kUnit;
        const uint32_t len = off >= n ? 0u : (uint32_t)std::min<uint64_t>(F::kUnit, n - off);
        uint32_t *rec = recs.data() + unit * F::kRecWords;
        F::template compress<LaneTeam>(*scratch, h_in + off, len, flag && unit + 1 == units, tokens.data(), reinterpret_cast<uint8_t *>(slot.data()), rec, &err);
        const uint32_t payload = rec[0], size = payload + F::kFrame;
        if (too_large<F>(payload) || at + size > capacity) err |= kErrCapacity;
        if (err) break;
        offsets[unit] = at;
        uint8_t *dst = h_out + at;
        if constexpr (F::kFrame != 0) {
            for (uint32_t i = 0; i < F::kHeader; ++i) dst[i] = F::header_byte(i, size);
            for (uint32_t t = 0; t < F::kTrailer; ++t) dst[F::kHeader + payload + t] = F::trailer_byte(t, rec);
        }
        std::memcpy(dst + F::kHeader, slot.data(), payload);
        at += size;
    }
    const uint32_t end = F::kIndexed && flag ? kEof : 0;   // the end kernel's part
    if (!err && at + end > capacity) err |= kErrCapacity;
    if (error_word<F>(who, err) != BT_OK) return BT_ERR;
    offsets[units] = at;
    for (uint32_t i = 0; i < end; ++i) h_out[at++] = eof_byte(i);
    *out_bytes = at;
    if (F::kIndexed && h_offsets) std::copy(offsets.begin(), offsets.end(), h_offsets);
    if (stats) {
        *stats = bt_deflate_stats{};
        add_records<F>(recs.data(), units, n, stats);
    }
    return BT_OK;
}

}  // namespace btgz
