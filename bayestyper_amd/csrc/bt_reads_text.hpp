// The second half of the converters that turn inflated bytes into reads text ("<bases>\n" per kept item), written once for bt_bam.hip (an item is a record)
// and bt_fastq.hip (an item is a line).  Device and driver code: only those two files include it, each gets its own copy of the kernels, and the host check
// programs under tools/ never see it.  A format finds its items and judges them (its measure kernel, which ends in tally_sizes); from sizes[] on the work is
// the same:
//   scan256               the inclusive scan of a 256-thread workgroup in LDS: every scan loop of the two files
//   tally_sizes           the end of a measure kernel: a sum per workgroup, the kept items and their bases into the result
//   text_offsets_kernel   one workgroup: exclusive scan over the workgroups' sums, the text's length
//   text_emit_kernel      a workgroup per 256 items rebuilds its items' offsets from sizes[]; a wavefront per item, a lane per base: 64 consecutive bytes of
//                         text per store instruction.  Where an item's sequence lies and how its bytes read is the format's Source.
//   TextWork, text_emit   the device arrays behind these kernels, and the driver's launches and copy-back
#pragma once
#include <algorithm>
#include <string>

#include "bt_bgzf_stream.hpp"
#include "bt_internal.hpp"

namespace bt {
namespace {

constexpr uint32_t kTextTile = 256;   // items per workgroup of the measure and emit kernels
constexpr unsigned long long kNoError = ~0ull;

// What the shared kernels leave; a format's result struct starts with it.
struct TextResult {
    unsigned long long err;   // item << 2 | condition of the first failing item, the smallest by a 64-bit atomic minimum; what names an item is the format's
    unsigned long long consumed, text_bytes, kept, bases;
    uint32_t overflow;        // 2: the text's capacity (1 is BAM's own)
};

// s[t] = op(... op(op(s[0], s[1]), s[2]) ..., s[t]) over the 256 threads' values v, in thread order: op(earlier, later) need not commute.  Two barriers per
// step; the result is there for every thread on return.
template <typename T, typename Op>
__device__ inline void scan256(T *s, T v, T identity, Op op) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const T o = threadIdx.x >= d ? s[threadIdx.x - d] : identity;
        __syncthreads();
        s[threadIdx.x] = op(o, s[threadIdx.x]);
        __syncthreads();
    }
}

struct Add {
    template <typename T>
    __device__ T operator()(T earlier, T later) const {
        return earlier + later;
    }
};

// Every thread of a measure kernel's workgroup ends here with its item's size: bases + 1, or 0 for an item that is not kept and for no item.
__device__ inline void tally_sizes(uint32_t size, unsigned long long *__restrict__ sums, TextResult *res) {
    __shared__ unsigned long long s_sum;
    __shared__ uint32_t s_kept;
    if (threadIdx.x == 0) s_sum = 0, s_kept = 0;
    __syncthreads();
    if (size) {
        atomicAdd(&s_sum, (unsigned long long)size);
        atomicAdd(&s_kept, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = s_sum;
        if (s_kept) {
            atomicAdd(&res->kept, (unsigned long long)s_kept);
            atomicAdd(&res->bases, s_sum - s_kept);
        }
    }
}

// sums[0..nb) -> exclusive prefix sums in place; the total is the text's length
__global__ __launch_bounds__(256) void text_offsets_kernel(unsigned long long *sums, uint32_t nb, TextResult *res) {
    __shared__ unsigned long long part[256];
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < nb; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const unsigned long long v = i < nb ? sums[i] : 0;
        scan256(part, v, 0ull, Add());
        if (i < nb) sums[i] = carry + part[threadIdx.x] - v;
        carry += part[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) res->text_bytes = carry;
}

// Source: sequence(i) is where item i's sequence starts, byte(seq, j) the text's byte j of it.
template <typename Source>
__global__ __launch_bounds__(kTextTile) void text_emit_kernel(const Source src, const uint32_t *__restrict__ sizes, const unsigned long long *__restrict__ sums, uint32_t n,
                                                              char *__restrict__ text, uint64_t capacity, TextResult *res) {
    __shared__ uint32_t part[kTextTile], size_of[kTextTile];
    const uint32_t first = blockIdx.x * kTextTile, i = first + threadIdx.x;
    const uint32_t v = i < n ? sizes[i] : 0;
    size_of[threadIdx.x] = v;
    scan256(part, v, 0u, Add());   // a tile's sizes sum to less than the data's length: 32 bits
    const uint64_t tile_at = sums[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, in_tile = std::min<uint32_t>(kTextTile, n - first);
    for (uint32_t r = threadIdx.x >> 6; r < in_tile; r += kTextTile / 64) {
        const uint32_t size = size_of[r];
        if (!size) continue;
        const uint64_t at = tile_at + part[r] - size;
        if (at + size > capacity) {   // nothing is written past the capacity
            if (lane == 0) res->overflow = 2;
            continue;
        }
        const uint8_t *seq = src.sequence(first + r);
        const uint32_t bases = size - 1;
        for (uint32_t j = lane; j < bases; j += 64) text[at + j] = (char)Source::byte(seq, j);
        if (lane == 0) text[at + bases] = '\n';
    }
}

template <typename... P>
void release(P *&...p) {
    for (void *q : {(void *)p...})
        if (q) (void)hipFree(q);
    ((p = nullptr), ...);
}

// Device arrays of one conversion that every format has: a size per item, a sum per 256 items, the result.  They stay for the next call of a stream object.
template <typename Result>
struct TextWork {
    uint32_t *d_sizes = nullptr;
    unsigned long long *d_sums = nullptr;
    Result *d_res = nullptr;
    uint64_t cap_sizes = 0, cap_sums = 0, cap_res = 0;   // bytes
    // the result of a call that has met nothing yet, here and on the device
    int start(bt_ctx *ctx, Result &r) {
        if (grow(reinterpret_cast<void **>(&d_res), &cap_res, sizeof(Result)) != BT_OK) return BT_ERR;
        r = Result{};
        r.err = kNoError;
        BT_HIP(hipMemcpyAsync(d_res, &r, sizeof r, hipMemcpyHostToDevice, ctx->stream));
        BT_HIP(hipStreamSynchronize(ctx->stream));   // (r is pageable: the copy has left it)
        return BT_OK;
    }
    int fetch(bt_ctx *ctx, Result &r) {
        BT_HIP(hipMemcpyAsync(&r, d_res, sizeof r, hipMemcpyDeviceToHost, ctx->stream));
        BT_HIP(hipStreamSynchronize(ctx->stream));
        return BT_OK;
    }
    int reserve(uint64_t items) {
        if (grow(reinterpret_cast<void **>(&d_sizes), &cap_sizes, items * 4) != BT_OK) return BT_ERR;
        return grow(reinterpret_cast<void **>(&d_sums), &cap_sums, (items / kTextTile + 1) * 8);
    }
    ~TextWork() { release(d_sizes, d_sums, d_res); }
};

// The driver's second half over n items (reserved): `measure(nb)` launches the format's measure kernel over nb workgroups, then the offsets, the text, and
// the result in r.  The format reports its own errors from r first, then a text that did not fit with capacity_error.
template <typename Result, typename Measure, typename Source>
int text_emit(bt_ctx *ctx, TextWork<Result> &w, uint32_t n, Measure measure, const Source &src, char *d_text, uint64_t capacity, Result &r) {
    if (!n) return BT_OK;
    const uint32_t nb = (n + kTextTile - 1) / kTextTile;
    measure(nb);
    BT_CHECK_LAUNCH();
    hipLaunchKernelGGL(text_offsets_kernel, dim3(1), dim3(256), 0, ctx->stream, w.d_sums, nb, static_cast<TextResult *>(w.d_res));
    BT_CHECK_LAUNCH();
    hipLaunchKernelGGL(text_emit_kernel<Source>, dim3(nb), dim3(kTextTile), 0, ctx->stream, src, (const uint32_t *)w.d_sizes, (const unsigned long long *)w.d_sums, n, d_text, capacity,
                       static_cast<TextResult *>(w.d_res));
    BT_CHECK_LAUNCH();
    return w.fetch(ctx, r);
}

inline int capacity_error(const char *who, uint64_t capacity, uint64_t text_bytes) {
    return fail(std::string(who) + ": capacity " + std::to_string(capacity) + " below the text's " + std::to_string(text_bytes) + " bytes");
}

}  // namespace
}  // namespace bt
