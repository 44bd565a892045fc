// libbtgpu: a BAM sample's reads as the reads text of bt_reads.hip, on the device.
//   bt_bam_reads_text      inflated BAM records -> "<bases>\n" per kept record (bt_bam.hpp holds the record's code, one text for kernels and host)
//   bt_bam_scan_*          the stream object: slabs of whole BGZF blocks from the host -> inflate (bt_bgzf_stream.hpp) behind the carried tail -> text
//   bt_diag_bam_reads_text the host run of the same record code
// What `samtools fastq` does on the host before the reads of a BAM can enter the reads route (the reference's workflow counts BAMs with kmc -fbam).
//
// Record starts are a dependent chain (each start comes from the previous block_size), and no workgroup may wait on another, so the chain is walked in segments
// from guessed entries, the guesses are checked in order, and wrong ones walked again (bam_guess_kernel, bam_stitch_kernel, bam_fill_kernel: see there).  Then:
//   bam_measure_kernel  a thread per record: fields checked, flag & skip_flags judged, l_seq + 1 (0 when skipped) into sizes[], a sum per workgroup
// From sizes[] on the work is that of every reads text and is written once, in bt_reads_text.hpp (which bt_fastq.hip shares):
//   text_offsets_kernel            one workgroup: exclusive scan over the workgroups' sums, the text's length
//   text_emit_kernel<BamSource>    a workgroup per 256 records rebuilds its records' offsets from sizes[]; a wavefront per record, a lane per base: 64
//                                  consecutive bytes of text per store instruction, 32 consecutive bytes of the packed sequence per load instruction
// The first failing record is the one at the smallest offset: a 64-bit atomic minimum over offset << 2 | condition.
#include <algorithm>
#include <memory>

#include "bt_bam.hpp"
#include "bt_bgzf_stream.hpp"
#include "bt_internal.hpp"
#include "bt_reads_text.hpp"

using namespace bt;
using namespace btbam;

namespace {

struct BamResult : TextResult {   // err: offset << 2 | condition of the first failing record; overflow 1: starts[] too small (never: it is sized for the shortest record)
    uint32_t n_records;
};

// ---- record starts ------------------------------------------------------------------------------------------------------------------------------------------
// The slab is cut into at most kMaxSegs segments of equal length.  A segment's walk needs its first record start, which only the walk of the segments before it
// can tell, so it is GUESSED, the walks run in parallel, and the guesses are then checked one after the other:
//   bam_guess_kernel   a wavefront per segment: the 64 lanes try 64 consecutive offsets at a time for one that starts three plausible records in a row
//                      (read_record's check), the first such offset is the guess; lane 0 walks from it to the segment's end and leaves the number of records
//                      and where the walk left the segment.  Segment 0 starts at offset 0, which is known.
//   bam_stitch_kernel  one workgroup: the segments' results into LDS, then thread 0 goes through them in order: the true entry of a segment is where the walk of
//                      the segment before left off; when the guess equals it the segment's result stands, otherwise thread 0 walks that segment again from the
//                      true entry.  It also sums the counts: entry[] and base[] per segment.
//   bam_fill_kernel    a thread per segment walks from the segment's true entry and stores the starts at their final places.
// So the starts are those of the chain from offset 0 whatever the data looks like; bytes that only look like records (in a quality string, an auxiliary array) cost
// time, never a wrong start.  No workgroup waits on another: the kernels follow each other on the stream.
constexpr uint32_t kMaxSegs = 2048, kMinSeg = 1024, kPlausible = 3;
constexpr unsigned long long kNone = ~0ull;
enum : uint32_t { kWalkOn = 0, kWalkEnd = 1, kWalkBad = 2 };   // left the segment; met a record that is not whole; met a block_size below 32

struct Seg {
    unsigned long long guess, exit;   // exit: the first start at or behind the segment's end, or where the walk stopped
    uint32_t count, stop;
};

__device__ inline Seg walk_segment(const uint8_t *__restrict__ bam, uint64_t len, uint64_t p, uint64_t limit, uint32_t *__restrict__ starts) {
    Seg w{p, p, 0, kWalkOn};
    while (p < limit) {
        if (len - p < 4) {
            w.stop = kWalkEnd;
            break;
        }
        const uint32_t bs = rd32(bam + p);
        if (bs < kFixed || bs > 0x7FFFFFFFu) {
            w.stop = kWalkBad;
            break;
        }
        if (4ull + bs > len - p) {
            w.stop = kWalkEnd;
            break;
        }
        if (starts) starts[w.count] = (uint32_t)p;
        ++w.count;
        p += 4ull + bs;
    }
    w.exit = p;
    return w;
}

// kPlausible records in a row from q on (fewer when the data ends first), each with what a writer always leaves: a block_size that covers its fields and stays
// below 64 MiB, reference indices of at least -1, a read name that ends with its NUL.  A chain that jumps past the data's end is none (only the slab's last
// segment can lose a true start to this rule, and then walks again).
__device__ inline bool plausible_start(const uint8_t *__restrict__ bam, uint64_t len, uint64_t q) {
    for (uint32_t i = 0; i < kPlausible; ++i) {
        if (q == len) return true;
        if (q > len) return false;
        if (len - q < kHead) return i > 0;
        if (rd32(bam + q) > (1u << 26)) return false;
        Record r;
        if (read_record(bam + q, len - q, r) != kRecOk) return false;
        const uint32_t l_read_name = bam[q + 12];
        if ((int32_t)rd32(bam + q + 4) < -1 || (int32_t)rd32(bam + q + 24) < -1 || l_read_name == 0) return false;
        if (len - q < kHead + l_read_name || bam[q + kHead + l_read_name - 1] != 0) return false;
        q += 4ull + r.block_size;
    }
    return true;
}

__global__ __launch_bounds__(64) void bam_guess_kernel(const uint8_t *__restrict__ bam, uint64_t len, uint64_t seg_len, Seg *__restrict__ segs) {
    const uint64_t begin = (uint64_t)blockIdx.x * seg_len, end = std::min<uint64_t>(len, begin + seg_len);
    unsigned long long guess = blockIdx.x == 0 ? 0 : kNone;
    for (uint64_t base = begin; guess == kNone && base < end; base += 64) {
        const uint64_t q = base + threadIdx.x;
        const unsigned long long hit = __ballot(q < end && plausible_start(bam, len, q));
        if (hit) guess = base + (uint64_t)__builtin_ctzll(hit);
    }
    if (threadIdx.x == 0) {
        Seg w{kNone, kNone, 0, kWalkOn};
        if (guess != kNone) w = walk_segment(bam, len, guess, end, nullptr);
        segs[blockIdx.x] = w;
    }
}

__global__ __launch_bounds__(256) void bam_stitch_kernel(const uint8_t *__restrict__ bam, uint64_t len, uint64_t seg_len, uint32_t num_segs, const Seg *__restrict__ segs,
                                                         unsigned long long *__restrict__ entry, uint32_t *__restrict__ base, BamResult *res) {
    __shared__ Seg sseg[kMaxSegs];
    for (uint32_t s = threadIdx.x; s < num_segs; s += blockDim.x) sseg[s] = segs[s];
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint64_t at = 0;
    uint32_t total = 0, stop = kWalkOn;
    for (uint32_t s = 0; s < num_segs; ++s) {
        const uint64_t end = std::min<uint64_t>(len, (uint64_t)(s + 1) * seg_len);
        base[s] = total;
        if (stop != kWalkOn || at >= end) {   // (a record longer than the segment: no start lies in it)
            entry[s] = kNone;
            continue;
        }
        Seg g = sseg[s];
        if (g.guess != at) g = walk_segment(bam, len, at, end, nullptr);
        entry[s] = at;
        total += g.count;
        at = g.exit;
        stop = g.stop;
    }
    if (stop == kWalkBad)
        atomicMin(&res->err, (unsigned long long)at << 2 | kRecShort);
    else if (len - at >= kHead) {   // the record that is not whole is judged by what is there of it
        Record r;
        const uint32_t e = read_record(bam + at, len - at, r);
        if (e != kRecOk) atomicMin(&res->err, (unsigned long long)at << 2 | e);
    }
    res->consumed = at;
    res->n_records = total;
}

__global__ __launch_bounds__(64) void bam_fill_kernel(const uint8_t *__restrict__ bam, uint64_t len, uint64_t seg_len, uint32_t num_segs, const unsigned long long *__restrict__ entry,
                                                      const uint32_t *__restrict__ base, uint32_t *__restrict__ starts, uint32_t starts_cap, BamResult *res) {
    const uint32_t s = blockIdx.x * 64 + threadIdx.x;
    if (s >= num_segs || entry[s] == kNone) return;
    if (res->n_records > starts_cap) {   // (never: starts[] is sized for the shortest record)
        res->overflow = 1;
        return;
    }
    walk_segment(bam, len, entry[s], std::min<uint64_t>(len, (uint64_t)(s + 1) * seg_len), starts + base[s]);
}

__global__ __launch_bounds__(kTextTile) void bam_measure_kernel(const uint8_t *__restrict__ bam, uint64_t len, const uint32_t *__restrict__ starts, uint32_t n, uint32_t skip_flags,
                                                            uint32_t *__restrict__ sizes, unsigned long long *__restrict__ sums, BamResult *res) {
    const uint32_t i = blockIdx.x * kTextTile + threadIdx.x;
    uint32_t size = 0;
    if (i < n) {
        const uint64_t at = starts[i];
        Record r;
        const uint32_t e = read_record(bam + at, len - at, r);   // (whole: the walk stored only whole records, of at least kHead bytes)
        if (e != kRecOk)
            atomicMin(&res->err, (unsigned long long)at << 2 | e);
        else if (!(r.flag & skip_flags))
            size = r.l_seq + 1;
        sizes[i] = size;
    }
    tally_sizes(size, sums, res);
}

// text_emit_kernel's view of the records: the packed sequence lies behind the record's name and CIGAR
struct BamSource {
    const uint8_t *__restrict__ bam;
    const uint32_t *__restrict__ starts;
    __device__ const uint8_t *sequence(uint32_t i) const {
        const uint8_t *rec = bam + starts[i];
        return rec + kHead + rec[12] + 4u * rd16(rec + 16);
    }
    __device__ static uint8_t byte(const uint8_t *seq, uint32_t j) { return base_at(seq, j); }
};

// device arrays of one conversion beside those of every reads text: a start per record; the segments' walks
struct BamWork {
    TextWork<BamResult> text;
    uint32_t *d_starts = nullptr;
    Seg *d_segs = nullptr;
    unsigned long long *d_entry = nullptr;
    uint32_t *d_base = nullptr;
    uint64_t cap_starts = 0, cap_segs = 0, cap_entry = 0, cap_base = 0;   // bytes
    int reserve(uint64_t len) {
        const uint64_t records = len / kHead + 1;
        if (grow(reinterpret_cast<void **>(&d_segs), &cap_segs, kMaxSegs * sizeof(Seg)) != BT_OK || grow(reinterpret_cast<void **>(&d_entry), &cap_entry, kMaxSegs * 8) != BT_OK ||
            grow(reinterpret_cast<void **>(&d_base), &cap_base, kMaxSegs * 4) != BT_OK || grow(reinterpret_cast<void **>(&d_starts), &cap_starts, records * 4) != BT_OK)
            return BT_ERR;
        return text.reserve(records);
    }
    ~BamWork() { release(d_starts, d_segs, d_entry, d_base); }
};

std::string record_error(uint64_t offset, uint32_t e) { return "BAM record at offset " + std::to_string(offset) + ": " + record_error_text(e); }

// d_bam [len] -> d_text; complete on return.  stream_offset: where d_bam[0] lies in the decompressed stream, for messages.
int bam_text_run(const char *who, bt_ctx *ctx, BamWork &w, const uint8_t *d_bam, uint64_t len, uint32_t skip_flags, char *d_text, uint64_t capacity, uint64_t stream_offset,
                 uint64_t *text_bytes, uint64_t *consumed, bt_bam_stats *stats) {
    *text_bytes = *consumed = 0;
    if (stats) *stats = bt_bam_stats{0, 0, 0};
    if (len < 4) return BT_OK;
    if (len >= 0xFFFFFFFFull) return fail(std::string(who) + ": at most 4 GiB - 2 of records per call");
    BT_HIP(hipSetDevice(ctx->device));
    BamResult r;
    if (w.reserve(len) != BT_OK || w.text.start(ctx, r) != BT_OK) return BT_ERR;
    BamResult *d_res = w.text.d_res;
    const uint64_t seg_len = std::max<uint64_t>(kMinSeg, (len + kMaxSegs - 1) / kMaxSegs);
    const uint32_t num_segs = (uint32_t)((len + seg_len - 1) / seg_len);
    hipLaunchKernelGGL(bam_guess_kernel, dim3(num_segs), dim3(64), 0, ctx->stream, d_bam, len, seg_len, w.d_segs);
    BT_CHECK_LAUNCH();
    hipLaunchKernelGGL(bam_stitch_kernel, dim3(1), dim3(256), 0, ctx->stream, d_bam, len, seg_len, num_segs, (const Seg *)w.d_segs, w.d_entry, w.d_base, d_res);
    BT_CHECK_LAUNCH();
    hipLaunchKernelGGL(bam_fill_kernel, dim3((num_segs + 63) / 64), dim3(64), 0, ctx->stream, d_bam, len, seg_len, num_segs, (const unsigned long long *)w.d_entry,
                       (const uint32_t *)w.d_base, w.d_starts, (uint32_t)std::min<uint64_t>(w.cap_starts / 4, 0xFFFFFFFFu), d_res);
    BT_CHECK_LAUNCH();
    if (w.text.fetch(ctx, r) != BT_OK) return BT_ERR;
    if (r.overflow) return fail(std::string(who) + ": more records than the shortest record allows");
    const uint32_t n = r.n_records;
    auto measure = [&](uint32_t nb) {
        hipLaunchKernelGGL(bam_measure_kernel, dim3(nb), dim3(kTextTile), 0, ctx->stream, d_bam, len, (const uint32_t *)w.d_starts, n, skip_flags, w.text.d_sizes, w.text.d_sums, d_res);
    };
    if (text_emit(ctx, w.text, n, measure, BamSource{d_bam, w.d_starts}, d_text, capacity, r) != BT_OK) return BT_ERR;
    if (r.err != kNoError) return fail(record_error(stream_offset + (r.err >> 2), (uint32_t)(r.err & 3u)));
    if (r.overflow) return capacity_error(who, capacity, r.text_bytes);
    *text_bytes = r.text_bytes;
    *consumed = r.consumed;
    if (stats) *stats = bt_bam_stats{r.kept, n - r.kept, r.bases};
    return BT_OK;
}

// the same walk on the host (bt_bam.hpp)
int bam_text_host(const char *who, const uint8_t *bam, uint64_t len, uint32_t skip_flags, char *text, uint64_t capacity, uint64_t stream_offset, uint64_t *text_bytes, uint64_t *consumed,
                  bt_bam_stats *stats) {
    *text_bytes = *consumed = 0;
    if (stats) *stats = bt_bam_stats{0, 0, 0};
    const HostText t = reads_text_host(bam, len, skip_flags, text, capacity);
    if (t.err != kRecOk) return fail(record_error(stream_offset + t.err_offset, t.err));
    if (t.too_small) return fail(std::string(who) + ": capacity " + std::to_string(capacity) + " too small for the text");
    *text_bytes = t.text_bytes;
    *consumed = t.consumed;
    if (stats) *stats = bt_bam_stats{t.kept, t.skipped, t.bases};
    return BT_OK;
}

}  // namespace

// Slabs of whole BGZF blocks in, reads text out.  The decompressed bytes of a call land behind the tail the call before left (the record that was not whole):
// bt_bgzf_stream.hpp holds that part, which bt_fastq_scan shares.
struct bt_bam_scan {
    BgzfStream st;
    uint32_t skip_flags = 0;
    uint64_t stream_offset = 0;   // decompressed offset of d_raw[0]
    uint64_t skip_left = 0;       // header bytes still to step over
    BamWork work;
};

extern "C" {

int bt_bam_reads_text(bt_ctx *ctx, const uint8_t *d_bam, uint64_t len, uint32_t skip_flags, char *d_text, uint64_t capacity, uint64_t *text_bytes, uint64_t *consumed, bt_bam_stats *stats) {
    if (!ctx || (len && !d_bam) || (capacity && !d_text) || !text_bytes || !consumed) return fail("bt_bam_reads_text: null argument");
    BamWork w;
    return bam_text_run("bt_bam_reads_text", ctx, w, d_bam, len, skip_flags, d_text, capacity, 0, text_bytes, consumed, stats);
}

int bt_diag_bam_reads_text(const uint8_t *h_bam, uint64_t len, uint32_t skip_flags, char *h_text, uint64_t capacity, uint64_t *text_bytes, uint64_t *consumed, bt_bam_stats *stats) {
    if ((len && !h_bam) || (capacity && !h_text) || !text_bytes || !consumed) return fail("bt_diag_bam_reads_text: null argument");
    return bam_text_host("bt_diag_bam_reads_text", h_bam, len, skip_flags, h_text, capacity, 0, text_bytes, consumed, stats);
}

int bt_bam_scan_create(bt_ctx *ctx, uint64_t max_in_bytes, uint32_t skip_flags, bt_bam_scan **out) {
    if (!ctx || !out) return fail("bt_bam_scan_create: null argument");
    std::unique_ptr<bt_bam_scan> s(new bt_bam_scan);
    s->skip_flags = skip_flags;
    const int rc = s->st.create("bt_bam_scan_create", ctx, max_in_bytes);
    if (rc != BT_OK) {
        s->st.release();
        return rc;
    }
    *out = s.release();
    return BT_OK;
}

int bt_bam_scan_text(bt_bam_scan *s, const uint8_t *h_blocks, uint64_t n_bytes, uint64_t skip_first_bytes, const char **d_text, uint64_t *text_len, bt_bam_stats *stats) {
    const char *who = "bt_bam_scan_text";
    if (!s || (n_bytes && !h_blocks) || !d_text || !text_len) return fail("bt_bam_scan_text: null argument");
    *d_text = nullptr;
    *text_len = 0;
    if (stats) *stats = bt_bam_stats{0, 0, 0};
    BgzfStream &st = s->st;
    if (n_bytes > st.max_in_bytes) return fail("bt_bam_scan_text: " + std::to_string(n_bytes) + " bytes handed in, the stream was created for " + std::to_string(st.max_in_bytes));
    if (skip_first_bytes && st.calls) return fail("bt_bam_scan_text: skip_first_bytes belongs to the first call");
    bt_ctx *ctx = st.ctx;
    BT_HIP(hipSetDevice(ctx->device));
    if (!st.calls) s->skip_left = skip_first_bytes;
    uint64_t raw = 0;
    if (st.inflate_slab(who, h_blocks, n_bytes, &raw) != BT_OK) return BT_ERR;
    // the header's bytes are stepped over; they never meet a tail, since no record precedes them
    const uint64_t skip = std::min(s->skip_left, raw);
    s->skip_left -= skip;
    uint64_t consumed = 0;
    const uint8_t *d_records = st.d_raw + skip;
    if (bam_text_run(who, ctx, s->work, d_records, raw - skip, s->skip_flags, st.d_text, st.cap_text, s->stream_offset + skip, text_len, &consumed, stats) != BT_OK) return BT_ERR;
    // what is left is the start of a record that is not whole: it waits in d_tail for the next call
    const uint64_t rest = raw - skip - consumed;
    s->stream_offset += skip + consumed;
    if (rest >= 4) {
        uint8_t head[4];
        BT_HIP(hipMemcpyAsync(head, d_records + consumed, 4, hipMemcpyDeviceToHost, ctx->stream));
        BT_HIP(hipStreamSynchronize(ctx->stream));
        const uint64_t record = 4ull + rd32(head), limit = 8 * st.max_in_bytes;
        if (record > limit)
            return fail("bt_bam_scan_text: the BAM record at offset " + std::to_string(s->stream_offset) + " takes " + std::to_string(record) + " bytes, more than a slab may hold (" +
                        std::to_string(limit) + ", 8 x max_in_bytes)");
    }
    if (st.keep_tail(d_records + consumed, rest) != BT_OK) return BT_ERR;
    *d_text = st.d_text;
    return BT_OK;
}

int bt_bam_scan_finish(bt_bam_scan *s) {
    if (!s) return fail("bt_bam_scan_finish: null argument");
    if (s->skip_left) return fail("bt_bam_scan_finish: the file ends inside the BAM header (" + std::to_string(s->skip_left) + " bytes missing): truncated");
    if (s->st.tail)
        return fail("bt_bam_scan_finish: the file ends inside the BAM record at offset " + std::to_string(s->stream_offset) + " (" + std::to_string(s->st.tail) + " bytes of it are there): truncated");
    return BT_OK;
}

void bt_bam_scan_destroy(bt_bam_scan *s) {
    if (!s) return;
    s->st.release();
    delete s;
}

}  // extern "C"
