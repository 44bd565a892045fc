// libbtgpu: a BGZF-compressed FASTQ sample's reads as the reads text of bt_reads.hip, on the device.
//   bt_fastq_reads_text      inflated FASTQ text -> "<bases>\n" per record with bases (bt_fastq.hpp holds the grammar, one text for kernels and host)
//   bt_fastq_scan_*          the stream object: slabs of whole BGZF blocks from the host -> inflate (bt_bgzf_stream.hpp) behind the carried tail -> text
//   bt_diag_fastq_reads_text the host run of the same line code
// What zlib and ReadsFile do on one host thread per file before the reads of a .fastq.gz written by bgzip or a sequencer's converter reach the reads route.
//
// Which of a record's four lines a line is depends on the blank lines before it; every newline carries a function on the four phases (bt_fastq.hpp), and
// the phases come out of a scan over them.  No workgroup waits on another: the kernels follow each other on the stream.
//   fastq_tiles_kernel<false>  a workgroup per tile of kCountTile bytes, 16 consecutive bytes per thread: the tile's newlines and composed function
//   fastq_scan_kernel          one workgroup: exclusive scan over the tiles' summaries; the number of lines, the phase the data ends in
//   fastq_tiles_kernel<true>   the same walk again: every newline stores its position at its line index, with the phase its line is entered in
//   fastq_measure_kernel       a thread per line: the line judged (judge_line); for the sequence line of a whole record bases + 1 into sizes[], a sum per workgroup
// From sizes[] on the work is that of every reads text and is written once, in bt_reads_text.hpp (which bt_bam.hip shares), as is the LDS scan of the kernels above:
//   text_offsets_kernel            one workgroup: exclusive scan over the workgroups' sums, the text's length
//   text_emit_kernel<FastqSource>  a workgroup per 256 lines rebuilds its lines' offsets from sizes[]; a wavefront per read, a lane per base: 64 consecutive
//                                  bytes per load and per store instruction
// The first violation is the one at the smallest line: a 64-bit atomic minimum over line << 2 | condition.
#include <algorithm>
#include <memory>

#include "bt_bgzf_stream.hpp"
#include "bt_fastq.hpp"
#include "bt_fastq_stream.hpp"
#include "bt_internal.hpp"
#include "bt_reads_text.hpp"

using namespace bt;
using namespace btfastq;

namespace {

constexpr uint32_t kBytesPerThread = 16, kCountTile = 256 * kBytesPerThread;   // bytes per workgroup of the tiles kernels

struct FastqResult : TextResult {   // err: (line index + 1) << 2 | condition of the first violation; kept: the reads
    uint32_t newlines, n_lines, end_phase, open_phase;   // n_lines: newlines + 1 when the data's last line has none and counts; open_phase: the phase that line is entered in
    uint32_t whole_lines;                                // lines of whole records and skipped blank lines
};

// What a stretch of bytes does to the line finding: its newlines, and their functions composed in byte order
struct LineSum {
    uint32_t count, fn;
};
struct JoinLines {
    __device__ LineSum operator()(LineSum earlier, LineSum later) const { return LineSum{earlier.count + later.count, compose(earlier.fn, later.fn)}; }
};

// The 16 bytes of a thread, and the summary of their newlines.  Bytes at and past len read as 0 (no newline).
__device__ inline void load_bytes(const uint8_t *__restrict__ data, uint64_t len, uint64_t p, uint8_t (&b)[kBytesPerThread]) {
    if (p + kBytesPerThread <= len)
        __builtin_memcpy(b, data + p, kBytesPerThread);
    else
        for (uint32_t j = 0; j < kBytesPerThread; ++j) b[j] = p + j < len ? data[p + j] : 0;
}

template <bool kStore>
__global__ __launch_bounds__(256) void fastq_tiles_kernel(const uint8_t *__restrict__ data, uint64_t len, uint32_t *__restrict__ tile_lines, uint8_t *__restrict__ tile_fn,
                                                          uint32_t *__restrict__ ends, uint8_t *__restrict__ phases, uint32_t n_lines, const FastqResult *__restrict__ res) {
    __shared__ LineSum s[256];
    const uint64_t p = (uint64_t)blockIdx.x * kCountTile + (uint64_t)threadIdx.x * kBytesPerThread;
    uint8_t b[kBytesPerThread];
    uint8_t before1 = 0, before2 = 0;
    uint32_t count = 0, fn = kIdentity;
    if (p < len) {
        load_bytes(data, len, p, b);
        if (p >= 1) before1 = data[p - 1];
        if (p >= 2) before2 = data[p - 2];
        uint8_t b1 = before1, b2 = before2;
        for (uint32_t j = 0; j < kBytesPerThread; ++j) {
            if (b[j] == '\n') {   // (bytes past len are 0)
                ++count;
                fn = compose(fn, newline_fn(p + j, b1, b2));
            }
            b2 = b1;
            b1 = b[j];
        }
    }
    scan256(s, LineSum{count, fn}, LineSum{0, kIdentity}, JoinLines());
    if (!kStore) {
        if (threadIdx.x == 255) {
            tile_lines[blockIdx.x] = s[255].count;
            tile_fn[blockIdx.x] = (uint8_t)s[255].fn;
        }
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && n_lines > res->newlines) {   // the last line, which has no newline
        ends[n_lines - 1] = (uint32_t)len;
        phases[n_lines - 1] = (uint8_t)res->open_phase;
    }
    if (!count) return;
    uint32_t line = tile_lines[blockIdx.x] + s[threadIdx.x].count - count;
    uint32_t phase = apply(tile_fn[blockIdx.x], 0);
    if (threadIdx.x) phase = apply(s[threadIdx.x - 1].fn, phase);
    uint8_t b1 = before1, b2 = before2;
    for (uint32_t j = 0; j < kBytesPerThread; ++j) {
        if (b[j] == '\n') {
            if (line < n_lines) {   // (always: n_lines counts these newlines)
                ends[line] = (uint32_t)(p + j);
                phases[line] = (uint8_t)phase;
            }
            phase = apply(newline_fn(p + j, b1, b2), phase);
            ++line;
        }
        b2 = b1;
        b1 = b[j];
    }
}

// tile_lines[0..nt), tile_fn[0..nt) -> exclusive prefixes in place; the totals into res.  final: the data's last line counts when it has no newline.
__global__ __launch_bounds__(256) void fastq_scan_kernel(const uint8_t *__restrict__ data, uint64_t len, int final, uint32_t *tile_lines, uint8_t *tile_fn, uint32_t nt, FastqResult *res) {
    __shared__ LineSum s[256];
    uint32_t carry_count = 0, carry_fn = kIdentity;
    for (uint32_t base = 0; base < nt; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < nt ? tile_lines[i] : 0, f = i < nt ? tile_fn[i] : kIdentity;
        scan256(s, LineSum{c, f}, LineSum{0, kIdentity}, JoinLines());
        if (i < nt) {
            tile_lines[i] = carry_count + s[threadIdx.x].count - c;
            tile_fn[i] = (uint8_t)compose(carry_fn, threadIdx.x ? s[threadIdx.x - 1].fn : kIdentity);
        }
        carry_count += s[255].count;
        carry_fn = compose(carry_fn, s[255].fn);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool open = final && len && data[len - 1] != '\n';
        uint32_t phase = apply(carry_fn, 0);
        res->newlines = carry_count;
        res->open_phase = phase;
        if (open) phase = apply(kAdvance, phase);
        res->n_lines = carry_count + (open ? 1u : 0u);
        res->end_phase = phase;
        res->whole_lines = res->n_lines - phase;   // the record under way holds as many lines as the phase says: inside a record every line advances it
    }
}

__global__ __launch_bounds__(kTextTile) void fastq_measure_kernel(const uint8_t *__restrict__ data, uint64_t len, const uint32_t *__restrict__ ends, const uint8_t *__restrict__ phases,
                                                                  uint32_t *__restrict__ sizes, unsigned long long *__restrict__ sums, FastqResult *res) {
    const uint32_t n = res->n_lines, whole = res->whole_lines, i = blockIdx.x * kTextTile + threadIdx.x;
    uint32_t size = 0;
    if (i < n) {
        const uint64_t start = i ? (uint64_t)ends[i - 1] + 1 : 0, end = ends[i];
        const uint32_t phase = phases[i];
        // a quality line has its record's three other lines before it in the data, which start at a record boundary
        uint64_t seq_start = 0, seq_end = 0;
        if (phase == 3 && i >= 2) seq_start = i >= 3 ? (uint64_t)ends[i - 3] + 1 : 0, seq_end = ends[i - 2];
        const Line l = judge_line(data, start, end, phase, i + 1 == n && n > res->newlines, seq_start, seq_end);
        if (l.verdict != kLineOk) atomicMin(&res->err, ((unsigned long long)i + 1) << 2 | l.verdict);
        size = l.bases && i < whole ? l.bases + 1 : 0;
        sizes[i] = size;
        if (i + 1 == whole) res->consumed = std::min<uint64_t>(end + 1, len);
    }
    tally_sizes(size, sums, res);
}

// text_emit_kernel's view of the lines: a line starts behind the end of the line before it, and its bytes are the text's
struct FastqSource {
    const uint8_t *__restrict__ data;
    const uint32_t *__restrict__ ends;
    __device__ const uint8_t *sequence(uint32_t line) const { return data + (line ? (uint64_t)ends[line - 1] + 1 : 0); }   // (a sequence line is never the data's first line)
    __device__ static uint8_t byte(const uint8_t *seq, uint32_t j) { return seq[j]; }
};

// device arrays of one conversion beside those of every reads text: a count and a function per tile of bytes; an end and a phase per line
struct FastqWork {
    TextWork<FastqResult> text;
    uint32_t *d_tile_lines = nullptr, *d_ends = nullptr;
    uint8_t *d_tile_fn = nullptr, *d_phases = nullptr;
    uint64_t cap_tile_lines = 0, cap_tile_fn = 0, cap_ends = 0, cap_phases = 0;   // bytes
    int reserve_tiles(uint64_t tiles) {
        if (grow(reinterpret_cast<void **>(&d_tile_lines), &cap_tile_lines, tiles * 4) != BT_OK) return BT_ERR;
        return grow(reinterpret_cast<void **>(&d_tile_fn), &cap_tile_fn, tiles);
    }
    int reserve_lines(uint64_t lines) {
        if (grow(reinterpret_cast<void **>(&d_ends), &cap_ends, lines * 4) != BT_OK || grow(reinterpret_cast<void **>(&d_phases), &cap_phases, lines) != BT_OK) return BT_ERR;
        return text.reserve(lines);
    }
    ~FastqWork() { release(d_tile_lines, d_tile_fn, d_ends, d_phases); }
};

// the bases and quality values of the record whose quality line is line `i` (0-based), for the message: read back from the device
int lengths_of(bt_ctx *ctx, const FastqWork &w, const uint8_t *d_data, uint64_t i, uint64_t *bases, uint64_t *quals) {
    uint32_t e[4] = {0, 0, 0, 0};   // ends of the lines i - 3 .. i
    const uint64_t from = i >= 3 ? i - 3 : 0, count = i - from + 1;
    BT_HIP(hipMemcpyAsync(e + (4 - count), w.d_ends + from, count * 4, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipStreamSynchronize(ctx->stream));
    const uint64_t span[2][2] = {{i >= 3 ? (uint64_t)e[0] + 1 : 0, e[1]}, {(uint64_t)e[2] + 1, e[3]}};
    uint64_t n[2];
    for (int k = 0; k < 2; ++k) {
        n[k] = span[k][1] - span[k][0];
        if (n[k]) {
            uint8_t last = 0;
            BT_HIP(hipMemcpyAsync(&last, d_data + span[k][1] - 1, 1, hipMemcpyDeviceToHost, ctx->stream));
            BT_HIP(hipStreamSynchronize(ctx->stream));
            if (last == '\r') --n[k];
        }
    }
    *bases = n[0];
    *quals = n[1];
    return BT_OK;
}

// d_data [len] -> d_text; complete on return
int fastq_text_run(const char *who, bt_ctx *ctx, FastqWork &w, const uint8_t *d_data, uint64_t len, int final, uint64_t first_line, char *d_text, uint64_t capacity, uint64_t *text_bytes,
                   uint64_t *consumed, bt_fastq_stats *stats) {
    *text_bytes = *consumed = 0;
    if (stats) *stats = bt_fastq_stats{0, 0, 0};
    if (!len) return BT_OK;
    if (len >= 0xFFFFFFFFull) return fail(std::string(who) + ": at most 4 GiB - 2 of text per call");
    BT_HIP(hipSetDevice(ctx->device));
    const uint32_t nt = (uint32_t)((len + kCountTile - 1) / kCountTile);
    FastqResult r;
    if (w.reserve_tiles(nt) != BT_OK || w.text.start(ctx, r) != BT_OK) return BT_ERR;
    FastqResult *d_res = w.text.d_res;
    hipLaunchKernelGGL(fastq_tiles_kernel<false>, dim3(nt), dim3(256), 0, ctx->stream, d_data, len, w.d_tile_lines, w.d_tile_fn, (uint32_t *)nullptr, (uint8_t *)nullptr, 0u,
                       (const FastqResult *)d_res);
    BT_CHECK_LAUNCH();
    hipLaunchKernelGGL(fastq_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, d_data, len, final, w.d_tile_lines, w.d_tile_fn, nt, d_res);
    BT_CHECK_LAUNCH();
    if (w.text.fetch(ctx, r) != BT_OK) return BT_ERR;
    const uint32_t n = r.n_lines;
    if (n) {
        if (w.reserve_lines(n) != BT_OK) return BT_ERR;
        hipLaunchKernelGGL(fastq_tiles_kernel<true>, dim3(nt), dim3(256), 0, ctx->stream, d_data, len, w.d_tile_lines, w.d_tile_fn, w.d_ends, w.d_phases, n, (const FastqResult *)d_res);
        BT_CHECK_LAUNCH();
    }
    auto measure = [&](uint32_t nb) {
        hipLaunchKernelGGL(fastq_measure_kernel, dim3(nb), dim3(kTextTile), 0, ctx->stream, d_data, len, (const uint32_t *)w.d_ends, (const uint8_t *)w.d_phases, w.text.d_sizes, w.text.d_sums, d_res);
    };
    if (text_emit(ctx, w.text, n, measure, FastqSource{d_data, w.d_ends}, d_text, capacity, r) != BT_OK) return BT_ERR;
    if (r.err != kNoError) {
        const uint64_t line = (r.err >> 2) - 1;
        const uint32_t verdict = (uint32_t)(r.err & 3u);
        uint64_t bases = 0, quals = 0;
        if (verdict == kLengths && lengths_of(ctx, w, d_data, line, &bases, &quals) != BT_OK) return BT_ERR;
        return fail(error_text(verdict, first_line + line, bases, quals, 0));
    }
    if (final && r.end_phase) return fail(error_text(kTruncated, 0, 0, 0, r.end_phase));
    if (r.overflow) return capacity_error(who, capacity, r.text_bytes);
    *text_bytes = r.text_bytes;
    *consumed = r.consumed;
    if (stats) *stats = bt_fastq_stats{r.kept, r.bases, r.whole_lines};
    return BT_OK;
}

// the same walk on the host (bt_fastq.hpp)
int fastq_text_host(const char *who, const uint8_t *data, uint64_t len, int final, uint64_t first_line, char *text, uint64_t capacity, uint64_t *text_bytes, uint64_t *consumed,
                    bt_fastq_stats *stats) {
    *text_bytes = *consumed = 0;
    if (stats) *stats = bt_fastq_stats{0, 0, 0};
    if (len >= 0xFFFFFFFFull) return fail(std::string(who) + ": at most 4 GiB - 2 of text per call");
    const HostText t = reads_text_host(data, len, final != 0, text, capacity);
    if (t.verdict != kLineOk) return fail(error_text(t.verdict, first_line + t.err_line, t.err_bases, t.err_quals, t.lines_of_four));
    if (t.too_small) return fail(std::string(who) + ": capacity " + std::to_string(capacity) + " too small for the text");
    *text_bytes = t.text_bytes;
    *consumed = t.consumed;
    if (stats) *stats = bt_fastq_stats{t.reads, t.bases, t.lines};
    return BT_OK;
}

}  // namespace

// The raw-to-text-and-tail half of a FASTQ stream object (bt_fastq_stream.hpp), whatever inflated the data: bt_fastq_scan (BGZF) and bt_fastq_gz_scan
// (one long gzip member, bt_gunzip.hip).
struct bt::FastqText {
    uint64_t line = 1;            // the file's line number of d_raw[0]
    uint64_t stream_offset = 0;   // decompressed offset of d_raw[0]
    FastqWork work;
};

namespace bt {

FastqText *fastq_text_create() { return new FastqText; }
void fastq_text_destroy(FastqText *ft) { delete ft; }

int fastq_text_slab(const char *who, BgzfStream &st, FastqText &ft, uint64_t raw, const char **d_text, uint64_t *text_len, bt_fastq_stats *stats) {
    uint64_t consumed = 0;
    bt_fastq_stats now{0, 0, 0};
    if (fastq_text_run(who, st.ctx, ft.work, st.d_raw, raw, 0, ft.line, st.d_text, st.cap_text, text_len, &consumed, &now) != BT_OK) return BT_ERR;
    if (stats) *stats = now;
    // what is left is the start of a record that is not whole: it waits in d_tail for the next call
    const uint64_t rest = raw - consumed, limit = 8 * st.max_in_bytes;
    ft.line += now.lines;
    ft.stream_offset += consumed;
    if (rest > limit)
        return fail(std::string(who) + ": the FASTQ record at line " + std::to_string(ft.line) + " (offset " + std::to_string(ft.stream_offset) + ") takes more than " + std::to_string(rest) +
                    " bytes, more than a slab may hold (" + std::to_string(limit) + ", 8 x max_in_bytes)");
    if (st.keep_tail(st.d_raw + consumed, rest) != BT_OK) return BT_ERR;
    *d_text = st.d_text;
    return BT_OK;
}

int fastq_text_finish(const char *who, BgzfStream &st, FastqText &ft, const char **d_text, uint64_t *text_len, bt_fastq_stats *stats) {
    if (!st.tail) return BT_OK;
    // the tail is the file's end: its last line needs no newline, and a record of fewer than four lines is a truncated file
    if (grow(reinterpret_cast<void **>(&st.d_text), &st.cap_text, st.tail) != BT_OK) return BT_ERR;
    uint64_t consumed = 0;
    bt_fastq_stats now{0, 0, 0};
    if (fastq_text_run(who, st.ctx, ft.work, st.d_tail, st.tail, 1, ft.line, st.d_text, st.cap_text, text_len, &consumed, &now) != BT_OK) return BT_ERR;
    if (stats) *stats = now;
    ft.line += now.lines;
    ft.stream_offset += consumed;
    st.tail = 0;
    *d_text = st.d_text;
    return BT_OK;
}

}  // namespace bt

// Slabs of whole BGZF blocks in, reads text out.  The decompressed bytes of a call land behind the tail the call before left (the record that was not whole).
struct bt_fastq_scan {
    BgzfStream st;
    FastqText ft;
};

extern "C" {

uint32_t bt_fastq_count_tile(void) { return kCountTile; }

int bt_fastq_reads_text(bt_ctx *ctx, const char *d_fastq, uint64_t len, int final, uint64_t first_line, char *d_text, uint64_t capacity, uint64_t *text_bytes, uint64_t *consumed,
                        bt_fastq_stats *stats) {
    if (!ctx || (len && !d_fastq) || (capacity && !d_text) || !text_bytes || !consumed) return fail("bt_fastq_reads_text: null argument");
    FastqWork w;
    return fastq_text_run("bt_fastq_reads_text", ctx, w, reinterpret_cast<const uint8_t *>(d_fastq), len, final, first_line, d_text, capacity, text_bytes, consumed, stats);
}

int bt_diag_fastq_reads_text(const char *h_fastq, uint64_t len, int final, uint64_t first_line, char *h_text, uint64_t capacity, uint64_t *text_bytes, uint64_t *consumed,
                             bt_fastq_stats *stats) {
    if ((len && !h_fastq) || (capacity && !h_text) || !text_bytes || !consumed) return fail("bt_diag_fastq_reads_text: null argument");
    return fastq_text_host("bt_diag_fastq_reads_text", reinterpret_cast<const uint8_t *>(h_fastq), len, final, first_line, h_text, capacity, text_bytes, consumed, stats);
}

int bt_fastq_scan_create(bt_ctx *ctx, uint64_t max_in_bytes, bt_fastq_scan **out) {
    if (!ctx || !out) return fail("bt_fastq_scan_create: null argument");
    std::unique_ptr<bt_fastq_scan> s(new bt_fastq_scan);
    const int rc = s->st.create("bt_fastq_scan_create", ctx, max_in_bytes);
    if (rc != BT_OK) {
        s->st.release();
        return rc;
    }
    *out = s.release();
    return BT_OK;
}

int bt_fastq_scan_text(bt_fastq_scan *s, const uint8_t *h_blocks, uint64_t n_bytes, const char **d_text, uint64_t *text_len, bt_fastq_stats *stats) {
    const char *who = "bt_fastq_scan_text";
    if (!s || (n_bytes && !h_blocks) || !d_text || !text_len) return fail("bt_fastq_scan_text: null argument");
    *d_text = nullptr;
    *text_len = 0;
    if (stats) *stats = bt_fastq_stats{0, 0, 0};
    BgzfStream &st = s->st;
    if (n_bytes > st.max_in_bytes) return fail("bt_fastq_scan_text: " + std::to_string(n_bytes) + " bytes handed in, the stream was created for " + std::to_string(st.max_in_bytes));
    bt_ctx *ctx = st.ctx;
    BT_HIP(hipSetDevice(ctx->device));
    uint64_t raw = 0;
    if (st.inflate_slab(who, h_blocks, n_bytes, &raw) != BT_OK) return BT_ERR;
    return fastq_text_slab(who, st, s->ft, raw, d_text, text_len, stats);
}

int bt_fastq_scan_finish(bt_fastq_scan *s, const char **d_text, uint64_t *text_len, bt_fastq_stats *stats) {
    const char *who = "bt_fastq_scan_finish";
    if (!s || !d_text || !text_len) return fail("bt_fastq_scan_finish: null argument");
    *d_text = nullptr;
    *text_len = 0;
    if (stats) *stats = bt_fastq_stats{0, 0, 0};
    BgzfStream &st = s->st;
    if (!st.tail) return BT_OK;
    BT_HIP(hipSetDevice(st.ctx->device));
    return fastq_text_finish(who, st, s->ft, d_text, text_len, stats);
}

void bt_fastq_scan_destroy(bt_fastq_scan *s) {
    if (!s) return;
    s->st.release();
    delete s;
}

}  // extern "C"
