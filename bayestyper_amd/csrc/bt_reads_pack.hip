// libbtgpu: the packed form of a reads text (bt_reads_pack.hpp) and the reads pack file (bt_reads_pack_file.hpp).
//   bt_reads_pack / bt_reads_unpack           (no counterpart: the reference reads a KMC database, never the reads)
//   bt_reads_pack_writer_* / _reader_* / bt_reads_pack_file_info   (no counterpart)
// The pack kernel is a pure map: one lane per 16-position word, one 16-byte text load, one codes word stored; the two lanes of a 32-position group combine their
// validity bits with a shuffle and the even one stores the validity word.  No two lanes store to the same word: no atomics, no LDS.
#include <cstring>
#include <new>

#include "bt_internal.hpp"
#include "bt_reads_pack.hpp"
#include "bt_reads_pack_file.hpp"

using namespace bt;

namespace {

constexpr unsigned PACK_LANES = 256;

struct alignas(16) Bytes16 {
    char b[PACK_WORD_POSITIONS];
};

// words = 8 * blocks (an even number): the two lanes of a pair sit in one wavefront, and every lane of the grid reaches the shuffle
__global__ __launch_bounds__(PACK_LANES) void reads_pack_kernel(const char *__restrict__ text, uint64_t n, uint32_t *__restrict__ packed, uint64_t words, int aligned) {
    const uint64_t w = (uint64_t)blockIdx.x * PACK_LANES + threadIdx.x, p0 = w * PACK_WORD_POSITIONS;
    const bool mine = w < words;
    uint32_t codes = 0, valid = 0;
    if (mine && p0 < n) {
        if (aligned && n - p0 >= PACK_WORD_POSITIONS) {
            const Bytes16 q = *reinterpret_cast<const Bytes16 *>(text + p0);
            pack_word(q.b, PACK_WORD_POSITIONS, &codes, &valid);
        } else {
            pack_word(text + p0, n - p0 < PACK_WORD_POSITIONS ? (unsigned)(n - p0) : PACK_WORD_POSITIONS, &codes, &valid);
        }
    }
    const uint32_t other = (uint32_t)__shfl_xor((int)valid, 1);
    if (!mine) return;
    packed[pack_codes_index(w)] = codes;
    if (!(w & 1u)) packed[pack_valid_index(w)] = valid | (other << 16);
}

__global__ __launch_bounds__(PACK_LANES) void reads_unpack_kernel(const uint32_t *__restrict__ packed, uint64_t positions, char *__restrict__ text, int aligned) {
    const uint64_t w = (uint64_t)blockIdx.x * PACK_LANES + threadIdx.x, p0 = w * PACK_WORD_POSITIONS;
    if (p0 >= positions) return;
    Bytes16 q;
    unpack_word(packed[pack_codes_index(w)], (packed[pack_valid_index(w)] >> pack_valid_shift(w)) & 0xFFFFu, q.b);
    if (aligned && positions - p0 >= PACK_WORD_POSITIONS) {
        *reinterpret_cast<Bytes16 *>(text + p0) = q;
    } else {
        for (unsigned i = 0; i < PACK_WORD_POSITIONS && p0 + i < positions; ++i) text[p0 + i] = q.b[i];
    }
}

int check_pack_args(const char *who, const void *text, uint64_t n, const void *packed) {
    if (n && (!text || !packed)) return fail(std::string(who) + ": null argument");
    if (reinterpret_cast<uintptr_t>(packed) & 3u) return fail(std::string(who) + ": the packed reads must be 4-byte aligned");
    if (n > (1ull << 48)) return fail(std::string(who) + ": more than 2^48 positions");
    return BT_OK;
}

}  // namespace

struct bt_reads_pack_writer {
    btpack::Writer w;
};
struct bt_reads_pack_reader {
    btpack::Reader r;
};

namespace {

void fill_info(const btpack::Reader &r, bt_reads_pack_info *info) {
    info->version = r.version;
    info->k = r.k;
    info->block_positions = btpack::BLOCK_POSITIONS;
    info->manifest_bytes = (uint32_t)r.manifest.size();
    info->sections = r.totals.sections;
    info->positions = r.totals.positions;
    info->bases = r.totals.bases;
    info->reads = r.totals.reads;
    info->max_section_positions = r.max_positions;
}

}  // namespace

extern "C" {

uint64_t bt_reads_packed_bytes(uint64_t positions) { return reads_packed_bytes(positions); }

int bt_reads_pack(bt_ctx *ctx, const char *d_text, uint64_t len, uint8_t *d_packed) {
    if (!ctx) return fail("bt_reads_pack: null argument");
    if (check_pack_args("bt_reads_pack", d_text, len, d_packed) != BT_OK) return BT_ERR;
    if (len == 0) return BT_OK;
    BT_HIP(hipSetDevice(ctx->device));
    const uint64_t words = reads_packed_blocks(len) * 8u;
    hipLaunchKernelGGL(reads_pack_kernel, dim3(grid_for(words, PACK_LANES)), dim3(PACK_LANES), 0, ctx->stream, d_text, len, reinterpret_cast<uint32_t *>(d_packed), words,
                       (int)((reinterpret_cast<uintptr_t>(d_text) & 15u) == 0));
    BT_CHECK_LAUNCH();
    return BT_OK;
}

int bt_reads_unpack(bt_ctx *ctx, const uint8_t *d_packed, uint64_t positions, char *d_text) {
    if (!ctx) return fail("bt_reads_unpack: null argument");
    if (check_pack_args("bt_reads_unpack", d_text, positions, d_packed) != BT_OK) return BT_ERR;
    if (positions == 0) return BT_OK;
    BT_HIP(hipSetDevice(ctx->device));
    const uint64_t words = (positions + PACK_WORD_POSITIONS - 1) / PACK_WORD_POSITIONS;
    hipLaunchKernelGGL(reads_unpack_kernel, dim3(grid_for(words, PACK_LANES)), dim3(PACK_LANES), 0, ctx->stream, reinterpret_cast<const uint32_t *>(d_packed), positions, d_text,
                       (int)((reinterpret_cast<uintptr_t>(d_text) & 15u) == 0));
    BT_CHECK_LAUNCH();
    return BT_OK;
}

int bt_diag_reads_pack(const char *h_text, uint64_t len, uint8_t *h_packed) {
    if (check_pack_args("bt_diag_reads_pack", h_text, len, h_packed) != BT_OK) return BT_ERR;
    reads_pack_host(h_text, len, reinterpret_cast<uint32_t *>(h_packed));
    return BT_OK;
}

int bt_diag_reads_unpack(const uint8_t *h_packed, uint64_t positions, char *h_text) {
    if (check_pack_args("bt_diag_reads_unpack", h_text, positions, h_packed) != BT_OK) return BT_ERR;
    reads_unpack_host(reinterpret_cast<const uint32_t *>(h_packed), positions, h_text);
    return BT_OK;
}

int bt_reads_pack_writer_create(const char *path, uint32_t k, const char *manifest, bt_reads_pack_writer **out) {
    if (!path || !out) return fail("bt_reads_pack_writer_create: null argument");
    bt_reads_pack_writer *w = new (std::nothrow) bt_reads_pack_writer;
    if (!w) return fail("bt_reads_pack_writer_create: out of memory");
    if (!w->w.open(path, k, manifest ? manifest : "")) {
        const std::string msg = w->w.error;
        delete w;
        return fail(msg);
    }
    *out = w;
    return BT_OK;
}

int bt_reads_pack_writer_add(bt_reads_pack_writer *w, const uint8_t *h_packed, uint64_t positions, uint64_t bases, uint64_t reads) {
    if (!w || (positions && !h_packed)) return fail("bt_reads_pack_writer_add: null argument");
    return w->w.section(h_packed, positions, bases, reads) ? BT_OK : fail(w->w.error);
}

int bt_reads_pack_writer_finish(bt_reads_pack_writer *w) {
    if (!w) return fail("bt_reads_pack_writer_finish: null argument");
    return w->w.finish() ? BT_OK : fail(w->w.error);
}

void bt_reads_pack_writer_destroy(bt_reads_pack_writer *w) { delete w; }

int bt_reads_pack_reader_open(const char *path, bt_reads_pack_reader **out, bt_reads_pack_info *info) {
    if (!path || !out) return fail("bt_reads_pack_reader_open: null argument");
    bt_reads_pack_reader *r = new (std::nothrow) bt_reads_pack_reader;
    if (!r) return fail("bt_reads_pack_reader_open: out of memory");
    if (!r->r.open(path)) {
        const std::string msg = r->r.error;
        delete r;
        return fail(msg);
    }
    if (info) fill_info(r->r, info);
    *out = r;
    return BT_OK;
}

int bt_reads_pack_reader_manifest(bt_reads_pack_reader *r, char *buf, uint64_t capacity, uint64_t *len) {
    if (!r || !len || (capacity && !buf)) return fail("bt_reads_pack_reader_manifest: null argument");
    *len = r->r.manifest.size();
    if (capacity < *len) return fail("bt_reads_pack_reader_manifest: buffer too small");
    if (*len) std::memcpy(buf, r->r.manifest.data(), (size_t)*len);
    return BT_OK;
}

int bt_reads_pack_reader_next(bt_reads_pack_reader *r, uint8_t *h_packed, uint64_t capacity, uint64_t *positions, uint64_t *bases, uint64_t *reads, int *end) {
    if (!r || !positions || !end || (capacity && !h_packed)) return fail("bt_reads_pack_reader_next: null argument");
    btpack::Section s;
    bool last = false;
    if (!r->r.next(h_packed, capacity, &s, &last)) return fail(r->r.error);
    *end = last ? 1 : 0;
    *positions = s.positions;
    if (bases) *bases = s.bases;
    if (reads) *reads = s.reads;
    return BT_OK;
}

void bt_reads_pack_reader_close(bt_reads_pack_reader *r) { delete r; }

int bt_reads_pack_file_info(const char *path, bt_reads_pack_info *info) {
    if (!path || !info) return fail("bt_reads_pack_file_info: null argument");
    btpack::Reader r;
    if (!r.open(path)) return fail(r.error);
    fill_info(r, info);
    return BT_OK;
}

}  // extern "C"
