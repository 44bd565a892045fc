// libbtgpu: BGZF read on the device (bt_bgzf_inflate), the host's block scan (bt_bgzf_scan_blocks) and the host run of the same decoder
// (bt_diag_bgzf_inflate).  The block's code is bt_inflate.hpp, one text for both.  What `samtools fastq` + zlib do on host threads before a BAM sample's
// reads reach the reads route.
//
// bgzf_inflate_kernel: one 64-thread workgroup = one wavefront per BGZF block (inflate_block<WaveTeam>): 5.6 KiB of LDS for the decode tables and the
//   CRC table.  Blocks are independent; no workgroup waits on another.  A block's status goes to status[block]; the smallest failing block index to
//   status[n_blocks] (one atomic minimum per failing block), which is all the host reads back when every block is sound.
#include <algorithm>
#include <cstring>
#include <memory>

#include "bt_bgzf_stream.hpp"
#include "bt_inflate.hpp"
#include "bt_internal.hpp"

using namespace bt;
using namespace btinflate;

namespace {

__host__ __device__ inline bool entry_in_range(const bt_bgzf_block &e, uint64_t in_bytes, uint64_t out_bytes) {
    return e.in_size >= btbgzf::kFrame && e.in_size <= btbgzf::kBlockMax && e.in_offset <= in_bytes && e.in_size <= in_bytes - e.in_offset && e.isize <= kMaxIsize && e.out_offset <= out_bytes &&
           e.isize <= out_bytes - e.out_offset;
}

__global__ __launch_bounds__(64) void bgzf_inflate_kernel(const uint8_t *__restrict__ in, uint64_t in_bytes, const bt_bgzf_block *__restrict__ table, uint32_t n_blocks, uint8_t *out,
                                                          uint64_t out_bytes, uint32_t *__restrict__ status) {
    __shared__ Shared sh;
    __shared__ btbgzf::CrcShared cs;
    for (uint32_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const bt_bgzf_block e = table[b];
        const uint32_t st = entry_in_range(e, in_bytes, out_bytes) ? inflate_block<WaveTeam>(sh, cs, in + e.in_offset, e.in_size, out + e.out_offset, e.isize) : (uint32_t)kBadTable;
        if (threadIdx.x == 0) {
            status[b] = st;
            if (st != kOk) atomicMin(&status[n_blocks], b);
        }
        __syncthreads();
    }
}

std::string block_error(uint64_t offset, uint32_t st) { return "BGZF block at offset " + std::to_string(offset) + ": " + status_text(st); }

}  // namespace

namespace bt {

int bgzf_inflate_launch(bt_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes, const bt_bgzf_block *d_blocks, uint64_t n_blocks, uint8_t *d_out, uint64_t out_bytes, uint32_t *d_status) {
    if (n_blocks >= 0xFFFFFFFFull) return fail("bgzf inflate: too many blocks in one call");
    BT_HIP(hipMemsetAsync(d_status + n_blocks, 0xFF, 4, ctx->stream));
    if (!n_blocks) return BT_OK;
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned)std::min<uint64_t>(n_blocks, 1u << 20)), dim3(64), 0, ctx->stream, d_in, in_bytes, d_blocks, (uint32_t)n_blocks, d_out, out_bytes, d_status);
    BT_CHECK_LAUNCH();
    return BT_OK;
}

int bgzf_inflate_result(bt_ctx *ctx, const bt_bgzf_block *d_blocks, uint64_t n_blocks, const uint32_t *d_status, uint64_t file_offset) {
    uint32_t bad = 0xFFFFFFFFu, st = kOk;
    BT_HIP(hipMemcpyAsync(&bad, d_status + n_blocks, 4, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipStreamSynchronize(ctx->stream));
    if (bad == 0xFFFFFFFFu) return BT_OK;
    if (bad >= n_blocks) return fail("bgzf inflate: the status words are damaged");
    bt_bgzf_block e;
    BT_HIP(hipMemcpyAsync(&st, d_status + bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipMemcpyAsync(&e, d_blocks + bad, sizeof e, hipMemcpyDeviceToHost, ctx->stream));
    BT_HIP(hipStreamSynchronize(ctx->stream));
    return fail(block_error(file_offset + e.in_offset, st));
}


// ---- the stream objects' common part (bt_bgzf_stream.hpp) ---------------------------------------------------------------------------------------------------
int grow(void **p, uint64_t *cap, uint64_t need) {
    if (need <= *cap) return BT_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const uint64_t bytes = need + need / 4 + 256;
    BT_HIP(hipMalloc(p, bytes));
    *cap = bytes;
    return BT_OK;
}

int BgzfStream::create(const char *who, bt_ctx *c, uint64_t max_in) {
    if (max_in < 65536 || max_in > (1ull << 30)) return fail(std::string(who) + ": max_in_bytes must lie in 64 KiB .. 1 GiB (a slab holds at least one whole BGZF block)");
    BT_HIP(hipSetDevice(c->device));
    ctx = c;
    max_in_bytes = max_in;
    const size_t need = (size_t)(max_in + 15) / 16 * 16;
    if (c->kmc_stage_bytes >= need && c->kmc_pin[0] && c->kmc_pin[1] && c->kmc_dev[0] && c->kmc_dev[1]) {
        stage_bytes = c->kmc_stage_bytes;
        for (int b = 0; b < 2; ++b) {
            pin[b] = c->kmc_pin[b];
            dev[b] = c->kmc_dev[b];
            c->kmc_pin[b] = c->kmc_dev[b] = nullptr;
        }
        c->kmc_stage_bytes = 0;
    } else {
        stage_bytes = need;
        // one slot: a call is complete on return, so no transfer overlaps the kernels of the call before (the context's slots come as a pair and go back as one)
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&pin[0]), need, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&dev[0]), need + 16);
        if (e != hipSuccess) return fail(std::string(who) + ": " + hipGetErrorString(e));
    }
    return BT_OK;
}

int BgzfStream::inflate_slab(const char *who, const uint8_t *h_blocks, uint64_t n_bytes, uint64_t *raw_out) {
    const std::string name(who);
    // the blocks of the slab
    uint64_t n_blocks = 0, taken = 0, total = 0;
    if (bt_bgzf_scan_blocks(h_blocks, n_bytes, nullptr, 0, &n_blocks, &taken, &total) != BT_OK) return BT_ERR;
    if (taken != n_bytes) return fail(name + ": the slab ends inside the BGZF block at offset " + std::to_string(file_offset + taken) + " (whole blocks are handed in)");
    blocks.resize(n_blocks);
    if (bt_bgzf_scan_blocks(h_blocks, n_bytes, blocks.data(), n_blocks, &n_blocks, &taken, &total) != BT_OK) return BT_ERR;
    const int b = 0;   // (one slot: nothing of this call overlaps the next)
    ++calls;
    if (n_blocks > cap_blocks) {
        if (d_blocks) (void)hipFree(d_blocks);
        if (d_status) (void)hipFree(d_status);
        d_blocks = nullptr;
        d_status = nullptr;
        cap_blocks = 0;
        const uint64_t cap = n_blocks + n_blocks / 4 + 64;
        BT_HIP(hipMalloc(reinterpret_cast<void **>(&d_blocks), cap * sizeof(bt_bgzf_block)));
        BT_HIP(hipMalloc(reinterpret_cast<void **>(&d_status), (cap + 1) * 4));
        cap_blocks = cap;
    }
    const uint64_t raw = tail + total;
    if (raw >= 0xFFFFFFFFull)
        return fail(name + ": the slab at offset " + std::to_string(file_offset) + " inflates to " + std::to_string(total) + " bytes (" + std::to_string(tail) +
                    " carried over): 4 GiB - 2 of records is the most a call takes; hand in smaller slabs");
    if (grow(reinterpret_cast<void **>(&d_raw), &cap_raw, raw) != BT_OK) return BT_ERR;
    if (grow(reinterpret_cast<void **>(&d_text), &cap_text, raw) != BT_OK) return BT_ERR;
    // through the pinned slot to the device, the tail in front, the blocks' data behind it
    if (n_bytes) {
        std::memcpy(pin[b], h_blocks, n_bytes);
        BT_HIP(hipMemcpyAsync(dev[b], pin[b], n_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    if (n_blocks) BT_HIP(hipMemcpyAsync(d_blocks, blocks.data(), n_blocks * sizeof(bt_bgzf_block), hipMemcpyHostToDevice, ctx->stream));
    if (tail) BT_HIP(hipMemcpyAsync(d_raw, d_tail, tail, hipMemcpyDeviceToDevice, ctx->stream));
    if (n_blocks) {
        if (bgzf_inflate_launch(ctx, dev[b], n_bytes, d_blocks, n_blocks, d_raw + tail, total, d_status) != BT_OK) return BT_ERR;
        if (bgzf_inflate_result(ctx, d_blocks, n_blocks, d_status, file_offset) != BT_OK) return BT_ERR;
    }
    BT_HIP(hipStreamSynchronize(ctx->stream));   // (the blocks' table and the pinned slot have been read)
    file_offset += n_bytes;
    *raw_out = raw;
    return BT_OK;
}

int BgzfStream::keep_tail(const uint8_t *from, uint64_t rest) {
    if (rest) {
        if (grow(reinterpret_cast<void **>(&d_tail), &cap_tail, rest) != BT_OK) return BT_ERR;
        BT_HIP(hipMemcpyAsync(d_tail, from, rest, hipMemcpyDeviceToDevice, ctx->stream));
        BT_HIP(hipStreamSynchronize(ctx->stream));
    }
    tail = rest;
    return BT_OK;
}

void BgzfStream::release() {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    const bool whole = pin[0] && pin[1] && dev[0] && dev[1];
    if (whole && stage_bytes >= ctx->kmc_stage_bytes && !ctx_caches_off()) {
        for (int b = 0; b < 2; ++b) {
            if (ctx->kmc_pin[b]) (void)hipHostFree(ctx->kmc_pin[b]);
            if (ctx->kmc_dev[b]) (void)hipFree(ctx->kmc_dev[b]);
            ctx->kmc_pin[b] = pin[b];
            ctx->kmc_dev[b] = dev[b];
        }
        ctx->kmc_stage_bytes = stage_bytes;
    } else
        for (int b = 0; b < 2; ++b) {
            if (pin[b]) (void)hipHostFree(pin[b]);
            if (dev[b]) (void)hipFree(dev[b]);
        }
    for (void *p : {(void *)d_blocks, (void *)d_status, (void *)d_raw, (void *)d_tail, (void *)d_text})
        if (p) (void)hipFree(p);
    pin[0] = pin[1] = dev[0] = dev[1] = nullptr;
    d_blocks = nullptr, d_status = nullptr, d_raw = d_tail = nullptr, d_text = nullptr;
    ctx = nullptr;
}
}  // namespace bt

extern "C" {

int bt_bgzf_scan_blocks(const uint8_t *h_in, uint64_t n, bt_bgzf_block *h_blocks, uint64_t blocks_capacity, uint64_t *n_blocks, uint64_t *consumed, uint64_t *out_bytes) {
    if ((n && !h_in) || !n_blocks || !consumed || !out_bytes) return fail("bt_bgzf_scan_blocks: null argument");
    uint64_t at = 0, blocks = 0, total = 0;
    while (n - at >= 12 && (!h_blocks || blocks < blocks_capacity)) {
        uint32_t bsize = 0;
        const uint8_t *p = h_in + at;
        // the fixed bytes can be judged as soon as they are there; the extra field only once it is whole
        if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return fail("bt_bgzf_scan_blocks: block at offset " + std::to_string(at) + ": not a BGZF header (magic, CM, FLG.FEXTRA)");
        const uint64_t xlen = p[10] | ((uint32_t)p[11] << 8);
        if (12 + xlen > n - at) break;
        const uint32_t payload_at = parse_header(p, n - at, &bsize);
        if (!payload_at) return fail("bt_bgzf_scan_blocks: block at offset " + std::to_string(at) + ": no BC subfield of two bytes in the extra field");
        const uint64_t size = (uint64_t)bsize + 1;
        if (size < payload_at + btbgzf::kTrailer) return fail("bt_bgzf_scan_blocks: block at offset " + std::to_string(at) + ": BSIZE smaller than the block's own header and trailer");
        if (size > n - at) break;
        const uint32_t isize = load32(p + size - 4);
        if (isize > kMaxIsize) return fail("bt_bgzf_scan_blocks: block at offset " + std::to_string(at) + ": ISIZE above 65536");
        if (h_blocks) h_blocks[blocks] = bt_bgzf_block{at, total, (uint32_t)size, isize};
        ++blocks;
        total += isize;
        at += size;
    }
    *n_blocks = blocks;
    *consumed = at;
    *out_bytes = total;
    return BT_OK;
}

int bt_bgzf_inflate(bt_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes, const bt_bgzf_block *d_blocks, uint64_t n_blocks, uint8_t *d_out, uint64_t capacity, uint64_t out_bytes,
                    uint64_t file_offset) {
    if (!ctx || (n_blocks && (!d_in || !d_blocks)) || (out_bytes && !d_out)) return fail("bt_bgzf_inflate: null argument");
    if (capacity < out_bytes) return fail("bt_bgzf_inflate: capacity " + std::to_string(capacity) + " below the block table's total of " + std::to_string(out_bytes));
    BT_HIP(hipSetDevice(ctx->device));
    uint32_t *d_status = nullptr;
    BT_HIP(hipMalloc(reinterpret_cast<void **>(&d_status), (n_blocks + 1) * 4));
    int rc = bgzf_inflate_launch(ctx, d_in, in_bytes, d_blocks, n_blocks, d_out, out_bytes, d_status);
    if (rc == BT_OK) rc = bgzf_inflate_result(ctx, d_blocks, n_blocks, d_status, file_offset);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_status);
    return rc;
}

int bt_diag_bgzf_inflate(const uint8_t *h_in, uint64_t in_bytes, const bt_bgzf_block *h_blocks, uint64_t n_blocks, uint8_t *h_out, uint64_t capacity, uint64_t out_bytes, uint64_t file_offset) {
    if ((n_blocks && (!h_in || !h_blocks)) || (out_bytes && !h_out)) return fail("bt_diag_bgzf_inflate: null argument");
    if (capacity < out_bytes) return fail("bt_diag_bgzf_inflate: capacity " + std::to_string(capacity) + " below the block table's total of " + std::to_string(out_bytes));
    std::unique_ptr<Shared> sh(new Shared);
    std::unique_ptr<btbgzf::CrcShared> cs(new btbgzf::CrcShared);
    uint64_t bad = n_blocks;
    uint32_t bad_status = kOk;
    for (uint64_t b = 0; b < n_blocks; ++b) {   // every block is run, as on the device: a failing block leaves the others' data intact
        const bt_bgzf_block &e = h_blocks[b];
        const uint32_t st = entry_in_range(e, in_bytes, out_bytes) ? inflate_block<LaneTeam>(*sh, *cs, h_in + e.in_offset, e.in_size, h_out + e.out_offset, e.isize) : (uint32_t)kBadTable;
        if (st != kOk && bad == n_blocks) bad = b, bad_status = st;
    }
    if (bad != n_blocks) return fail(block_error(file_offset + h_blocks[bad].in_offset, bad_status));
    return BT_OK;
}

}  // extern "C"
