// libbtgpu: BGZF on the device (bt_bgzf), BGZF files written through it (bt_bgzf_save) and the host runs of the same code (bt_diag_bgzf, bt_diag_crc32).
// The block's code is bt_bgzf.hpp over bt_deflate.hpp, one text for both.  Replaces the bgzip + tabix pass a user runs over the VCF of `genotype -z`.
//
// bgzf_block_kernel: one 64-thread workgroup = one wavefront per block of 65280 input bytes: deflate_piece as in deflate_piece_kernel, then the CRC-32 of
//   the block's input by the same wavefront while the block is still in the cache (1.25 KiB of LDS beside btdeflate::Shared).
// bgzf_frame_kernel: btgz::place_unit with framing — deflate_compact_kernel's scan over the batch's sizes, each plus the 26 bytes of framing; a workgroup
//   writes its block's header, payload, CRC-32 and length to its place and the block's offset into the offsets array.
// bgzf_end_kernel: one workgroup writes the last offset, the EOF block when asked for, and the stream's length.
// Everything behind the kernels — the scratch, the batches of a call, the slab pipeline of bt_bgzf_save, the host replay — is bt_gz_pipeline.hpp over the
// policy btgz::Bgzf, shared with bt_deflate.hip.  What is left here: the three kernels, their launches, the file's block offsets, argument checks.
#include <zlib.h>

#include <algorithm>
#include <memory>

#include "bt_gz_pipeline.hpp"

using namespace btgz;

namespace {

__global__ __launch_bounds__(64) void bgzf_block_kernel(const uint8_t *__restrict__ in, uint64_t n, uint64_t first_block, uint32_t *__restrict__ tokens, uint8_t *__restrict__ stage,
                                                        uint32_t *__restrict__ recs, uint32_t *error) {
    __shared__ Shared sh;
    __shared__ CrcShared cs;
    const uint64_t block = first_block + blockIdx.x, off = block * kBlock;
    if (off >= n) return;   // (the grid is the number of blocks: never)
    const uint32_t len = (uint32_t)std::min<uint64_t>(kBlock, n - off);
    bgzf_block<WaveTeam>(sh, cs, in + off, len, tokens + (uint64_t)blockIdx.x * kPiece, stage + (uint64_t)blockIdx.x * kPieceOut, recs + block * kBlockRecWords, error);
}

__global__ __launch_bounds__(COPY_BLOCK) void bgzf_frame_kernel(const uint8_t *__restrict__ stage, const uint32_t *__restrict__ recs, uint64_t first_block, uint32_t batch_blocks,
                                                                unsigned long long *bases, uint32_t batch, uint8_t *__restrict__ out, uint64_t capacity,
                                                                unsigned long long *__restrict__ offsets, uint32_t *error) {
    place_unit<Bgzf>(stage, recs, first_block, batch_blocks, bases, batch, out, capacity, offsets, error);
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

// what bt_bgzf_save keeps of the slabs: every block's offset in the file, and behind the last slab's the offset of the EOF block
struct FileOffsets : NoExtras {
    uint64_t *h_block_offsets = nullptr;
    uint64_t block_at = 0;
    void drained(const unsigned long long *offsets, uint64_t blocks, uint64_t file_at, bool last_slab) {
        if (h_block_offsets)
            for (uint64_t k = 0; k < blocks + (last_slab ? 1 : 0); ++k) h_block_offsets[block_at + k] = file_at + offsets[k];
        block_at += blocks;
    }
};

}  // namespace

void Bgzf::launch_batch(Work<Bgzf> &w, hipStream_t st, const Job &job, uint64_t first, uint32_t count, uint32_t batch) {
    hipLaunchKernelGGL(bgzf_block_kernel, dim3(count), dim3(64), 0, st, job.d_in, job.n, first, w.d_tokens, w.d_stage, w.d_recs, w.d_error);
    hipLaunchKernelGGL(bgzf_frame_kernel, dim3(count), dim3(COPY_BLOCK), 0, st, (const uint8_t *)w.d_stage, (const uint32_t *)w.d_recs, first, count, w.d_bases, batch, job.d_out, job.capacity,
                       w.d_offsets, w.d_error);
}

void Bgzf::launch_end(Work<Bgzf> &w, hipStream_t st, const Job &job, uint64_t blocks, uint32_t batches) {
    hipLaunchKernelGGL(bgzf_end_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long *)w.d_bases, batches, blocks, job.flag, job.d_out, job.capacity, w.d_offsets, w.d_error);
}

extern "C" {

int bt_bgzf_bound(uint64_t n, uint64_t *capacity, uint64_t *blocks) {
    if (!capacity || !blocks) return fail("bt_bgzf_bound: null argument");
    *capacity = bgzf_bound(n);
    *blocks = num_blocks(n);
    return BT_OK;
}

int bt_bgzf(bt_ctx *ctx, const uint8_t *d_in, uint64_t n, int eof, uint8_t *d_out, uint64_t capacity, uint64_t *h_out_bytes, uint64_t *h_block_offsets, bt_deflate_stats *stats) {
    if (!ctx || (n && !d_in) || !d_out || !h_out_bytes) return fail("bt_bgzf: null argument");
    if (capacity < bgzf_bound(n)) return too_small("bt_bgzf", capacity, "bt_bgzf_bound", bgzf_bound(n));
    return run_once<Bgzf>("bt_bgzf", ctx, Job{d_in, n, eof, d_out, capacity}, h_out_bytes, h_block_offsets, stats);
}

int bt_bgzf_save(bt_ctx *ctx, const char *path, const uint8_t *h_data, uint64_t n, uint32_t threads, uint64_t *h_block_offsets, uint64_t offsets_capacity, bt_deflate_stats *stats) {
    (void)threads;   // no host CRC on this route: nothing here runs on a thread pool, and the bytes cannot depend on it
    if (!ctx || !path || (n && !h_data)) return fail("bt_bgzf_save: null argument");
    if (h_block_offsets && offsets_capacity < num_blocks(n) + 1)
        return fail("bt_bgzf_save: room for " + std::to_string(offsets_capacity) + " block offsets, " + std::to_string(num_blocks(n) + 1) + " needed");
    FileOffsets offsets;
    offsets.h_block_offsets = h_block_offsets;
    return save<Bgzf>("bt_bgzf_save", ctx, path, h_data, n, offsets, stats);
}

int bt_diag_bgzf(const uint8_t *h_in, uint64_t n, int eof, uint8_t *h_out, uint64_t capacity, uint64_t *out_bytes, uint64_t *h_block_offsets, bt_deflate_stats *stats) {
    if ((n && !h_in) || !h_out || !out_bytes) return fail("bt_diag_bgzf: null argument");
    if (capacity < bgzf_bound(n)) return too_small("bt_diag_bgzf", capacity, "bt_bgzf_bound", bgzf_bound(n));
    return replay<Bgzf>("bt_diag_bgzf", h_in, n, eof, h_out, capacity, out_bytes, h_block_offsets, stats);
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
