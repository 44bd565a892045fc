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
// deflate_compact_kernel: btgz::place_unit without framing — one workgroup per piece sums the sizes of the batch's pieces before its own and copies its
//   slot to its place; the workgroup of the batch's last piece leaves the running total for the next batch.
// Everything behind the kernels — the scratch, the batches of a call, the slab pipeline of bt_gzip_save, the host replay — is bt_gz_pipeline.hpp over the
// policy btgz::RawDeflate, shared with bt_bgzf.hip.  What is left here: the two kernels, their launch, the gzip member around the slabs, argument checks.
#include <zlib.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "bt_gz_pipeline.hpp"

using namespace btgz;

namespace {

__global__ __launch_bounds__(64) void deflate_piece_kernel(const uint8_t *__restrict__ in, uint64_t n, uint64_t first_piece, uint64_t total_pieces, int last,
                                                           uint32_t *__restrict__ tokens, uint8_t *__restrict__ stage, uint32_t *__restrict__ recs, uint32_t *error) {
    __shared__ Shared sh;
    const uint64_t piece = first_piece + blockIdx.x, off = piece * kPiece;
    const uint32_t len = off >= n ? 0u : (uint32_t)std::min<uint64_t>(kPiece, n - off);
    deflate_piece<WaveTeam>(sh, in + off, len, last && piece + 1 == total_pieces, tokens + (uint64_t)blockIdx.x * kPiece, stage + (uint64_t)blockIdx.x * kPieceOut,
                            recs + piece * kRecWords, error);
}

__global__ __launch_bounds__(COPY_BLOCK) void deflate_compact_kernel(const uint8_t *__restrict__ stage, const uint32_t *__restrict__ recs, uint64_t first_piece, uint32_t batch_pieces,
                                                                     unsigned long long *bases, uint32_t batch, uint8_t *__restrict__ out, uint64_t capacity, uint32_t *error) {
    place_unit<RawDeflate>(stage, recs, first_piece, batch_pieces, bases, batch, out, capacity, nullptr, error);
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

// what bt_gzip_save puts around the slabs' streams: writeGzFile's header, and the CRC-32 (computed slab by slab while the device works) and length behind
struct GzipMember : NoExtras {
    uint64_t n = 0;
    unsigned threads = 1;
    uLong crc = crc32(0L, Z_NULL, 0);
    bool before(TmpFile &file) {
        const unsigned char header[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};   // deflate, no flags, no time stamp, unix
        return file.write(header, 10);
    }
    void overlap(const uint8_t *slab, uint64_t len) { crc = crc32_combine(crc, crc_parallel(slab, len, threads), (z_off_t)len); }
    bool after(TmpFile &file) {
        const uint32_t trailer[2] = {(uint32_t)crc, (uint32_t)(n & 0xFFFFFFFFu)};
        return file.write(trailer, 8);
    }
};

}  // namespace

void RawDeflate::launch_batch(Work<RawDeflate> &w, hipStream_t st, const Job &job, uint64_t first, uint32_t count, uint32_t batch) {
    hipLaunchKernelGGL(deflate_piece_kernel, dim3(count), dim3(64), 0, st, job.d_in, job.n, first, num_pieces(job.n), job.flag, w.d_tokens, w.d_stage, w.d_recs, w.d_error);
    hipLaunchKernelGGL(deflate_compact_kernel, dim3(count), dim3(COPY_BLOCK), 0, st, (const uint8_t *)w.d_stage, (const uint32_t *)w.d_recs, first, count, w.d_bases, batch, job.d_out,
                       job.capacity, w.d_error);
}

extern "C" {

int bt_deflate_bound(uint64_t n, uint64_t *capacity) {
    if (!capacity) return fail("bt_deflate_bound: null argument");
    *capacity = stream_bound(n);
    return BT_OK;
}

int bt_deflate(bt_ctx *ctx, const uint8_t *d_in, uint64_t n, int last, uint8_t *d_out, uint64_t capacity, uint64_t *h_out_bytes, bt_deflate_stats *stats) {
    if (!ctx || (n && !d_in) || !d_out || !h_out_bytes) return fail("bt_deflate: null argument");
    if (capacity < stream_bound(n)) return too_small("bt_deflate", capacity, "bt_deflate_bound", stream_bound(n));
    return run_once<RawDeflate>("bt_deflate", ctx, Job{d_in, n, last, d_out, capacity}, h_out_bytes, nullptr, stats);
}

int bt_gzip_save(bt_ctx *ctx, const char *path, const uint8_t *h_data, uint64_t n, uint32_t threads, bt_deflate_stats *stats) {
    if (!ctx || !path || (n && !h_data)) return fail("bt_gzip_save: null argument");
    GzipMember member;
    member.n = n;
    member.threads = std::max(1u, threads);
    return save<RawDeflate>("bt_gzip_save", ctx, path, h_data, n, member, stats);
}

int bt_diag_deflate(const uint8_t *h_in, uint64_t n, int last, uint8_t *h_out, uint64_t capacity, uint64_t *out_bytes, bt_deflate_stats *stats) {
    if ((n && !h_in) || !h_out || !out_bytes) return fail("bt_diag_deflate: null argument");
    if (capacity < stream_bound(n)) return too_small("bt_diag_deflate", capacity, "bt_deflate_bound", stream_bound(n));
    return replay<RawDeflate>("bt_diag_deflate", h_in, n, last, h_out, capacity, out_bytes, nullptr, stats);
}

}  // extern "C"
