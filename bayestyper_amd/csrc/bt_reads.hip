// libbtgpu: a sample's k-mers straight from its reads — the consumers of a KMC database without the database.
//   bt_reads_count      <- KmerCounter::parseSampleKmers + parseSampleKmersCallBack (KmerCounter.cpp:388-524)
//   bt_reads_make_bloom <- bayesTyperTools makeBloom (MakeBloom.cpp:200-295)
//   bt_reads_sketch     (no counterpart: the number of distinct k-mers a KMC database states in its header, estimated)
//   bt_reads_*_packed   the same three over packed reads (bt_reads_pack.hpp: 2-bit codes and validity bits), the input of a pass that reads a sample's reads pack
// Both reference consumers are pure functions of the multiset of canonical k-mers of the reads (makeBloom of the set alone), so one streaming pass over
// the reads text computes what they compute from the database: no database is written, no k-mer sorted.  The window code is bt_reads_window.hpp, one
// front end over a consumer policy; the table and Bloom primitives are those of the KMC scan (bt_table_device.hpp, bt_kmer_device.hpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>

#include "bt_reads_window.hpp"
#include "bt_table_device.hpp"

using namespace bt;

namespace {

// A workgroup as the front end's team.  RUN = 60: a lane's run starts 15 LDS words after its neighbour's — an odd stride, so the byte reads of the 64 lanes of a
// wavefront fall into 64 different banks — and the k - 1 steps that fill a lane's first window are spread over 60 windows.
struct BlockTeam {
    static constexpr unsigned LANES = 256, RUN = 60;
    uint8_t *lds;
    __device__ unsigned lane() const { return threadIdx.x; }
    __device__ uint64_t first_tile() const { return blockIdx.x; }
    __device__ uint64_t tile_stride() const { return gridDim.x; }
    __device__ uint8_t *codes() { return lds; }
    __device__ void sync() { __syncthreads(); }
};
constexpr uint64_t READS_TILE = (uint64_t)BlockTeam::LANES * BlockTeam::RUN;

// parseSampleKmersCallBack (KmerCounter.cpp:412-419): path Bloom lookup, addKmer, addSampleCount(sample, 1) per occurrence (saturating, as the database's
// count capped at 255 is)
struct CountConsumer {
    TableView t;
    BloomView bloom;
    uint32_t sample_idx;
    unsigned long long *hit_count;   // optional
    unsigned hits;
    __device__ void operator()(Kmer can, uint64_t h, uint64_t) {
        if (!bloom_contains(h, bloom)) return;
        ++hits;
        const int64_t slot = table_find_or_insert(t, can);
        if (slot >= 0) sat_add_byte(t.counts(slot), sample_idx, 1u);
    }
    __device__ void finish() {   // one atomic per workgroup
        __shared__ unsigned block_hits;
        if (threadIdx.x == 0) block_hits = 0;
        __syncthreads();
        if (hits) atomicAdd(&block_hits, hits);
        __syncthreads();
        if (threadIdx.x == 0 && hit_count && block_hits) atomicAdd(hit_count, (unsigned long long)block_hits);
    }
};

// MakeBloom.cpp:262-271: every k-mer into the sample's filter, as kmc_make_bloom_kernel does per record
struct BloomConsumer {
    BloomView bloom;
    __device__ void operator()(Kmer, uint64_t h, uint64_t) { bloom_insert(h, bloom); }
    __device__ void finish() {}
};

// HyperLogLog: a byte-wise maximum through a 32-bit compare-and-swap, like sat_add_byte; a maximum is order-independent, so the registers are a pure function
// of the text
struct SketchConsumer {
    uint32_t *words;   // SKETCH_REGISTERS bytes
    __device__ void operator()(Kmer, uint64_t h, uint64_t) {
        uint32_t reg, rank;
        sketch_slot(h, &reg, &rank);
        uint32_t *w = &words[reg >> 2];
        const unsigned sh = (reg & 3u) * 8u;
        uint32_t old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (((old >> sh) & 0xFFu) < rank) {
            const uint32_t desired = (old & ~(0xFFu << sh)) | (rank << sh);
            const uint32_t prev = atomicCAS(w, old, desired);
            if (prev == old) return;
            old = prev;
        }
    }
    __device__ void finish() {}
};

template <class Consumer>
__global__ __launch_bounds__(BlockTeam::LANES) void reads_kernel(const char *__restrict__ text, uint64_t len, uint64_t first_end, RollConst c, Consumer consumer) {
    __shared__ uint8_t codes[READS_TILE + READS_MAX_HALO + 1];
    BlockTeam team{codes};
    reads_front_end(team, text, len, first_end, c, consumer);
    consumer.finish();
}

template <class Consumer>
int reads_launch(bt_ctx *ctx, const char *d_text, uint64_t len, uint64_t first_end, unsigned k, const Consumer &consumer) {
    if (len == 0 || first_end >= len) return BT_OK;
    BT_HIP(hipSetDevice(ctx->device));
    const unsigned grid = grid_for(len, (unsigned)READS_TILE, (unsigned)ctx->num_cu * 8u);
    hipLaunchKernelGGL(reads_kernel<Consumer>, dim3(grid), dim3(BlockTeam::LANES), 0, ctx->stream, d_text, len, first_end, make_roll_const(k), consumer);
    BT_CHECK_LAUNCH();
    return BT_OK;
}

// the sibling over a packed text (bt_reads_pack.hpp): the image starts 64 positions before the tile, so it is as large as the text kernels'
template <class Consumer>
__global__ __launch_bounds__(BlockTeam::LANES) void reads_packed_kernel(const uint32_t *__restrict__ packed, uint64_t positions, uint64_t first_end, RollConst c, Consumer consumer) {
    __shared__ __attribute__((aligned(16))) uint8_t codes[READS_TILE + READS_PACKED_LEAD];
    BlockTeam team{codes};
    reads_front_end_packed(team, packed, positions, first_end, c, consumer);
    consumer.finish();
}

template <class Consumer>
int reads_launch_packed(bt_ctx *ctx, const uint8_t *d_packed, uint64_t positions, uint64_t first_end, unsigned k, const Consumer &consumer) {
    if (positions == 0 || first_end >= positions) return BT_OK;
    BT_HIP(hipSetDevice(ctx->device));
    const unsigned grid = grid_for(positions, (unsigned)READS_TILE, (unsigned)ctx->num_cu * 8u);
    hipLaunchKernelGGL(reads_packed_kernel<Consumer>, dim3(grid), dim3(BlockTeam::LANES), 0, ctx->stream, reinterpret_cast<const uint32_t *>(d_packed), positions, first_end,
                       make_roll_const(k), consumer);
    BT_CHECK_LAUNCH();
    return BT_OK;
}
int check_packed(const char *who, const void *packed, uint64_t positions) {
    if (positions && !packed) return fail(std::string(who) + ": null argument");
    if (reinterpret_cast<uintptr_t>(packed) & 3u) return fail(std::string(who) + ": the packed reads must be 4-byte aligned");
    return BT_OK;
}

int check_count_args(const char *who, bt_ctx *ctx, bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx) {
    if (!ctx || !path_bloom || !table) return fail(std::string(who) + ": null argument");
    if (path_bloom->k != table->k) return fail(std::string(who) + ": k mismatch between table and bloom");
    if (table->k < 1 || table->k > 64) return fail(std::string(who) + ": k must lie in 1 .. 64");
    if (sample_idx >= table->num_samples) return fail(std::string(who) + ": sample index out of range");
    if (path_bloom->ctx->device != ctx->device || table->ctx->device != ctx->device) return fail(std::string(who) + ": the filter and the table must live on the context's device");
    return BT_OK;
}
int check_bloom_args(const char *who, bt_ctx *ctx, bt_bloom *sample_bloom, uint32_t k) {
    if (!ctx || !sample_bloom) return fail(std::string(who) + ": null argument");
    if (k < 1 || k > 64) return fail(std::string(who) + ": k must lie in 1 .. 64");
    if (sample_bloom->k != k) return fail(std::string(who) + ": k mismatch");
    if (sample_bloom->ctx->device != ctx->device) return fail(std::string(who) + ": the filter must live on the context's device");
    return BT_OK;
}
CountConsumer count_consumer(bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx, uint64_t *d_hit_count) {
    return CountConsumer{table->v, path_bloom->view(), sample_idx, reinterpret_cast<unsigned long long *>(d_hit_count), 0u};
}

// Host data through the context's two staging slots (the pinned and device buffers bt_kmc_scan_run_host leaves with the context: taken when they are large enough,
// left there afterwards): copy, transfer (own stream) and scan of consecutive chunks overlap.  next(chunk): the next chunk's bytes in host memory (at most `need`),
// the size it is launched with and the first position whose windows are new, false when none is left.  launch(d_chunk, size, first_end).  Blocking.
struct ReadsChunk {
    const void *src;
    uint64_t bytes, size, first_end;
};
using ReadsChunkNext = std::function<bool(ReadsChunk &)>;
using ReadsChunkLaunch = std::function<int(const char *, uint64_t, uint64_t)>;
int reads_stream_chunks(bt_ctx *ctx, const char *what, size_t need, const ReadsChunkNext &next, const ReadsChunkLaunch &launch) {
    BT_HIP(hipSetDevice(ctx->device));
    need = (need + 15) / 16 * 16;
    uint8_t *pin[2] = {nullptr, nullptr}, *dev[2] = {nullptr, nullptr};
    size_t have = 0;
    hipError_t e = hipSuccess;
    if (ctx->kmc_stage_bytes >= need && ctx->kmc_pin[0] && ctx->kmc_pin[1] && ctx->kmc_dev[0] && ctx->kmc_dev[1]) {
        have = ctx->kmc_stage_bytes;
        for (int b = 0; b < 2; ++b) {
            pin[b] = ctx->kmc_pin[b];
            dev[b] = ctx->kmc_dev[b];
            ctx->kmc_pin[b] = ctx->kmc_dev[b] = nullptr;
        }
        ctx->kmc_stage_bytes = 0;
    } else {
        have = need;
        for (int b = 0; b < 2 && e == hipSuccess; ++b) {
            e = hipHostMalloc(reinterpret_cast<void **>(&pin[b]), need, hipHostMallocDefault);
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&dev[b]), need + 16);
        }
    }
    hipStream_t copy_stream = nullptr;
    hipEvent_t copied[2] = {nullptr, nullptr}, scanned[2] = {nullptr, nullptr};
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking);
    for (int b = 0; b < 2 && e == hipSuccess; ++b) {
        e = hipEventCreateWithFlags(&copied[b], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&scanned[b], hipEventDisableTiming);
    }
    int rc = BT_OK;
    ReadsChunk chunk;
    for (uint64_t i = 0; e == hipSuccess && rc == BT_OK && next(chunk); ++i) {
        const int b = (int)(i & 1);
        if (i >= 2) e = hipEventSynchronize(copied[b]);   // the pinned buffer of this slot has been read by its previous transfer
        if (e != hipSuccess) break;
        std::memcpy(pin[b], chunk.src, chunk.bytes);
        if (i >= 2) e = hipStreamWaitEvent(copy_stream, scanned[b], 0);   // the device buffer of this slot has been scanned
        if (e == hipSuccess) e = hipMemcpyAsync(dev[b], pin[b], chunk.bytes, hipMemcpyHostToDevice, copy_stream);
        if (e == hipSuccess) e = hipEventRecord(copied[b], copy_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, copied[b], 0);
        if (e != hipSuccess) break;
        rc = launch(reinterpret_cast<const char *>(dev[b]), chunk.size, chunk.first_end);
        if (rc == BT_OK) e = hipEventRecord(scanned[b], ctx->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (copy_stream) (void)hipStreamSynchronize(copy_stream);
    for (int b = 0; b < 2; ++b) {
        if (copied[b]) (void)hipEventDestroy(copied[b]);
        if (scanned[b]) (void)hipEventDestroy(scanned[b]);
    }
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    // the slots go (back) to the context when they are whole and no smaller than what it holds
    const bool whole = pin[0] && pin[1] && dev[0] && dev[1];
    if (whole && have >= ctx->kmc_stage_bytes && !ctx_caches_off()) {
        for (int b = 0; b < 2; ++b) {
            if (ctx->kmc_pin[b]) (void)hipHostFree(ctx->kmc_pin[b]);
            if (ctx->kmc_dev[b]) (void)hipFree(ctx->kmc_dev[b]);
            ctx->kmc_pin[b] = pin[b];
            ctx->kmc_dev[b] = dev[b];
        }
        ctx->kmc_stage_bytes = have;
    } else {
        for (int b = 0; b < 2; ++b) {
            if (pin[b]) (void)hipHostFree(pin[b]);
            if (dev[b]) (void)hipFree(dev[b]);
        }
    }
    if (rc != BT_OK) return rc;
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(std::string(what) + ": " + hipGetErrorString(e));
    return BT_OK;
}

// A reads text: a chunk starts k - 1 bytes before its first new byte and the kernel consumes only the windows that end at a new byte, so the chunk size changes
// no result.
int reads_stream(bt_ctx *ctx, const char *what, const char *h_text, uint64_t len, unsigned k, uint64_t chunk_bytes, const ReadsChunkLaunch &launch) {
    if (len == 0) return BT_OK;
    const uint64_t halo = k - 1u;
    chunk_bytes = std::max<uint64_t>(64, std::min<uint64_t>(chunk_bytes ? chunk_bytes : (64ull << 20), len));
    uint64_t done = 0;
    return reads_stream_chunks(ctx, what, (size_t)(chunk_bytes + halo), [&](ReadsChunk &c) {
        if (done >= len) return false;
        const uint64_t end = std::min(len, done + chunk_bytes), lo = done >= halo ? done - halo : 0;
        c = ReadsChunk{h_text + lo, end - lo, end - lo, done - lo};
        done = end;
        return true;
    }, launch);
}

// A packed text: the text route's rule in whole blocks.  A chunk starts on the block boundary at or before done - (k - 1) and is launched with first_end = done -
// chunk start; chunk_bytes (0: 64 MiB) counts packed bytes, at least one block.
int reads_stream_packed(bt_ctx *ctx, const char *what, const uint8_t *h_packed, uint64_t positions, unsigned k, uint64_t chunk_bytes, const ReadsChunkLaunch &launch) {
    if (positions == 0) return BT_OK;
    const uint64_t halo = k - 1u, total = reads_packed_bytes(positions);
    const uint64_t chunk_positions = std::max<uint64_t>(1, std::min<uint64_t>(chunk_bytes ? chunk_bytes : (64ull << 20), total) / PACK_BLOCK_BYTES) * PACK_BLOCK_POSITIONS;
    uint64_t done = 0;   // a multiple of 128 until the end
    return reads_stream_chunks(ctx, what, (size_t)reads_packed_bytes(chunk_positions + PACK_BLOCK_POSITIONS), [&](ReadsChunk &c) {
        if (done >= positions) return false;
        const uint64_t end = std::min(positions, done + chunk_positions), lo = (done >= halo ? done - halo : 0) / PACK_BLOCK_POSITIONS * PACK_BLOCK_POSITIONS;
        c = ReadsChunk{h_packed + lo / PACK_BLOCK_POSITIONS * PACK_BLOCK_BYTES, reads_packed_bytes(end - lo), end - lo, done - lo};
        done = end;
        return true;
    }, launch);
}

// the host variants of the count and of the sketch around whichever stream feeds them: stream(d_hits) / stream(d_registers) launches every chunk
int count_host(const char *who, bt_ctx *ctx, bt_table *table, uint64_t *h_hit_count, const std::function<int(uint64_t *)> &stream) {
    BT_HIP(hipSetDevice(ctx->device));
    uint64_t *d_hits = nullptr;
    BT_HIP(hipMalloc(reinterpret_cast<void **>(&d_hits), 8));
    unsigned long long hits = 0;
    hipError_t e = hipMemsetAsync(d_hits, 0, 8, ctx->stream);
    int rc = e == hipSuccess ? BT_OK : fail(std::string(who) + ": " + hipGetErrorString(e));
    if (rc == BT_OK) rc = stream(d_hits);
    if (rc == BT_OK) {
        e = hipMemcpyAsync(&hits, d_hits, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = fail(std::string(who) + ": " + hipGetErrorString(e));
    }
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_hits);
    if (rc != BT_OK) return rc;
    int overflowed = 0;
    if (bt_table_status(table, nullptr, nullptr, &overflowed) != BT_OK) return BT_ERR;
    if (overflowed) return fail(std::string(who) + ": the count table is full, matched k-mers were dropped (bt_table_reserve before the scan)");
    if (h_hit_count) *h_hit_count = hits;
    return BT_OK;
}
int sketch_host(const char *who, bt_ctx *ctx, uint8_t *h_registers, const std::function<int(uint32_t *)> &stream) {
    BT_HIP(hipSetDevice(ctx->device));
    uint8_t *d_reg = nullptr;
    BT_HIP(hipMalloc(reinterpret_cast<void **>(&d_reg), SKETCH_REGISTERS));
    hipError_t e = hipMemcpyAsync(d_reg, h_registers, SKETCH_REGISTERS, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (h_registers is pageable: the copy has left it)
    int rc = e == hipSuccess ? BT_OK : fail(std::string(who) + ": " + hipGetErrorString(e));
    if (rc == BT_OK) rc = stream(reinterpret_cast<uint32_t *>(d_reg));
    if (rc == BT_OK) {
        e = hipMemcpyAsync(h_registers, d_reg, SKETCH_REGISTERS, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = fail(std::string(who) + ": " + hipGetErrorString(e));
    }
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_reg);
    return rc;
}

}  // namespace

extern "C" {

int bt_reads_count(bt_ctx *ctx, bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx, const char *d_text, uint64_t len, uint64_t *d_hit_count) {
    if (check_count_args("bt_reads_count", ctx, path_bloom, table, sample_idx) != BT_OK) return BT_ERR;
    if (len && !d_text) return fail("bt_reads_count: null argument");
    return reads_launch(ctx, d_text, len, 0, table->k, count_consumer(path_bloom, table, sample_idx, d_hit_count));
}

int bt_reads_make_bloom(bt_ctx *ctx, bt_bloom *sample_bloom, const char *d_text, uint64_t len, uint32_t k) {
    if (check_bloom_args("bt_reads_make_bloom", ctx, sample_bloom, k) != BT_OK) return BT_ERR;
    if (len && !d_text) return fail("bt_reads_make_bloom: null argument");
    return reads_launch(ctx, d_text, len, 0, k, BloomConsumer{sample_bloom->view()});
}

int bt_reads_sketch(bt_ctx *ctx, const char *d_text, uint64_t len, uint32_t k, uint8_t *d_registers) {
    if (!ctx || !d_registers || (len && !d_text)) return fail("bt_reads_sketch: null argument");
    if (k < 1 || k > 64) return fail("bt_reads_sketch: k must lie in 1 .. 64");
    if (reinterpret_cast<uintptr_t>(d_registers) & 3u) return fail("bt_reads_sketch: d_registers must be 4-byte aligned");
    return reads_launch(ctx, d_text, len, 0, k, SketchConsumer{reinterpret_cast<uint32_t *>(d_registers)});
}

int bt_reads_count_host(bt_ctx *ctx, bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx, const char *h_text, uint64_t len, uint64_t chunk_bytes, uint64_t *h_hit_count) {
    const char *who = "bt_reads_count_host";
    if (check_count_args(who, ctx, path_bloom, table, sample_idx) != BT_OK) return BT_ERR;
    if (len && !h_text) return fail("bt_reads_count_host: null argument");
    return count_host(who, ctx, table, h_hit_count, [&](uint64_t *d_hits) {
        return reads_stream(ctx, who, h_text, len, table->k, chunk_bytes, [&](const char *d, uint64_t n, uint64_t first_end) {
            return reads_launch(ctx, d, n, first_end, table->k, count_consumer(path_bloom, table, sample_idx, d_hits));
        });
    });
}

int bt_reads_make_bloom_host(bt_ctx *ctx, bt_bloom *sample_bloom, const char *h_text, uint64_t len, uint32_t k, uint64_t chunk_bytes) {
    const char *who = "bt_reads_make_bloom_host";
    if (check_bloom_args(who, ctx, sample_bloom, k) != BT_OK) return BT_ERR;
    if (len && !h_text) return fail("bt_reads_make_bloom_host: null argument");
    return reads_stream(ctx, who, h_text, len, k, chunk_bytes,
                        [&](const char *d, uint64_t n, uint64_t first_end) { return reads_launch(ctx, d, n, first_end, k, BloomConsumer{sample_bloom->view()}); });
}

int bt_reads_sketch_host(bt_ctx *ctx, const char *h_text, uint64_t len, uint32_t k, uint64_t chunk_bytes, uint8_t *h_registers) {
    const char *who = "bt_reads_sketch_host";
    if (!ctx || !h_registers || (len && !h_text)) return fail("bt_reads_sketch_host: null argument");
    if (k < 1 || k > 64) return fail("bt_reads_sketch_host: k must lie in 1 .. 64");
    return sketch_host(who, ctx, h_registers, [&](uint32_t *d_reg) {
        return reads_stream(ctx, who, h_text, len, k, chunk_bytes,
                            [&](const char *d, uint64_t n, uint64_t first_end) { return reads_launch(ctx, d, n, first_end, k, SketchConsumer{d_reg}); });
    });
}

// The same three consumers over a packed text (bt_reads_pack.hpp), device buffers and host buffers: (packed, positions) in place of (text, len).
int bt_reads_count_packed(bt_ctx *ctx, bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx, const uint8_t *d_packed, uint64_t positions, uint64_t *d_hit_count) {
    const char *who = "bt_reads_count_packed";
    if (check_count_args(who, ctx, path_bloom, table, sample_idx) != BT_OK || check_packed(who, d_packed, positions) != BT_OK) return BT_ERR;
    return reads_launch_packed(ctx, d_packed, positions, 0, table->k, count_consumer(path_bloom, table, sample_idx, d_hit_count));
}

int bt_reads_make_bloom_packed(bt_ctx *ctx, bt_bloom *sample_bloom, const uint8_t *d_packed, uint64_t positions, uint32_t k) {
    const char *who = "bt_reads_make_bloom_packed";
    if (check_bloom_args(who, ctx, sample_bloom, k) != BT_OK || check_packed(who, d_packed, positions) != BT_OK) return BT_ERR;
    return reads_launch_packed(ctx, d_packed, positions, 0, k, BloomConsumer{sample_bloom->view()});
}

int bt_reads_sketch_packed(bt_ctx *ctx, const uint8_t *d_packed, uint64_t positions, uint32_t k, uint8_t *d_registers) {
    const char *who = "bt_reads_sketch_packed";
    if (!ctx || !d_registers) return fail("bt_reads_sketch_packed: null argument");
    if (check_packed(who, d_packed, positions) != BT_OK) return BT_ERR;
    if (k < 1 || k > 64) return fail("bt_reads_sketch_packed: k must lie in 1 .. 64");
    if (reinterpret_cast<uintptr_t>(d_registers) & 3u) return fail("bt_reads_sketch_packed: d_registers must be 4-byte aligned");
    return reads_launch_packed(ctx, d_packed, positions, 0, k, SketchConsumer{reinterpret_cast<uint32_t *>(d_registers)});
}

int bt_reads_count_packed_host(bt_ctx *ctx, bt_bloom *path_bloom, bt_table *table, uint32_t sample_idx, const uint8_t *h_packed, uint64_t positions, uint64_t chunk_bytes,
                               uint64_t *h_hit_count) {
    const char *who = "bt_reads_count_packed_host";
    if (check_count_args(who, ctx, path_bloom, table, sample_idx) != BT_OK || check_packed(who, h_packed, positions) != BT_OK) return BT_ERR;
    return count_host(who, ctx, table, h_hit_count, [&](uint64_t *d_hits) {
        return reads_stream_packed(ctx, who, h_packed, positions, table->k, chunk_bytes, [&](const char *d, uint64_t n, uint64_t first_end) {
            return reads_launch_packed(ctx, reinterpret_cast<const uint8_t *>(d), n, first_end, table->k, count_consumer(path_bloom, table, sample_idx, d_hits));
        });
    });
}

int bt_reads_make_bloom_packed_host(bt_ctx *ctx, bt_bloom *sample_bloom, const uint8_t *h_packed, uint64_t positions, uint32_t k, uint64_t chunk_bytes) {
    const char *who = "bt_reads_make_bloom_packed_host";
    if (check_bloom_args(who, ctx, sample_bloom, k) != BT_OK || check_packed(who, h_packed, positions) != BT_OK) return BT_ERR;
    return reads_stream_packed(ctx, who, h_packed, positions, k, chunk_bytes, [&](const char *d, uint64_t n, uint64_t first_end) {
        return reads_launch_packed(ctx, reinterpret_cast<const uint8_t *>(d), n, first_end, k, BloomConsumer{sample_bloom->view()});
    });
}

int bt_reads_sketch_packed_host(bt_ctx *ctx, const uint8_t *h_packed, uint64_t positions, uint32_t k, uint64_t chunk_bytes, uint8_t *h_registers) {
    const char *who = "bt_reads_sketch_packed_host";
    if (!ctx || !h_registers) return fail("bt_reads_sketch_packed_host: null argument");
    if (check_packed(who, h_packed, positions) != BT_OK) return BT_ERR;
    if (k < 1 || k > 64) return fail("bt_reads_sketch_packed_host: k must lie in 1 .. 64");
    return sketch_host(who, ctx, h_registers, [&](uint32_t *d_reg) {
        return reads_stream_packed(ctx, who, h_packed, positions, k, chunk_bytes, [&](const char *d, uint64_t n, uint64_t first_end) {
            return reads_launch_packed(ctx, reinterpret_cast<const uint8_t *>(d), n, first_end, k, SketchConsumer{d_reg});
        });
    });
}

int bt_reads_sketch_estimate(const uint8_t *h_registers, double *out) {
    if (!h_registers || !out) return fail("bt_reads_sketch_estimate: null argument");
    const double m = (double)SKETCH_REGISTERS;
    double sum = 0;
    uint32_t zeros = 0;
    for (uint32_t i = 0; i < SKETCH_REGISTERS; ++i) {
        if (h_registers[i] > 64u - SKETCH_BITS + 1u) return fail("bt_reads_sketch_estimate: a register above 49");
        sum += std::ldexp(1.0, -(int)h_registers[i]);
        zeros += h_registers[i] == 0;
    }
    const double alpha = 0.7213 / (1.0 + 1.079 / m);
    double est = alpha * m * m / sum;
    if (est <= 2.5 * m && zeros) est = m * std::log(m / (double)zeros);   // linear counting
    *out = est;
    return BT_OK;
}

int bt_diag_reads_kmers(const char *h_text, uint64_t len, uint32_t k, uint64_t *h_kmers, uint64_t *h_hashes, uint64_t *h_ends, uint64_t capacity, uint64_t *n) {
    if ((len && !h_text) || !n) return fail("bt_diag_reads_kmers: null argument");
    if (k < 1 || k > 64) return fail("bt_diag_reads_kmers: k must lie in 1 .. 64");
    HostTeam team;
    uint64_t count = 0;
    auto consume = [&](Kmer can, uint64_t h, uint64_t end) {
        if (count < capacity) {
            if (h_kmers) {
                h_kmers[2 * count] = can.lo;
                h_kmers[2 * count + 1] = can.hi;
            }
            if (h_hashes) h_hashes[count] = h;
            if (h_ends) h_ends[count] = end;
        }
        ++count;
    };
    reads_front_end(team, h_text, len, 0, make_roll_const(k), consume);
    *n = count;
    if (count > capacity) return fail("bt_diag_reads_kmers: buffer too small");
    return BT_OK;
}

int bt_diag_reads_kmers_packed(const uint8_t *h_packed, uint64_t positions, uint32_t k, uint64_t *h_kmers, uint64_t *h_hashes, uint64_t *h_ends, uint64_t capacity, uint64_t *n) {
    if (!n) return fail("bt_diag_reads_kmers_packed: null argument");
    if (check_packed("bt_diag_reads_kmers_packed", h_packed, positions) != BT_OK) return BT_ERR;
    if (k < 1 || k > 64) return fail("bt_diag_reads_kmers_packed: k must lie in 1 .. 64");
    PackedHostTeam team;
    uint64_t count = 0;
    auto consume = [&](Kmer can, uint64_t h, uint64_t end) {
        if (count < capacity) {
            if (h_kmers) {
                h_kmers[2 * count] = can.lo;
                h_kmers[2 * count + 1] = can.hi;
            }
            if (h_hashes) h_hashes[count] = h;
            if (h_ends) h_ends[count] = end;
        }
        ++count;
    };
    reads_front_end_packed(team, reinterpret_cast<const uint32_t *>(h_packed), positions, 0, make_roll_const(k), consume);
    *n = count;
    if (count > capacity) return fail("bt_diag_reads_kmers_packed: buffer too small");
    return BT_OK;
}

int bt_diag_reads_sketch(const char *h_text, uint64_t len, uint32_t k, uint8_t *h_registers) {
    if ((len && !h_text) || !h_registers) return fail("bt_diag_reads_sketch: null argument");
    if (k < 1 || k > 64) return fail("bt_diag_reads_sketch: k must lie in 1 .. 64");
    HostTeam team;
    auto consume = [&](Kmer, uint64_t h, uint64_t) {
        uint32_t reg, rank;
        sketch_slot(h, &reg, &rank);
        if (h_registers[reg] < rank) h_registers[reg] = (uint8_t)rank;
    };
    reads_front_end(team, h_text, len, 0, make_roll_const(k), consume);
    return BT_OK;
}

}  // extern "C"
