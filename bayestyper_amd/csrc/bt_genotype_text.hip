// libbtgpu: the genotype-derived text of the VCF lines formatted ON THE DEVICE from bt_gibbs_genotypes' record string (bt_genotype_text, bt_genotype_text_sizes;
// bt_gibbs_genotype_text in bt_gibbs.hip runs the same passes), and the host-side diagnostics of the same code (bt_diag_genotype_text, bt_diag_format_g6).
// The formatting itself is bt_genotype_text.hpp, shared with the host.  Replaces GenotypeWriter.cpp:84-143 (the allele fields) and :261-345 (writeSamples,
// writeAlleleKmerStats) of the reference, which format on the writer's host threads.
//
// Lane mapping: as geno_cell_kernel's — one lane per (variant, sample) cell, a flat index over the string's variants, for the samples piece; one lane per
// variant for the stats and cover pieces.  Two passes: COUNT (each lane counts the bytes it will write; the variant lane turns its cells' lengths into offsets
// inside the samples piece), a scan of the variants' byte counts (64-bit offsets: the text of a thirty-sample launch approaches 4 GB), and WRITE (each lane
// formats again, into its place).  The text of a launch is exactly sized and contiguous in the string's variant order.
#include <algorithm>
#include <cstring>
#include <vector>

#include "bt_genotype_text.hpp"
#include "bt_internal.hpp"

using bt::fail;

namespace {

constexpr unsigned BLOCK = 256;
using namespace btgtext;

__global__ __launch_bounds__(BLOCK) void text_count_cell_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ var_off, uint32_t num_variants, uint32_t S,
                                                                uint32_t *__restrict__ cells) {
    const uint64_t idx = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= (uint64_t)num_variants * S) return;
    const uint32_t gv = (uint32_t)(idx / S), s = (uint32_t)(idx - (uint64_t)gv * S);
    count_cell(words, var_off, gv, s, cells + 2u * idx);
}
// status: [0] flags of all variants or-ed  [1] number of not-covered variants
__global__ __launch_bounds__(BLOCK) void text_count_variant_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ var_off, uint32_t num_variants, uint32_t S,
                                                                   uint32_t *__restrict__ variants, uint32_t *__restrict__ cells, uint32_t *__restrict__ status) {
    const uint32_t gv = blockIdx.x * BLOCK + threadIdx.x;
    if (gv >= num_variants) return;
    const uint32_t flags = count_variant(words, var_off, gv, S, variants + (uint64_t)kVariantWords * gv, cells + 2ull * gv * S);
    if (flags) atomicOr(&status[0], flags);
    if (flags & kFlagNotCovered) atomicAdd(&status[1], 1u);
}
// block-wise exclusive scan of the variants' byte counts, as scan_block_kernel (bt_paths.hip) with 64-bit sums: 1024 variants per workgroup (4 per lane);
// the offsets inside the block go to the variants' offset words, the block totals to `sums`
__global__ __launch_bounds__(BLOCK) void text_scan_block_kernel(uint32_t *__restrict__ variants, uint32_t num_variants, unsigned long long *__restrict__ sums) {
    __shared__ unsigned long long part[BLOCK];
    const uint64_t base = (uint64_t)blockIdx.x * (BLOCK * 4) + (uint64_t)threadIdx.x * 4;
    unsigned long long v[4], s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[q] = 0;
        if (base + q < num_variants) {
            const uint32_t *iv = variants + (base + q) * kVariantWords;
            v[q] = (unsigned long long)iv[IV_LEN_STATS] + iv[IV_LEN_COVER] + iv[IV_LEN_SAMPLES];
        }
        s += v[q];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (unsigned off = 1; off < BLOCK; off <<= 1) {   // Hillis-Steele over the 256 lane totals
        const unsigned long long add = threadIdx.x >= off ? part[threadIdx.x - off] : 0ull;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned long long run = part[threadIdx.x] - s;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (base + q < num_variants) {
            uint32_t *iv = variants + (base + q) * kVariantWords;
            iv[IV_OFF_LO] = (uint32_t)run;
            iv[IV_OFF_HI] = (uint32_t)(run >> 32);
        }
        run += v[q];
    }
    if (threadIdx.x == BLOCK - 1) sums[blockIdx.x] = part[BLOCK - 1];
}
__global__ __launch_bounds__(BLOCK) void text_scan_add_kernel(uint32_t *__restrict__ variants, uint32_t num_variants, const unsigned long long *__restrict__ block_off) {
    const uint64_t base = (uint64_t)blockIdx.x * (BLOCK * 4) + (uint64_t)threadIdx.x * 4;
    const unsigned long long add = block_off[blockIdx.x];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (base + q < num_variants) {
            uint32_t *iv = variants + (base + q) * kVariantWords;
            const unsigned long long off = variant_text_offset(iv) + add;
            iv[IV_OFF_LO] = (uint32_t)off;
            iv[IV_OFF_HI] = (uint32_t)(off >> 32);
        }
}
__global__ __launch_bounds__(BLOCK) void text_write_cell_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ var_off, uint32_t num_variants, uint32_t S,
                                                                const uint32_t *__restrict__ variants, uint32_t *__restrict__ cells, unsigned char *__restrict__ text) {
    const uint64_t idx = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= (uint64_t)num_variants * S) return;
    const uint32_t gv = (uint32_t)(idx / S), s = (uint32_t)(idx - (uint64_t)gv * S);
    write_cell(words, var_off, gv, s, variants + (uint64_t)kVariantWords * gv, cells + 2u * idx, text);
}
__global__ __launch_bounds__(BLOCK) void text_write_variant_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ var_off, uint32_t num_variants,
                                                                   const uint32_t *__restrict__ variants, unsigned char *__restrict__ text) {
    const uint32_t gv = blockIdx.x * BLOCK + threadIdx.x;
    if (gv >= num_variants) return;
    write_variant(words, var_off, gv, variants + (uint64_t)kVariantWords * gv, text);
}

// the head of a record string checked against its length, so that no pass reads outside it: h = [C, NV, S, x], cluster_var_off [C + 1], var_off [NV + 1]
int check_head(const char *who, const uint32_t *head4, uint64_t num_words, const uint32_t *tables, bt::GenoTextShape &sh) {
    sh.C = head4[0];
    sh.NV = head4[1];
    sh.S = head4[2];
    sh.at_voff = 4ull + sh.C + 1;
    const uint64_t at_rec = (sh.at_voff + sh.NV + 1 + 1) & ~1ull;
    if (num_words < at_rec) return fail(std::string(who) + ": the record string is shorter than its tables");
    if (tables) {
        const uint32_t *cvo = tables, *voff = tables + sh.C + 1;
        bool ok = cvo[0] == 0 && cvo[sh.C] == sh.NV && voff[0] >= at_rec && voff[sh.NV] <= num_words;
        for (uint32_t c = 0; ok && c < sh.C; ++c) ok = cvo[c] <= cvo[c + 1];
        for (uint32_t v = 0; ok && v < sh.NV; ++v) ok = voff[v] <= voff[v + 1];
        if (!ok) return fail(std::string(who) + ": the record string's offset tables are not those of bt_gibbs_genotypes");
    }
    sh.index_words = btgtext::index_words(sh.C, sh.NV, sh.S);
    if (sh.index_words >> 32 || ((uint64_t)sh.NV * sh.S + BLOCK - 1) / BLOCK >> 31) return fail(std::string(who) + ": more than 2^32 index words");
    return BT_OK;
}

}  // namespace

namespace bt {

int geno_text_shape(bt_ctx *ctx, const uint32_t *d_words, uint64_t num_words, GenoTextShape &sh, const char *who) {
    if (num_words < 4) return fail(std::string(who) + ": the record string is shorter than its head");
    hipStream_t st = ctx->stream;
    uint32_t head4[4];
    BT_HIP(hipMemcpyAsync(head4, d_words, 16, hipMemcpyDeviceToHost, st));
    BT_HIP(hipStreamSynchronize(st));
    int rc = check_head(who, head4, num_words, nullptr, sh);
    if (rc != BT_OK) return rc;
    sh.tables.resize((size_t)sh.C + 1 + sh.NV + 1);
    BT_HIP(hipMemcpyAsync(sh.tables.data(), d_words + 4, sh.tables.size() * 4, hipMemcpyDeviceToHost, st));
    BT_HIP(hipStreamSynchronize(st));
    return check_head(who, head4, num_words, sh.tables.data(), sh);
}

// the count pass and the scan: d_index (sh.index_words words) holds the finished index except the cells' words, which write_cell completes
int geno_text_count(bt_ctx *ctx, const uint32_t *d_words, const GenoTextShape &sh, uint32_t *d_index, uint64_t *text_bytes, uint32_t *not_covered, const char *who) {
    hipStream_t st = ctx->stream;
    const uint32_t C = sh.C, NV = sh.NV, S = sh.S;
    const uint64_t cells = (uint64_t)NV * S, nblk = ((uint64_t)NV + BLOCK * 4 - 1) / (BLOCK * 4);
    void *d_tmp = nullptr;   // block totals u64 [nblk] | status [2]
    struct Free {
        void *&p;
        ~Free() {
            if (p) (void)hipFree(p);
        }
    } fr{d_tmp};
    BT_HIP(hipMalloc(&d_tmp, nblk * 8 + 8));
    unsigned long long *d_sums = (unsigned long long *)d_tmp;
    uint32_t *d_status = (uint32_t *)(d_sums + nblk);
    BT_HIP(hipMemsetAsync(d_status, 0, 8, st));
    std::vector<uint32_t> head(kIndexHead + (size_t)C + 1, 0);
    head[0] = C;
    head[1] = NV;
    head[2] = S;
    std::memcpy(head.data() + kIndexHead, sh.tables.data(), ((size_t)C + 1) * 4);
    BT_HIP(hipMemcpyAsync(d_index, head.data(), head.size() * 4, hipMemcpyHostToDevice, st));
    const uint32_t *d_voff = d_words + sh.at_voff;
    uint32_t *d_variants = d_index + index_variants_at(C), *d_cells = d_index + index_cells_at(C, NV);
    if (cells) {
        hipLaunchKernelGGL(text_count_cell_kernel, dim3((unsigned)((cells + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, d_words, d_voff, NV, S, d_cells);
        BT_CHECK_LAUNCH();
    }
    std::vector<unsigned long long> sums(nblk);
    uint32_t status[2] = {0, 0};
    if (NV) {
        hipLaunchKernelGGL(text_count_variant_kernel, dim3((NV + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, d_words, d_voff, NV, S, d_variants, d_cells, d_status);
        BT_CHECK_LAUNCH();
        hipLaunchKernelGGL(text_scan_block_kernel, dim3((unsigned)nblk), dim3(BLOCK), 0, st, d_variants, NV, d_sums);
        BT_CHECK_LAUNCH();
        BT_HIP(hipMemcpyAsync(sums.data(), d_sums, nblk * 8, hipMemcpyDeviceToHost, st));
    }
    BT_HIP(hipMemcpyAsync(status, d_status, 8, hipMemcpyDeviceToHost, st));
    BT_HIP(hipStreamSynchronize(st));
    if (status[0] & kFlagMalformed) return fail(std::string(who) + ": a variant record does not have the layout of bt_gibbs_genotypes' string");
    uint64_t total = 0;   // the totals of the 1024-variant blocks pass through the host (NV / 1024 words), as in bt_paths.hip's scan
    for (uint64_t i = 0; i < nblk; ++i) {
        const uint64_t v = sums[i];
        sums[i] = total;
        total += v;
    }
    if (NV) {
        BT_HIP(hipMemcpyAsync(d_sums, sums.data(), nblk * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(text_scan_add_kernel, dim3((unsigned)nblk), dim3(BLOCK), 0, st, d_variants, NV, (const unsigned long long *)d_sums);
        BT_CHECK_LAUNCH();
    }
    BT_HIP(hipMemcpyAsync(d_index + 3, &status[1], 4, hipMemcpyHostToDevice, st));
    BT_HIP(hipStreamSynchronize(st));
    *text_bytes = total;
    *not_covered = status[1];
    return BT_OK;
}

// the write pass into d_text (as many bytes as geno_text_count told); complete on return
int geno_text_write(bt_ctx *ctx, const uint32_t *d_words, const GenoTextShape &sh, uint32_t *d_index, uint8_t *d_text) {
    hipStream_t st = ctx->stream;
    const uint64_t cells = (uint64_t)sh.NV * sh.S;
    const uint32_t *d_voff = d_words + sh.at_voff;
    uint32_t *d_variants = d_index + index_variants_at(sh.C), *d_cells = d_index + index_cells_at(sh.C, sh.NV);
    if (cells) {
        hipLaunchKernelGGL(text_write_cell_kernel, dim3((unsigned)((cells + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, d_words, d_voff, sh.NV, sh.S, (const uint32_t *)d_variants, d_cells, d_text);
        BT_CHECK_LAUNCH();
    }
    if (sh.NV) {
        hipLaunchKernelGGL(text_write_variant_kernel, dim3((sh.NV + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, d_words, d_voff, sh.NV, (const uint32_t *)d_variants, d_text);
        BT_CHECK_LAUNCH();
    }
    BT_HIP(hipStreamSynchronize(st));
    return BT_OK;
}

}  // namespace bt

extern "C" {

int bt_genotype_text_sizes(bt_ctx *ctx, const uint32_t *d_words, uint64_t num_words, uint64_t *text_bytes, uint64_t *index_words) {
    return bt_genotype_text(ctx, d_words, num_words, nullptr, 0, nullptr, 0, text_bytes, index_words, nullptr);
}

int bt_genotype_text(bt_ctx *ctx, const uint32_t *d_words, uint64_t num_words, uint8_t *d_text, uint64_t text_capacity, uint32_t *d_index, uint64_t index_capacity,
                     uint64_t *text_bytes, uint64_t *index_words, uint32_t *num_not_covered) {
    const bool sizes_only = !d_text && !d_index && !text_capacity && !index_capacity;
    const char *who = sizes_only ? "bt_genotype_text_sizes" : "bt_genotype_text";
    if (!ctx || !d_words || !text_bytes || !index_words) return fail(std::string(who) + ": null argument");
    BT_HIP(hipSetDevice(ctx->device));
    bt::GenoTextShape sh;
    int rc = bt::geno_text_shape(ctx, d_words, num_words, sh, who);
    if (rc != BT_OK) return rc;
    uint32_t *d_work = nullptr;   // the index is counted here: a text buffer that proves too small must leave the caller's index as it was
    struct Free {
        uint32_t *&p;
        ~Free() {
            if (p) (void)hipFree(p);
        }
    } fr{d_work};
    BT_HIP(hipMalloc(reinterpret_cast<void **>(&d_work), sh.index_words * 4));
    uint64_t total = 0;
    uint32_t not_covered = 0;
    rc = bt::geno_text_count(ctx, d_words, sh, d_work, &total, &not_covered, who);
    if (rc != BT_OK) return rc;
    *text_bytes = total;
    *index_words = sh.index_words;
    if (num_not_covered) *num_not_covered = not_covered;
    if (sizes_only) return BT_OK;
    if (!d_index || index_capacity < sh.index_words || (total && !d_text) || text_capacity < total) return fail("bt_genotype_text: buffer too small");
    BT_HIP(hipMemcpyAsync(d_index, d_work, sh.index_words * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return bt::geno_text_write(ctx, d_words, sh, d_index, d_text);
}

int bt_diag_genotype_text(const uint32_t *h_words, uint64_t num_words, uint8_t *h_text, uint64_t text_capacity, uint32_t *h_index, uint64_t index_capacity, uint64_t *text_bytes,
                          uint64_t *index_words, uint32_t *num_not_covered) {
    const char *who = "bt_diag_genotype_text";
    if (!h_words || !text_bytes || !index_words || !num_not_covered) return fail("bt_diag_genotype_text: null argument");
    if (num_words < 4) return fail("bt_diag_genotype_text: the record string is shorter than its head");
    bt::GenoTextShape sh;
    int rc = check_head(who, h_words, num_words, nullptr, sh);
    if (rc == BT_OK) rc = check_head(who, h_words, num_words, h_words + 4, sh);
    if (rc != BT_OK) return rc;
    const uint32_t C = sh.C, NV = sh.NV, S = sh.S;
    std::vector<uint32_t> index(sh.index_words, 0);
    index[0] = C;
    index[1] = NV;
    index[2] = S;
    std::memcpy(index.data() + kIndexHead, h_words + 4, ((size_t)C + 1) * 4);
    const uint32_t *voff = h_words + sh.at_voff;
    uint32_t *variants = index.data() + index_variants_at(C), *cells = index.data() + index_cells_at(C, NV);
    uint64_t total = 0;
    uint32_t not_covered = 0, all_flags = 0;
    for (uint32_t gv = 0; gv < NV; ++gv) {
        for (uint32_t s = 0; s < S; ++s) count_cell(h_words, voff, gv, s, cells + 2ull * ((uint64_t)gv * S + s));
        uint32_t *iv = variants + (uint64_t)kVariantWords * gv;
        const uint32_t flags = count_variant(h_words, voff, gv, S, iv, cells + 2ull * gv * S);
        all_flags |= flags;
        if (flags & kFlagNotCovered) ++not_covered;
        iv[IV_OFF_LO] = (uint32_t)total;
        iv[IV_OFF_HI] = (uint32_t)(total >> 32);
        total += (uint64_t)iv[IV_LEN_STATS] + iv[IV_LEN_COVER] + iv[IV_LEN_SAMPLES];
    }
    if (all_flags & kFlagMalformed) return fail("bt_diag_genotype_text: a variant record does not have the layout of bt_gibbs_genotypes' string");
    index[3] = not_covered;
    *text_bytes = total;
    *index_words = sh.index_words;
    *num_not_covered = not_covered;
    if (!h_index || index_capacity < sh.index_words || (total && !h_text) || text_capacity < total) return fail("bt_diag_genotype_text: buffer too small");
    for (uint32_t gv = 0; gv < NV; ++gv) {
        const uint32_t *iv = variants + (uint64_t)kVariantWords * gv;
        for (uint32_t s = 0; s < S; ++s) write_cell(h_words, voff, gv, s, iv, cells + 2ull * ((uint64_t)gv * S + s), h_text);
        write_variant(h_words, voff, gv, iv, h_text);
    }
    std::memcpy(h_index, index.data(), sh.index_words * 4);
    return BT_OK;
}

int bt_diag_format_g6(const double *h_values, uint64_t n, char *h_text16, int32_t *h_len) {
    if ((n && (!h_values || !h_text16)) || !h_len) return fail("bt_diag_format_g6: null argument");
    for (uint64_t i = 0; i < n; ++i) {
        unsigned char buf[16] = {0};
        StoreSink o(buf);
        const bool ok = format_g6(o, h_values[i]);
        o.finish();
        std::memcpy(h_text16 + 16 * i, buf, 16);
        h_len[i] = ok ? (int32_t)o.count() : -1;
    }
    return BT_OK;
}

}  // extern "C"
