// The part of a stream object that is BGZF and nothing else (bt_bam_scan, bt_fastq_scan): slabs of whole compressed blocks from the host, through a pinned
// staging slot (the context's when they are large enough), inflated on the device (bt_inflate.hip) behind the tail the call before left, the text buffer beside
// them.  What the data is — BAM records, FASTQ lines — is the owner's business: it reads d_raw, writes d_text and says with keep_tail what waits for the next call.
// `who` names the owner's entry point in the messages.  Implemented in bt_inflate.hip.
#pragma once
#include <cstdint>
#include <vector>

#include "bt_internal.hpp"

namespace bt {

struct BgzfStream {
    bt_ctx *ctx = nullptr;
    uint64_t max_in_bytes = 0;
    uint8_t *pin[2] = {nullptr, nullptr}, *dev[2] = {nullptr, nullptr};   // the staging slots: the context's when they are large enough
    size_t stage_bytes = 0;
    uint64_t calls = 0;
    std::vector<bt_bgzf_block> blocks;
    bt_bgzf_block *d_blocks = nullptr;
    uint32_t *d_status = nullptr;
    uint64_t cap_blocks = 0;
    uint8_t *d_raw = nullptr, *d_tail = nullptr;
    char *d_text = nullptr;
    uint64_t cap_raw = 0, cap_tail = 0, cap_text = 0;
    uint64_t tail = 0;          // bytes that wait in d_tail for the next call
    uint64_t file_offset = 0;   // compressed bytes taken so far

    // max_in_bytes must lie in 64 KiB .. 1 GiB.  After a failure release() still has to run.
    int create(const char *who, bt_ctx *ctx, uint64_t max_in_bytes);
    // h_blocks [n_bytes] (whole blocks) -> d_raw [*raw]: the tail, then the blocks' data; d_text has room for *raw bytes.  Complete on return.
    int inflate_slab(const char *who, const uint8_t *h_blocks, uint64_t n_bytes, uint64_t *raw);
    // from [rest] (in d_raw) waits in d_tail for the next call
    int keep_tail(const uint8_t *from, uint64_t rest);
    // the slots go (back) to the context when they are whole and no smaller than what it holds
    void release();
};

// device memory of at least `need` bytes behind *p (contents are not kept)
int grow(void **p, uint64_t *cap, uint64_t need);

}  // namespace bt
