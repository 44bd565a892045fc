// BAM alignment records (SAM specification section 4.2) -> the reads text of bt_reads_window.hpp (the bases of a read, then '\n'), written once for the
// host and the device: the kernels of bt_bam.hip and the host run (bt_diag_bam_reads_text, tools/bam_host_check.cpp) read a record through the same
// functions.  Only what the text needs is looked at: block_size chains the records, flag selects them, l_seq and the 4-bit sequence give the bases.
//   A record: block_size (4 bytes), then block_size bytes: refID, pos, l_read_name (1), mapq (1), bin (2), n_cigar_op (2), flag (2), l_seq (4), next_refID,
//   next_pos, tlen — 32 bytes — read_name [l_read_name], cigar [4 * n_cigar_op], seq [(l_seq + 1) / 2], qual [l_seq], auxiliary fields to the end.
//   Everything is little-endian and nothing is aligned, so fields are read byte-wise (rd16 / rd32).
// The 4-bit codes 1, 2, 4, 8 are A, C, G, T; every other code ('=', the IUPAC sets, N) becomes 'N', which ends a window in the reads kernels as it does
// in the FASTA / FASTQ text.  Reverse-strand records store the reverse complement; canonical k-mers do not care, so nothing is flipped.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BTB_HD __host__ __device__
#else
#define BTB_HD
#endif

namespace btbam {

constexpr uint32_t kFixed = 32;          // the fixed fields behind block_size
constexpr uint32_t kHead = 4 + kFixed;   // what has to be there for a record to be checked

enum : uint32_t { kRecOk = 0, kRecShort = 1, kRecNegative = 2 };   // block_size below what its own fields need; negative l_seq

BTB_HD inline uint32_t rd16(const uint8_t *p) { return p[0] | ((uint32_t)p[1] << 8); }
BTB_HD inline uint32_t rd32(const uint8_t *p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

struct Record {
    uint32_t block_size, flag, l_seq, seq_at;   // seq_at: offset of the packed sequence from the record's first byte
};

// rec[0..avail): the bytes from a record's start on, avail >= 4.  With fewer than kHead bytes only block_size is judged.
BTB_HD inline uint32_t read_record(const uint8_t *rec, uint64_t avail, Record &r) {
    r.block_size = rd32(rec);
    r.flag = r.l_seq = r.seq_at = 0;
    if (r.block_size < kFixed || r.block_size > 0x7FFFFFFFu) return kRecShort;
    if (avail < kHead) return kRecOk;
    const uint32_t l_read_name = rec[12], n_cigar_op = rd16(rec + 16);
    r.flag = rd16(rec + 18);
    r.l_seq = rd32(rec + 20);
    if (r.l_seq > 0x7FFFFFFFu) return kRecNegative;
    r.seq_at = kHead + l_read_name + 4 * n_cigar_op;
    const uint64_t need = (uint64_t)kFixed + l_read_name + 4ull * n_cigar_op + (r.l_seq + 1ull) / 2 + r.l_seq;
    return r.block_size < need ? kRecShort : kRecOk;
}

BTB_HD inline uint8_t base_char(uint32_t code) { return code == 1 ? 'A' : code == 2 ? 'C' : code == 4 ? 'G' : code == 8 ? 'T' : 'N'; }
// base i of a packed sequence: the high nibble comes first
BTB_HD inline uint8_t base_at(const uint8_t *seq, uint32_t i) { return base_char((seq[i >> 1] >> ((~i & 1u) << 2)) & 15u); }

inline const char *record_error_text(uint32_t e) { return e == kRecNegative ? "negative l_seq" : "block_size smaller than the record's own fields"; }

// The walk on one host thread, record by record: what the kernels of bt_bam.hip compute.  err != kRecOk: the record at err_offset fails; too_small: the
// text does not fit the capacity (nothing is written past it).
struct HostText {
    uint64_t text_bytes = 0, consumed = 0, kept = 0, skipped = 0, bases = 0, err_offset = 0;
    uint32_t err = kRecOk;
    bool too_small = false;
};
inline HostText reads_text_host(const uint8_t *bam, uint64_t len, uint32_t skip_flags, char *text, uint64_t capacity) {
    HostText t;
    uint64_t at = 0, out = 0;
    while (len - at >= 4) {
        Record r;
        const uint32_t e = read_record(bam + at, len - at, r);
        if (e != kRecOk) {
            t.err = e;
            t.err_offset = at;
            return t;
        }
        if (4ull + r.block_size > len - at) break;
        if (r.flag & skip_flags)
            ++t.skipped;
        else {
            if (out + r.l_seq + 1ull > capacity) {
                t.too_small = true;
                return t;
            }
            const uint8_t *seq = bam + at + r.seq_at;
            for (uint32_t j = 0; j < r.l_seq; ++j) text[out + j] = (char)base_at(seq, j);
            text[out + r.l_seq] = '\n';
            out += r.l_seq + 1ull;
            ++t.kept;
            t.bases += r.l_seq;
        }
        at += 4ull + r.block_size;
    }
    t.text_bytes = out;
    t.consumed = at;
    return t;
}

}  // namespace btbam
