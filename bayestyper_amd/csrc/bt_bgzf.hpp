// BGZF (the blocked gzip of the SAM specification, section 4.1) over the compressor of bt_deflate.hpp, written once for the host and the device:
// bgzf_block_kernel (bt_bgzf.hip) runs bgzf_block<WaveTeam>, one wavefront per block; bt_diag_bgzf, bt_diag_crc32 and tools/bgzf_selfcheck.cpp run
// bgzf_block<LaneTeam>, a team of one thread, over the same lines.
//
// The content is cut into blocks of kBlock = 65280 input bytes (htslib's size).  A block's payload is deflate_piece with final_piece set — a complete raw
// deflate stream of at most piece_bound(65280) = 65290 bytes — so a block is at most 65316 bytes, below the format's 65536.  Around it go 18 bytes of
// header (frame_byte), the CRC-32 of the block's input and its length.
//
// crc32_team: zlib's crc32 (reflected polynomial edb88320) by the team that compressed the block, from ONE 256-entry table in Shared (1 KiB of LDS; gfx950
// has no carry-less multiply).  CRC-32 without its two complements is linear over GF(2): the register after A || B is the register after A advanced over
// |B| zero bytes, XOR the register after B alone — and advancing over k zero bytes is a multiplication by x^(8k) mod P (crc_mul: 32 shift-and-XOR steps,
// zlib's multmodp; the operators are compile-time constants).
//   The block is seen as rows of 64 segments of 16 bytes, ALIGNED FROM ITS END: row r, slot s holds the bytes at n - (rows - r) * 1024 + 16 s.  A row is
//   1 KiB contiguous, so the wavefront's loads are coalesced (a lane-contiguous split of the block would have every load instruction touch 64 cache
//   lines).  What is missing in front of the first row counts as zero bytes: they leave a zero register zero.
//   Slot s runs its column top to bottom: register advanced over the 1008 bytes between two of its segments, then 16 table steps.  The initial
//   complement is the register ffffffff set right before byte 0, by the one slot that holds byte 0.
//   Then six pairing levels: a slot's register advanced over the 16 d bytes of its right neighbour's span, XOR the neighbour's.  Aligned from the end,
//   no operator depends on the block's length.  The final complement is taken once.
// Every loop is bounded by 64, 32, 16 or 256.
#pragma once
#include "bt_deflate.hpp"

namespace btbgzf {

using namespace btdeflate;

constexpr uint32_t kBlock = 65280;                     // input bytes per block
constexpr uint32_t kHeader = 18, kTrailer = 8, kFrame = kHeader + kTrailer, kEof = 28;
constexpr uint32_t kBlockMax = 65536;                  // the format's limit: BSIZE is 16 bits
constexpr uint32_t kBlockRecWords = 8;                     // per-block record: deflate_piece's five words, [5] CRC-32 of the input, [6] its length, [7] unused
constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcSeg = 16, kCrcRow = kRound * kCrcSeg;

inline uint64_t num_blocks(uint64_t n) { return (n + kBlock - 1) / kBlock; }
BTD_HD inline uint32_t block_bound(uint32_t n) { return piece_bound(n) + kFrame; }
inline uint64_t bgzf_bound(uint64_t n) {   // the data blocks and the EOF block
    const uint64_t full = n / kBlock, rem = n % kBlock;
    return full * block_bound(kBlock) + (rem ? block_bound((uint32_t)rem) : 0) + kEof;
}
static_assert(kBlock + 5 * 2 + kFrame <= kBlockMax, "a stored block must fit BSIZE");

// byte i < 18 of a block's header; bsize = the block's total size - 1
BTD_HD inline uint8_t frame_byte(uint32_t i, uint32_t bsize) {
    const uint8_t fixed[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    return i < 16 ? fixed[i] : (uint8_t)(bsize >> (8 * (i - 16)));
}
// the canonical empty block that ends a BGZF file (htslib writes these bytes; the compressor's empty piece is a stored block, which is not this form)
BTD_HD inline uint8_t eof_byte(uint32_t i) {
    const uint8_t eof[kEof] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return eof[i];
}

// ---- CRC-32 ---------------------------------------------------------------------------------------------------------------------------------------------
struct CrcShared {
    uint32_t table[256];
    uint32_t part[kRound];
};

constexpr uint32_t crc_times_x(uint32_t b) { return (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u); }
// x^(8 bytes) mod P, bit 31 = x^0: the operator that advances a register over `bytes` zero bytes
constexpr uint32_t crc_xpow8(uint32_t bytes) {
    uint32_t b = 0x80000000u;
    for (uint32_t i = 0; i < 8 * bytes; ++i) b = crc_times_x(b);
    return b;
}
// a * b mod P (zlib's multmodp without its early exit): a is an operator, b a register
BTD_HD inline uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32; ++i) {
        p ^= (a & (0x80000000u >> i)) ? b : 0u;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}
BTD_HD inline uint32_t crc_level(uint32_t level) {   // advance over the 16 << level bytes of the right neighbour's span
    constexpr uint32_t op[6] = {crc_xpow8(16), crc_xpow8(32), crc_xpow8(64), crc_xpow8(128), crc_xpow8(256), crc_xpow8(512)};
    return op[level];
}

// CRC-32 of in[0..n), n <= 65536 (64 rows), the same value on every lane
template <class T>
BTD_HD inline uint32_t crc32_team(CrcShared &cs, const uint8_t *in, uint32_t n) {
    constexpr uint32_t kNextRow = crc_xpow8(kCrcRow - kCrcSeg);
    T::sync();   // (whoever read part[] of the block before is done)
    for (uint32_t i = T::lane(); i < 256; i += T::W) {
        uint32_t c = i;
        for (uint32_t k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? kCrcPoly : 0u);
        cs.table[i] = c;
    }
    T::sync();
    const uint32_t rows = n > kPiece ? 0u : (n + kCrcRow - 1) / kCrcRow;
    for (uint32_t slot = T::lane(); slot < kRound; slot += T::W) {
        uint32_t s = 0;
        for (uint32_t r = 0; r < rows; ++r) {
            const int32_t off = (int32_t)n - (int32_t)((rows - r) * kCrcRow) + (int32_t)(slot * kCrcSeg);
            if (off <= -(int32_t)kCrcSeg) continue;   // all in front of the block
            if (off > 0) {
                s = crc_mul(kNextRow, s);
                uint64_t w[2] = {load64(in + off), load64(in + off + 8)};
                for (uint32_t h = 0; h < 2; ++h)
                    for (uint32_t j = 0; j < 8; ++j) {
                        s = cs.table[(s ^ (uint32_t)w[h]) & 0xFFu] ^ (s >> 8);
                        w[h] >>= 8;
                    }
            } else {   // the segment that holds byte 0: the register is still zero
                s = 0xFFFFFFFFu;   // the initial complement
                for (uint32_t j = (uint32_t)(-off); j < kCrcSeg; ++j) s = cs.table[(s ^ in[(uint32_t)(off + (int32_t)j)]) & 0xFFu] ^ (s >> 8);
            }
        }
        cs.part[slot] = s;
    }
    for (uint32_t level = 0, d = 1; d < kRound; d <<= 1, ++level) {
        T::sync();
        for (uint32_t slot = T::lane(); slot < kRound; slot += T::W)
            if ((slot & (2 * d - 1)) == 0) cs.part[slot] = crc_mul(crc_level(level), cs.part[slot]) ^ cs.part[slot + d];
    }
    T::sync();
    return n ? ~cs.part[0] : 0u;
}

// ---- one block: payload into the staging slot, record with CRC and length ---------------------------------------------------------------------------------
// in[0..n), 1 <= n <= kBlock; tokens: kPiece words; out: kPieceOut bytes, 4-byte aligned; rec: kBlockRecWords words
template <class T>
BTD_HD inline void bgzf_block(Shared &sh, CrcShared &cs, const uint8_t *in, uint32_t n, uint32_t *tokens, uint8_t *out, uint32_t *rec, uint32_t *error) {
    deflate_piece<T>(sh, in, n, true, tokens, out, rec, error);
    const uint32_t crc = crc32_team<T>(cs, in, n);
    if (T::lane() == 0) {
        rec[5] = crc;
        rec[6] = n;
        rec[7] = 0;
    }
}

}  // namespace btbgzf
