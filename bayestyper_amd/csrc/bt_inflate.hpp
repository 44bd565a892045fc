// A raw-deflate decoder (RFC 1951) and the BGZF block reader over it (SAM specification section 4.1), written once for the host and the device:
// bgzf_inflate_kernel (bt_inflate.hip) runs inflate_block<WaveTeam>, one 64-thread workgroup = one wavefront per BGZF block; bt_diag_bgzf_inflate and
// tools/bam_host_check.cpp run inflate_block<LaneTeam>, a team of one thread, over the same lines.  The reading half of bt_bgzf.hpp.
//
// One block, one team.  Blocks are independent: nothing here waits on another team.
//   Symbol decoding is serial, and every lane runs it: the bit buffer, the positions and the status are functions of the input alone, so they hold the
//   same values on all lanes and every branch is uniform.  Lane 0 stores the literals and the short match copies.
//   What the other lanes add: zeroing and filling the decode tables, the bytes of stored blocks, match copies of kWideCopy bytes and more, the CRC-32.
//   A byte one lane stored is read by another lane only across a team barrier.
// Decode tables (in Shared, LDS on the device): codes of up to kLitBits / kDistBits bits resolve in one lookup of the next bits; longer codes (rare) walk
//   the canonical code length by length over count[] / sym[] (the symbols ordered by code).  An entry is symbol << 4 | length, 0 = no code.
//
// Damaged input is an error, never a fault or a hang:
//   every load of the payload is below its end, every store below the block's ISIZE (checked before it is made);
//   every turn of a loop consumes at least one input bit or produces at least one output byte, so a block takes at most 8 * payload + ISIZE turns;
//   the first failing condition is the block's status (Status below), and nothing is decoded after it.
#pragma once
#include "bt_bgzf.hpp"

namespace btinflate {

using btdeflate::LaneTeam;
using btdeflate::load32;
using btdeflate::load64;
#if defined(__HIPCC__)
using btdeflate::WaveTeam;
#endif

constexpr uint32_t kLitBits = 10, kDistBits = 8;   // one-lookup code lengths
constexpr uint32_t kMaxBits = 15, kNumLit = 288, kNumDist = 32, kNumClen = 19;
constexpr uint32_t kWideCopy = 24;                 // a match at least this long is copied by the team
constexpr uint32_t kMaxIsize = 65536;              // SAM 4.1: a block holds at most 2^16 bytes of data

enum Status : uint32_t {
    kOk = 0,
    kBadHeader,        // the block's gzip header (re-read on the device) does not frame a payload inside the block
    kBadBlockType,     // reserved block type 3, or a stored block whose LEN and NLEN disagree
    kBadCodeSet,       // an over-subscribed or incomplete code set
    kBadCodeLengths,   // more than 286 / 30 codes, a repeat with nothing to repeat or past the last code, no end-of-block code
    kBadSymbol,        // length symbol 286 / 287, distance symbol 30 / 31, or bits that are no code of the set
    kBadDistance,      // a distance reaching before the block's own output
    kInputEnd,         // the stream runs past the payload's end
    kTrailing,         // the stream ends before the payload's end
    kBadLength,        // output length != ISIZE
    kBadCrc,           // CRC-32 mismatch
    kBadTable,         // the block table's entry lies outside the input or the output
    kBadStreamDistance,   // (bt_gunzip.hpp) a distance reaching before the first byte of a gzip member, or of the window handed in
    kNumStatus
};
inline const char *status_text(uint32_t s) {
    const char *text[kNumStatus] = {"ok",
                                    "bad gzip header",
                                    "reserved deflate block type or stored length check",
                                    "over-subscribed or incomplete code set",
                                    "invalid code lengths",
                                    "invalid length or distance symbol",
                                    "distance reaches before the block's output",
                                    "deflate stream runs past the payload's end",
                                    "deflate stream ends before the payload's end",
                                    "output length differs from ISIZE",
                                    "CRC-32 mismatch",
                                    "block table entry out of range",
                                    "distance reaches before the stream's start"};
    return s < kNumStatus ? text[s] : "unknown status";
}

struct Shared {
    uint16_t lit[1u << kLitBits];     // also the code-length code's table while a dynamic header is read (7 bits)
    uint16_t dist[1u << kDistBits];
    uint16_t lsym[kNumLit], dsym[kNumDist];   // symbols in code order
    uint16_t lcount[kMaxBits + 1], dcount[kMaxBits + 1];
    uint16_t code[kNumLit];           // a set's canonical codes while its table is filled
    uint16_t offs[kMaxBits + 2], next[kMaxBits + 2];
    uint8_t len[kNumLit + kNumDist];  // code lengths: literal-length symbols, then distance symbols
    uint8_t cllen[kNumClen + 1];
    uint32_t built;                   // Status of the set lane 0 just counted
};

struct Bits {
    const uint8_t *in;
    uint32_t n, pos;     // payload length; next byte to load
    uint64_t buf;
    int32_t cnt;         // valid bits in buf; negative once more bits were taken than the payload holds
    BTD_HD void refill() {
        if (cnt < 0) return;
        if (pos + 8 <= n) {
            buf |= load64(in + pos) << cnt;
            pos += (uint32_t)(63 - cnt) >> 3;
            cnt |= 56;
        } else
            while (cnt <= 56 && pos < n) {
                buf |= (uint64_t)in[pos++] << cnt;
                cnt += 8;
            }
    }
    BTD_HD uint32_t peek(uint32_t nb) const { return (uint32_t)buf & ((1u << nb) - 1u); }
    BTD_HD void drop(uint32_t nb) {
        buf >>= nb;
        cnt -= (int32_t)nb;
    }
    BTD_HD uint32_t take(uint32_t nb) {
        const uint32_t v = peek(nb);
        drop(nb);
        return v;
    }
};

BTD_HD inline uint32_t reverse_bits(uint32_t c, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) r |= ((c >> i) & 1u) << (n - 1 - i);
    return r;
}

// One prefix code from len[0..n): table (1 << fast entries), sym / count for the longer codes.  zlib's rules: over-subscribed is an error; incomplete
// is an error unless the set is a single code of one bit (a distance code set of a single code); an empty set is accepted when allow_empty (a block of
// literals alone needs no distance code) and then every lookup fails.
template <class T>
BTD_HD inline uint32_t build_table(Shared &sh, const uint8_t *len, uint32_t n, uint16_t *table, uint32_t fast, uint16_t *sym, uint16_t *count, bool allow_empty) {
    T::sync();   // (whoever read the table before is done)
    for (uint32_t i = T::lane(); i < (1u << fast); i += T::W) table[i] = 0;
    if (T::lane() == 0) {
        for (uint32_t l = 0; l <= kMaxBits; ++l) count[l] = 0;
        for (uint32_t s = 0; s < n; ++s) ++count[len[s]];
        uint32_t status = kOk, maxlen = 0;
        int32_t left = 1;
        for (uint32_t l = 1; l <= kMaxBits; ++l) {
            left = left * 2 - (int32_t)count[l];
            if (left < 0) break;
            if (count[l]) maxlen = l;
        }
        if (left < 0) status = kBadCodeSet;
        else if (left > 0 && !(maxlen == 1 || (maxlen == 0 && allow_empty))) status = kBadCodeSet;
        if (status == kOk) {
            uint16_t *offs = sh.offs, *next = sh.next;
            uint32_t c = 0;
            offs[1] = 0;
            count[0] = 0;   // (unused symbols have no code)
            for (uint32_t l = 1; l <= kMaxBits; ++l) {
                c = (c + count[l - 1]) << 1;
                next[l] = (uint16_t)c;
                offs[l + 1] = (uint16_t)(offs[l] + count[l]);
            }
            for (uint32_t s = 0; s < n; ++s) {
                const uint32_t l = len[s];
                if (!l) continue;
                sym[offs[l]++] = (uint16_t)s;
                sh.code[s] = next[l]++;
            }
        }
        sh.built = status;
    }
    T::sync();
    const uint32_t status = sh.built;
    if (status != kOk) return status;
    for (uint32_t s = T::lane(); s < n; s += T::W) {
        const uint32_t l = len[s];
        if (!l || l > fast) continue;
        for (uint32_t e = reverse_bits(sh.code[s], l); e < (1u << fast); e += 1u << l) table[e] = (uint16_t)((s << 4) | l);
    }
    T::sync();
    return kOk;
}

// the next symbol of a code: its bits are dropped; kNoSymbol when the next bits are no code of the set
constexpr uint32_t kNoSymbol = 0xFFFFu;
BTD_HD inline uint32_t decode(Bits &b, const uint16_t *table, uint32_t fast, const uint16_t *sym, const uint16_t *count) {
    const uint32_t e = table[b.peek(fast)];
    if (e) {
        b.drop(e & 15u);
        return e >> 4;
    }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= kMaxBits; ++l) {
        code |= (uint32_t)(b.buf >> (l - 1)) & 1u;
        const uint32_t c = count[l];
        if (code < first + c) {
            b.drop(l);
            return sym[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return kNoSymbol;
}

// decode() fails only in a set that is not complete: a single code of one bit, or no code at all (build_table accepts no other).  There the first bit alone
// says that no code follows (zlib's entry for it is one bit long), so a failure with one bit of input in the buffer is damage and not the input's end.
BTD_HD inline uint32_t no_symbol_status(const Bits &b) { return b.cnt < 1 ? kInputEnd : kBadSymbol; }

// The two decode tables of a fixed (type 1, RFC 1951 3.2.6) or dynamic (type 2, 3.2.7: its header is read from b) block.  The same status on every lane.
template <class T>
BTD_HD inline uint32_t block_tables(Shared &sh, Bits &b, uint32_t type) {
    uint32_t nlit = kNumLit, ndist = kNumDist;
    if (type == 1) {   // RFC 1951 3.2.6
        for (uint32_t s = T::lane(); s < kNumLit + kNumDist; s += T::W) sh.len[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
    } else {           // 3.2.7
        nlit = b.take(5) + 257;
        ndist = b.take(5) + 1;
        const uint32_t nclen = b.take(4) + 4;
        if (b.cnt < 0) return kInputEnd;
        if (nlit > 286 || ndist > 30) return kBadCodeLengths;
        for (uint32_t i = 0; i < kNumClen; ++i) {
            uint32_t v = 0;
            if (i < nclen) {
                b.refill();
                v = b.take(3);
            }
            if (T::lane() == 0) sh.cllen[btdeflate::clen_order(i)] = (uint8_t)v;
        }
        if (b.cnt < 0) return kInputEnd;
        const uint32_t st = build_table<T>(sh, sh.cllen, kNumClen, sh.lit, 7, sh.lsym, sh.lcount, false);
        if (st != kOk) return st;
        uint32_t prev = 0;
        for (uint32_t i = 0; i < nlit + ndist;) {
            b.refill();
            const uint32_t s = decode(b, sh.lit, 7, sh.lsym, sh.lcount);
            if (s == kNoSymbol) return no_symbol_status(b);
            uint32_t rep = 1, v = s;
            if (s == 16) {
                if (i == 0) return kBadCodeLengths;
                v = prev, rep = 3 + b.take(2);
            } else if (s == 17)
                v = 0, rep = 3 + b.take(3);
            else if (s == 18)
                v = 0, rep = 11 + b.take(7);
            if (b.cnt < 0) return kInputEnd;
            if (rep > nlit + ndist - i) return kBadCodeLengths;
            if (T::lane() == 0)
                for (uint32_t j = 0; j < rep; ++j) {
                    const uint32_t at = i + j;
                    sh.len[at < nlit ? at : kNumLit + (at - nlit)] = (uint8_t)v;
                }
            prev = v;
            i += rep;
        }
    }
    T::sync();
    if (sh.len[256] == 0) return kBadCodeLengths;
    uint32_t st = build_table<T>(sh, sh.len, nlit, sh.lit, kLitBits, sh.lsym, sh.lcount, false);
    if (st == kOk) st = build_table<T>(sh, sh.len + kNumLit, ndist, sh.dist, kDistBits, sh.dsym, sh.dcount, true);
    return st;
}

// in[0..n): a raw deflate stream that has to end at n exactly; out[0..isize): what it has to decode to.  The same status on every lane.
template <class T>
BTD_HD inline uint32_t inflate_stream(Shared &sh, const uint8_t *in, uint32_t n, uint8_t *out, uint32_t isize) {
    Bits b{in, n, 0, 0, 0};
    uint32_t opos = 0;
    for (bool last = false; !last;) {
        b.refill();
        last = b.take(1) != 0;
        const uint32_t type = b.take(2);
        if (b.cnt < 0) return kInputEnd;
        if (type == 3) return kBadBlockType;
        if (type == 0) {   // stored: to the byte boundary, LEN, NLEN, LEN bytes
            b.drop((uint32_t)b.cnt & 7u);
            b.refill();
            const uint32_t len = b.take(16), nlen = b.take(16);
            if (b.cnt < 0) return kInputEnd;
            if ((len ^ nlen) != 0xFFFFu) return kBadBlockType;
            const uint32_t at = b.pos - ((uint32_t)b.cnt >> 3);
            if (len > n - at) return kInputEnd;
            if (len > isize - opos) return kBadLength;
            for (uint32_t i = T::lane(); i < len; i += T::W) out[opos + i] = in[at + i];
            T::sync();
            opos += len;
            b.pos = at + len;
            b.buf = 0;
            b.cnt = 0;
            continue;
        }
        const uint32_t st = block_tables<T>(sh, b, type);
        if (st != kOk) return st;
        for (;;) {   // a turn takes at most 15 + 5 + 15 + 13 = 48 bits; a refill leaves at least 56 unless the payload ends
            b.refill();
            const uint32_t s = decode(b, sh.lit, kLitBits, sh.lsym, sh.lcount);
            if (s == kNoSymbol) return no_symbol_status(b);
            if (s < 256) {
                if (b.cnt < 0) return kInputEnd;
                if (opos >= isize) return kBadLength;
                if (T::lane() == 0) out[opos] = (uint8_t)s;
                ++opos;
                continue;
            }
            if (s == 256) {
                if (b.cnt < 0) return kInputEnd;
                break;
            }
            if (s >= 286) return kBadSymbol;
            const uint32_t lc = s - 257, leb = lc < 8 || lc == 28 ? 0 : (lc >> 2) - 1;
            const uint32_t len = lc == 28 ? 258 : lc < 8 ? 3 + lc : 3 + ((4 + (lc & 3)) << leb) + b.take(leb);
            const uint32_t dc = decode(b, sh.dist, kDistBits, sh.dsym, sh.dcount);
            if (dc == kNoSymbol) return no_symbol_status(b);
            if (dc >= 30) return kBadSymbol;
            const uint32_t deb = dc < 4 ? 0 : (dc >> 1) - 1;
            const uint32_t dist = dc < 4 ? 1 + dc : 1 + ((2 + (dc & 1)) << deb) + b.take(deb);
            if (b.cnt < 0) return kInputEnd;
            if (dist > opos) return kBadDistance;
            if (len > isize - opos) return kBadLength;
            if (T::W == 1 || len < kWideCopy) {
                if (T::lane() == 0)
                    for (uint32_t i = 0; i < len; ++i) out[opos + i] = out[opos - dist + i];
            } else {   // the source of byte i lies in the dist bytes before the match, also when the copy overlaps itself
                T::sync();
                for (uint32_t i = T::lane(); i < len; i += T::W) out[opos + i] = out[opos - dist + (dist >= len ? i : i % dist)];
                T::sync();
            }
            opos += len;
        }
    }
    if (b.pos - ((uint32_t)b.cnt >> 3) != n) return kTrailing;
    if (opos != isize) return kBadLength;
    return kOk;
}

// ---- a BGZF block ---------------------------------------------------------------------------------------------------------------------------------------
// Byte i of a header, read as the field it belongs to (SAM 4.1): returns the payload's offset in the block, 0 when the header is not BGZF's.  block[0..avail)
// holds at least the 12 fixed bytes; *bsize = the BC subfield's value.  The extra field may carry other subfields beside BC.
BTD_HD inline uint32_t parse_header(const uint8_t *block, uint64_t avail, uint32_t *bsize) {
    if (avail < 12) return 0;
    if (block[0] != 0x1f || block[1] != 0x8b || block[2] != 8 || !(block[3] & 4)) return 0;   // magic, CM = deflate, FLG.FEXTRA
    if (block[3] & ~4u) return 0;   // (FNAME, FCOMMENT, FHCRC would put fields between the extra field and the payload; BGZF sets none)
    const uint32_t xlen = block[10] | ((uint32_t)block[11] << 8);
    if (12ull + xlen > avail) return 0;
    uint32_t found = 0;
    for (uint32_t at = 0; at + 4 <= xlen;) {
        const uint8_t *f = block + 12 + at;
        const uint32_t slen = f[2] | ((uint32_t)f[3] << 8);
        if (at + 4 + slen > xlen) return 0;
        if (f[0] == 'B' && f[1] == 'C') {
            if (slen != 2 || found) return 0;
            *bsize = f[4] | ((uint32_t)f[5] << 8);
            found = 1;
        }
        at += 4 + slen;
    }
    return found ? 12 + xlen : 0;
}

// block[0..size): one whole BGZF block; out[0..isize): its data.  The same status on every lane.
template <class T>
BTD_HD inline uint32_t inflate_block(Shared &sh, btbgzf::CrcShared &cs, const uint8_t *block, uint32_t size, uint8_t *out, uint32_t isize) {
    uint32_t bsize = 0;
    const uint32_t at = size >= btbgzf::kFrame ? parse_header(block, size, &bsize) : 0;
    if (!at || bsize + 1 != size || at + btbgzf::kTrailer > size) return kBadHeader;
    if (isize > kMaxIsize) return kBadLength;
    const uint32_t n = size - btbgzf::kTrailer - at;
    if (load32(block + size - 4) != isize) return kBadLength;
    const uint32_t st = inflate_stream<T>(sh, block + at, n, out, isize);
    if (st != kOk) return st;
    T::sync();   // (the last bytes lane 0 stored)
    if (btbgzf::crc32_team<T>(cs, out, isize) != load32(block + size - 8)) return kBadCrc;
    return kOk;
}

}  // namespace btinflate
