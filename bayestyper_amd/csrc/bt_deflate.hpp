// A deflate compressor (RFC 1951) written once for the host and the device: deflate_piece_kernel (bt_deflate.hip) runs deflate_piece<WaveTeam>, one 64-thread
// workgroup = one wavefront per piece; bt_diag_deflate and tools/deflate_selfcheck.cpp run deflate_piece<LaneTeam>, a team of one thread, over the same
// lines.  The bytes are a function of the content alone.
//
// The input is cut into pieces of kPiece = 64 KiB.  No piece carries history from the one before it.  A piece becomes
//   one dynamic-Huffman block, or (when that would not be smaller) stored blocks of at most 65535 bytes,
//   then an EMPTY STORED BLOCK that closes it on a byte boundary (pigz's sync flush; what Z_SYNC_FLUSH leaves), BFINAL set in the last piece of a stream.
// So the pieces' bytes laid end to end are one raw deflate stream, and a piece is at most piece_bound(len) bytes.
//
// One piece, one team.  All data that passes between the lanes goes through `Shared` (LDS on the device) with a team barrier in between; a lane's
// private values of a round live in Shared's per-slot arrays, so that the team of one thread runs the 64 slots of a round one after the other.
//   (a) matching, in rounds of kRound = 64 positions: the slot of position p hashes the kMinMatch bytes at p, reads the head table (the latest earlier
//       position with that hash, from the rounds BEFORE this one), drops a candidate further back than 32768, and extends it 8 bytes at a time up to 258.
//       After the round every position enters the table with a maximum: the result does not depend on the order in which the lanes arrive.
//   (b) the greedy parse of the round, the same on every lane: ballot of the slots with a match, first set bit at or after the cursor, skip its length.
//       Tokens go to the piece's token area (a 32-bit word each), symbol counts into the histogram with integer adds.
//   (c) code lengths: symbols ranked by (count, symbol) in parallel, then on one lane Moffat & Katajainen's in-place minimum-redundancy lengths, folded
//       to the limit (15; 7 for the code-length code) with a Kraft repair, and canonical codes.  An alphabet with fewer than two symbols in use gets two
//       (zlib's rule), so a piece without a match still carries a complete distance code.  Code lengths are written one by one (no symbols 16-18).
//   (d) emission in rounds of 64 items: bit lengths, an exclusive scan, bits OR-ed into a window in Shared whose complete words are then stored.
// Every loop is bounded by the piece size, an alphabet size, 258 or 64; a bound that fails or a block that does not end where its size was computed sets
// the error word.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BTD_HD __host__ __device__
#else
#define BTD_HD
#endif

namespace btdeflate {

constexpr uint32_t kPiece = 65536;      // input bytes per piece: positions inside a piece fit 16 bits
constexpr uint32_t kRound = 64;         // positions matched per round, items emitted per round
constexpr uint32_t kHashBits = 12;      // head table: 2^12 words = 16 KiB of LDS
constexpr uint32_t kMinMatch = 4, kMaxMatch = 258, kWindow = 32768;
constexpr uint32_t kNumLitLen = 286, kNumDist = 30, kDistAt = 288, kHist = 320;   // histogram / code arrays: literal-length symbols at 0, distance symbols at 288
constexpr uint32_t kStoredMax = 65535;
constexpr uint32_t kRecWords = 5;       // per-piece record: out bytes, stored (0/1), literals, matches, matched bytes
constexpr uint32_t kWinWords = 104;     // 31 carried bits + 64 items of at most 48 bits = 97 words, + 2 words a last item may spill into
enum : uint32_t { kErrKraft = 1, kErrBlockEnd = 2, kErrTokens = 4, kErrCapacity = 8 };

BTD_HD inline uint32_t stored_bytes(uint32_t n) { return n + 5u * ((n + kStoredMax - 1) / kStoredMax); }
BTD_HD inline uint32_t piece_bound(uint32_t n) { return stored_bytes(n) + 5u; }   // + the closing empty block
constexpr uint32_t kPieceOut = 65552;   // piece_bound(kPiece) = 65551, rounded up to 16 bytes: the stride of the pieces' staging slots
inline uint64_t num_pieces(uint64_t n) { return n ? (n + kPiece - 1) / kPiece : 1; }
inline uint64_t stream_bound(uint64_t n) {
    const uint64_t full = n / kPiece, rem = n % kPiece;
    return full * piece_bound(kPiece) + ((rem || !n) ? piece_bound((uint32_t)rem) : 0);
}

struct Shared {
    uint32_t head[1u << kHashBits];   // position + 1 of the latest entry, 0 = none
    uint32_t hist[kHist];
    uint32_t A[288];                  // counts in rank order, then code lengths in place
    uint16_t sym[288];                // symbol of a rank
    uint16_t code[kHist];             // bit-reversed codes
    uint8_t len[kHist];
    uint32_t clfreq[20];
    uint16_t clcode[20];
    uint8_t cllen[20];
    uint32_t num[36], next_code[20];  // codes per length
    uint32_t used, forced[2];
    uint32_t hlit, hdist, hclen, dyn_bits, use_dyn;
    uint16_t mlen[kRound], mdist[kRound];
    uint32_t nb[kRound];
    uint64_t val[kRound];
    uint32_t win[kWinWords];
};

// ---- who runs a piece ---------------------------------------------------------------------------------------------------------------------------------
struct LaneTeam {
    static constexpr uint32_t W = 1;
    BTD_HD static uint32_t lane() { return 0; }
    BTD_HD static void sync() {}
    BTD_HD static uint64_t ballot_nonzero(const uint16_t *a) {
        uint64_t m = 0;
        for (uint32_t i = 0; i < kRound; ++i) m |= (uint64_t)(a[i] != 0) << i;
        return m;
    }
    BTD_HD static uint32_t exscan(uint32_t *a) {   // a[0..64) -> exclusive prefix sums; returns the total
        uint32_t run = 0;
        for (uint32_t i = 0; i < kRound; ++i) {
            const uint32_t v = a[i];
            a[i] = run;
            run += v;
        }
        return run;
    }
    BTD_HD static void add32(uint32_t *p, uint32_t v) { *p += v; }
    BTD_HD static void or32(uint32_t *p, uint32_t v) { *p |= v; }
    BTD_HD static void max32(uint32_t *p, uint32_t v) {
        if (v > *p) *p = v;
    }
};
#if defined(__HIPCC__)
struct WaveTeam {   // the 64 lanes of a one-wavefront workgroup; the pointers are LDS
    static constexpr uint32_t W = 64;
    __device__ static uint32_t lane() { return threadIdx.x; }
    __device__ static void sync() { __syncthreads(); }
    __device__ static uint64_t ballot_nonzero(const uint16_t *a) { return __ballot(a[threadIdx.x] != 0); }
    __device__ static uint32_t exscan(uint32_t *a) {
        const uint32_t v = a[threadIdx.x];
        uint32_t s = v;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(s, d, 64);
            if (threadIdx.x >= d) s += o;
        }
        a[threadIdx.x] = s - v;
        return __shfl(s, 63, 64);
    }
    __device__ static void add32(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
    __device__ static void or32(uint32_t *p, uint32_t v) { atomicOr(p, v); }
    __device__ static void max32(uint32_t *p, uint32_t v) { atomicMax(p, v); }
};
#endif

// ---- small pieces -------------------------------------------------------------------------------------------------------------------------------------
BTD_HD inline uint32_t load32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
BTD_HD inline uint64_t load64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
BTD_HD inline uint32_t hash_at(const uint8_t *p) {
    uint32_t x = load32(p);
    if (kMinMatch == 3) x &= 0xFFFFFFu;
    return (x * 2654435761u) >> (32 - kHashBits);
}
// common prefix of a and b, at most maxl bytes; both ranges lie inside the piece
BTD_HD inline uint32_t match_len(const uint8_t *a, const uint8_t *b, uint32_t maxl) {
    uint32_t l = 0;
    while (l + 8 <= maxl) {
        const uint64_t x = load64(a + l) ^ load64(b + l);
        if (x) return l + ((uint32_t)__builtin_ctzll(x) >> 3);
        l += 8;
    }
    while (l < maxl && a[l] == b[l]) ++l;
    return l;
}
BTD_HD inline uint64_t bits_from_to(uint32_t a, uint32_t b) {   // bits a .. b - 1, a <= b <= 64, a < 64
    const uint64_t below_b = b >= 64 ? ~0ull : (1ull << b) - 1;
    return below_b & ~((1ull << a) - 1);
}
// length 3..258 -> symbol 257 + code, number of extra bits, their value
BTD_HD inline void length_code(uint32_t len, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    const uint32_t l = len - 3;
    if (l < 8) {
        sym = 257 + l, eb = 0, ev = 0;
    } else if (l == 255) {
        sym = 285, eb = 0, ev = 0;
    } else {
        eb = (31 - (uint32_t)__builtin_clz(l)) - 2;
        sym = 257 + 4 * eb + 4 + ((l >> eb) & 3);
        ev = l & ((1u << eb) - 1);
    }
}
// distance 1..32768 -> code, extra bits, value
BTD_HD inline void dist_code(uint32_t dist, uint32_t &code, uint32_t &eb, uint32_t &ev) {
    const uint32_t d = dist - 1;
    if (d < 4) {
        code = d, eb = 0, ev = 0;
    } else {
        const uint32_t k = 31 - (uint32_t)__builtin_clz(d);
        eb = k - 1;
        code = 2 * k + ((d >> eb) & 1);
        ev = d & ((1u << eb) - 1);
    }
}
BTD_HD inline uint32_t litlen_extra(uint32_t s) { return (s < 265 || s == 285) ? 0 : (s - 261) / 4; }
BTD_HD inline uint32_t dist_extra(uint32_t d) { return d < 4 ? 0 : d / 2 - 1; }
BTD_HD inline uint32_t reverse_bits(uint32_t c, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) r |= ((c >> i) & 1u) << (n - 1 - i);
    return r;
}
BTD_HD inline uint32_t clen_order(uint32_t i) {   // RFC 1951 3.2.7: the order in which the code-length code's lengths are sent
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}
// token words: a literal is its byte; a match is bit 31 | (length - 3) << 15 | (distance - 1)
BTD_HD inline uint32_t match_token(uint32_t len, uint32_t dist) { return 0x80000000u | ((len - 3) << 15) | (dist - 1); }

// ---- (c) one prefix code: lengths limited to maxbits and canonical codes for freq[0..nsym) ------------------------------------------------------------
template <class T>
BTD_HD inline void build_code(Shared &sh, uint32_t *freq, uint32_t nsym, uint32_t maxbits, uint8_t *len, uint16_t *code, uint32_t *error) {
    if (T::lane() == 0) {   // at least two symbols in use, so that the code is complete
        uint32_t used = 0, first = 0;
        for (uint32_t s = 0; s < nsym; ++s)
            if (freq[s]) {
                if (!used) first = s;
                ++used;
            }
        sh.forced[0] = sh.forced[1] = nsym;
        if (used == 0) sh.forced[0] = 0, sh.forced[1] = 1;
        else if (used == 1) sh.forced[0] = first ? 0 : 1;
        for (uint32_t j = 0; j < 2; ++j)
            if (sh.forced[j] < nsym) freq[sh.forced[j]] = 1, ++used;
        sh.used = used;
    }
    T::sync();
    for (uint32_t s = T::lane(); s < nsym; s += T::W) {   // rank by (count, symbol)
        len[s] = 0;
        const uint32_t f = freq[s];
        if (!f) continue;
        uint32_t r = 0;
        for (uint32_t t = 0; t < nsym; ++t) {
            const uint32_t g = freq[t];
            r += (g != 0 && (g < f || (g == f && t < s))) ? 1u : 0u;
        }
        sh.sym[r] = (uint16_t)s;
        sh.A[r] = f;
    }
    T::sync();
    if (T::lane() == 0) {
        const int n = (int)sh.used;
        uint32_t *A = sh.A;
        // Moffat & Katajainen, "In-place calculation of minimum-redundancy codes": counts ascending in A -> code lengths, non-increasing
        A[0] += A[1];
        int root = 0, leaf = 2, next;
        for (next = 1; next < n - 1; ++next) {
            if (leaf >= n || A[root] < A[leaf]) {
                A[next] = A[root];
                A[root++] = (uint32_t)next;
            } else
                A[next] = A[leaf++];
            if (leaf >= n || (root < next && A[root] < A[leaf])) {
                A[next] += A[root];
                A[root++] = (uint32_t)next;
            } else
                A[next] += A[leaf++];
        }
        A[n - 2] = 0;
        for (next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
        int avbl = 1, used = 0, dpth = 0;
        root = n - 2;
        next = n - 1;
        for (int guard = 0; avbl > 0 && guard <= n; ++guard) {
            while (root >= 0 && (int)A[root] == dpth) ++used, --root;
            while (avbl > used && next >= 0) A[next--] = (uint32_t)dpth, --avbl;
            avbl = 2 * used;
            ++dpth;
            used = 0;
        }
        if (next >= 0) T::or32(error, kErrKraft);
        // lengths above the limit fold into it; the Kraft sum is repaired by lengthening the shortest codes that can give
        for (uint32_t l = 0; l <= maxbits; ++l) sh.num[l] = 0;
        for (int i = 0; i < n; ++i) ++sh.num[A[i] < maxbits ? A[i] : maxbits];
        uint32_t total = 0;
        for (uint32_t l = maxbits; l >= 1; --l) total += sh.num[l] << (maxbits - l);
        for (int guard = 0; total > (1u << maxbits) && guard <= n; ++guard) {
            --sh.num[maxbits];
            for (uint32_t l = maxbits - 1; l >= 1; --l)
                if (sh.num[l]) {
                    --sh.num[l];
                    sh.num[l + 1] += 2;
                    break;
                }
            --total;
        }
        if (total != (1u << maxbits)) T::or32(error, kErrKraft);
        int at = 0;   // rank 0 is the rarest symbol: it takes the longest code
        for (uint32_t l = maxbits; l >= 1; --l)
            for (uint32_t c = 0; c < sh.num[l] && at < n; ++c) len[sh.sym[at++]] = (uint8_t)l;
        uint32_t c = 0;
        sh.num[0] = 0;
        for (uint32_t l = 1; l <= maxbits; ++l) {
            c = (c + sh.num[l - 1]) << 1;
            sh.next_code[l] = c;
        }
        for (uint32_t s = 0; s < nsym; ++s)
            if (len[s]) code[s] = (uint16_t)reverse_bits(sh.next_code[len[s]]++, len[s]);
        for (uint32_t j = 0; j < 2; ++j)
            if (sh.forced[j] < nsym) freq[sh.forced[j]] = 0;   // the counts again say what the block holds
    }
    T::sync();
}

// ---- (d) the bit writer: sh.val[i] / sh.nb[i] of the 64 slots appended at bitpos ----------------------------------------------------------------------
template <class T>
BTD_HD inline void put_round(Shared &sh, uint32_t *out32, uint32_t &bitpos) {
    T::sync();
    const uint32_t total = T::exscan(sh.nb);
    T::sync();
    const uint32_t w0 = bitpos >> 5, s0 = bitpos & 31;
    for (uint32_t i = T::lane(); i < kRound; i += T::W) {
        const uint64_t v = sh.val[i];
        if (!v) continue;   // OR-ing nothing
        const uint32_t o = s0 + sh.nb[i], w = o >> 5, s = o & 31;
        const uint64_t hi = (v >> 1) >> (31 - s);
        T::or32(&sh.win[w], (uint32_t)(v << s));
        if ((uint32_t)hi) T::or32(&sh.win[w + 1], (uint32_t)hi);
        if (hi >> 32) T::or32(&sh.win[w + 2], (uint32_t)(hi >> 32));
    }
    T::sync();
    const uint32_t newpos = bitpos + total, nfull = (newpos >> 5) - w0;   // nfull <= 97
    for (uint32_t j = T::lane(); j < nfull; j += T::W) out32[w0 + j] = sh.win[j];
    const uint32_t carry = sh.win[nfull];
    T::sync();
    for (uint32_t j = T::lane(); j <= nfull + 2 && j < kWinWords; j += T::W) sh.win[j] = j == 0 ? carry : 0;
    T::sync();
    bitpos = newpos;
}

// ---- one piece ----------------------------------------------------------------------------------------------------------------------------------------
// in[0..n): the piece; tokens: kPiece words; out: kPieceOut bytes, 4-byte aligned; rec: kRecWords words
template <class T>
BTD_HD inline void deflate_piece(Shared &sh, const uint8_t *in, uint32_t n, bool final_piece, uint32_t *tokens, uint8_t *out, uint32_t *rec, uint32_t *error) {
    for (uint32_t i = T::lane(); i < (1u << kHashBits); i += T::W) sh.head[i] = 0;
    for (uint32_t i = T::lane(); i < kHist; i += T::W) sh.hist[i] = 0;
    for (uint32_t i = T::lane(); i < kWinWords; i += T::W) sh.win[i] = 0;
    T::sync();
    uint32_t next = 0, ntok = 0, nlit = 0, nmat = 0, matched = 0;
    for (uint32_t base = 0; base < n; base += kRound) {
        // (a) a candidate per position
        for (uint32_t i = T::lane(); i < kRound; i += T::W) {
            const uint32_t p = base + i;
            uint32_t L = 0, D = 0;
            if (p >= next && p + kMinMatch <= n) {
                const uint32_t c1 = sh.head[hash_at(in + p)];
                if (c1 && p - (c1 - 1) <= kWindow) {
                    D = p - (c1 - 1);
                    const uint32_t room = n - p;
                    L = match_len(in + (c1 - 1), in + p, room < kMaxMatch ? room : kMaxMatch);
                    if (L < kMinMatch) L = 0;
                }
            }
            sh.mlen[i] = (uint16_t)L;
            sh.mdist[i] = (uint16_t)(D - 1);
        }
        T::sync();
        for (uint32_t i = T::lane(); i < kRound; i += T::W) {
            const uint32_t p = base + i;
            if (p + kMinMatch <= n) T::max32(&sh.head[hash_at(in + p)], p + 1);
        }
        // (b) the parse, the same on every lane
        const uint64_t m = T::ballot_nonzero(sh.mlen);
        const uint32_t lim = n - base < kRound ? n - base : kRound;
        uint32_t cur = next > base ? next - base : 0;
        uint64_t lit = 0, mat = 0;
        for (uint32_t guard = 0; cur < lim && guard < kRound; ++guard) {
            const uint64_t rest = m & bits_from_to(cur, lim);
            if (!rest) {
                lit |= bits_from_to(cur, lim);
                cur = lim;
                break;
            }
            const uint32_t q = (uint32_t)__builtin_ctzll(rest);
            lit |= bits_from_to(cur, q);
            mat |= 1ull << q;
            const uint32_t L = sh.mlen[q];
            matched += L;
            cur = q + L;
        }
        next = base + cur;
        const uint64_t emit = lit | mat;
        for (uint32_t i = T::lane(); i < kRound; i += T::W) {
            if (!((emit >> i) & 1)) continue;
            const uint32_t at = ntok + (uint32_t)__builtin_popcountll(emit & ((1ull << i) - 1));
            if (at >= kPiece) continue;
            if ((mat >> i) & 1) {
                const uint32_t L = sh.mlen[i], D = (uint32_t)sh.mdist[i] + 1;
                uint32_t ls, dc, eb, ev;
                length_code(L, ls, eb, ev);
                dist_code(D, dc, eb, ev);
                tokens[at] = match_token(L, D);
                T::add32(&sh.hist[ls], 1);
                T::add32(&sh.hist[kDistAt + dc], 1);
            } else {
                const uint32_t b = in[base + i];
                tokens[at] = b;
                T::add32(&sh.hist[b], 1);
            }
        }
        ntok += (uint32_t)__builtin_popcountll(emit);
        nlit += (uint32_t)__builtin_popcountll(lit);
        nmat += (uint32_t)__builtin_popcountll(mat);
        T::sync();
    }
    if (ntok > kPiece || nlit + matched != n) {
        if (T::lane() == 0) T::or32(error, kErrTokens);
        ntok = 0;
        n = 0;
    }
    bool use_dyn = false;
    if (n) {
        // (c) the piece's codes and what the dynamic block would cost
        if (T::lane() == 0) sh.hist[256] = 1;
        T::sync();
        build_code<T>(sh, sh.hist, kNumLitLen, 15, sh.len, sh.code, error);
        build_code<T>(sh, sh.hist + kDistAt, kNumDist, 15, sh.len + kDistAt, sh.code + kDistAt, error);
        if (T::lane() == 0) {
            uint32_t hlit = 257, hdist = 1;
            for (uint32_t s = 257; s < kNumLitLen; ++s)
                if (sh.len[s]) hlit = s + 1;
            for (uint32_t d = 1; d < kNumDist; ++d)
                if (sh.len[kDistAt + d]) hdist = d + 1;
            for (uint32_t l = 0; l < 19; ++l) sh.clfreq[l] = 0;
            for (uint32_t s = 0; s < hlit; ++s) ++sh.clfreq[sh.len[s]];
            for (uint32_t d = 0; d < hdist; ++d) ++sh.clfreq[sh.len[kDistAt + d]];
            sh.hlit = hlit;
            sh.hdist = hdist;
        }
        T::sync();
        build_code<T>(sh, sh.clfreq, 19, 7, sh.cllen, sh.clcode, error);
        if (T::lane() == 0) {
            uint32_t hclen = 4;
            for (uint32_t i = 4; i < 19; ++i)
                if (sh.cllen[clen_order(i)]) hclen = i + 1;
            uint32_t bits = 3 + 5 + 5 + 4 + 3 * hclen;
            for (uint32_t l = 0; l < 16; ++l) bits += sh.clfreq[l] * sh.cllen[l];
            for (uint32_t s = 0; s < kNumLitLen; ++s) bits += sh.hist[s] * (sh.len[s] + litlen_extra(s));
            for (uint32_t d = 0; d < kNumDist; ++d) bits += sh.hist[kDistAt + d] * (sh.len[kDistAt + d] + dist_extra(d));
            sh.hclen = hclen;
            sh.dyn_bits = bits;
            sh.use_dyn = (bits + 7) / 8 < stored_bytes(n) ? 1u : 0u;   // (e) the stored fallback bounds a piece by piece_bound(n)
        }
        T::sync();
        use_dyn = sh.use_dyn != 0;
    }
    uint32_t out_bytes = 0;
    if (use_dyn) {
        uint32_t *out32 = reinterpret_cast<uint32_t *>(out);
        uint32_t bitpos = 0;
        const uint32_t hlit = sh.hlit, hdist = sh.hdist, hclen = sh.hclen;
        // the block header: BFINAL 0, BTYPE 10, HLIT, HDIST, HCLEN, the code-length code's lengths
        for (uint32_t i = T::lane(); i < kRound; i += T::W) {
            uint64_t v = 0;
            uint32_t nb = 0;
            if (i == 0) v = (2u << 1) | ((hlit - 257) << 3) | ((hdist - 1) << 8) | ((hclen - 4) << 13), nb = 17;
            else if (i <= hclen) v = sh.cllen[clen_order(i - 1)], nb = 3;
            sh.val[i] = v;
            sh.nb[i] = nb;
        }
        put_round<T>(sh, out32, bitpos);
        for (uint32_t j0 = 0; j0 < hlit + hdist; j0 += kRound) {   // the two codes' lengths, one by one
            for (uint32_t i = T::lane(); i < kRound; i += T::W) {
                const uint32_t j = j0 + i;
                uint64_t v = 0;
                uint32_t nb = 0;
                if (j < hlit + hdist) {
                    const uint32_t l = j < hlit ? sh.len[j] : sh.len[kDistAt + j - hlit];
                    v = sh.clcode[l], nb = sh.cllen[l];
                }
                sh.val[i] = v;
                sh.nb[i] = nb;
            }
            put_round<T>(sh, out32, bitpos);
        }
        for (uint32_t t0 = 0; t0 <= ntok; t0 += kRound) {   // the tokens, then the end-of-block symbol
            for (uint32_t i = T::lane(); i < kRound; i += T::W) {
                const uint32_t t = t0 + i;
                uint64_t v = 0;
                uint32_t nb = 0;
                if (t < ntok) {
                    const uint32_t tok = tokens[t];
                    if (tok & 0x80000000u) {
                        uint32_t ls, leb, lev, dc, deb, dev;
                        length_code(((tok >> 15) & 0xFFu) + 3, ls, leb, lev);
                        dist_code((tok & 0x7FFFu) + 1, dc, deb, dev);
                        v = sh.code[ls], nb = sh.len[ls];
                        v |= (uint64_t)lev << nb, nb += leb;
                        v |= (uint64_t)sh.code[kDistAt + dc] << nb, nb += sh.len[kDistAt + dc];
                        v |= (uint64_t)dev << nb, nb += deb;
                    } else
                        v = sh.code[tok], nb = sh.len[tok];
                } else if (t == ntok)
                    v = sh.code[256], nb = sh.len[256];
                sh.val[i] = v;
                sh.nb[i] = nb;
            }
            put_round<T>(sh, out32, bitpos);
        }
        if (bitpos != sh.dyn_bits && T::lane() == 0) T::or32(error, kErrBlockEnd);
        // the closing empty stored block: BFINAL, BTYPE 00, padding to the byte, LEN 0, NLEN ffff
        const uint32_t pad = (8 - ((bitpos + 3) & 7)) & 7;
        for (uint32_t i = T::lane(); i < kRound; i += T::W) {
            sh.val[i] = i == 0 ? ((final_piece ? 1ull : 0ull) | (0xFFFFull << (3 + pad + 16))) : 0;
            sh.nb[i] = i == 0 ? 3 + pad + 32 : 0;
        }
        put_round<T>(sh, out32, bitpos);
        if ((bitpos & 31) && T::lane() == 0) out32[bitpos >> 5] = sh.win[0];
        out_bytes = bitpos >> 3;
    } else {
        uint32_t o = 0;
        for (uint32_t off = 0; off < n; off += kStoredMax) {
            const uint32_t len = n - off < kStoredMax ? n - off : kStoredMax;
            if (T::lane() == 0) {
                out[o] = 0;
                out[o + 1] = (uint8_t)len, out[o + 2] = (uint8_t)(len >> 8);
                out[o + 3] = (uint8_t)~len, out[o + 4] = (uint8_t)(~len >> 8);
            }
            for (uint32_t j = T::lane(); j < len; j += T::W) out[o + 5 + j] = in[off + j];
            o += 5 + len;
        }
        if (T::lane() == 0) {
            out[o] = final_piece ? 1 : 0;
            out[o + 1] = 0, out[o + 2] = 0, out[o + 3] = 0xFF, out[o + 4] = 0xFF;
        }
        out_bytes = o + 5;
    }
    if (T::lane() == 0) {
        rec[0] = out_bytes;
        rec[1] = use_dyn ? 0u : 1u;
        rec[2] = nlit;
        rec[3] = nmat;
        rec[4] = matched;
    }
}

}  // namespace btdeflate
