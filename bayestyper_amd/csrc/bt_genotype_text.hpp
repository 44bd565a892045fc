// The genotype-derived TEXT of one variant's VCF line, formatted from its record of bt_gibbs_genotypes' word string (bt_genotypes.hpp), written once for the
// host and the device: text_cell_kernel / text_variant_kernel (bt_genotype_text.hip), bt_diag_genotype_text and bt_diag_format_g6 run this code.
// It produces what the host layer's stream insertions produce (bayestyper_amd/host/Genotypes.cpp: formatQualityFilterAndStats without QUAL and FILTER,
// formatAlleleCover, formatSampleColumns; a restatement of GenotypeWriter.cpp:84-143, 202-230, 261-345):
//   stats piece    "AC=..;AF=..;AN=..;ACP=.."
//   cover piece    ";ANC=.." (ascending alleles) or nothing
//   samples piece  per sample "\tGT:" + a GQ SLOT OF NO BYTES + ":GPP:APP:NAK:FAK:MAC:SAF", or "\t:.:.:.:.:.:." for ploidy 0 (no slot)
// GQ and QUAL are not formatted here (bt_genotypes.hpp tells why): the index carries `best` and the slot's offset, and the host splices its own digits in.
//
// Floats and doubles: the host prints both with operator<<, which is printf's %g at precision 6 of the value widened to double.  format_g6 is that
// conversion done exactly in integers:
//   v = m * 2^e with m the 53-bit significand; x = floor(log10 v) starts one above floor(log10 2^floor(log2 v)) (so it is x or x + 1) and is lowered once
//   if the scaled value turns out below 10^5; D = round-half-even(v * 10^(5 - x)) = (m * 5^a) >> k with a = 5 - x, k = -(e + a): the product is exact in
//   128 bits (5^32 < 2^75, m < 2^53), the bits shifted out are compared with the half, a tie goes to the even D, and D = 10^6 becomes 10^5 at x + 1.
// That holds for 1e-27 <= |v| < 1e6 (0 <= a <= 32, 1 <= k <= 110).  Zero prints as "0".  For anything else —
// non-finite, subnormal, outside that range — format_g6 reports NOT COVERED and emits nothing: a condition, never a guess.  The caller flags the variant.
#pragma once
#include <cstdint>

#include "bt_genotypes.hpp"

namespace btgtext {

// ---- sinks: where the characters go.  put(c) appends one byte. ------------------------------------------------------------------------------------
struct CountSink {   // the count pass
    uint64_t n = 0;
    BTG_HD inline void put(char) { ++n; }
    BTG_HD inline uint64_t count() const { return n; }
    BTG_HD inline void finish() {}
};
// The write pass.  A lane's bytes are consecutive but start anywhere, and its neighbours' bytes share its first and last dword: whole dwords that belong
// to this lane alone are assembled in a register and stored once; the bytes of a shared dword are stored one by one.
struct StoreSink {
    unsigned char *at;   // next byte
    uint64_t n = 0;
    uint32_t acc = 0, first;   // the dword being assembled; the index of its first byte that is this lane's
    BTG_HD explicit StoreSink(unsigned char *p) : at(p), first((uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u)) {}
    BTG_HD inline void put(char c) {
        const uint32_t r = (uint32_t)(reinterpret_cast<uintptr_t>(at) & 3u);
        acc |= (uint32_t)(unsigned char)c << (8u * r);
        ++at;
        ++n;
        if (r == 3u) flush(4u);
    }
    BTG_HD inline uint64_t count() const { return n; }
    BTG_HD inline void finish() {
        const uint32_t r = (uint32_t)(reinterpret_cast<uintptr_t>(at) & 3u);
        if (r != 0u) {
            at += 4u - r;   // flush() addresses the dword from its end
            flush(r);
            at -= 4u - r;
        }
    }

   private:
    BTG_HD inline void flush(uint32_t end) {   // bytes first .. end - 1 of the dword that ends at `at`
        unsigned char *dword = at - 4;
        if (first == 0u && end == 4u) *reinterpret_cast<uint32_t *>(dword) = acc;
        else
            for (uint32_t i = first; i < end; ++i) dword[i] = (unsigned char)(acc >> (8u * i));
        acc = 0;
        first = 0;
    }
};

// ---- numbers -------------------------------------------------------------------------------------------------------------------------------------------
template <class Sink>
BTG_HD inline void put_uint(Sink &o, uint32_t v) {   // operator<< of an unsigned integer
    uint32_t div = 1;
    while (v / div >= 10u) div *= 10u;
    for (; div; div /= 10u) o.put((char)('0' + (v / div) % 10u));
}

// %g at precision 6 of v (what operator<< prints for a double, and for a float through its exact widening).  Returns false, with nothing emitted, when v
// is not covered (see the head of this file).
template <class Sink>
BTG_HD inline bool format_g6(Sink &o, double v) {
    uint64_t bits;
    __builtin_memcpy(&bits, &v, 8);
    const bool neg = (bits >> 63) != 0;
    const uint32_t ef = (uint32_t)((bits >> 52) & 0x7FFu);
    const uint64_t frac = bits & 0xFFFFFFFFFFFFFull;
    if (ef == 0x7FFu) return false;          // infinity, NaN
    if (ef == 0u) {
        if (frac != 0) return false;         // subnormal
        if (neg) o.put('-');
        o.put('0');
        return true;
    }
    const double av = neg ? -v : v;
    if (!(av >= 1e-27 && av < 1e6)) return false;
    const uint64_t m = frac | (1ull << 52);
    const int e = (int)ef - 1075;            // v = m * 2^e
    const int b = (int)ef - 1023;            // floor(log2 v): -90 .. 19
    // floor(b * log10 2) for |b| < 1650 (78913 / 2^18 = 0.30102920..., the arithmetic shift floors); 2^b <= v < 2^(b + 1) < 10 * 2^b, so floor(log10 v) is this or this + 1
    int x = ((b * 78913) >> 18) + 1;
    if (x > 5) x = 5;                        // v < 10^6
    uint64_t D = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const int a = 5 - x;                 // 0 .. 32
        uint64_t p = 1;                      // 5^min(a, 27) fits 64 bits
        for (int i = 0; i < (a < 27 ? a : 27); ++i) p *= 5u;
        unsigned __int128 N = (unsigned __int128)m * p;
        for (int i = 27; i < a; ++i) N *= 5u;
        const unsigned k = (unsigned)(-(e + a));   // v * 10^a = N * 2^-k; e <= -33 and a <= 32: 1 <= k, and k <= 110 since v * 10^a >= 10^4
        D = (uint64_t)(N >> k);
        const unsigned __int128 rem = N & ((((unsigned __int128)1) << k) - 1u), half = ((unsigned __int128)1) << (k - 1u);
        const bool up = rem > half || (rem == half && (D & 1u));
        if (D < 100000u && attempt == 0) {   // floor(v * 10^(5 - x)) < 10^5: x was one too high
            --x;
            continue;
        }
        if (up) ++D;
        break;
    }
    if (D >= 1000000u) {                     // 999999.5 and its like: carried into a seventh digit
        D = 100000u;
        ++x;
    }
    uint32_t d = (uint32_t)D, nd = 6;
    while (nd > 1u && d % 10u == 0u) {       // %g strips trailing zeros
        d /= 10u;
        --nd;
    }
    // d holds the nd significant digits; digit(i) = the i-th from the left
    uint32_t top = 1;
    for (uint32_t i = 1; i < nd; ++i) top *= 10u;
    auto digit = [&](uint32_t i) -> char {
        uint32_t q = top;
        for (uint32_t j = 0; j < i; ++j) q /= 10u;
        return (char)('0' + (d / q) % 10u);
    };
    if (neg) o.put('-');
    if (x < -4 || x >= 6) {                  // d.ddddde+XX
        o.put(digit(0));
        if (nd > 1u) {
            o.put('.');
            for (uint32_t i = 1; i < nd; ++i) o.put(digit(i));
        }
        o.put('e');
        o.put(x < 0 ? '-' : '+');
        const uint32_t ax = (uint32_t)(x < 0 ? -x : x);
        o.put((char)('0' + ax / 10u));
        o.put((char)('0' + ax % 10u));
    } else if (x >= 0) {
        const uint32_t ip = (uint32_t)x + 1u;   // digits before the point
        for (uint32_t i = 0; i < ip; ++i) o.put(i < nd ? digit(i) : '0');
        if (nd > ip) {
            o.put('.');
            for (uint32_t i = ip; i < nd; ++i) o.put(digit(i));
        }
    } else {
        o.put('0');
        o.put('.');
        for (int i = -1; i > x; --i) o.put('0');
        for (uint32_t i = 0; i < nd; ++i) o.put(digit(i));
    }
    return true;
}

// ---- the index (32-bit words; include/btgpu.h: bt_genotype_text) ------------------------------------------------------------------------------------------
//   [0] C  [1] NV  [2] S  [3] number of not-covered variants     cluster_var_off [C + 1]
//   per variant, 9 words: text offset (low, high), length of the stats / cover / samples piece, A, total_count, max_alt_allele_call_probability (f32), flags
//   per cell (v * S + s), 2 words: best (f32), byte offset of the GQ slot inside the samples piece (kNoSlot: ploidy 0)
constexpr uint32_t kIndexHead = 4, kVariantWords = 9, kCellWords = 2, kNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kFlagNotCovered = 1u;   // a value of the variant is outside format_g6's range: its text is not to be used
constexpr uint32_t kFlagMalformed = 2u;    // the record does not have the layout of bt_genotypes.hpp (an entry fails on it)
enum { IV_OFF_LO = 0, IV_OFF_HI, IV_LEN_STATS, IV_LEN_COVER, IV_LEN_SAMPLES, IV_A, IV_TOTAL_COUNT, IV_MAX_ALT, IV_FLAGS };
BTG_HD inline uint64_t index_variants_at(uint32_t C) { return kIndexHead + (uint64_t)C + 1; }
BTG_HD inline uint64_t index_cells_at(uint32_t C, uint32_t NV) { return index_variants_at(C) + (uint64_t)kVariantWords * NV; }
BTG_HD inline uint64_t index_words(uint32_t C, uint32_t NV, uint32_t S) { return index_cells_at(C, NV) + (uint64_t)kCellWords * NV * S; }

// ---- the pieces --------------------------------------------------------------------------------------------------------------------------------------------
// "AC=..;AF=..;AN=..;ACP=.." of the variant record `rec`; false if a value was not covered
template <class Sink>
BTG_HD inline bool stats_piece(Sink &o, const uint32_t *rec) {
    const uint32_t A = rec[0];
    const uint32_t *al = rec + btgeno::kVariantHead;
    bool ok = true;
    o.put('A'), o.put('C'), o.put('=');
    for (uint32_t a = 1; a < A; ++a) {
        if (a > 1u) o.put(',');
        put_uint(o, al[4u * a + 1]);
    }
    o.put(';'), o.put('A'), o.put('F'), o.put('=');
    for (uint32_t a = 1; a < A; ++a) {
        if (a > 1u) o.put(',');
        ok &= format_g6(o, (double)btgeno::word_as_float(al[4u * a + 2]));
    }
    o.put(';'), o.put('A'), o.put('N'), o.put('=');
    put_uint(o, rec[1]);
    o.put(';'), o.put('A'), o.put('C'), o.put('P'), o.put('=');
    for (uint32_t a = 0; a < A; ++a) {
        if (a) o.put(',');
        ok &= format_g6(o, (double)btgeno::word_as_float(al[4u * a]));
    }
    return ok;
}
// ";ANC=a,b,.." or nothing
template <class Sink>
BTG_HD inline void cover_piece(Sink &o, const uint32_t *rec) {
    const uint32_t A = rec[0];
    const uint32_t *al = rec + btgeno::kVariantHead;
    bool any = false;
    for (uint32_t a = 0; a < A; ++a) {
        if (!al[4u * a + 3]) continue;
        if (!any) o.put(';'), o.put('A'), o.put('N'), o.put('C'), o.put('=');
        else o.put(',');
        any = true;
        put_uint(o, a);
    }
}
// one sample's columns from its sample record `sr` (ploidy <= 2 checked by the caller); *gq_slot = the number of bytes in front of the GQ slot (kNoSlot: none);
// false if a value was not covered
template <class Sink>
BTG_HD inline bool sample_piece(Sink &o, const uint32_t *sr, uint32_t A, uint32_t *gq_slot) {
    const uint32_t ploidy = sr[0];
    const uint64_t start = o.count();
    o.put('\t');
    if (ploidy == 0u) {
        o.put(':');
        for (uint32_t i = 0; i < 6u; ++i) {
            if (i) o.put(':');
            o.put('.');
        }
        *gq_slot = kNoSlot;
        return true;
    }
    const uint32_t est[2] = {sr[1] & 0xFFFFu, sr[1] >> 16};
    for (uint32_t i = 0; i < ploidy; ++i) {
        if (i) o.put('/');
        if (est[i] != btgeno::NONE) put_uint(o, est[i]);
        else o.put('.');
    }
    o.put(':');
    *gq_slot = (uint32_t)(o.count() - start);
    o.put(':');
    bool ok = true;
    const uint64_t G = btgeno::num_genotypes(A, ploidy);
    const uint32_t *p = sr + btgeno::kSampleHead;
    for (uint64_t i = 0; i < G; ++i) {
        if (i) o.put(',');
        ok &= format_g6(o, (double)btgeno::word_as_float(p[i]));
    }
    o.put(':');
    for (uint32_t a = 0; a < A; ++a) {
        if (a) o.put(',');
        ok &= format_g6(o, (double)btgeno::word_as_float(p[G + a]));
    }
    const uint32_t *mw = sr + btgeno::sample_means_at(A, ploidy);   // doubles on an even word of an 8-byte aligned string; read as two words
    for (uint32_t k = 0; k < 3u; ++k) {
        o.put(':');
        for (uint32_t a = 0; a < A; ++a) {
            if (a) o.put(',');
            const uint32_t *w = mw + 2u * (3u * a + k);
            const uint64_t bits = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
            double m;
            __builtin_memcpy(&m, &bits, 8);
            ok &= format_g6(o, m);
        }
    }
    o.put(':');
    for (uint32_t a = 0; a < A; ++a) {
        if (a) o.put(',');
        put_uint(o, p[G + A + a] & 0xFFFFu);   // the host holds the filter bits in 16 bits
    }
    return ok;
}

// The word offset of sample s's record inside the variant record of `rec_words` words, walking the records in front of it; false if a ploidy is above 2 or
// the record would end past the variant's (a string that is not bt_gibbs_genotypes').
BTG_HD inline bool sample_record_at(const uint32_t *rec, uint64_t rec_words, uint32_t s, uint64_t *at) {
    if (rec_words < btgeno::kVariantHead) return false;
    const uint32_t A = rec[0];
    if (A == 0u || A > 0xFFFFu) return false;
    uint64_t w = btgeno::variant_head_words(A);
    for (uint32_t s2 = 0;; ++s2) {
        if (w + btgeno::kSampleHead > rec_words) return false;
        const uint32_t ploidy = rec[w];
        if (ploidy > 2u) return false;
        const uint64_t n = btgeno::sample_words(A, ploidy);
        if (w + n > rec_words) return false;
        if (s2 == s) break;
        w += n;
    }
    *at = w;
    return true;
}

// ---- the two passes, one cell or one variant at a time (the kernels give a lane each; bt_diag_genotype_text loops) ------------------------------------
// var_off: the string's var_off table; iv: the variant's 9 index words; cell: the cell's 2 index words.  Between the passes a cell's words hold its flags and
// its length, then (after count_variant) its offset inside the samples piece; write_cell leaves the final `best` and GQ slot there.
BTG_HD inline void count_cell(const uint32_t *words, const uint32_t *var_off, uint32_t gv, uint32_t s, uint32_t *cell) {
    const uint32_t *rec = words + var_off[gv];
    const uint64_t rec_words = var_off[gv + 1] - var_off[gv];
    uint64_t at = 0;
    uint32_t slot = 0, flags = 0;
    CountSink o;
    if (!sample_record_at(rec, rec_words, s, &at)) flags = kFlagMalformed;
    else if (!sample_piece(o, rec + at, rec[0], &slot)) flags = kFlagNotCovered;
    if (o.count() >> 31) flags |= kFlagMalformed;   // (no record of a 2^32-word string gets there)
    cell[0] = flags;
    cell[1] = (flags & kFlagMalformed) ? 0u : (uint32_t)o.count();
}
// after count_cell of the variant's S cells (cells: their 2 S words); returns the variant's flags
BTG_HD inline uint32_t count_variant(const uint32_t *words, const uint32_t *var_off, uint32_t gv, uint32_t S, uint32_t *iv, uint32_t *cells) {
    const uint32_t *rec = words + var_off[gv];
    const uint64_t rec_words = var_off[gv + 1] - var_off[gv];
    uint32_t flags = 0;
    uint64_t at = 0;
    if (rec_words < btgeno::kVariantHead || rec[0] == 0u || rec[0] > 0xFFFFu || btgeno::variant_head_words(rec[0]) > rec_words) flags = kFlagMalformed;
    else if (S && !sample_record_at(rec, rec_words, S - 1u, &at)) flags = kFlagMalformed;
    for (uint32_t s = 0; s < S; ++s) flags |= cells[2u * s];
    uint64_t len_stats = 0, len_cover = 0, len_samples = 0;
    if (!(flags & kFlagMalformed)) {
        CountSink a, b;
        if (!stats_piece(a, rec)) flags |= kFlagNotCovered;
        cover_piece(b, rec);
        len_stats = a.count();
        len_cover = b.count();
        for (uint32_t s = 0; s < S; ++s) {
            const uint32_t len = cells[2u * s + 1];
            cells[2u * s + 1] = (uint32_t)len_samples;
            len_samples += len;
        }
        if ((len_samples | len_stats | len_cover) >> 31) {
            flags |= kFlagMalformed;
            len_stats = len_cover = len_samples = 0;
        }
    }
    iv[IV_OFF_LO] = iv[IV_OFF_HI] = 0;
    iv[IV_LEN_STATS] = (uint32_t)len_stats;
    iv[IV_LEN_COVER] = (uint32_t)len_cover;
    iv[IV_LEN_SAMPLES] = (uint32_t)len_samples;
    const bool readable = rec_words >= btgeno::kVariantHead;
    iv[IV_A] = readable ? rec[0] : 0u;
    iv[IV_TOTAL_COUNT] = readable ? rec[1] : 0u;
    iv[IV_MAX_ALT] = readable ? rec[2] : 0u;
    iv[IV_FLAGS] = flags;
    return flags;
}
BTG_HD inline uint64_t variant_text_offset(const uint32_t *iv) { return (uint64_t)iv[IV_OFF_LO] | ((uint64_t)iv[IV_OFF_HI] << 32); }
BTG_HD inline void write_cell(const uint32_t *words, const uint32_t *var_off, uint32_t gv, uint32_t s, const uint32_t *iv, uint32_t *cell, unsigned char *text) {
    if (iv[IV_FLAGS] & kFlagMalformed) return;
    const uint32_t *rec = words + var_off[gv];
    uint64_t at = 0;
    if (!sample_record_at(rec, var_off[gv + 1] - var_off[gv], s, &at)) return;
    StoreSink o(text + variant_text_offset(iv) + iv[IV_LEN_STATS] + iv[IV_LEN_COVER] + cell[1]);
    uint32_t slot = 0;
    (void)sample_piece(o, rec + at, rec[0], &slot);
    o.finish();
    cell[0] = rec[at + 2];
    cell[1] = slot == kNoSlot ? kNoSlot : cell[1] + slot;
}
BTG_HD inline void write_variant(const uint32_t *words, const uint32_t *var_off, uint32_t gv, const uint32_t *iv, unsigned char *text) {
    if (iv[IV_FLAGS] & kFlagMalformed) return;
    const uint32_t *rec = words + var_off[gv];
    StoreSink o(text + variant_text_offset(iv));
    (void)stats_piece(o, rec);
    cover_piece(o, rec);
    o.finish();
}

}  // namespace btgtext
