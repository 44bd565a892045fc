// The packed form of a reads text (bt_reads_pack / bt_reads_unpack, the *_packed consumers of bt_reads.hip, the reads pack file): what reads_front_end makes
// of every byte before it does anything else — a 2-bit code or "not a base" — stored instead of the byte.  One text for the device and the host.
//
// A reads text of n bytes becomes ceil(n / 128) blocks of 48 bytes (12 little-endian 32-bit words); block b covers positions 128 b .. 128 b + 127:
//   words 0 - 7    the codes: position j of the block in word j / 16, bits 2 (j % 16) and up
//   words 8 - 11   the validity bits: position j in word 8 + j / 32, bit j % 32
// nt_code's rule: ACGTacgt give 0..3 and valid, every other byte code 0 and invalid; positions at and beyond n in the last block are written as code 0,
// invalid.  Position for position, no compaction: a pure map that needs no scan.  The inverse gives the canonical text: upper-case bases, every invalid
// position a newline.
#pragma once
#include <stdint.h>

#include "bt_kmer_device.hpp"

namespace bt {

constexpr unsigned PACK_BLOCK_POSITIONS = 128, PACK_BLOCK_WORDS = 12, PACK_BLOCK_BYTES = 4 * PACK_BLOCK_WORDS, PACK_WORD_POSITIONS = 16;

__host__ __device__ inline uint64_t reads_packed_blocks(uint64_t n) { return n / PACK_BLOCK_POSITIONS + (n % PACK_BLOCK_POSITIONS != 0); }
__host__ __device__ inline uint64_t reads_packed_bytes(uint64_t n) { return reads_packed_blocks(n) * PACK_BLOCK_BYTES; }

// where the 16-position word w (positions 16 w .. 16 w + 15) keeps its codes, and where and at which bit its 16 validity bits
__host__ __device__ inline uint64_t pack_codes_index(uint64_t w) { return (w >> 3) * PACK_BLOCK_WORDS + (w & 7u); }
__host__ __device__ inline uint64_t pack_valid_index(uint64_t w) { return (w >> 3) * PACK_BLOCK_WORDS + 8u + ((w & 7u) >> 1); }
__host__ __device__ inline unsigned pack_valid_shift(uint64_t w) { return (unsigned)(w & 1u) * 16u; }

// m <= 16 bytes -> their codes word and validity bits (the positions from m on: code 0, invalid)
__host__ __device__ inline void pack_word(const char *bytes, unsigned m, uint32_t *codes, uint32_t *valid) {
    uint32_t c = 0, v = 0;
    for (unsigned i = 0; i < m; ++i) {
        const int code = nt_code(bytes[i]);
        if (code >= 0) {
            c |= (uint32_t)code << (2u * i);
            v |= 1u << i;
        }
    }
    *codes = c;
    *valid = v;
}

// the inverse: 16 characters of the canonical text
__host__ __device__ inline void unpack_word(uint32_t codes, uint32_t valid, char *out16) {
    for (unsigned i = 0; i < PACK_WORD_POSITIONS; ++i) {
        const unsigned code = (codes >> (2u * i)) & 3u;
        out16[i] = (valid >> i) & 1u ? (char)(code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : 'T') : '\n';
    }
}

// 16 positions as 16 code bytes in four words (byte i of the 16 = position i): the code, or 0xFF where the validity bit is clear, whatever the code bits say
__host__ __device__ inline void pack_word_code_bytes(uint32_t codes, uint32_t valid, uint32_t out[4]) {
    for (unsigned q = 0; q < 4; ++q) {
        const uint32_t c = (codes >> (8u * q)) & 0xFFu, v = (valid >> (4u * q)) & 0xFu;
        const uint32_t spread = (c | (c << 6) | (c << 12) | (c << 18)) & 0x03030303u;
        const uint32_t ok = (v | (v << 7) | (v << 14) | (v << 21)) & 0x01010101u;
        out[q] = spread | ((ok ^ 0x01010101u) * 0xFFu);
    }
}

// The code bytes of word w of a packed text of `positions` positions, w < ceil(positions / 16) not required: a word at or beyond the end is all 0xFF (nothing
// is loaded), and so is every position at and beyond `positions` of the last word, whatever the padding bits say.
__host__ __device__ inline void packed_word_code_bytes(const uint32_t *__restrict__ packed, uint64_t w, uint64_t positions, uint32_t out[4]) {
    const uint64_t p0 = w * PACK_WORD_POSITIONS;
    if (p0 >= positions) {
        out[0] = out[1] = out[2] = out[3] = 0xFFFFFFFFu;
        return;
    }
    uint32_t valid = (packed[pack_valid_index(w)] >> pack_valid_shift(w)) & 0xFFFFu;
    if (positions - p0 < PACK_WORD_POSITIONS) valid &= (1u << (unsigned)(positions - p0)) - 1u;
    pack_word_code_bytes(packed[pack_codes_index(w)], valid, out);
}

// the whole map on one host thread (bt_diag_reads_pack, the host layer's -p threads, the stand-alone host check); packed: reads_packed_bytes(n) bytes
inline void reads_pack_host(const char *text, uint64_t n, uint32_t *packed) {
    const uint64_t words = reads_packed_blocks(n) * 8u;
    for (uint64_t w = 0; w < words; w += 2) {
        uint32_t v[2];
        for (unsigned h = 0; h < 2; ++h) {
            const uint64_t p0 = (w + h) * PACK_WORD_POSITIONS;
            const unsigned m = p0 >= n ? 0u : n - p0 < PACK_WORD_POSITIONS ? (unsigned)(n - p0) : PACK_WORD_POSITIONS;
            pack_word(text + (m ? p0 : 0), m, &packed[pack_codes_index(w + h)], &v[h]);
        }
        packed[pack_valid_index(w)] = v[0] | (v[1] << 16);
    }
}
inline void reads_unpack_host(const uint32_t *packed, uint64_t positions, char *text) {
    for (uint64_t w = 0; w * PACK_WORD_POSITIONS < positions; ++w) {
        char out[PACK_WORD_POSITIONS];
        unpack_word(packed[pack_codes_index(w)], (packed[pack_valid_index(w)] >> pack_valid_shift(w)) & 0xFFFFu, out);
        const uint64_t p0 = w * PACK_WORD_POSITIONS;
        for (unsigned i = 0; i < PACK_WORD_POSITIONS && p0 + i < positions; ++i) text[p0 + i] = out[i];
    }
}

}  // namespace bt
