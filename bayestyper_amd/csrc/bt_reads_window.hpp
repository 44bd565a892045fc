// The window code of the reads scan (bt_reads.hip), written once over a team and a consumer, as bt_gz_pipeline.hpp is over its formats:
//   a tile of a reads text -> 2-bit codes in the team's buffer (halo k-1) -> every lane walks a run of consecutive positions, the forward and the
//   reverse-complement k-mer and their ntHash words rolled by one base per step -> consume(canonical k-mer, its hash, end position).
// A reads text is ASCII bases, one read per line: every byte outside ACGTacgt (nt_code's rule: N, the newline, anything else) ends the window, so no
// k-mer spans two reads.  The team is a workgroup with the codes in LDS on the device and a single thread on the host (bt_diag_reads_kmers, the
// stand-alone host check): the k-mers and hashes the tests compare against their brute-force restatement come out of the code the kernels run.
#pragma once
#include <stdint.h>

#include "bt_kmer_device.hpp"
#include "bt_reads_pack.hpp"

namespace bt {

constexpr unsigned READS_MAX_HALO = 63;   // k - 1 for k <= 64

// What a launch knows about k before it starts: the hash words of the all-A window (the state every lane starts from) and the rotation constants.
struct RollConst {
    unsigned k;
    uint64_t h_all_a, h_all_t;   // nthash64 of A^k and of T^k (the reverse complement of A^k)
    Kmer mask;                   // the low 2k bits
};
inline RollConst make_roll_const(unsigned k) {
    RollConst c;
    c.k = k;
    c.mask = kmer_mask(Kmer{~0ULL, ~0ULL}, k);
    c.h_all_a = nthash64(Kmer{0, 0}, k);
    c.h_all_t = nthash64(c.mask, k);
    return c;
}

// The window ending at the last byte rolled in.  A byte outside the alphabet enters as A and clears `valid`, so the four words always describe k real
// codes — the base that leaves is nucleotide 0 of fw, no second read of the text — and a lane "re-seeds" simply by rolling on: the window counts again once k
// valid bases have entered behind the invalid one.
struct RollState {
    Kmer fw, rc;         // nucleotide i at bits (2i, 2i + 1), as everywhere (bt_kmer_device.hpp)
    uint64_t hf, hr;     // nthash64(fw, k), nthash64(rc, k)
    unsigned valid;      // valid bases at the end of the window, saturated at k
};
__host__ __device__ inline RollState roll_start(const RollConst &c) { return RollState{Kmer{0, 0}, c.mask, c.h_all_a, c.h_all_t, 0u}; }

// code: 0..3, or 0xFF for a byte outside the alphabet
__host__ __device__ inline void roll_step(RollState &s, const RollConst &c, uint8_t code) {
    const unsigned k = c.k;
    const bool ok = code != 0xFFu;
    const unsigned in = ok ? (unsigned)code : 0u;
    const unsigned out = (unsigned)(s.fw.lo & 3u);
    s.valid = ok ? (s.valid < k ? s.valid + 1u : k) : 0u;
    // nthash64 in Horner form is XOR_i rol(seed[c_i], k - 1 - i): the forward word loses rol(seed[out], k - 1), turns by one and takes seed[in] at rotation 0;
    // the reverse word holds seed[3 - c_i] at rotation i: it loses seed[3 - out] at rotation 0, turns back by one and takes seed[3 - in] at rotation k - 1
    s.hf = rol64(s.hf, 1) ^ rol64(nt_seed(out), k) ^ nt_seed(in);
    const uint64_t r = s.hr ^ nt_seed(3u - out);
    s.hr = ((r >> 1) | (r << 63)) ^ rol64(nt_seed(3u - in), k - 1u);
    // forward k-mer: nucleotide 0 leaves at the low end, the new one enters at position k - 1; reverse complement: the other way round
    s.fw.lo = (s.fw.lo >> 2) | (s.fw.hi << 62);
    s.fw.hi >>= 2;
    if (k <= 32u) s.fw.lo |= (uint64_t)in << (2u * (k - 1u));
    else s.fw.hi |= (uint64_t)in << (2u * (k - 33u));
    s.rc.hi = ((s.rc.hi << 2) | (s.rc.lo >> 62)) & c.mask.hi;
    s.rc.lo = ((s.rc.lo << 2) | (uint64_t)(3u - in)) & c.mask.lo;
}

// the canonical k-mer of a full window (kmer_canonical's order: ties return the forward k-mer) and its hash, picked by strand
__host__ __device__ inline Kmer roll_canonical(const RollState &s, uint64_t *h) {
    const bool use_rc = kmer_lex_less(s.rc, s.fw);
    *h = use_rc ? s.hr : s.hf;
    return use_rc ? s.rc : s.fw;
}

// One lane's walk over its run of a tile, as the packed front end calls it: run[i] is the code of position run_start - halo + i.  The first halo steps fill the
// window; every later step that completes a window of k valid bases ending at or after first_end is consumed.  It restates the walk inside reads_front_end line
// for line: routing the text front end through this function too changed the text kernels' device code (register allocation and address arithmetic), so that one
// keeps its walk in place.
template <unsigned run_len, class Consume>
__host__ __device__ __attribute__((always_inline)) inline void reads_walk_run(const uint8_t *run, uint64_t run_start, uint64_t len, uint64_t first_end, const RollConst &c, Consume &consume) {
    const unsigned halo = c.k - 1u;
    RollState s = roll_start(c);
    for (unsigned i = 0; i < halo; ++i) roll_step(s, c, run[i]);
    const uint64_t n = len - run_start < run_len ? len - run_start : run_len;
    for (uint64_t i = 0; i < n; ++i) {
        roll_step(s, c, run[halo + i]);
        if (s.valid == c.k && run_start + i >= first_end) {
            uint64_t h;
            const Kmer can = roll_canonical(s, &h);
            consume(can, h, run_start + i);
        }
    }
}

// The front end.  Team: LANES, RUN (start positions a lane walks per tile), lane(), first_tile(), tile_stride(), codes() (LANES * RUN + READS_MAX_HALO
// bytes shared by the team), sync().  consume(canonical, hash, end): called once for every window of k valid bases that ENDS at text[end], first_end <= end < len
// (first_end > 0: the caller has consumed the windows ending before it with an earlier slab that overlaps this one by k - 1 bytes).
template <class Team, class Consume>
__host__ __device__ inline void reads_front_end(Team &team, const char *__restrict__ text, uint64_t len, uint64_t first_end, const RollConst &c, Consume &consume) {
    constexpr uint64_t TILE = (uint64_t)Team::LANES * Team::RUN;
    const unsigned halo = c.k - 1u;
    uint8_t *codes = team.codes();
    const uint64_t num_tiles = (len + TILE - 1) / TILE;
    for (uint64_t tile = team.first_tile(); tile < num_tiles; tile += team.tile_stride()) {
        const uint64_t tile_start = tile * TILE;
        // codes[j] is the byte at tile_start - halo + j
        for (uint64_t j = team.lane(); j < TILE + halo; j += Team::LANES) {
            uint8_t code = 0xFFu;
            if (tile_start + j >= halo && tile_start + j - halo < len) {
                const int v = nt_code(text[tile_start + j - halo]);
                code = v < 0 ? 0xFFu : (uint8_t)v;
            }
            codes[j] = code;
        }
        team.sync();
        const uint64_t run_start = tile_start + (uint64_t)team.lane() * Team::RUN;
        if (run_start < len && run_start + Team::RUN > first_end) {
            const uint8_t *run = codes + (uint64_t)team.lane() * Team::RUN;   // run[i]: the byte at run_start - halo + i
            RollState s = roll_start(c);
            for (unsigned i = 0; i < halo; ++i) roll_step(s, c, run[i]);
            const uint64_t n = len - run_start < Team::RUN ? len - run_start : Team::RUN;
            for (uint64_t i = 0; i < n; ++i) {
                roll_step(s, c, run[halo + i]);
                if (s.valid == c.k && run_start + i >= first_end) {
                    uint64_t h;
                    const Kmer can = roll_canonical(s, &h);
                    consume(can, h, run_start + i);
                }
            }
        }
        team.sync();
    }
}

// The sibling over a packed text (bt_reads_pack.hpp): the same walk, another tile fill.  A tile is a whole number of 128-position blocks, so it starts on a
// block boundary and the halo (k - 1 <= 63) lies in the one block before it: the team's image is laid out from position tile_start - 64, and every
// 16-position word expands to 16 code bytes (0xFF where invalid or at and beyond `positions`) stored at a 16-byte-aligned address.  Team::codes(): LANES * RUN
// + READS_PACKED_LEAD bytes, 16-byte aligned.  `packed` holds reads_packed_bytes(positions) bytes; its padding bits are never trusted.
constexpr unsigned READS_PACKED_LEAD = 64;
struct alignas(16) CodeBytes16 {
    uint32_t w[4];
};
template <class Team, class Consume>
__host__ __device__ inline void reads_front_end_packed(Team &team, const uint32_t *__restrict__ packed, uint64_t positions, uint64_t first_end, const RollConst &c, Consume &consume) {
    constexpr uint64_t TILE = (uint64_t)Team::LANES * Team::RUN;
    static_assert(TILE % PACK_BLOCK_POSITIONS == 0 && READS_PACKED_LEAD > READS_MAX_HALO && READS_PACKED_LEAD % PACK_WORD_POSITIONS == 0, "a tile is whole blocks");
    constexpr unsigned LEAD_WORDS = READS_PACKED_LEAD / PACK_WORD_POSITIONS, IMAGE_WORDS = (unsigned)(TILE / PACK_WORD_POSITIONS) + LEAD_WORDS;
    const unsigned halo = c.k - 1u;
    uint8_t *codes = team.codes();
    const uint64_t num_tiles = (positions + TILE - 1) / TILE;
    for (uint64_t tile = team.first_tile(); tile < num_tiles; tile += team.tile_stride()) {
        const uint64_t tile_start = tile * TILE, tile_word = tile_start / PACK_WORD_POSITIONS;
        // codes[j] is the code of position tile_start - 64 + j
        for (unsigned w = team.lane(); w < IMAGE_WORDS; w += Team::LANES) {
            CodeBytes16 q;
            if (tile_word + w < LEAD_WORDS) q.w[0] = q.w[1] = q.w[2] = q.w[3] = 0xFFFFFFFFu;   // before the text
            else packed_word_code_bytes(packed, tile_word + w - LEAD_WORDS, positions, q.w);
            *reinterpret_cast<CodeBytes16 *>(codes + (size_t)w * PACK_WORD_POSITIONS) = q;
        }
        team.sync();
        const uint64_t run_start = tile_start + (uint64_t)team.lane() * Team::RUN;
        if (run_start < positions && run_start + Team::RUN > first_end)
            reads_walk_run<Team::RUN>(codes + (READS_PACKED_LEAD - halo) + (uint64_t)team.lane() * Team::RUN, run_start, positions, first_end, c, consume);
        team.sync();
    }
}

// a team of one host thread
struct HostTeam {
    static constexpr unsigned LANES = 1, RUN = 4096;
    uint8_t buf[RUN + READS_MAX_HALO];
    unsigned lane() const { return 0; }
    uint64_t first_tile() const { return 0; }
    uint64_t tile_stride() const { return 1; }
    uint8_t *codes() { return buf; }
    void sync() {}
};
struct PackedHostTeam {   // RUN: a whole number of 128-position blocks
    static constexpr unsigned LANES = 1, RUN = 4096;
    alignas(16) uint8_t buf[RUN + READS_PACKED_LEAD];
    unsigned lane() const { return 0; }
    uint64_t first_tile() const { return 0; }
    uint64_t tile_stride() const { return 1; }
    uint8_t *codes() { return buf; }
    void sync() {}
};

// the sketch's hash of a k-mer hash, and the register it names and the rank it brings (2^16 one-byte registers)
__host__ __device__ inline uint64_t splitmix64_finalise(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
constexpr unsigned SKETCH_BITS = 16;
constexpr uint32_t SKETCH_REGISTERS = 1u << SKETCH_BITS;
__host__ __device__ inline void sketch_slot(uint64_t kmer_hash, uint32_t *reg, uint32_t *rank) {
    const uint64_t x = splitmix64_finalise(kmer_hash);
    *reg = (uint32_t)(x >> (64u - SKETCH_BITS));
    const uint64_t rest = x << SKETCH_BITS;   // the remaining 48 bits at the top, zeros below
    *rank = 1u + (rest ? (unsigned)__builtin_clzll(rest) : 64u - SKETCH_BITS);   // 1 .. 49
}

}  // namespace bt
