// The interpreter behind bt_rng_probe / bt_diag_rng_probe (include/btgpu.h): a short case program run on ONE generator of bt_rng_device.hpp, the same text
// on the device (a lane of a 64-lane case, its neighbours running theirs) and on the host (a team of one).  A test harness: no production kernel includes
// this file.  Every loop here is bounded by a count of the program; the host entry points validate the program before anything runs (probe_validate).
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/btgpu.h"
#include "bt_rng_device.hpp"

namespace bt {
namespace probe {

constexpr uint32_t LANES = 64, FINAL_WORDS = 12, TAIL_WORDS = 8, RING_WORDS = 64 + MT_RING_HDR;
constexpr uint32_t MAX_CASES = 4096, MAX_STEPS = 64, MAX_N = 2048, MAX_TOTAL = 8192, MAX_DISCARD = 3 * MT_N, MAX_SHUFFLE = 448, MAX_ROW = 1u << 16;

// a row of 32-bit output words with a capacity: a double is two words (low, high), a 64-bit ballot likewise
struct Out {
    uint32_t BT_GAS *row;
    uint32_t cap, o;
    BT_HD void put(uint32_t at, uint32_t v) const {
        if (at < cap) row[at] = v;
    }
    BT_HD void w(uint32_t v) { put(o++, v); }
    BT_HD void d(double x) {
        uint64_t b;
        memcpy(&b, &x, 8);
        w((uint32_t)b);
        w((uint32_t)(b >> 32));
    }
};

// words a step writes (the two state words after it included)
inline uint64_t step_words(const bt_rng_probe_step &s) {
    const uint64_t n = s.n, raw = s.c != 0.0 ? 1u : 0u;
    switch (s.kind) {
        case BT_PROBE_DRAW: case BT_PROBE_UNIFORM_INT: case BT_PROBE_BERNOULLI: case BT_PROBE_SHUFFLE: case BT_PROBE_DIRECT: return n + 2;
        case BT_PROBE_CANONICAL: return 2 * n + 2;
        case BT_PROBE_CANONICAL2: return 4 * n + 2;
        case BT_PROBE_NORMAL: case BT_PROBE_GAMMA: return (2 + raw) * n + 2;
        case BT_PROBE_BULK: return 3 * n + 2;
        case BT_PROBE_SCREEN: return 1 + 2;
        default: return 2;   // top-up, close and reopen
    }
}

// "" when the program is well formed, else what is wrong with it
inline std::string probe_validate(uint32_t num_cases, const int32_t *lane_gen, const bt_rng_probe_gen *gens, const bt_rng_probe_step *steps, uint64_t num_steps, uint32_t row_cap) {
    if (!num_cases || num_cases > MAX_CASES) return "number of cases out of range";
    if (!row_cap || row_cap > MAX_ROW) return "row capacity out of range";
    for (uint32_t c = 0; c < num_cases; ++c) {
        uint64_t held[LANES] = {};
        for (uint32_t l = 0; l < LANES; ++l) {
            const int32_t g = lane_gen[c * LANES + l];
            if (g < -1 || g >= (int32_t)LANES) return "lane map entry out of range";
            if (g >= 0) held[g] |= 1ull << l;
        }
        for (uint32_t g = 0; g < LANES; ++g) {
            if (!held[g]) continue;
            const bt_rng_probe_gen &G = gens[c * LANES + g];
            if (G.ring_cap != 8 && G.ring_cap != 16 && G.ring_cap != 32 && G.ring_cap != 64) return "ring cap must be 8, 16, 32 or 64";
            if (G.ring_place > BT_PROBE_RING_LDS_FLAT) return "unknown ring place";
            if (G.discard > MAX_DISCARD) return "discard too long";
            if (G.num_steps > MAX_STEPS || (uint64_t)G.step_off + G.num_steps > num_steps) return "step list out of range";
            if (!G.copies || G.copies > LANES || (LANES % G.copies)) return "copies must divide 64";
            // the lanes that share a generator are the lockstep copies g0 + k * (64 / copies): they run one program, the generator's
            const uint32_t width = LANES / G.copies, first = (uint32_t)__builtin_ctzll(held[g]);
            uint64_t want = 0;
            for (uint32_t k = 0; k < G.copies; ++k) want |= 1ull << (first % width + k * width);
            if (held[g] != want) return "the lanes of a generator must be its `copies` lockstep copies";
            uint64_t words = 0, total = G.discard;
            for (uint32_t s = 0; s < G.num_steps; ++s) {
                const bt_rng_probe_step &S = steps[G.step_off + s];
                if (S.kind >= BT_PROBE_KINDS) return "unknown step kind";
                if (S.n > MAX_N) return "step count too large";
                total += S.n;
                words += step_words(S);
                switch (S.kind) {
                    case BT_PROBE_UNIFORM_INT:
                        if (!(S.a >= 1.0 && S.a <= 4294967295.0) || S.a != floor(S.a)) return "uniform_int range out of range";
                        break;
                    case BT_PROBE_BERNOULLI: case BT_PROBE_BULK:
                        if (!(S.a >= 0.0 && S.a <= 1.0)) return "probability out of range";
                        break;
                    case BT_PROBE_SHUFFLE:
                        if (S.n > MAX_SHUFFLE) return "shuffle too long";
                        break;
                    case BT_PROBE_GAMMA:
                        if (!(S.a > 0.0 && S.a <= 1e300 && S.b > 0.0 && S.b <= 1e300)) return "gamma parameters out of range";
                        break;
                    case BT_PROBE_DIRECT:
                        if (S.a != 1.0 && S.a != 2.0 && S.a != 4.0) return "direct-form width must be 1, 2 or 4";
                        if (S.n % (uint32_t)S.a) return "direct-form count must be a multiple of the width";
                        if (G.copies != 1) return "direct-form draws need a generator of one lane";
                        break;
                    default: break;
                }
            }
            if (total > MAX_TOTAL) return "program too long";
            if (words > row_cap) return "program writes more than a row holds";
        }
    }
    return "";
}

#ifdef BT_RNG_BULK   // (the block form of the ring generator: the only form the probe knows)
// the memory of one lane's run beside the ring generator itself
struct Mem {
    uint32_t *direct;     // MT_WORDS: the direct-form generator of the same seed (its own stream position)
    uint32_t *scratch;    // MAX_SHUFFLE
    double *saved;        // NormalState
    uint32_t *available;
};

// R: an open ring generator.  reopen(m): mt_close, then the matching mt_ring_open.  bulk(m, n, p, emit): rng_bernoulli_bulk with the lane's team.
template <class R, class Reopen, class Bulk>
BT_HD void run_program(R &m, uint32_t seed, uint32_t discard, const bt_rng_probe_step *steps, uint32_t num_steps, const Mem &mem, Out &out, uint32_t BT_GAS *fin, Reopen &&reopen,
                       Bulk &&bulk) {
    mt_seed(mem.direct, seed);
    *mem.saved = 0.0;
    *mem.available = 0;
    const NormalState nd{mem.saved, mem.available};
    for (uint32_t i = 0; i < discard; ++i) (void)m.next();
    for (uint32_t s = 0; s < num_steps; ++s) {
        const bt_rng_probe_step S = steps[s];
        const uint32_t n = S.n;
        switch (S.kind) {
            case BT_PROBE_DRAW:
                for (uint32_t i = 0; i < n; ++i) out.w(m.next());
                break;
            case BT_PROBE_TOPUP:
                m.topup();
                break;
            case BT_PROBE_REOPEN:
                reopen(m);
                break;
            case BT_PROBE_CANONICAL:
                for (uint32_t i = 0; i < n; ++i) out.d(rng_canonical(m));
                break;
            case BT_PROBE_CANONICAL2:
                for (uint32_t i = 0; i < n; ++i) {
                    double x, y;
                    rng_canonical2(m, x, y);
                    out.d(x);
                    out.d(y);
                }
                break;
            case BT_PROBE_UNIFORM_INT:
                for (uint32_t i = 0; i < n; ++i) out.w(rng_uniform_int(m, (uint32_t)S.a));
                break;
            case BT_PROBE_BERNOULLI:
                for (uint32_t i = 0; i < n; ++i) out.w(rng_bernoulli(m, S.a) ? 1u : 0u);
                break;
            case BT_PROBE_SHUFFLE:
                for (uint32_t i = 0; i < n; ++i) mem.scratch[i] = i;
                rng_shuffle_u32(m, sptr1(mem.scratch), n);
                for (uint32_t i = 0; i < n; ++i) out.w(mem.scratch[i]);
                break;
            case BT_PROBE_NORMAL:
                for (uint32_t i = 0; i < n; ++i) {
                    out.d(rng_normal(m, nd));
                    if (S.c != 0.0) out.w(m.next());
                }
                break;
            case BT_PROBE_GAMMA:
                for (uint32_t i = 0; i < n; ++i) {
                    out.d(rng_gamma(m, nd, S.a, S.b));
                    if (S.c != 0.0) out.w(m.next());
                }
                break;
            case BT_PROBE_BULK: {
                const uint32_t base = out.o;
                bulk(m, n, S.a, [&](uint32_t i, bool sel, unsigned long long b) {
                    if (i < n) {
                        out.put(base + 3u * i, sel ? 1u : 0u);
                        out.put(base + 3u * i + 1u, (uint32_t)b);
                        out.put(base + 3u * i + 2u, (uint32_t)(b >> 32));
                    }
                });
                out.o = base + 3u * n;
                break;
            }
            case BT_PROBE_DIRECT: {
                Mt dm = mt_open(mem.direct);
                const uint32_t width = (uint32_t)S.a;
                for (uint32_t i = 0; i < n; i += width) {
                    if (width == 1u) {
                        out.w(dm.next());
                    } else if (width == 2u) {
                        uint32_t w2[2];
                        dm.next_n<2>(w2);
                        out.w(w2[0]), out.w(w2[1]);
                    } else {
                        uint32_t w4[4];
                        dm.next_n<4>(w4);
                        out.w(w4[0]), out.w(w4[1]), out.w(w4[2]), out.w(w4[3]);
                    }
                }
                mt_close(dm);
                break;
            }
            case BT_PROBE_SCREEN:
                out.w(gamma_second_test_rejects(S.a, S.b, S.c, S.d) ? 1u : 0u);
                break;
            default: break;
        }
        out.w(m.pos | m.flags);
        out.w(m.head | (m.avail << 16));
    }
    fin[0] = m.pos, fin[1] = m.flags, fin[2] = m.head, fin[3] = m.avail;
    for (uint32_t k = 0; k < TAIL_WORDS; ++k) fin[4u + k] = m.next();
}

// the host twin behind bt_diag_rng_probe (and tools/bulk_subset_host_check.cpp under a host sanitizer): every generator a lane holds runs its program once, as
// a team of one; rows [cases][64 GENERATORS][row_cap] and finals [cases][64][FINAL_WORDS], 0xFFFFFFFF where nothing was written.  The program is validated.
__host__ inline void host_twin(uint32_t num_cases, const int32_t *lane_gen, const bt_rng_probe_gen *gens, const bt_rng_probe_step *steps, uint32_t row_cap, uint32_t *rows,
                               uint32_t *finals) {
    typedef SPtrF<uint32_t, 1> RP;
    std::vector<uint32_t> st(2 * MT_BUF), ring(RING_WORDS), direct(MT_BUF), scratch(MAX_SHUFFLE);
    for (size_t slot = 0; slot < (size_t)num_cases * LANES; ++slot) {
        uint32_t *row = rows + slot * row_cap, *fin = finals + slot * FINAL_WORDS;
        std::fill(row, row + row_cap, 0xFFFFFFFFu);
        std::fill(fin, fin + FINAL_WORDS, 0xFFFFFFFFu);
        const uint32_t c = (uint32_t)(slot / LANES);
        bool held = false;
        for (uint32_t l = 0; l < LANES; ++l) held |= lane_gen[c * LANES + l] == (int32_t)(slot % LANES);
        if (!held) continue;
        const bt_rng_probe_gen &G = gens[slot];
        std::fill(st.begin(), st.end(), 0u);
        std::fill(ring.begin(), ring.end(), 0u);
        double saved = 0;
        uint32_t available = 0;
        const RP rp{ring.data(), 0u, 0u};
        mt_ring_seed(st.data(), rp, G.ring_cap, G.seed);
        MtRing m = mt_ring_open(st.data(), rp, G.ring_cap);
        const Mem mem{direct.data(), scratch.data(), &saved, &available};
        Out out{(uint32_t BT_GAS *)row, row_cap, 0u};
        run_program(
            m, G.seed, G.discard, steps + G.step_off, G.num_steps, mem, out, (uint32_t BT_GAS *)fin,
            [&](MtRing &r) {
                mt_close(r);
                r = mt_ring_open(st.data(), rp, G.ring_cap);
            },
            [&](MtRing &r, uint32_t n, double p, auto &&emit) {
                const MtTeamOne team;
                rng_bernoulli_bulk(r, n, p, team, emit);
            });
    }
}
#endif

}  // namespace probe
}  // namespace bt
