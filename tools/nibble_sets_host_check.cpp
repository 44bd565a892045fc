// Stand-alone host check of the packed set primitives (nset_*, bt_rng_device.hpp) against the unordered_set emulation (uset_*), meant to be built with a
// host sanitizer:
//   hipcc --offload-host-only -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/nibble_sets_host_check.cpp -o build/nibble_sets_host_check && build/nibble_sets_host_check
// 1. random operation lists on one set, every universe 1 .. NSET_MAX: the replay in both forms gives the same order and the same picked elements;
// 2. the literal sequence of the sampler on a zero and a plus set that share their link words — freq_reset, hfd_increment moves, the add-zeros picks,
//    the re-insertion at the end of a frequency draw — compared after every step;
// 3. universe NSET_MAX + 1: the packed replay refuses it, and some history does give the lists an order that "push front / remove" does not — the
//    limit is where the derivation puts it.
// Exit status 0 when all of that holds.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../bayestyper_amd/csrc/bt_rng_device.hpp"

using namespace bt;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) % n);
}

static bool same_order(const USet &l, const uint32_t *next, const NSet &p) {
    uint32_t j = 0;
    for (uint32_t e = uset_begin(l); e != US_NONE; e = next[e], ++j)
        if (j >= nset_size(p) || nset_at(p, j) != e) return false;
    return j == nset_size(p) && uset_size(l) == nset_size(p);
}

// the sampler's use of the two sets over H haplotypes, `draws` frequency draws; returns the number of steps that differed
static unsigned sampler_sequence(uint32_t H, unsigned draws) {
    const uint32_t cap = uset_bucket_capacity(H);
    std::vector<uint32_t> zh(4), ph(4), zb(cap), pb(cap), next(H);
    USet lz{sptr1(zh.data()), sptr1(zb.data()), sptr1(next.data()), cap}, lp{sptr1(ph.data()), sptr1(pb.data()), sptr1(next.data()), cap};
    uset_init(lz);
    uset_init(lp);
    NSet z{0, 0}, p{0, 0};
    unsigned bad = 0;
    auto check = [&]() { bad += !(same_order(lz, next.data(), z) && same_order(lp, next.data(), p)); };
    // freq_reset
    uset_clear(lp);
    uset_clear(lz);
    for (uint32_t h = 0; h < H; ++h) uset_insert(lz, h);
    nset_clear(p);
    z = nset_descending(H);
    check();
    for (unsigned d = 0; d < draws; ++d) {
        // hfd_increment: some haplotypes get their first observation
        const uint32_t moves = 1 + rnd(H);
        for (uint32_t m = 0; m < moves && nset_size(z); ++m) {
            const uint32_t h = nset_at(z, rnd(nset_size(z)));
            uset_erase(lz, h);
            uset_insert(lp, h);
            nset_erase(z, h);
            nset_insert(p, h);
            check();
        }
        // add zeros: positions 0, |zero| - 1 and random ones
        const uint32_t add = nset_size(z) ? rnd(nset_size(z) + 1) : 0;
        for (uint32_t a = 0; a < add; ++a) {
            const uint32_t size = uset_size(lz), pos = a == 0 ? 0 : (a == 1 ? size - 1 : rnd(size));
            uint32_t e = uset_begin(lz);
            for (uint32_t i = 0; i < pos; ++i) e = next[e];
            uset_erase(lz, e);
            uset_insert(lp, e);
            const uint32_t e2 = nset_at(z, pos);
            nset_erase_at(z, pos);
            nset_insert(p, e2);
            bad += e != e2;
            check();
        }
        // the end of the draw: plus's order is recorded, plus is cleared, zero takes the elements in that order
        std::vector<uint32_t> rec;
        for (uint32_t e = uset_begin(lp); e != US_NONE; e = next[e]) rec.push_back(e);
        uset_clear(lp);
        for (uint32_t e : rec) uset_insert(lz, e);
        if (d & 1u) nset_move_all(z, p);
        else {   // the sampler's own form: one insert per element, then the clear
            for (uint32_t i = 0; i < nset_size(p); ++i) nset_insert(z, nset_at(p, i));
            nset_clear(p);
        }
        check();
        if (d % 7 == 6) {   // a new chain: freq_reset again
            uset_clear(lp);
            uset_clear(lz);
            for (uint32_t h = 0; h < H; ++h) uset_insert(lz, h);
            nset_clear(p);
            z = nset_descending(H);
            check();
        }
    }
    return bad;
}

int main() {
    unsigned cases = 0, bad = 0;
    for (uint32_t universe = 1; universe <= NSET_MAX; ++universe) {
        for (unsigned rep = 0; rep < 4000; ++rep) {
            const uint32_t n = 1 + rnd(96);
            std::vector<uint8_t> ops(n);
            std::vector<uint32_t> vals(n), o1(universe), o2(universe), a1(n), a2(n);
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t r = rnd(40);
                ops[i] = r == 0 ? 2 : (r < 16 ? 0 : (r < 28 ? 1 : (r < 36 ? 3 : 4)));
                vals[i] = rnd(universe);
            }
            uint32_t n1 = 0, n2 = 0;
            const int r1 = set_replay(false, universe, ops.data(), vals.data(), n, o1.data(), &n1, a1.data());
            const int r2 = set_replay(true, universe, ops.data(), vals.data(), n, o2.data(), &n2, a2.data());
            ++cases;
            if (r1 || r2 || n1 != n2 || memcmp(o1.data(), o2.data(), 4 * n1) || memcmp(a1.data(), a2.data(), 4 * n)) {
                ++bad;
                printf("MISMATCH universe %u history %u (%u operations)\n", universe, rep, n);
            }
        }
        for (unsigned rep = 0; rep < 200; ++rep) {
            ++cases;
            const unsigned b = sampler_sequence(universe, 30);
            if (b) {
                ++bad;
                printf("MISMATCH universe %u sampler sequence %u: %u steps differ\n", universe, rep, b);
            }
        }
    }
    // past the limit
    {
        const uint32_t universe = NSET_MAX + 1;
        uint8_t op = 0;
        uint32_t val = 0, order[16], n = 0;
        ++cases;
        if (set_replay(true, universe, &op, &val, 1, order, &n, nullptr) != 2) {
            ++bad;
            printf("the packed replay accepted universe %u\n", universe);
        }
        // insert 0 .. universe-1: "push front" would give universe-1, ..., 0; the 14th insert rehashes and reverses what was there
        std::vector<uint8_t> ops(universe, 0);
        std::vector<uint32_t> vals(universe), o(universe);
        for (uint32_t i = 0; i < universe; ++i) vals[i] = i;
        set_replay(false, universe, ops.data(), vals.data(), universe, o.data(), &n, nullptr);
        bool lifo = n == universe;
        for (uint32_t i = 0; i < n && lifo; ++i) lifo = o[i] == universe - 1 - i;
        ++cases;
        if (lifo) {
            ++bad;
            printf("universe %u: the lists still iterate in push-front order: derive the limit again before raising it\n", universe);
        }
    }
    printf("%u cases, %u mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
