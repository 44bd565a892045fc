// Stand-alone host check of rng_bernoulli_bulk (bt_rng_device.hpp): the cases of tests/test_bulk_subset_cpu.py, meant to be built with a host sanitizer:
//   hipcc --offload-host-only -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/bulk_subset_host_check.cpp -o build/bulk_subset_host_check && build/bulk_subset_host_check
// Exit status 0 when the call-by-call draws, the bulk routine and the direct-form generator agree in every case.
// With a file argument it also runs the generator probe's host twin (bt_rng_probe.hpp: probe_validate, host_twin) over a case corpus written by
// `python tests/_rng_probe.py <file>` — the corpus of tests/test_rng_probe_*.py — twice, and expects equal rows: the sanitizers see every step kind.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../bayestyper_amd/csrc/bt_rng_device.hpp"
#include "../bayestyper_amd/csrc/bt_rng_probe.hpp"

static int run_corpus(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) return printf("cannot open %s\n", path), 1;
    uint64_t head[3];   // cases, steps, row capacity
    if (fread(head, 8, 3, f) != 3 || head[0] > bt::probe::MAX_CASES || head[1] > (1u << 24)) return printf("bad corpus header\n"), 1;
    const size_t slots = (size_t)head[0] * 64;
    std::vector<int32_t> lane_gen(slots);
    std::vector<bt_rng_probe_gen> gens(slots);
    std::vector<bt_rng_probe_step> steps(head[1]);
    if (fread(lane_gen.data(), 4, slots, f) != slots || fread(gens.data(), sizeof(bt_rng_probe_gen), slots, f) != slots ||
        fread(steps.data(), sizeof(bt_rng_probe_step), steps.size(), f) != steps.size())
        return printf("short corpus file\n"), 1;
    fclose(f);
    const std::string why = bt::probe::probe_validate((uint32_t)head[0], lane_gen.data(), gens.data(), steps.data(), steps.size(), (uint32_t)head[2]);
    if (!why.empty()) return printf("corpus refused: %s\n", why.c_str()), 1;
    std::vector<uint32_t> rows[2], fin[2];
    for (int r = 0; r < 2; ++r) {
        rows[r].resize(slots * head[2]);
        fin[r].resize(slots * bt::probe::FINAL_WORDS);
        bt::probe::host_twin((uint32_t)head[0], lane_gen.data(), gens.data(), steps.data(), (uint32_t)head[2], rows[r].data(), fin[r].data());
    }
    const bool same = rows[0] == rows[1] && fin[0] == fin[1];
    printf("probe corpus: %llu cases, %llu steps, two runs %s\n", (unsigned long long)head[0], (unsigned long long)head[1], same ? "equal" : "DIFFER");
    return same ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc > 1 && run_corpus(argv[1])) return 1;
    const uint32_t ns[] = {0, 1, 311, 312, 313, 1000};
    const uint64_t discards[] = {0, 1, 623, 624 + 5, 624 + 623, 2 * 624, 330};
    const double ps[] = {0.0, 1.0, (double)0.1f};
    const uint32_t caps[] = {8, 16, 32, 64};
    unsigned cases = 0, bad = 0;
    for (uint32_t cap : caps)
        for (int ahead = 0; ahead < 2; ++ahead)
            for (uint64_t discard : discards)
                for (uint32_t n : ns)
                    for (double p : ps) {
                        std::vector<uint8_t> flags(3 * (size_t)n + 1);
                        uint32_t tail[24], state[8];
                        bt::bulk_bernoulli_check(12345u + cap, discard, n, p, cap, ahead, flags.data(), tail, state);
                        const bool ok = !memcmp(flags.data(), flags.data() + n, n) && !memcmp(flags.data(), flags.data() + 2 * (size_t)n, n) && !memcmp(tail, tail + 8, 32) &&
                                        !memcmp(tail, tail + 16, 32) && !memcmp(state, state + 4, 16);
                        ++cases;
                        if (!ok) {
                            ++bad;
                            printf("MISMATCH cap %u ahead %d discard %llu n %u p %g: state {%u %x %u %u} vs {%u %x %u %u}\n", cap, ahead, (unsigned long long)discard, n, p, state[0], state[1],
                                   state[2], state[3], state[4], state[5], state[6], state[7]);
                        }
                    }
    printf("%u cases, %u mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
