// Stand-alone host check of rng_bernoulli_bulk (bt_rng_device.hpp): the cases of tests/test_bulk_subset_cpu.py, meant to be built with a host sanitizer:
//   hipcc --offload-host-only -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/bulk_subset_host_check.cpp -o build/bulk_subset_host_check && build/bulk_subset_host_check
// Exit status 0 when the call-by-call draws, the bulk routine and the direct-form generator agree in every case.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../bayestyper_amd/csrc/bt_rng_device.hpp"

int main() {
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
