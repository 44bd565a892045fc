// Stand-alone host check of the reads route's host code: the reads reader (bayestyper_amd/host/ReadsFile.cpp) and the kernels' window code run by one thread
// (bayestyper_amd/csrc/bt_reads_window.hpp), for a sanitizer build.  No GPU, no library: it parses the read files given, and prints the number of k-mers.
//
//   hipcc --offload-host-only -x hip -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/reads_host_check.cpp -x c++ bayestyper_amd/host/ReadsFile.cpp -lz -o reads_host_check
//   ./reads_host_check <k> <slab bytes> <read file>...
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>

#include "../bayestyper_amd/csrc/bt_reads_window.hpp"
#include "../bayestyper_amd/host/ReadsFile.hpp"

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <k> <slab bytes> <read file>...\n", argv[0]);
        return 2;
    }
    const unsigned k = (unsigned)std::atoi(argv[1]);
    const size_t slab_bytes = (size_t)std::strtoull(argv[2], nullptr, 0);
    if (k < 1 || k > 64) {
        std::fprintf(stderr, "k must lie in 1 .. 64\n");
        return 2;
    }
    int bad = 0;
    for (int i = 3; i < argc; i++) {
        try {
            bthost::ReadsFile file(argv[i], k, slab_bytes);
            const bt::RollConst c = bt::make_roll_const(k);
            bt::HostTeam team;
            unsigned long long kmers = 0, slabs = 0, checksum = 0;
            auto consume = [&](bt::Kmer can, uint64_t h, uint64_t) {
                kmers++;
                checksum += h ^ can.lo ^ can.hi;   // order-independent: the same for every slab size
            };
            for (std::string slab; file.next(slab); slabs++) bt::reads_front_end(team, slab.data(), slab.size(), 0, c, consume);
            std::printf("%s\treads %llu\tbases %llu\tslabs %llu\tkmers %llu\tchecksum %016llx\n", argv[i], (unsigned long long)file.reads(), (unsigned long long)file.bases(), slabs, kmers,
                        checksum);
        } catch (const std::exception &e) {
            std::printf("%s\terror: %s\n", argv[i], e.what());
            bad++;
        }
    }
    return bad ? 1 : 0;
}
