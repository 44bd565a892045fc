// bt_rng_probe / bt_diag_rng_probe: the random-number stack of bt_rng_device.hpp run DIRECTLY, a wavefront per case, so that a test can put a chosen set
// of lanes at a block end, a top-up or a bulk draw and compare every word with the textbook stream — instead of learning from a whole sampler run that
// "the trace diverges at sweep k".  A test harness: nothing here is launched by a production path.
//
// A case is one 64-thread workgroup (one wavefront).  A lane holds a generator or is idle (it leaves at once and is out of the exec mask); the lanes that
// share a generator are its lockstep copies g0 + k * (64 / copies), as in a narrow Gibbs tile.  The ring of a generator lies where the program says,
// behind the pointer types the kernels use: lane-interleaved words in HBM or in LDS behind a generic pointer (mt_ring_open, the tile kernels), or in LDS
// behind an LDS-address-space pointer (mt_ring_open_as, the simple kernel).
#include <vector>

#include "bt_internal.hpp"
#include "bt_rng_probe.hpp"

namespace bt {
namespace probe {

// lane-interleaved array in LDS, as bt_gibbs_simple.hpp's LdsArr
struct LdsWords {
    uint32_t BT_LAS *p;
    __device__ inline uint32_t BT_LAS &operator[](uint32_t i) const { return p[i * LANES]; }
};

struct DeviceArgs {
    const int32_t *lane_gen;          // [cases][64]
    const bt_rng_probe_gen *gens;     // [cases][64]
    const bt_rng_probe_step *steps;
    uint32_t row_cap;
    uint32_t *rows;                   // [cases][64 lanes][row_cap]
    uint32_t *fin;                    // [cases][64 lanes][FINAL_WORDS]
    uint32_t *states;                 // [cases][64 generators][2 * MT_BUF]
    uint32_t *rings;                  // [cases][RING_WORDS][64 generators]
    uint32_t *direct;                 // [cases][64 lanes][MT_BUF]
    uint32_t *scratch;                // [cases][64 lanes][MAX_SHUFFLE]
    double *saved;                    // [cases][64 lanes]
    uint32_t *available;              // [cases][64 lanes]
};

#ifdef BT_RNG_BULK
template <class R, class Reopen>
__device__ inline void run_lane(R &m, const bt_rng_probe_gen &G, const DeviceArgs &a, uint32_t slot, uint32_t part, Reopen &&reopen) {
    const Mem mem{a.direct + (size_t)slot * MT_BUF, a.scratch + (size_t)slot * MAX_SHUFFLE, a.saved + slot, a.available + slot};
    Out out{(uint32_t BT_GAS *)(a.rows + (size_t)slot * a.row_cap), a.row_cap, 0u};
    const uint32_t copies = G.copies;
    run_program(m, G.seed, G.discard, a.steps + G.step_off, G.num_steps, mem, out, (uint32_t BT_GAS *)(a.fin + (size_t)slot * FINAL_WORDS), reopen,
                [&](R &r, uint32_t n, double p, auto &&emit) {
                    if (copies > 1u) {
                        const MtTeamCopies team(part, copies);
                        rng_bernoulli_bulk(r, n, p, team, emit);
                    } else {
                        const MtTeamOne team;
                        rng_bernoulli_bulk(r, n, p, team, emit);
                    }
                });
    mt_close(m);
}

__global__ __launch_bounds__(64) void rng_probe_kernel(DeviceArgs a) {
    __shared__ uint32_t lds_rings[RING_WORDS * LANES];
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    const int32_t gi = a.lane_gen[c * LANES + lane];
    if (gi < 0) return;
    const uint32_t g = (uint32_t)gi, slot = c * LANES + lane;
    const bt_rng_probe_gen G = a.gens[c * LANES + g];
    const uint32_t cap = G.ring_cap, width = LANES / G.copies, part = lane / width;
    uint32_t *st = a.states + (size_t)(c * LANES + g) * (2 * MT_BUF);
    if (G.ring_place == BT_PROBE_RING_LDS) {
        const LdsWords ring{(uint32_t BT_LAS *)lds_rings + g};
        mt_ring_seed(st, ring, cap, G.seed);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the seeded words are read by the lanes that help with the first twist
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        MtRingT<LdsWords> m = mt_ring_open_as(st, ring, cap);
        run_lane(m, G, a, slot, part, [&](MtRingT<LdsWords> &r) {
            mt_close(r);
            r = mt_ring_open_as(st, ring, cap);
        });
    } else {
        uint32_t *base = G.ring_place == BT_PROBE_RING_HBM ? a.rings + (size_t)c * RING_WORDS * LANES : (uint32_t *)lds_rings;
        const SPtrF<uint32_t, LANES> ring{base, g, 6u};
        mt_ring_seed(st, ring, cap, G.seed);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the seeded words are read by the lanes that help with the first twist
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        MtRing m = mt_ring_open(st, ring, cap);
        run_lane(m, G, a, slot, part, [&](MtRing &r) {
            mt_close(r);
            r = mt_ring_open(st, ring, cap);
        });
    }
}

#endif

static int check_args(const char *who, uint32_t num_cases, const int32_t *lane_gen, const bt_rng_probe_gen *gens, const bt_rng_probe_step *steps, uint64_t num_steps, uint32_t row_cap,
                      const uint32_t *rows, const uint32_t *fin) {
    if (!lane_gen || !gens || (num_steps && !steps) || !rows || !fin) return fail(std::string(who) + ": null argument");
    const std::string why = probe_validate(num_cases, lane_gen, gens, steps, num_steps, row_cap);
    if (!why.empty()) return fail(std::string(who) + ": " + why);
    return BT_OK;
}

}  // namespace probe
}  // namespace bt

using namespace bt;
using namespace bt::probe;

extern "C" {

int bt_rng_probe(bt_ctx *ctx, uint32_t num_cases, const int32_t *h_lane_gen, const bt_rng_probe_gen *h_gens, const bt_rng_probe_step *h_steps, uint64_t num_steps, uint32_t row_cap,
                 uint32_t *h_rows, uint32_t *h_final) {
#ifndef BT_RNG_BULK
    return fail("bt_rng_probe: this build has no block-form generator");
#else
    if (!ctx) return fail("bt_rng_probe: null argument");
    if (int rc = check_args("bt_rng_probe", num_cases, h_lane_gen, h_gens, h_steps, num_steps, row_cap, h_rows, h_final)) return rc;
    BT_HIP(hipSetDevice(ctx->device));
    const size_t slots = (size_t)num_cases * LANES;
    const size_t sizes[10] = {slots * sizeof(int32_t),        slots * sizeof(bt_rng_probe_gen),  (size_t)(num_steps ? num_steps : 1) * sizeof(bt_rng_probe_step),
                              slots * row_cap * 4,            slots * FINAL_WORDS * 4,           slots * 2 * MT_BUF * 4,
                              slots * RING_WORDS * 4,         slots * MT_BUF * 4,                slots * MAX_SHUFFLE * 4,
                              slots * 16};
    size_t off[11] = {0};
    for (int i = 0; i < 10; ++i) off[i + 1] = (off[i] + sizes[i] + 255) & ~(size_t)255;
    uint8_t *d = nullptr;
    BT_HIP(hipMalloc(&d, off[10]));
    auto run = [&]() -> int {
        BT_HIP(hipMemsetAsync(d, 0, off[10], ctx->stream));
        BT_HIP(hipMemsetAsync(d + off[3], 0xFF, sizes[3] + 0, ctx->stream));   // a row word no step wrote reads 0xFFFFFFFF
        BT_HIP(hipMemsetAsync(d + off[4], 0xFF, sizes[4], ctx->stream));
        BT_HIP(hipMemcpyAsync(d + off[0], h_lane_gen, sizes[0], hipMemcpyHostToDevice, ctx->stream));
        BT_HIP(hipMemcpyAsync(d + off[1], h_gens, sizes[1], hipMemcpyHostToDevice, ctx->stream));
        if (num_steps) BT_HIP(hipMemcpyAsync(d + off[2], h_steps, (size_t)num_steps * sizeof(bt_rng_probe_step), hipMemcpyHostToDevice, ctx->stream));
        DeviceArgs a;
        a.lane_gen = (const int32_t *)(d + off[0]);
        a.gens = (const bt_rng_probe_gen *)(d + off[1]);
        a.steps = (const bt_rng_probe_step *)(d + off[2]);
        a.row_cap = row_cap;
        a.rows = (uint32_t *)(d + off[3]);
        a.fin = (uint32_t *)(d + off[4]);
        a.states = (uint32_t *)(d + off[5]);
        a.rings = (uint32_t *)(d + off[6]);
        a.direct = (uint32_t *)(d + off[7]);
        a.scratch = (uint32_t *)(d + off[8]);
        a.saved = (double *)(d + off[9]);
        a.available = (uint32_t *)(d + off[9] + slots * 8);
        hipLaunchKernelGGL(rng_probe_kernel, dim3(num_cases), dim3(LANES), 0, ctx->stream, a);
        BT_CHECK_LAUNCH();
        BT_HIP(hipMemcpyAsync(h_rows, d + off[3], sizes[3], hipMemcpyDeviceToHost, ctx->stream));
        BT_HIP(hipMemcpyAsync(h_final, d + off[4], sizes[4], hipMemcpyDeviceToHost, ctx->stream));
        BT_HIP(hipStreamSynchronize(ctx->stream));
        return BT_OK;
    };
    const int rc = run();
    (void)hipFree(d);
    return rc;
#endif
}

// the host twin: every generator a lane holds runs its program once, as a team of one.  h_rows [cases][64 GENERATORS][row_cap], h_final likewise.
int bt_diag_rng_probe(uint32_t num_cases, const int32_t *h_lane_gen, const bt_rng_probe_gen *h_gens, const bt_rng_probe_step *h_steps, uint64_t num_steps, uint32_t row_cap,
                      uint32_t *h_rows, uint32_t *h_final) {
#ifdef BT_RNG_BULK
    if (int rc = check_args("bt_diag_rng_probe", num_cases, h_lane_gen, h_gens, h_steps, num_steps, row_cap, h_rows, h_final)) return rc;
    host_twin(num_cases, h_lane_gen, h_gens, h_steps, row_cap, h_rows, h_final);
    return BT_OK;
#else
    return fail("bt_diag_rng_probe: this build has no block-form generator");
#endif
}

}  // extern "C"
