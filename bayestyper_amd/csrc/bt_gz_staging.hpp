// What bt_gzip_save (bt_deflate.hip) and bt_bgzf_save (bt_bgzf.hip) share: the double-buffered staging of a slab pipeline, the file that keeps a temporary
// name until it is complete, and a host stopwatch.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <string>

namespace btgz {

// what a slab pipeline stages through: per slab parity a pinned input, a device input, a device output, a pinned output, the records' pinned copy
struct GzStaging {
    uint8_t *pin_in[2] = {}, *pin_out[2] = {}, *d_in[2] = {}, *d_out[2] = {};
    uint32_t *pin_recs[2] = {};
    unsigned long long *pin_total[2] = {};   // [0] the stream's length [1] the error word
    hipEvent_t ev[2][6] = {};                // h2d begin / end, kernels end, results copied, d2h begin / end
    hipStream_t copy_out = nullptr;
    hipStream_t main = nullptr;
    hipError_t alloc(hipStream_t on, uint64_t slab, uint64_t bound, uint64_t rec_bytes, int n) {
        main = on;
        hipError_t e = hipStreamCreateWithFlags(&copy_out, hipStreamNonBlocking);
        for (int i = 0; i < n && e == hipSuccess; ++i) {
            e = hipHostMalloc(reinterpret_cast<void **>(&pin_in[i]), std::max<uint64_t>(slab, 1), hipHostMallocDefault);
            if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&pin_out[i]), bound, hipHostMallocDefault);
            if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&pin_recs[i]), rec_bytes, hipHostMallocDefault);
            if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&pin_total[i]), 16, hipHostMallocDefault);
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_in[i]), std::max<uint64_t>(slab, 1));
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d_out[i]), bound);
            for (int k = 0; k < 6 && e == hipSuccess; ++k) e = hipEventCreate(&ev[i][k]);
        }
        return e;
    }
    ~GzStaging() {
        if (main) (void)hipStreamSynchronize(main);   // (an error path may leave work in flight)
        if (copy_out) {
            (void)hipStreamSynchronize(copy_out);
            (void)hipStreamDestroy(copy_out);
        }
        for (int i = 0; i < 2; ++i) {
            if (pin_in[i]) (void)hipHostFree(pin_in[i]);
            if (pin_out[i]) (void)hipHostFree(pin_out[i]);
            if (pin_recs[i]) (void)hipHostFree(pin_recs[i]);
            if (pin_total[i]) (void)hipHostFree(pin_total[i]);
            (void)hipFree(d_in[i]);
            (void)hipFree(d_out[i]);
            for (int k = 0; k < 6; ++k)
                if (ev[i][k]) (void)hipEventDestroy(ev[i][k]);
        }
    }
};

// the file under a temporary name until it is complete
struct TmpFile {
    FILE *f = nullptr;
    std::string path, tmp;
    ~TmpFile() {
        if (f) {
            fclose(f);
            remove(tmp.c_str());
        }
    }
    bool open(const char *p) {
        path = p;
        tmp = path + ".tmp";
        f = fopen(tmp.c_str(), "wb");
        return f != nullptr;
    }
    bool write(const void *p, size_t n) { return !n || fwrite(p, 1, n, f) == n; }
    bool finish() {
        const bool ok = fflush(f) == 0;
        const bool closed = fclose(f) == 0;
        f = nullptr;
        if (!ok || !closed || rename(tmp.c_str(), path.c_str()) != 0) {
            remove(tmp.c_str());
            return false;
        }
        return true;
    }
};

inline double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

}  // namespace btgz
