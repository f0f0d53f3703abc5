// measure_scratch.h — the device scratch and the fixed-order sums of one map-measurement call
// (measurements.hip, depth_image.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "kernels.h"

namespace deftri {

static inline unsigned nblk(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

// fixed-order sums of `cnt` consecutive arrays of n doubles (device) -> host
static inline int sums(const double *d_terms, int64_t n, int cnt, double *part, double *d_out, double *h_out,
                       hipStream_t st) {
    for (int c = 0; c < cnt; c++) launch_sum(n, d_terms + c * n, nullptr, 0, 0, part, 256, d_out + c, st);
    if (hipMemcpyAsync(h_out, d_out, sizeof(double) * cnt, hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
    return hipStreamSynchronize(st) == hipSuccess ? 0 : -1;
}

// device scratch of one measurement call (freed before returning)
struct Scratch {
    std::vector<void *> p;
    ~Scratch() { for (void *q : p) hipFree(q); }
    template <class T>
    T *put(const std::vector<T> &v) {
        void *d = nullptr;
        if (hipMalloc(&d, sizeof(T) * std::max<size_t>(v.size(), 1)) != hipSuccess) return nullptr;
        p.push_back(d);
        if (!v.empty()) hipMemcpy(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
        return (T *)d;
    }
    double *alloc(size_t n) {
        void *d = nullptr;
        if (hipMalloc(&d, sizeof(double) * std::max<size_t>(n, 1)) != hipSuccess) return nullptr;
        p.push_back(d);
        return (double *)d;
    }
};

}  // namespace deftri
