// measure_scratch.h — the block count and the fixed-order sums of one map-measurement call
// (measurements.hip, depth_image.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

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

}  // namespace deftri
