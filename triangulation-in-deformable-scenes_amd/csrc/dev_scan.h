// dev_scan.h — the exclusive scan of a short array by one workgroup, for the map-side builders whose
// arrays are a few thousand long (the feature grid's cells, the Delaunay rows, the triangulation matcher's
// rows): one launch, no second pass, no scratch.
#pragma once
#include <hip/hip_runtime.h>

namespace deftri {
namespace dev {

// start [n + 1] = the exclusive prefix sums of count [n], start[n] the total; cursor [n] = start when it is
// given.  Each of the B threads sums a contiguous chunk, thread 0 scans the B sums, each thread writes its chunk.
template <typename T, int B>
__global__ void __launch_bounds__(B) k_excl_scan(long long n, const T *__restrict__ count, T *__restrict__ start,
                                                 T *__restrict__ cursor) {
    __shared__ T sums[B];
    const long long chunk = (n + B - 1) / B;
    const long long lo = min((long long)threadIdx.x * chunk, n), hi = min(lo + chunk, n);
    T s = 0;
    for (long long c = lo; c < hi; c++) s += count[c];
    sums[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        T run = 0;
        for (int t = 0; t < B; t++) { const T v = sums[t]; sums[t] = run; run += v; }
        start[n] = run;
    }
    __syncthreads();
    T run = sums[threadIdx.x];
    for (long long c = lo; c < hi; c++) {
        start[c] = run;
        if (cursor) cursor[c] = run;
        run += count[c];
    }
}

template <typename T, int B> void launch_excl_scan(long long n, const T *count, T *start, T *cursor, hipStream_t st) {
    hipLaunchKernelGGL((k_excl_scan<T, B>), dim3(1), dim3(B), 0, st, n, count, start, cursor);
}

}  // namespace dev
}  // namespace deftri
