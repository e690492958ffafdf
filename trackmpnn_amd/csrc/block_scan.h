// Workgroup-wide exclusive prefix sum of one int per thread, for kernels that compact lists (csrc/trackops.hip,
// csrc/trainbuild.hip): wave64 shuffles, then the wave totals in LDS.  NT: the workgroup size (a multiple of 64);
// s_wave: NT / 64 + 1 ints of LDS.  Every thread of the workgroup must call it (it holds three barriers).
#pragma once
#include <hip/hip_runtime.h>

namespace tmpnn {

// exclusive prefix of v over the workgroup; *total = the sum (every thread)
template <int NT>
__device__ __forceinline__ int block_scan(int v, int* s_wave, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int w = 0; w < NT / 64; ++w) { const int t = s_wave[w]; s_wave[w] = run; run += t; }
        s_wave[NT / 64] = run;
    }
    __syncthreads();
    const int res = s_wave[wave] + inc - v;
    *total = s_wave[NT / 64];
    __syncthreads();
    return res;
}

}  // namespace tmpnn
