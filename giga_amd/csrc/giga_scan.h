// Scan helpers shared by the count / scan / emit kernels (giga_mesh.hip, giga_mise.hip).  Every prefix is taken in lane order by
// shuffles: no atomics, so equal input gives equal output positions.
#pragma once
#include <hip/hip_runtime.h>

namespace giga {

// inclusive scan across a wave by shuffles (fixed order)
template <typename T>
__device__ __forceinline__ T wave_incl(T x, unsigned lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (lane >= (unsigned)o) x += y;
    }
    return x;
}

// exclusive prefix of x over a workgroup of WAVES waves, in thread order; `total` = the workgroup's sum.  wsum: WAVES words of LDS.
// (One __syncthreads inside: every thread of the workgroup must call it.)
template <int WAVES>
__device__ __forceinline__ unsigned block_excl(unsigned x, unsigned* wsum, unsigned& total) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned incl = wave_incl(x, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned pre = incl - x;
    total = 0;
#pragma unroll
    for (unsigned w = 0; w < (unsigned)WAVES; ++w) {
        if (w < wave) pre += wsum[w];
        total += wsum[w];
    }
    return pre;
}

}  // namespace giga
