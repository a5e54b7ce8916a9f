// The one place a prefix sum is written: the count / scan / emit stages (giga_mesh.hip, giga_tsdf.hip, giga_mise.hip,
// giga_affordance.hip, giga_simplify.hip, giga_eval.hip, giga_candidates.hip) take every prefix from here.  Prefixes are taken in lane order by shuffles:
// no atomics, so equal input gives equal output positions.
//
// A ragged per-scene list is emitted in three steps.  Every workgroup of a count kernel leaves its sum in blk[scene][workgroup]
// (block_excl).  scene_offsets_kernel turns the sums of a scene into exclusive offsets in place and writes the scene's total;
// scene_bases_kernel turns the totals into the scenes' first positions in the packed output.  The emit kernel repeats the count
// kernel's block_excl and writes at (scene base + workgroup offset + prefix).
#pragma once
#include <hip/hip_runtime.h>

namespace giga {

constexpr int SCAN_BLOCK = 1024;                // threads of scene_offsets_kernel

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

// The same for a count of three bits, by ballot and popcount in place of the six shuffle steps: the exclusive prefix across the
// wave and, in `sum`, the wave's total.  Bit 0 of a lane counts 1, bit 1 counts W1, bit 2 counts W2: <1, 1> adds up three flags,
// <2, 4> a binary number.  (Marching cubes on 32 grids of 129^3 ran about 2 % slower with the shuffle form, against a run-to-run
// spread of 0.3 %; packing its two counts into the halves of one word cost as much again, hence the uint2 of block_combine.)
template <unsigned W1, unsigned W2>
__device__ __forceinline__ unsigned wave_excl_bits3(unsigned bits, unsigned lane, unsigned& sum) {
    const unsigned long long lt = (1ull << lane) - 1ull;
    const unsigned long long b0 = __ballot(bits & 1), b1 = __ballot(bits & 2), b2 = __ballot(bits & 4);
    sum = __popcll(b0) + W1 * __popcll(b1) + W2 * __popcll(b2);
    return __popcll(b0 & lt) + W1 * __popcll(b1 & lt) + W2 * __popcll(b2 & lt);
}

// From the prefix inside the wave to the prefix inside a workgroup of WAVES waves, in thread order: `sum` is the wave's total in
// the lane that is its `writer`; `total` = the workgroup's sum.  wsum: WAVES words of LDS.  T: an integer, or uint2 for a pair of
// counts that are summed side by side.  (One __syncthreads inside: every thread of the workgroup must call it.)
template <int WAVES, typename T>
__device__ __forceinline__ T block_combine(T pre, T sum, bool writer, T* wsum, T& total) {
    const unsigned wave = threadIdx.x >> 6;
    if (writer) wsum[wave] = sum;
    __syncthreads();
    total = T();
#pragma unroll
    for (unsigned w = 0; w < (unsigned)WAVES; ++w) {
        if (w < wave) pre += wsum[w];
        total += wsum[w];
    }
    return pre;
}

// exclusive prefix of x over a workgroup of WAVES waves, in thread order; `total` = the workgroup's sum (block_combine's barrier)
template <int WAVES, typename T>
__device__ __forceinline__ T block_excl(T x, T* wsum, T& total) {
    const unsigned lane = threadIdx.x & 63;
    const T incl = wave_incl(x, lane);
    return block_combine<WAVES>(incl - x, incl, lane == 63, wsum, total);
}

// exclusive prefix over n elements by one workgroup of WAVES waves, 64 WAVES elements a round: store(i, prefix before element i)
// for every i < n, in index order; returns the sum of all.  The running total is a register that every thread keeps.
template <int WAVES, typename T, typename Load, typename Store>
__device__ __forceinline__ T block_scan_rounds(unsigned n, T* wsum, Load load, Store store) {
    T run = 0;
    for (unsigned base = 0; base < n; base += 64 * WAVES) {
        const unsigned i = base + threadIdx.x;
        T total;
        const T pre = run + block_excl<WAVES>(i < n ? load(i) : T(0), wsum, total);
        if (i < n) store(i, pre);
        run += total;
        __syncthreads();                        // wsum is written again by the next round
    }
    return run;
}

// One workgroup per scene: the scene's nblk workgroup sums become exclusive offsets, in place, and the scene's total goes to `counts`
// and, where given, to `counts2`.  T = unsigned: one count.  T = unsigned long long: two counts side by side, the first in the low
// word (a uint2 in memory); each stays below 2^32 for a whole scene, so the halves never carry into each other.  The two totals
// are stored interleaved: counts[2 scene], counts[2 scene + 1].
template <typename T>
__global__ __launch_bounds__(SCAN_BLOCK) void scene_offsets_kernel(T* __restrict__ blk, unsigned nblk, int* __restrict__ counts,
                                                                   int* __restrict__ counts2) {
    constexpr int NC = sizeof(T) / sizeof(unsigned);
    __shared__ T wsum[SCAN_BLOCK / 64];
    T* b = blk + (size_t)blockIdx.x * nblk;
    const T total = block_scan_rounds<SCAN_BLOCK / 64>(nblk, wsum, [&](unsigned i) { return b[i]; }, [&](unsigned i, T pre) { b[i] = pre; });
    if (threadIdx.x < NC) {
        const int c = (int)(unsigned)((unsigned long long)total >> (32 * threadIdx.x));
        counts[NC * blockIdx.x + threadIdx.x] = c;
        if (counts2) counts2[NC * blockIdx.x + threadIdx.x] = c;
    }
}

// One wave: bases[NC b + c] = component c of the totals of the scenes before b; bases[NC B + c] = the grand totals.
template <int NC>
__global__ __launch_bounds__(64) void scene_bases_kernel(const int* __restrict__ counts, int B, unsigned long long* __restrict__ bases) {
    const unsigned lane = threadIdx.x;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        unsigned long long carry = 0;
        for (int base = 0; base < B; base += 64) {
            const int b = base + (int)lane;
            const unsigned long long n = b < B ? (unsigned)counts[NC * b + c] : 0u;
            const unsigned long long inc = wave_incl(n, lane);
            if (b < B) bases[NC * b + c] = carry + inc - n;
            carry += __shfl(inc, 63, 64);
        }
        if (lane == 0) bases[NC * B + c] = carry;
    }
}

// how many of `total` entries do not fit into `cap`, saturated at INT_MAX
__device__ __forceinline__ int scan_shortfall(unsigned long long total, unsigned long long cap) {
    const unsigned long long big = 0x7fffffffull;
    return (int)(total > cap ? (total - cap < big ? total - cap : big) : 0);
}

}  // namespace giga
