// Philox-4x32 with 10 rounds (Salmon et al., SC 2011): the counter-based generator of giga_mesh_sample (giga_eval.hip),
// giga_depth_noise (giga_noise.hip), giga_refine_face_points (giga_refine.hip) and giga_grasp_candidates (giga_candidates.hip).
// Pure integer arithmetic: a numpy restatement reproduces every word (tests/eval_emu.py).  The double-precision uniforms and
// Box-Muller normals built on a block (noise_*) are the depth noise's, shared with the refinement's barycentric draws and the
// candidates' grasp depth; each of their operations is one IEEE rounding (there is no multiply-add pair to contract).
#ifndef GIGA_PHILOX_H_
#define GIGA_PHILOX_H_
#include <hip/hip_runtime.h>

namespace giga {

struct Philox { unsigned x[4]; };
__device__ __forceinline__ Philox philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox{{c0, c1, c2, c3}};
}

struct NoisePair { double z0, z1; };

// 53 bits of two words, strictly inside (0, 1): k 2^-53, and 2^-54 in place of 0
__device__ __forceinline__ double noise_u53(unsigned hi, unsigned lo) {
    const unsigned long long k = ((unsigned long long)(hi >> 5) << 26) | (unsigned long long)(lo >> 6);
    return k ? (double)k * 0x1p-53 : 0x1p-54;
}

__device__ __forceinline__ NoisePair noise_pair(unsigned block, unsigned id_lo, unsigned id_hi, unsigned stream, unsigned k0, unsigned k1) {
    const Philox r = philox4x32_10(block, id_lo, id_hi, stream, k0, k1);
    const double u1 = noise_u53(r.x[0], r.x[1]), u2 = noise_u53(r.x[2], r.x[3]);
    const double rad = sqrt(-2.0 * log(u1)), th = 6.283185307179586 * u2;
    return NoisePair{rad * cos(th), rad * sin(th)};
}

__device__ __forceinline__ double noise_normal(unsigned e, unsigned id_lo, unsigned id_hi, unsigned stream, unsigned k0, unsigned k1) {
    const NoisePair q = noise_pair(e >> 1, id_lo, id_hi, stream, k0, k1);
    return (e & 1u) ? q.z1 : q.z0;
}

}  // namespace giga
#endif  // GIGA_PHILOX_H_
