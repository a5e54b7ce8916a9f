// Philox-4x32 with 10 rounds (Salmon et al., SC 2011): the counter-based generator of giga_mesh_sample (giga_eval.hip) and
// giga_depth_noise (giga_noise.hip).  Pure integer arithmetic: a numpy restatement reproduces every word (tests/eval_emu.py).
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

}  // namespace giga
#endif  // GIGA_PHILOX_H_
