// Arguments of the persistent data-gradient kernel (giga_encoder.hip: unet_dgrad_mega_kernel), shared with its caller
// (giga_encoder_bwd.hip).
#pragma once
#include "giga_conv16.h"

namespace giga {

struct BwdPool {               // dS = S > 0 ? dcat[..., coff : coff + C] + unpool(dQ) : 0   (pool_bwd_add_kernel, giga_encoder_bwd.hip)
    float* dS; const float* dcat; const float* dQ; const float* S; const float* Q;   // unpool: see pool_first_max
    int cs, coff, H, W, C;
};

// MaxPool2d(2,2) backward routing, torch.max_pool2d's rule: of a window's elements equal to its maximum Q, only the FIRST
// in row-major order ((0,0), (0,1), (1,0), (1,1)) receives dQ.  (Handing dQ to every tied element multiplies the window's
// gradient by the number of ties; ties are common where the input is constant, e.g. the empty space of a TSDF.)
// s = S at pixel pix = (y, x) of an H x W image, channels [c, c + 4); returns 1.f per channel where the element is that one.
__device__ __forceinline__ float4 pool_first_max(const float* __restrict__ S, size_t pix, int y, int x, int W, int C, int c,
                                                 float4 s, float4 q) {
    bool tx = false, ty = false, tz = false, tw = false;        // an earlier element of the window equals q
    const int r = (y & 1) * 2 + (x & 1);
    const size_t p0 = pix - (size_t)(y & 1) * W - (x & 1);
    for (int j = 0; j < r; ++j) {
        const float4 e = *reinterpret_cast<const float4*>(S + (p0 + (size_t)(j >> 1) * W + (j & 1)) * C + c);
        tx |= e.x == q.x; ty |= e.y == q.y; tz |= e.z == q.z; tw |= e.w == q.w;
    }
    return make_float4(s.x == q.x && !tx ? 1.f : 0.f, s.y == q.y && !ty ? 1.f : 0.f,
                       s.z == q.z && !tz ? 1.f : 0.f, s.w == q.w && !tw ? 1.f : 0.f);
}
struct BwdMegaArgs {
    ConvArgs layer[13];        // in stage order L12 L11 L10 L9 L8 L7 L6 L5 L4 L3 L2 L1 L0 (nimg = all 3B images)
    BwdPool pool[2];           // pool1 (between L4 and L3), pool0 (between L2 and L1)
    unsigned* sync;            // MEGA_SYNC_WORDS words of scratch
};
constexpr int MEGA_SYNC_WORDS = (8 + 32) * 32;    // barrier words of the persistent U-Net kernels: 8 per-XCD + 32 per-group counters, 128 B apart
int launch_unet_dgrad_mega(BwdMegaArgs m, bool bf16, hipStream_t s);

}  // namespace giga
