// Pieces shared by the decoder kernels (giga_decoder.hip, giga_decoder_bwd.hip, giga_decoder_pgrad.hip, giga_decoder_train16.hip):
// the LDS-DMA fill of a fragment image, the D-register layout idioms, the bilinear gather of the 96 plane features in its two
// fp32 forms, the [.][96] row store of the training decoders, the f16 aux operand, and the fp32 recompute / gradient chain that the backward and the point-gradient kernel run on
// the same fragments in the same MFMA order.
#pragma once
#include "giga_dev.h"

namespace giga {

// CHUNKS fragments (64 lanes x 16 B each) of a packed image by LDS-DMA (global_load_lds_dwordx4, no VGPR round trip), dealt over
// the workgroup's NW waves.  The caller waits (vmcnt(0) through the builtin, then the workgroup barrier).
template <int NW, int CHUNKS>
__device__ __forceinline__ void lds_dma_frags(const uint8_t* src, uint8_t* lds_dst, int wave, int lane) {
    for (int c = wave; c < CHUNKS; c += NW)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)c * FRAG + lane * 16),
                                         (__attribute__((address_space(3))) void*)(lds_dst + c * FRAG), 16, 0, 0);
}

// Head-resident f16-class kernels (decoder_f16s_kernel, decoder_lat_kernel): workgroup -> (head, slot of the head's tile or slab
// range), slots = workgroups per head.  Workgroup i runs on XCD i % 8; when the grid is a multiple of 8 * nheads the slots of one XCD
// are made contiguous (an eighth of the points = an eighth of the scenes: their planes stay in that XCD's L2; with the plain
// i % nheads / i / nheads map every XCD walked every scene: 527 MB of fabric traffic per launch).  dec_plan (giga_dec_plan.h) reports
// the same condition as xcd_remap.
__device__ __forceinline__ void dec16_head_slot(int nheads, int& hsel, int& slot, int& slots) {
    slots = gridDim.x / nheads;
    hsel = blockIdx.x % nheads;
    slot = blockIdx.x / nheads;
    if (gridDim.x % (8 * nheads) == 0) {
        const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3, spx = slots >> 3;
        hsel = k % nheads;
        slot = xcd * spx + k / nheads;
    }
}

// ---- D layout of the 32x32 MFMAs: register r of lane half hi holds feature (row) drow(r, hi) of the lane's point ----
__device__ __forceinline__ int drow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }
// row `row` of a head image's C table (32 biases) as an accumulator image
__device__ __forceinline__ f32x16 ctab_row(const float* ctab, int row, int hi) {
    f32x16 c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(ctab + row * 32 + 8 * q + 4 * hi);
        c[4 * q + 0] = v.x; c[4 * q + 1] = v.y; c[4 * q + 2] = v.z; c[4 * q + 3] = v.w;
    }
    return c;
}
// bit r = (x[r] > 0): all the backward chains need of a pre-activation
__device__ __forceinline__ unsigned sign_mask(const f32x16& x) {
    unsigned m = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) m |= (x[r] > 0.f ? 1u : 0u) << r;
    return m;
}

// a . b over four terms as four rounded products summed left to right.  Contraction is switched off for it: left to the optimiser,
// `a0 * b0 + a1 * b1 + ...` came out as separate multiplies and adds or as an fma chain depending on the code AROUND the expression
// (the normalize backward of the rot head did), and the two differ in the last bits.
__device__ __forceinline__ float dot4_rn(float a0, float b0, float a1, float b1, float a2, float b2, float a3, float b3) {
#pragma clang fp contract(off)
    return a0 * b0 + a1 * b1 + a2 * b2 + a3 * b3;
}

// ---- bilinear sample of four channels, the fma order of aten's grid_sampler: nw, ne, sw, se ----
__device__ __forceinline__ float4 bilerp(const float4& v00, const float4& v01, const float4& v10, const float4& v11,
                                         float w00, float w01, float w10, float w11) {
    float4 o;
    o.x = fmaf(v11.x, w11, fmaf(v10.x, w10, fmaf(v01.x, w01, v00.x * w00)));
    o.y = fmaf(v11.y, w11, fmaf(v10.y, w10, fmaf(v01.y, w01, v00.y * w00)));
    o.z = fmaf(v11.z, w11, fmaf(v10.z, w10, fmaf(v01.z, w01, v00.z * w00)));
    o.w = fmaf(v11.w, w11, fmaf(v10.w, w10, fmaf(v01.w, w01, v00.w * w00)));
    return o;
}
// the same on the four taps of `bl`, channels off .. off + 3 of the pixel rows at `base`
__device__ __forceinline__ float4 bilerp(const float* base, const Bilin& bl, int off = 0) {
    return bilerp(*reinterpret_cast<const float4*>(base + (size_t)bl.o00 * CD + off), *reinterpret_cast<const float4*>(base + (size_t)bl.o01 * CD + off),
                  *reinterpret_cast<const float4*>(base + (size_t)bl.o10 * CD + off), *reinterpret_cast<const float4*>(base + (size_t)bl.o11 * CD + off),
                  bl.w00, bl.w01, bl.w10, bl.w11);
}

// Per-lane gather of a point's fp32 B operands from NHWC planes [3][B][40][40][32]: cf[16 pl + s] = feature pl*32 + 16*hi + s of
// scene b at the footprints bl[pl]  (xz: (x,z)  xy: (x,y)  yz: (y,z), common.py:246-251)
__device__ __forceinline__ void gather_plane16(const float* base, const Bilin& bl, float* cf16) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 o = bilerp(base, bl, 4 * q);
        cf16[4 * q + 0] = o.x; cf16[4 * q + 1] = o.y; cf16[4 * q + 2] = o.z; cf16[4 * q + 3] = o.w;
    }
}
__device__ __forceinline__ void gather_direct48(const float* planes, size_t plane_stride, int b, const Bilin (&bl)[3], int hi,
                                                float (&cf)[48]) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
        gather_plane16(planes + pl * plane_stride + (size_t)b * RES * RES * CD + 16 * hi, bl[pl], cf + 16 * pl);
}
// the same from the normalised coordinates, for a caller that does not keep the footprints
__device__ __forceinline__ void gather_direct48(const float* planes, size_t plane_stride, int b, float nx, float ny, float nz, int hi,
                                                float (&cf)[48]) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        const Bilin bl = bilin_setup(pl == 2 ? ny : nx, pl == 1 ? ny : nz);
        gather_plane16(planes + pl * plane_stride + (size_t)b * RES * RES * CD + 16 * hi, bl, cf + 16 * pl);
    }
}

// Line-friendly gather of a 32-point tile (points tile0 .. tile0 + 31 of p [P][3], clamped to P - 1).  A load in which every lane
// fetches 16 B of its OWN point touches 64 cache lines; here four adjacent lanes fetch the four 16-B quads of one (point, channel
// half), one whole 64-B line per four lanes, interpolate them, and the tile is transposed to the operand layout (lane = point,
// cf as in gather_direct48) through the wave-private stage S [32][96].  DS operations of one wave execute in order: no barrier.
__device__ __forceinline__ void gather_staged48(float* S, const float* planes, size_t plane_stride, const float* p, long long tile0,
                                                long long P, int N, float invN, int lane, float (&cf)[48]) {
    const int n = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int part = 0; part < 4; ++part) {
        const int pair = part * 16 + (lane >> 2), pt = pair >> 1, hf = pair & 1, qd = lane & 3;
        long long gp = tile0 + pt;
        if (gp >= P) gp = P - 1;
        int bp, rp;
        split_scene(gp, N, invN, bp, rp);
        const float nx = norm_coord(p[3 * gp + 0]), ny = norm_coord(p[3 * gp + 1]), nz = norm_coord(p[3 * gp + 2]);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            const Bilin bl = bilin_setup(pl == 2 ? ny : nx, pl == 1 ? ny : nz);
            const float* base = planes + pl * plane_stride + (size_t)bp * RES * RES * CD + 16 * hf + 4 * qd;
            *reinterpret_cast<float4*>(S + pt * 96 + pl * 32 + 16 * hf + 4 * qd) = bilerp(base, bl);
        }
    }
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(S + n * 96 + pl * 32 + 16 * hi + 4 * q);
            cf[16 * pl + 4 * q + 0] = v.x; cf[16 * pl + 4 * q + 1] = v.y; cf[16 * pl + 4 * q + 2] = v.z; cf[16 * pl + 4 * q + 3] = v.w;
        }
}

// ---- rows of [.][96] from D-layout images (lane = point, registers = features drow(r, hi)), features 0..95 in order: the training
// decoders' dc rows for plane_gather_kernel in HBM and the value part of their scatter stages in LDS.  One plane's 32 features:
template <class Row>
__device__ __forceinline__ void store_row96_plane(float* dst, Row row, int hi, int pl, const f32x16& v) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(dst + row * 96 + pl * 32 + 8 * q + 4 * hi) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}
// all three planes
template <class Row>
__device__ __forceinline__ void store_row96(float* dst, Row row, int hi, const f32x16 (&v)[3]) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) store_row96_plane(dst, row, hi, pl, v[pl]);
}

// aux operand of the f16 chains: [p_hi(3), 1, p_lo(3), 1] on hi = 0 lanes, [p_hi(3), 0 ...] on hi = 1 lanes (exact by itself)
__device__ __forceinline__ half8 aux_half8(float px, float py, float pz, int hi) {
    const half_t xh = (half_t)px, yh = (half_t)py, zh = (half_t)pz;
    half8 av = {xh, yh, zh, (half_t)0, (half_t)0, (half_t)0, (half_t)0, (half_t)0};
    if (hi == 0) {
        av[3] = (half_t)1.0f;
        av[4] = (half_t)(px - (float)xh); av[5] = (half_t)(py - (float)yh);
        av[6] = (half_t)(pz - (float)zh); av[7] = (half_t)1.0f;
    }
    return av;
}

// =============================== the fp32 chain of the backward kernels =============================================
// decoder_bwd_kernel and decoder_pgrad_kernel recompute the forward on the fp32 head image (fragment order of
// giga_pack.cpp::pack_head32, the MFMA order of decoder_f32_kernel) and run the gradient chain on the transposed image
// (giga_pack.cpp::pack_bwd: block b -> Wc^T 20b..20b+11, W0^T +12..15, W1^T +16..19).  lane = point, registers = features.
// A Tap sees every tensor the weight-gradient GEMMs need as it comes to exist: tap(slot, values) with the row-array index of
// decoder_bwd_kernel as slot (11 + blk XN, 16 + blk XH, 21 XO, 6 + blk DH, blk DN).  Tap::active == false: nothing is formed for it.
struct Dec32NoTap {
    static constexpr bool active = false;
    __device__ __forceinline__ void operator()(int, const f32x16&) const {}
};

// acc += W(fragments k0 .. k0+3) x (RELU ? relu(x) : x): 16 MFMAs on one accumulator, registers of x in order
template <bool RELU>
__device__ __forceinline__ f32x16 dec32_dense(const float4* W, int k0, int lane, const f32x16& x, f32x16 acc) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 A = W[(k0 + q) * 64 + lane];
        if constexpr (RELU) {
            acc = mfma32(A.x, relu_ieee(x[4 * q + 0]), acc); acc = mfma32(A.y, relu_ieee(x[4 * q + 1]), acc);
            acc = mfma32(A.z, relu_ieee(x[4 * q + 2]), acc); acc = mfma32(A.w, relu_ieee(x[4 * q + 3]), acc);
        } else {
            acc = mfma32(A.x, x[4 * q + 0], acc); acc = mfma32(A.y, x[4 * q + 1], acc);
            acc = mfma32(A.z, x[4 * q + 2], acc); acc = mfma32(A.w, x[4 * q + 3], acc);
        }
    }
    return acc;
}
// the sign mask of a pre-activation; an active tap gets relu(x) (the X operand of the next layer's weight gradient)
template <class Tap>
__device__ __forceinline__ unsigned dec32_mask_tap(const f32x16& x, int slot, const Tap& tap) {
    if constexpr (Tap::active) {
        f32x16 t;
        unsigned m = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) { t[r] = relu_ieee(x[r]); m |= (x[r] > 0.f ? 1u : 0u) << r; }
        tap(slot, t);
        return m;
    } else {
        return sign_mask(x);
    }
}
// Forward recompute up to net5 (the stream in front of fc_out): per block fc_c (12 fragments on cf) + aux (ax0, ax1, ax2),
// fc_0 on the C-table row, fc_1 onto the stream; then the last fc_1 bias.  Only the signs stay: mnet[blk] of the stream in front
// of block blk (mnet[NBLK]: net5), mhid[blk] of the hidden pre-activation.  Returns the index of the next fragment (fc_out's first).
template <class Tap>
__device__ __forceinline__ int dec32_recompute(const float4* W, const float* ctab, int lane, int hi, const float (&cf)[48], float ax0,
                                               float ax1, float ax2, unsigned (&mnet)[NBLK + 1], unsigned (&mhid)[NBLK], f32x16& net,
                                               const Tap& tap) {
#pragma unroll
    for (int r = 0; r < 16; ++r) net[r] = 0.f;
    int k = 0;
#pragma unroll
    for (int blk = 0; blk < NBLK; ++blk) {
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            const float4 A = W[(k++) * 64 + lane];
            net = mfma32(A.x, cf[4 * q + 0], net); net = mfma32(A.y, cf[4 * q + 1], net);
            net = mfma32(A.z, cf[4 * q + 2], net); net = mfma32(A.w, cf[4 * q + 3], net);
        }
        {
            const float4 A = W[(k++) * 64 + lane];
            net = mfma32(A.x, ax0, net); net = mfma32(A.y, ax1, net); net = mfma32(A.z, ax2, net);
        }
        mnet[blk] = dec32_mask_tap(net, 11 + blk, tap);                       // XN[blk]
        f32x16 hcur = dec32_dense<true>(W, k, lane, net, ctab_row(ctab, blk, hi));
        k += 4;
        net = dec32_dense<true>(W, k, lane, hcur, net);
        k += 4;
        mhid[blk] = dec32_mask_tap(hcur, 16 + blk, tap);                      // XH[blk] (no MFMA waits for it: behind fc_1)
    }
    {   // + fc_1 bias of the last block -> net5
        const float4 A = W[(k++) * 64 + lane];
        net = mfma32(A.y, ax1, net);
    }
    mnet[NBLK] = dec32_mask_tap(net, 21, tap);                                // XO
    return k;
}
// DN[5] = (Wout^T dO) * (net5 > 0); wout: [4][32] behind the transposed image.  The sum over the (at most four) outputs is written
// out in both roundings the two kernels had before they shared this code -- the compiler had turned the same source line into an
// fma chain in decoder_bwd_kernel (FUSED) and into four products and three sums in decoder_pgrad_kernel -- so that each keeps its
// bits; they differ for the rot head only (one output: the other three terms are exact zeros).
template <bool FUSED>
__device__ __forceinline__ f32x16 dec32_dn5(const float* wout, const float (&dO)[4], unsigned mask5, int hi) {
    f32x16 G;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int f = drow(r, hi);
        float v;
        if constexpr (FUSED) v = fmaf(wout[96 + f], dO[3], fmaf(wout[64 + f], dO[2], fmaf(wout[f], dO[0], wout[32 + f] * dO[1])));
        else v = dot4_rn(wout[f], dO[0], wout[32 + f], dO[1], wout[64 + f], dO[2], wout[96 + f], dO[3]);
        G[r] = (mask5 >> r & 1u) ? v : 0.f;
    }
    return G;
}
// G = DN[blk + 1] on entry of a block:  DH[blk] = (W1^T G) * (h > 0);  G = DN[blk] = G + (W0^T DH[blk]) * (net > 0);  dc += Wc^T DN[blk].
// G leaves as DN[0].
template <class Tap>
__device__ __forceinline__ void dec32_grad_chain(const float4* W, int lane, f32x16& G, const unsigned (&mnet)[NBLK + 1],
                                                 const unsigned (&mhid)[NBLK], f32x16 (&dc)[3], const Tap& tap) {
    f32x16 zero;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero[r] = 0.f;
#pragma unroll
    for (int blk = NBLK - 1; blk >= 0; --blk) {
        const int kb = 20 * blk;
        f32x16 dh = dec32_dense<false>(W, kb + 16, lane, G, zero);             // W1^T G
#pragma unroll
        for (int r = 0; r < 16; ++r) dh[r] = (mhid[blk] >> r & 1u) ? dh[r] : 0.f;
        tap(6 + blk, dh);
        const f32x16 dn = dec32_dense<false>(W, kb + 12, lane, dh, zero);      // W0^T DH
#pragma unroll
        for (int r = 0; r < 16; ++r) G[r] += (mnet[blk] >> r & 1u) ? dn[r] : 0.f;
        tap(blk, G);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) dc[pl] = dec32_dense<false>(W, kb + 4 * pl, lane, G, dc[pl]);    // dc += Wc^T DN[blk]
    }
}

}  // namespace giga
