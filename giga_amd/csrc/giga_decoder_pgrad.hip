// Gradient of the decoder heads with respect to the QUERY POINTS (fp32): d/dp of sum_h <dout_h, head_h(p)>, with the planes held
// constant.  Reference: autograd through conv_onet/models/decoder.py:117-176 w.r.t. p, as used by
// ConvolutionalOccupancyNetwork.grad_refine (models/__init__.py:136-164) and Generator3D.estimate_normals (generation.py:430-455).
//
// decoder_pgrad_kernel, per 32-point tile (lane = point, as in decoder_bwd_kernel) and head:
//   1. recompute the forward chain (same fragments and MFMA order as decoder_f32_kernel), keeping only the ReLU sign masks;
//      fc_out runs as in the forward too, so the optional head outputs are decoder_f32_kernel's bit for bit;
//   2. seed dO with the upstream gradient after the head's epilogue (qual: sigmoid, rot: F.normalize eps 1e-12, width / tsdf:
//      raw), swap the LDS image to the transposed matrices and run decoder_bwd_kernel's gradient chain -- but nothing leaves
//      the registers: no (dY, X) rows, no plane atomics;
//   3. dp = sum_h Wp_h^T DN0_h                                    (fc_p, the 3 x 32 weights read from the forward image)
//         + sum_planes J_plane(p)^T (sum_h dc_h)[plane slice]      (bilinear sample, taps re-read in the D-layout channel order)
//      with d f / d fx = by (f01 - f00) + ay (f11 - f10), d f / d fy = bx (f10 - f00) + ax (f11 - f01) in pixel units,
//      d fx / d p = 39 / 1.00001, and zero for a coordinate that norm_coord clamps (common.py:255-260 writes the clamp in place).
// Planes are the encoder's FINAL planes (after conv_final): the transposed fc_c images exist for those only, so GIGA_FOLD_FINAL
// is not accepted; a caller holding folded planes re-encodes without the flag (giga_amd/convonet.py does).
#include "giga_dev.h"

namespace giga {

struct PgradArgs {
    const float* planes;        // NHWC fp32 [3][B][40][40][32], final planes
    const float* p;             // [P][3]
    const uint8_t* blob;        // forward blob (fp32 images)
    const uint8_t* bwd_blob;    // backward blob (transposed matrices)
    size_t head_off[NHEADS], bwd_off[NHEADS];
    int head_id[NHEADS];
    const float* dout[NHEADS];  // upstream gradients of the post-epilogue outputs
    float* out[NHEADS];         // optional post-epilogue outputs (nullptr: not written)
    float* dp;                  // [P][3], written
    int nheads, B, N;
    long long P;
    int nbatch; float invN;
};

constexpr int PG_NW = 4;        // waves per workgroup, one 32-point tile each (436 VGPRs: one wave per SIMD; 8 waves spill)

template <int CHUNKS>
__device__ __forceinline__ void pg_dma_image(const uint8_t* src, uint8_t* lds_dst, int wave, int lane) {
    for (int c = wave; c < CHUNKS; c += PG_NW)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (size_t)c * FRAG + lane * 16),
                                         (__attribute__((address_space(3))) void*)(lds_dst + c * FRAG), 16, 0, 0);
}

__global__ __launch_bounds__(PG_NW * 64, 1) void decoder_pgrad_kernel(PgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 31, hi = lane >> 5;
    const float4* W = reinterpret_cast<const float4*>(smem);
    const size_t plane_stride = (size_t)a.B * RES * RES * CD;

    for (int bseq = blockIdx.x; bseq < a.nbatch; bseq += gridDim.x) {
        const int batch = xcd_swizzle(bseq, a.nbatch);
        long long g = ((long long)batch * PG_NW + wave) * 32 + n;
        const bool valid = g < a.P;
        if (!valid) g = a.P - 1;
        int b, rdummy;
        split_scene(g, a.N, a.invN, b, rdummy);
        const float px = a.p[3 * g + 0], py = a.p[3 * g + 1], pz = a.p[3 * g + 2];
        const float ax0 = hi ? py : px, ax1 = hi ? 1.0f : pz, ax2 = hi ? 0.0f : 1.0f;
        float cf[48];                                          // B operands: feature pl*32 + 16*hi + s
        {
            const float nx = norm_coord(px), ny = norm_coord(py), nz = norm_coord(pz);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                const Bilin bl = bilin_setup(pl == 2 ? ny : nx, pl == 1 ? ny : nz);     // xz: (x,z)  xy: (x,y)  yz: (y,z)
                const float* base = a.planes + pl * plane_stride + (size_t)b * RES * RES * CD + 16 * hi;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 v00 = *reinterpret_cast<const float4*>(base + (size_t)bl.o00 * CD + 4 * q);
                    const float4 v01 = *reinterpret_cast<const float4*>(base + (size_t)bl.o01 * CD + 4 * q);
                    const float4 v10 = *reinterpret_cast<const float4*>(base + (size_t)bl.o10 * CD + 4 * q);
                    const float4 v11 = *reinterpret_cast<const float4*>(base + (size_t)bl.o11 * CD + 4 * q);
                    cf[16 * pl + 4 * q + 0] = fmaf(v11.x, bl.w11, fmaf(v10.x, bl.w10, fmaf(v01.x, bl.w01, v00.x * bl.w00)));
                    cf[16 * pl + 4 * q + 1] = fmaf(v11.y, bl.w11, fmaf(v10.y, bl.w10, fmaf(v01.y, bl.w01, v00.y * bl.w00)));
                    cf[16 * pl + 4 * q + 2] = fmaf(v11.z, bl.w11, fmaf(v10.z, bl.w10, fmaf(v01.z, bl.w01, v00.z * bl.w00)));
                    cf[16 * pl + 4 * q + 3] = fmaf(v11.w, bl.w11, fmaf(v10.w, bl.w10, fmaf(v01.w, bl.w01, v00.w * bl.w00)));
                }
            }
        }
        f32x16 dc[3];                                          // sum over heads of d/d(sampled features), D layout per plane
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int r = 0; r < 16; ++r) dc[pl][r] = 0.f;
        float dpp[3] = {0.f, 0.f, 0.f};                        // this lane's 16 features of sum_h Wp_h^T DN0_h

        for (int h = 0; h < a.nheads; ++h) {
            // ================= 1. forward recompute (fragment order of giga_pack.cpp::pack_head32) ==================
            __syncthreads();
            pg_dma_image<(int)(DEC32_BYTES / FRAG)>(a.blob + a.head_off[h], smem, wave, lane);
            __builtin_amdgcn_s_waitcnt(0x0F70);
            __syncthreads();
            const float* ctab = reinterpret_cast<const float*>(smem + (size_t)DEC32_FRAGS * FRAG);
            unsigned mnet[NBLK + 1], mhid[NBLK];
            f32x16 net;
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
                unsigned m = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) m |= (net[r] > 0.f ? 1u : 0u) << r;
                mnet[blk] = m;
                f32x16 hcur;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 v = *reinterpret_cast<const float4*>(ctab + blk * 32 + 8 * q + 4 * hi);
                    hcur[4 * q + 0] = v.x; hcur[4 * q + 1] = v.y; hcur[4 * q + 2] = v.z; hcur[4 * q + 3] = v.w;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 A = W[(k++) * 64 + lane];
                    hcur = mfma32(A.x, relu_ieee(net[4 * q + 0]), hcur); hcur = mfma32(A.y, relu_ieee(net[4 * q + 1]), hcur);
                    hcur = mfma32(A.z, relu_ieee(net[4 * q + 2]), hcur); hcur = mfma32(A.w, relu_ieee(net[4 * q + 3]), hcur);
                }
                m = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) m |= (hcur[r] > 0.f ? 1u : 0u) << r;
                mhid[blk] = m;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 A = W[(k++) * 64 + lane];
                    net = mfma32(A.x, relu_ieee(hcur[4 * q + 0]), net); net = mfma32(A.y, relu_ieee(hcur[4 * q + 1]), net);
                    net = mfma32(A.z, relu_ieee(hcur[4 * q + 2]), net); net = mfma32(A.w, relu_ieee(hcur[4 * q + 3]), net);
                }
            }
            {   // + fc_1 bias of the last block -> net5
                const float4 A = W[(k++) * 64 + lane];
                net = mfma32(A.y, ax1, net);
            }
            {
                unsigned m = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) m |= (net[r] > 0.f ? 1u : 0u) << r;
                mnet[NBLK] = m;
            }
            // raw head output z = fc_out(relu(net5)): rows 0..3 of D live in registers 0..3 of the lower lane half
            float z[4];
            {
                f32x16 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 v = *reinterpret_cast<const float4*>(ctab + NBLK * 32 + 8 * q + 4 * hi);
                    o[4 * q + 0] = v.x; o[4 * q + 1] = v.y; o[4 * q + 2] = v.z; o[4 * q + 3] = v.w;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 A = W[(k++) * 64 + lane];
                    o = mfma32(A.x, relu_ieee(net[4 * q + 0]), o); o = mfma32(A.y, relu_ieee(net[4 * q + 1]), o);
                    o = mfma32(A.z, relu_ieee(net[4 * q + 2]), o); o = mfma32(A.w, relu_ieee(net[4 * q + 3]), o);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float t = __shfl_xor(o[j], 32);
                    z[j] = hi ? t : o[j];
                }
            }
            // ================= 2. epilogue and its backward: dO (identical in both lane halves) ======================
            const int id = a.head_id[h];
            float dO[4] = {0.f, 0.f, 0.f, 0.f};
            if (id == 1) {          // r = z / max(|z|, eps): dz = (dr - r (r.dr)) / max(|z|, eps)
                const float nrm = sqrtf(z[0] * z[0] + z[1] * z[1] + z[2] * z[2] + z[3] * z[3]);
                const float inv = 1.0f / fmaxf(nrm, 1e-12f);
                const float r0 = z[0] * inv, r1 = z[1] * inv, r2 = z[2] * inv, r3 = z[3] * inv;
                const float4 d4 = *reinterpret_cast<const float4*>(a.dout[h] + 4 * g);
                const float rd = r0 * d4.x + r1 * d4.y + r2 * d4.z + r3 * d4.w;
                dO[0] = (d4.x - r0 * rd) * inv; dO[1] = (d4.y - r1 * rd) * inv;
                dO[2] = (d4.z - r2 * rd) * inv; dO[3] = (d4.w - r3 * rd) * inv;
                if (a.out[h] && valid && hi == 0) *reinterpret_cast<float4*>(a.out[h] + 4 * g) = make_float4(r0, r1, r2, r3);
            } else {
                float d = a.dout[h][g], v = z[0];
                if (id == 0) { v = 1.0f / (1.0f + expf(-z[0])); d *= v * (1.0f - v); }      // sigmoid'
                dO[0] = d;
                if (a.out[h] && valid && hi == 0) a.out[h][g] = v;
            }
            // ================= 3. swap to the transposed image ===========================================================
            __syncthreads();
            pg_dma_image<(int)(DECB_BYTES / FRAG)>(a.bwd_blob + a.bwd_off[h], smem, wave, lane);
            __builtin_amdgcn_s_waitcnt(0x0F70);
            __syncthreads();
            const float* wout = reinterpret_cast<const float*>(smem + (size_t)DECB_FRAGS * FRAG);   // [4][32]
            // DN[5] = (Wout^T dO) * (net5 > 0)
            f32x16 G;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = (r & 3) + 8 * (r >> 2) + 4 * hi;
                const float v = wout[f] * dO[0] + wout[32 + f] * dO[1] + wout[64 + f] * dO[2] + wout[96 + f] * dO[3];
                G[r] = (mnet[NBLK] >> r & 1u) ? v : 0.f;
            }
            // ================= 4. gradient chain (decoder_bwd_kernel's, registers only) =================================
#pragma unroll
            for (int blk = NBLK - 1; blk >= 0; --blk) {
                const int kb = 20 * blk;
                f32x16 dh;
#pragma unroll
                for (int r = 0; r < 16; ++r) dh[r] = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {                       // W1^T G
                    const float4 A = W[(kb + 16 + q) * 64 + lane];
                    dh = mfma32(A.x, G[4 * q + 0], dh); dh = mfma32(A.y, G[4 * q + 1], dh);
                    dh = mfma32(A.z, G[4 * q + 2], dh); dh = mfma32(A.w, G[4 * q + 3], dh);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) dh[r] = (mhid[blk] >> r & 1u) ? dh[r] : 0.f;
                f32x16 dn;
#pragma unroll
                for (int r = 0; r < 16; ++r) dn[r] = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {                       // W0^T DH
                    const float4 A = W[(kb + 12 + q) * 64 + lane];
                    dn = mfma32(A.x, dh[4 * q + 0], dn); dn = mfma32(A.y, dh[4 * q + 1], dn);
                    dn = mfma32(A.z, dh[4 * q + 2], dn); dn = mfma32(A.w, dh[4 * q + 3], dn);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) G[r] += (mnet[blk] >> r & 1u) ? dn[r] : 0.f;     // DN[blk]
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)                      // dc += Wc^T DN[blk]
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 A = W[(kb + 4 * pl + q) * 64 + lane];
                        dc[pl] = mfma32(A.x, G[4 * q + 0], dc[pl]); dc[pl] = mfma32(A.y, G[4 * q + 1], dc[pl]);
                        dc[pl] = mfma32(A.z, G[4 * q + 2], dc[pl]); dc[pl] = mfma32(A.w, G[4 * q + 3], dc[pl]);
                    }
            }
            // fc_p: dp += Wp^T DN[0].  Wp lives in block 0's aux fragment of the forward image (pack_head32::aux):
            // float 0 of lane f = Wp[f][0], float 0 of lane 32 + f = Wp[f][1], float 1 of lane f = Wp[f][2]
            const float* wp = reinterpret_cast<const float*>(a.blob + a.head_off[h] + (size_t)12 * FRAG);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = (r & 3) + 8 * (r >> 2) + 4 * hi;
                dpp[0] = fmaf(wp[4 * f + 0], G[r], dpp[0]);
                dpp[1] = fmaf(wp[4 * (32 + f) + 0], G[r], dpp[1]);
                dpp[2] = fmaf(wp[4 * f + 1], G[r], dpp[2]);
            }
        }
        // ---------------- bilinear term: J_plane^T dc, this lane's 16 channels 8q + 4hi + j of every plane ----------------
        const float s = 39.0f / 1.00001f;                          // d fx / d p (pix_coord(norm_coord(p)), unclamped)
        const float vx = px / 1.00001f + 0.5f, vy = py / 1.00001f + 0.5f, vz = pz / 1.00001f + 0.5f;
        const float mx = (vx < 1.0f && vx >= 0.0f) ? s : 0.f;      // norm_coord's clamp: zero gradient there
        const float my = (vy < 1.0f && vy >= 0.0f) ? s : 0.f;
        const float mz = (vz < 1.0f && vz >= 0.0f) ? s : 0.f;
        const float nx = norm_coord(px), ny = norm_coord(py), nz = norm_coord(pz);
        float gu[3], gv[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            const float u = pl == 2 ? ny : nx, v = pl == 1 ? ny : nz;
            const Bilin bl = bilin_setup(u, v);
            const float fx = pix_coord(u), fy = pix_coord(v);
            const float x0f = floorf(fx), y0f = floorf(fy);
            const float ax = fx - x0f, ay = fy - y0f, bx = (x0f + 1.0f) - fx, by = (y0f + 1.0f) - fy;
            const float* base = a.planes + pl * plane_stride + (size_t)b * RES * RES * CD + 4 * hi;
            float su = 0.f, sv = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v00 = *reinterpret_cast<const float4*>(base + (size_t)bl.o00 * CD + 8 * q);
                const float4 v01 = *reinterpret_cast<const float4*>(base + (size_t)bl.o01 * CD + 8 * q);
                const float4 v10 = *reinterpret_cast<const float4*>(base + (size_t)bl.o10 * CD + 8 * q);
                const float4 v11 = *reinterpret_cast<const float4*>(base + (size_t)bl.o11 * CD + 8 * q);
                const float f00[4] = {v00.x, v00.y, v00.z, v00.w}, f01[4] = {v01.x, v01.y, v01.z, v01.w};
                const float f10[4] = {v10.x, v10.y, v10.z, v10.w}, f11[4] = {v11.x, v11.y, v11.z, v11.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float d = dc[pl][4 * q + j];
                    su = fmaf(d, by * (f01[j] - f00[j]) + ay * (f11[j] - f10[j]), su);
                    sv = fmaf(d, bx * (f10[j] - f00[j]) + ax * (f11[j] - f01[j]), sv);
                }
            }
            gu[pl] = su; gv[pl] = sv;
        }
        // xz: (u, v) = (x, z)   xy: (x, y)   yz: (y, z)
        float dx = dpp[0] + mx * (gu[0] + gu[1]);
        float dy = dpp[1] + my * (gv[1] + gu[2]);
        float dz = dpp[2] + mz * (gv[0] + gv[2]);
        dx += __shfl_xor(dx, 32); dy += __shfl_xor(dy, 32); dz += __shfl_xor(dz, 32);
        if (valid && hi == 0) {
            a.dp[3 * g + 0] = dx; a.dp[3 * g + 1] = dy; a.dp[3 * g + 2] = dz;
        }
    }
}

int launch_decoder_point_grad(const float* planes, const float* p, const uint8_t* blob, const uint8_t* bwd_blob, int head_mask,
                              const float* const* douts, float* const* outs, float* dp, int B, int N, hipStream_t s) {
    const long long P = (long long)B * N;
    const PackOff ko = pack_offsets();
    const BwdPackOff bo = bwd_pack_offsets();
    PgradArgs a{};
    a.planes = planes; a.p = p; a.blob = blob; a.bwd_blob = bwd_blob; a.dp = dp;
    a.B = B; a.N = N; a.P = P; a.invN = 1.0f / (float)N;
    for (int h = 0; h < NHEADS; ++h) {
        if (!(head_mask >> h & 1)) continue;
        a.head_id[a.nheads] = h; a.head_off[a.nheads] = ko.dec32[h]; a.bwd_off[a.nheads] = bo.dec[h];
        a.dout[a.nheads] = douts[h]; a.out[a.nheads] = outs[h];
        ++a.nheads;
    }
    const long long tiles = (P + 31) / 32;
    a.nbatch = (int)((tiles + PG_NW - 1) / PG_NW);
    const int grid = a.nbatch < 256 ? a.nbatch : 256;
    const size_t lds = DEC32_BYTES > DECB_BYTES ? DEC32_BYTES : DECB_BYTES;
    giga::dyn_lds_once(reinterpret_cast<const void*>(decoder_pgrad_kernel), (int)lds);
    GIGA_LAUNCH(decoder_pgrad_kernel, dim3(grid), dim3(PG_NW * 64), lds, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // namespace giga
