// Gradient of the decoder heads with respect to the QUERY POINTS (fp32): d/dp of sum_h <dout_h, head_h(p)>, with the planes held
// constant.  Reference: autograd through conv_onet/models/decoder.py:117-176 w.r.t. p, as used by
// ConvolutionalOccupancyNetwork.grad_refine (models/__init__.py:136-164) and Generator3D.estimate_normals (generation.py:430-455).
//
// decoder_pgrad_kernel, per 32-point tile (lane = point, as in decoder_bwd_kernel) and head:
//   1. recompute the forward chain (same fragments and MFMA order as decoder_f32_kernel), keeping only the ReLU sign masks;
//      fc_out runs as in the forward too, so the optional head outputs are decoder_f32_kernel's bit for bit;
//   2. seed dO with the upstream gradient after the head's epilogue (qual: sigmoid, rot: F.normalize eps 1e-12, width / tsdf:
//      raw), swap the LDS image to the transposed matrices and run decoder_bwd_kernel's gradient chain -- but nothing leaves
//      the registers: no (dY, X) rows, no plane atomics (the recompute and the chain are giga_dec_common.h's, with an empty tap);
//   3. dp = sum_h Wp_h^T DN0_h                                    (fc_p, the 3 x 32 weights read from the forward image)
//         + sum_planes J_plane(p)^T (sum_h dc_h)[plane slice]      (bilinear sample, taps re-read in the D-layout channel order)
//      with d f / d fx = by (f01 - f00) + ay (f11 - f10), d f / d fy = bx (f10 - f00) + ax (f11 - f01) in pixel units,
//      d fx / d p = 39 / 1.00001, and zero for a coordinate that norm_coord clamps (common.py:255-260 writes the clamp in place).
// Planes are the encoder's FINAL planes (after conv_final): the transposed fc_c images exist for those only, so GIGA_FOLD_FINAL
// is not accepted; a caller holding folded planes re-encodes without the flag (giga_amd/convonet.py does).
//
// decoder_pgrad_kernel<true> (giga_decoder_point_hess, mesh refinement) adds the second derivative of the occupancy logit f.  The
// heads are piecewise linear in (p, c) and c(p) is bilinear per plane, so almost everywhere the Hessian of f has a zero diagonal and
// one entry per plane, d2 f / du dv = s_u s_v sum_ch dc[plane][ch] (f00 - f01 - f10 + f11)[ch], accumulated against the dc the tile
// holds anyway.  That instantiation runs the occupancy head alone with upstream gradient 1 and writes the raw logit, dp and
// (H_xy, H_xz, H_yz); logit and dp are <false>'s bit for bit.  <false> is the point gradient as it was before the template.
#include "giga_dec_common.h"
#include "../../include/giga_hip.h"

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
    float* hess;                // HESS: [P][3] = (H_xy, H_xz, H_yz), written (last: the other offsets are the point gradient's)
};

constexpr int PG_NW = 4;        // waves per workgroup, one 32-point tile each (436 VGPRs: one wave per SIMD; 8 waves spill)

template <bool HESS>
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
        f32x16 dc[3];                                          // sum over heads of d/d(sampled features), D layout per plane
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int r = 0; r < 16; ++r) dc[pl][r] = 0.f;
        float dpp[3] = {0.f, 0.f, 0.f};                        // this lane's 16 features of sum_h Wp_h^T DN0_h
        float cf[48];                                          // B operands: feature pl*32 + 16*hi + s
        gather_direct48(a.planes, plane_stride, b, norm_coord(px), norm_coord(py), norm_coord(pz), hi, cf);

        for (int h = 0; h < a.nheads; ++h) {
            // ================= 1. forward recompute (fragment order of giga_pack.cpp::pack_head32), signs only ==========
            __syncthreads();
            lds_dma_frags<PG_NW, (int)(DEC32_BYTES / FRAG)>(a.blob + a.head_off[h], smem, wave, lane);
            __builtin_amdgcn_s_waitcnt(0x0F70);
            __syncthreads();
            const float* ctab = reinterpret_cast<const float*>(smem + (size_t)DEC32_FRAGS * FRAG);
            unsigned mnet[NBLK + 1], mhid[NBLK];
            f32x16 net;
            const int k = dec32_recompute(W, ctab, lane, hi, cf, ax0, ax1, ax2, mnet, mhid, net, Dec32NoTap{});
            // raw head output z = fc_out(relu(net5)): rows 0..3 of D live in registers 0..3 of the lower lane half
            float z[4];
            {
                const f32x16 o = dec32_dense<true>(W, k, lane, net, ctab_row(ctab, NBLK, hi));
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
                const float rd = dot4_rn(r0, d4.x, r1, d4.y, r2, d4.z, r3, d4.w);
                dO[0] = (d4.x - r0 * rd) * inv; dO[1] = (d4.y - r1 * rd) * inv;
                dO[2] = (d4.z - r2 * rd) * inv; dO[3] = (d4.w - r3 * rd) * inv;
                if (a.out[h] && valid && hi == 0) *reinterpret_cast<float4*>(a.out[h] + 4 * g) = make_float4(r0, r1, r2, r3);
            } else {
                float d = 1.0f, v = z[0];
                if constexpr (HESS) asm volatile("" : "+v"(d));     // upstream gradient 1, opaque: the chain compiles as <false>'s
                else d = a.dout[h][g];
                if (id == 0) { v = 1.0f / (1.0f + expf(-z[0])); d *= v * (1.0f - v); }      // sigmoid'
                dO[0] = d;
                if (a.out[h] && valid && hi == 0) a.out[h][g] = v;
            }
            // ================= 3. swap to the transposed image ===========================================================
            __syncthreads();
            lds_dma_frags<PG_NW, (int)(DECB_BYTES / FRAG)>(a.bwd_blob + a.bwd_off[h], smem, wave, lane);
            __builtin_amdgcn_s_waitcnt(0x0F70);
            __syncthreads();
            const float* wout = reinterpret_cast<const float*>(smem + (size_t)DECB_FRAGS * FRAG);   // [4][32]
            // ================= 4. gradient chain (decoder_bwd_kernel's, registers only) =================================
            f32x16 G = dec32_dn5<false>(wout, dO, mnet[NBLK], hi);
            dec32_grad_chain(W, lane, G, mnet, mhid, dc, Dec32NoTap{});
            // fc_p: dp += Wp^T DN[0].  Wp lives in block 0's aux fragment of the forward image (pack_head32::aux):
            // float 0 of lane f = Wp[f][0], float 0 of lane 32 + f = Wp[f][1], float 1 of lane f = Wp[f][2]
            const float* wp = reinterpret_cast<const float*>(a.blob + a.head_off[h] + (size_t)12 * FRAG);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = drow(r, hi);
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
        if constexpr (HESS) {                                      // one cross term per plane; a clamped axis zeroes its entries
            // The taps are read again (cache hits) through a pointer the compiler cannot see through, in a loop of their own:
            // sharing the loop above changes which of its multiply-adds get fused, and dp must stay <false>'s bit for bit.
            float guv[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                const float u = pl == 2 ? ny : nx, v = pl == 1 ? ny : nz;
                const Bilin bl = bilin_setup(u, v);
                const float* base = a.planes + pl * plane_stride + (size_t)b * RES * RES * CD + 4 * hi;
                asm volatile("" : "+v"(base));
                float suv = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 v00 = *reinterpret_cast<const float4*>(base + (size_t)bl.o00 * CD + 8 * q);
                    const float4 v01 = *reinterpret_cast<const float4*>(base + (size_t)bl.o01 * CD + 8 * q);
                    const float4 v10 = *reinterpret_cast<const float4*>(base + (size_t)bl.o10 * CD + 8 * q);
                    const float4 v11 = *reinterpret_cast<const float4*>(base + (size_t)bl.o11 * CD + 8 * q);
                    suv = fmaf(dc[pl][4 * q + 0], (v00.x - v01.x) - (v10.x - v11.x), suv);
                    suv = fmaf(dc[pl][4 * q + 1], (v00.y - v01.y) - (v10.y - v11.y), suv);
                    suv = fmaf(dc[pl][4 * q + 2], (v00.z - v01.z) - (v10.z - v11.z), suv);
                    suv = fmaf(dc[pl][4 * q + 3], (v00.w - v01.w) - (v10.w - v11.w), suv);
                }
                guv[pl] = suv;
            }
            float hxy = mx * my * guv[1], hxz = mx * mz * guv[0], hyz = my * mz * guv[2];
            hxy += __shfl_xor(hxy, 32); hxz += __shfl_xor(hxz, 32); hyz += __shfl_xor(hyz, 32);
            if (valid && hi == 0) {
                a.hess[3 * g + 0] = hxy; a.hess[3 * g + 1] = hxz; a.hess[3 * g + 2] = hyz;
            }
        }
    }
}

template <bool HESS>
static int launch_pgrad(const float* planes, const float* p, const uint8_t* blob, const uint8_t* bwd_blob, int head_mask,
                        const float* const* douts, float* const* outs, float* dp, float* hess, int B, int N, hipStream_t s) {
    const long long P = (long long)B * N;
    const PackOff ko = pack_offsets();
    const BwdPackOff bo = bwd_pack_offsets();
    PgradArgs a{};
    a.planes = planes; a.p = p; a.blob = blob; a.bwd_blob = bwd_blob; a.dp = dp; a.hess = hess;
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
    giga::dyn_lds_once(reinterpret_cast<const void*>(decoder_pgrad_kernel<HESS>), (int)lds);
    GIGA_LAUNCH(decoder_pgrad_kernel<HESS>, dim3(grid), dim3(PG_NW * 64), lds, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // namespace giga

using namespace giga;

extern "C" {

int giga_decoder_point_grad(const void* planes_nhwc, const float* p, const void* packed, const void* bwd_packed,
                            int head_mask, const float* dqual, const float* drot, const float* dwidth, const float* dtsdf,
                            float* dp, float* out_qual, float* out_rot, float* out_width, float* out_tsdf,
                            int B, int N, int flags, void* stream) {
    if (head_mask <= 0 || (head_mask & ~15) != 0) return -1;
    if (B <= 0 || N <= 0) return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    if ((long long)B * N >= (1LL << 31)) return -1;         // split_scene's point index is exact below 2^31
    if (flags != 0) return -5;
    if (!planes_nhwc || !p || !packed || !bwd_packed || !dp) return -1;
    const float* douts[NHEADS] = {dqual, drot, dwidth, dtsdf};
    float* outs[NHEADS] = {out_qual, out_rot, out_width, out_tsdf};
    for (int h = 0; h < NHEADS; ++h)
        if ((head_mask >> h & 1) && !douts[h]) return -6;
    return launch_pgrad<false>(static_cast<const float*>(planes_nhwc), p, static_cast<const uint8_t*>(packed),
                               static_cast<const uint8_t*>(bwd_packed), head_mask, douts, outs, dp, nullptr, B, N,
                               static_cast<hipStream_t>(stream));
}

// occupancy head alone, upstream gradient 1: raw logit, dp and the three Hessian entries per point
int giga_decoder_point_hess(const void* planes_nhwc, const float* p, const void* packed, const void* bwd_packed, float* logit,
                            float* dp, float* hess, int B, int N, void* stream) {
    if (B <= 0 || N <= 0) return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    if ((long long)B * N >= (1LL << 31)) return -1;         // split_scene's point index is exact below 2^31
    if (!planes_nhwc || !p || !packed || !bwd_packed || !logit || !dp || !hess) return -1;
    const float* douts[NHEADS] = {nullptr, nullptr, nullptr, nullptr};
    float* outs[NHEADS] = {nullptr, nullptr, nullptr, logit};
    return launch_pgrad<true>(static_cast<const float*>(planes_nhwc), p, static_cast<const uint8_t*>(packed),
                              static_cast<const uint8_t*>(bwd_packed), 8, douts, outs, dp, hess, B, N, static_cast<hipStream_t>(stream));
}

}  // extern "C"
