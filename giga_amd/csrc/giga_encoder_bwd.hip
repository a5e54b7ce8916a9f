// Encoder backward (training path, fp32): gradients of every LocalVoxelEncoder / UNet parameter
// (reference: autograd through ConvONets/encoder/voxels.py:89-121 and encoder/unet.py:225-239, driven by
// scripts/train_giga.py:198-211).
//   * data gradients of the convolutions reuse conv16_kernel with flipped/transposed weight fragments
//     (backward blob, giga_pack.cpp::pack_conv_dgrad); ConvTranspose2d's data gradient is the DOWN kind
//   * weight gradients: conv_wgrad_kernel, an MFMA reduction over pixels D[co][ci] += dY[p][co] * X[p+tap][ci]
//   * ReLU / max-pool / concat backward: small elementwise kernels on the saved NHWC activations
//   * conv_in: recompute the pre-activation (never stored by the forward), mask, and reduce
//     dW[c][tap] = sum_voxels dF[c][v] * tsdf[v + tap] on the MFMA as well.
// Weight/bias gradients are ACCUMULATED into the flat fp32 gradient buffer (reference state-dict order) with
// fp32 atomics (summation order is not fixed, as with PyTorch's own CUDA/HIP backward kernels).
#include "../../include/giga_hip.h"
#include "giga_conv16.h"
#include "giga_wino.h"
#include "giga_wgrad3.h"
#include <atomic>
#include <functional>
#include <mutex>

#include "giga_side.h"
#include "giga_args.h"
#include "giga_enc_plan.h"

namespace giga {

// ------------------------------- elementwise ------------------------------------------------------------
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
// dS[img][y][x][c] = dCat[img][y][x][coff + c] (skip half of the concat gradient, channel stride cs)
//                  + (S[y][x][c] is the first of its window == Q[y/2][x/2][c] ? dQ[y/2][x/2][c] : 0)   (MaxPool2d(2,2)
// backward: ties go to the first maximum in row-major window order, as in torch; pool_first_max)
// and, S being the ReLU output of the layer below, its backward in the same pass: dS = S > 0 ? dS : 0
// (one thread per FOUR channels: 16-byte loads and stores; C, cs and coff are multiples of 4)
__global__ void pool_bwd_add_kernel(float* __restrict__ dS, const float* __restrict__ dcat, int cs, int coff,
                                    const float* __restrict__ dQ, const float* __restrict__ S,
                                    const float* __restrict__ Q, int nimg, int H, int W, int C) {
    const int C4 = C >> 2;
    const size_t total = (size_t)nimg * H * W * C4;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = 4 * (int)(i % C4);
    const size_t pix = i / C4;
    const int x = (int)(pix % W), y = (int)((pix / W) % H);
    const size_t img = pix / ((size_t)W * H);
    const size_t qi = ((img * (H / 2) + y / 2) * (W / 2) + x / 2) * C + c;
    const float4 s = *reinterpret_cast<const float4*>(S + pix * C + c);
    const float4 d = *reinterpret_cast<const float4*>(dcat + pix * cs + coff + c);
    const float4 q = *reinterpret_cast<const float4*>(Q + qi);
    const float4 g = *reinterpret_cast<const float4*>(dQ + qi);
    const float4 f = pool_first_max(S, pix, y, x, W, C, c, s, q);
    float4 o;
    o.x = s.x > 0.f ? d.x + (f.x != 0.f ? g.x : 0.f) : 0.f;
    o.y = s.y > 0.f ? d.y + (f.y != 0.f ? g.y : 0.f) : 0.f;
    o.z = s.z > 0.f ? d.z + (f.z != 0.f ? g.z : 0.f) : 0.f;
    o.w = s.w > 0.f ? d.w + (f.w != 0.f ? g.w : 0.f) : 0.f;
    *reinterpret_cast<float4*>(dS + pix * C + c) = o;
}

// ------------------------------- weight gradient (MFMA reduction over pixels) ----------------------------
// D[m][n] += sum_p R[p][m] * Cc[map(p, tap)][n]   on v_mfma_f32_32x32x2_f32 (2 pixels per MFMA).
//   CONV3 / CONV1 : R = dPre (m = co), Cc = layer input at the tap-shifted pixel (n = ci, zero outside)
//   UPCONV        : R = layer input (m = ci), Cc = dU at (2y+dy, 2x+dx) (n = co)
// Operands come straight from HBM/L2 (32 lanes x 4 B contiguous per pixel), no LDS staging: one MFMA
// (64 cycles) per two 128-byte loads.  Block = (tap, 32x32 block of dW, pixel range); its 16 waves split
// the range, partials are summed through LDS and added to the gradient buffer with one atomic per element.
// ~256 workgroups per launch: these launches are bound by their ATOMICS, not by the reduction (float atomics are fabric
// operations, and all pixel ranges of a block hit the same 1024 addresses): with 768 workgroups of 4 waves the 1x1 layer's
// gradient took 39 us and the two ConvTranspose layers' 31 us each for 4-5 us of loads and MFMAs; a third of the workgroups
// with four times the waves issue a third of the atomics and keep the same number of loads in flight.
struct WgradArgs {
    const float* R; int csR, coR;                 // row tensor, channel stride, first channel
    const float* C0p; const float* C1p;           // column tensor(s) (concat order), channel strides / split
    int csC0, csC1, nC0;                          // columns n < nC0 come from C0p, the rest from C1p
    float* dW; int sM, sN, sT;                    // dW[m*sM + n*sN + tap*sT]
    int kind, taps, Mb, Nb;                       // 32-row / 32-column blocks
    int nimg, H, W;                               // base pixel grid (the R tensor's)
    unsigned mHW, mW;                             // magic multipliers for / (H*W) and / W
    long long npix; int pix_per_block;
    float* partial;                               // [workgroup][16 registers][64 lanes]: the workgroups' 32x32 tiles, summed by conv_wgrad_reduce_kernel;
                                                  // behind them [workgroup][32]: column sums of the gradient tensor (bias gradient)
    float* db; int nbias;                         // bias gradient (cout entries) or nullptr
};

constexpr int WG_NW = 16;                          // waves per workgroup of conv_wgrad_kernel
template <bool UP>                                 // UP: the ConvTranspose form (a.kind == UPCONV); else CONV3 / CONV1
__global__ __launch_bounds__(WG_NW * 64) void conv_wgrad_kernel(WgradArgs a) {
    __shared__ float red[WG_NW][16][64];             // [wave][register][lane]: conflict-free both ways, 64 KiB
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 31, hi = lane >> 5;
    int b = blockIdx.x;
    const int nb = b % a.Nb; b /= a.Nb;
    const int mb = b % a.Mb; b /= a.Mb;
    const int tap = b % a.taps; b /= a.taps;
    const long long p0 = (long long)b * a.pix_per_block;
    long long p1 = p0 + a.pix_per_block;
    if (p1 > a.npix) p1 = a.npix;
    const int n0 = nb * 32;
    const float* Cc = n0 < a.nC0 ? a.C0p : a.C1p;
    const int csC = n0 < a.nC0 ? a.csC0 : a.csC1;
    const int cn = (n0 < a.nC0 ? n0 : n0 - a.nC0) + i;
    const int HW = a.H * a.W;
    const int ky = !UP && a.kind == CONV3 ? tap / 3 - 1 : 0, kx = !UP && a.kind == CONV3 ? tap % 3 - 1 : 0;

    // fp32 MFMA shares the VALU, so the loop keeps per-load vector work at zero: W is even, hence a pixel pair
    // (p even, p+1) never straddles a row and the pair's (image, row, column) are wave-uniform SALU values; the
    // per-lane part of every address (odd pixel of the pair for the upper lane half, channel) is loop-invariant.
    // The SCALAR work matters just as much: a CU has one scalar unit for its sixteen waves, and the first version of this loop
    // (two magic divisions and 64-bit index arithmetic per pixel pair, ~80 SALU instructions) made these launches 21-39 us for
    // ~4 us of loads and MFMAs.  Now: one division per step of four pairs, the pairs after the first by increment, 32-bit
    // element offsets from the tensor bases (launch_wgrad bounds the tensors), all eight loads of a step issued before the
    // first use.
    const unsigned laneR = (unsigned)(hi * a.csR + a.coR + mb * 32 + i);
    const unsigned laneC = (unsigned)((UP ? 2 * hi : hi) * csC + cn);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float bsum = 0.f;
    // this wave's share: pixels p0 + 8*wave + 8*WG_NW*k + {0..7}; lane half hi takes the odd pixel of each pair
    for (long long base = p0 + 8 * wave; base < p1; base += 8 * WG_NW) {
        int img = div_magic((int)base, a.mHW), rem = (int)base - img * HW;
        int py = div_magic(rem, a.mW), px = rem - py * a.W;
        unsigned oR[4], oC[4];
        bool okR[4], okC[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            okR[s] = base + 2 * s < p1;                           // npix and the block ranges are even
            oR[s] = (unsigned)((int)base + 2 * s) * (unsigned)a.csR + laneR;
            if constexpr (UP) {
                const unsigned q = (unsigned)((img * 2 * a.H + 2 * py + (tap >> 1)) * (2 * a.W) + 2 * px + (tap & 1));
                oC[s] = q * (unsigned)csC + laneC; okC[s] = okR[s];
            } else {
                const int qy = py + ky, qx = px + kx;             // column of the even pixel's tap
                const bool row_in = qy >= 0 && qy < a.H;
                const bool lo_ok = qx >= 0, hi_ok = qx + 1 < a.W;           // uniform; qx+1 >= 0 and qx < W always
                okC[s] = okR[s] && row_in && (hi ? hi_ok : lo_ok);
                oC[s] = (unsigned)(img * HW + qy * a.W + qx) * (unsigned)csC + laneC;
            }
            if (!okR[s]) oR[s] = oR[0];                           // (clamped: the value is zeroed below)
            if (!okC[s]) oC[s] = laneC;
            px += 2;
            if (px >= a.W) { px = 0; if (++py >= a.H) { py = 0; ++img; } }
        }
        float av[4], bv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) { av[s] = a.R[oR[s]]; bv[s] = Cc[oC[s]]; }
#pragma unroll
        for (int s = 0; s < 4; ++s) { av[s] = okR[s] ? av[s] : 0.f; bv[s] = okC[s] ? bv[s] : 0.f; }
#pragma unroll
        for (int s = 0; s < 4; ++s) bsum += UP ? bv[s] : av[s];   // the gradient tensor's channel of this lane (bias gradient)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma32(av[s], bv[s], acc);
    }
    // D: lane (n = lane&31, hi), reg r <-> row m = drow(r, hi), column n.  Every wave parks its tile; wave w then sums register w
    // of all sixteen tiles (sixteen LDS reads per wave, side by side -- one wave summing fifteen tiles took longer than the loop).
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
    static_assert(WG_NW == 16, "one wave per accumulator register");
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < WG_NW; ++w) v += red[w][wave][lane];
    a.partial[((size_t)blockIdx.x * 16 + wave) * 64 + lane] = v;
    // bias gradient = column sums of the gradient tensor (dPre, or dU for the ConvTranspose form): the blocks that see every
    // channel exactly once per pixel range hand over their sums (UP: column block nb of every tap, first row block; else: row
    // block mb, first column block and tap)
    if (a.db && (UP ? mb == 0 : (nb == 0 && tap == 0))) {
        bsum += __shfl_xor(bsum, 32);
        __syncthreads();                                         // the tiles in `red` have been read
        if (hi == 0) red[wave][0][i] = bsum;
        __syncthreads();
        if (wave == 0 && hi == 0) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WG_NW; ++w) t += red[w][0][i];
            a.partial[(size_t)gridDim.x * 1024 + (size_t)blockIdx.x * 32 + i] = t;
        }
    }
}

// dW[m][n][tap] += sum over the pixel ranges of the workgroups' tiles.  One workgroup per 64 tile elements: four quarter sums
// per element (every thread a quarter of the ranges, eight loads in flight), folded through LDS; every dW element has exactly
// one writer.  (Atomics instead -- 256...768 workgroups adding onto the same 1024 addresses per block -- made these launches
// 27-39 us for 4-5 us of loads and MFMAs: float atomics are fabric operations.)
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(WgradArgs a, int blocks_wn, int ksplit) {
    __shared__ float part[4][64];
    if ((int)blockIdx.x >= blocks_wn * 16) {                     // the workgroups behind the tiles: bias gradient, 32 channels each
        const int cb = (int)blockIdx.x - blocks_wn * 16, i = threadIdx.x & 31, q8 = threadIdx.x >> 5;   // 8 partial sums per channel
        const bool up = a.kind == UPCONV;
        const float* bsrc = a.partial + (size_t)blocks_wn * ksplit * 1024;
        // contributing blocks: UP: (tap 0..3, mb = 0, nb = cb); else: (tap 0, mb = cb, nb = 0); index ((ks*taps + tap)*Mb + mb)*Nb + nb
        const int ntap = up ? a.taps : 1;
        float t = 0.f;
        for (int j = q8; j < ksplit * ntap; j += 8) {
            const int ks = j / ntap, tap = j - ks * ntap;
            const int blk = up ? ((ks * a.taps + tap) * a.Mb) * a.Nb + cb : ((ks * a.taps) * a.Mb + cb) * a.Nb;
            t += bsrc[(size_t)blk * 32 + i];
        }
        part[q8 >> 1][(q8 & 1) * 32 + i] = t;
        __syncthreads();
        if (threadIdx.x < 32) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) v += part[k >> 1][(k & 1) * 32 + i];
            a.db[cb * 32 + i] += v;
        }
        return;
    }
    const int blk = blockIdx.x >> 4, e = ((blockIdx.x & 15) << 6) + (threadIdx.x & 63), q = threadIdx.x >> 6;
    const float* src = a.partial + (size_t)blk * 1024 + e;
    const size_t stride = (size_t)blocks_wn * 1024;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int ks = q;
    for (; ks + 12 < ksplit; ks += 16) {
        s0 += src[(size_t)ks * stride]; s1 += src[(size_t)(ks + 4) * stride];
        s2 += src[(size_t)(ks + 8) * stride]; s3 += src[(size_t)(ks + 12) * stride];
    }
    for (; ks < ksplit; ks += 4) s0 += src[(size_t)ks * stride];
    part[q][threadIdx.x & 63] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (q == 0) {
        const float v = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        int b = blk;
        const int nb = b % a.Nb; b /= a.Nb;
        const int mb = b % a.Mb; b /= a.Mb;
        const int tap = b;
        const int r = e >> 6, lane = e & 63, i = lane & 31, hi = lane >> 5;
        const int m = mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi, n = nb * 32 + i;
        a.dW[(size_t)m * a.sM + (size_t)n * a.sN + (size_t)tap * a.sT] += v;
    }
}

static int launch_wgrad(WgradArgs a, hipStream_t s) {
    a.npix = (long long)a.nimg * a.H * a.W;
    a.mHW = (unsigned)((0x100000000ULL + (unsigned)(a.H * a.W) - 1) / (unsigned)(a.H * a.W));
    a.mW = (unsigned)((0x100000000ULL + (unsigned)a.W - 1) / (unsigned)a.W);
    // conv_wgrad_kernel addresses its tensors with 32-bit element offsets
    const long long cpix = a.npix * (a.kind == UPCONV ? 4 : 1);
    if (a.npix >= (1ll << 31) || a.npix * a.csR >= (1ll << 31) || cpix * (a.csC0 > a.csC1 ? a.csC0 : a.csC1) >= (1ll << 31)) return -7;
    const int blocks_wn = a.taps * a.Mb * a.Nb;
    int ksplit = 256 / blocks_wn;      // few workgroups per gradient element: every atomic is a fabric operation
    if (ksplit < 1) ksplit = 1;
    long long ppb = (a.npix + ksplit - 1) / ksplit;
    ppb = (ppb + 31) / 32 * 32;
    if (ppb < 32) ppb = 32;
    a.pix_per_block = (int)ppb;
    ksplit = (int)((a.npix + ppb - 1) / ppb);
    if (a.kind == UPCONV) GIGA_LAUNCH(conv_wgrad_kernel<true>, dim3(blocks_wn * ksplit), dim3(WG_NW * 64), 0, s, a);
    else GIGA_LAUNCH(conv_wgrad_kernel<false>, dim3(blocks_wn * ksplit), dim3(WG_NW * 64), 0, s, a);
    GIGA_LAUNCH(conv_wgrad_reduce_kernel, dim3(blocks_wn * 16 + (a.db ? a.nbias / 32 : 0)), dim3(256), 0, s, a, blocks_wn, ksplit);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

// (the 3x3 layers: giga_wgrad3.h)

// ------------------------------- conv_in backward ----------------------------------------------------------
// Same decomposition as convin_project_kernel: workgroup = (x-part, iy-group x channel half, scene), the haloed TSDF
// sub-volume is staged in LDS once, every wave owns SXW slices and runs without workgroup barriers; units of 16 voxels x
// 16 channels.  Per unit: recompute pre = conv_in(x) + b (7 MFMAs), dF = (pre > 0) * (gxz + gxy + gyz) / 40, then
// dW^T[tap][ch] += X^T[tap][voxel] * dF[voxel][ch] as 2 tap halves x 4 k-steps = 8 more MFMAs (the D registers of the
// forward unit ARE the B operand of these).  The yz-plane gradient of a lane's 100 voxels does not depend on the slice and
// lives in registers; the xz / xy rows of a slice are loaded into registers at the top of the slice.  Every workgroup
// leaves one partial (27x16 weights + 16 biases, fixed-order sum of its 8 waves through LDS); convin_bwd_reduce_kernel adds
// the workgroups up (no same-address atomics: those are resolved outside the XCD-local L2, one fabric operation each).
constexpr int CB_RS = 44, CB_ROWS = 12;           // staged sub-volume: (XW+2) x 12 rows x 44 floats (iz + 1 in [0, 41])
constexpr int CB_PART = 27 * 16 + 16;             // floats per workgroup partial: dW^T[tap][ch16], db[ch16]
constexpr size_t cb_lds_bytes(int sxw) { return (size_t)(8 * sxw + 2) * CB_ROWS * CB_RS * sizeof(float); }

// MASK: the forward (convin_project_kernel<.., MASK = true>, GIGA_CONVIN_MASK) has left one bit per pre-activation z, set when !(z > 0) -- per
// (scene, workgroup row, ix) and lane one 16-byte word, value k = (zg * 5 + ip) * 4 + r in word k >> 5 at bit (n - 1 - (k & 31)),
// n = 32 (4 in the last word) -- and the seven recomputation MFMAs of every unit fall away (8 instead of 15 per unit).
template <int SXW, bool MASK = false>
__global__ __launch_bounds__(512) void convin_bwd_kernel(const float* __restrict__ tsdf, const float* __restrict__ wpk,
                                                         const float* __restrict__ bias,
                                                         const float* __restrict__ gplanes,   // [3][B][40][40][32]
                                                         float* __restrict__ partial,         // [workgroup][CB_PART]
                                                         int B, const uint4* __restrict__ relu_mask = nullptr) {
    constexpr int XW = 8 * SXW;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 15, g = lane >> 4;
    const int xp = blockIdx.x, grp = blockIdx.y >> 1, chh = blockIdx.y & 1, b = blockIdx.z;
    const int x0 = xp * XW;
    const float* vol = tsdf + (size_t)b * RES * RES * RES;
    for (int v = tid; v < (XW + 2) * CB_ROWS * 10; v += 512) {
        const int q = v % 10, row = v / 10, yl = row % CB_ROWS, xl = row / CB_ROWS;
        const int ix = x0 - 1 + xl, iy = 10 * grp - 1 + yl;
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ix >= 0 && ix < RES && iy >= 0 && iy < RES)
            val = *reinterpret_cast<const float4*>(vol + ((size_t)ix * RES + iy) * RES + 4 * q);
        float* dst = lds + row * CB_RS + 1 + 4 * q;
        dst[0] = val.x; dst[1] = val.y; dst[2] = val.z; dst[3] = val.w;
        if (q == 0) dst[-1] = 0.f;
        if (q == 9) dst[4] = 0.f;
    }
    float wreg[7];
#pragma unroll
    for (int s = 0; s < 7; ++s) wreg[s] = wpk[(chh * 7 + s) * 64 + lane];
    const int ch = 16 * chh + j;
    const float bn = bias[ch];
    const size_t img_stride = (size_t)RES * RES * CD;
    const float* gxz = gplanes + ((size_t)0 * B + b) * img_stride;
    const float* gxy = gplanes + ((size_t)1 * B + b) * img_stride;
    const float* gyz = gplanes + ((size_t)2 * B + b) * img_stride;
    const float inv = 1.0f / RES;
    // forward A operand: row i = lane&15 is voxel (iy_l = i>>3, iz_l = 4*((i>>2)&1) + (i&3)); k-slot g -> tap 4s+g
    int abase[7];
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        int t = 4 * s + g;
        t = t > 26 ? 26 : t;
        abase[s] = ((t / 9) * CB_ROWS + (j >> 3) + (t / 3) % 3) * CB_RS + 4 * ((j >> 2) & 1) + (j & 3) + t % 3;
    }
    // backward A operand: row = tap (lane&15 + 16*th), k-slot g -> voxel row 4g + r of the unit (iy_l = g>>1, iz_l = 4(g&1)+r)
    int tbase[2];
#pragma unroll
    for (int th = 0; th < 2; ++th) {
        int t = j + 16 * th;
        t = t > 26 ? 26 : t;                      // rows >= 27 of dW^T are never written back
        tbase[th] = ((t / 9) * CB_ROWS + (g >> 1) + (t / 3) % 3) * CB_RS + 4 * (g & 1) + t % 3;
    }
    // the yz-plane gradient of this lane's 100 voxels does not depend on the slice: registers, loaded once
    f32x4v gz[5][5];
#pragma unroll
    for (int ip = 0; ip < 5; ++ip)
#pragma unroll
        for (int zg = 0; zg < 5; ++zg)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                gz[ip][zg][r] = gyz[((8 * zg + 4 * (g & 1) + r) * RES + grp * 10 + 2 * ip + (g >> 1)) * CD + ch];
    f32x4v accw[2] = {f32x4v{0.f, 0.f, 0.f, 0.f}, f32x4v{0.f, 0.f, 0.f, 0.f}};
    float accb = 0.f;
    const f32x4v bias4 = {bn, bn, bn, bn};
    __syncthreads();

    for (int sx = 0; sx < SXW; ++sx) {
        const int ixl = wave * SXW + sx, ix = x0 + ixl;
        const int so = ixl * CB_ROWS * CB_RS;
        // upstream gradients of this slice that do not depend on the unit: xy row per iy-pair, xz rows per (zg, r)
        float gy[5];
        f32x4v gx[5];
        unsigned mwv[4] = {0u, 0u, 0u, 0u};
        if constexpr (MASK) {
            const uint4 m4 = relu_mask[(((size_t)b * 8 + blockIdx.y) * RES + ix) * 64 + lane];
            mwv[0] = m4.x; mwv[1] = m4.y; mwv[2] = m4.z; mwv[3] = m4.w;
        }
#pragma unroll
        for (int ip = 0; ip < 5; ++ip) gy[ip] = gxy[((grp * 10 + 2 * ip + (g >> 1)) * RES + ix) * CD + ch];
#pragma unroll
        for (int zg = 0; zg < 5; ++zg)
#pragma unroll
            for (int r = 0; r < 4; ++r) gx[zg][r] = gxz[((8 * zg + 4 * (g & 1) + r) * RES + ix) * CD + ch];
#pragma unroll
        for (int zg = 0; zg < 5; ++zg) {
            // forward recompute: five independent 7-MFMA chains (bias in the C operand, as the forward does) -- or the stored mask bits
            f32x4v d[5];
            if constexpr (!MASK) {
#pragma unroll
                for (int ip = 0; ip < 5; ++ip) d[ip] = bias4;
#pragma unroll
                for (int s = 0; s < 7; ++s)
#pragma unroll
                    for (int ip = 0; ip < 5; ++ip)
                        d[ip] = mfma32_16(lds[abase[s] + so + 2 * ip * CB_RS + 8 * zg], wreg[s], d[ip]);
            }
#pragma unroll
            for (int ip = 0; ip < 5; ++ip) {
                const int uo = so + 2 * ip * CB_RS + 8 * zg;
                f32x4v dF;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float gsum = gx[zg][r] + gy[ip] + gz[ip][zg][r];
                    bool pos;
                    if constexpr (MASK) {
                        const int k = (zg * 5 + ip) * 4 + r, wd = k >> 5, bit = (wd == 3 ? 3 : 31) - (k & 31);
                        pos = ((mwv[wd] >> bit) & 1u) == 0u;                 // bit clear: z > 0
                    } else {
                        pos = d[ip][r] > 0.f;
                    }
                    dF[r] = pos ? gsum * inv : 0.f;
                    accb += dF[r];
                }
#pragma unroll
                for (int th = 0; th < 2; ++th)
#pragma unroll
                    for (int r = 0; r < 4; ++r) accw[th] = mfma32_16(lds[tbase[th] + uo + r], dF[r], accw[th]);
            }
        }
    }
    // ---- workgroup partial: fixed-order sum of the 8 waves.  accw[th][r]: dW^T[tap = 16th + 4g + r][ch] ----------------
    accb += __shfl_xor(accb, 16);
    accb += __shfl_xor(accb, 32);
    __syncthreads();                                  // every wave is done with the sub-volume
    float* red = lds;                                 // [wave][CB_PART]
#pragma unroll
    for (int th = 0; th < 2; ++th)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tap = 16 * th + 4 * g + r;
            if (tap < 27) red[wave * CB_PART + tap * 16 + j] = accw[th][r];
        }
    if (g == 0) red[wave * CB_PART + 27 * 16 + j] = accb;
    __syncthreads();
    if (tid < CB_PART) {
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) sum += red[w * CB_PART + tid];
        const int wgi = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[(size_t)wgi * CB_PART + tid] = sum;
    }
}

// dW[ch][tap] / db[ch] = sum over the scene's workgroups of one (channel half): partial[scene][grp*2+chh][xp][CB_PART]
__global__ __launch_bounds__(256) void convin_bwd_reduce_kernel(const float* __restrict__ partial, int B, int nxp,
                                                                float* __restrict__ dW, float* __restrict__ db) {
    __shared__ float sm[256];
    const int e = blockIdx.x, chh = blockIdx.y;       // e: element of the partial (tap*16 + j, or 432 + j)
    float s = 0.f;
    const int per_scene = 8 * nxp;                    // workgroups per scene, (grp*2+chh) major, x-part minor
    for (int i = threadIdx.x; i < B * 4 * nxp; i += 256) {
        const int bq = i / (4 * nxp), rest = i % (4 * nxp), grp = rest / nxp, xp = rest % nxp;
        s += partial[((size_t)bq * per_scene + (grp * 2 + chh) * nxp + xp) * CB_PART + e];
    }
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) sm[threadIdx.x] += sm[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int jj = e & 15, ch = 16 * chh + jj;
        if (e < 27 * 16) dW[ch * 27 + (e >> 4)] += sm[0];
        else db[ch] += sm[0];
    }
}

// ------------------------------- the library's side stream (giga_side.h) -------------------------------------------
static std::mutex g_side_mutex[64];               // one per device: callers on different devices do not wait for each other
static SideStream g_side[64];
SideScope::SideScope(hipStream_t main, bool enable) : main_(main) {
    if (!enable) return;
    // the device that OWNS the caller's stream (the null stream belongs to the current device); a caller whose current device is
    // another one gets the inactive scope: recording this device's events on a foreign stream would fail halfway through the pass
    int dev = 0, sdev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return;
    if (main && (hipStreamGetDevice(main, &sdev) != hipSuccess || sdev != dev)) return;
    g_side_mutex[dev].lock();
    SideStream* w = &g_side[dev];
    if (!w->ok) {
        bool ok = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) == hipSuccess;
        for (int i = 0; i < 16 && ok; ++i) ok = hipEventCreateWithFlags(&w->fork[i], hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < 4 && ok; ++i) ok = hipEventCreateWithFlags(&w->join[i], hipEventDisableTiming) == hipSuccess;
        w->ok = ok;
    }
    if (w->ok) { side_ = w; dev_ = dev; }
    else g_side_mutex[dev].unlock();
}
SideScope::~SideScope() {
    if (!side_) return;
    if (nfork_ > 0 && njoin_ == 0) (void)join();      // an error path left the side stream forked (inside a capture: unjoined): join it anyway
    g_side_mutex[dev_].unlock();
}
int SideScope::fork() {
    if (!side_) return 0;
    hipEvent_t e = side_->fork[nfork_++ & 15];
    return (hipEventRecord(e, main_) == hipSuccess && hipStreamWaitEvent(side_->stream, e, 0) == hipSuccess) ? 0 : -10;
}
int SideScope::join() {
    if (!side_) return 0;
    hipEvent_t e = side_->join[njoin_++ & 3];
    return (hipEventRecord(e, side_->stream) == hipSuccess && hipStreamWaitEvent(main_, e, 0) == hipSuccess) ? 0 : -10;
}
void side_streams_forget() {
    for (int d = 0; d < 64; ++d) {
        std::lock_guard<std::mutex> lk(g_side_mutex[d]);
        g_side[d] = SideStream{};
    }
}

// ------------------------------- driver -----------------------------------------------------------------------
// forward activations: the encoder workspace (giga_enc_plan.h::EncWs, fp32).  Gradient workspace carve:
// (struct BwdWs: giga_args.h)
// what the last backward of this process ran its data-gradient chain on (giga_backward_last_path: tests pin the launch form to it)
static std::atomic<int> g_last_bwd_path{0};

BwdWs enc_bwd_workspace(int B) {
    const size_t n = 3 * (size_t)B;
    BwdWs w{};
    size_t at = 0;
    auto take = [&](size_t elems) { size_t o = at; at += align_up(elems * 4, 256); return o; };
    auto gin = [&](int l) { return take(n * conv_in_elems(l)); };           // gradient of layer l's (concatenated) input / of its output
    auto gout = [&](int l) { return take(n * conv_out_elems(l)); };
    w.gA6 = gin(12); w.gA5 = gin(11); w.gC1 = gin(10);
    w.gA4 = gin(9);  w.gA3 = gin(8);  w.gC0 = gin(7);
    w.gS2 = gin(6);  w.gA2 = gin(5);  w.gQ1 = gin(4);
    w.gS1 = gout(3); w.gA1 = gin(3);  w.gQ0 = gin(2);
    w.gS0 = gout(1); w.gA0 = gin(1);  w.gP0 = gin(0);
    w.WG = take((size_t)WG3_MAX_PARTS * 32 * 288 + WG3_BIAS_FLOATS);      // per-workgroup weight-gradient partials (conv_wgrad_kernel; giga_wgrad3.h with one reduce per layer)
    // one region per 3x3 layer for the single reduce launch at the end (wgrad3_reduce_all_kernel): 256 x min(blocks, 8) partial
    // images of 36 KiB + the bias partials; 368 MB in all, whatever the batch size
    for (int l = 0; l < 12; ++l) {
        w.WG3[l] = 0;
        if (kConv[l].kind != CONV3) continue;
        const int nblk = (kConv[l].cout / 32) * ((kConv[l].cin0 + kConv[l].cin1) / 32);
        w.WG3[l] = take((size_t)256 * (nblk < 8 ? nblk : 8) * 32 * 288 + WG3_BIAS_FLOATS);
    }
    w.CINP = take((size_t)B * 8 * 5 * CB_PART);    // conv_in's workgroup partials (their own: the backward runs beside the weight gradients' stream)
    w.total = at;
    return w;
}

// MATH: arithmetic of the thirteen data-gradient convolutions (MATH_NATIVE fp32 MFMA, or MATH_BF16: bf16 operands from the
// backward blob's bf16 images, fp32 accumulate and fp32 gradients in memory); everything else is fp32.
template <int V> using IC = std::integral_constant<int, V>;
// The two numbers of a layer's backward that are not its shape (giga_layout.h::kConv[l]): NB of its data gradient (16-channel output
// blocks per unit, giga_conv16.h) and the rows per strip of its 3x3 weight gradient (giga_wgrad3.h; 0: not a 3x3 layer)
struct BwdTune { int nb, rows; };
constexpr BwdTune kBwdTune[NCONV] = {{2, 4}, {2, 4}, {2, 4}, {1, 4}, {1, 2}, {1, 2}, {1, 0}, {1, 2}, {1, 4}, {2, 0}, {2, 2}, {2, 4}, {2, 0}};
template <int MATH>
static int encoder_backward_impl(const float* tsdf, const uint8_t* blob, const uint8_t* bwd_blob, const uint8_t* fws,
                                 float* gplanes /* [3B][40][40][32], in: dLoss/dPlanes (read only: L12's input and its weight gradient's dY) */, uint8_t* gws,
                                 float* grads /* flat, state-dict order */, int head_present, int B, hipStream_t s, bool convin_mask,
                                 SideScope& side) {
    if (B <= 0) return 0;
    const PackOff ko = pack_offsets();
    const BwdPackOff bo = bwd_pack_offsets();
    const ParamOff po = param_offsets(head_present);
    const EncWs f = enc_workspace(B, 0);
    const BwdWs g = enc_bwd_workspace(B);
    const int nimg = 3 * B;
    auto F = [&](size_t off) { return reinterpret_cast<const float*>(fws + off); };
    auto G = [&](size_t off) { return reinterpret_cast<float*>(gws + off); };
    int rc = 0;
    // the ten reduces of the 3x3 layers' partial weight gradients as ONE launch behind the last of them (GIGA_WGRAD_ONE_REDUCE=0: one
    // launch per layer, right behind its weight-gradient kernel, as before round 5)
    const bool one_reduce = [] { const char* e = getenv("GIGA_WGRAD_ONE_REDUCE"); return !e || atoi(e) != 0; }();     // (per call)
    Wg3RedArgs RED{};
    // the weight gradients on the device's side stream (`side`: giga_side.h; inactive = on the caller's stream, between the data gradients)
    const hipStream_t ws = side.stream();
    auto fork = [&]() { rc |= side.fork(); };
    // weight gradient of layer l: R = dPre (channels = cout), columns = layer input (in0 [, in1])
    auto wgrad3_now = [&](auto lc, const float* dpre, const float* in0, const float* in1) {
        constexpr int l = decltype(lc)::value;
        constexpr ConvLayerDesc d = kConv[l];
        if constexpr (d.kind == CONV3) {
            Wgrad3Args w3{dpre, in0, in1, grads + po.conv_w[l], grads + po.conv_b[l], one_reduce ? G(g.WG3[l]) : G(g.WG), nimg};
            Wg3RedArgs* defer = one_reduce ? &RED : nullptr;
            rc |= MATH == MATH_BF16 ? launch_wgrad3_bf16<d.cin0, d.cin1, d.cout, d.H, kBwdTune[l].rows>(w3, ws, defer)
                                    : launch_wgrad3<d.cin0, d.cin1, d.cout, d.H, kBwdTune[l].rows>(w3, ws, defer);
        } else {                                                    // CONV1 (the 1x1 layer at the end)
            const int cin = d.cin0 + d.cin1;
            WgradArgs a{};
            a.R = dpre; a.csR = d.cout; a.coR = 0;
            a.C0p = in0; a.C1p = in1; a.csC0 = d.cin0; a.csC1 = d.cin1; a.nC0 = d.cin0;
            a.dW = grads + po.conv_w[l]; a.sM = cin; a.sN = 1; a.sT = 1;
            a.kind = d.kind; a.taps = 1; a.Mb = d.cout / 32; a.Nb = cin / 32;
            a.nimg = nimg; a.H = d.H; a.W = d.W;
            a.partial = G(g.WG);
            a.db = grads + po.conv_b[l]; a.nbias = d.cout;          // bias gradient = column sums of dPre, folded into the same two launches
            rc |= launch_wgrad(a, ws);
        }
    };
    // ConvTranspose2d(cin, cout, 2, 2): dW[ci][co][d] = sum In[p][ci] * dU[up(p,d)][co]; dU = channels [0,cout) of dcat
    auto wgrad_up_now = [&](int l, const float* in, const float* dcat, int cs_cat) {
        const ConvLayerDesc& d = kConv[l];
        WgradArgs a{};
        a.R = in; a.csR = d.cin0; a.coR = 0;
        a.C0p = dcat; a.C1p = dcat; a.csC0 = cs_cat; a.csC1 = cs_cat; a.nC0 = d.cout;
        a.dW = grads + po.conv_w[l]; a.sM = d.cout * 4; a.sN = 4; a.sT = 1;
        a.kind = UPCONV; a.taps = 4; a.Mb = d.cin0 / 32; a.Nb = d.cout / 32;
        a.nimg = nimg; a.H = d.H; a.W = d.W;
        a.partial = G(g.WG);
        a.db = grads + po.conv_b[l]; a.nbias = d.cout;          // bias gradient = column sums of dU over all four taps
        rc |= launch_wgrad(a, ws);
    };
    // Forks are not free (an event record drains the caller's queue between two data gradients, the wait costs the side queue a few
    // microseconds): GIGA_WGRAD_FORK_EVERY = n enqueues the weight gradients in groups of n behind ONE fork (default 1).
    const int fork_every = [] { const char* e = getenv("GIGA_WGRAD_FORK_EVERY"); const int v = e ? atoi(e) : 1; return v < 1 ? 1 : v; }();
    std::function<void()> pending[16];
    int npending = 0;
    auto flush = [&]() {
        if (npending == 0) return;
        fork();
        for (int i = 0; i < npending; ++i) pending[i]();
        npending = 0;
    };
    auto defer = [&](std::function<void()> f) {
        pending[npending++] = std::move(f);
        if (npending >= fork_every) flush();
    };
    auto wgrad3 = [&](auto lc, const float* dpre, const float* in0, const float* in1) {
        defer([=, &wgrad3_now]() { wgrad3_now(lc, dpre, in0, in1); });
    };
    auto wgrad_up = [&](int l, const float* in, const float* dcat, int cs_cat) {
        defer([=, &wgrad_up_now]() { wgrad_up_now(l, in, dcat, cs_cat); });
    };
    // data gradient of layer l; relu_of: the forward activation the gradient flows into next (ReLU output of the layer
    // below): its backward mask is applied in the convolution's epilogue instead of by a separate pass over the tensor
    auto dgrad_args = [&](int l, const float* in, int cs, void* out, const float* relu_of = nullptr) {
        ConvArgs a{};
        a.in0 = in; a.in1 = nullptr; a.w = bwd_blob + (MATH == MATH_BF16 ? bo.convbf[l] : bo.conv[l]); a.bias = nullptr; a.out = out; a.nimg = nimg;
        a.cs0 = cs;
        a.mask = relu_of;
        a.xcd_local = 1;                 // images onto XCDs, all weight groups of an image on one L2 (giga_conv16.h: conv_wg_map)
        return a;
    };
    const size_t n40 = (size_t)nimg * 1600, n20 = (size_t)nimg * 400, n10 = (size_t)nimg * 100;

    // ---- the data-gradient chain.  Stage order L12 L11 L10 L9 L8 L7 L6 L5 L4 [pool1] L3 L2 [pool0] L1 L0: one launch per stage.
    // (The chain as ONE persistent launch measured slower at 8, 32 and 128 scenes in every training mode: back-to-back launches already
    // overlap their dispatch with the predecessor's tail, fifteen group barriers are not free, and the weight gradients, pushed behind
    // the whole chain, find their dY further down the cache hierarchy.  profiles/r05/dgrad_mega.txt)
    const ConvArgs stage[13] = {
        dgrad_args(12, gplanes, 0, G(g.gA6), F(f.A6)),         // L12 conv_final (1x1, no activation): gplanes = dOUT
        dgrad_args(11, G(g.gA6), 0, G(g.gA5), F(f.A5)),        // L11 up1.conv2: A5 -> A6
        dgrad_args(10, G(g.gA5), 0, G(g.gC1)),                 // L10 up1.conv1: cat(U1, S0) -> A5; 64 channels out (dU1 | dS0 skip part)
        dgrad_args(9, G(g.gC1), 64, G(g.gA4), F(f.A4)),        // L9 up1.upconv: A4 (20x20x64) -> U1; dU1 = gC1[..., 0:32]
        dgrad_args(8, G(g.gA4), 0, G(g.gA3), F(f.A3)),         // L8 up0.conv2: A3 -> A4
        dgrad_args(7, G(g.gA3), 0, G(g.gC0)),                  // L7 up0.conv1: cat(U0, S1) -> A3; 128 channels out
        dgrad_args(6, G(g.gC0), 128, G(g.gS2), F(f.S2)),       // L6 up0.upconv: S2 (10x10x128) -> U0; dU0 = gC0[..., 0:64]
        dgrad_args(5, G(g.gS2), 0, G(g.gA2), F(f.A2)),         // L5 down2.conv2: A2 -> S2
        dgrad_args(4, G(g.gA2), 0, G(g.gQ1)),                  // L4 down2.conv1: Q1 -> A2
        dgrad_args(3, G(g.gS1), 0, G(g.gA1), F(f.A1)),         // L3 down1.conv2: A1 -> S1
        dgrad_args(2, G(g.gA1), 0, G(g.gQ0)),                  // L2 down1.conv1: Q0 -> A1
        dgrad_args(1, G(g.gS0), 0, G(g.gA0), F(f.A0)),         // L1 down0.conv2: A0 -> S0
        dgrad_args(0, G(g.gA0), 0, G(g.gP0))};                 // L0 down0.conv1: P0 -> A0
    // fp32 step: the data gradients of the 3x3 layers are stride-1 3x3 convolutions too (flipped taps, channels swapped) and run as
    // Winograd F(2x2, 3x3) on the images giga_derive_winograd leaves behind the backward blob's other regions (giga_wino.h; the ReLU
    // mask of the layer below in the epilogue as before).  GIGA_WINOGRAD_BWD=0: the direct conv16 kernels.
    static const int env_wino_bwd = [] { const char* e = getenv("GIGA_WINOGRAD_BWD"); return e ? atoi(e) : 1; }();
    constexpr bool CAN_WINO_BWD = MATH == MATH_NATIVE;
    const bool wino_bwd = CAN_WINO_BWD && env_wino_bwd != 0;
    // the data gradient of layer L is stage 12 - L of the chain: a convolution of the layer's kind (ConvTranspose: DOWN) with the channels swapped
    auto dgrad = [&](auto lc) {
        constexpr int L = decltype(lc)::value, KIND = kConv[L].kind, C0 = kConv[L].cout, COUT = kConv[L].cin0 + kConv[L].cin1;
        constexpr int H = kConv[L].H, W = kConv[L].W, NB = kBwdTune[L].nb;
        const ConvArgs& st = stage[NCONV - 1 - L];
        if constexpr (CAN_WINO_BWD && KIND == CONV3) {
            if (wino_bwd) {
                ConvArgs a = st;
                a.w = bwd_blob + bo.wino[L];
                return launch_wino<C0, 0, COUT, H, W, false, false>(a, s);
            }
        }
        return launch_conv<float, KIND == UPCONV ? DOWN : KIND, C0, 0, COUT, H, W, NB, false, false, MATH>(st, s);
    };
    g_last_bwd_path.store((wino_bwd ? GIGA_BWD_PATH_WINOGRAD : 0) | (MATH == MATH_BF16 ? GIGA_BWD_PATH_BF16 : 0), std::memory_order_relaxed);
    // one launch per stage, the weight gradient of a layer right behind the launch that produced its dPre (it is still in the
    // Infinity Cache then)
    wgrad3(IC<12>{}, gplanes, F(f.A6), nullptr);
    rc |= dgrad(IC<12>{});
    wgrad3(IC<11>{}, G(g.gA6), F(f.A5), nullptr);
    rc |= dgrad(IC<11>{});
    wgrad3(IC<10>{}, G(g.gA5), F(f.U1), F(f.S0));
    rc |= dgrad(IC<10>{});
    wgrad_up(9, F(f.A4), G(g.gC1), 64);
    rc |= dgrad(IC<9>{});
    wgrad3(IC<8>{}, G(g.gA4), F(f.A3), nullptr);
    rc |= dgrad(IC<8>{});
    wgrad3(IC<7>{}, G(g.gA3), F(f.U0), F(f.S1));
    rc |= dgrad(IC<7>{});
    wgrad_up(6, F(f.S2), G(g.gC0), 128);
    rc |= dgrad(IC<6>{});
    wgrad3(IC<5>{}, G(g.gS2), F(f.A2), nullptr);
    rc |= dgrad(IC<5>{});
    wgrad3(IC<4>{}, G(g.gA2), F(f.Q1), nullptr);
    rc |= dgrad(IC<4>{});
    {
        const size_t tot = n20 * 64 / 4;
        GIGA_LAUNCH(pool_bwd_add_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, G(g.gS1),
                           G(g.gC0), 128, 64, G(g.gQ1), F(f.S1), F(f.Q1), nimg, 20, 20, 64);
    }
    wgrad3(IC<3>{}, G(g.gS1), F(f.A1), nullptr);
    rc |= dgrad(IC<3>{});
    wgrad3(IC<2>{}, G(g.gA1), F(f.Q0), nullptr);
    rc |= dgrad(IC<2>{});
    {
        const size_t tot = n40 * 32 / 4;
        GIGA_LAUNCH(pool_bwd_add_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, G(g.gS0),
                           G(g.gC1), 64, 32, G(g.gQ0), F(f.S0), F(f.Q0), nimg, 40, 40, 32);
    }
    wgrad3(IC<1>{}, G(g.gS0), F(f.A0), nullptr);
    rc |= dgrad(IC<1>{});
    wgrad3(IC<0>{}, G(g.gA0), F(f.P0), nullptr);
    rc |= dgrad(IC<0>{});
    flush();
    rc |= launch_wgrad3_reduce_all(RED, ws);
    // conv_in + projection
    {
        const int nxp = enc_nxp(B);
        const float* cw = reinterpret_cast<const float*>(blob + ko.convin_w);
        const float* cb = reinterpret_cast<const float*>(blob + ko.convin_b);
        float* part = G(g.CINP);
        const uint4* mask = convin_mask ? reinterpret_cast<const uint4*>(fws + f.MASK) : nullptr;
        auto go = [&](auto kern, int sxw, dim3 grid) {
            giga::dyn_lds_once(reinterpret_cast<const void*>(kern), (int)cb_lds_bytes(sxw));
            GIGA_LAUNCH(kern, grid, dim3(512), cb_lds_bytes(sxw), s, tsdf, cw, cb, G(g.gP0), part, B, mask);
        };
        if (nxp == 1) { if (mask) go(convin_bwd_kernel<5, true>, 5, dim3(1, 8, B)); else go(convin_bwd_kernel<5, false>, 5, dim3(1, 8, B)); }
        else          { if (mask) go(convin_bwd_kernel<1, true>, 1, dim3(5, 8, B)); else go(convin_bwd_kernel<1, false>, 1, dim3(5, 8, B)); }
        GIGA_LAUNCH(convin_bwd_reduce_kernel, dim3(CB_PART, 2), dim3(256), 0, s, part, B, nxp, grads + po.conv_in_w,
                           grads + po.conv_in_b);
    }
    rc |= side.join();                                // the caller's stream carries every gradient (the side stream's queue is far behind: its work ended with the reduce)
    if (hipGetLastError() != hipSuccess) rc |= -10;
    return rc;
}

int launch_encoder_backward(const float* tsdf, const uint8_t* blob, const uint8_t* bwd_blob, const uint8_t* fws, float* gplanes,
                            uint8_t* gws, float* grads, int head_present, int B, hipStream_t s, bool bf16_convs, bool convin_mask,
                            SideScope& side) {
    return bf16_convs ? encoder_backward_impl<MATH_BF16>(tsdf, blob, bwd_blob, fws, gplanes, gws, grads, head_present, B, s, convin_mask, side)
                      : encoder_backward_impl<MATH_NATIVE>(tsdf, blob, bwd_blob, fws, gplanes, gws, grads, head_present, B, s, convin_mask, side);
}

}  // namespace giga

extern "C" int giga_backward_last_path(void) { return giga::g_last_bwd_path.load(std::memory_order_relaxed); }

#ifdef GIGA_TRACE
extern "C" int giga_debug_wgrad3_trace(long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(giga::g_wg3_trace), sizeof(long long) * 8 * 32) == hipSuccess ? 0 : -10;
}
#endif
