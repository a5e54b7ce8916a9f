// Weight gradient of the 3x3 layers (training path; included by giga_encoder_bwd.hip): the LDS-staged fp32 kernel, the three bf16
// kernels, the reduce over their partial images and the two launchers.  Staging, tap shifts, epilogue, bias fold and strip
// geometry are written once here and shared by the kernels -- and, for the LDS byte counts, by the launchers.
#pragma once
#include "giga_dev.h"
#include "giga_launch.h"

namespace giga {

// ------------------------------- 3x3 weight gradient, LDS-staged -------------------------------------------------
// dW[co][ci][tap] += sum_p dY[p][co] * X[p + tap][ci] for one 3x3 layer.  Unit = (image, strip of RS rows): the
// workgroup stages the haloed input strip (all input channels, zero outside the image) and the dY strip (all
// output channels) in LDS ONCE; its 8 waves then take their operands from LDS (one ds_read_b32 per 64-cycle MFMA,
// immediate tap offsets, two VALU per pixel pair -- fp32 MFMA shares the VALU).  A wave owns one 32x32 (co, ci)
// block for ALL nine taps (nine 32x32 accumulators, the dY operand is read once per nine MFMAs) and one of KS
// interleaved shares of the strip's pixel pairs; blocks beyond 8 per workgroup go to blockIdx.y.  Accumulators
// live across the whole persistent strip loop; the next strip is prefetched into registers under the MFMAs.
// Epilogue: the waves of a block park their tiles in LDS slots, the sharers are summed and the result goes tap-major
// into this workgroup's partial image (wg3_slot_epilogue); wgrad3_reduce_all_kernel sums the workgroups.
struct Wgrad3Args {
    const float* dY;                 // [img][H][W][COUT]   gradient of the layer's pre-activation
    const float* in0; const float* in1;   // layer input (concat order), dense NHWC with C0 / C1 channels
    float* dW;                       // [COUT][CIN][3][3], accumulated by wgrad3_reduce_all_kernel
    float* db;                       // [COUT] bias gradient = column sums of dY, accumulated by wgrad3_reduce_all_kernel
    float* partial;                  // per-workgroup partial sums (workspace): [by][bx][block][9][32][32], then [bx][COUT]
    int nimg;
};
constexpr int WG3_MAX_PARTS = 256 * 8;       // (workgroup, block) partial images of 9x32x32 floats
constexpr int WG3_BIAS_FLOATS = 256 * 128;   // per-workgroup bias partials behind them
constexpr int WG3_RN = 9 * 1024;             // floats of one block's partial image: [tap][co][ci]
constexpr size_t WG3_SLOT_BYTES = (size_t)8 * 3 * 4 * 64 * 16;       // the epilogue's LDS slots (96 KiB): [wave][tap of the round][r4][lane] float4

#ifdef GIGA_TRACE
static __device__ long long g_wg3_trace[8 * 32];
#define WG3_T(idx) do { if (blockIdx.x == 0 && blockIdx.y == 0 && lane == 0 && (idx) < 32) \
        g_wg3_trace[wave * 32 + (idx)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define WG3_T(idx) do {} while (0)
#endif

// LDS carve-up of the fp32 kernel's strip: kernel and launcher read the same numbers
template <int CIN, int COUT, int H, int RS>
struct Wg3GeomF32 {
    static constexpr int W = H, XW = W + 2, XR = RS + 2;
    static constexpr int XS = CIN + (CIN % 64 == 0 ? 32 : 0);      // LDS pixel strides (floats): odd multiple of 32 so that
    static constexpr int YS = COUT + (COUT % 64 == 0 ? 32 : 0);    // the two pixels of a pair fall into different bank halves
    static constexpr int XFLOATS = XR * XW * XS;                   // the dY strip sits behind the X strip
    static constexpr size_t STRIP_BYTES = ((size_t)XFLOATS + (size_t)RS * W * YS) * 4;
    static constexpr size_t LDS_BYTES = STRIP_BYTES > WG3_SLOT_BYTES ? STRIP_BYTES : WG3_SLOT_BYTES;
    static_assert(H % RS == 0 && W % 2 == 0, "strip geometry");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// ---- epilogue of the kernels in which a wave owns a block for all nine taps: three rounds of three taps.  Every wave parks its
// three 32x32 tiles in its own LDS slot (register layout, 16-B vectors, conflict-free), then all 512 threads sum the KS slots of
// every block and store the result tap-major ([block][tap][co][ci], coalesced) into this workgroup's partial image `part`;
// wgrad3_reduce_all_kernel sums the workgroups and transposes to the parameter layout.  (Device-scope float atomics from 256
// workgroups onto one 36 KiB image, and LDS float atomics, each cost several times the MFMA loop.)
template <int BPG, int KS>
__device__ __forceinline__ void wg3_slot_epilogue(float* wg_lds, float* part, const f32x16 (&acc)[9], int tid, int wave, int lane) {
    float4* slot = reinterpret_cast<float4*>(wg_lds);                 // [wave][tap of the round][r4][lane]
#pragma unroll
    for (int g3 = 0; g3 < 3; ++g3) {
        __syncthreads();
#pragma unroll
        for (int tl = 0; tl < 3; ++tl)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4)
                slot[((wave * 3 + tl) * 4 + r4) * 64 + lane] =
                    make_float4(acc[3 * g3 + tl][4 * r4], acc[3 * g3 + tl][4 * r4 + 1], acc[3 * g3 + tl][4 * r4 + 2],
                                acc[3 * g3 + tl][4 * r4 + 3]);
        __syncthreads();
        for (int v = tid; v < BPG * 3 * 4 * 64; v += 512) {
            const int ln = v & 63, r4 = (v >> 6) & 3, tl = (v >> 8) % 3, b = v / 768;
            float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int q = 0; q < KS; ++q) {
                const float4 x = slot[(((b * KS + q) * 3 + tl) * 4 + r4) * 64 + ln];
                sum.x += x.x; sum.y += x.y; sum.z += x.z; sum.w += x.w;
            }
            const int n = ln & 31, m0 = 8 * r4 + 4 * (ln >> 5);       // D rows of registers 4*r4 .. 4*r4+3: m0 .. m0+3
            float* dst = part + ((size_t)(b * 9 + 3 * g3 + tl) * 32 + m0) * 32 + n;
            dst[0] = sum.x; dst[32] = sum.y; dst[64] = sum.z; dst[96] = sum.w;
        }
    }
}

template <int C0, int C1, int COUT, int H, int RS>
__global__ __launch_bounds__(512) void conv3_wgrad_kernel(Wgrad3Args a) {
    using GE = Wg3GeomF32<C0 + C1, COUT, H, RS>;
    constexpr int W = H, CIN = C0 + C1;
    constexpr int NBK = CIN / 32, NBLK = (COUT / 32) * NBK;
    constexpr int BPG = NBLK < 8 ? NBLK : 8;          // blocks per workgroup
    constexpr int KS = 8 / BPG;                       // waves sharing a block (K split)
    constexpr int XS = GE::XS, YS = GE::YS, XW = GE::XW, XR = GE::XR;
    constexpr int NVX = XR * XW * (CIN / 4), NVY = RS * W * (COUT / 4), NV = NVX + NVY;
    constexpr int NLD = (NV + 511) / 512;
    constexpr int NPAIR = RS * W / 2;
    extern __shared__ __attribute__((aligned(16))) float wg_lds[];
    float* Xs = wg_lds;
    float* Ys = wg_lds + GE::XFLOATS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, k = lane >> 5;
    const int blk = blockIdx.y * BPG + wave / KS, ks = wave % KS;
    const int mb = blk / NBK, nb = blk % NBK;

    // staging geometry of this thread's vectors (fixed for the whole kernel): LDS float offset and source coordinates
    int st_lds[NLD], st_src[NLD];                     // src: X: row<<20 | col<<10 | channel ; dY: 1<<30 | pixel<<10 | channel
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
        const int v = tid + 512 * q;
        if (v < NVX) {
            const int pix = v / (CIN / 4), c = (v % (CIN / 4)) * 4;
            st_lds[q] = pix * XS + c;
            st_src[q] = ((pix / XW) << 20) | ((pix % XW) << 10) | c;
        } else if (v < NV) {
            const int u = v - NVX, pix = u / (COUT / 4), c = (u % (COUT / 4)) * 4;
            st_lds[q] = GE::XFLOATS + pix * YS + c;
            st_src[q] = (1 << 30) | (pix << 10) | c;
        } else {
            st_lds[q] = -1; st_src[q] = 0;
        }
    }
    constexpr int SPI = H / RS;                       // strips per image
    const int nstrips = a.nimg * SPI;
    float4 stg[NLD];
    auto issue = [&](int st) {
        const int img = st / SPI, y0 = (st % SPI) * RS;
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            const int sd = st_src[q], c = sd & 1023;
            if (st_lds[q] >= 0) {
                if (sd >> 30) {
                    const int pix = (sd >> 10) & 0xFFFFF;
                    val = *reinterpret_cast<const float4*>(a.dY + ((size_t)(img * H + y0) * W + pix) * COUT + c);
                } else {
                    const int gy = y0 - 1 + (sd >> 20), gx = ((sd >> 10) & 1023) - 1;
                    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                        const size_t px = (size_t)(img * H + gy) * W + gx;
                        val = c < C0 ? *reinterpret_cast<const float4*>(a.in0 + px * C0 + c)
                                     : *reinterpret_cast<const float4*>(a.in1 + px * C1 + (c - C0));
                    }
                }
            }
            stg[q] = val;
        }
    };

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int lane_a = k * YS + mb * 32 + i;          // dY operand: row = co, k = pixel of the pair
    const int lane_b = k * XS + nb * 32 + i;          // X operand: column = ci

    WG3_T(0);
    int tc = 1;
    float bsum = 0.f;
    int st = blockIdx.x;
    if (st < nstrips) issue(st);
    for (; st < nstrips; st += gridDim.x) {
        __syncthreads();                              // everyone is done reading the previous strip
#pragma unroll
        for (int q = 0; q < NLD; ++q)
            if (st_lds[q] >= 0) *reinterpret_cast<float4*>(wg_lds + st_lds[q]) = stg[q];
        __syncthreads();
        WG3_T(tc); ++tc;
        if (st + (int)gridDim.x < nstrips) issue(st + gridDim.x);      // flies under this strip's MFMAs
        WG3_T(tc); ++tc;
        // bias gradient: column sums of the staged dY strip (ten adds per thread per strip)
        if (blockIdx.y == 0) {
            const int bc = tid % COUT;
            for (int px = tid / COUT; px < RS * W; px += 512 / COUT) bsum += Ys[px * YS + bc];
        }
        // this wave's pixel pairs ks, ks+KS, ...: the ten operands of pair j+1 are read from LDS before the nine
        // MFMAs of pair j are issued (ping-pong registers), so the LDS round trip never stalls the MFMA pipe
        constexpr int CNT = NPAIR / KS;
        static_assert(NPAIR % KS == 0 && CNT % 2 == 0, "pair split");
        auto ld = [&](int j, float& av, float (&bv)[9]) {
            const int pi = ks + j * KS;
            const int r = pi / (W / 2), x = 2 * (pi % (W / 2));
            av = Ys[(r * W + x) * YS + lane_a];
            const float* xb = Xs + (r * XW + x) * XS + lane_b;
#pragma unroll
            for (int t = 0; t < 9; ++t) bv[t] = xb[((t / 3) * XW + (t % 3)) * XS];
        };
        float a0, b0[9], a1, b1[9];
        ld(0, a0, b0);
        for (int j = 0; j < CNT; j += 2) {
            ld(j + 1, a1, b1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[t] = mfma32(a0, b0[t], acc[t]);
            __builtin_amdgcn_sched_barrier(0);
            if (j + 2 < CNT) ld(j + 2, a0, b0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[t] = mfma32(a1, b1[t], acc[t]);
            __builtin_amdgcn_sched_barrier(0);
        }
        WG3_T(tc); ++tc;
    }
    WG3_T(30);
    if (blockIdx.y == 0) {                                            // fold the 512/COUT pixel shares of every channel
        __syncthreads();
        wg_lds[tid] = bsum;
        __syncthreads();
        if (tid < COUT) {
            float sb = 0.f;
            for (int q = 0; q < 512 / COUT; ++q) sb += wg_lds[q * COUT + tid];
            a.partial[(size_t)gridDim.y * gridDim.x * BPG * WG3_RN + (size_t)blockIdx.x * COUT + tid] = sb;
        }
    }
    wg3_slot_epilogue<BPG, KS>(wg_lds, a.partial + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * BPG) * WG3_RN, acc, tid, wave, lane);
    WG3_T(31);
}

// ------------------------------- the reduce over the partial images -----------------------------------------------
// dW[co][ci][tap] of block gb = sum over the nx workgroups of partial[by][bx][b][tap][co][ci]   (gb = by*bpg + b).
// A workgroup takes 64 elements of a block; every element's sum over the nx partial images is cut into four interleaved quarter
// sums (one per wave, up to eight loads in flight), folded through LDS; every dW element has exactly one writer.  (Round 2: one
// thread per element walked all nx = 128-256 images -- a chain of 32-64 dependent round trips, 13-24 us per layer, 128 us of the
// bf16 step -- or, for the small layers, NZ groups meeting in dW with atomics.)  Block `local` of a layer's 144 * blocks + 1:
// the last one folds the per-workgroup bias partials behind the images.
struct Wg3RedLayer {
    const float* partial; float* dW; float* db;
    int nx, ny, bpg, cin, cout, first_block;      // first_block: prefix sum of (144 * nblk + 1) over the layers before this one
};
__device__ __forceinline__ void wg3_reduce_block(const float* partial, float* dW, float* db, int nx, int ny, int bpg, int cin,
                                                 int cout, int local, float* sb /* [256] LDS */) {
    const int nbk = cin >> 5, nblk = (cout >> 5) * nbk;
    if (local == 144 * nblk) {                                  // the layer's bias gradient
        const int c = threadIdx.x % cout, part = threadIdx.x / cout, np = 256 / cout;     // cout divides 256
        const float* bsrc = partial + (size_t)ny * nx * bpg * WG3_RN + c;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
        int x = part;
        for (; x + 3 * np < nx; x += 4 * np) {
            v0 += bsrc[(size_t)x * cout]; v1 += bsrc[(size_t)(x + np) * cout];
            v2 += bsrc[(size_t)(x + 2 * np) * cout]; v3 += bsrc[(size_t)(x + 3 * np) * cout];
        }
        for (; x < nx; x += np) v0 += bsrc[(size_t)x * cout];
        sb[threadIdx.x] = (v0 + v1) + (v2 + v3);
        __syncthreads();
        if ((int)threadIdx.x < cout) {
            float t = 0.f;
            for (int q = 0; q < np; ++q) t += sb[q * cout + threadIdx.x];
            db[threadIdx.x] += t;
        }
        return;
    }
    const int gb = local / 144, ex = local - gb * 144;
    const int e = ex * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    const int by = gb / bpg, b = gb - by * bpg;
    const float* src = partial + ((size_t)by * nx * bpg + b) * WG3_RN + e;
    const size_t ST = (size_t)bpg * WG3_RN;
    float sacc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) sacc[k] = 0.f;
    int x = q;
    for (; x + 28 < nx; x += 32) {
#pragma unroll
        for (int k = 0; k < 8; ++k) sacc[k] += src[(size_t)(x + 4 * k) * ST];
    }
    for (; x < nx; x += 4) sacc[0] += src[(size_t)x * ST];
    sb[threadIdx.x] = ((sacc[0] + sacc[1]) + (sacc[2] + sacc[3])) + ((sacc[4] + sacc[5]) + (sacc[6] + sacc[7]));
    __syncthreads();
    if (q == 0) {
        const float v = (sb[threadIdx.x] + sb[64 + threadIdx.x]) + (sb[128 + threadIdx.x] + sb[192 + threadIdx.x]);
        const int t = e >> 10, m = (e >> 5) & 31, n = e & 31;
        const int gmb = gb / nbk, gnb = gb - gmb * nbk;
        dW[((size_t)(gmb * 32 + m) * cin + gnb * 32 + n) * 9 + t] += v;
    }
}

// ONE reduce launch for the 3x3 layers of a backward pass (round 5): every layer's weight-gradient launch leaves its partial images in
// its OWN region of the workspace and a descriptor here; this kernel runs wg3_reduce_block for all of them in one grid.  Ten
// launches of 145 x NBLK blocks -- 9-13 us each, none of them filling the chip -- become one of ~6 800 blocks.  The per-layer form
// (GIGA_WGRAD_ONE_REDUCE=0) is this kernel with a one-layer descriptor: the same blocks, element -> thread map and order of
// summation, hence bit-identical results.
constexpr int WG3_RED_MAX = 10;
struct Wg3RedArgs { Wg3RedLayer L[WG3_RED_MAX]; int nlayers; int nblocks; };

__global__ __launch_bounds__(256) void wgrad3_reduce_all_kernel(Wg3RedArgs A) {
    __shared__ float sb[256];
    const int bid = blockIdx.x;
    const float* partial = A.L[0].partial; float* dW = A.L[0].dW; float* db = A.L[0].db;
    int nx = A.L[0].nx, ny = A.L[0].ny, bpg = A.L[0].bpg, cin = A.L[0].cin, cout = A.L[0].cout, first = 0;
#pragma unroll
    for (int i = 1; i < WG3_RED_MAX; ++i)
        if (i < A.nlayers && bid >= A.L[i].first_block) {
            partial = A.L[i].partial; dW = A.L[i].dW; db = A.L[i].db;
            nx = A.L[i].nx; ny = A.L[i].ny; bpg = A.L[i].bpg; cin = A.L[i].cin; cout = A.L[i].cout; first = A.L[i].first_block;
        }
    wg3_reduce_block(partial, dW, db, nx, ny, bpg, cin, cout, bid - first, sb);
}

static int launch_wgrad3_reduce_all(const Wg3RedArgs& R, hipStream_t s) {
    if (R.nlayers == 0) return 0;
    GIGA_LAUNCH(wgrad3_reduce_all_kernel, dim3(R.nblocks), dim3(256), 0, s, R);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}
// what every launcher does behind its weight-gradient kernel (grid nx x ny, bpg blocks per workgroup): describe the layer's
// reduce for the one launch at the end of the pass (`defer`), or launch it now for this layer alone (defer == nullptr)
static int wg3_reduce(Wg3RedArgs* defer, const Wgrad3Args& a, int nx, int ny, int bpg, int cin, int cout, hipStream_t s) {
    Wg3RedArgs one{};
    Wg3RedArgs* R = defer ? defer : &one;
    Wg3RedLayer& L = R->L[R->nlayers++];
    L.partial = a.partial; L.dW = a.dW; L.db = a.db; L.nx = nx; L.ny = ny; L.bpg = bpg; L.cin = cin; L.cout = cout;
    L.first_block = R->nblocks;
    R->nblocks += 144 * (cout / 32) * (cin / 32) + 1;
    return defer ? (hipGetLastError() == hipSuccess ? 0 : -10) : launch_wgrad3_reduce_all(one, s);
}

template <int C0, int C1, int COUT, int H, int RS>
static int launch_wgrad3(const Wgrad3Args& a, hipStream_t s, Wg3RedArgs* defer = nullptr) {
    using GE = Wg3GeomF32<C0 + C1, COUT, H, RS>;
    constexpr int CIN = C0 + C1;
    constexpr int NBLK = (COUT / 32) * (CIN / 32), BPG = NBLK < 8 ? NBLK : 8, NY = NBLK / BPG;
    const int nstrips = a.nimg * (H / RS);
    int gx = 256 / NY;
    if (gx > nstrips) gx = nstrips;
    auto kern = conv3_wgrad_kernel<C0, C1, COUT, H, RS>;
    giga::dyn_lds_once(reinterpret_cast<const void*>(kern), (int)GE::LDS_BYTES);
    GIGA_LAUNCH(kern, dim3(gx, NY), dim3(512), GE::LDS_BYTES, s, a);
    return wg3_reduce(defer, a, gx, NY, BPG, CIN, COUT, s);
}

// ------------------------------- 3x3 weight gradient on bf16 MFMA (BASELINE c5) -----------------------------
// dW[co][ci][tap] = sum_pixels dY[p][co] * X[p + tap][ci]   with bf16 operands, fp32 accumulation: v_mfma_f32_32x32x16_bf16,
// D[co][ci] += A[co][k] * B[k][ci], k = 16 PIXELS per instruction (the fp32 kernel above: 2 pixels per 64-cycle instruction).
// Same decomposition, partial images, epilogue and reduce kernel as conv3_wgrad_kernel; what changes is the operand side:
//   * the contraction runs over pixels, so a lane needs 8 consecutive pixels of ONE channel: the strips are staged
//     TRANSPOSED, channel-major bf16 -- Xt[ci][row][col], Yt[co][row][col].  A staging item is (4 channels, row, 8-pixel
//     group): eight coalesced float4 loads (a pixel's channels are contiguous across lanes), converted and written as four
//     16-byte rows.  Rounding to bf16 happens here, once per element.
//   * a k-chunk = two 8-pixel groups (lane half hi takes group 2j + hi); groups tile the rows (40 = 5 groups; 20 and 10 are
//     padded to 24 / 16 with zeros, which contribute nothing).
//   * the three horizontal taps are ONE aligned 16-byte read plus the two neighbouring elements (two 4-byte reads), shifted
//     into place with v_alignbyte_b32: per k-chunk 1 + 3 x 3 LDS reads and 24 VALU feed nine MFMAs (288 matrix cycles).
//   X columns: data at col 8 + x; cols < 8 and >= 8 + 8G stay zero (the convolution's zero padding), zeroed once.
typedef __bf16 wbf8 __attribute__((ext_vector_type(8)));
// channel stride (bf16 elements) of the transposed strips: the smallest value >= n that is 8 mod 128, i.e. 16 bytes mod 256: the 32
// lanes of an operand read (one channel each, 16 bytes) then fall into 16 different 16-byte bank groups per pass -- with the natural
// stride (rows x pitch: 0 or 64 bytes mod 256 for every layer) they shared one to four (a third of the launch's cycles carried LDS
// bank conflicts: 2-8.6 M per launch) -- and the staging stores of 16 channel quads hit four bank groups instead of one.
constexpr int wg_cs(int n) { return (n - 8 + 127) / 128 * 128 + 8; }

// transposed bf16 strips of a workgroup that stages CINW input and COUTW output channels: kernels and launcher read the same numbers
template <int CINW, int COUTW, int H, int RS>
struct Wg3Geom {
    static constexpr int W = H;
    static constexpr int G = (W + 7) / 8;                    // 8-pixel groups per row
    static constexpr int PY = 8 * G, PX = 8 * G + 16;        // row pitches (bf16 elements)
    static constexpr int XR = RS + 2;
    static constexpr int QX = CINW / 4, QY = COUTW / 4;      // channel quads
    static constexpr int NVX = QX * XR * G, NVY = QY * RS * G, NV = NVX + NVY;     // staging items
    static constexpr int XCS = wg_cs(XR * PX), YCS = wg_cs(RS * PY);               // channel strides
    static constexpr int XELEMS = CINW * XCS, YELEMS = COUTW * YCS;                // the dY image sits behind the X image
    static constexpr int NCH = RS * G / 2;                   // k-chunks (two groups each) per strip
    static constexpr int SPI = H / RS;                       // strips per image
    static constexpr size_t STRIP_BYTES = ((size_t)XELEMS + YELEMS) * 2;
    static constexpr size_t LDS_BYTES = STRIP_BYTES > WG3_SLOT_BYTES ? STRIP_BYTES : WG3_SLOT_BYTES;   // strip, or the slots of wg3_slot_epilogue
    static_assert(NV <= 512, "one staging item per thread");
    static_assert((RS * G) % 2 == 0 && H % RS == 0, "strip geometry");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// a thread's staging item: 4 channels (quad cq of the staged X or dY channels) x strip row sr x 8-pixel group sg
struct Wg3Item { bool isx, isy; int cq, sg, sr; };
// (Filled in by the kernels themselves, WG3_ITEM: as a function -- by-value return, out-parameter, member, with the thread range
// asserted -- the same five lines schedule differently and three instantiations of conv3_wgrad_bf16_kernel lose 1-2 VGPRs.)
#define WG3_ITEM(GE, tid)                                                                                   \
    const bool isx = (tid) < GE::NVX, isy = !isx && (tid) < GE::NV;                                          \
    const int u = isx ? (tid) : (tid) - GE::NVX;                                                             \
    const int cq = isx ? u % GE::QX : u % GE::QY;             /* channel quad inside the staged channels */  \
    const int rest = isx ? u / GE::QX : u / GE::QY;                                                          \
    const int sg = rest % GE::G, sr = rest / GE::G;           /* group within the row, strip row */          \
    const Wg3Item it{isx, isy, cq, sg, sr}

// Load item `it` of strip st: channels cx0 + 4 cq .. of the layer input, or cy0 + 4 cq .. of dY.
// All eight loads of a staging item are issued UNCONDITIONALLY from clamped addresses and zeroed when they are stored
// (`ok`, bit e: element e of the item is inside the image): behind `if`s every load sat in its own basic block, the register
// allocator overlapped their destinations and the compiler put s_waitcnt vmcnt(0) between them -- an item cost two to three
// dependent memory round trips instead of one (the strip loop ran at ~6 k clocks per strip, tools/gpu_wgrad_trace.py).
template <int C0, int C1, int COUT, int H, int RS>
__device__ __forceinline__ void wg3_stage_load(const Wgrad3Args& a, const Wg3Item& it, int st, int cx0, int cy0,
                                               float4 (&stg)[8], unsigned& ok) {
    constexpr int W = H, SPI = H / RS;
    const int img = st / SPI, y0 = (st % SPI) * RS;
    const int gy = y0 - 1 + it.sr, gyc = gy < 0 ? 0 : gy >= H ? H - 1 : gy;
    const int c = 4 * it.cq + (it.isx ? cx0 : cy0);             // channel in the tensor
    // (threads without an item read like a dY item of row 0: always a valid address)
    const float* rowp = !it.isx ? a.dY + ((size_t)(img * H + y0 + (it.isy ? it.sr : 0)) * W) * COUT + c
                                : c < C0 ? a.in0 + ((size_t)(img * H + gyc) * W) * C0 + c
                                         : a.in1 + ((size_t)(img * H + gyc) * W) * C1 + (c - C0);
    const int ps = !it.isx ? COUT : c < C0 ? C0 : C1;
    const bool row_ok = it.isy || (it.isx && gy >= 0 && gy < H);
    ok = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int x = 8 * it.sg + e, xc = x < W ? x : W - 1;
        stg[e] = *reinterpret_cast<const float4*>(rowp + (size_t)xc * ps);
        ok |= (row_ok && x < W) ? 1u << e : 0u;
    }
}

__device__ __forceinline__ float wg3_comp(const float4& v, int ch) { return ch == 0 ? v.x : ch == 1 ? v.y : ch == 2 ? v.z : v.w; }
// Store a loaded item into the transposed strips: zero what lies outside the image (okc), transpose the eight pixels x four
// channels, round to bf16, four 16-byte stores.  bias: add the item's fp32 dY values to the thread's four channel sums.
template <class GE>
__device__ __forceinline__ void wg3_stage_store(__bf16* Xt, __bf16* Yt, const Wg3Item& it, const float4 (&stg)[8], unsigned okc,
                                                bool bias, float (&bsum)[4]) {
    if (it.isx || it.isy) {
        __bf16* dst = it.isx ? Xt + (size_t)(4 * it.cq) * GE::XCS + it.sr * GE::PX + 8 + 8 * it.sg
                             : Yt + (size_t)(4 * it.cq) * GE::YCS + it.sr * GE::PY + 8 * it.sg;
        const int cstride = it.isx ? GE::XCS : GE::YCS;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            float v8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v8[e] = (okc >> e & 1u) ? wg3_comp(stg[e], ch) : 0.f;
            wbf8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (__bf16)v8[e];
            *reinterpret_cast<wbf8*>(dst + (size_t)ch * cstride) = o;
            if (it.isy && bias)                       // bias gradient: column sums of dY, from the fp32 values
                bsum[ch] += ((v8[0] + v8[1]) + (v8[2] + v8[3])) + ((v8[4] + v8[5]) + (v8[6] + v8[7]));
        }
    }
}

// the horizontal taps of eight pixels from the aligned 16-byte read `mid` of elements x0 .. x0+7: the same row one element to
// the left (wp = elements x0-2, x0-1) and one to the right (wn = elements x0+8, x0+9)
__device__ __forceinline__ uint4 wg3_tap_left(const uint4& mid, unsigned wp) {
    return uint4{__builtin_amdgcn_alignbyte(mid.x, wp, 2), __builtin_amdgcn_alignbyte(mid.y, mid.x, 2),
                 __builtin_amdgcn_alignbyte(mid.z, mid.y, 2), __builtin_amdgcn_alignbyte(mid.w, mid.z, 2)};
}
__device__ __forceinline__ uint4 wg3_tap_right(const uint4& mid, unsigned wn) {
    return uint4{__builtin_amdgcn_alignbyte(mid.y, mid.x, 2), __builtin_amdgcn_alignbyte(mid.z, mid.y, 2),
                 __builtin_amdgcn_alignbyte(mid.w, mid.z, 2), __builtin_amdgcn_alignbyte(wn, mid.w, 2)};
}
// all three from one row pointer (X row, col of the group's x0)
__device__ __forceinline__ void wg3_taps(const __bf16* row, uint4& left, uint4& mid, uint4& right) {
    mid = *reinterpret_cast<const uint4*>(row);
    const unsigned wp = *reinterpret_cast<const unsigned*>(row - 2);
    const unsigned wn = *reinterpret_cast<const unsigned*>(row + 8);
    left = wg3_tap_left(mid, wp);
    right = wg3_tap_right(mid, wn);
}

// Bias partials of a workgroup of NT threads: the threads of the dY items hold 4 channels each for their (row, group); per-channel
// totals through LDS atomics on red[nch] (<= RS*G addends per channel), stored to dst[0 .. nch).
template <int NT>
__device__ __forceinline__ void wg3_bias_fold(float* red, float* dst, int nch, const Wg3Item& it, const float (&bsum)[4], int tid) {
    __syncthreads();
    for (int c = tid; c < nch; c += NT) red[c] = 0.f;
    __syncthreads();
    if (it.isy) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) atomicAdd(red + 4 * it.cq + ch, bsum[ch]);
    }
    __syncthreads();
    if (tid < nch) dst[tid] = red[tid];
}

// a workgroup stages ALL channels and takes min(blocks, 8) of the 32x32 blocks; blocks beyond 8 go to blockIdx.y
template <int C0, int C1, int COUT, int H, int RS>
__global__ __launch_bounds__(512) void conv3_wgrad_bf16_kernel(Wgrad3Args a) {
    using GE = Wg3Geom<C0 + C1, COUT, H, RS>;
    constexpr int NBK = (C0 + C1) / 32, NBLK = (COUT / 32) * NBK;
    constexpr int BPG = NBLK < 8 ? NBLK : 8;          // blocks per workgroup
    constexpr int KS = 8 / BPG;                       // waves sharing a block (K split)
    extern __shared__ __attribute__((aligned(16))) float wg_lds[];
    __bf16* Xt = reinterpret_cast<__bf16*>(wg_lds);
    __bf16* Yt = Xt + GE::XELEMS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, hi = lane >> 5;
    const int blk = blockIdx.y * BPG + wave / KS, ks = wave % KS;
    const int mb = blk / NBK, nb = blk % NBK;

    // zero the whole X image once: the halo columns are never written again
    for (int v = tid; v < GE::XELEMS / 8; v += 512) reinterpret_cast<uint4*>(Xt)[v] = make_uint4(0, 0, 0, 0);

    WG3_ITEM(GE, tid);
    const int nstrips = a.nimg * GE::SPI;
    float4 stg[8];
    unsigned ok = 0;
    auto issue = [&](int st) { wg3_stage_load<C0, C1, COUT, H, RS>(a, it, st, 0, 0, stg, ok); };

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const __bf16* ya = Yt + (size_t)(mb * 32 + n) * GE::YCS;              // this lane's dY channel row block
    const __bf16* xb = Xt + (size_t)(nb * 32 + n) * GE::XCS + 8;          // this lane's X channel, col of x = 0

    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    int st = blockIdx.x;
    if (st < nstrips) issue(st);
    for (; st < nstrips; st += gridDim.x) {
        __syncthreads();                              // everyone is done reading the previous strip (and the zero fill)
        wg3_stage_store<GE>(Xt, Yt, it, stg, ok, blockIdx.y == 0, bsum);
        __syncthreads();
        if (st + (int)gridDim.x < nstrips) issue(st + gridDim.x);      // flies under this strip's MFMAs
        for (int j = ks; j < GE::NCH; j += KS) {
            const int gi = 2 * j + hi, r = gi / GE::G, xg = gi % GE::G;
            const wbf8 A = *reinterpret_cast<const wbf8*>(ya + r * GE::PY + 8 * xg);
#pragma unroll
            for (int ty = 0; ty < 3; ++ty) {
                uint4 left, mid, right;
                wg3_taps(xb + (r + ty) * GE::PX + 8 * xg, left, mid, right);          // X row y + ty - 1, col of the group's x0
                acc[3 * ty + 0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, __builtin_bit_cast(wbf8, left), acc[3 * ty + 0], 0, 0, 0);
                acc[3 * ty + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, __builtin_bit_cast(wbf8, mid), acc[3 * ty + 1], 0, 0, 0);
                acc[3 * ty + 2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, __builtin_bit_cast(wbf8, right), acc[3 * ty + 2], 0, 0, 0);
            }
        }
    }
    // ---- epilogue: as conv3_wgrad_kernel (the D layout of the bf16 MFMA is the same 32x32 map) ----------------------
    if (blockIdx.y == 0)
        wg3_bias_fold<512>(wg_lds, a.partial + (size_t)gridDim.y * gridDim.x * BPG * WG3_RN + (size_t)blockIdx.x * COUT, COUT, it, bsum, tid);
    wg3_slot_epilogue<BPG, KS>(wg_lds, a.partial + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * BPG) * WG3_RN, acc, tid, wave, lane);
}

// ---- the same kernel with the OUTPUT split over the workgroups as well (the layers with eight or sixteen 32x32 blocks) -------------
// In conv3_wgrad_bf16_kernel a workgroup computes eight blocks for its share of the strips and leaves a partial image of 8 x 36 KiB:
// with 256 workgroups that is 75 MB written and 75 MB read back by the reduce kernel PER LAYER (up0.conv1, down2.conv1, down2.conv2:
// 450 MB of the step's traffic for 7 MB of gradients) against 20-40 MB of operands.  Here a workgroup owns BX blocks that share
// their dY channels (one 32-channel block mb, the X blocks nb0 .. nb0 + BX - 1), the grid is (strips' share, all block groups), and
// only the channels those blocks need are staged: 32 of dY and 32 BX of X.  Same strips, k-chunks, MFMAs and epilogue; 8 / BX
// waves share a block (K split inside the workgroup).  Partial images: 256 workgroups x BX x 36 KiB = 19 MB at BX = 2.
// (Two kernels, not one template over the staged window: with the strip loop in a shared function every instantiation of both
// took two more VGPRs.)
template <int C0, int C1, int COUT, int H, int RS, int BX>
__global__ __launch_bounds__(512) void conv3_wgrad_bf16_ns_kernel(Wgrad3Args a) {
    using GE = Wg3Geom<32 * BX, 32, H, RS>;           // channels this workgroup stages
    constexpr int NBK = (C0 + C1) / 32;
    constexpr int KS = 8 / BX;                        // waves sharing a block (K split); BX blocks per workgroup: (mb, nb0 .. nb0 + BX - 1)
    constexpr int NGX = NBK / BX;                     // X block groups per dY block
    static_assert(NBK % BX == 0 && 8 % BX == 0 && (C1 == 0 || C0 % (32 * BX) == 0), "block groups");
    extern __shared__ __attribute__((aligned(16))) float wg_lds[];
    __bf16* Xt = reinterpret_cast<__bf16*>(wg_lds);
    __bf16* Yt = Xt + GE::XELEMS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, hi = lane >> 5;
    const int mb = blockIdx.y / NGX, nb0 = (blockIdx.y % NGX) * BX;       // this workgroup's dY block and first X block
    const int nbl = wave / KS, ks = wave % KS;                            // this wave's block (local X block index) and K share

    // zero the whole X image once: the halo columns are never written again
    for (int v = tid; v < GE::XELEMS / 8; v += 512) reinterpret_cast<uint4*>(Xt)[v] = make_uint4(0, 0, 0, 0);

    WG3_ITEM(GE, tid);
    const int nstrips = a.nimg * GE::SPI;
    float4 stg[8];
    unsigned ok = 0;
    auto issue = [&](int st) { wg3_stage_load<C0, C1, COUT, H, RS>(a, it, st, 32 * nb0, 32 * mb, stg, ok); };

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const __bf16* ya = Yt + (size_t)n * GE::YCS;                           // this lane's dY channel (of block mb)
    const __bf16* xb = Xt + (size_t)(nbl * 32 + n) * GE::XCS + 8;          // this lane's X channel, col of x = 0

    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    int st = blockIdx.x;
    if (st < nstrips) issue(st);
    for (; st < nstrips; st += gridDim.x) {
        __syncthreads();                              // everyone is done reading the previous strip (and the zero fill)
        wg3_stage_store<GE>(Xt, Yt, it, stg, ok, nb0 == 0, bsum);
        __syncthreads();
        if (st + (int)gridDim.x < nstrips) issue(st + gridDim.x);      // flies under this strip's MFMAs
        for (int j = ks; j < GE::NCH; j += KS) {
            const int gi = 2 * j + hi, r = gi / GE::G, xg = gi % GE::G;
            const wbf8 A = *reinterpret_cast<const wbf8*>(ya + r * GE::PY + 8 * xg);
#pragma unroll
            for (int ty = 0; ty < 3; ++ty) {
                uint4 left, mid, right;
                wg3_taps(xb + (r + ty) * GE::PX + 8 * xg, left, mid, right);          // X row y + ty - 1, col of the group's x0
                acc[3 * ty + 0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, __builtin_bit_cast(wbf8, left), acc[3 * ty + 0], 0, 0, 0);
                acc[3 * ty + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, __builtin_bit_cast(wbf8, mid), acc[3 * ty + 1], 0, 0, 0);
                acc[3 * ty + 2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, __builtin_bit_cast(wbf8, right), acc[3 * ty + 2], 0, 0, 0);
            }
        }
    }
    // ---- epilogue: as conv3_wgrad_kernel; the bias partials of this block's 32 channels ---------------------------------
    if (nb0 == 0)
        wg3_bias_fold<512>(wg_lds, a.partial + (size_t)gridDim.y * gridDim.x * BX * WG3_RN + (size_t)blockIdx.x * COUT + 32 * mb, 32, it, bsum, tid);
    wg3_slot_epilogue<BX, KS>(wg_lds, a.partial + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * BX) * WG3_RN, acc, tid, wave, lane);
}

// ---- the same weight gradient for layers with at most four 32x32 blocks: the NINE TAPS go to nine waves ----------------------
// In conv3_wgrad_bf16_kernel a wave owns a block for all nine taps (144 accumulator registers) and the waves of a block split the
// pixels.  For the layers with one to four blocks (32 -> 32 and 32 + 32 -> 32 at 40x40, 32 -> 64 and 64 -> 64 at 20x20) that leaves
//   * no registers for a second strip of loads in flight: a strip is ~600 clocks of MFMAs against a ~6 k-clock memory round trip,
//     one strip deep the loop runs at one strip per round trip (tools/gpu_wgrad_trace.py, profiles/r03/wgrad3_bf16_trace_layer0.txt);
//   * an epilogue of three LDS rounds in which the 8 waves' tiles are summed (9.6 k of the launch's 44 k clocks).
// Here wave t takes tap t of EVERY block and every k-chunk of the strip: 16 x NBLK accumulator registers, the same number of
// MFMAs per wave, no cross-wave sum at all (a wave writes its tiles straight to the partial image), and two strips of loads in
// flight (ping-pong staging registers).  Workgroup barriers inside the loop are s_barrier after lgkmcnt(0) only: __syncthreads()
// also waits for vmcnt(0), i.e. for the prefetched loads.  Staging, partial-image layout and reduce kernel are unchanged.
template <int C0, int C1, int COUT, int H, int RS>
__global__ __launch_bounds__(576) void conv3_wgrad_bf16_taps_kernel(Wgrad3Args a) {
    using GE = Wg3Geom<C0 + C1, COUT, H, RS>;
    constexpr int CIN = C0 + C1;
    constexpr int NBK = CIN / 32, NMB = COUT / 32, NBLK = NMB * NBK;
    static_assert(NBLK <= 4, "one tap per wave: few blocks");
    constexpr bool DEEP = NBLK == 1;                  // two strips of loads in flight; with 2-4 blocks (32-64 accumulator registers) the second
                                                      // staging set no longer fits the 168 registers of a 9-wave workgroup (100-400 B of scratch)
    constexpr int G = GE::G, PX = GE::PX, PY = GE::PY, XCS = GE::XCS, YCS = GE::YCS, NCH = GE::NCH;
    extern __shared__ __attribute__((aligned(16))) float wg_lds[];
    __bf16* Xt = reinterpret_cast<__bf16*>(wg_lds);
    __bf16* Yt = Xt + GE::XELEMS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // = tap
    const int n = lane & 31, hi = lane >> 5;
    const int ty = wave / 3, tx = wave - 3 * ty;

    for (int v = tid; v < GE::XELEMS / 8; v += 576) reinterpret_cast<uint4*>(Xt)[v] = make_uint4(0, 0, 0, 0);

    WG3_ITEM(GE, tid);
    const int nstrips = a.nimg * GE::SPI;
    auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    float4 stgA[8], stgB[8];
    unsigned okA = 0, okB = 0;
    auto issue = [&](int st, float4 (&stg)[8], unsigned& ok) { wg3_stage_load<C0, C1, COUT, H, RS>(a, it, st, 0, 0, stg, ok); };

    f32x16 acc[NBLK];
#pragma unroll
    for (int b = 0; b < NBLK; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    int st = blockIdx.x;
    const int gstep = (int)gridDim.x;
    if (st < nstrips) issue(st, stgA, okA);
    if (DEEP && st + gstep < nstrips) issue(st + gstep, stgB, okB);
    __syncthreads();                                  // the zero fill of the X image
    auto strip = [&](float4 (&stg)[8], unsigned& ok, int st_) {
        lds_barrier();                                // everyone is done reading the previous strip
        wg3_stage_store<GE>(Xt, Yt, it, stg, ok, true, bsum);
        if (st_ + (DEEP ? 2 : 1) * gstep < nstrips) issue(st_ + (DEEP ? 2 : 1) * gstep, stg, ok);   // into the registers just drained
        lds_barrier();
#pragma unroll 2
        for (int j = 0; j < NCH; ++j) {
            const int gi = 2 * j + hi, r = gi / G, xg = gi % G;
            wbf8 A[NMB], B[NBK];
#pragma unroll
            for (int m = 0; m < NMB; ++m) A[m] = *reinterpret_cast<const wbf8*>(Yt + (size_t)(m * 32 + n) * YCS + r * PY + 8 * xg);
#pragma unroll
            for (int k = 0; k < NBK; ++k) {
                const __bf16* row = Xt + (size_t)(k * 32 + n) * XCS + 8 + (r + ty) * PX + 8 * xg;   // X row y + ty - 1, col of the group's x0
                const uint4 mid = *reinterpret_cast<const uint4*>(row);
                uint4 sel = mid;
                if (tx == 0) sel = wg3_tap_left(mid, *reinterpret_cast<const unsigned*>(row - 2));
                else if (tx == 2) sel = wg3_tap_right(mid, *reinterpret_cast<const unsigned*>(row + 8));
                B[k] = __builtin_bit_cast(wbf8, sel);
            }
#pragma unroll
            for (int m = 0; m < NMB; ++m)
#pragma unroll
                for (int k = 0; k < NBK; ++k)
                    acc[m * NBK + k] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[m], B[k], acc[m * NBK + k], 0, 0, 0);
        }
    };
    if constexpr (DEEP) {
        for (;;) {
            if (st >= nstrips) break;
            strip(stgA, okA, st); st += gstep;
            if (st >= nstrips) break;
            strip(stgB, okB, st); st += gstep;
        }
    } else {
        for (; st < nstrips; st += gstep) strip(stgA, okA, st);
    }
    // ---- epilogue: every wave writes its tap's tiles (D layout: lane (n, hi), register r <-> row (r&3) + 8(r>>2) + 4hi) ------------
    float* part = a.partial + (size_t)blockIdx.x * NBLK * WG3_RN;
#pragma unroll
    for (int b = 0; b < NBLK; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            part[((size_t)(b * 9 + wave) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi) * 32 + n] = acc[b][r];
    wg3_bias_fold<576>(wg_lds, a.partial + (size_t)gridDim.x * NBLK * WG3_RN + (size_t)blockIdx.x * COUT, COUT, it, bsum, tid);
}

template <int C0, int C1, int COUT, int H, int RS>
static int launch_wgrad3_bf16(const Wgrad3Args& a, hipStream_t s, Wg3RedArgs* defer = nullptr) {
    using GE = Wg3Geom<C0 + C1, COUT, H, RS>;
    constexpr int CIN = C0 + C1;
    constexpr int NBLK = (COUT / 32) * (CIN / 32), BPG = NBLK < 8 ? NBLK : 8, NY = NBLK / BPG;
    const int nstrips = a.nimg * GE::SPI;
    int gx = 256 / NY;
    if (gx > nstrips) gx = nstrips;
    if constexpr (NBLK <= 4) {                        // one tap per wave (conv3_wgrad_bf16_taps_kernel)
        static const bool taps = [] { const char* e = getenv("GIGA_WGRAD_TAPS"); return !e || atoi(e) != 0; }();
        if (taps) {
            auto kern = conv3_wgrad_bf16_taps_kernel<C0, C1, COUT, H, RS>;
            giga::dyn_lds_once(reinterpret_cast<const void*>(kern), (int)GE::STRIP_BYTES);
            GIGA_LAUNCH(kern, dim3(gx), dim3(576), GE::STRIP_BYTES, s, a);
            return wg3_reduce(defer, a, gx, NY, BPG, CIN, COUT, s);
        }
    }
    if constexpr (NBLK > 4) {                         // the output split over the workgroups too (conv3_wgrad_bf16_ns_kernel)
        static const bool nsplit = [] { const char* e = getenv("GIGA_WGRAD_NSPLIT"); return !e || atoi(e) != 0; }();
        if (nsplit) {
            constexpr int BX = 2, NYS = NBLK / BX;
            using GN = Wg3Geom<32 * BX, 32, H, RS>;
            int gxs = 256 / NYS;
            if (gxs > nstrips) gxs = nstrips;
            auto kns = conv3_wgrad_bf16_ns_kernel<C0, C1, COUT, H, RS, BX>;
            giga::dyn_lds_once(reinterpret_cast<const void*>(kns), (int)GN::LDS_BYTES);
            GIGA_LAUNCH(kns, dim3(gxs, NYS), dim3(512), GN::LDS_BYTES, s, a);
            return wg3_reduce(defer, a, gxs, NYS, BX, CIN, COUT, s);
        }
    }
    auto kern = conv3_wgrad_bf16_kernel<C0, C1, COUT, H, RS>;
    giga::dyn_lds_once(reinterpret_cast<const void*>(kern), (int)GE::LDS_BYTES);
    GIGA_LAUNCH(kern, dim3(gx, NY), dim3(512), GE::LDS_BYTES, s, a);
    return wg3_reduce(defer, a, gx, NY, BPG, CIN, COUT, s);
}

}  // namespace giga
