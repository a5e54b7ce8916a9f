// The extern "C" entry points of libgiga_hip.so (declared in include/giga_hip.h) that span kernel files or belong to none: version and
// giga_strerror, packing / repacking / deriving the weight images (with their kernels), the encoder forward call
// with its probe, giga_backward and its workspace functions, the launch probe and counter, giga_forget_device_state, the event
// helpers and host register / unregister.  Every other entry point stands in the file of its kernels, after them (giga_post.hip,
// giga_eval.hip, giga_mesh.hip, ...); host checks that several of those share are in giga_check.h.
#include <hip/hip_runtime.h>

#include <cstring>

#include "giga_launch.h"

#include "../../include/giga_hip.h"
#include "giga_layout.h"
#include "giga_conv32_geom.h"
#include "giga_dect.h"
#include "giga_args.h"
#include "giga_enc_plan.h"
#include "giga_side.h"
#include "giga_dec_bwd_launch.h"

namespace giga {
// giga_pack.cpp
size_t packed_bytes();
int pack_weights_host(const float* P, size_t n_params, int head_present, uint8_t* blob, size_t blob_bytes);
int pack_map_host(int head_present, int32_t* map, size_t nwords);
size_t bwd_packed_bytes();
int pack_bwd_host(const float* P, size_t n_params, int head_present, uint8_t* blob, size_t blob_bytes);
int pack_bwd_map_host(int head_present, int32_t* map, size_t nwords);
int packed_check_host(const uint8_t* blob, size_t bytes, int backward);
// giga_encoder_bwd.hip (the training decoder's launchers: giga_dec_bwd_launch.h)
void persistent_forget();
int launch_encoder_backward(const float* tsdf, const uint8_t* blob, const uint8_t* bwd_blob, const uint8_t* fws,
                            float* gplanes, uint8_t* gws, float* grads, int head_present, int B, hipStream_t s, bool bf16_convs, bool convin_mask,
                            SideScope& side);
// giga_encoder.hip
int launch_encoder(const float* tsdf, const uint8_t* blob, void* planes_nhwc, float* planes_nchw, int B,
                   int precision, uint8_t* ws, hipStream_t s, int probe_stage, void* ev0, void* ev1);
}  // namespace giga

using namespace giga;

std::atomic<unsigned long long> giga::g_launch_count{0};
std::atomic<unsigned long long> giga::g_probe_target{0};
void* giga::g_probe_ev[2] = {nullptr, nullptr};
const char* volatile giga::g_probe_name = "";

// blob word w <- params[map[w]] (map >= 0) | 0 (map == -1) | untouched (map == -2)
__global__ void repack_kernel(const float* __restrict__ params, const int32_t* __restrict__ map,
                              float* __restrict__ words, size_t nwords) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwords) return;
    const int m = map[i];
    if (m >= 0) words[i] = params[m];
    else if (m == -1) words[i] = 0.f;
}

// bf16 fragment images (f16 fragment layout: lane (j, g) holds channels 8g..8g+7 of k-group kg32) from the fp32 fragments
// (lane (j, g') holds channels 4g'..4g'+3 of k-group kg16 = 2*kg32 + h): one workgroup per bf16 fragment.
struct BfRegions { size_t src[2 * NCONV], dst[2 * NCONV]; int first[2 * NCONV + 1]; int n; };
__device__ __forceinline__ void derive_bf16_block(uint8_t* fwd, uint8_t* bwd, const BfRegions& r, int blk) {
    int reg = 0;
    while (reg + 1 < r.n && blk >= r.first[reg + 1]) ++reg;
    const int i16 = blk - r.first[reg], lane = threadIdx.x;
    uint8_t* base = reg < NCONV ? fwd : bwd;
    if (!base) return;
    const float* f32 = reinterpret_cast<const float*>(base + r.src[reg]);
    __bf16* out = reinterpret_cast<__bf16*>(base + r.dst[reg]) + ((size_t)i16 * 64 + lane) * 8;
    const int j = lane & 15, g = lane >> 4;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = 8 * g + e;
        out[e] = (__bf16)f32[((size_t)(2 * i16 + c / 16) * 64 + ((c % 16) / 4) * 16 + j) * 4 + c % 4];
    }
}

// bf16 conv32 images (A operands of v_mfma_f32_32x32x16_bf16, giga_pack.cpp: lane (i, hi), element e -> W[32 cs + c32_row_cout(i)][16 kc +
// 8 hi + e][tap], fragment order [sub][cs][tap][kc]) from the fp32 conv16 fragments of the same layer (lane (j, g), element e ->
// W[16 nb + j][16 kg + 4 g + e][tap], order [sub][nb][tap][kg]): one workgroup per conv32 fragment.
struct C32bRegions { size_t src[NCONV], dst[NCONV]; int first[NCONV + 1]; int nbt[NCONV], taps[NCONV], kg[NCONV]; };
__device__ __forceinline__ void derive_c32b_block(uint8_t* fwd, const C32bRegions& r, int blk) {
    int l = 0;
    while (l + 1 < NCONV && blk >= r.first[l + 1]) ++l;
    const int f = blk - r.first[l], lane = threadIdx.x;
    const int KG = r.kg[l], TAPS = r.taps[l], NBT = r.nbt[l], CS = NBT / 2;
    const int kc = f % KG, tap = (f / KG) % TAPS, cs = (f / (KG * TAPS)) % CS, sub = f / (KG * TAPS * CS);
    const int i = lane & 31, hi = lane >> 5;
    const int co = 32 * cs + c32_row_cout(i), nb = co >> 4, j = co & 15;
    const float* f32 = reinterpret_cast<const float*>(fwd + r.src[l]);
    const size_t i32 = ((size_t)(sub * NBT + nb) * TAPS + tap) * KG + kc;
    __bf16* out = reinterpret_cast<__bf16*>(fwd + r.dst[l]) + ((size_t)f * 64 + lane) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int rr = 8 * hi + e;
        out[e] = (__bf16)f32[(i32 * 64 + (rr >> 2) * 16 + j) * 4 + (rr & 3)];
    }
}

// Winograd F(2x2, 3x3) images (giga_wino.h; giga_pack.cpp::pack_wino) from the fp32 conv16 fragments of the same layer: one workgroup per
// 512-byte piece [grp][kpass][pos][chunk][half] = 64 lanes x 2 floats, U = G g G^T accumulated in double in the packer's order, so the
// device image equals the host's bit for bit.
struct WinoRegions { size_t src[NCONV], dst[NCONV]; int first[NCONV + 1]; int cin[NCONV]; };
__device__ __forceinline__ void derive_wino_block(uint8_t* fwd, const WinoRegions& r, int blk) {
    int l = 0;
    while (l + 1 < NCONV && blk >= r.first[l + 1]) ++l;
    const int f = blk - r.first[l], lane = threadIdx.x;
    const int cin = r.cin[l], kp = cin > 64 ? cin / 64 : 1, cinp = cin / kp, nchunk = cinp / 16, KG = cin / 16;
    const int h = f & 1, cc = (f >> 1) % nchunk, pos = (f / (2 * nchunk)) & 15, k = (f / (32 * nchunk)) % kp, grp = f / (32 * nchunk * kp);
    const int j = lane & 15, g = lane >> 4, xi = pos >> 2, nu = pos & 3;
    const float* f32 = reinterpret_cast<const float*>(fwd + r.src[l]);           // [nb][tap][kg][lane (j, g')][e']: W[16 nb + j][16 kg + 4 g' + e'][tap]
    float* out = reinterpret_cast<float*>(fwd + r.dst[l]) + ((size_t)f * 64 + lane) * 2;
    const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int ci = cinp * k + 16 * cc + 4 * g + 2 * h + e;
        double u = 0.0;
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) {
                const float w = f32[((((size_t)grp * 9 + ky * 3 + kx) * KG + ci / 16) * 64 + ((ci % 16) / 4) * 16 + j) * 4 + ci % 4];
                u += G[xi][ky] * G[nu][kx] * (double)w;
            }
        out[e] = (float)u;
    }
}

constexpr int DECT_DERIVE_BLOCKS = (59 + 51) * NHEADS;
struct DeriveArgs {
    BfRegions r; C32bRegions c; int n16, n32;
    size_t dec32_0, dec32_stride, dectf_0, dectf_stride, decb_0, decb_stride, dectb_0, dectb_stride;
    size_t convin_w, convin_ws;
};
__global__ __launch_bounds__(64) void derive_all_kernel(uint8_t* fwd, uint8_t* bwd, DeriveArgs d) {
    const int b = blockIdx.x;
    if (b < d.n16) derive_bf16_block(fwd, bwd, d.r, b);
    else if (b < d.n16 + d.n32) derive_c32b_block(fwd, d.c, b - d.n16);
    else if (b == d.n16 + d.n32 + DECT_DERIVE_BLOCKS) {
        // f16x3 split conv_in operands (giga_pack.cpp): [2 channel halves][hi | lo][lane (j, g)][8 halfs e] <- W[16 h + j][ci16_tap(g, e)],
        // from the fp32 image [h][K-step s of 4 taps][lane (j, k)] = W[16 h + j][4 s + k]
        if (!fwd) return;
        const float* cw = reinterpret_cast<const float*>(fwd + d.convin_w);
        _Float16* cs = reinterpret_cast<_Float16*>(fwd + d.convin_ws);
        const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
        for (int h = 0; h < 2; ++h)
            for (int e = 0; e < 8; ++e) {
                const int tap = ci16_tap(g, e);
                const float w = tap >= 0 ? cw[(h * 7 + tap / 4) * 64 + (tap % 4) * 16 + j] : 0.f;
                const _Float16 hi = (_Float16)w;
                cs[((2 * h) * 64 + lane) * 8 + e] = hi;
                cs[((2 * h + 1) * 64 + lane) * 8 + e] = (_Float16)(w - (float)hi);
            }
    } else {
        const int k = b - d.n16 - d.n32;
        dect_derive_block(fwd, bwd, k % (59 + 51), k / (59 + 51), d.dec32_0, d.dec32_stride, d.dectf_0, d.dectf_stride, d.decb_0,
                          d.decb_stride, d.dectb_0, d.dectb_stride);
    }
}
__global__ void repack2_kernel(const float* __restrict__ params, const int32_t* __restrict__ map_a, float* __restrict__ words_a, size_t na,
                               const int32_t* __restrict__ map_b, float* __restrict__ words_b, size_t nb) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t* map = map_a; float* words = words_a;
    if (i >= na) { i -= na; if (i >= nb) return; map = map_b; words = words_b; }
    const int m = map[i];
    if (m >= 0) words[i] = params[m];
    else if (m == -1) words[i] = 0.f;
}

// one launch for both blobs: blocks [0, nf) derive the forward blob's images, the rest the backward blob's
__global__ __launch_bounds__(64) void derive_wino_kernel(uint8_t* fwd, WinoRegions wf, int nf, uint8_t* bwd, WinoRegions wb) {
    const int b = (int)blockIdx.x;
    if (b < nf) derive_wino_block(fwd, wf, b);
    else derive_wino_block(bwd, wb, b - nf);
}

extern "C" {

/* Winograd images of the fp32 3x3 layers (giga_wino.h) from the fp32 fragments of the same DEVICE blob, after giga_repack_device:
 * the forward blob's (the layers themselves) and / or the backward blob's (their data-gradient convolutions: the same fragment layout
 * with the channels swapped) -- either pointer may be NULL */
int giga_derive_winograd(void* packed_dev, void* bwd_packed_dev, void* stream) {
    if (!packed_dev && !bwd_packed_dev) return -1;
    const PackOff ko = pack_offsets();
    const BwdPackOff bo = bwd_pack_offsets();
    WinoRegions w[2] = {};
    int n[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        if (!(pass ? bwd_packed_dev : packed_dev)) continue;
        int nw = 0;
        for (int l = 0; l < NCONV; ++l) {
            const ConvLayerDesc& cd = kConv[l];
            w[pass].src[l] = pass ? bo.conv[l] : ko.conv[l].w32; w[pass].dst[l] = pass ? bo.wino[l] : ko.conv[l].wino; w[pass].first[l] = nw;
            w[pass].cin[l] = pass ? cd.cout : cd.cin0 + cd.cin1;                      // channels IN of the convolution the image is for
            if (cd.kind == CONV3) nw += (cd.cin0 + cd.cin1) * cd.cout / 8;           // 512-byte pieces of the layer's image
        }
        w[pass].first[NCONV] = nw;
        n[pass] = nw;
    }
    GIGA_LAUNCH(derive_wino_kernel, dim3(n[0] + n[1]), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<uint8_t*>(packed_dev), w[0], n[0],
                static_cast<uint8_t*>(bwd_packed_dev), w[1]);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int giga_derive_bf16_fragments(void* packed_dev, void* bwd_packed_dev, void* stream) {
    if (!packed_dev && !bwd_packed_dev) return -1;
    const PackOff ko = pack_offsets();
    const BwdPackOff bo = bwd_pack_offsets();
    DeriveArgs d{};
    int at = 0;
    for (int l = 0; l < NCONV; ++l) { d.r.src[l] = ko.conv[l].w32; d.r.dst[l] = ko.conv[l].wbf; d.r.first[l] = at; at += ko.conv[l].nfrag16; }
    for (int l = 0; l < NCONV; ++l) {
        d.r.src[NCONV + l] = bo.conv[l]; d.r.dst[NCONV + l] = bo.convbf[l]; d.r.first[NCONV + l] = at; at += bo.nfrag[l] / 2;
    }
    d.r.first[2 * NCONV] = at;
    d.r.n = 2 * NCONV;
    d.n16 = at;
    int n32 = 0;
    for (int l = 0; l < NCONV; ++l) {
        const ConvLayerDesc& cd = kConv[l];
        d.c.src[l] = ko.conv[l].w32; d.c.dst[l] = ko.conv[l].c32b; d.c.first[l] = n32; n32 += ko.conv[l].nfragc32;
        d.c.nbt[l] = cd.cout / 16; d.c.taps[l] = conv_taps(cd); d.c.kg[l] = (cd.cin0 + cd.cin1) / 16;
    }
    d.c.first[NCONV] = n32;
    d.n32 = packed_dev ? n32 : 0;
    d.dec32_0 = ko.dec32[0]; d.dec32_stride = ko.dec32[1] - ko.dec32[0]; d.dectf_0 = ko.dect[0]; d.dectf_stride = ko.dect[1] - ko.dect[0];
    d.decb_0 = bo.dec[0]; d.decb_stride = bo.dec[1] - bo.dec[0]; d.dectb_0 = bo.dect[0]; d.dectb_stride = bo.dect[1] - bo.dect[0];
    d.convin_w = ko.convin_w; d.convin_ws = ko.convin_ws;
    // ONE launch: the bf16 conv16 fragments of both blobs, the bf16 conv32 images, the bf16 decoder images (giga_dect.h), the f16x3 conv_in operands
    GIGA_LAUNCH(derive_all_kernel, dim3(d.n16 + d.n32 + DECT_DERIVE_BLOCKS + 1), dim3(64), 0, static_cast<hipStream_t>(stream),
                static_cast<uint8_t*>(packed_dev), static_cast<uint8_t*>(bwd_packed_dev), d);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

/* both weight images in ONE launch (training: every step) */
int giga_repack_device2(const float* params_dev, const int32_t* map_fwd_dev, void* packed_dev, size_t nwords_fwd,
                        const int32_t* map_bwd_dev, void* bwd_packed_dev, size_t nwords_bwd, void* stream) {
    if (!params_dev || !map_fwd_dev || !packed_dev || !map_bwd_dev || !bwd_packed_dev) return -1;
    const size_t n = nwords_fwd + nwords_bwd;
    if (n == 0) return 0;
    GIGA_LAUNCH(repack2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), params_dev,
                map_fwd_dev, static_cast<float*>(packed_dev), nwords_fwd, map_bwd_dev, static_cast<float*>(bwd_packed_dev), nwords_bwd);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

static_assert(GIGA_ABI_VERSION == PACK_ABI_VERSION, "the blob stamp carries the ABI version");
int giga_abi_version(void) { return GIGA_ABI_VERSION; }

int giga_packed_check(const void* packed_host, size_t bytes, int backward) {
    if (!packed_host) return -1;
    return packed_check_host(static_cast<const uint8_t*>(packed_host), bytes, backward ? 1 : 0);
}

const char* giga_strerror(int code) {
    switch (code) {
        case 0: return "ok";
        case -1: return "invalid argument";
        case -2: return "parameter count does not match the head set";
        case -3: return "packed buffer too small";
        case -4: return "workspace too small";
        case -5: return "unsupported precision";
        case -6: return "null pointer for a requested output";
        case -7: return "more than GIGA_MAX_SCENES scenes in one call";
        case -8: return "packed blob was not produced by this version of the library (repack the weights)";
        case -10: return "HIP launch failed";
        case -11: return "a face index lies outside its mesh's vertex range";
        case -12: return "mesh simplification: a pass exceeded its round bound, or the reference-list capacity is too small for one collapse";
        default: return "unknown error";
    }
}

size_t giga_param_count(int head_present) { return param_offsets(head_present & 15).total; }

size_t giga_packed_bytes(void) { return packed_bytes(); }

int giga_pack_weights(const float* params_host, size_t n_params, int head_present, void* packed_host,
                      size_t packed_bytes_) {
    if (!params_host || !packed_host) return -1;
    return pack_weights_host(params_host, n_params, head_present & 15, static_cast<uint8_t*>(packed_host),
                             packed_bytes_);
}

int giga_pack_map(int head_present, int32_t* map_host, size_t nwords) {
    if (!map_host) return -1;
    return pack_map_host(head_present & 15, map_host, nwords);
}

int giga_repack_device(const float* params_dev, const int32_t* map_dev, void* packed_dev, size_t nwords,
                       void* stream) {
    if (!params_dev || !map_dev || !packed_dev) return -1;
    if (nwords == 0) return 0;
    GIGA_LAUNCH(repack_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), params_dev, map_dev, static_cast<float*>(packed_dev), nwords);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

size_t giga_encoder_workspace_bytes(int B, int precision) {
    if (B <= 0) return 0;
    return enc_workspace(B, enc_call_from_flags(precision).precision).total;
}

int giga_encoder_workspace_layout(int B, int precision, size_t* offsets) {
    if (B <= 0 || !offsets) return -1;
    precision = enc_call_from_flags(precision).precision;
    if (precision < 0 || precision > 3) return -5;
    const EncWs w = enc_workspace(B, precision);
    const size_t v[17] = {w.P0, w.A0, w.S0, w.Q0, w.A1, w.S1, w.Q1, w.A2, w.S2, w.U0, w.A3, w.A4, w.U1, w.A5, w.A6,
                          w.YZ, w.XZ};
    for (int i = 0; i < 17; ++i) offsets[i] = v[i];
    return 0;
}

// the checks of an encoder call that need no pointer: giga_encoder_forward_probe and giga_encoder_plan answer alike
static int enc_call_check(int B, const EncCall& c) {
    if (B > GIGA_MAX_SCENES) return -7;
    if (c.precision < 0 || c.precision > 3) return -5;
    // only the fp32 and bf16 encoders store conv_in's ReLU mask: a precision 1 / 2 forward that claims to would leave giga_backward
    // (GIGA_CONVIN_MASK_BWD) reading workspace bytes nobody wrote
    if (c.convin_mask && (c.precision == 1 || c.precision == 2)) return -5;
    return 0;
}

int giga_encoder_forward_probe(const float* tsdf, const void* packed, void* planes_nhwc, float* planes_nchw,
                               int B, int precision, void* workspace, size_t workspace_bytes, void* stream,
                               int probe_stage, void* ev_start, void* ev_stop) {
    if (B < 0 || (B > 0 && (!tsdf || !packed || !planes_nhwc || !workspace))) return -1;
    const EncCall call = enc_call_from_flags(precision);
    if (const int rc = enc_call_check(B, call)) return rc;
    if (call.fold_final && planes_nchw) return -1;            // the reference-layout copy is the FINAL planes only
    if (workspace_bytes < giga_encoder_workspace_bytes(B, call.precision)) return -4;
    return launch_encoder(tsdf, static_cast<const uint8_t*>(packed), planes_nhwc, planes_nchw, B, precision,
                          static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream), probe_stage,
                          ev_start, ev_stop);
}

/* host only: the plan an encoder call of these arguments would get now on a device of `cus` compute units, environment knobs included
   (giga_enc_plan.h) */
int giga_encoder_plan(int B, int precision_word, int cus, int probe_stage, int32_t* plan_words) {
    static_assert(ENC_PLAN_WORDS == GIGA_ENCODER_PLAN_WORDS && sizeof(int) == sizeof(int32_t), "the plan's words are the header's");
    static_assert(ENC_FORM_LAYERS_CONV16 == GIGA_ENC_FORM_LAYERS_CONV16 && ENC_FORM_LAYERS_CONV32 == GIGA_ENC_FORM_LAYERS_CONV32 &&
                  ENC_FORM_PERSIST_CONV16 == GIGA_ENC_FORM_PERSIST_CONV16 && ENC_FORM_PERSIST_WINO == GIGA_ENC_FORM_PERSIST_WINO &&
                  ENC_FORM_PERSIST_CONV32 == GIGA_ENC_FORM_PERSIST_CONV32 && ENC_LAYER_CONV16 == GIGA_ENC_LAYER_CONV16 &&
                  ENC_LAYER_CONV32 == GIGA_ENC_LAYER_CONV32 && ENC_LAYER_WINO == GIGA_ENC_LAYER_WINO && ENC_LAYER_UP == GIGA_ENC_LAYER_UP &&
                  (GIGA_ENCODER_PLAN_NO_SLOT & GIGA_ENCODER_FLAGS) == 0, "the form and family ids are the header's");
    if (B < 0 || !plan_words) return -1;
    const bool slot_free = !(precision_word & GIGA_ENCODER_PLAN_NO_SLOT);
    const EncCall call = enc_call_from_flags(precision_word & ~GIGA_ENCODER_PLAN_NO_SLOT);
    if (const int rc = enc_call_check(B, call)) return rc;
    const EncPlan pl = enc_plan(call, B, cus > 0 ? cus : ENC_FULL_DEVICE_CUS, probe_stage, slot_free, enc_knobs_from_env());
    memcpy(plan_words, &pl, sizeof pl);
    return 0;
}

int giga_encoder_forward(const float* tsdf, const void* packed, void* planes_nhwc, float* planes_nchw, int B,
                         int precision, void* workspace, size_t workspace_bytes, void* stream) {
    return giga_encoder_forward_probe(tsdf, packed, planes_nhwc, planes_nchw, B, precision, workspace,
                                      workspace_bytes, stream, -1, nullptr, nullptr);
}

unsigned long long giga_launch_count(void) { return g_launch_count.load(std::memory_order_relaxed); }

int giga_launch_probe(unsigned long long ordinal, void* ev_start, void* ev_stop) {
    if (ordinal != 0 && (!ev_start || !ev_stop)) return -1;
    g_probe_target.store(0, std::memory_order_relaxed);
    g_probe_ev[0] = ev_start; g_probe_ev[1] = ev_stop;
    g_probe_target.store(ordinal, std::memory_order_release);
    return 0;
}
const char* giga_launch_probe_name(void) { return g_probe_name; }

void giga_forget_device_state(void) {
    giga::dyn_lds_forget();
    giga::persistent_forget();
    giga::side_streams_forget();
}

void* giga_event_create(void) {
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? static_cast<void*>(e) : nullptr;
}
void giga_event_destroy(void* ev) { if (ev) (void)hipEventDestroy(static_cast<hipEvent_t>(ev)); }
int giga_event_record(void* ev, void* stream) {
    if (!ev) return -1;
    return hipEventRecord(static_cast<hipEvent_t>(ev), static_cast<hipStream_t>(stream)) == hipSuccess ? 0 : -10;
}
int giga_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms) {
    if (!ev_start || !ev_stop || !ms) return -1;
    if (hipEventSynchronize(static_cast<hipEvent_t>(ev_stop)) != hipSuccess) return -10;
    return hipEventElapsedTime(ms, static_cast<hipEvent_t>(ev_start), static_cast<hipEvent_t>(ev_stop)) == hipSuccess
               ? 0 : -10;
}


// ---------------------------------------------------------------------------------------------------------
// training path (fp32)
size_t giga_bwd_packed_bytes(void) { return bwd_packed_bytes(); }

int giga_pack_bwd_weights(const float* params_host, size_t n_params, int head_present, void* packed_host,
                          size_t packed_bytes_) {
    if (!params_host || !packed_host) return -1;
    return pack_bwd_host(params_host, n_params, head_present & 15, static_cast<uint8_t*>(packed_host), packed_bytes_);
}

int giga_pack_bwd_map(int head_present, int32_t* map_host, size_t nwords) {
    if (!map_host) return -1;
    return pack_bwd_map_host(head_present & 15, map_host, nwords);
}

size_t giga_backward_workspace_bytes(int B, int N, int M, int head_present) {
    if (B <= 0) return 0;
    head_present &= 15;
    // (the size call does not know the decoder's precision: the larger of the two needs.  bf16 -- the dc rows of the occupancy head and
    //  the partial gradient tiles of both calls -- is far below the fp32 path's row arrays except for a handful of points)
    const long long f32 = train_dec_plan(B, N, M, head_present, false, false).scratch_floats;
    const long long b16 = train_dec_plan(B, N, M, head_present, false, true).scratch_floats;
    return align_up((size_t)3 * B * RES * RES * CD * sizeof(float), 256) + enc_bwd_workspace(B).total +
           align_up((size_t)(f32 > b16 ? f32 : b16) * sizeof(float), 256);
}

int giga_backward_workspace_layout(int B, size_t* offsets) {
    if (B <= 0 || !offsets) return -1;
    const BwdWs g = enc_bwd_workspace(B);
    const size_t base = align_up((size_t)3 * B * RES * RES * CD * sizeof(float), 256);     // the plane gradients come first
    const size_t o[15] = {g.gA6, g.gA5, g.gC1, g.gA4, g.gA3, g.gC0, g.gS2, g.gA2, g.gQ1, g.gS1, g.gA1, g.gQ0, g.gS0, g.gA0, g.gP0};
    for (int i = 0; i < 15; ++i) offsets[i] = base + o[i];
    return 0;
}

int giga_backward(const float* tsdf, const void* packed, const void* bwd_packed, const void* enc_workspace_fwd,
                  const void* planes_nhwc, const float* p, const float* p_tsdf, const float* const* outs,
                  const float* const* douts, float* grads, size_t n_params, int head_present, int B, int N, int M,
                  void* workspace, size_t workspace_bytes, void* stream) {
    if (B <= 0) return 0;
    if (!tsdf || !packed || !bwd_packed || !enc_workspace_fwd || !planes_nhwc || !outs || !douts || !grads ||
        !workspace)
        return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    const bool detach_occ = (head_present & GIGA_DETACH_OCC) != 0;     // detach_tsdf, models/__init__.py:61-63
    const bool bf16_convs = (head_present & GIGA_BF16_CONVS) != 0;     // data-gradient convolutions on bf16 MFMA
    const bool bf16_dec = (head_present & GIGA_BF16_DECODER) != 0;     // decoder backward on the fused bf16 kernel
    const bool convin_mask = (head_present & GIGA_CONVIN_MASK_BWD) != 0;   // the forward kept conv_in's ReLU mask (GIGA_CONVIN_MASK)
    head_present &= 15;
    if (N < 0 || M < 0) return -1;
    if (n_params != param_offsets(head_present).total) return -2;
    for (int h = 0; h < NHEADS; ++h) {                                  // every head that will run needs out and dout
        const bool runs = (head_present >> h & 1) && (h < 3 ? N > 0 : (M > 0 && p_tsdf != nullptr));
        if (runs && (!outs[h] || !douts[h])) return -6;
    }
    if ((head_present & 7) && N > 0 && !p) return -1;                   // (every argument is checked before anything is enqueued)
    if (workspace_bytes < giga_backward_workspace_bytes(B, N, M, head_present)) return -4;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const size_t gp_bytes = align_up((size_t)3 * B * RES * RES * CD * sizeof(float), 256);
    float* gplanes = reinterpret_cast<float*>(ws);
    uint8_t* gws = ws + gp_bytes;
    float* scratch = reinterpret_cast<float*>(gws + enc_bwd_workspace(B).total);
    const uint8_t* blob = static_cast<const uint8_t*>(packed);
    const uint8_t* bblob = static_cast<const uint8_t*>(bwd_packed);
    // The decoder part as train_dec_plan lays it out (giga_dec_bwd_plan.h): the occupancy call first -- with many queries per scene
    // it WRITES the plane gradients (plane_gather_kernel: a gather over binned points instead of global atomics) and nothing needs
    // clearing -- then the grasp call, which adds its own with atomics.
    const TrainDecPlan plan = train_dec_plan(B, N, M, p_tsdf ? head_present : head_present & 7, detach_occ, bf16_dec);
    if (plan.clear_planes && hipMemsetAsync(gplanes, 0, gp_bytes, s) != hipSuccess) return -10;
    if (hipMemsetAsync(grads, 0, n_params * sizeof(float), s) != hipSuccess) return -10;
    int rc = 0;
    // work that waits for ONE launch of the caller's stream only goes to the device's side stream (giga_side.h; GIGA_WGRAD_STREAM=0: none)
    SideScope side(s, [] { const char* e = getenv("GIGA_WGRAD_STREAM"); return !e || atoi(e) != 0; }());
    const float* nhwc = static_cast<const float*>(planes_nhwc);
    DectPending pend{};
    struct { const DecBwdCall& c; long long base; const float* p; int mask, n; } calls[2] = {
        {plan.occ, plan.occ_base, p_tsdf, 8, M}, {plan.grasp, plan.grasp_base, p, head_present & 7, N}};
    for (const auto& k : calls) {
        if (!k.c.runs) continue;
        float* sc = scratch + k.base;
        float* gp = k.c.planes ? gplanes : nullptr;
        float* dcbuf = k.c.gather ? sc + k.c.dcbuf_off : nullptr;
        // fp32: the weight gradients go to the side stream (the occupancy call's may still be reading their rows while the grasp call
        // runs: the calls' scratch lies apart).  bf16: one fused launch, its partial tiles wait for the reduce below.
        if (bf16_dec) rc |= launch_dect_backward(k.c, nhwc, k.p, blob, bblob, k.mask, outs, douts, gp, dcbuf, sc, B, k.n, s, &pend);
        else rc |= launch_decoder_backward(k.c, nhwc, k.p, blob, bblob, k.mask, outs, douts, gp, dcbuf, grads, head_present, sc, B, k.n, s, &side);
        if (dcbuf && bf16_dec) rc |= launch_plane_gather(dcbuf, k.p, gplanes, B, k.n, s);   // (fp32: in front of its weight gradients)
    }
    // ONE reduce for every head of the bf16 step (on the caller's stream: moved to the side stream it delays the first weight gradients
    // there, 894 -> 899 us per step)
    if (plan.reduce) rc |= launch_dect_reduce(pend, grads, head_present, s);
    rc |= launch_encoder_backward(tsdf, blob, bblob, static_cast<const uint8_t*>(enc_workspace_fwd), gplanes, gws,
                                  grads, head_present, B, s, bf16_convs, convin_mask, side);
    return rc;
}

/* host only: what the decoder part of giga_backward would do for these arguments (giga_dec_bwd_plan.h) */
int giga_decoder_backward_plan(int B, int N, int M, int head_present, int32_t* plan_words) {
    static_assert(TRAIN_DEC_PLAN_WORDS == GIGA_DECODER_BACKWARD_PLAN_WORDS && DEC_BWD_CALL_WORDS == GIGA_DECODER_BACKWARD_CALL_WORDS &&
                  TRAIN_DEC_MAX_LAUNCHES == GIGA_DECODER_BACKWARD_MAX_LAUNCHES && sizeof(int) == sizeof(int32_t), "the plan's words are the header's");
    static_assert(DBK_DECODER_BWD == GIGA_DEC_BWD_KERNEL_DECODER_BWD && DBK_PLANE_GATHER == GIGA_DEC_BWD_KERNEL_PLANE_GATHER &&
                  DBK_LINEAR_WGRAD == GIGA_DEC_BWD_KERNEL_LINEAR_WGRAD && DBK_DECT == GIGA_DEC_BWD_KERNEL_DECT &&
                  DBK_DECT_REDUCE == GIGA_DEC_BWD_KERNEL_DECT_REDUCE, "the kernel ids are the header's");
    if (!plan_words) return -1;
    TrainDecPlan plan{};
    if (B > 0) {
        if (B > GIGA_MAX_SCENES) return -7;
        if (N < 0 || M < 0) return -1;
        plan = train_dec_plan(B, N, M, head_present & 15, (head_present & GIGA_DETACH_OCC) != 0, (head_present & GIGA_BF16_DECODER) != 0);
    }
    memcpy(plan_words, &plan, sizeof plan);
    return 0;
}

/* page-lock (and map for DMA) a host range the caller owns, e.g. a shared-memory batch ring written by reader processes */
int giga_host_register(void* ptr, size_t bytes) {
    if (!ptr || bytes == 0) return -1;
    return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? 0 : -10;
}
int giga_host_unregister(void* ptr) {
    if (!ptr) return -1;
    return hipHostUnregister(ptr) == hipSuccess ? 0 : -10;
}

}  // extern "C"
