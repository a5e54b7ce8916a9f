// The launch and memory policy of the encoder forward (giga_encoder.hip::launch_encoder), host only: how the `precision` word of a
// call is taken apart, which two environment knobs it reads, where every activation lies in the caller's workspace, and what a call of
// (precision word, B scenes) on a device of `cus` compute units launches -- conv_in's instantiation and grid, plane_finalize's grid,
// the form of the U-Net (one launch per layer or one persistent launch; conv16, conv32 or Winograd stages; fused pairs), the kernel
// family of every layer, the number of launches and the GIGA_PATH_* word.  launch_encoder launches exactly what enc_plan returns,
// giga_encoder_workspace_bytes / _layout read enc_workspace, and giga_encoder_plan (C ABI) returns the same plan to a caller that
// only asks: the tests read the policy from here.  No HIP in this header: it compiles with a plain C++ compiler.
// Not here, because they are not policy: the LDS sizes (fixed per instantiation: constexpr functions beside the kernels, with their
// static_asserts) and the grids of the per-layer launchers launch_conv, launch_conv32, launch_wino and launch_up (template arithmetic
// of those launchers over the layer's shape and a.nimg; giga_conv16.h, giga_conv32.h, giga_wino.h).
#pragma once
#include <cstddef>
#include <cstdlib>

#include "../../include/giga_hip.h"
#include "giga_conv32_geom.h"
#include "giga_layout.h"

namespace giga {

// ---- constants of the launches -------------------------------------------------------------------------------------------------
constexpr int CONV_NW = 12;       // conv16: waves per workgroup (3 per SIMD; VGPR use is < 80)
constexpr int MEGA_NW = CONV_NW;  // waves per workgroup of the persistent conv16 kernel
constexpr int WINO_NW = 8;        // Winograd stages: two waves per SIMD, 256 registers each (64 accumulators + 32 transformed
                                  // values + a prefetched chunk do not fit the 168 of three per SIMD)
constexpr int CI_NW = 8;          // conv_in: 8 waves x 5 slices.  (4 waves x 10 slices -- one wave per SIMD, half the yz partials -- measured
                                  // slower for the fp32 path, 50.5 vs 47.3 us at 32 scenes: the second wave of a SIMD hides the
                                  // slice-boundary and LDS-issue bubbles.)
// layers that run as Winograd by default (bit l = U-Net layer l of giga_layout.h::kConv); settled by measurement
constexpr unsigned WINO_DEFAULT_MASK = 0xFFF;     // all ten 3x3 layers (0, 1, 2, 3, 4, 5, 7, 8, 10, 11) as Winograd, the two ConvTranspose layers
                                                  // (6, 9) as plain GEMMs on the same lane layout (up_run); profiles/r06/wino_ab_*.txt
// Groups of the persistent U-Net launches (giga_encoder.hip) and of conv32's per-layer launches: 8 workgroups on one XCD each
constexpr int MEGA_GROUP = 8;                     // workgroups per group
constexpr int MEGA_SLOTS = 4;                     // group slots per XCD at most: 8 x 4 x 8 = 256 workgroups, one per CU
inline int mega_groups(int nimg) {                // groups of a launch: 8 (one per XCD) per slot, a slot per 8 images
    const int slots = (nimg + 7) / 8 < MEGA_SLOTS ? (nimg + 7) / 8 : MEGA_SLOTS;
    return 8 * slots;
}
// words of MegaArgs::sync, carved below: the barrier words of the persistent U-Net kernels, 8 per-XCD + 32 per-group counters, 128 B apart
constexpr int MEGA_SYNC_WORDS = (8 + 32) * 32;
// x-parts of conv_in+project: 1 (8*B workgroups, five slices per wave) from 32 scenes up, else 5 (40*B workgroups)
constexpr int ENC_NXP_ONE_FROM_SCENES = 32;
inline int enc_nxp(int B) { return B >= ENC_NXP_ONE_FROM_SCENES ? 1 : 5; }
// The persistent form assumes that every XCD receives an eighth of the grid: a whole MI355X, 8 XCDs x 32 CUs, one workgroup per CU
constexpr int ENC_FULL_DEVICE_CUS = 256;
// ... and is the default from this many images (8 scenes) up in fp32 / bf16: below that an fp32 layer's barrier + first patch cost
// what its launch costs (152 vs 156 us at one scene).  The f16-class modes take it at every batch size.
constexpr int ENC_PERSIST_MIN_IMAGES = 24;
// conv32 (giga_conv32.h) or conv16 for the f16-class modes: left alone, conv32 runs up to 16 scenes (48 images) and conv16 beyond:
// conv32's encoder is 3-9 % faster up to 32 scenes, but from ~24 scenes on -- every CU busy -- the chip holds a 3-5 % lower shader
// clock while and after the conv32 launch runs (at LOWER socket power: a current limit), which costs a sustained 32-scene step up to
// 4 % and a 128-scene step up to 6 % (tools/gpu_sustained_power.py, profiles/r04/final/sustained_power.txt).
constexpr int C32_AUTO_MAX_IMAGES = 48;
// Fused same-resolution pairs (C32Pair) while a member's rows fit ONE sub-band of the pair: up to this many images per group (the halo
// rows a member recomputes are 2 of ~12; beyond that the pair needs smaller sub-bands than the single layers and measured slower,
// profiles/r04/conv32_fused_pairs.txt).  Bit-identical either way.
constexpr int C32_FUSE_MAX_IMAGES_PER_GROUP = 2;
// probe stages (giga_encoder_forward_probe): 0 conv_in, 1 plane_finalize, 2..14 U-Net layers 0..12, 15 the whole U-Net.  A probed
// layer needs its own launch.
constexpr int ENC_STAGE_LAYER0 = 2, ENC_STAGE_UNET = 15;

// ---- the workspace -------------------------------------------------------------------------------------------------------------
// Byte offsets of the encoder's activations inside its caller-allocated workspace (all NHWC, the precision's element type):
//   P0 planes_in [3B,40,40,32] | A0 | S0 (skip 0) | Q0 [3B,20,20,32] | A1 [..,20,20,64] | S1 | Q1 [..,10,10,64]
//   | A2 [..,10,10,128] | S2 | U0 [..,20,20,64] | A3 | A4 | U1 [..,40,40,32] | A5 | A6 | YZ partials fp32 | SYNC | MASK
struct EncWs {
    size_t P0, A0, S0, Q0, A1, S1, Q1, A2, S2, U0, A3, A4, U1, A5, A6, YZ, XZ, total;   // XZ unused (kept for the ABI)
    size_t SYNC;               // barrier counter + timeout flag of the persistent U-Net kernel
    size_t MASK;               // conv_in ReLU mask of a training forward (GIGA_CONVIN_MASK): [B][8][40][64 lanes] x 16 bytes
};
inline EncWs enc_workspace(int B, int precision) {
    const size_t es = precision == 1 ? 2 : 4;
    const size_t n = 3 * (size_t)B;
    EncWs w{};
    size_t at = 0;
    auto take = [&](size_t elems, size_t esz) { size_t o = at; at += align_up(elems * esz, 256); return o; };
    auto in = [&](int l) { return take(n * conv_in_elems(l), es); };        // layer l's input, output, pooled output (kConv)
    auto out = [&](int l) { return take(n * conv_out_elems(l), es); };
    auto pool = [&](int l) { return take(n * conv_pool_elems(l), es); };
    w.P0 = in(0);   w.A0 = out(0);  w.S0 = out(1);
    w.Q0 = pool(1); w.A1 = out(2);  w.S1 = out(3);
    w.Q1 = pool(3); w.A2 = out(4);  w.S2 = out(5);
    w.U0 = out(6);  w.A3 = out(7);  w.A4 = out(8);
    w.U1 = out(9);  w.A5 = out(10); w.A6 = out(11);
    // conv_in's partials and its mask are not U-Net tensors: their sizes are conv_in's (40^2 pixels x 32 channels per scene, not per image)
    w.YZ = take((size_t)(4 + enc_nxp(B)) * B * 1600 * 32, 4);   // 4 xz partials (iy-groups) + NXP yz partials (x-parts)
    w.XZ = w.YZ;
    w.SYNC = take(MEGA_SYNC_WORDS * 4, 4); // barrier counters of the persistent U-Net kernel (8 per-XCD + 32 per-group, 128 B apart)
    w.MASK = take((size_t)B * 8 * RES * 64 * 4, 4);   // conv_in ReLU mask (training forward with GIGA_CONVIN_MASK; 10 MB at 32 scenes)
    w.total = at;
    return w;
}

// ---- the call ------------------------------------------------------------------------------------------------------------------
// every per-call flag OR-ed into `precision` of giga_encoder_forward* (include/giga_hip.h); what is left is the precision 0..3
constexpr int GIGA_ENCODER_FLAGS = GIGA_FOLD_FINAL | GIGA_PERSIST_UNET | GIGA_LAYERWISE_UNET | GIGA_CONV32_UNET | GIGA_CONV16_UNET |
                                   GIGA_CONVIN_MASK | GIGA_DIRECT_CONV;
struct EncCall {
    int precision;           // 0 fp32, 1 f16, 2 f16x3, 3 bf16 (the training forward); anything else: the C ABI answers -5
    int fold_final;          // the caller's decoder carries conv_final inside its fc_c weights: the last layer is not launched
    int persist;             // -1 one launch per layer, 0 the policy decides, 1 the persistent launch
    int conv32;              // 1 conv32, -1 conv16, 0 the policy decides (precisions 1..3; precision 0 has conv16 only)
    int convin_mask;         // training forward (precisions 0 and 3): conv_in keeps its ReLU mask for the backward
    int direct_conv;         // precision 0: no Winograd stages in this call
};
// The only decoder of the word.  GIGA_LAYERWISE_UNET beats GIGA_PERSIST_UNET, GIGA_CONV32_UNET beats GIGA_CONV16_UNET.
inline EncCall enc_call_from_flags(int precision_word) {
    EncCall c{};
    c.precision = precision_word & ~GIGA_ENCODER_FLAGS;
    c.fold_final = (precision_word & GIGA_FOLD_FINAL) != 0;
    c.persist = (precision_word & GIGA_LAYERWISE_UNET) ? -1 : (precision_word & GIGA_PERSIST_UNET) ? 1 : 0;
    c.conv32 = (precision_word & GIGA_CONV32_UNET) ? 1 : (precision_word & GIGA_CONV16_UNET) ? -1 : 0;
    c.convin_mask = (precision_word & GIGA_CONVIN_MASK) != 0;
    c.direct_conv = (precision_word & GIGA_DIRECT_CONV) != 0;
    return c;
}

// ---- knobs ---------------------------------------------------------------------------------------------------------------------
// The encoder forward's two environment knobs, read on every call (A/B runs and cross-checks in one process); this is the only place
// that reads them.
//   GIGA_WINOGRAD=<mask>   the layers of precision 0 that run as Winograd stages (strtoul base 0: 0x3, 3, 0 = none); unset: WINO_DEFAULT_MASK.
//                          (A blob rebuilt on the device needs giga_derive_winograd before such a forward.)
//   GIGA_C32_FUSE=0 / 1    forces the fused-pairs form of the persistent conv32 launch off / on; unset (or negative): the rule decides
struct EncKnobs {
    unsigned winograd = WINO_DEFAULT_MASK;
    int c32_fuse = -1;                       // < 0: the policy decides
};
inline EncKnobs enc_knobs_from_env() {
    EncKnobs k;
    if (const char* e = getenv("GIGA_WINOGRAD")) k.winograd = (unsigned)strtoul(e, nullptr, 0);
    if (const char* e = getenv("GIGA_C32_FUSE")) k.c32_fuse = atoi(e);
    return k;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------
enum EncForm {
    ENC_FORM_NONE = 0,               // nothing is launched (no scenes)
    ENC_FORM_LAYERS_CONV16 = 1,      // one launch per layer: conv16_kernel, and in exact fp32 wino_kernel / up_kernel where wino_mask says
    ENC_FORM_LAYERS_CONV32 = 2,      // one launch per layer: conv32_kernel
    ENC_FORM_PERSIST_CONV16 = 3,     // unet_mega_kernel<T, MATH, false>
    ENC_FORM_PERSIST_WINO = 4,       // unet_mega_kernel<float, MATH_NATIVE, true>: Winograd stages where wino_mask says
    ENC_FORM_PERSIST_CONV32 = 5,     // unet32_mega_kernel<MODE, fused>
};
enum EncLayerKernel {                // the kernel family of a layer (its own launch, or its stage of the persistent kernel)
    ENC_LAYER_NONE = 0,              // not launched (conv_final of a folded call)
    ENC_LAYER_CONV16 = 1,            // conv16_kernel / conv16_run
    ENC_LAYER_CONV32 = 2,            // conv32_kernel / c32_run
    ENC_LAYER_WINO = 3,              // wino_kernel / wino_run
    ENC_LAYER_UP = 4,                // up_kernel / up_run: a ConvTranspose as plain GEMMs on the Winograd lane layout
};
// The fields in the order giga_encoder_plan writes them (include/giga_hip.h: GIGA_ENCODER_PLAN_WORDS).
struct EncPlan {
    int nimg;                // plane images, 3 B
    int nlayers;             // 12 (conv_final folded into the decoder) or 13
    // conv_in: convin_project_kernel<T, ci_sxw, ci_f16, ci_nw, ci_lo, ci_mask>
    int nxp;                 // x-parts (5: every wave walks one slice; 1: five)
    int ci_f16;              // the f16 operand image (convin_ws) and the f16 MFMA; 0: fp32 operands and MFMA
    int ci_lo;               // ... with f16x3 split operands; 0: hi only (plain f16)
    int ci_mask;             // stores the ReLU mask
    int ci_sxw, ci_nw;       // slices per wave, waves per workgroup
    int ci_grid_x, ci_grid_y, ci_grid_z, ci_block;
    // plane_finalize_kernel<T>
    int fin_grid, fin_block;
    // the U-Net
    int form;                // EncForm
    int persistent, conv32, fused;
    unsigned wino_mask;      // bit l: layer l runs as a Winograd stage / an up-GEMM (precision 0 only; CONV3 / UPCONV layers of kConv only)
    int groups;              // mega_groups(nimg): groups of 8 workgroups of the persistent launch (and of conv32's per-layer launches)
    int grid, block;         // the persistent launch (0: one launch per layer)
    int layer_kernel[NCONV]; // EncLayerKernel
    int launches;            // kernel launches of the call
    int path;                // GIGA_PATH_*: what giga_encoder_last_path() reports after the call
};
constexpr int ENC_PLAN_WORDS = sizeof(EncPlan) / sizeof(int);

// All of the decision arithmetic of an encoder call, and nothing else.  cus: compute units of the device the call runs on;
// probe_stage: the stage a probe brackets (-1: none); slot_free: the device has room for one more persistent launch (the launcher
// asks persistent_slot, which reserves one, only when the plan wants it, and plans again with `false` when the answer is no).
inline EncPlan enc_plan(const EncCall& c, int B, int cus, int probe_stage, bool slot_free, const EncKnobs& knobs) {
    EncPlan p{};
    if (B <= 0) return p;
    const bool f16class = c.precision == 1 || c.precision == 2;
    p.nimg = 3 * B;
    p.nlayers = c.fold_final ? NCONV - 1 : NCONV;
    // conv_in arithmetic: fp32 MFMA (precision 0), the f16 MFMA with hi only (plain f16) or with f16x3 split operands (precision 2).
    // The bf16 training forward: PLAIN f16 operands when it also stores the ReLU mask for the backward (GIGA_CONVIN_MASK: the backward
    // then uses the forward's own decisions; f16's 11 bits are finer than the bf16 rounding the next layer applies to this kernel's
    // output; -17 us per step against the split form), else the f16x3 form -- fp32-grade (<= 1e-5 of the fp32 kernel), so that a
    // backward that RECOMPUTES the mask in fp32 agrees with it.
    p.nxp = enc_nxp(B);
    p.ci_mask = c.convin_mask && (c.precision == 0 || c.precision == 3);
    p.ci_f16 = c.precision != 0;
    p.ci_lo = c.precision == 2 || (c.precision == 3 && !p.ci_mask);
    p.ci_nw = CI_NW;
    p.ci_sxw = (p.nxp == 1 ? RES : 8) / CI_NW;
    p.ci_grid_x = p.nxp == 1 ? 8 * B : 5;
    p.ci_grid_y = p.nxp == 1 ? 1 : 8;
    p.ci_grid_z = p.nxp == 1 ? 1 : B;
    p.ci_block = CI_NW * 64;
    p.fin_grid = (int)(((size_t)B * RES * RES * CD / 4 + 255) / 256);
    p.fin_block = 256;
    // exact fp32 only: the stride-1 3x3 layers whose bit is set run as Winograd F(2x2, 3x3) (giga_wino.h) on their own weight image,
    // the ConvTranspose layers as up-GEMMs; on unless the call says GIGA_DIRECT_CONV
    if (c.precision == 0 && !c.direct_conv)
        for (int l = 0; l < NCONV; ++l)
            if ((kConv[l].kind == CONV3 || kConv[l].kind == UPCONV) && (knobs.winograd >> l & 1u)) p.wino_mask |= 1u << l;
    // One persistent launch for the whole U-Net is the default, unless a single layer is being probed -- for every batch size in the
    // f16-class modes, from ENC_PERSIST_MIN_IMAGES up in fp32 / bf16.  GIGA_LAYERWISE_UNET keeps one launch per layer;
    // GIGA_PERSIST_UNET forces the persistent form where the default would not take it.  At most MEGA_MAX_IN_FLIGHT of them are in
    // flight per device (slot_free; giga_encoder.hip::persistent_slot).
    const bool probe_layer = probe_stage >= ENC_STAGE_LAYER0 && probe_stage < ENC_STAGE_LAYER0 + NCONV;
    const bool by_default = f16class || p.nimg >= ENC_PERSIST_MIN_IMAGES;
    p.persistent = cus == ENC_FULL_DEVICE_CUS && !probe_layer && (c.persist > 0 || (c.persist == 0 && by_default)) && slot_free;
    // conv32 or conv16: a call (GIGA_CONV32_UNET / GIGA_CONV16_UNET) can force one
    p.conv32 = c.precision != 0 && (c.conv32 != 0 ? c.conv32 > 0 : p.nimg <= C32_AUTO_MAX_IMAGES);
    p.groups = mega_groups(p.nimg);
    p.fused = p.persistent && p.conv32 &&
              (knobs.c32_fuse >= 0 ? knobs.c32_fuse != 0 : (p.nimg + p.groups - 1) / p.groups <= C32_FUSE_MAX_IMAGES_PER_GROUP);
    p.form = p.conv32 ? (p.persistent ? ENC_FORM_PERSIST_CONV32 : ENC_FORM_LAYERS_CONV32)
                      : !p.persistent ? ENC_FORM_LAYERS_CONV16 : p.wino_mask ? ENC_FORM_PERSIST_WINO : ENC_FORM_PERSIST_CONV16;
    if (p.persistent) {
        p.grid = p.groups * MEGA_GROUP;
        p.block = 64 * (p.conv32 ? C32_NW : p.wino_mask ? WINO_NW : MEGA_NW);
    }
    for (int l = 0; l < p.nlayers; ++l)
        p.layer_kernel[l] = p.conv32 ? ENC_LAYER_CONV32
                          : !(p.wino_mask >> l & 1u) ? ENC_LAYER_CONV16 : kConv[l].kind == CONV3 ? ENC_LAYER_WINO : ENC_LAYER_UP;
    p.launches = 2 + (p.persistent ? 1 : p.nlayers);
    p.path = p.conv32 ? GIGA_PATH_CONV32 | (p.persistent ? GIGA_PATH_PERSISTENT : 0) | (p.fused ? GIGA_PATH_FUSED_PAIRS : 0)
                      : (p.persistent ? GIGA_PATH_PERSISTENT : 0) | (p.wino_mask ? GIGA_PATH_WINOGRAD : 0);
    return p;
}

}  // namespace giga
