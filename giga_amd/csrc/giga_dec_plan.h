// The launch policy of the decoder forward (giga_decoder.hip::launch_decoder), host only: which kernel and instantiation a launch of
// (precision, B, N, R, nheads) gets, its grid, block and LDS size, and the launch-dependent fields of DecArgs.  launch_decoder
// launches exactly what dec_plan returns, and giga_decoder_plan (C ABI) returns the same plan to a caller that only asks: the tests
// read the policy from here.  No HIP in this header: it compiles with a plain C++ compiler.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <initializer_list>

#include "giga_layout.h"

namespace giga {

// ---- LDS sizes of the decoder kernels ------------------------------------------------------------------------------------------
constexpr size_t DEC32_LDS = DEC32_BYTES + 4 * 32 * 96 * sizeof(float);     // weight image + the gather's per-wave stage
static_assert(DEC32_LDS <= 160 * 1024, "LDS budget of the fp32 decoder");
constexpr size_t DEC32_TILE_LDS = 4 * 32 * 96 * sizeof(float) + NBLK * 4 * 64 * 16 + 46 * FRAG;   // 4 gather stages, FC exchange (float4), chain fragments
constexpr size_t DEC32_POINT_LDS = 46 * FRAG + (4 * 96 + NBLK * 32 + 32) * sizeof(float);   // chain fragments, 4 gather stages, FC exchange, GEMV input
// Up to this many points the point kernel is the default.  HIP-event medians of seven, mask 7, point / tile kernel
// (profiles/dec_point/sweep.txt): P = 32 7.2 / 16.1 us, 256 9.7 / 16.1, 384 13.5 / 16.1, 512 15.0 / 16.2, 768 20.0 / 16.3: the curves
// cross between 512 and 768; the bound sits at the last size with a margin well outside the run-to-run spread.
constexpr int DEC32_POINT_MAX_P = 256;
// decoder_lat_kernel
constexpr int LAT_ROWS = 2 * NBLK + 1;     // line rows: G_xz[0..4], G_xy[0..4], and the bias of the last fc_1 as G_xy[5]
constexpr int LAT_MAX_R = 40;
template <bool SPLIT, bool DBUF>
constexpr size_t lat_lds_bytes(int R) {
    return (size_t)(32 * (SPLIT ? 2 : 1) + 1) * FRAG + (size_t)(DBUF ? 2 : 1) * LAT_ROWS * (R / 4) * 32 * 16 + 16;
}

// ---- knobs ---------------------------------------------------------------------------------------------------------------------
// The decoder's four environment knobs, read on every call (A/B runs and cross-checks in one process); this is the only place
// that reads them.
//   GIGA_DEC_LAT=0 / 1         forces decoder_lat_kernel off / on where it can run (f16-class lattice launches, R % 8 == 0, R <= 40)
//   GIGA_DEC16_RESIDENT=0 / 1  forces the head-resident kernel off / on for plain f16
//   GIGA_DEC32_TILE=0          neither one-query kernel: decoder_f32_kernel, the general kernel
//   GIGA_DEC32_POINT=0         no point kernel: the tile kernel where its own rule holds
//   GIGA_DEC32_POINT=n         n > 1: the point kernel up to n points instead of DEC32_POINT_MAX_P (sweeps; at most the tile rule's 3072)
// Anything else for GIGA_DEC32_POINT (unset, 1, negative, not a number) leaves the default bound.
struct DecKnobs {
    int dec_lat = -1;                        // -1: the policy decides
    int dec16_resident = -1;                 // -1: the policy decides
    bool dec32_tile = true;                  // the one-query kernels may run
    int dec32_point = DEC32_POINT_MAX_P;     // the point kernel's bound in points (0: never)
};
inline DecKnobs dec_knobs_from_env() {
    DecKnobs k;
    if (const char* e = getenv("GIGA_DEC_LAT")) k.dec_lat = atoi(e);
    if (const char* e = getenv("GIGA_DEC16_RESIDENT")) k.dec16_resident = atoi(e);
    if (const char* e = getenv("GIGA_DEC32_TILE")) k.dec32_tile = atoi(e) != 0;
    if (const char* e = getenv("GIGA_DEC32_POINT")) {
        const int v = atoi(e);
        if (v == 0 && e[0] == '0') k.dec32_point = 0;
        else if (v > 1) k.dec32_point = v < 3072 ? v : 3072;
    }
    return k;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------
enum DecKernel {
    DEC_K_NONE = 0,          // nothing to launch (no points or no heads)
    DEC_K_F16 = 1,           // decoder_f16_kernel<T, LATTICE, NW>: shared features, double-buffered head images
    DEC_K_F16S = 2,          // decoder_f16s_kernel<T, LATTICE, NW, SPLIT>: head-resident
    DEC_K_LAT = 3,           // decoder_lat_kernel<SPLIT, NW, DBUF>: separable fc_c on the lattice
    DEC_K_F32 = 4,           // decoder_f32_kernel<T, LATTICE>: the general exact kernel
    DEC_K_F32_TILE = 5,      // decoder_f32_tile_kernel: one query per scene, one tile and head per workgroup
    DEC_K_F32_POINT = 6,     // decoder_f32_point_kernel: one query per scene, one point and head per workgroup
};
// The fields in the order giga_decoder_plan writes them (include/giga_hip.h: GIGA_DECODER_PLAN_WORDS).  LATTICE of an
// instantiation is R > 0.
struct DecPlan {
    int kernel;              // DecKernel
    int T;                   // 32-point tiles per wave and round (1 where the kernel has no such parameter)
    int NW;                  // waves per workgroup
    int split;               // operand form: 1 = [hi, lo] f16 pairs (f16x3), 0 = single operands
    int dbuf;                // decoder_lat_kernel: two line buffers
    int grid_x, grid_y, block;
    int lds;                 // dynamic LDS bytes
    int nbatch, heads_per_wg, lat_parts;     // DecArgs fields of the same names (0: the kernel does not read it)
    int slots;               // head-resident kernels: workgroups per head (grid_x = slots * nheads)
    int xcd_remap;           // head-resident kernels: the XCD-contiguous (head, slot) map applies
};
constexpr int DEC_PLAN_WORDS = sizeof(DecPlan) / sizeof(int);

// All of the decision arithmetic of a decoder launch, and nothing else.  precision 0 fp32, 1 f16, 2 f16x3; R > 0: a lattice launch
// (N = R^3 on lattice-resampled planes).
inline DecPlan dec_plan(int precision, int B, int N, int R, int nheads, const DecKnobs& knobs) {
    DecPlan p{};
    const long long P = (long long)B * N;
    if (P <= 0 || nheads <= 0) return p;
    const long long tiles = (P + 31) / 32;
    const bool lat = R > 0;
    p.T = 1;
    p.grid_y = 1;
    // the head-resident kernels map workgroup -> (head, slot); with a grid that is a multiple of 8 * nheads the slots of one XCD are
    // made contiguous (dec16_head_slot)
    auto resident_grid = [&](int slots) {
        p.slots = slots;
        p.nbatch = slots;
        p.grid_x = slots * nheads;
        p.xcd_remap = p.grid_x % (8 * nheads) == 0;
    };
    // Lattice launches of the f16-class modes with R % 8 == 0 (the inference lattice: R = 40): the separable-fc_c kernel
    // (decoder_lat_kernel) -- f16x3 always (1 scene 31.8 -> 27.8 us, 32 scenes 0.754 -> 0.583 ms), plain f16 from 4 scenes up (32 scenes
    // 0.279 -> 0.260 ms; a single scene is latency-bound and 1 us faster on the head-resident kernel below, which also serves other
    // lattices).
    if (lat && (precision == 1 || precision == 2) && R <= LAT_MAX_R && R % 8 == 0 &&
        (knobs.dec_lat >= 0 ? knobs.dec_lat != 0 : (precision == 2 || B >= 4))) {
        const int cap = 256 / nheads, cap8 = 256 / (8 * nheads) * 8;
        // small launches: hand a slab out in parts (NP divides the tile count), so that a single scene still covers the chip; a
        // part costs its tiles plus one line phase (~ the time of 12 tiles on a workgroup)
        const int ntile = (R / 4) * (R / 8);
        int np = 1;
        double best = 1e30;
        for (int c : {1, 2, 5}) {
            if (ntile % c) continue;
            const long long units = (long long)B * R * c;
            const long long rounds = (units + cap - 1) / cap;
            const double cost = (double)rounds * ((double)ntile / c + 12.0);
            if (cost < best - 1e-9) { best = cost; np = c; }
        }
        p.lat_parts = np;
        const int nslab = B * R * np;
        resident_grid(nslab < cap ? nslab : (nslab >= 2 * cap8 && cap8 > 0 ? cap8 : cap));
        p.kernel = DEC_K_LAT;
        // 16 waves per workgroup, four per SIMD (against 12: 0.267 -> 0.257 ms at 32 scenes).  Two line buffers fit beside the
        // 33-KiB image of the plain mode, not beside the 65 KiB of f16x3.
        p.NW = 16;
        p.split = precision == 2;
        p.dbuf = precision != 2;
        p.lds = (int)(precision == 2 ? lat_lds_bytes<true, false>(R) : lat_lds_bytes<false, true>(R));
        p.block = p.NW * 64;
        return p;
    }
    // Head-resident kernel: always for the f16x3 split mode; for plain f16 when the launch is small (the shared-feature
    // kernel below walks rounds of NW*T tiles per workgroup with all heads on the same CU: a single scene's 2000 tiles then
    // keep only 84 CUs busy: 31.6 -> 16.3 us for the three grasp heads of one scene's 64 000 lattice points; from ~8 scenes
    // up the shared-feature kernel is the faster one, 297 vs 323 us at 32 scenes).  grid = slots x nheads <= 256 (one workgroup per
    // CU).  Two tiles per wave (the weight fragments are read from LDS once per two tiles) when every workgroup gets at least two
    // such rounds, else one tile per wave.  (measurements in DESIGN.md)
    const bool resident = precision == 2 ||
                          (precision == 1 && (knobs.dec16_resident >= 0 ? knobs.dec16_resident != 0 : tiles * nheads < (lat ? 16000 : 6000)));
    if (resident) {
        const int cap = 256 / nheads;                          // one workgroup per CU
        const int cap8 = 256 / (8 * nheads) * 8;               // ... or a multiple of 8 slots: XCD-contiguous ranges (L2 locality)
        const bool two = tiles >= 2LL * cap * 8 * 2;
        p.kernel = DEC_K_F16S;
        p.split = precision == 2;
        p.T = two ? 2 : 1;
        // plain f16: 112-142 VGPRs with one tile per wave (12 waves), 2 tiles need the 256-register budget (8 waves)
        p.NW = precision == 2 || two ? 8 : 12;
        p.lds = (int)(precision == 2 ? DEC16S_BYTES : DEC16_BYTES);
        const int per_round = p.NW * p.T;
        int slots = (int)((tiles + per_round - 1) / per_round);
        // large launches trade the last few CUs for L2 locality; small ones (a single scene: 2000 tiles) are latency-bound and
        // take every CU -- 240 instead of 255 workgroups would add a third, nearly empty round
        if (slots > cap) slots = tiles >= 8LL * cap * per_round ? cap8 : cap;
        else if (slots >= 8 && tiles >= 8LL * slots) slots &= ~7;
        resident_grid(slots);
    } else if (precision == 1) {
        // shared-feature kernel, one persistent workgroup per CU.  Lattice variant: 155 VGPRs -> 12 waves (3 per SIMD, phases
        // 0/1/2 over the heads); else 8 waves
        p.kernel = DEC_K_F16;
        p.T = 2;
        p.NW = lat ? 12 : 8;
        p.nbatch = (int)((tiles + p.NW * p.T - 1) / (p.NW * p.T));
        p.grid_x = p.nbatch < 256 ? p.nbatch : 256;
        p.lds = (int)(2 * DEC16_BYTES);
    } else if (!lat && N == 1 && knobs.dec32_tile && P <= knobs.dec32_point) {
        // ONE query per scene (train_giga's literal call): one point and head per workgroup, GEMVs on the VALU (no padded MFMA
        // tile).  DEC32_POINT_MAX_P comes from the sweep against the tile kernel below (profiles/dec_point/sweep.txt).
        // (Only for N == 1, like the tile kernel below and for the same reason.)
        p.kernel = DEC_K_F32_POINT;
        p.NW = 4;
        p.grid_x = (int)P;
        p.grid_y = nheads;
        p.lds = (int)DEC32_POINT_LDS;
    } else if (!lat && N == 1 && tiles * nheads <= 96 && knobs.dec32_tile) {
        // ONE query per scene (train_giga's literal call) and few scenes: one tile and head per workgroup, four waves per chain.
        // (Only for N == 1: the kernel sums the stream in a different order than decoder_f32_kernel, and callers that split a
        // query set into chunks -- Generator3D.eval_points -- rely on a point's result not depending on the chunk it is in.)
        p.kernel = DEC_K_F32_TILE;
        p.NW = 4;
        p.grid_x = (int)tiles;
        p.grid_y = nheads;
        p.lds = (int)DEC32_TILE_LDS;
    } else {
        // the general exact kernel.  Enough work for two tiles per wave on every CU: the 111 KiB weight image is staged half as
        // often.  Else one tile, and when the point batches cannot fill the chip every head gets its own workgroups.
        p.kernel = DEC_K_F32;
        p.NW = 4;
        p.T = tiles >= 2 * 4 * 256 ? 2 : 1;
        p.nbatch = (int)((tiles + 4 * p.T - 1) / (4 * p.T));
        p.grid_x = p.nbatch < 256 ? p.nbatch : 256;
        const bool per_head = p.T == 1 && p.grid_x * nheads <= 256;
        p.heads_per_wg = per_head ? 1 : nheads;
        p.grid_y = per_head ? nheads : 1;
        p.lds = (int)DEC32_LDS;
    }
    p.block = p.NW * 64;
    return p;
}

}  // namespace giga
