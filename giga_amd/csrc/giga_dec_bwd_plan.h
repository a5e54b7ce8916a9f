// The launch and memory policy of the training decoder's backward (giga_decoder_bwd.hip: fp32; giga_decoder_train16.hip: bf16), host
// only: what one backward call of (precision, B, N, nheads) launches -- grids, blocks, LDS sizes, the split of the weight-gradient
// launch -- where every region of its scratch lies, and how the calls of one training step share the step's scratch, which of them
// runs first and what the decoder part of giga_backward enqueues, in order.  The launchers launch exactly what their DecBwdCall
// says, giga_backward and giga_backward_workspace_bytes read train_dec_plan, and giga_decoder_backward_plan (C ABI) returns the
// same plan to a caller that only asks: the tests read the policy from here.  No HIP in this header: it compiles with a plain C++
// compiler.
#pragma once
#include <cstddef>
#include <initializer_list>

#include "giga_layout.h"

namespace giga {

// ---- fp32 path (giga_decoder_bwd.hip) ------------------------------------------------------------------------------------------
// per-head row arrays of decoder_bwd_kernel, each [P][32] fp32 (row = point, D-layout feature order restored to 0..31)
//   0..5 DN[i]   6..10 DH[i]   11..15 XN[i]   16..20 XH[i]   21 XO   22 DO (cols >= out_dim zero)
// shared by the heads of a call: C [P][96], PP [P][32] (cols 0..2 = p, rest zero), dc rows [P][96] (plane_gather_kernel's input)
constexpr int DB_NARR = 23;
constexpr size_t DEC_BWD_LDS = DEC32_BYTES > DECB_BYTES ? DEC32_BYTES : DECB_BYTES;      // the forward image, then the transposed one
// plane_gather_kernel
constexpr int PS_NW = 16;                                   // waves per workgroup
constexpr int PS_MAXN = 4096;                               // points per scene this path takes (LDS: 6 + 16 bytes per point)
constexpr int PS_MINN = 256;                                // ... and the fewest: below, the atomics are the faster route
constexpr int PS_CELLS = RES * RES;
constexpr size_t PS_LDS = (size_t)(2 * PS_CELLS + 64) * 4 + (size_t)PS_MAXN * (6 + 16);
// linear_wgrad_kernel: 17 problems dW = dY^T X per head (fc_out, 5 x (fc_1, fc_0, fc_c), fc_p) in 27 column blocks of 32 (fc_c: 3)
constexpr int LIN_PER_HEAD = 17;
constexpr int LIN_NB_PER_HEAD = 27;
constexpr int LIN_MAX = 52;                                 // up to three heads in one launch (the argument struct stays under the 4-KiB kernarg limit)
constexpr int LIN_BLOCKS = 2048;                            // workgroups a launch aims at: the points are split to reach it

// ---- bf16 path (giga_decoder_train16.hip) --------------------------------------------------------------------------------------
constexpr int DECT_FWD_FRAGS = DEC16_FRAGS;                            // 58
constexpr size_t DECT_FWD_BYTES = DEC16_BYTES;                         // 59 KiB
constexpr int DECT_BWD_FRAGS = NBLK * 10;                              // 50
constexpr size_t DECT_BWD_BYTES = (size_t)(DECT_BWD_FRAGS + 1) * FRAG; // 51 KiB
// gradient tiles of a head: tile id 6 b + t: t = 0..2 fc_c[b] columns 32 t .. 32 t + 31, 3 bias tile of block b, 4 fc_1[b], 5 fc_0[b]; 30 fc_out.
// bias tile columns: 0..2 dY x p_hi, 3 colsum(DN[b]), 4..6 dY x p_lo, 8 colsum(DH[b]), 9 colsum(DN[5]) (b = 4), 10 colsum(dO) (b = 4)
constexpr int DECT_NTILES = 6 * NBLK + 1;                       // 31
constexpr int DECT_TILE_FLOATS = 1024;
// LDS layout of dect_kernel:
// [zone: per wave 2 x (XH, DH, XN) step buffers + 3 DN slots = 9 tiles; the forward image overlays it while the forward chain runs]
// [per wave: C tiles (3), aux tile [8 columns][32 points], dO tile [4][32]] [backward image]
constexpr int TILE_B = 2048;
constexpr int ZONE_WAVE = 9 * TILE_B;                           // 18432
constexpr int ZONE_B = 4 * ZONE_WAVE;                           // 73728 >= DECT_FWD_BYTES
constexpr int CW_B = 3 * TILE_B + 512 + 256;                    // 6912
constexpr int LDS_FWD = ZONE_B + 4 * CW_B;                      // 101376: end of the backward's per-wave regions
constexpr int LDS_BWD = LDS_FWD + (int)DECT_BWD_BYTES;          // 153600
constexpr int FWD_NW = 8;
constexpr int LDS_FWD8 = ZONE_B + FWD_NW * CW_B;                // 129024: forward kernel (image in the zone + 8 waves' C tiles)
static_assert(ZONE_B >= (int)DECT_FWD_BYTES && LDS_BWD <= 160 * 1024, "LDS budget of the bf16 training decoder");

// ---- one backward call -----------------------------------------------------------------------------------------------------------
enum DecBwdKernel {
    DBK_NONE = 0,
    DBK_DECODER_BWD = 1,     // decoder_bwd_kernel
    DBK_PLANE_GATHER = 2,    // plane_gather_kernel
    DBK_LINEAR_WGRAD = 3,    // linear_wgrad_kernel
    DBK_DECT = 4,            // dect_kernel<true, 4>
    DBK_DECT_REDUCE = 5,     // dect_reduce_kernel
};
// Everything one backward call derives from its arguments, in the order giga_decoder_backward_plan writes it (include/giga_hip.h:
// GIGA_DECODER_BACKWARD_CALL_WORDS; the 64-bit fields as two words, low first).  Offsets count floats from the call's scratch base;
// -1: the call has no such region.
struct DecBwdCall {
    int runs;                // 0: no points or no heads, nothing is launched and every other field is 0
    int kernel;              // DBK_DECODER_BWD or DBK_DECT
    int nheads;
    int planes;              // the call's plane gradient is wanted (0: the head is detached from the planes)
    int gather;              // ... and is gathered and WRITTEN by plane_gather_kernel from the dc rows, not added with atomics
    int nbatch;              // batches of 4 tiles (fp32: decoder_bwd_kernel's persistent loop walks them)
    int grid_x, grid_y, block;
    int lds;                 // dynamic LDS bytes
    int heads_per_wg;        // fp32: heads one workgroup walks: 1 (grid_y = nheads) while the point batches cannot fill the chip
    int wgrad_merged;        // fp32: the heads' weight-gradient problems share ONE linear_wgrad_kernel launch
    int wgrad_launches;      // fp32: linear_wgrad_kernel launches (bf16: 0, the gradients leave as partial tiles)
    int nb_total;            // fp32: column blocks of one weight-gradient launch
    int ksplit_cap;          // fp32: blocks of points a launch may use, LIN_BLOCKS / nb_total
    int ksplit;              // fp32: ... and the blocks it uses, each of
    int pts_per_block;       // fp32: this many points (a multiple of 32); grid of a launch = nb_total * ksplit
    int launches;            // kernel launches of the call: the main kernel, the gather, the weight gradients
    int fwd_grid_x;          // bf16: the training forward of the same points, dect_kernel<false, FWD_NW> (grid_y = nheads)
    int fwd_block, fwd_lds;
    int bf16;
    long long P;             // points
    long long tiles;         // 32-point tiles
    long long head_off;      // head k of the call: fp32 its DB_NARR row arrays, bf16 its partial tiles [grid_x][DECT_NTILES][1024], at
    long long head_stride;   //   head_off + k * head_stride
    long long cbuf_off;      // fp32: C [P][96]
    long long pbuf_off;      // fp32: PP [P][32]
    long long dcbuf_off;     // dc rows [P][96]: fp32 always, bf16 in the call that may gather
    long long scratch_floats;    // the call's total
};
constexpr int DEC_BWD_CALL_WORDS = sizeof(DecBwdCall) / sizeof(int);

// planes_wanted: the call's plane gradient reaches the encoder; may_gather: the step lets this call WRITE the plane gradient (it is
// the step's first: the occupancy call).  The gather then runs for one head with PS_MINN .. PS_MAXN points per scene.
inline DecBwdCall dec_bwd_call_plan(bool bf16, int B, int N, int nheads, bool planes_wanted, bool may_gather) {
    DecBwdCall c{};
    const long long P = (long long)B * N;
    if (P <= 0 || nheads <= 0) return c;
    c.runs = 1;
    c.bf16 = bf16;
    c.nheads = nheads;
    c.planes = planes_wanted;
    c.gather = planes_wanted && may_gather && nheads == 1 && N >= PS_MINN && N <= PS_MAXN;
    c.P = P;
    c.tiles = (P + 31) / 32;
    const long long nbatch = (c.tiles + 3) / 4;                 // four waves of one tile each
    c.nbatch = (int)nbatch;
    c.grid_x = (int)(nbatch < 256 ? nbatch : 256);              // one persistent workgroup per CU
    c.block = 256;
    if (bf16) {
        // one fused launch: every head gets its own workgroups, which leave their weight gradients as partial tiles
        c.kernel = DBK_DECT;
        c.grid_y = nheads;
        c.heads_per_wg = 1;
        c.lds = LDS_BWD;
        c.launches = 1 + c.gather;
        const long long fwd = (c.tiles + FWD_NW - 1) / FWD_NW;
        c.fwd_grid_x = (int)(fwd < 256 ? fwd : 256);
        c.fwd_block = FWD_NW * 64;
        c.fwd_lds = LDS_FWD8;
        c.cbuf_off = c.pbuf_off = -1;
        c.dcbuf_off = may_gather ? 0 : -1;
        c.head_off = may_gather ? P * 96 : 0;
        c.head_stride = (long long)c.grid_x * DECT_NTILES * DECT_TILE_FLOATS;
        c.scratch_floats = c.head_off + c.head_stride * nheads;
        return c;
    }
    c.kernel = DBK_DECODER_BWD;
    // few point batches (train_giga's single grasp query per scene = ONE batch): every head gets its own workgroup -- the three
    // grasp heads of 32 points took 120 us one after the other in a single workgroup, 40 us side by side
    const bool split = c.grid_x * nheads <= 256;
    c.heads_per_wg = split ? 1 : nheads;
    c.grid_y = split ? nheads : 1;
    c.lds = (int)DEC_BWD_LDS;
    // weight / bias gradients: one launch per head, or ONE for all heads when their problems fit one argument struct (the three
    // grasp heads of a one-query call: three 6-us launches of a handful of workgroups each)
    c.wgrad_merged = nheads > 1 && LIN_PER_HEAD * nheads <= LIN_MAX;
    c.wgrad_launches = c.wgrad_merged ? 1 : nheads;
    c.nb_total = LIN_NB_PER_HEAD * (c.wgrad_merged ? nheads : 1);
    c.ksplit_cap = LIN_BLOCKS / c.nb_total < 1 ? 1 : LIN_BLOCKS / c.nb_total;
    long long ppb = (P + c.ksplit_cap - 1) / c.ksplit_cap;
    ppb = (ppb + 31) / 32 * 32;
    c.pts_per_block = (int)ppb;
    c.ksplit = (int)((P + ppb - 1) / ppb);
    c.launches = 1 + c.gather + c.wgrad_launches;
    c.head_off = 0;
    c.head_stride = P * 32 * DB_NARR;
    c.cbuf_off = c.head_stride * nheads;
    c.pbuf_off = c.cbuf_off + P * 96;
    c.dcbuf_off = c.pbuf_off + P * 32;
    c.scratch_floats = c.dcbuf_off + P * 96;
    return c;
}

// ---- the decoder part of one training step (giga_backward) ---------------------------------------------------------------------
// The occupancy call (head bit 8, M queries per scene) runs first: where it gathers, it WRITES the plane gradients and nothing needs
// clearing; the grasp call (head bits 0..2, N queries per scene) then adds its own with atomics.  fp32: the occupancy call's weight
// gradients go to the side stream and may still be reading their rows while the grasp call runs, so the two calls' scratch lies
// apart.  bf16: the partial tiles of both calls wait for the one dect_reduce_kernel launch at the end.
constexpr int TRAIN_DEC_MAX_LAUNCHES = 8;
struct TrainDecPlan {
    int bf16;
    int clear_planes;        // the plane-gradient buffer is cleared first (no call writes it)
    int reduce;              // bf16: dect_reduce_kernel ends the decoder part
    int launches;            // kernel launches of the decoder part, and
    int order[TRAIN_DEC_MAX_LAUNCHES];     // their kernels (DecBwdKernel) in the order they are enqueued
    long long occ_base;      // the calls' scratch bases, in floats from the step's decoder scratch
    long long grasp_base;
    long long scratch_floats;    // the step's decoder scratch at this precision
    DecBwdCall occ, grasp;
};
constexpr int TRAIN_DEC_PLAN_WORDS = sizeof(TrainDecPlan) / sizeof(int);
static_assert(sizeof(DecBwdCall) == 22 * sizeof(int) + 8 * sizeof(long long) &&
              sizeof(TrainDecPlan) == 12 * sizeof(int) + 3 * sizeof(long long) + 2 * sizeof(DecBwdCall), "the plans have no padding");

// head_present: the head bits alone.  A caller without occupancy queries to hand (giga_backward without p_tsdf) clears bit 8.
inline TrainDecPlan train_dec_plan(int B, int N, int M, int head_present, bool detach_occ, bool bf16) {
    TrainDecPlan t{};
    t.bf16 = bf16;
    int ng = 0;
    for (int h = 0; h < 3; ++h) ng += head_present >> h & 1;
    t.occ = dec_bwd_call_plan(bf16, B, M, head_present >> 3 & 1, !detach_occ, true);
    t.grasp = dec_bwd_call_plan(bf16, B, N, ng, true, false);
    t.clear_planes = !t.occ.gather;
    t.occ_base = 0;
    t.grasp_base = t.occ.scratch_floats;
    t.scratch_floats = t.occ.scratch_floats + t.grasp.scratch_floats;
    for (const DecBwdCall* c : {&t.occ, &t.grasp}) {
        if (!c->runs) continue;
        t.order[t.launches++] = c->kernel;
        if (c->gather) t.order[t.launches++] = DBK_PLANE_GATHER;
        for (int k = 0; k < c->wgrad_launches; ++k) t.order[t.launches++] = DBK_LINEAR_WGRAD;
    }
    t.reduce = bf16 && (t.occ.runs || t.grasp.runs);
    if (t.reduce) t.order[t.launches++] = DBK_DECT_REDUCE;
    return t;
}

}  // namespace giga
