// Geometry scoring (scripts/eval_geometry_voxel.py, src/vgn/dataset_voxel_occ.py:109-128): the query points inside the region of
// interest of the successful grasps, and per-scene confusion counts of an occupancy prediction.  Plain vector code, no LDS.
//
//   roi_points  one thread per point of a ragged batch.  The thread finds its grasp by binary search in the prefix of the
//               per-grasp counts (a grasp with count 0 owns no point and is never found), draws three float64 uniforms from two
//               Philox-4x32-10 blocks keyed by (seed; point index inside its scene, data-set scene index), and forms the
//               reference's box point in double, one rounding per operation (no contraction in this file):
//                   x = (u0 - 1) e,  y = (u1 - 0.5) width,  z = (u2 - 1) e,      e = finger_depth * ROI_scale
//                   world = ((R[.][0] x + R[.][1] y) + R[.][2] z) + pos
//                   normalised = float32(world / size - 0.5), rounded once
//               Nothing depends on the batch, the launch shape or the thread that computes a point.
//   confusion   [tp, fp, fn, tn] per scene as 64-bit integer atomics (order independent).  Where both arrays are 16-byte aligned a
//               lane takes 16 elements per step (one 16-byte load of targets, four of logits or one of predictions) and counts its
//               own bit masks; the unaligned head and the tail of a scene go one element per lane, counted by wave64 ballots.
//               Both loops stride over the grid inside the scene.  A wave adds its four sums once.
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "giga_check.h"
#include "giga_philox.h"
#include "giga_ws.h"
#include <cstdint>

#pragma clang fp contract(off)

namespace giga {

constexpr int GEO_BLOCK = 256;
constexpr int GEO_VEC = 16;                   // elements per lane and step of the aligned body
constexpr int GEO_MAX_BLOCKS_X = 1024;        // grid-stride beyond (256 CUs x 4)
constexpr unsigned ROI_STREAM = 0x524F49u;    // counter word 3 of the ROI draws ("ROI"): no other generator of the library uses it

// ------------------------------------------------------------------------------------------------------------------ ROI points
__global__ __launch_bounds__(GEO_BLOCK) void roi_points_kernel(const double* __restrict__ grasps, const int* __restrict__ offsets,
                                                               const int* __restrict__ scene, const int* __restrict__ first, int G,
                                                               int n, unsigned k0, unsigned k1, double extent, double size,
                                                               double* __restrict__ world, float* __restrict__ normalised) {
    const int i = blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = G - 1;                   // the first grasp whose end lies beyond i: offsets[G] = n > i, so there is one
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid + 1] > i) hi = mid; else lo = mid + 1;
    }
    const double* g = grasps + 13 * (size_t)lo;
    const unsigned point = (unsigned)(i - offsets[lo] + first[lo]), sc = (unsigned)scene[lo];
    const Philox a = philox4x32_10(point, sc, 0u, ROI_STREAM, k0, k1), b = philox4x32_10(point, sc, 1u, ROI_STREAM, k0, k1);
    const double u0 = noise_u53(a.x[0], a.x[1]), u1 = noise_u53(a.x[2], a.x[3]), u2 = noise_u53(b.x[0], b.x[1]);
    const double x = (u0 - 1.0) * extent, y = (u1 - 0.5) * g[12], z = (u2 - 1.0) * extent;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double w = ((g[3 * q] * x + g[3 * q + 1] * y) + g[3 * q + 2] * z) + g[9 + q];
        world[3 * (size_t)i + q] = w;
        normalised[3 * (size_t)i + q] = (float)(w / size - 0.5);
    }
}

struct RoiWs { size_t grasps, ints, total; };
static RoiWs roi_workspace(int G) {
    WsLayout L;
    RoiWs w;
    w.grasps = L.take<double>((size_t)G * 13);
    w.ints = L.take<int>((size_t)3 * G + 1);
    w.total = L.total;
    return w;
}

static int launch_roi_points(const double* grasps, const int* offsets, const int* scene, const int* first, int G, unsigned long long seed,
                             double extent, double size, double* world, float* normalised, uint8_t* ws, hipStream_t s) {
    const int n = offsets[G];
    if (n == 0) return 0;
    const RoiWs w = roi_workspace(G);
    double* d_g = reinterpret_cast<double*>(ws + w.grasps);
    int* d_off = reinterpret_cast<int*>(ws + w.ints);
    int* d_scene = d_off + (G + 1);
    int* d_first = d_scene + G;
    if (hipMemcpyAsync(d_g, grasps, (size_t)G * 13 * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    if (hipMemcpyAsync(d_off, offsets, (size_t)(G + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    if (hipMemcpyAsync(d_scene, scene, (size_t)G * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    if (hipMemcpyAsync(d_first, first, (size_t)G * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    GIGA_LAUNCH(roi_points_kernel, dim3((unsigned)((n + GEO_BLOCK - 1) / GEO_BLOCK)), dim3(GEO_BLOCK), 0, s, d_g, d_off, d_scene, d_first,
                G, n, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), extent, size, world, normalised);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

// ------------------------------------------------------------------------------------------------------------ confusion counts
__device__ __forceinline__ unsigned nonzero_bytes(unsigned w) {          // 4 bits: which bytes of w are not 0
    return ((w & 0xffu) ? 1u : 0u) | ((w & 0xff00u) ? 2u : 0u) | ((w & 0xff0000u) ? 4u : 0u) | ((w & 0xff000000u) ? 8u : 0u);
}
__device__ __forceinline__ unsigned nonzero_bytes16(uint4 v) {
    return nonzero_bytes(v.x) | nonzero_bytes(v.y) << 4 | nonzero_bytes(v.z) << 8 | nonzero_bytes(v.w) << 12;
}
__device__ __forceinline__ unsigned above4(float4 v, double th) {        // NaN compares false
    return ((double)v.x > th ? 1u : 0u) | ((double)v.y > th ? 2u : 0u) | ((double)v.z > th ? 4u : 0u) | ((double)v.w > th ? 8u : 0u);
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool LOGITS>
__global__ __launch_bounds__(GEO_BLOCK) void occ_confusion_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ pred,
                                                                  double th, const uint8_t* __restrict__ target,
                                                                  const int* __restrict__ offsets, int aligned,
                                                                  unsigned long long* __restrict__ counts) {
    const int sc = blockIdx.y;
    const long long s0 = offsets[sc], n = (long long)offsets[sc + 1] - s0;
    if (n <= 0) return;
    // [0, head) one element per lane, [head, head + 16 nvec) 16 per lane at 16-byte aligned addresses, then the tail
    long long head = n, nvec = 0;
    if (aligned) {
        head = (GEO_VEC - (s0 & (GEO_VEC - 1))) & (GEO_VEC - 1);
        head = head < n ? head : n;
        nvec = (n - head) / GEO_VEC;
    }
    const long long tail = head + nvec * GEO_VEC, ns = head + (n - tail);
    const long long tid = (long long)blockIdx.x * GEO_BLOCK + threadIdx.x, stride = (long long)gridDim.x * GEO_BLOCK;
    const int lane = threadIdx.x & 63;
    unsigned long long c[4] = {0, 0, 0, 0};                              // tp, fp, fn, tn of this lane
    for (long long v = tid; v < nvec; v += stride) {
        const size_t e = (size_t)(s0 + head + v * GEO_VEC);
        const unsigned t = nonzero_bytes16(*reinterpret_cast<const uint4*>(target + e));
        unsigned p;
        if (LOGITS) {
            const float4* l = reinterpret_cast<const float4*>(logits + e);
            p = above4(l[0], th) | above4(l[1], th) << 4 | above4(l[2], th) << 8 | above4(l[3], th) << 12;
        } else {
            p = nonzero_bytes16(*reinterpret_cast<const uint4*>(pred + e));
        }
        c[0] += __popc(p & t);
        c[1] += __popc(p & ~t);
        c[2] += __popc(~p & t & 0xffffu);
        c[3] += __popc(~p & ~t & 0xffffu);
    }
    // (the trip count is the wave's: every lane of a wave reaches every ballot)
    unsigned long long b[4] = {0, 0, 0, 0};
    for (long long base = tid - lane; base < ns; base += stride) {
        const long long j = base + lane;
        const bool live = j < ns;
        const size_t e = (size_t)(s0 + (live ? (j < head ? j : tail + (j - head)) : 0));
        const bool t = target[e] != 0;
        const bool p = LOGITS ? (double)logits[e] > th : pred[e] != 0;
        b[0] += __popcll(__ballot(live && p && t));
        b[1] += __popcll(__ballot(live && p && !t));
        b[2] += __popcll(__ballot(live && !p && t));
        b[3] += __popcll(__ballot(live && !p && !t));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long sum = wave_sum(c[k]) + b[k];
        if (lane == 0 && sum) atomicAdd(&counts[4 * (size_t)sc + k], sum);
    }
}

static size_t confusion_workspace_bytes(int B) {
    WsLayout L;
    L.take<int>((size_t)B + 1);
    return L.total;
}

static int launch_occ_confusion(const float* logits, const uint8_t* pred, double th, const uint8_t* target, const int* offsets, int B,
                                unsigned long long* counts, uint8_t* ws, hipStream_t s) {
    if (hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(unsigned long long), s) != hipSuccess) return -10;
    const int max_n = ragged_max_count(offsets, B);
    if (max_n == 0) return 0;
    int* d_off = reinterpret_cast<int*>(ws);
    if (hipMemcpyAsync(d_off, offsets, (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(logits ? (const void*)logits : (const void*)pred);
    const int aligned = (addr & 15u) == 0 ? 1 : 0;
    long long bx = ((long long)max_n + (long long)GEO_BLOCK * GEO_VEC - 1) / ((long long)GEO_BLOCK * GEO_VEC);
    bx = bx > GEO_MAX_BLOCKS_X ? GEO_MAX_BLOCKS_X : bx;
    const dim3 grid((unsigned)bx, (unsigned)B);
    if (logits)
        GIGA_LAUNCH(occ_confusion_kernel<true>, grid, dim3(GEO_BLOCK), 0, s, logits, pred, th, target, d_off, aligned, counts);
    else
        GIGA_LAUNCH(occ_confusion_kernel<false>, grid, dim3(GEO_BLOCK), 0, s, logits, pred, th, target, d_off, aligned, counts);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // namespace giga

using namespace giga;

extern "C" {

size_t giga_roi_points_workspace_bytes(int n_grasps) {
    if (n_grasps <= 0) return 0;
    return roi_workspace(n_grasps).total;
}

int giga_roi_points(const double* grasps, const int32_t* point_offsets, const int32_t* grasp_scene, const int32_t* grasp_first,
                    int n_grasps, uint64_t seed, double finger_depth, double roi_scale, double size, double* world,
                    float* normalised, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_grasps < 0) return -1;
    if (!finite_f64(finger_depth) || !finite_f64(roi_scale) || !finite_f64(size) || size == 0.0) return -1;
    if (n_grasps == 0) return 0;
    if (!ragged_ok(point_offsets, n_grasps)) return -1;
    if (point_offsets[n_grasps] == 0) return 0;
    if (!grasps || !grasp_scene || !grasp_first || !workspace) return -1;
    for (int g = 0; g < n_grasps; ++g) {
        // (the point index inside the scene is one 32-bit counter word)
        if (grasp_scene[g] < 0 || grasp_first[g] < 0 ||
            (long long)grasp_first[g] + (point_offsets[g + 1] - point_offsets[g]) > 0x7fffffffLL)
            return -1;
        for (int q = 0; q < 13; ++q)
            if (!finite_f64(grasps[13 * (size_t)g + q])) return -1;
    }
    if (!world || !normalised) return -6;
    if (workspace_bytes < giga_roi_points_workspace_bytes(n_grasps)) return -4;
    return launch_roi_points(grasps, point_offsets, grasp_scene, grasp_first, n_grasps, seed, finger_depth * roi_scale, size, world,
                             normalised, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

size_t giga_occ_confusion_workspace_bytes(int B) {
    if (B <= 0 || B > GIGA_MAX_SCENES) return 0;
    return confusion_workspace_bytes(B);
}

int giga_occ_confusion(const float* logits, const uint8_t* pred, double logit_threshold, const uint8_t* target,
                       const int32_t* offsets, int B, uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = ragged_batch_check(B)) return rc;
    if (B == 0) return 0;
    if (!ragged_ok(offsets, B)) return -1;
    if ((logits != nullptr) == (pred != nullptr) && offsets[B] > 0) return -1;         // exactly one form of the prediction
    if ((offsets[B] > 0 && !target) || !workspace) return -1;
    if (logits && !(logit_threshold == logit_threshold)) return -1;
    if (!counts) return -6;
    if (workspace_bytes < giga_occ_confusion_workspace_bytes(B)) return -4;
    return launch_occ_confusion(logits, pred, logit_threshold, target, offsets, B, reinterpret_cast<unsigned long long*>(counts),
                                static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

}  // extern "C"
