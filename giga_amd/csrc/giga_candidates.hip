// Grasp candidates from the oriented cloud: the geometry of scripts/generate_data_parallel.py around its physics step
// (sample_grasp_point :133-144, the frame and yaw angles of evaluate_grasp_point :147-161), for a ragged batch of scenes.
// include/giga_hip.h spells the arithmetic out; all of it is float64 with one rounding per operation (no contraction in this file),
// so that a numpy restatement reproduces the bytes (tests/candidates_emu.py).
//
//   one workgroup per scene, two phases
//   list   the scene's points in rounds of CAND_BLOCK: a thread decides whether its point is eligible, block_scan_rounds
//          (giga_scan.h) gives the prefix in point order, and the point's index goes to list[prefix].  No atomics.
//   draw   thread t takes the candidates t, t + CAND_BLOCK, ...: one Philox block, the e-th entry of the list, position, frame, and
//          the yaw quaternions from the caller's (sin, cos) table, which is read through a wave-uniform address.
// The list is written and read by the same workgroup; block_scan_rounds ends every round with a barrier.  The work is small (24 B
// read per point, 28 + 32 Y B written per candidate), so one workgroup per scene keeps a scene's result independent of the batch
// without a second launch.
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "giga_check.h"
#include "giga_philox.h"
#include "giga_scan.h"
#include "giga_ws.h"
#include <cstdint>

#pragma clang fp contract(off)

namespace giga {

constexpr int CAND_BLOCK = SCAN_BLOCK;
constexpr int CAND_WAVES = CAND_BLOCK / 64;
constexpr unsigned CAND_STREAM = 0x47525350u;   // counter word 3 of the candidate draws ("GRSP"): no other generator of the library uses it

struct CandBox { double lower[3], upper[3]; };

__device__ __forceinline__ bool cand_finite(double x) { return x - x == 0.0; }

__device__ __forceinline__ bool cand_eligible(const float* __restrict__ p, const float* __restrict__ n, const CandBox& box) {
    const double P[3] = {(double)p[0], (double)p[1], (double)p[2]}, N[3] = {(double)n[0], (double)n[1], (double)n[2]};
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) ok = ok && cand_finite(P[c]) && cand_finite(N[c]) && P[c] >= box.lower[c] && P[c] <= box.upper[c];
    return ok && N[2] > -0.1 && (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2] > 0.0;
}

__device__ __forceinline__ void cand_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void cand_normalise(double* a) {
    const double len = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    a[0] /= len; a[1] /= len; a[2] /= len;
}

// the quaternion (xyzw) of the frame whose z axis is -N / |N|
__device__ __forceinline__ void cand_frame(const double* N, double* q) {
    const double len = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
    const double z[3] = {-N[0] / len, -N[1] / len, -N[2] / len};
    double x[3] = {1.0, 0.0, 0.0}, y[3];
    if (fabs(fabs((x[0] * z[0] + x[1] * z[1]) + x[2] * z[2]) - 1.0) <= 1e-8 + 1e-4) { x[0] = 0.0; x[1] = 1.0; }
    cand_cross(z, x, y);
    cand_cross(y, z, x);
    cand_normalise(x);
    cand_normalise(y);
    const double m00 = x[0], m01 = y[0], m02 = z[0], m10 = x[1], m11 = y[1], m12 = z[1], m20 = x[2], m21 = y[2], m22 = z[2];
    const double t = (m00 + m11) + m22;
    int choice = 0;
    double best = m00;
    if (m11 > best) { best = m11; choice = 1; }
    if (m22 > best) { best = m22; choice = 2; }
    if (t > best) choice = 3;
    if (choice == 0) { q[0] = (1.0 - t) + 2.0 * m00; q[1] = m10 + m01; q[2] = m20 + m02; q[3] = m21 - m12; }
    else if (choice == 1) { q[0] = m01 + m10; q[1] = (1.0 - t) + 2.0 * m11; q[2] = m21 + m12; q[3] = m02 - m20; }
    else if (choice == 2) { q[0] = m02 + m20; q[1] = m12 + m21; q[2] = (1.0 - t) + 2.0 * m22; q[3] = m10 - m01; }
    else { q[0] = m21 - m12; q[1] = m02 - m20; q[2] = m10 - m01; q[3] = 1.0 + t; }
    const double norm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    q[0] /= norm; q[1] /= norm; q[2] /= norm; q[3] /= norm;
}

__global__ __launch_bounds__(CAND_BLOCK) void grasp_candidates_kernel(const float* __restrict__ points, const float* __restrict__ normals,
                                                                      const int* __restrict__ offsets, const unsigned* __restrict__ scene_ids,
                                                                      const double* __restrict__ yaw_table, CandBox box, int K, int Y,
                                                                      double lo, double span, unsigned k0, unsigned k1, int* list,
                                                                      double* __restrict__ pos, double* __restrict__ quat,
                                                                      int* __restrict__ index, int* __restrict__ counts) {
    __shared__ unsigned wsum[CAND_WAVES];
    const unsigned b = blockIdx.x;
    const int first = offsets[b], n = offsets[b + 1] - first;
    const float* __restrict__ P = points + 3 * (size_t)first;
    const float* __restrict__ N = normals + 3 * (size_t)first;
    int* mine = list + first;                                                  // the scene's list: at most n entries
    unsigned flag = 0;                                                         // of the point the thread loaded in this round
    const unsigned E = block_scan_rounds<CAND_WAVES, unsigned>(
        (unsigned)n, wsum, [&](unsigned i) { return flag = cand_eligible(P + 3 * (size_t)i, N + 3 * (size_t)i, box) ? 1u : 0u; },
        [&](unsigned i, unsigned pre) {
            if (flag) mine[pre] = (int)i;
        });
    if (threadIdx.x == 0) counts[b] = (int)E;
    if (E == 0) return;
    const unsigned id = scene_ids[b];
    for (int k = threadIdx.x; k < K; k += CAND_BLOCK) {
        const Philox r = philox4x32_10((unsigned)k, id, 0u, CAND_STREAM, k0, k1);
        const unsigned e = (unsigned)(((unsigned long long)r.x[0] * E) >> 32);
        const int i = mine[e];
        const double depth = lo + span * noise_u53(r.x[2], r.x[3]);
        const size_t row = (size_t)b * K + k;
        double Nd[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Nd[c] = (double)N[3 * (size_t)i + c];
            pos[3 * row + c] = (double)P[3 * (size_t)i + c] + Nd[c] * depth;
        }
        index[row] = i;
        double q[4];
        cand_frame(Nd, q);
        double* o = quat + row * (size_t)Y * 4;
        for (int j = 0; j < Y; ++j) {
            const double s = yaw_table[2 * j], c = yaw_table[2 * j + 1];
            o[4 * j] = q[0] * c + q[1] * s;
            o[4 * j + 1] = q[1] * c - q[0] * s;
            o[4 * j + 2] = q[2] * c + q[3] * s;
            o[4 * j + 3] = q[3] * c - q[2] * s;
        }
    }
}

struct CandWs { size_t offsets, ids, table, list, total; };
static CandWs candidates_workspace(int B, int n, int Y) {
    WsLayout L;
    CandWs w;
    w.offsets = L.take<int>((size_t)B + 1);
    w.ids = L.take<unsigned>((size_t)B);
    w.table = L.take<double>((size_t)Y * 2);
    w.list = L.take<int>((size_t)n);
    w.total = L.total;
    return w;
}

}  // namespace giga

using namespace giga;

extern "C" {

size_t giga_grasp_candidates_workspace_bytes(int B, int n_points, int n_rotations) {
    if (B <= 0 || B > GIGA_MAX_SCENES || n_points < 0 || n_rotations < 1 || n_rotations > GIGA_CANDIDATES_MAX_ROTATIONS) return 0;
    return candidates_workspace(B, n_points, n_rotations).total;
}

int giga_grasp_candidates(const float* points, const float* normals, const int32_t* offsets, const uint32_t* scene_ids, int B, int K,
                          const double* lower, const double* upper, double finger_depth, double eps, const double* yaw_table,
                          int n_rotations, uint64_t seed, double* pos, double* quat, int32_t* index, int32_t* counts, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (const int rc = ragged_batch_check(B)) return rc;
    const int Y = n_rotations;
    if (K < 0 || Y < 1 || Y > GIGA_CANDIDATES_MAX_ROTATIONS) return -1;
    if (!finite_f64(finger_depth) || !finite_f64(eps)) return -1;
    if (B == 0 || K == 0) return 0;
    if (!lower || !upper || !yaw_table || !scene_ids || !ragged_ok(offsets, B)) return -1;
    CandBox box;
    for (int c = 0; c < 3; ++c) {
        if (!finite_f64(lower[c]) || !finite_f64(upper[c])) return -1;
        box.lower[c] = lower[c];
        box.upper[c] = upper[c];
    }
    for (int j = 0; j < 2 * Y; ++j)
        if (!finite_f64(yaw_table[j])) return -1;
    const int n = offsets[B];
    if (n > 0 && (!points || !normals)) return -1;
    if (!workspace) return -1;
    if (!pos || !quat || !index || !counts) return -6;
    if (workspace_bytes < giga_grasp_candidates_workspace_bytes(B, n, Y)) return -4;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const CandWs w = candidates_workspace(B, n, Y);
    int* d_off = reinterpret_cast<int*>(ws + w.offsets);
    unsigned* d_ids = reinterpret_cast<unsigned*>(ws + w.ids);
    double* d_table = reinterpret_cast<double*>(ws + w.table);
    // (pageable host memory: the copies have left the caller's arrays when the call returns)
    if (hipMemcpyAsync(d_off, offsets, (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    if (hipMemcpyAsync(d_ids, scene_ids, (size_t)B * sizeof(unsigned), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    if (hipMemcpyAsync(d_table, yaw_table, (size_t)Y * 2 * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    const double lo = -eps * finger_depth, hi = (1.0 + eps) * finger_depth;
    GIGA_LAUNCH(grasp_candidates_kernel, dim3(B), dim3(CAND_BLOCK), 0, s, points, normals, d_off, d_ids, d_table, box, K, Y, lo, hi - lo,
                (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), reinterpret_cast<int*>(ws + w.list), pos, quat, index, counts);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // extern "C"
