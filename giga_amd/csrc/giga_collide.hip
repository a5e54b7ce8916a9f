// Do two triangle meshes intersect?  M bodies packed back to back (the ragged layout of giga_eval.hip), P pairs of body indices,
// one byte per pair.  The decision is the one include/giga_hip.h writes out: orientation determinants in double with one rounding
// per operation (no contraction in this file), a segment hits a triangle when its ends are not strictly on one side of the plane
// and the three edge determinants agree in sign (zero counts), two triangles intersect when an edge of either hits the other.
//
//   boxes     one workgroup per body: the float32 box over the vertices of its usable triangles (indices in range, finite
//             corners).  min / max of float32 are exact.  A body without a usable triangle gets (+inf, -inf): disjoint from all.
//   pairs     a workgroup owns a pair and a tile of CO_BLOCK triangles of its larger body, one per lane.  Pairs whose boxes are
//             disjoint end there.  Otherwise only triangles whose own box meets the INTERSECTION of the two body boxes take part:
//             the lanes' triangles are flagged once, the other body's triangles are walked CO_BLOCK at a time and the survivors
//             are compacted into an LDS list by ballot and popcount (giga_scan.h's block_combine, lane order).  When the list
//             cannot take another CO_BLOCK entries (or the walk ends) every live lane tests its triangle against each entry;
//             all lanes read the same entry, a broadcast.  The workgroup stops as soon as one lane has found an intersection, or
//             when it sees that another workgroup has decided the pair.
// hit[p] is zeroed by an init kernel; the only other write is a plain store of 1, so racing workgroups agree, and a pair's byte
// depends on its two bodies alone.  No atomics, no scratch.
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "giga_check.h"
#include "giga_scan.h"
#include "giga_ws.h"
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace giga {

constexpr int CO_BLOCK = 256;
constexpr int CO_WAVES = CO_BLOCK / 64;
constexpr int CO_LIST = 512;                  // LDS list entries (3 float4 each: 24 KB); flushed above CO_LIST - CO_BLOCK
constexpr int CO_MAX_GRID_Y = 65535;

// a triangle as the pair kernel sees it: nine float32 coordinates and whether it takes part
struct CoTri { float x[9]; bool ok; };

// face f of a body (indices count from the body's first vertex): ok = f < nf, indices in range, every coordinate finite
__device__ __forceinline__ CoTri co_load(const float* __restrict__ v, int nv, const int* __restrict__ t, int nf, int f) {
    CoTri r;
    const bool in = f < nf;
    const int i0 = in ? t[3 * (size_t)f] : 0, i1 = in ? t[3 * (size_t)f + 1] : 0, i2 = in ? t[3 * (size_t)f + 2] : 0;
    r.ok = in && (unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        r.x[q] = r.ok ? v[3 * (size_t)i0 + q] : 0.f;
        r.x[3 + q] = r.ok ? v[3 * (size_t)i1 + q] : 0.f;
        r.x[6 + q] = r.ok ? v[3 * (size_t)i2 + q] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) r.ok = r.ok && r.x[q] - r.x[q] == 0.f;      // (inf - inf and NaN - NaN are NaN)
    return r;
}

// ------------------------------------------------------------------------------------------------------------------ body boxes
__global__ __launch_bounds__(CO_BLOCK) void collide_bbox_kernel(const float* __restrict__ vertices, const int* __restrict__ vo,
                                                                 const int* __restrict__ triangles, const int* __restrict__ fo,
                                                                 float* __restrict__ bbox) {
    __shared__ float s_lo[CO_WAVES][3], s_hi[CO_WAVES][3];
    const int body = blockIdx.x, f0 = fo[body], nf = fo[body + 1] - f0, nv = vo[body + 1] - vo[body];
    const float* v = vertices + 3 * (size_t)vo[body];
    const int* t = triangles + 3 * (size_t)f0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int f = threadIdx.x; f < nf; f += CO_BLOCK) {
        const CoTri r = co_load(v, nv, t, nf, f);
        if (!r.ok) continue;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            lo[q] = fminf(lo[q], fminf(r.x[q], fminf(r.x[3 + q], r.x[6 + q])));
            hi[q] = fmaxf(hi[q], fmaxf(r.x[q], fmaxf(r.x[3 + q], r.x[6 + q])));
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[q] = fminf(lo[q], __shfl_xor(lo[q], o, 64));
            hi[q] = fmaxf(hi[q], __shfl_xor(hi[q], o, 64));
        }
        if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6][q] = lo[q]; s_hi[threadIdx.x >> 6][q] = hi[q]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int q = threadIdx.x;
        float l = s_lo[0][q], h = s_hi[0][q];
        for (int w = 1; w < CO_WAVES; ++w) { l = fminf(l, s_lo[w][q]); h = fmaxf(h, s_hi[w][q]); }
        bbox[6 * (size_t)body + q] = l;
        bbox[6 * (size_t)body + 3 + q] = h;
    }
}

__global__ __launch_bounds__(CO_BLOCK) void collide_init_kernel(uint8_t* __restrict__ hit, int n) {
    const int i = blockIdx.x * CO_BLOCK + threadIdx.x;
    if (i < n) hit[i] = 0;
}

// ------------------------------------------------------------------------------------------------------------ the exact test
// orient(a, b, c, d) of include/giga_hip.h, in its order
__device__ __forceinline__ double co_orient(const double* a, const double* b, const double* c, const double* d) {
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double wx = d[0] - a[0], wy = d[1] - a[1], wz = d[2] - a[2];
    return (ux * (vy * wz - vz * wy) - uy * (vx * wz - vz * wx)) + uz * (vx * wy - vy * wx);
}

// segment (p, q) against triangle (a, b, c); sp, sq = orient(a, b, c, p), orient(a, b, c, q)
__device__ __forceinline__ bool co_seg_tri(const double* p, const double* q, const double* a, const double* b, const double* c,
                                           double sp, double sq) {
    if ((sp > 0.0 && sq > 0.0) || (sp < 0.0 && sq < 0.0)) return false;
    if (sp == 0.0 && sq == 0.0) return false;                              // in the triangle's plane: not detected
    if (sp != sp || sq != sq) return false;
    const double d0 = co_orient(p, q, a, b), d1 = co_orient(p, q, b, c), d2 = co_orient(p, q, c, a);
    return (d0 >= 0.0 && d1 >= 0.0 && d2 >= 0.0) || (d0 <= 0.0 && d1 <= 0.0 && d2 <= 0.0);
}

// does an edge of triangle x (x, x + 3, x + 6) hit triangle y?  (the three plane determinants are taken once: an edge's sp and
// sq are those of its two ends, the same operations on the same operands)
__device__ __forceinline__ bool co_edges_hit(const double* x, const double* y) {
    const double s0 = co_orient(y, y + 3, y + 6, x), s1 = co_orient(y, y + 3, y + 6, x + 3), s2 = co_orient(y, y + 3, y + 6, x + 6);
    return co_seg_tri(x, x + 3, y, y + 3, y + 6, s0, s1) || co_seg_tri(x + 3, x + 6, y, y + 3, y + 6, s1, s2) ||
           co_seg_tri(x + 6, x, y, y + 3, y + 6, s2, s0);
}

// does the triangle's own box meet the box lo .. hi?
__device__ __forceinline__ bool co_meets(const CoTri& r, const float* lo, const float* hi) {
    bool m = r.ok;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float l = fminf(r.x[q], fminf(r.x[3 + q], r.x[6 + q])), h = fmaxf(r.x[q], fmaxf(r.x[3 + q], r.x[6 + q]));
        m = m && l <= hi[q] && h >= lo[q];
    }
    return m;
}

__global__ __launch_bounds__(CO_BLOCK) void collide_pair_kernel(const float* __restrict__ vertices, const int* __restrict__ vo,
                                                                 const int* __restrict__ triangles, const int* __restrict__ fo,
                                                                 const float* __restrict__ bbox, const int* __restrict__ pairs,
                                                                 uint8_t* hit) {
    __shared__ float4 s_tri[CO_LIST * 3];
    __shared__ unsigned s_wsum[CO_WAVES];
    const int p = blockIdx.x;
    int a = pairs[2 * (size_t)p], b = pairs[2 * (size_t)p + 1];
    if (fo[b + 1] - fo[b] > fo[a + 1] - fo[a]) { const int c = a; a = b; b = c; }     // the lanes own the larger body's triangles
    const int na = fo[a + 1] - fo[a], nb = fo[b + 1] - fo[b];
    float lo[3], hi[3];
    bool apart = false;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        lo[q] = fmaxf(bbox[6 * (size_t)a + q], bbox[6 * (size_t)b + q]);
        hi[q] = fminf(bbox[6 * (size_t)a + 3 + q], bbox[6 * (size_t)b + 3 + q]);
        apart = apart || !(lo[q] <= hi[q]);
    }
    if (apart) return;                                                      // uniform over the workgroup
    const float* va = vertices + 3 * (size_t)vo[a];
    const float* vb = vertices + 3 * (size_t)vo[b];
    const int* ta = triangles + 3 * (size_t)fo[a];
    const int* tb = triangles + 3 * (size_t)fo[b];
    const int nva = vo[a + 1] - vo[a], nvb = vo[b + 1] - vo[b];
    const unsigned lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    volatile const uint8_t* decided = hit + p;

    for (long long first = (long long)blockIdx.y * CO_BLOCK; first < na; first += (long long)gridDim.y * CO_BLOCK) {
        const CoTri own = co_load(va, nva, ta, na, (int)first + (int)threadIdx.x);
        const bool live = co_meets(own, lo, hi);
        if (!__syncthreads_or(live)) continue;
        double x[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) x[q] = (double)own.x[q];
        int count = 0;                                                      // entries in the list (the same in every thread)
        bool found = false;
        for (int base = 0; base < nb; base += CO_BLOCK) {
            const CoTri other = co_load(vb, nvb, tb, nb, base + (int)threadIdx.x);
            const bool keep = co_meets(other, lo, hi);
            const unsigned long long mask = __ballot(keep);
            unsigned total;
            const unsigned at = count + block_combine<CO_WAVES>((unsigned)__popcll(mask & below), (unsigned)__popcll(mask), lane == 0,
                                                                s_wsum, total);
            if (keep) {                                                     // at < count + CO_BLOCK <= CO_LIST
                s_tri[3 * at] = make_float4(other.x[0], other.x[1], other.x[2], other.x[3]);
                s_tri[3 * at + 1] = make_float4(other.x[4], other.x[5], other.x[6], other.x[7]);
                s_tri[3 * at + 2] = make_float4(other.x[8], 0.f, 0.f, 0.f);
            }
            count += (int)total;
            __syncthreads();                                                // the list is written; s_wsum may be written again
            if (count <= CO_LIST - CO_BLOCK && base + CO_BLOCK < nb) continue;
            if (live) {
                for (int e = 0; e < count && !found; ++e) {
                    const float4 t0 = s_tri[3 * e], t1 = s_tri[3 * e + 1], t2 = s_tri[3 * e + 2];
                    const double y[9] = {(double)t0.x, (double)t0.y, (double)t0.z, (double)t0.w, (double)t1.x,
                                         (double)t1.y, (double)t1.z, (double)t1.w, (double)t2.x};
                    found = co_edges_hit(x, y) || co_edges_hit(y, x);
                }
            }
            count = 0;
            // one thread looks whether another workgroup has decided the pair; the barrier also frees the list
            if (__syncthreads_or(found || (threadIdx.x == 0 && *decided != 0))) {
                if (threadIdx.x == 0) hit[p] = 1;
                return;
            }
        }
    }
}

struct CollideWs { size_t offs, pairs, bbox, total; };
static CollideWs collide_workspace(int M, int P) {
    WsLayout L;
    CollideWs w;
    w.offs = L.take<int>((size_t)2 * (M + 1));
    w.pairs = L.take<int>((size_t)2 * P);
    w.bbox = L.take<float>((size_t)6 * M);
    w.total = L.total;
    return w;
}
static int launch_mesh_collide(const float* vertices, const int* vertex_offsets, const int* triangles, const int* triangle_offsets, int M,
                               const int* pairs, int P, uint8_t* hit, uint8_t* ws, hipStream_t s) {
    const CollideWs w = collide_workspace(M, P);
    int* vo = reinterpret_cast<int*>(ws + w.offs);
    int* fo = vo + (M + 1);
    int* pr = reinterpret_cast<int*>(ws + w.pairs);
    float* bbox = reinterpret_cast<float*>(ws + w.bbox);
    // (pageable host memory: the copies have left the caller's arrays when the call returns)
    if (hipMemcpyAsync(vo, vertex_offsets, (size_t)(M + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    if (hipMemcpyAsync(fo, triangle_offsets, (size_t)(M + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    if (hipMemcpyAsync(pr, pairs, (size_t)2 * P * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    GIGA_LAUNCH(collide_init_kernel, dim3((P + CO_BLOCK - 1) / CO_BLOCK), dim3(CO_BLOCK), 0, s, hit, P);
    const int max_f = ragged_max_count(triangle_offsets, M);
    if (max_f > 0) {
        GIGA_LAUNCH(collide_bbox_kernel, dim3(M), dim3(CO_BLOCK), 0, s, vertices, vo, triangles, fo, bbox);
        const int tiles = (max_f + CO_BLOCK - 1) / CO_BLOCK;
        GIGA_LAUNCH(collide_pair_kernel, dim3(P, tiles < CO_MAX_GRID_Y ? tiles : CO_MAX_GRID_Y), dim3(CO_BLOCK), 0, s, vertices, vo,
                    triangles, fo, bbox, pr, hit);
    }
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // namespace giga

using namespace giga;

extern "C" {

size_t giga_mesh_collide_workspace_bytes(int M, int P) {
    if (M <= 0 || M > GIGA_MAX_SCENES || P < 0) return 0;
    return collide_workspace(M, P).total;
}

int giga_mesh_collide(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                      int M, const int32_t* pairs, int P, uint8_t* hit, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = ragged_batch_check(M)) return rc;
    if (P < 0) return -1;
    if (M == 0 || P == 0) return 0;
    if (!mesh_batch_check(vertex_offsets, triangle_offsets, M, vertices, triangles) || !pairs || !workspace) return -1;
    for (size_t i = 0; i < (size_t)P; ++i) {
        const int32_t a = pairs[2 * i], b = pairs[2 * i + 1];
        if (a < 0 || a >= M || b < 0 || b >= M || a == b) return -1;
    }
    if (!hit) return -6;
    if (workspace_bytes < giga_mesh_collide_workspace_bytes(M, P)) return -4;
    return launch_mesh_collide(vertices, vertex_offsets, triangles, triangle_offsets, M, pairs, P, hit, static_cast<uint8_t*>(workspace),
                               static_cast<hipStream_t>(stream));
}

}  // extern "C"
