// Quadric edge collapse on B triangle meshes: the device counterpart of the reference's `simplify_mesh(mesh, n, 5.)`
// (utils/libsimplify/Simplify.h, `Simplify::simplify_mesh(target, agressiveness)` on value-initialised records), face for face
// and vertex for vertex in float64.
//
// Arithmetic.  Everything is fp64 in the header's order of operations: contraction is off for this file (no product-sum is
// fused), `/` and sqrt are the IEEE ones, comparisons are the plain operators (false on NaN, so a face with a NaN normal counts
// as "not flipped", as in the header), min is fmin.  The per-iteration threshold 1e-9 pow(iteration + 3, agressiveness) is
// computed on the host.
//
// State (B meshes back to back; vertex and triangle numbers are global inside the workspace): vertices p[3], q[10], border,
// list (start, count); triangles v[3], err[4], n[3], deleted, dirty; `refs`, the per-vertex lists of (triangle << 2 | corner)
// entries, one region per mesh of 3 F entries plus room for appended lists; per mesh a counter of deleted triangles.
//
// Initialisation (update_mesh(0)): face normals; the lists are filled by a count / scan / fill and then SORTED per vertex, so
// that the gather of a vertex's quadric adds the plane quadrics of its faces in ascending triangle index, as the header's
// loop does (no floating-point atomics: the order of the additions is part of the result); the edge errors; then the border
// flags -- in the header's order: the first errors are computed while every border flag is still 0.
// Every fifth iteration after the first: stable compaction of the triangle records, lists rebuilt; nothing else recomputed.
//
// A pass at threshold thr.  The header visits the candidates (!(err[3] > thr), not deleted, not dirty) in index order.  Here a
// pass is a sequence of ROUNDS of three launches:
//   claim    every pending triangle that is still a candidate (a dirtied or deleted one drops out) claims, with atomicMax of
//            (round tag << 32 | ~index), every vertex of every live face around its three vertices: the lowest index wins;
//   verify   a triangle that holds all its claims is a winner;
//   execute  every winner runs the header's loop body (first edge below thr with equal border flags that flips nothing:
//            move v0, add the quadrics, delete the faces with both ends, re-point and re-rate the other faces of v1, new
//            list of v0) and is retired, whether it collapsed or not.
// The lowest pending index always wins, so a pass needs at most as many rounds as it has candidates; the host loop carries
// that bound and gives up (-12) beyond it.  A collapse reads and writes only inside its triangle's claim set and only adds
// adjacency inside it, the claim sets of a round's winners are disjoint, and a triangle runs only after every lower candidate
// whose claim set meets its own has run or dropped out: the result is the sequential loop's.  The order of the entries
// inside a list influences nothing.  SIMP_BATCH rounds are launched between two readbacks of the pending counts.
//
// Face budget.  The header leaves a pass right after the collapse that brings faces - deleted <= target.  The state is copied
// before a pass; every collapse logs the faces it deleted under its triangle's index; when a pass crosses the budget, a scan
// in index order finds the triangle i* at which it is reached, and unless that is the last collapse of the pass the mesh is
// restored and the pass run again over the candidates <= i* (lower indices never depend on higher ones).
//
// Overflow of the appended region of `refs`: the collapse is not carried out (the space is claimed before anything is
// changed), its triangle stays pending, a flag is raised; the host rebuilds the lists from the live faces and goes on.
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "giga_check.h"
#include "giga_scan.h"
#include "giga_ws.h"
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#pragma clang fp contract(off)

namespace giga {

constexpr int SIMP_BLOCK = 256;
constexpr int SIMP_SCAN_BLOCK = 1024;
constexpr int SIMP_BATCH = 4;                  // rounds between two readbacks of the pending counts
constexpr int SIMP_MIN_REF_EXTRA = 64;         // == GIGA_SIMPLIFY_MIN_REF_EXTRA

struct SimpMesh {
    int voff, nv, toff, nt, roff, rcap;        // first vertex / count, first triangle / live slots, region of refs
    int active, limit, need;                   // in the current pass; highest candidate (local index); faces to the budget
    int ovoff, otoff, pad;                     // first vertex / triangle of the output
};

struct SimpDev {
    double *P, *Q, *terr, *tn, *terr2, *tn2;
    int *border, *tstart, *tcount, *vcur, *vmesh, *vflag, *vnew;
    unsigned long long* claim;
    int *tv, *tdel, *tv2, *tdel2, *tdirty, *pend, *win, *logdel, *tmesh, *tdst;
    int* refs;
    int *rused, *ndel, *cand, *ovf, *ring, *tot, *budget, *err;     // small per-mesh words (ctl block)
    SimpMesh* mesh;
    int B, Vt, Tt;
};

// ---- the header's arithmetic -------------------------------------------------------------------------------------------------
__device__ __forceinline__ double simp_det(const double* m, int a11, int a12, int a13, int a21, int a22, int a23, int a31, int a32,
                                           int a33) {
    return m[a11] * m[a22] * m[a33] + m[a13] * m[a21] * m[a32] + m[a12] * m[a23] * m[a31] - m[a13] * m[a22] * m[a31] -
           m[a11] * m[a23] * m[a32] - m[a12] * m[a21] * m[a33];
}

__device__ __forceinline__ double simp_vertex_error(const double* q, double x, double y, double z) {
    return q[0] * x * x + 2 * q[1] * x * y + 2 * q[2] * x * z + 2 * q[3] * x + q[4] * y * y + 2 * q[5] * y * z + 2 * q[6] * y +
           q[7] * z * z + 2 * q[8] * z + q[9];
}

__device__ double simp_calculate_error(const SimpDev& s, int a, int b, double* p) {
    double q[10];
#pragma unroll
    for (int m = 0; m < 10; ++m) q[m] = s.Q[10 * (size_t)a + m] + s.Q[10 * (size_t)b + m];
    const int border = s.border[a] & s.border[b];
    const double det = simp_det(q, 0, 1, 2, 1, 4, 5, 2, 5, 7);
    if (det != 0 && !border) {
        p[0] = -1 / det * simp_det(q, 1, 2, 3, 4, 5, 6, 5, 7, 8);
        p[1] = 1 / det * simp_det(q, 0, 2, 3, 1, 5, 6, 2, 7, 8);
        p[2] = -1 / det * simp_det(q, 0, 1, 3, 1, 4, 6, 2, 5, 8);
        return simp_vertex_error(q, p[0], p[1], p[2]);
    }
    const double* p1 = s.P + 3 * (size_t)a;
    const double* p2 = s.P + 3 * (size_t)b;
    const double p3[3] = {(p1[0] + p2[0]) / 2, (p1[1] + p2[1]) / 2, (p1[2] + p2[2]) / 2};
    const double e1 = simp_vertex_error(q, p1[0], p1[1], p1[2]);
    const double e2 = simp_vertex_error(q, p2[0], p2[1], p2[2]);
    const double e3 = simp_vertex_error(q, p3[0], p3[1], p3[2]);
    const double error = fmin(e1, fmin(e2, e3));
    p[0] = p[1] = p[2] = 0.0;                   // (the header leaves p unset when all three are NaN)
    if (e1 == error) { p[0] = p1[0]; p[1] = p1[1]; p[2] = p1[2]; }
    if (e2 == error) { p[0] = p2[0]; p[1] = p2[1]; p[2] = p2[2]; }
    if (e3 == error) { p[0] = p3[0]; p[1] = p3[1]; p[2] = p3[2]; }
    return error;
}

__device__ void simp_errors(const SimpDev& s, int t) {
    const int* v = s.tv + 3 * (size_t)t;
    double p[3];
    double* e = s.terr + 4 * (size_t)t;
    const double e0 = simp_calculate_error(s, v[0], v[1], p);
    const double e1 = simp_calculate_error(s, v[1], v[2], p);
    const double e2 = simp_calculate_error(s, v[2], v[0], p);
    e[0] = e0; e[1] = e1; e[2] = e2;
    e[3] = fmin(e0, fmin(e1, e2));
}

__device__ __forceinline__ void simp_normalize(double* v) {
    const double square = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] /= square; v[1] /= square; v[2] /= square;
}

// length of vertex v's list, never more than its mesh's region (every loop over a list is bounded by the capacity)
__device__ __forceinline__ int simp_list_len(const SimpDev& s, int v, int rcap) {
    const int c = s.tcount[v];
    return c < rcap ? c : rcap;
}

__device__ bool simp_flipped(const SimpDev& s, const double* p, int i0, int i1, int rcap) {
    const int start = s.tstart[i0], n = simp_list_len(s, i0, rcap);
    for (int k = 0; k < n; ++k) {
        const int r = s.refs[start + k], t = r >> 2, c = r & 3;
        if (s.tdel[t]) continue;
        const int* v = s.tv + 3 * (size_t)t;
        const int id1 = v[(c + 1) % 3], id2 = v[(c + 2) % 3];
        if (id1 == i1 || id2 == i1) continue;
        double d1[3], d2[3], nn[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) { d1[m] = s.P[3 * (size_t)id1 + m] - p[m]; d2[m] = s.P[3 * (size_t)id2 + m] - p[m]; }
        simp_normalize(d1);
        simp_normalize(d2);
        if (fabs(d2[0] * d1[0] + d2[1] * d1[1] + d2[2] * d1[2]) > 0.999) return true;
        nn[0] = d1[1] * d2[2] - d1[2] * d2[1];
        nn[1] = d1[2] * d2[0] - d1[0] * d2[2];
        nn[2] = d1[0] * d2[1] - d1[1] * d2[0];
        simp_normalize(nn);
        const double* tn = s.tn + 3 * (size_t)t;
        if (tn[0] * nn[0] + tn[1] * nn[1] + tn[2] * nn[2] < 0.2) return true;
    }
    return false;
}

// ---- small helpers -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int simp_find_mesh(const SimpMesh* mesh, int B, int i, bool triangle) {
    int lo = 0, hi = B - 1;                    // the last mesh whose first slot is <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((triangle ? mesh[mid].toff : mesh[mid].voff) <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// adds the number of lanes with `flag` to counter[m]: one atomic per wave where the wave's lanes agree on m
__device__ __forceinline__ void simp_count_add(int* counter, int m, bool flag) {
    const unsigned long long mask = __ballot(flag);
    if (mask == 0) return;
    const int first = __ffsll((long long)mask) - 1;
    const int m0 = __shfl(m, first, 64);
    if (__ballot(flag && m != m0) == 0) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(counter + m0, __popcll(mask));
    } else if (flag) {
        atomicAdd(counter + m, 1);
    }
}

// triangle slot i of an active mesh (or of any mesh, `all`), inside the live range of its mesh
__device__ __forceinline__ bool simp_slot(const SimpDev& s, int i, bool all, int& m) {
    if (i >= s.Tt) return false;
    m = s.tmesh[i];
    const SimpMesh& me = s.mesh[m];
    return (all || me.active) && i - me.toff < me.nt;
}

// ---- input -------------------------------------------------------------------------------------------------------------------
__global__ void simp_widen_kernel(SimpDev s, const void* vertices, int f64) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i >= s.Vt) return;
    s.vmesh[i] = simp_find_mesh(s.mesh, s.B, i, false);
    for (int m = 0; m < 3; ++m)
        s.P[3 * (size_t)i + m] = f64 ? static_cast<const double*>(vertices)[3 * (size_t)i + m]
                                     : (double)static_cast<const float*>(vertices)[3 * (size_t)i + m];
}

// the check launch: a face index outside its mesh's vertex range raises err and never becomes an address
__global__ void simp_faces_kernel(SimpDev s, const int* triangles) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i >= s.Tt) return;
    const int m = simp_find_mesh(s.mesh, s.B, i, true);
    s.tmesh[i] = m;
    s.tdel[i] = 0;
    const SimpMesh me = s.mesh[m];
    bool bad = false;
    for (int j = 0; j < 3; ++j) {
        const int v = triangles[3 * (size_t)i + j];
        const bool ok = v >= 0 && v < me.nv;
        bad |= !ok;
        s.tv[3 * (size_t)i + j] = me.voff + (ok ? v : 0);
    }
    if (bad) atomicOr(s.err, 1);
}

// ---- reference lists ---------------------------------------------------------------------------------------------------------
__global__ void simp_list_zero_kernel(SimpDev s) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i < s.Vt && s.mesh[s.vmesh[i]].active) s.tcount[i] = 0;
}

__global__ void simp_list_count_kernel(SimpDev s) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    int m;
    if (!simp_slot(s, i, false, m) || s.tdel[i]) return;
    for (int j = 0; j < 3; ++j) atomicAdd(s.tcount + s.tv[3 * (size_t)i + j], 1);
}

// one workgroup per mesh: exclusive prefix, in index order, of
//   mode 0  the list lengths of its vertices   -> tstart (inside the mesh's region of refs), fill cursors zeroed, rused = total
//   mode 1  the live flags of its triangles    -> tdst, tot[b] = total
//   mode 2  the referenced flags of its vertices -> vnew, tot[B + b] = total
__global__ void __launch_bounds__(SIMP_SCAN_BLOCK) simp_scan_kernel(SimpDev s, int mode, int all) {
    __shared__ unsigned wsum[SIMP_SCAN_BLOCK / 64];
    const int b = blockIdx.x;
    const SimpMesh me = s.mesh[b];
    if (!all && !me.active) return;
    const int n = mode == 1 ? me.nt : me.nv, off = mode == 1 ? me.toff : me.voff;
    const unsigned run = block_scan_rounds<SIMP_SCAN_BLOCK / 64>(
        (unsigned)(n > 0 ? n : 0), wsum,
        [&](unsigned i) { return mode == 0 ? (unsigned)s.tcount[off + i] : mode == 1 ? (s.tdel[off + i] ? 0u : 1u) : (unsigned)s.vflag[off + i]; },
        [&](unsigned i, unsigned pre) {
            if (mode == 0) { s.tstart[off + i] = me.roff + (int)pre; s.vcur[off + i] = 0; }
            else if (mode == 1) s.tdst[off + i] = (int)pre;
            else s.vnew[off + i] = (int)pre;
        });
    if (threadIdx.x == 0) {
        if (mode == 0) s.rused[b] = (int)run;
        else s.tot[(mode == 1 ? 0 : s.B) + b] = (int)run;
    }
}

__global__ void simp_list_fill_kernel(SimpDev s) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    int m;
    if (!simp_slot(s, i, false, m) || s.tdel[i]) return;
    for (int j = 0; j < 3; ++j) {
        const int v = s.tv[3 * (size_t)i + j];
        s.refs[s.tstart[v] + atomicAdd(s.vcur + v, 1)] = i << 2 | j;
    }
}

// ascending (triangle, corner) inside every list: the order in which the header's loops meet the entries
__global__ void simp_list_sort_kernel(SimpDev s) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i >= s.Vt) return;
    const SimpMesh& me = s.mesh[s.vmesh[i]];
    if (!me.active) return;
    int* r = s.refs + s.tstart[i];
    const int n = simp_list_len(s, i, me.rcap);
    for (int a = 1; a < n; ++a) {
        const int x = r[a];
        int b = a - 1;
        while (b >= 0 && r[b] > x) { r[b + 1] = r[b]; --b; }
        r[b + 1] = x;
    }
}

// ---- initialisation ----------------------------------------------------------------------------------------------------------
__global__ void simp_normals_kernel(SimpDev s) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    int m;
    if (!simp_slot(s, i, false, m)) return;
    const int* v = s.tv + 3 * (size_t)i;
    const double *p0 = s.P + 3 * (size_t)v[0], *p1 = s.P + 3 * (size_t)v[1], *p2 = s.P + 3 * (size_t)v[2];
    const double a[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, b[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    simp_normalize(n);
    s.tn[3 * (size_t)i] = n[0]; s.tn[3 * (size_t)i + 1] = n[1]; s.tn[3 * (size_t)i + 2] = n[2];
}

__global__ void simp_quadric_kernel(SimpDev s) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i >= s.Vt) return;
    const SimpMesh& me = s.mesh[s.vmesh[i]];
    if (!me.active) return;
    double q[10];
    for (int m = 0; m < 10; ++m) q[m] = 0.0;
    const int start = s.tstart[i], n = simp_list_len(s, i, me.rcap);
    for (int k = 0; k < n; ++k) {
        const int t = s.refs[start + k] >> 2;
        const double* tn = s.tn + 3 * (size_t)t;
        const double* p0 = s.P + 3 * (size_t)s.tv[3 * (size_t)t];
        const double a = tn[0], b = tn[1], c = tn[2];
        const double d = -(p0[0] * a + p0[1] * b + p0[2] * c);
        const double plane[10] = {a * a, a * b, a * c, a * d, b * b, b * c, b * d, c * c, c * d, d * d};
        for (int m = 0; m < 10; ++m) q[m] = q[m] + plane[m];
    }
    for (int m = 0; m < 10; ++m) s.Q[10 * (size_t)i + m] = q[m];
}

// a neighbour met exactly once among the corners of a vertex's incident faces is a border vertex (border was zeroed)
__global__ void simp_border_kernel(SimpDev s) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i >= s.Vt) return;
    const SimpMesh& me = s.mesh[s.vmesh[i]];
    if (!me.active) return;
    const int start = s.tstart[i], n = simp_list_len(s, i, me.rcap);
    for (int k = 0; k < 3 * n; ++k) {
        const int id = s.tv[3 * (size_t)(s.refs[start + k / 3] >> 2) + k % 3];
        int seen = 0;
        for (int l = 0; l < 3 * n && seen < 2; ++l) seen += s.tv[3 * (size_t)(s.refs[start + l / 3] >> 2) + l % 3] == id;
        if (seen == 1) s.border[id] = 1;
    }
}

__global__ void simp_errors_kernel(SimpDev s) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    int m;
    if (!simp_slot(s, i, false, m)) return;
    simp_errors(s, i);
}

// ---- compaction of the triangle records (update_mesh(iteration > 0)); a mesh that is not active is copied through ----------
__global__ void simp_compact_kernel(SimpDev s) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    int m;
    if (!simp_slot(s, i, true, m)) return;
    const SimpMesh& me = s.mesh[m];
    int d = i, del = s.tdel[i];
    if (me.active) {
        if (del) return;
        d = me.toff + s.tdst[i];
    }
    for (int j = 0; j < 3; ++j) { s.tv2[3 * (size_t)d + j] = s.tv[3 * (size_t)i + j]; s.tn2[3 * (size_t)d + j] = s.tn[3 * (size_t)i + j]; }
    for (int j = 0; j < 4; ++j) s.terr2[4 * (size_t)d + j] = s.terr[4 * (size_t)i + j];
    s.tdel2[d] = del;
}

// ---- a pass ------------------------------------------------------------------------------------------------------------------
__global__ void simp_mark_kernel(SimpDev s, double thr) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    int m = 0;
    bool cand = false;
    if (simp_slot(s, i, false, m)) {
        s.tdirty[i] = 0;
        s.logdel[i] = 0;
        cand = !(s.terr[4 * (size_t)i + 3] > thr) && !s.tdel[i] && i - s.mesh[m].toff <= s.mesh[m].limit;
        s.pend[i] = cand;
    } else if (i < s.Tt) {
        s.pend[i] = 0;
    }
    simp_count_add(s.cand, m, cand);
}

// calls f(vertex) for every vertex of every live face around the three vertices of triangle i; stops when f returns false
template <typename F>
__device__ __forceinline__ bool simp_walk(const SimpDev& s, int i, int rcap, F f) {
    for (int j = 0; j < 3; ++j) {
        const int v = s.tv[3 * (size_t)i + j];
        const int start = s.tstart[v], n = simp_list_len(s, v, rcap);
        for (int k = 0; k < n; ++k) {
            const int t = s.refs[start + k] >> 2;
            if (s.tdel[t]) continue;
            for (int c = 0; c < 3; ++c)
                if (!f(s.tv[3 * (size_t)t + c])) return false;
        }
    }
    return true;
}

__device__ __forceinline__ unsigned long long simp_key(unsigned tag, int i) {
    return (unsigned long long)tag << 32 | (0xFFFFFFFFu - (unsigned)i);
}

__global__ void simp_claim_kernel(SimpDev s, unsigned tag, int slot) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    int m = 0;
    bool pending = i < s.Tt && s.pend[i];
    if (pending) {
        m = s.tmesh[i];
        if (s.tdel[i] || s.tdirty[i]) { s.pend[i] = 0; pending = false; }
    }
    simp_count_add(s.ring + slot * s.B, m, pending);
    if (!pending) return;
    const unsigned long long key = simp_key(tag, i);
    simp_walk(s, i, s.mesh[m].rcap, [&](int w) { atomicMax(s.claim + w, key); return true; });
}

__global__ void simp_verify_kernel(SimpDev s, unsigned tag) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i >= s.Tt || !s.pend[i]) return;
    const unsigned long long key = simp_key(tag, i);
    s.win[i] = simp_walk(s, i, s.mesh[s.tmesh[i]].rcap, [&](int w) { return s.claim[w] == key; });
}

// `deleted[k]` of the header for entry r of `own`'s list: the face holds the other end of the edge
__device__ __forceinline__ bool simp_holds(const SimpDev& s, int r, int other) {
    const int t = r >> 2, c = r & 3;
    return s.tv[3 * (size_t)t + (c + 1) % 3] == other || s.tv[3 * (size_t)t + (c + 2) % 3] == other;
}

// update_triangles for the list [start, start + n) of one end; survivors are appended at refs[dst + w]
__device__ void simp_update_triangles(const SimpDev& s, int i0, int other, int start, int n, int dst, int& w, int& deleted) {
    for (int k = 0; k < n; ++k) {
        const int r = s.refs[start + k], t = r >> 2;
        if (s.tdel[t]) continue;
        if (simp_holds(s, r, other)) { s.tdel[t] = 1; ++deleted; continue; }
        s.tv[3 * (size_t)t + (r & 3)] = i0;
        s.tdirty[t] = 1;
        simp_errors(s, t);
        s.refs[dst + w++] = r;
    }
}

__global__ void simp_execute_kernel(SimpDev s, double thr) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i >= s.Tt || !s.pend[i] || !s.win[i]) return;
    const int m = s.tmesh[i];
    const SimpMesh& me = s.mesh[m];
    const int v[3] = {s.tv[3 * (size_t)i], s.tv[3 * (size_t)i + 1], s.tv[3 * (size_t)i + 2]};
    const double e[3] = {s.terr[4 * (size_t)i], s.terr[4 * (size_t)i + 1], s.terr[4 * (size_t)i + 2]};
    for (int j = 0; j < 3; ++j) {
        if (!(e[j] < thr)) continue;
        const int i0 = v[j], i1 = v[(j + 1) % 3];
        if (s.border[i0] != s.border[i1]) continue;
        double p[3];
        simp_calculate_error(s, i0, i1, p);
        if (simp_flipped(s, p, i0, i1, me.rcap)) continue;
        if (simp_flipped(s, p, i1, i0, me.rcap)) continue;
        const int s0 = s.tstart[i0], n0 = simp_list_len(s, i0, me.rcap), s1 = s.tstart[i1], n1 = simp_list_len(s, i1, me.rcap);
        int count = 0;
        for (int k = 0; k < n0; ++k) { const int r = s.refs[s0 + k]; count += !s.tdel[r >> 2] && !simp_holds(s, r, i1); }
        for (int k = 0; k < n1; ++k) { const int r = s.refs[s1 + k]; count += !s.tdel[r >> 2] && !simp_holds(s, r, i0); }
        int dst = s0;                            // the header's "save ram": a list that did not grow is rewritten in place
        if (count > n0) {
            const int old = atomicAdd(s.rused + m, count);
            if (old + count > me.rcap) {         // no room: nothing has been changed, the triangle stays pending
                atomicSub(s.rused + m, count);
                s.ovf[m] = 1;
                return;
            }
            dst = me.roff + old;
        }
        for (int c = 0; c < 3; ++c) s.P[3 * (size_t)i0 + c] = p[c];
        for (int c = 0; c < 10; ++c) s.Q[10 * (size_t)i0 + c] = s.Q[10 * (size_t)i1 + c] + s.Q[10 * (size_t)i0 + c];
        int w = 0, deleted = 0;
        simp_update_triangles(s, i0, i1, s0, n0, dst, w, deleted);
        simp_update_triangles(s, i0, i0, s1, n1, dst, w, deleted);
        s.tstart[i0] = dst;
        s.tcount[i0] = w;
        s.logdel[i] = deleted;
        atomicAdd(s.ndel + m, deleted);
        break;
    }
    s.pend[i] = 0;
}

// one workgroup per mesh that crossed its budget: budget[2 b] = the triangle (local index) at which the prefix sum of the logged
// deletions, in index order, reaches `need`; budget[2 b + 1] = the last triangle that logged a collapse
__global__ void __launch_bounds__(SIMP_BLOCK) simp_budget_kernel(SimpDev s) {
    __shared__ unsigned wsum[SIMP_BLOCK / 64];
    __shared__ int last;
    const int b = blockIdx.x;
    const SimpMesh me = s.mesh[b];
    if (!me.active || me.need <= 0) return;
    if (threadIdx.x == 0) { last = -1; s.budget[2 * b] = -1; }
    __syncthreads();
    unsigned run = 0;
    int mine = -1;
    for (int c = 0; c < me.nt; c += SIMP_BLOCK) {
        const int i = c + (int)threadIdx.x;
        const unsigned x = i < me.nt ? (unsigned)s.logdel[me.toff + i] : 0u;
        unsigned total;
        const unsigned pre = run + block_excl<SIMP_BLOCK / 64>(x, wsum, total);
        if (x > 0) {
            mine = i;
            if (pre < (unsigned)me.need && pre + x >= (unsigned)me.need) s.budget[2 * b] = i;
        }
        run += total;
        __syncthreads();
    }
    if (mine >= 0) atomicMax(&last, mine);
    __syncthreads();
    if (threadIdx.x == 0) s.budget[2 * b + 1] = last;
}

// ---- compact_mesh ------------------------------------------------------------------------------------------------------------
__global__ void simp_used_kernel(SimpDev s) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    int m;
    if (!simp_slot(s, i, true, m) || s.tdel[i]) return;
    for (int j = 0; j < 3; ++j) s.vflag[s.tv[3 * (size_t)i + j]] = 1;
}

__global__ void simp_emit_vertices_kernel(SimpDev s, double* out) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    if (i >= s.Vt || !s.vflag[i]) return;
    const size_t d = (size_t)s.mesh[s.vmesh[i]].ovoff + s.vnew[i];
    for (int c = 0; c < 3; ++c) out[3 * d + c] = s.P[3 * (size_t)i + c];
}

__global__ void simp_emit_faces_kernel(SimpDev s, int* out) {
    const int i = blockIdx.x * SIMP_BLOCK + threadIdx.x;
    int m;
    if (!simp_slot(s, i, true, m) || s.tdel[i]) return;
    const size_t d = (size_t)s.mesh[m].otoff + s.tdst[i];
    for (int j = 0; j < 3; ++j) out[3 * d + j] = s.vnew[s.tv[3 * (size_t)i + j]];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static long long simplify_ref_capacity(int n_triangles_of_mesh, int ref_extra) {
    return 3LL * n_triangles_of_mesh + (ref_extra < 0 ? 3LL * n_triangles_of_mesh + SIMP_MIN_REF_EXTRA : ref_extra);
}

namespace {
// carves the workspace; with base == nullptr only the size is computed.  `snap` receives the copies taken before a pass.
size_t simp_carve(uint8_t* base, int B, size_t Vt, size_t Tt, size_t R, SimpDev* d, SimpDev* snap) {
    WsLayout L;
    SimpDev dev{}, sn{};
    auto f64 = [&](size_t n) { return reinterpret_cast<double*>(base + L.take<double>(n)); };
    auto i32 = [&](size_t n) { return reinterpret_cast<int*>(base + L.take<int>(n)); };
    dev.P = f64(3 * Vt); dev.Q = f64(10 * Vt); dev.terr = f64(4 * Tt); dev.tn = f64(3 * Tt); dev.terr2 = f64(4 * Tt); dev.tn2 = f64(3 * Tt);
    sn.P = f64(3 * Vt); sn.Q = f64(10 * Vt); sn.terr = f64(4 * Tt);
    dev.claim = reinterpret_cast<unsigned long long*>(base + L.take<unsigned long long>(Vt));
    dev.border = i32(Vt); dev.tstart = i32(Vt); dev.tcount = i32(Vt); dev.vcur = i32(Vt); dev.vmesh = i32(Vt); dev.vflag = i32(Vt);
    dev.vnew = i32(Vt);
    sn.tstart = i32(Vt); sn.tcount = i32(Vt);
    dev.tv = i32(3 * Tt); dev.tv2 = i32(3 * Tt); dev.tdel = i32(Tt); dev.tdel2 = i32(Tt); dev.tdirty = i32(Tt); dev.pend = i32(Tt);
    dev.win = i32(Tt); dev.logdel = i32(Tt); dev.tmesh = i32(Tt); dev.tdst = i32(Tt);
    sn.tv = i32(3 * Tt); sn.tdel = i32(Tt);
    dev.refs = i32(R); sn.refs = i32(R);
    // the ctl block: rused, ndel | cand, ovf, ring | tot, budget, err  (the middle part is zeroed before every batch of rounds)
    const size_t nb = (size_t)B;
    int* ctl = i32(nb * (2 + 2 + SIMP_BATCH + 2 + 2) + 1);
    dev.rused = ctl; dev.ndel = ctl + nb; dev.cand = ctl + 2 * nb; dev.ovf = ctl + 3 * nb; dev.ring = ctl + 4 * nb;
    dev.tot = ctl + (4 + SIMP_BATCH) * nb; dev.budget = dev.tot + 2 * nb; dev.err = dev.budget + 2 * nb;
    sn.rused = i32(2 * nb); sn.ndel = sn.rused + nb;
    dev.mesh = reinterpret_cast<SimpMesh*>(base + L.take<SimpMesh>(nb));
    if (d) *d = dev;
    if (snap) *snap = sn;
    return L.total;
}
}  // namespace

#define SIMP_HIP(call)                      \
    do {                                    \
        if ((call) != hipSuccess) return -10; \
    } while (0)

namespace {
struct SimpHost {
    SimpDev d, snap;
    std::vector<SimpMesh> mesh;
    hipStream_t st;
    unsigned tag = 0;
    int gv, gt;                                  // grids over the vertices / the triangle slots
    std::vector<int> rounds, repeats, rebuilds, iterations;

    int upload() {
        SIMP_HIP(hipMemcpyAsync(d.mesh, mesh.data(), mesh.size() * sizeof(SimpMesh), hipMemcpyHostToDevice, st));
        SIMP_HIP(hipStreamSynchronize(st));      // (the host copy changes again before the next readback)
        return 0;
    }
    int download(void* host, const void* dev, size_t bytes) {
        SIMP_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
        SIMP_HIP(hipStreamSynchronize(st));
        return 0;
    }
    // the lists of the active meshes from their live faces
    void build_lists(bool sorted) {
        GIGA_LAUNCH(simp_list_zero_kernel, dim3(gv), dim3(SIMP_BLOCK), 0, st, d);
        GIGA_LAUNCH(simp_list_count_kernel, dim3(gt), dim3(SIMP_BLOCK), 0, st, d);
        GIGA_LAUNCH(simp_scan_kernel, dim3(d.B), dim3(SIMP_SCAN_BLOCK), 0, st, d, 0, 0);
        GIGA_LAUNCH(simp_list_fill_kernel, dim3(gt), dim3(SIMP_BLOCK), 0, st, d);
        if (sorted) GIGA_LAUNCH(simp_list_sort_kernel, dim3(gv), dim3(SIMP_BLOCK), 0, st, d);
    }
    void swap_triangles() {
        std::swap(d.tv, d.tv2); std::swap(d.terr, d.terr2); std::swap(d.tn, d.tn2); std::swap(d.tdel, d.tdel2);
    }
    int copy(void* dst, const void* src, size_t bytes) {
        if (bytes) SIMP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    // copies the part of the state that a pass changes: all of it (b < 0, forward) or mesh b's ranges (back)
    int snapshot(int b) {
        const bool back = b >= 0;
        const size_t v0 = back ? mesh[b].voff : 0, nv = back ? mesh[b].nv : d.Vt, t0 = back ? mesh[b].toff : 0, nt = back ? mesh[b].nt : d.Tt;
        const size_t r0 = back ? mesh[b].roff : 0, nr = back ? mesh[b].rcap : (size_t)(mesh.back().roff + mesh.back().rcap);
        const size_t m0 = back ? b : 0, nm = back ? 1 : mesh.size();
        const SimpDev &from = back ? snap : d, &to = back ? d : snap;
        if (int rc = copy(to.P + 3 * v0, from.P + 3 * v0, 3 * nv * sizeof(double))) return rc;
        if (int rc = copy(to.Q + 10 * v0, from.Q + 10 * v0, 10 * nv * sizeof(double))) return rc;
        if (int rc = copy(to.tstart + v0, from.tstart + v0, nv * sizeof(int))) return rc;
        if (int rc = copy(to.tcount + v0, from.tcount + v0, nv * sizeof(int))) return rc;
        if (int rc = copy(to.terr + 4 * t0, from.terr + 4 * t0, 4 * nt * sizeof(double))) return rc;
        if (int rc = copy(to.tv + 3 * t0, from.tv + 3 * t0, 3 * nt * sizeof(int))) return rc;
        if (int rc = copy(to.tdel + t0, from.tdel + t0, nt * sizeof(int))) return rc;
        if (int rc = copy(to.refs + r0, from.refs + r0, nr * sizeof(int))) return rc;
        if (int rc = copy(to.rused + m0, from.rused + m0, nm * sizeof(int))) return rc;
        return copy(to.ndel + m0, from.ndel + m0, nm * sizeof(int));
    }

    // one pass over the active meshes (mesh[] is uploaded); rounds until no triangle is pending
    int run_pass(double thr) {
        const int B = d.B;
        SIMP_HIP(hipMemsetAsync(d.cand, 0, (size_t)B * (2 + SIMP_BATCH) * sizeof(int), st));
        GIGA_LAUNCH(simp_mark_kernel, dim3(gt), dim3(SIMP_BLOCK), 0, st, d, thr);
        std::vector<int> back((size_t)B * (2 + SIMP_BATCH)), cand(B, -1), used(B, 0), stuck(B, -1);
        for (bool first = true;; first = false) {
            if (!first) SIMP_HIP(hipMemsetAsync(d.ovf, 0, (size_t)B * (1 + SIMP_BATCH) * sizeof(int), st));
            for (int k = 0; k < SIMP_BATCH; ++k) {
                ++tag;
                GIGA_LAUNCH(simp_claim_kernel, dim3(gt), dim3(SIMP_BLOCK), 0, st, d, tag, k);
                GIGA_LAUNCH(simp_verify_kernel, dim3(gt), dim3(SIMP_BLOCK), 0, st, d, tag);
                GIGA_LAUNCH(simp_execute_kernel, dim3(gt), dim3(SIMP_BLOCK), 0, st, d, thr);
            }
            if (int rc = download(back.data(), d.cand, back.size() * sizeof(int))) return rc;
            if (first) for (int b = 0; b < B; ++b) cand[b] = back[b];
            const int* ovf = back.data() + B;
            const int* ring = back.data() + 2 * B;
            bool pending = false, overflow = false;
            for (int b = 0; b < B; ++b) {
                for (int k = 0; k < SIMP_BATCH; ++k)
                    if (ring[k * B + b] > 0) { ++rounds[b]; ++used[b]; }
                const int left = ring[(SIMP_BATCH - 1) * B + b];
                pending |= left > 0;
                if (ovf[b]) {
                    // nothing retired since the last rebuild: the room beyond the live lists is too small for one collapse
                    if (stuck[b] == left) return -12;
                    stuck[b] = left;
                    ++rebuilds[b];
                    used[b] -= SIMP_BATCH;       // (the rounds of a batch that overflowed are not held against the bound)
                    overflow = true;
                }
                if (used[b] > cand[b]) return -12;      // cannot happen: the lowest pending triangle always wins
            }
            if (overflow) build_lists(false);
            if (!pending) return 0;              // (a round without pending triangles changes nothing)
        }
    }
};
}  // namespace

static int launch_mesh_simplify(const void* vertices, int vertices_f64, const int* vertex_offsets, const int* triangles,
                                const int* triangle_offsets, const int* targets, int B, double agressiveness, int ref_extra,
                                double* out_vertices, int* out_triangles, int* out_counts, int* stats, uint8_t* ws, hipStream_t st) {
    SimpHost h;
    h.st = st;
    h.mesh.resize(B);
    long long R = 0;
    for (int b = 0; b < B; ++b) {
        SimpMesh& me = h.mesh[b];
        me = SimpMesh{};
        me.voff = vertex_offsets[b]; me.nv = vertex_offsets[b + 1] - vertex_offsets[b];
        me.toff = triangle_offsets[b]; me.nt = triangle_offsets[b + 1] - triangle_offsets[b];
        me.roff = (int)R; me.rcap = (int)simplify_ref_capacity(me.nt, ref_extra);
        me.limit = INT_MAX;
        R += me.rcap;
    }
    const int Vt = vertex_offsets[B], Tt = triangle_offsets[B];
    std::vector<int> counts(2 * (size_t)B, 0);
    h.rounds.assign(B, 0); h.repeats.assign(B, 0); h.rebuilds.assign(B, 0); h.iterations.assign(B, 0);
    auto finish = [&]() {
        if (stats)
            for (int b = 0; b < B; ++b) {
                stats[4 * b] = h.iterations[b]; stats[4 * b + 1] = h.rounds[b]; stats[4 * b + 2] = h.repeats[b];
                stats[4 * b + 3] = h.rebuilds[b];
            }
    };
    if (Tt == 0) {                               // no face at all: every face list is empty and no vertex is referenced
        SIMP_HIP(hipMemsetAsync(out_counts, 0, 2 * (size_t)B * sizeof(int), st));
        finish();
        return 0;
    }
    if (Vt == 0) return -11;
    simp_carve(ws, B, Vt, Tt, (size_t)R, &h.d, &h.snap);
    SimpDev& d = h.d;
    d.B = B; d.Vt = Vt; d.Tt = Tt;
    h.gv = (Vt + SIMP_BLOCK - 1) / SIMP_BLOCK;
    h.gt = (Tt + SIMP_BLOCK - 1) / SIMP_BLOCK;

    std::vector<int> deleted(B, 0), faces(B);
    std::vector<char> live(B);
    for (int b = 0; b < B; ++b) {
        faces[b] = h.mesh[b].nt;
        live[b] = faces[b] > targets[b];
        h.mesh[b].active = live[b];
    }
    if (int rc = h.upload()) return rc;
    SIMP_HIP(hipMemsetAsync(d.claim, 0, (size_t)Vt * sizeof(unsigned long long), st));
    SIMP_HIP(hipMemsetAsync(d.border, 0, (size_t)Vt * sizeof(int), st));
    SIMP_HIP(hipMemsetAsync(d.rused, 0, ((size_t)B * (8 + SIMP_BATCH) + 1) * sizeof(int), st));
    GIGA_LAUNCH(simp_widen_kernel, dim3(h.gv), dim3(SIMP_BLOCK), 0, st, d, vertices, vertices_f64);
    GIGA_LAUNCH(simp_faces_kernel, dim3(h.gt), dim3(SIMP_BLOCK), 0, st, d, triangles);
    int err = 0;
    if (int rc = h.download(&err, d.err, sizeof(int))) return rc;
    if (err) return -11;

    for (int iteration = 0; iteration < 100; ++iteration) {
        bool any = false;
        for (int b = 0; b < B; ++b) any |= (bool)live[b];
        if (!any) break;
        for (int b = 0; b < B; ++b) {
            h.mesh[b].active = live[b]; h.mesh[b].limit = INT_MAX; h.mesh[b].need = 0;
            h.iterations[b] += live[b];
        }
        if (int rc = h.upload()) return rc;
        if (iteration == 0) {                    // update_mesh(0)
            GIGA_LAUNCH(simp_normals_kernel, dim3(h.gt), dim3(SIMP_BLOCK), 0, st, d);
            h.build_lists(true);
            GIGA_LAUNCH(simp_quadric_kernel, dim3(h.gv), dim3(SIMP_BLOCK), 0, st, d);
            // the header rates the edges BEFORE it identifies the boundary: the first errors see border = 0 on every vertex
            // (value-initialised records), so even a boundary edge starts with the error of its optimal point
            GIGA_LAUNCH(simp_errors_kernel, dim3(h.gt), dim3(SIMP_BLOCK), 0, st, d);
            GIGA_LAUNCH(simp_border_kernel, dim3(h.gv), dim3(SIMP_BLOCK), 0, st, d);
        } else if (iteration % 5 == 0) {         // update_mesh(iteration): compact the triangles, rebuild the lists
            GIGA_LAUNCH(simp_scan_kernel, dim3(B), dim3(SIMP_SCAN_BLOCK), 0, st, d, 1, 0);
            GIGA_LAUNCH(simp_compact_kernel, dim3(h.gt), dim3(SIMP_BLOCK), 0, st, d);
            h.swap_triangles();
            std::vector<int> tot(B);
            if (int rc = h.download(tot.data(), d.tot, (size_t)B * sizeof(int))) return rc;
            for (int b = 0; b < B; ++b)
                if (live[b]) h.mesh[b].nt = tot[b];
            if (int rc = h.upload()) return rc;
            h.build_lists(false);
        }
        const double thr = 0.000000001 * std::pow(double(iteration + 3), agressiveness);
        if (int rc = h.snapshot(-1)) return rc;
        if (int rc = h.run_pass(thr)) return rc;
        std::vector<int> ndel(B);
        if (int rc = h.download(ndel.data(), d.ndel, (size_t)B * sizeof(int))) return rc;
        bool crossed = false;
        for (int b = 0; b < B; ++b) {
            h.mesh[b].active = live[b] && faces[b] - ndel[b] <= targets[b];
            h.mesh[b].need = h.mesh[b].active ? (faces[b] - deleted[b]) - targets[b] : 0;
            crossed |= (bool)h.mesh[b].active;
        }
        if (crossed) {
            if (int rc = h.upload()) return rc;
            GIGA_LAUNCH(simp_budget_kernel, dim3(B), dim3(SIMP_BLOCK), 0, st, d);
            std::vector<int> budget(2 * (size_t)B);
            if (int rc = h.download(budget.data(), d.budget, budget.size() * sizeof(int))) return rc;
            bool again = false;
            for (int b = 0; b < B; ++b) {
                const bool met = h.mesh[b].active;
                if (met) live[b] = 0;            // the budget is met in this pass: the mesh is finished after it
                h.mesh[b].active = met && budget[2 * b] >= 0 && budget[2 * b] != budget[2 * b + 1];
                if (h.mesh[b].active) {
                    h.mesh[b].limit = budget[2 * b];
                    ++h.repeats[b];
                    again = true;
                    if (int rc = h.snapshot(b)) return rc;
                }
            }
            if (again) {
                if (int rc = h.upload()) return rc;
                if (int rc = h.run_pass(thr)) return rc;
                if (int rc = h.download(ndel.data(), d.ndel, (size_t)B * sizeof(int))) return rc;
            }
        }
        deleted = ndel;
    }

    // compact_mesh: live faces in order, the vertices a live face refers to in index order, the faces renumbered
    SIMP_HIP(hipMemsetAsync(d.vflag, 0, (size_t)Vt * sizeof(int), st));
    GIGA_LAUNCH(simp_used_kernel, dim3(h.gt), dim3(SIMP_BLOCK), 0, st, d);
    GIGA_LAUNCH(simp_scan_kernel, dim3(B), dim3(SIMP_SCAN_BLOCK), 0, st, d, 1, 1);
    GIGA_LAUNCH(simp_scan_kernel, dim3(B), dim3(SIMP_SCAN_BLOCK), 0, st, d, 2, 1);
    std::vector<int> tot(2 * (size_t)B);
    if (int rc = h.download(tot.data(), d.tot, tot.size() * sizeof(int))) return rc;
    int ov = 0, ot = 0;
    for (int b = 0; b < B; ++b) {
        h.mesh[b].ovoff = ov; h.mesh[b].otoff = ot;
        counts[2 * b] = tot[B + b]; counts[2 * b + 1] = tot[b];
        ov += tot[B + b]; ot += tot[b];
    }
    if (int rc = h.upload()) return rc;
    GIGA_LAUNCH(simp_emit_vertices_kernel, dim3(h.gv), dim3(SIMP_BLOCK), 0, st, d, out_vertices);
    GIGA_LAUNCH(simp_emit_faces_kernel, dim3(h.gt), dim3(SIMP_BLOCK), 0, st, d, out_triangles);
    SIMP_HIP(hipMemcpyAsync(out_counts, counts.data(), counts.size() * sizeof(int), hipMemcpyHostToDevice, st));
    SIMP_HIP(hipStreamSynchronize(st));
    finish();
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // namespace giga

using namespace giga;

extern "C" {

// the reference-list entries of a batch of B meshes with n_triangles faces in all (every mesh: 3 F entries + the appended room)
static long long simplify_ref_total(int B, long long n_triangles, int ref_extra) {
    return ref_extra < 0 ? 6 * n_triangles + (long long)GIGA_SIMPLIFY_MIN_REF_EXTRA * B : 3 * n_triangles + (long long)ref_extra * B;
}
static int simplify_shape_check(int B, long long n_vertices, long long n_triangles, int ref_extra) {
    if (B < 0 || n_vertices < 0 || n_triangles < 0) return -1;
    if (ref_extra >= 0 && ref_extra < GIGA_SIMPLIFY_MIN_REF_EXTRA) return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    if (n_vertices > GIGA_SIMPLIFY_MAX_FACES || n_triangles > GIGA_SIMPLIFY_MAX_FACES) return -1;
    if (simplify_ref_total(B, n_triangles, ref_extra) >= (1LL << 31)) return -1;
    return 0;
}

size_t giga_simplify_workspace_bytes(int B, int n_vertices, int n_triangles, int ref_extra) {
    if (B <= 0 || simplify_shape_check(B, n_vertices, n_triangles, ref_extra) != 0) return 0;
    return simp_carve(nullptr, B, (size_t)n_vertices, (size_t)n_triangles, (size_t)simplify_ref_total(B, n_triangles, ref_extra), nullptr,
                      nullptr);
}

int giga_mesh_simplify(const void* vertices, int vertices_f64, const int32_t* vertex_offsets, const int32_t* triangles,
                       const int32_t* triangle_offsets, const int32_t* targets, int B, double agressiveness, int ref_extra,
                       double* out_vertices, int32_t* out_triangles, int32_t* out_counts, int32_t* stats, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (const int rc = ragged_batch_check(B)) return rc;
    if (B == 0) return 0;
    if (!(agressiveness == agressiveness) || (vertices_f64 != 0 && vertices_f64 != 1)) return -1;
    // (every check from here to the workspace pointer answers -1: simplify_shape_check has no other code once B is in range)
    if (!mesh_batch_check(vertex_offsets, triangle_offsets, B, vertices, triangles) || !targets || !workspace) return -1;
    if (const int rc = simplify_shape_check(B, vertex_offsets[B], triangle_offsets[B], ref_extra)) return rc;
    for (int b = 0; b < B; ++b)
        if (targets[b] < 0) return -1;
    if (!out_counts || (vertex_offsets[B] > 0 && triangle_offsets[B] > 0 && (!out_vertices || !out_triangles))) return -6;
    if (workspace_bytes < giga_simplify_workspace_bytes(B, vertex_offsets[B], triangle_offsets[B], ref_extra)) return -4;
    return launch_mesh_simplify(vertices, vertices_f64, vertex_offsets, triangles, triangle_offsets, targets, B, agressiveness, ref_extra,
                                out_vertices, out_triangles, out_counts, stats, static_cast<uint8_t*>(workspace),
                                static_cast<hipStream_t>(stream));
}

}  // extern "C"
