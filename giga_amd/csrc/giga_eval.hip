// Mesh evaluation on ragged batches (B scenes packed back to back, int32 offsets of length B + 1): the device counterpart of
// the reference's vgn.ConvONets.eval -- nearest neighbours between two point clouds (distance_p2p's KD-tree query), uniform
// surface samples with face normals (trimesh's mesh.sample / face_normals) and point-in-mesh (libmesh/inside_mesh.py).
//
//   nn        exact brute force on fp32 DIFFERENCES, (dx*dx + dy*dy) + dz*dz with one rounding per operation (no contraction
//             in this file).  A lane keeps NN_PTS source points in registers, the workgroup streams tiles of the scene's
//             targets through LDS (every lane reads the same target: a broadcast), running minimum and index in registers.
//             The targets are split over gridDim.y workgroups; partial results meet in a 64-bit atomicMin on
//             (bits of d2 << 32 | index): d2 >= 0, so the integer order is the order of (distance, index) and the result
//             does not depend on how the targets were split or on which workgroup came first.  Ties go to the lowest index.
//   sample    face areas (double) -> inclusive prefix sums inside the scene (one workgroup per scene, fixed order) -> per
//             sample one Philox-4x32-10 block keyed by (seed; sample, scene), a binary search for the first prefix sum
//             above r0 * total (a face without area is never the first), the barycentric point in double.
//   contains  the reference's ray-parity test in double, operation for operation; candidates are culled by the 2-D CELL test
//             the reference's triangle hash makes (a triangle is a candidate in every cell its bounding box touches), as
//             integer compares against tiles of cell ranges in LDS; the exact test runs on the few survivors.  The two hit
//             parities meet in an integer atomicXor (order independent).
// No float atomics anywhere: equal input gives equal bytes, a batch gives scene b the bytes of a call on scene b alone.
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "giga_check.h"
#include "giga_philox.h"
#include "giga_scan.h"
#include "giga_ws.h"
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace giga {

constexpr int EV_BLOCK = 256;
constexpr int NN_PTS = 4;             // source points per lane
constexpr int NN_TILE = 1024;         // targets per LDS tile (16 KB as float4)
constexpr int IN_PTS = 2;             // query points per lane of the containment kernel
constexpr int IN_TILE = 1024;         // triangles per LDS tile (16 KB as int4)
constexpr int EV_SCAN = 1024;
constexpr unsigned long long NN_NONE = 0x7f800000ffffffffull;     // (+inf, -1)
constexpr int EV_FILL_BLOCKS = 1024;  // split the inner set until a launch has about this many workgroups (256 CUs x 4)

static int ev_div_up(long long a, long long b) { return (int)((a + b - 1) / b); }

// ---------------------------------------------------------------------------------------------------------- nearest neighbour
__global__ __launch_bounds__(EV_BLOCK) void nn_init_kernel(unsigned long long* __restrict__ best, int n) {
    const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
    if (i < n) best[i] = NN_NONE;
}

__global__ __launch_bounds__(EV_BLOCK) void nn_query_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                             const int* __restrict__ so, const int* __restrict__ to,
                                                             int tiles_per_split, unsigned long long* __restrict__ best) {
    __shared__ float4 s_t[NN_TILE];
    const int scene = blockIdx.z;
    const int s0 = so[scene], ns = so[scene + 1] - s0, t0 = to[scene], nt = to[scene + 1] - t0;
    const int first = blockIdx.x * (EV_BLOCK * NN_PTS);
    const long long tb = (long long)blockIdx.y * tiles_per_split * NN_TILE;
    if (first >= ns || tb >= nt) return;                                  // uniform over the workgroup
    const int te = (int)(tb + (long long)tiles_per_split * NN_TILE < nt ? tb + (long long)tiles_per_split * NN_TILE : nt);
    float px[NN_PTS], py[NN_PTS], pz[NN_PTS], bd[NN_PTS];
    int bi[NN_PTS];
#pragma unroll
    for (int k = 0; k < NN_PTS; ++k) {
        const int i = first + k * EV_BLOCK + (int)threadIdx.x;
        const bool live = i < ns;
        const float* p = src + 3 * (size_t)(s0 + (live ? i : 0));
        px[k] = live ? p[0] : 0.f; py[k] = live ? p[1] : 0.f; pz[k] = live ? p[2] : 0.f;
        bd[k] = INFINITY;
        bi[k] = -1;
    }
    for (int base = (int)tb; base < te; base += NN_TILE) {
        const int cnt = te - base < NN_TILE ? te - base : NN_TILE;
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += EV_BLOCK) {
            const float* q = tgt + 3 * (size_t)(t0 + base + j);
            s_t[j] = make_float4(q[0], q[1], q[2], 0.f);
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const float4 q = s_t[j];
#pragma unroll
            for (int k = 0; k < NN_PTS; ++k) {
                const float dx = px[k] - q.x, dy = py[k] - q.y, dz = pz[k] - q.z;
                const float d = (dx * dx + dy * dy) + dz * dz;
                const bool lt = d < bd[k];                                 // strict: the lowest index keeps a tie
                bd[k] = lt ? d : bd[k];
                bi[k] = lt ? base + j : bi[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NN_PTS; ++k) {
        const int i = first + k * EV_BLOCK + (int)threadIdx.x;
        if (i < ns && bi[k] >= 0)
            atomicMin(&best[s0 + i], (unsigned long long)__float_as_uint(bd[k]) << 32 | (unsigned)bi[k]);
    }
}

__global__ __launch_bounds__(EV_BLOCK) void nn_final_kernel(const unsigned long long* __restrict__ best, int n,
                                                             float* __restrict__ dist, int* __restrict__ idx) {
    const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned long long b = best[i];
    dist[i] = sqrtf(__uint_as_float((unsigned)(b >> 32)));
    idx[i] = (int)(unsigned)b;
}

struct NnWs { size_t offs, best, total; };
static NnWs nn_workspace(int B, int n_src) {
    WsLayout L;
    NnWs w;
    w.offs = L.take<int>((size_t)2 * (B + 1));
    w.best = L.take<unsigned long long>((size_t)n_src);
    w.total = L.total;
    return w;
}

// how many ways to split `tiles` tiles of the inner set when the outer set alone gives `blocks` workgroups
static int ev_split(int tiles, long long blocks) {
    int want = (int)((EV_FILL_BLOCKS + blocks - 1) / blocks);
    if (want > tiles) want = tiles;
    return want < 1 ? 1 : want;
}

static int launch_nn_query(const float* src, const int* src_offsets, const float* tgt, const int* tgt_offsets, int B, float* dist,
                           int* idx, uint8_t* ws, hipStream_t s) {
    const int n_src = src_offsets[B] - src_offsets[0], base = src_offsets[0];
    if (n_src == 0) return 0;
    const NnWs w = nn_workspace(B, src_offsets[B]);
    int* so = reinterpret_cast<int*>(ws + w.offs);
    int* to = so + (B + 1);
    unsigned long long* best = reinterpret_cast<unsigned long long*>(ws + w.best);
    // (pageable host memory: the copy has left the caller's arrays when the call returns)
    if (hipMemcpyAsync(so, src_offsets, (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    if (hipMemcpyAsync(to, tgt_offsets, (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    const int nblk = ev_div_up(n_src, EV_BLOCK);
    GIGA_LAUNCH(nn_init_kernel, dim3(nblk), dim3(EV_BLOCK), 0, s, best + base, n_src);
    const int max_s = ragged_max_count(src_offsets, B), max_t = ragged_max_count(tgt_offsets, B);
    if (max_t > 0) {
        const int bx = ev_div_up(max_s, EV_BLOCK * NN_PTS), tiles = ev_div_up(max_t, NN_TILE);
        const int split = ev_split(tiles, (long long)bx * B), tps = ev_div_up(tiles, split);
        GIGA_LAUNCH(nn_query_kernel, dim3(bx, ev_div_up(tiles, tps), B), dim3(EV_BLOCK), 0, s, src, tgt, so, to, tps, best);
    }
    GIGA_LAUNCH(nn_final_kernel, dim3(nblk), dim3(EV_BLOCK), 0, s, best + base, n_src, dist + base, idx + base);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

// ------------------------------------------------------------------------------------------------------------ surface samples
struct Tri3 { double a[3], b[3], c[3]; bool ok; };

// the three corners of face f of a scene (vertex indices count from the scene's first vertex); ok = all indices in range
__device__ __forceinline__ Tri3 load_tri(const float* __restrict__ v, int nv, const int* __restrict__ t, int f) {
    Tri3 r;
    const int i0 = t[3 * (size_t)f], i1 = t[3 * (size_t)f + 1], i2 = t[3 * (size_t)f + 2];
    r.ok = (unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        r.a[q] = r.ok ? (double)v[3 * (size_t)i0 + q] : 0.0;
        r.b[q] = r.ok ? (double)v[3 * (size_t)i1 + q] : 0.0;
        r.c[q] = r.ok ? (double)v[3 * (size_t)i2 + q] : 0.0;
    }
    return r;
}

__device__ __forceinline__ void cross3(const double* x, const double* y, double* n) {
    n[0] = x[1] * y[2] - x[2] * y[1];
    n[1] = x[2] * y[0] - x[0] * y[2];
    n[2] = x[0] * y[1] - x[1] * y[0];
}

__global__ __launch_bounds__(EV_BLOCK) void sample_area_kernel(const float* __restrict__ vertices, const int* __restrict__ vo,
                                                                const int* __restrict__ triangles, const int* __restrict__ fo,
                                                                double* __restrict__ cum) {
    const int scene = blockIdx.y, f0 = fo[scene], nf = fo[scene + 1] - f0, f = blockIdx.x * EV_BLOCK + threadIdx.x;
    if (f >= nf) return;
    const Tri3 t = load_tri(vertices + 3 * (size_t)vo[scene], vo[scene + 1] - vo[scene], triangles + 3 * (size_t)f0, f);
    double e1[3], e2[3], n[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { e1[q] = t.b[q] - t.a[q]; e2[q] = t.c[q] - t.a[q]; }
    cross3(e1, e2, n);
    const double area = 0.5 * sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    cum[f0 + f] = (t.ok && area > 0.0 && area < INFINITY) ? area : 0.0;    // (NaN compares false)
}

// inclusive prefix sums of a scene's face areas, in place; the order of the additions depends on the face count alone:
// ((carry + wsum[0]) + ... + wsum[wave - 1]) + the wave's inclusive sum, which tests/eval_emu.py restates.  That order is part of
// the result, and it is not block_excl's (which starts from the in-wave prefix), so the loop over the waves is written out here.
__global__ __launch_bounds__(EV_SCAN) void sample_scan_kernel(double* __restrict__ cum, const int* __restrict__ fo, int n,
                                                               double* __restrict__ totals, int* __restrict__ counts) {
    __shared__ double wsum[EV_SCAN / 64];
    __shared__ double carry;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int scene = blockIdx.x, f0 = fo[scene], nf = fo[scene + 1] - f0;
    if (threadIdx.x == 0) carry = 0.0;
    __syncthreads();
    for (int base = 0; base < nf; base += EV_SCAN) {
        const int f = base + (int)threadIdx.x;
        const double own = f < nf ? cum[f0 + f] : 0.0;
        const double inc = wave_incl(own, lane);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        double pre = carry, all = 0.0;
#pragma unroll
        for (unsigned w = 0; w < EV_SCAN / 64; ++w) {
            if (w < wave) pre += wsum[w];
            all += wsum[w];
        }
        if (f < nf) cum[f0 + f] = pre + inc;
        __syncthreads();
        if (threadIdx.x == 0) carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // the scene's total as the search sees it: the last prefix sum
        const double total = nf > 0 ? cum[f0 + nf - 1] : 0.0;
        const bool usable = total > 0.0 && total < INFINITY;
        totals[scene] = usable ? total : 0.0;
        counts[scene] = usable ? n : 0;
    }
}

__global__ __launch_bounds__(EV_BLOCK) void sample_draw_kernel(const float* __restrict__ vertices, const int* __restrict__ vo,
                                                                const int* __restrict__ triangles, const int* __restrict__ fo,
                                                                const double* __restrict__ cum, const double* __restrict__ totals,
                                                                int n, unsigned long long seed, unsigned first_scene, float* __restrict__ points,
                                                                int* __restrict__ face, float* __restrict__ normals) {
    const int scene = blockIdx.y, i = blockIdx.x * EV_BLOCK + threadIdx.x;
    const double total = totals[scene];
    if (i >= n || !(total > 0.0)) return;
    const int f0 = fo[scene], nf = fo[scene + 1] - f0;
    const Philox r = philox4x32_10((unsigned)i, first_scene + (unsigned)scene, 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32));
    const double r0 = r.x[0] * 0x1p-32, r1 = r.x[1] * 0x1p-32, r2 = r.x[2] * 0x1p-32;
    const double x = r0 * total;
    const double* c = cum + f0;
    int lo = 0, hi = nf - 1;                      // first f with c[f] > x; c[nf-1] = total > x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] > x) hi = mid; else lo = mid + 1;
    }
    const Tri3 t = load_tri(vertices + 3 * (size_t)vo[scene], vo[scene + 1] - vo[scene], triangles + 3 * (size_t)f0, lo);
    const double sr = sqrt(r1), wa = 1.0 - sr, wb = sr * (1.0 - r2), wc = sr * r2;
    double e1[3], e2[3], nr[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { e1[q] = t.b[q] - t.a[q]; e2[q] = t.c[q] - t.a[q]; }
    cross3(e1, e2, nr);
    const double len = sqrt((nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2]);
    const size_t o = 3 * ((size_t)scene * n + i);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        points[o + q] = (float)((wa * t.a[q] + wb * t.b[q]) + wc * t.c[q]);
        normals[o + q] = (float)(nr[q] / len);
    }
    face[(size_t)scene * n + i] = lo;
}

struct SampleWs { size_t offs, cum, totals, total; };
static SampleWs sample_workspace(int B, int n_tri) {
    WsLayout L;
    SampleWs w;
    w.offs = L.take<int>((size_t)2 * (B + 1));
    w.cum = L.take<double>((size_t)n_tri);
    w.totals = L.take<double>((size_t)B);
    w.total = L.total;
    return w;
}

static int launch_mesh_sample(const float* vertices, const int* vertex_offsets, const int* triangles, const int* triangle_offsets, int B,
                              int n, unsigned long long seed, int first_scene, float* points, int* face, float* normals, int* counts,
                              uint8_t* ws, hipStream_t s) {
    const SampleWs w = sample_workspace(B, triangle_offsets[B]);
    int* vo = reinterpret_cast<int*>(ws + w.offs);
    int* fo = vo + (B + 1);
    double* cum = reinterpret_cast<double*>(ws + w.cum);
    double* totals = reinterpret_cast<double*>(ws + w.totals);
    if (hipMemcpyAsync(vo, vertex_offsets, (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    if (hipMemcpyAsync(fo, triangle_offsets, (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    const int max_f = ragged_max_count(triangle_offsets, B);
    if (max_f > 0)
        GIGA_LAUNCH(sample_area_kernel, dim3(ev_div_up(max_f, EV_BLOCK), B), dim3(EV_BLOCK), 0, s, vertices, vo, triangles, fo, cum);
    GIGA_LAUNCH(sample_scan_kernel, dim3(B), dim3(EV_SCAN), 0, s, cum, fo, n, totals, counts);
    if (n > 0 && max_f > 0)
        GIGA_LAUNCH(sample_draw_kernel, dim3(ev_div_up(n, EV_BLOCK), B), dim3(EV_BLOCK), 0, s, vertices, vo, triangles, fo, cum,
                    totals, n, seed, (unsigned)first_scene, points, face, normals);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

// ---------------------------------------------------------------------------------------------------------------- containment
constexpr int IN_FAR = 0x40000000;            // a cell no point and no triangle has

// per scene: bounding box of the vertices its faces use -> scale [3], translate [3] (inside_mesh.py:17-21)
__global__ __launch_bounds__(EV_SCAN) void contains_bbox_kernel(const float* __restrict__ vertices, const int* __restrict__ vo,
                                                                 const int* __restrict__ triangles, const int* __restrict__ fo,
                                                                 int resolution, double* __restrict__ xform) {
    __shared__ float s_lo[EV_SCAN / 64][3], s_hi[EV_SCAN / 64][3];
    const int scene = blockIdx.x, f0 = fo[scene], nf = fo[scene + 1] - f0, nv = vo[scene + 1] - vo[scene];
    const float* v = vertices + 3 * (size_t)vo[scene];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool nan = false;
    for (int f = threadIdx.x; f < nf; f += EV_SCAN) {
        const Tri3 t = load_tri(v, nv, triangles + 3 * (size_t)f0, f);
        if (!t.ok) continue;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float a = (float)t.a[q], b = (float)t.b[q], c = (float)t.c[q];
            nan |= !(a == a) || !(b == b) || !(c == c);                     // numpy's min / max hand a NaN on
            lo[q] = fminf(lo[q], fminf(a, fminf(b, c)));
            hi[q] = fmaxf(hi[q], fmaxf(a, fmaxf(b, c)));
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (nan) lo[q] = hi[q] = NAN;
        for (int o = 32; o > 0; o >>= 1) {
            const float l = __shfl_xor(lo[q], o, 64), h = __shfl_xor(hi[q], o, 64);
            lo[q] = (l != l || lo[q] != lo[q]) ? NAN : fminf(lo[q], l);
            hi[q] = (h != h || hi[q] != hi[q]) ? NAN : fmaxf(hi[q], h);
        }
        if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6][q] = lo[q]; s_hi[threadIdx.x >> 6][q] = hi[q]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int q = threadIdx.x;
        float l = s_lo[0][q], h = s_hi[0][q];
        for (int w = 1; w < EV_SCAN / 64; ++w) {
            l = (l != l || s_lo[w][q] != s_lo[w][q]) ? NAN : fminf(l, s_lo[w][q]);
            h = (h != h || s_hi[w][q] != s_hi[w][q]) ? NAN : fmaxf(h, s_hi[w][q]);
        }
        const double scale = (double)(resolution - 1) / ((double)h - (double)l);
        xform[6 * scene + q] = scale;
        xform[6 * scene + 3 + q] = 0.5 - scale * (double)l;
    }
}

// the reference's `<int> x` followed by min(max(., 0), resolution - 1), without the undefined conversions
__device__ __forceinline__ int cell_clamped(double x, int resolution) {
    const double t = trunc(x);
    return t <= 0.0 ? 0 : (t >= (double)(resolution - 1) ? resolution - 1 : (int)t);
}

// per face: the rescaled corners (9 doubles) and its cell range {x0, y0, x1 - x0, y1 - y0} (triangle_hash.pyx, _build_hash)
__global__ __launch_bounds__(EV_BLOCK) void contains_prep_kernel(const float* __restrict__ vertices, const int* __restrict__ vo,
                                                                  const int* __restrict__ triangles, const int* __restrict__ fo,
                                                                  int resolution, const double* __restrict__ xform,
                                                                  double* __restrict__ tri, int4* __restrict__ cells) {
    const int scene = blockIdx.y, f0 = fo[scene], nf = fo[scene + 1] - f0, f = blockIdx.x * EV_BLOCK + threadIdx.x;
    if (f >= nf) return;
    const Tri3 t = load_tri(vertices + 3 * (size_t)vo[scene], vo[scene + 1] - vo[scene], triangles + 3 * (size_t)f0, f);
    double r[9];
    bool ok = t.ok;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double sc = xform[6 * scene + q], tr = xform[6 * scene + 3 + q];
        r[q] = sc * t.a[q] + tr;
        r[3 + q] = sc * t.b[q] + tr;
        r[6 + q] = sc * t.c[q] + tr;
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        tri[9 * (size_t)(f0 + f) + q] = r[q];
        ok = ok && r[q] == r[q];
    }
    int4 c = make_int4(IN_FAR, IN_FAR, 0, 0);
    if (ok) {
        const int x0 = cell_clamped(fmin(r[0], fmin(r[3], r[6])), resolution), x1 = cell_clamped(fmax(r[0], fmax(r[3], r[6])), resolution);
        const int y0 = cell_clamped(fmin(r[1], fmin(r[4], r[7])), resolution), y1 = cell_clamped(fmax(r[1], fmax(r[4], r[7])), resolution);
        c = make_int4(x0, y0, x1 - x0, y1 - y0);
    }
    cells[f0 + f] = c;
}

__global__ __launch_bounds__(EV_BLOCK) void contains_init_kernel(unsigned* __restrict__ hits, int n) {
    const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
    if (i < n) hits[i] = 0u;
}

// check_triangles + compute_intersection_depth (inside_mesh.py:75-106, 129-153) for one point and one triangle, in the
// reference's operand order; returns 0 (no hit, or a vertical triangle), 1 (depth >= p.z |n.z|) or 0x10000 (depth < ...).
// Only the parity of each count matters, so the two counts are kept as two parity bits and combined by exclusive or
__device__ __forceinline__ unsigned ray_hit(const double* __restrict__ t, double px, double py, double pz) {
    const double a00 = t[0] - t[6], a01 = t[3] - t[6], a10 = t[1] - t[7], a11 = t[4] - t[7];
    const double y0 = px - t[6], y1 = py - t[7];
    const double det = a00 * a11 - a01 * a10;
    const double adet = fabs(det);
    if (!(adet != 0.0)) return 0u;
    const double sd = det > 0.0 ? 1.0 : -1.0;
    const double u = (a11 * y0 - a01 * y1) * sd;
    const double v = (-a10 * y0 + a00 * y1) * sd;
    const double uv = u + v;
    if (!(0.0 < u && u < adet && 0.0 < v && v < adet && 0.0 < uv && uv < adet)) return 0u;
    double v1[3], v2[3], n[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { v1[q] = t[6 + q] - t[q]; v2[q] = t[3 + q] - t[q]; }
    cross3(v1, v2, n);
    const double alpha = n[0] * (t[0] - px) + n[1] * (t[1] - py);
    const double an = fabs(n[2]);
    if (!(an != 0.0)) return 0u;                                            // NaN depth: neither side
    const double sn = n[2] > 0.0 ? 1.0 : -1.0;
    const double depth = t[2] * an + alpha * sn, ref = pz * an;
    return depth >= ref ? 1u : (depth < ref ? 0x10000u : 0u);
}

__global__ __launch_bounds__(EV_BLOCK) void contains_query_kernel(const double* __restrict__ points, const int* __restrict__ po,
                                                                   const int* __restrict__ fo, int resolution,
                                                                   const double* __restrict__ xform, const double* __restrict__ tri,
                                                                   const int4* __restrict__ cells, int tiles_per_split,
                                                                   unsigned* __restrict__ hits) {
    __shared__ int4 s_c[IN_TILE];
    const int scene = blockIdx.z;
    const int p0 = po[scene], np = po[scene + 1] - p0, f0 = fo[scene], nf = fo[scene + 1] - f0;
    const int first = blockIdx.x * (EV_BLOCK * IN_PTS);
    const long long tb = (long long)blockIdx.y * tiles_per_split * IN_TILE;
    if (first >= np || tb >= nf) return;
    const int te = (int)(tb + (long long)tiles_per_split * IN_TILE < nf ? tb + (long long)tiles_per_split * IN_TILE : nf);
    double px[IN_PTS], py[IN_PTS], pz[IN_PTS];
    int cx[IN_PTS], cy[IN_PTS];
    unsigned acc[IN_PTS];
#pragma unroll
    for (int k = 0; k < IN_PTS; ++k) {
        const int i = first + k * EV_BLOCK + (int)threadIdx.x;
        const bool live = i < np;
        const double* p = points + 3 * (size_t)(p0 + (live ? i : 0));
        px[k] = xform[6 * scene + 0] * p[0] + xform[6 * scene + 3];
        py[k] = xform[6 * scene + 1] * p[1] + xform[6 * scene + 4];
        pz[k] = xform[6 * scene + 2] * p[2] + xform[6 * scene + 5];
        const double res = (double)resolution;
        // inside_mesh.py:40-41 (0 <= p <= resolution on all axes), then triangle_hash.pyx:61-64 (0 <= int(p) < resolution)
        const bool in = live && 0.0 <= px[k] && px[k] <= res && 0.0 <= py[k] && py[k] <= res && 0.0 <= pz[k] && pz[k] <= res &&
                        px[k] < res && py[k] < res;
        cx[k] = in ? (int)px[k] : -IN_FAR;
        cy[k] = in ? (int)py[k] : -IN_FAR;
        acc[k] = 0u;
    }
    for (int base = (int)tb; base < te; base += IN_TILE) {
        const int cnt = te - base < IN_TILE ? te - base : IN_TILE;
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += EV_BLOCK) s_c[j] = cells[f0 + base + j];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const int4 c = s_c[j];
#pragma unroll
            for (int k = 0; k < IN_PTS; ++k) {
                if ((unsigned)(cx[k] - c.x) <= (unsigned)c.z && (unsigned)(cy[k] - c.y) <= (unsigned)c.w)
                    acc[k] ^= ray_hit(tri + 9 * (size_t)(f0 + base + j), px[k], py[k], pz[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < IN_PTS; ++k) {
        const int i = first + k * EV_BLOCK + (int)threadIdx.x;
        if (i < np && acc[k]) atomicXor(&hits[p0 + i], acc[k]);
    }
}

__global__ __launch_bounds__(EV_BLOCK) void contains_final_kernel(const unsigned* __restrict__ hits, int n, uint8_t* __restrict__ inside) {
    const int i = blockIdx.x * EV_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned h = hits[i];
    inside[i] = (uint8_t)((h & 1u) & (h >> 16 & 1u));
}

struct ContainsWs { size_t offs, xform, tri, cells, hits, total; };
static ContainsWs contains_workspace(int B, int n_tri, int n_pts) {
    WsLayout L;
    ContainsWs w;
    w.offs = L.take<int>((size_t)3 * (B + 1));
    w.xform = L.take<double>((size_t)B * 6);
    w.tri = L.take<double>((size_t)n_tri * 9);
    w.cells = L.take<int4>((size_t)n_tri);
    w.hits = L.take<unsigned>((size_t)n_pts);
    w.total = L.total;
    return w;
}

static int launch_mesh_contains(const float* vertices, const int* vertex_offsets, const int* triangles, const int* triangle_offsets,
                                const double* points, const int* point_offsets, int B, int resolution, uint8_t* inside, uint8_t* ws,
                                hipStream_t s) {
    const int n_pts = point_offsets[B] - point_offsets[0], pbase = point_offsets[0];
    if (n_pts == 0) return 0;
    const ContainsWs w = contains_workspace(B, triangle_offsets[B], point_offsets[B]);
    int* vo = reinterpret_cast<int*>(ws + w.offs);
    int* fo = vo + (B + 1);
    int* po = fo + (B + 1);
    double* xform = reinterpret_cast<double*>(ws + w.xform);
    double* tri = reinterpret_cast<double*>(ws + w.tri);
    int4* cells = reinterpret_cast<int4*>(ws + w.cells);
    unsigned* hits = reinterpret_cast<unsigned*>(ws + w.hits);
    if (hipMemcpyAsync(vo, vertex_offsets, (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    if (hipMemcpyAsync(fo, triangle_offsets, (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    if (hipMemcpyAsync(po, point_offsets, (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    const int nblk = ev_div_up(n_pts, EV_BLOCK);
    GIGA_LAUNCH(contains_init_kernel, dim3(nblk), dim3(EV_BLOCK), 0, s, hits + pbase, n_pts);
    const int max_f = ragged_max_count(triangle_offsets, B), max_p = ragged_max_count(point_offsets, B);
    if (max_f > 0) {
        GIGA_LAUNCH(contains_bbox_kernel, dim3(B), dim3(EV_SCAN), 0, s, vertices, vo, triangles, fo, resolution, xform);
        GIGA_LAUNCH(contains_prep_kernel, dim3(ev_div_up(max_f, EV_BLOCK), B), dim3(EV_BLOCK), 0, s, vertices, vo, triangles, fo,
                    resolution, xform, tri, cells);
        const int bx = ev_div_up(max_p, EV_BLOCK * IN_PTS), tiles = ev_div_up(max_f, IN_TILE);
        const int split = ev_split(tiles, (long long)bx * B), tps = ev_div_up(tiles, split);
        GIGA_LAUNCH(contains_query_kernel, dim3(bx, ev_div_up(tiles, tps), B), dim3(EV_BLOCK), 0, s, points, po, fo, resolution,
                    xform, tri, cells, tps, hits);
    }
    GIGA_LAUNCH(contains_final_kernel, dim3(nblk), dim3(EV_BLOCK), 0, s, hits + pbase, n_pts, inside + pbase);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // namespace giga

using namespace giga;

extern "C" {

size_t giga_nn_query_workspace_bytes(int B, int n_src) {
    if (B <= 0 || B > GIGA_MAX_SCENES || n_src < 0) return 0;
    return nn_workspace(B, n_src).total;
}

int giga_nn_query(const float* src, const int32_t* src_offsets, const float* tgt, const int32_t* tgt_offsets, int B, float* dist,
                  int32_t* idx, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = ragged_batch_check(B)) return rc;
    if (B == 0) return 0;
    if (!ragged_ok(src_offsets, B) || !ragged_ok(tgt_offsets, B)) return -1;
    if (src_offsets[B] == 0) return 0;
    if (!src || (tgt_offsets[B] > 0 && !tgt) || !workspace) return -1;
    if (!dist || !idx) return -6;
    if (workspace_bytes < giga_nn_query_workspace_bytes(B, src_offsets[B])) return -4;
    return launch_nn_query(src, src_offsets, tgt, tgt_offsets, B, dist, idx, static_cast<uint8_t*>(workspace),
                           static_cast<hipStream_t>(stream));
}

size_t giga_mesh_sample_workspace_bytes(int B, int n_triangles) {
    if (B <= 0 || B > GIGA_MAX_SCENES || n_triangles < 0) return 0;
    return sample_workspace(B, n_triangles).total;
}

int giga_mesh_sample(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                     int B, int n, uint64_t seed, int first_scene, float* points, int32_t* face, float* normals, int32_t* counts,
                     void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = ragged_batch_check(B)) return rc;
    if (n < 0 || first_scene < 0 || (long long)B * n >= (1LL << 31)) return -1;
    if (B == 0) return 0;
    if (!mesh_batch_check(vertex_offsets, triangle_offsets, B, vertices, triangles) || !workspace) return -1;
    if (!counts || (n > 0 && (!points || !face || !normals))) return -6;
    if (workspace_bytes < giga_mesh_sample_workspace_bytes(B, triangle_offsets[B])) return -4;
    return launch_mesh_sample(vertices, vertex_offsets, triangles, triangle_offsets, B, n, seed, first_scene, points, face, normals, counts,
                              static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

size_t giga_mesh_contains_workspace_bytes(int B, int n_triangles, int n_points) {
    if (B <= 0 || B > GIGA_MAX_SCENES || n_triangles < 0 || n_points < 0) return 0;
    return contains_workspace(B, n_triangles, n_points).total;
}

int giga_mesh_contains(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                       const double* points, const int32_t* point_offsets, int B, int resolution, uint8_t* inside, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (const int rc = ragged_batch_check(B)) return rc;
    if (resolution < 2 || resolution > GIGA_CONTAINS_MAX_RESOLUTION) return -1;
    if (B == 0) return 0;
    if (!ragged_ok(vertex_offsets, B) || !ragged_ok(triangle_offsets, B) || !ragged_ok(point_offsets, B)) return -1;
    if (point_offsets[B] == 0) return 0;                    // (whatever the data pointers: only the offsets are looked at before)
    if (!mesh_batch_check(vertex_offsets, triangle_offsets, B, vertices, triangles) || !points || !workspace) return -1;
    if (!inside) return -6;
    if (workspace_bytes < giga_mesh_contains_workspace_bytes(B, triangle_offsets[B], point_offsets[B])) return -4;
    return launch_mesh_contains(vertices, vertex_offsets, triangles, triangle_offsets, points, point_offsets, B, resolution, inside,
                                static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

}  // extern "C"
