// Grasp affordance of a scene mesh: the device counterpart of affordance_visual (reference src/vgn/utils/visual.py:22-98), which
// colours every face of the scene mesh by the grasp quality the network predicts near it.  The reference is a dense faces x points
// reduction in numpy over (F, P, 3) float64 temporaries; the semantics kept here are spelled out in include/giga_hip.h
// (giga_affordance_points / giga_affordance_faces).  Every operation is one IEEE rounding -- no contraction in this file -- so
// that a numpy restatement reproduces the bytes of the points, of the 'max' affordance and of its colours (tests/affordance_emu.py).
//
//   points   a stream compaction of the voxels with q > th in voxel order: count per 256 voxels, scan per scene, emit
//            (giga_scan.h: prefixes by shuffles, no atomics).
//   faces    one workgroup per 256 faces of one scene, one face per lane.
//     dense  the scene's points pass through LDS 256 at a time as (x, y, z, q, w); every lane reads the same record, so the read
//            is a broadcast.  w is what depends on the point alone (exp(q temp) of 'softmax'), computed once per staged point.
//            The sums run in ascending point order in every lane.
//     grid   'max' needs only the points within rad, and a maximum does not depend on the order.  One workgroup per scene sorts
//            the points by the cell of a uniform grid (a stable radix sort, one bit per pass, positions by scans) and writes
//            where each cell starts; a lane then walks the 3 x 3 columns around its face centre, each column being ONE run of the
//            sorted order because z is the fastest cell coordinate.  The cells are wider than rad by a factor 1 + 2^-20 and every
//            step of the cell assignment is monotone, so a point within rad of a centre (rounding of the distance included, which is
//            a few 2^-53) is never more than one cell away; a point that the walk does not reach fails dist <= rad anyway.  The
//            test itself is the same expression on the same numbers as in the dense form, so the grid changes no bit.
//            ('softmax' must sum in ascending point order, which a walk over cells does not give; a grid form that listed the
//            points in range per lane and summed over the sorted list was measured at twice the dense form's time on the timing
//            tool's scene and is not kept: DESIGN.md section 3q.)
//   dist <= rad is evaluated as d2 <= T, where d2 is the rounded sum of squares and T the largest double whose correctly rounded
//   square root is <= rad (found on the host): sqrt is monotone, so the two tests agree for every d2, and 'max' and 'softmax' need
//   no square root.  'mean' takes the correctly rounded root.
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "giga_check.h"
#include "giga_scan.h"
#include "giga_ws.h"
#include "../../include/giga_hip.h"
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace giga {

#pragma clang fp contract(off)

constexpr int AFF_BLOCK = 256;                    // voxels per compaction block, faces per workgroup, points per LDS tile
constexpr int AFF_WAVES = AFF_BLOCK / 64;
constexpr int AFF_SORT_BLOCK = 1024;              // the one workgroup that sorts a scene's points
constexpr int AFF_SORT_WAVES = AFF_SORT_BLOCK / 64;
constexpr int AFF_GRID_MAX = 32;                  // cells per axis at most: 32^3 + 1 cell starts per scene in the workspace
constexpr int AFF_GRID_MIN = 3;                   // fewer cells per axis than this: every walk visits everything, take the dense form
constexpr long long AFF_GRID_MAX_VOXELS = 1 << 20;   // the sort is one workgroup per scene; larger lattices take the dense form

// matplotlib's 'Reds': the nine ColorBrewer anchors ff f5 f0, fe e0 d2, fc bb a1, fc 92 72, fb 6a 4a, ef 3b 2c, cb 18 1d, a5 0f 15,
// 67 00 0d (each / 255) interpolated linearly at i / 255, i = 0 .. 255, then rint(255 c).  giga_affordance_colormap hands the
// table out; tests/test_affordance_host.py rebuilds it from the anchors.
static const uint8_t AFF_REDS[256][3] = {
    {255,245,240}, {255,244,239}, {255,244,238}, {255,243,237}, {255,242,236}, {255,242,235}, {255,241,234}, {255,240,233},
    {255,240,232}, {255,239,232}, {255,238,231}, {255,238,230}, {255,237,229}, {255,236,228}, {255,236,227}, {255,235,226},
    {254,234,225}, {254,234,224}, {254,233,223}, {254,232,222}, {254,232,221}, {254,231,220}, {254,231,219}, {254,230,218},
    {254,229,217}, {254,229,216}, {254,228,216}, {254,227,215}, {254,227,214}, {254,226,213}, {254,225,212}, {254,225,211},
    {254,224,210}, {254,223,208}, {254,222,207}, {254,220,205}, {254,219,204}, {254,218,202}, {254,217,201}, {254,216,199},
    {253,215,198}, {253,213,196}, {253,212,194}, {253,211,193}, {253,210,191}, {253,209,190}, {253,208,188}, {253,206,187},
    {253,205,185}, {253,204,184}, {253,203,182}, {253,202,181}, {253,201,179}, {253,199,178}, {253,198,176}, {253,197,174},
    {252,196,173}, {252,195,171}, {252,194,170}, {252,193,168}, {252,191,167}, {252,190,165}, {252,189,164}, {252,188,162},
    {252,187,161}, {252,185,159}, {252,184,158}, {252,183,156}, {252,182,155}, {252,180,153}, {252,179,152}, {252,178,150},
    {252,176,149}, {252,175,147}, {252,174,146}, {252,173,144}, {252,171,143}, {252,170,141}, {252,169,140}, {252,167,139},
    {252,166,137}, {252,165,136}, {252,164,134}, {252,162,133}, {252,161,131}, {252,160,130}, {252,158,128}, {252,157,127},
    {252,156,125}, {252,155,124}, {252,153,122}, {252,152,121}, {252,151,119}, {252,149,118}, {252,148,116}, {252,147,115},
    {252,146,114}, {252,144,112}, {252,143,111}, {252,142,110}, {252,141,109}, {252,139,107}, {252,138,106}, {252,137,105},
    {252,135,103}, {252,134,102}, {252,133,101}, {252,132,100}, {252,130,98}, {252,129,97}, {252,128,96}, {252,127,95},
    {251,125,93}, {251,124,92}, {251,123,91}, {251,122,90}, {251,120,88}, {251,119,87}, {251,118,86}, {251,117,85},
    {251,115,83}, {251,114,82}, {251,113,81}, {251,112,80}, {251,110,78}, {251,109,77}, {251,108,76}, {251,107,75},
    {251,105,74}, {250,104,73}, {250,102,72}, {250,101,71}, {249,99,70}, {249,98,69}, {249,96,68}, {248,95,67},
    {248,93,66}, {247,92,65}, {247,91,64}, {247,89,63}, {246,88,62}, {246,86,61}, {246,85,60}, {245,83,59},
    {245,82,58}, {244,80,58}, {244,79,57}, {244,77,56}, {243,76,55}, {243,74,54}, {243,73,53}, {242,71,52},
    {242,70,51}, {241,68,50}, {241,67,49}, {241,65,48}, {240,64,47}, {240,63,46}, {240,61,45}, {239,60,44},
    {238,58,44}, {237,57,43}, {236,56,43}, {235,55,42}, {234,54,42}, {233,53,41}, {232,52,41}, {230,51,40},
    {229,50,40}, {228,48,39}, {227,47,39}, {226,46,39}, {225,45,38}, {224,44,38}, {222,43,37}, {221,42,37},
    {220,41,36}, {219,40,36}, {218,39,35}, {217,37,35}, {216,36,34}, {215,35,34}, {213,34,33}, {212,33,33},
    {211,32,32}, {210,31,32}, {209,30,31}, {208,29,31}, {207,28,31}, {206,26,30}, {204,25,30}, {203,24,29},
    {202,24,29}, {201,24,29}, {200,23,28}, {199,23,28}, {197,23,28}, {196,22,28}, {195,22,27}, {194,22,27},
    {193,22,27}, {191,21,27}, {190,21,26}, {189,21,26}, {188,20,26}, {187,20,26}, {185,20,25}, {184,20,25},
    {183,19,25}, {182,19,25}, {181,19,24}, {179,18,24}, {178,18,24}, {177,18,24}, {176,18,23}, {175,17,23},
    {173,17,23}, {172,17,23}, {171,16,22}, {170,16,22}, {169,16,22}, {168,16,22}, {166,15,21}, {165,15,21},
    {163,15,21}, {161,14,21}, {159,14,20}, {157,13,20}, {156,13,20}, {154,12,20}, {152,12,19}, {150,11,19},
    {148,11,19}, {146,10,19}, {144,10,18}, {142,9,18}, {140,9,18}, {138,8,18}, {136,8,17}, {134,8,17},
    {132,7,17}, {130,7,17}, {128,6,16}, {126,6,16}, {124,5,16}, {122,5,16}, {121,4,15}, {119,4,15},
    {117,3,15}, {115,3,15}, {113,2,14}, {111,2,14}, {109,1,14}, {107,1,14}, {105,0,13}, {103,0,13}};

static void affordance_colormap(uint8_t* rgba) {
    for (int i = 0; i < 256; ++i) {
        for (int c = 0; c < 3; ++c) rgba[4 * i + c] = AFF_REDS[i][c];
        rgba[4 * i + 3] = 255;
    }
}

// ------------------------------------------------------------------------------------------------------------------ points
struct AffPointArgs {
    const float* qual;
    const float* rot;
    double* points;
    unsigned* block_base;                         // [B][nblk]: counts after the first kernel, exclusive prefixes after the scan
    double step, size;
    float th, depth, offset;
    int R, nblk, move_center;
    unsigned V;
};

__global__ __launch_bounds__(AFF_BLOCK) void affordance_count_kernel(AffPointArgs g) {
    __shared__ unsigned wsum[AFF_WAVES];
    const unsigned v = blockIdx.x * AFF_BLOCK + threadIdx.x;
    const bool keep = v < g.V && g.qual[(size_t)blockIdx.y * g.V + v] > g.th;
    unsigned total;
    block_excl<AFF_WAVES>(keep ? 1u : 0u, wsum, total);
    if (threadIdx.x == 0) g.block_base[(size_t)blockIdx.y * g.nblk + blockIdx.x] = total;
}

__global__ __launch_bounds__(AFF_BLOCK) void affordance_emit_kernel(AffPointArgs g) {
    __shared__ unsigned wsum[AFF_WAVES];
    const unsigned v = blockIdx.x * AFF_BLOCK + threadIdx.x;
    const size_t at = (size_t)blockIdx.y * g.V + v;
    const float q = v < g.V ? g.qual[at] : 0.0f;
    const bool keep = v < g.V && q > g.th;
    unsigned total;
    const unsigned pre = block_excl<AFF_WAVES>(keep ? 1u : 0u, wsum, total);
    if (!keep) return;
    const int R = g.R;
    const int idx[3] = {(int)(v / (unsigned)(R * R)), (int)((v / (unsigned)R) % (unsigned)R), (int)(v % (unsigned)R)};
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = idx[a] == R - 1 ? g.size : (double)idx[a] * g.step;      // np.linspace(0, size, R)
    if (g.move_center) {
        const float* __restrict__ r = g.rot + 4 * at;
        const float r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
        const float z[3] = {(2.0f * r0) * r2 + (2.0f * r1) * r3, (2.0f * r1) * r2 - (2.0f * r0) * r3,
                            (1.0f - (2.0f * r0) * r0) - (2.0f * r1) * r1};
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = p[a] + (double)((z[a] * g.depth) * g.offset);
    }
    const unsigned row = g.block_base[(size_t)blockIdx.y * g.nblk + blockIdx.x] + pre;          // < the scene's count <= V
    double* __restrict__ o = g.points + 4 * ((size_t)blockIdx.y * g.V + row);
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = (double)q;
}

// ------------------------------------------------------------------------------------------------------------------- grid
struct AffGrid {
    double lo, h;                                 // cell of a coordinate x: clamp(floor((x - lo) / h), 0, n - 1)
    int n, bits;                                  // cells per axis; bits of a cell number
};

__device__ __forceinline__ int aff_cell1(double x, const AffGrid& gr) {
    const double c = floor((x - gr.lo) / gr.h);   // every step is monotone in x; NaN ends in cell 0 (fmax drops it)
    return (int)fmin(fmax(c, 0.0), (double)(gr.n - 1));
}

struct AffSortArgs {
    const double* points;
    const int* counts;
    unsigned* keys[2];                            // [B][V] each: cell numbers, ping and pong
    unsigned* order[2];                           // [B][V] each: point numbers in cell order
    unsigned* start;                              // [B][n^3 + 1]
    AffGrid grid;
    unsigned V;
};

// One workgroup per scene.  Stable least-significant-bit-first radix sort of (cell, point number), one bit per pass: thread t owns
// the contiguous slice [t per, (t + 1) per) of the array, counts its zeros, and a scan over the threads places them.
__global__ __launch_bounds__(AFF_SORT_BLOCK) void affordance_sort_kernel(AffSortArgs g) {
    __shared__ unsigned wsum[AFF_SORT_WAVES];
    const unsigned t = threadIdx.x;
    const size_t sb = (size_t)blockIdx.x * g.V;
    const unsigned P = (unsigned)g.counts[blockIdx.x];
    const unsigned per = (P + AFF_SORT_BLOCK - 1) / AFF_SORT_BLOCK;
    const unsigned s0 = min(t * per, P), s1 = min(s0 + per, P);
    const int n = g.grid.n;
    const unsigned ncell = (unsigned)(n * n * n);
    unsigned* __restrict__ start = g.start + (size_t)blockIdx.x * (ncell + 1);
    {
        const double* __restrict__ pts = g.points + 4 * sb;
        unsigned* __restrict__ k = g.keys[0] + sb;
        unsigned* __restrict__ o = g.order[0] + sb;
        for (unsigned s = s0; s < s1; ++s) {
            const int cx = aff_cell1(pts[4 * (size_t)s], g.grid), cy = aff_cell1(pts[4 * (size_t)s + 1], g.grid),
                      cz = aff_cell1(pts[4 * (size_t)s + 2], g.grid);
            k[s] = (unsigned)((cx * n + cy) * n + cz);
            o[s] = s;
        }
    }
    __syncthreads();
    for (int bit = 0; bit < g.grid.bits; ++bit) {
        const unsigned* __restrict__ ki = g.keys[bit & 1] + sb;
        const unsigned* __restrict__ oi = g.order[bit & 1] + sb;
        unsigned* __restrict__ ko = g.keys[(bit & 1) ^ 1] + sb;
        unsigned* __restrict__ oo = g.order[(bit & 1) ^ 1] + sb;
        unsigned zeros = 0;
        for (unsigned s = s0; s < s1; ++s) zeros += ((ki[s] >> bit) & 1u) ^ 1u;
        unsigned total;
        unsigned z = block_excl<AFF_SORT_WAVES>(zeros, wsum, total);      // zeros before this slice; total = all zeros
        for (unsigned s = s0; s < s1; ++s) {
            const unsigned key = ki[s];
            const bool one = (key >> bit) & 1u;
            const unsigned to = one ? total + (s - z) : z;                 // s - z = ones before s; to < P
            if (!one) ++z;
            ko[to] = key;
            oo[to] = oi[s];
        }
        __syncthreads();                          // the pass is in memory (one workgroup: one CU) and wsum is free again
    }
    const unsigned* __restrict__ k = g.keys[g.grid.bits & 1] + sb;
    if (P == 0) {
        for (unsigned c = t; c <= ncell; c += AFF_SORT_BLOCK) start[c] = 0;
        return;
    }
    // start[c] = number of points in cells < c: slot s writes the cells in (key[s - 1], key[s]], the last slot the rest
    for (unsigned s = s0; s < s1; ++s) {
        const unsigned key = k[s];                // < ncell
        for (unsigned c = s == 0 ? 0u : k[s - 1] + 1; c <= key; ++c) start[c] = s;
        if (s == P - 1)
            for (unsigned c = key + 1; c <= ncell; ++c) start[c] = P;
    }
}

// ------------------------------------------------------------------------------------------------------------------ faces
struct AffFaceArgs {
    const float* vertices;
    const int* triangles;
    const int* voffs;                             // workspace copies (device)
    const int* toffs;
    const int* boffs;                             // first workgroup of each scene
    const uchar4* reds;                           // the colour table, [256]
    const double* points;
    const int* counts;
    const unsigned* order;                        // grid form only
    const unsigned* start;
    double* affordance;
    uint8_t* rgba;
    AffGrid grid;
    double th, temp, limit2;                      // limit2: the T of the head of the file
    int B;
    unsigned V;
};

struct AffPoint { double x, y, z, q, w; };

__device__ __forceinline__ double aff_dist2(double cx, double cy, double cz, double px, double py, double pz) {
    const double dx = cx - px, dy = cy - py, dz = cz - pz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// MODE: GIGA_AFFORDANCE_MAX / _SOFTMAX / _MEAN; GRID: walk the cell grid (MODE max only)
template <int MODE, bool GRID>
__global__ __launch_bounds__(AFF_BLOCK) void affordance_faces_kernel(AffFaceArgs g) {
    __shared__ AffPoint tile[GRID ? 1 : AFF_BLOCK];
    // the scene of this workgroup: the last b with boffs[b] <= blockIdx.x (B + 1 entries, boffs[B] = gridDim.x)
    int lo = 0, hi = g.B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g.boffs[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    const int scene = lo;
    const int vbase = g.voffs[scene], nv = g.voffs[scene + 1] - vbase;
    const long long face = g.toffs[scene] + (long long)((int)blockIdx.x - g.boffs[scene]) * AFF_BLOCK + (int)threadIdx.x;
    const bool live = face < (long long)g.toffs[scene + 1];
    const int P = g.counts[scene];
    const double* __restrict__ pts = g.points + 4 * (size_t)scene * g.V;

    const double nan = __builtin_nan("");
    double cx = nan, cy = nan, cz = nan;
    bool valid = false;                           // a face with a vertex index outside its scene: NaN affordance, colour (0,0,0,0)
    if (live) {
        const int* __restrict__ f = g.triangles + 3 * (size_t)face;
        const int ia = f[0], ib = f[1], ic = f[2];
        if ((unsigned)ia < (unsigned)nv && (unsigned)ib < (unsigned)nv && (unsigned)ic < (unsigned)nv) {
            const float* __restrict__ a = g.vertices + 3 * ((size_t)vbase + ia);
            const float* __restrict__ b = g.vertices + 3 * ((size_t)vbase + ib);
            const float* __restrict__ c = g.vertices + 3 * ((size_t)vbase + ic);
            valid = true;
            cx = (((double)a[0] + (double)b[0]) + (double)c[0]) / 3.0;
            cy = (((double)a[1] + (double)b[1]) + (double)c[1]) / 3.0;
            cz = (((double)a[2] + (double)b[2]) + (double)c[2]) / 3.0;
        }
    }

    double aff = nan;
    if (GRID) {
        // max_p (in ? q : 0): the maximum over the points in range, and 0 as soon as one point is out of range
        double best = -__builtin_huge_val();
        int n_in = 0;
        if (live && cx == cx && cy == cy && cz == cz) {
            const int n = g.grid.n;
            const unsigned* __restrict__ start = g.start + (size_t)scene * ((size_t)n * n * n + 1);
            const unsigned* __restrict__ order = g.order + (size_t)scene * g.V;
            const int kx = aff_cell1(cx, g.grid), ky = aff_cell1(cy, g.grid), kz = aff_cell1(cz, g.grid);
            const int z0 = max(kz - 1, 0), z1 = min(kz + 1, n - 1);
            for (int x = max(kx - 1, 0); x <= min(kx + 1, n - 1); ++x)
                for (int y = max(ky - 1, 0); y <= min(ky + 1, n - 1); ++y) {
                    const unsigned col = (unsigned)((x * n + y) * n);
                    const unsigned e = start[col + z1 + 1];
                    for (unsigned s = start[col + z0]; s < e; ++s) {
                        const double* __restrict__ p = pts + 4 * (size_t)order[s];     // order[s] < P
                        if (aff_dist2(cx, cy, cz, p[0], p[1], p[2]) <= g.limit2) {
                            best = fmax(best, p[3]);
                            ++n_in;
                        }
                    }
                }
        }
        if (P > 0) aff = n_in < P ? fmax(best, 0.0) : best;              // (a NaN centre: no comparison holds, 0 as in the dense form)
    } else {
        double best = -__builtin_huge_val(), sw = 0.0, swq = 0.0;
        for (int base = 0; base < P; base += AFF_BLOCK) {
            __syncthreads();
            const int s = base + (int)threadIdx.x;
            if (s < P) {
                const double* __restrict__ p = pts + 4 * (size_t)s;
                AffPoint r;
                r.x = p[0]; r.y = p[1]; r.z = p[2]; r.q = p[3];
                r.w = MODE == GIGA_AFFORDANCE_SOFTMAX ? exp(r.q * g.temp) : 0.0;
                tile[threadIdx.x] = r;
            }
            __syncthreads();
            const int m = min(AFF_BLOCK, P - base);
            for (int i = 0; i < m; ++i) {
                const AffPoint& r = tile[GRID ? 0 : i];                    // every lane reads the same record: broadcast
                const double d2 = aff_dist2(cx, cy, cz, r.x, r.y, r.z);
                if (MODE == GIGA_AFFORDANCE_MAX) {
                    best = fmax(best, d2 <= g.limit2 ? r.q : 0.0);
                } else if (MODE == GIGA_AFFORDANCE_SOFTMAX) {
                    const double w = d2 <= g.limit2 ? r.w : 0.0;
                    sw = sw + w;
                    swq = swq + w * r.q;
                } else {
                    const double w = exp(-__dsqrt_rn(d2) * g.temp);
                    sw = sw + w;
                    swq = swq + w * r.q;
                }
            }
        }
        if (P > 0) aff = MODE == GIGA_AFFORDANCE_MAX ? best : MODE == GIGA_AFFORDANCE_SOFTMAX ? swq / (sw + 1e-5) : swq / sw;
    }
    if (!live) return;
    if (!valid) aff = nan;
    uint8_t c[4] = {102, 102, 102, 255};          // no points: trimesh's default face colour
    if (P > 0) {
        double a = aff < g.th ? g.th : aff;       // np.clip(a, th, 1): NaN stays NaN
        a = a > 1.0 ? 1.0 : a;
        aff = (a - g.th) / (1.0 - g.th);
        const double x = ((aff * aff) * (aff * aff)) * 256.0;
        if (x == x) {
            const int i = x < 0.0 ? 0 : x >= 255.0 ? 255 : (int)x;        // matplotlib: int(x N), N itself and beyond -> N - 1, under -> first
            const uchar4 r = g.reds[i];
            c[0] = r.x; c[1] = r.y; c[2] = r.z; c[3] = r.w;
        } else {
            c[0] = c[1] = c[2] = c[3] = 0;        // the map's 'bad' colour
        }
    }
    g.affordance[(size_t)face] = aff;
    *reinterpret_cast<uchar4*>(g.rgba + 4 * (size_t)face) = make_uchar4(c[0], c[1], c[2], c[3]);
}

// ------------------------------------------------------------------------------------------------------------------- host
struct AffWs { size_t reds, voffs, toffs, boffs, block_base, keys[2], order[2], start, total; };
static AffWs aff_workspace(int B, int R) {
    const size_t V = (size_t)R * R * R, nblk = (V + AFF_BLOCK - 1) / AFF_BLOCK;
    const size_t sortV = (long long)V <= AFF_GRID_MAX_VOXELS ? V : 0;
    WsLayout L;
    AffWs w;
    w.reds = L.take<uchar4>(256);
    w.voffs = L.take<int>((size_t)B + 1);
    w.toffs = L.take<int>((size_t)B + 1);
    w.boffs = L.take<int>((size_t)B + 1);
    w.block_base = L.take<unsigned>((size_t)B * nblk);
    for (int i = 0; i < 2; ++i) w.keys[i] = L.take<unsigned>((size_t)B * sortV);
    for (int i = 0; i < 2; ++i) w.order[i] = L.take<unsigned>((size_t)B * sortV);
    w.start = L.take<unsigned>(sortV ? (size_t)B * ((size_t)AFF_GRID_MAX * AFF_GRID_MAX * AFF_GRID_MAX + 1) : 0);
    w.total = L.total;
    return w;
}

static int launch_affordance_points(const float* qual, const float* rot, int B, int R, const GigaAffordanceParams* prm, double* points,
                                    int* counts, uint8_t* ws, hipStream_t s) {
    const AffWs w = aff_workspace(B, R);
    AffPointArgs g;
    g.qual = qual; g.rot = rot; g.points = points;
    g.block_base = reinterpret_cast<unsigned*>(ws + w.block_base);
    g.step = prm->size / (double)(R - 1);
    g.size = prm->size;
    g.th = (float)prm->th; g.depth = (float)prm->finger_depth; g.offset = (float)prm->finger_offset;
    g.R = R; g.move_center = prm->move_center;
    g.V = (unsigned)((size_t)R * R * R);
    g.nblk = (int)((g.V + AFF_BLOCK - 1) / AFF_BLOCK);
    GIGA_LAUNCH(affordance_count_kernel, dim3((unsigned)g.nblk, (unsigned)B), dim3(AFF_BLOCK), 0, s, g);
    GIGA_LAUNCH(scene_offsets_kernel<unsigned>, dim3((unsigned)B), dim3(SCAN_BLOCK), 0, s, g.block_base, (unsigned)g.nblk, counts,
                static_cast<int*>(nullptr));
    GIGA_LAUNCH(affordance_emit_kernel, dim3((unsigned)g.nblk, (unsigned)B), dim3(AFF_BLOCK), 0, s, g);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

// the largest double whose correctly rounded square root is <= rad (-1: none, rad < 0)
static double aff_limit2(double rad) {
    if (rad < 0.0) return -1.0;
    double t = rad * rad;
    while (std::sqrt(t) > rad) t = std::nextafter(t, 0.0);
    for (double u = std::nextafter(t, HUGE_VAL); u != t && std::sqrt(u) <= rad; u = std::nextafter(t, HUGE_VAL)) t = u;
    return t;
}

// the cell grid of a call, n = 0 for the dense form
static AffGrid aff_grid(int R, const GigaAffordanceParams* prm) {
    AffGrid gr = {0.0, 1.0, 0, 0};
    const int mode = prm->aggregation & 0xff;
    if (mode != GIGA_AFFORDANCE_MAX || (prm->aggregation & GIGA_AFFORDANCE_DENSE)) return gr;
    if ((long long)R * R * R > AFF_GRID_MAX_VOXELS || !(prm->rad > 0.0) || !(prm->size > 0.0)) return gr;
    // the lattice spans [0, size]; move_center shifts a point by at most |finger_depth finger_offset| per axis when the quaternion
    // has unit length.  Points further out (other quaternions) fall into the outermost cells: the clamp is monotone too.
    const double margin = prm->move_center ? std::fabs(prm->finger_depth * prm->finger_offset) : 0.0;
    const double extent = prm->size + 2.0 * margin;
    double h = prm->rad * (1.0 + 0x1p-20);
    if (!(extent / h < (double)AFF_GRID_MAX)) h = std::fmax(h, extent / (double)AFF_GRID_MAX);
    const double cells = std::floor(extent / h) + 1.0;
    if (!(cells >= (double)AFF_GRID_MIN) || !(h > 0.0) || h - h != 0.0) return gr;
    gr.lo = -margin;
    gr.h = h;
    gr.n = cells > (double)AFF_GRID_MAX ? AFF_GRID_MAX : (int)cells;
    while ((1 << gr.bits) < gr.n * gr.n * gr.n) ++gr.bits;
    return gr;
}

static int launch_affordance_faces(const float* vertices, const int* vertex_offsets, const int* triangles, const int* triangle_offsets,
                                   const double* points, const int* counts, int B, int R, const GigaAffordanceParams* prm,
                                   double* affordance, uint8_t* rgba, uint8_t* ws, hipStream_t s) {
    const AffWs w = aff_workspace(B, R);
    // one staging buffer, one copy (pageable host memory: the copy has left it when the call returns)
    std::vector<int> host(w.block_base / sizeof(int), 0);
    int* boffs = &host[w.boffs / sizeof(int)];
    affordance_colormap(reinterpret_cast<uint8_t*>(&host[w.reds / sizeof(int)]));
    std::memcpy(&host[w.voffs / sizeof(int)], vertex_offsets, (size_t)(B + 1) * sizeof(int));
    std::memcpy(&host[w.toffs / sizeof(int)], triangle_offsets, (size_t)(B + 1) * sizeof(int));
    long long blocks = 0;
    for (int b = 0; b < B; ++b) {
        boffs[b] = (int)blocks;
        blocks += (triangle_offsets[b + 1] - triangle_offsets[b] + AFF_BLOCK - 1) / AFF_BLOCK;
    }
    boffs[B] = (int)blocks;
    if (blocks == 0) return 0;
    if (hipMemcpyAsync(ws, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;

    const AffGrid gr = aff_grid(R, prm);
    AffFaceArgs g;
    g.vertices = vertices; g.triangles = triangles;
    g.voffs = reinterpret_cast<const int*>(ws + w.voffs);
    g.toffs = reinterpret_cast<const int*>(ws + w.toffs);
    g.boffs = reinterpret_cast<const int*>(ws + w.boffs);
    g.reds = reinterpret_cast<const uchar4*>(ws + w.reds);
    g.points = points; g.counts = counts;
    g.order = reinterpret_cast<const unsigned*>(ws + w.order[gr.bits & 1]);
    g.start = reinterpret_cast<const unsigned*>(ws + w.start);
    g.affordance = affordance; g.rgba = rgba;
    g.grid = gr;
    g.th = prm->th; g.temp = prm->temp; g.limit2 = aff_limit2(prm->rad);
    g.B = B;
    g.V = (unsigned)((size_t)R * R * R);
    const dim3 grid((unsigned)blocks), block(AFF_BLOCK);
    const int mode = prm->aggregation & 0xff;
    if (gr.n) {
        AffSortArgs a;
        a.points = points; a.counts = counts;
        for (int i = 0; i < 2; ++i) {
            a.keys[i] = reinterpret_cast<unsigned*>(ws + w.keys[i]);
            a.order[i] = reinterpret_cast<unsigned*>(ws + w.order[i]);
        }
        a.start = reinterpret_cast<unsigned*>(ws + w.start);
        a.grid = gr;
        a.V = g.V;
        GIGA_LAUNCH(affordance_sort_kernel, dim3((unsigned)B), dim3(AFF_SORT_BLOCK), 0, s, a);
        GIGA_LAUNCH((affordance_faces_kernel<GIGA_AFFORDANCE_MAX, true>), grid, block, 0, s, g);
    } else if (mode == GIGA_AFFORDANCE_MAX) {
        GIGA_LAUNCH((affordance_faces_kernel<GIGA_AFFORDANCE_MAX, false>), grid, block, 0, s, g);
    } else if (mode == GIGA_AFFORDANCE_SOFTMAX) {
        GIGA_LAUNCH((affordance_faces_kernel<GIGA_AFFORDANCE_SOFTMAX, false>), grid, block, 0, s, g);
    } else {
        GIGA_LAUNCH((affordance_faces_kernel<GIGA_AFFORDANCE_MEAN, false>), grid, block, 0, s, g);
    }
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // namespace giga

using namespace giga;

extern "C" {

static int affordance_check(int B, int R, const GigaAffordanceParams* p) {
    if (const int rc = ragged_batch_check(B)) return rc;
    if (!p || R < 2 || R > GIGA_TSDF_MAX_R) return -1;
    const int mode = p->aggregation & ~GIGA_AFFORDANCE_DENSE;
    if (mode != GIGA_AFFORDANCE_MAX && mode != GIGA_AFFORDANCE_SOFTMAX && mode != GIGA_AFFORDANCE_MEAN) return -1;
    if (!finite_f64(p->size) || !finite_f64(p->th) || !finite_f64(p->temp) || !finite_f64(p->rad) || !finite_f64(p->finger_depth) ||
        !finite_f64(p->finger_offset))
        return -1;
    return 0;
}

size_t giga_affordance_workspace_bytes(int B, int R, int n_faces_total) {
    if (B <= 0 || B > GIGA_MAX_SCENES || R < 2 || R > GIGA_TSDF_MAX_R || n_faces_total < 0) return 0;
    return aff_workspace(B, R).total;
}

int giga_affordance_points(const float* qual, const float* rot, int B, int R, const GigaAffordanceParams* params, double* points,
                           int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = affordance_check(B, R, params)) return rc;
    if (B == 0) return 0;
    if (!qual || (params->move_center && !rot) || !points || !counts || !workspace) return -1;
    if (workspace_bytes < giga_affordance_workspace_bytes(B, R, 0)) return -4;
    return launch_affordance_points(qual, rot, B, R, params, points, counts, static_cast<uint8_t*>(workspace),
                                    static_cast<hipStream_t>(stream));
}

int giga_affordance_faces(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                          const double* points, const int32_t* counts, int B, int R, const GigaAffordanceParams* params,
                          double* affordance, uint8_t* rgba, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = affordance_check(B, R, params)) return rc;
    if (B == 0) return 0;
    if (!ragged_ok(vertex_offsets, B) || !ragged_ok(triangle_offsets, B)) return -1;
    if (triangle_offsets[B] == 0) return 0;                 // (whatever the data pointers: only the offsets are looked at before)
    if (!mesh_batch_check(vertex_offsets, triangle_offsets, B, vertices, triangles) || !points || !counts || !affordance || !rgba ||
        !workspace)
        return -1;
    if (workspace_bytes < giga_affordance_workspace_bytes(B, R, triangle_offsets[B])) return -4;
    return launch_affordance_faces(vertices, vertex_offsets, triangles, triangle_offsets, points, counts, B, R, params, affordance, rgba,
                                   static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

void giga_affordance_colormap(uint8_t* rgba) {
    if (rgba) affordance_colormap(rgba);
}

}  // extern "C"
