// Marching cubes on B dense value grids [B][nx][ny][nz] (occupancy logits): the device counterpart of
// `libmcubes.marching_cubes(np.pad(occ_hat, 1, constant_values=-1e6), threshold)` plus the coordinate mapping of
// `Generator3D.extract_mesh` (reference conv_onet/generation.py:360-393, the `vol_bound is None` branch).
//
// Cells.  The padded grid has (n+2) samples and (n+1) cells per axis; the padding is virtual (a sample outside the grid
// reads -1e6).  Cell (i, j, k), 0 <= i <= nx, has its corner 6 -- the corner with the largest coordinates -- at grid
// sample (i, j, k) and its corner 0 at (i-1, j-1, k-1).  A cell OWNS the three edges that meet in corner 6 (edge 6 along
// x, edge 5 along y, edge 10 along z, in that order); every crossed edge of the padded grid is owned by exactly one cell
// (an edge inside a boundary plane joins two padding samples and is never crossed).  Cells are numbered with k fastest,
// like the grid, so that a wave reads consecutive samples.
//
// Passes (B scenes in each launch, gridDim.y = scene):
//   classify  one thread per cell: case index from 8 samples, the 3 owned-edge flags, the triangle count from the table.
//             Exclusive scan of both counts inside the workgroup: ballot + popcount inside a wave (the vertex count is
//             three 1-bit flags, the triangle count three binary digits), LDS across the four waves (giga_scan.h).  Per cell one word
//             (vertex prefix inside the workgroup << 3 | flags), per workgroup the two sums.
//   scan      giga_scan.h: one workgroup per scene walks the workgroup sums in order (exclusive, in place) and writes the
//             scene's totals to `counts`; one wave then turns the B totals into 64-bit bases.
//   emit      same cell mapping: owned crossed edges write their vertex at (scene base + workgroup offset + prefix); each
//             triangle looks its three vertices up through the owning cells' words.
// Every output position is a sum of counts in cell order: no atomics, two runs give the same bytes.
// Integer work on a few bytes per cell: no MFMA, 4.3 KB of LDS for the case tables (read with a divergent index).
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "giga_check.h"
#include "giga_scan.h"
#include "giga_ws.h"
#define GIGA_MC_QUAL __device__ __attribute__((aligned(16)))
#include "giga_mc_tables.h"
#include <cmath>
#include <cstdint>

namespace giga {

constexpr int MESH_BLOCK = 256;
constexpr int MESH_WAVES = MESH_BLOCK / 64;
constexpr float MESH_PAD = -1e6f;
static_assert(GIGA_MC_MAX_TRIS <= 7, "the triangle count is scanned as three binary digits");
static_assert(sizeof(GIGA_MC_TRIS) == 4096, "one uint4 per thread fills the LDS copy");

struct MeshDims {
    int nx, ny, nz;          // samples per axis
    unsigned cy, cz;         // cells per axis (n + 1) of the two fast axes
    unsigned cells;          // (nx+1)(ny+1)(nz+1)
    unsigned nblk;           // workgroups per scene
};

// Owner of cube edge e: the cell whose corner 6 is the edge's larger endpoint.  bits 0-1: axis of the edge (0 x, 1 y, 2 z);
// bits 2, 3, 4: the owner is one cell back along x, y, z.
__device__ __forceinline__ unsigned edge_owner(int e) {
    // e:          0          1        2        3          4        5   6   7        8           9        10  11
    // packed 5 bits per edge, low bits first
    constexpr unsigned long long T =
        ((0ull | 8 | 16) << 0) | ((1ull | 16) << 5) | ((0ull | 16) << 10) | ((1ull | 4 | 16) << 15) | ((0ull | 8) << 20) |
        (1ull << 25) | (0ull << 30) | ((1ull | 4) << 35) | ((2ull | 4 | 8) << 40) | ((2ull | 8) << 45) | (2ull << 50) |
        ((2ull | 4) << 55);
    return (unsigned)(T >> (5 * e)) & 31u;
}

struct CellRead {
    float v[8];
    unsigned cube;           // case index
    unsigned flags;          // bit 0 / 1 / 2: owned x / y / z edge is crossed
};

__device__ __forceinline__ CellRead read_cell(const float* __restrict__ g, const MeshDims& d, unsigned cell, float isof) {
    const int k = (int)(cell % d.cz);
    const unsigned r = cell / d.cz;
    const int j = (int)(r % d.cy), i = (int)(r / d.cy);
    CellRead c;
    // corner m = (dx, dy, dz) in the customary order 000 100 110 010 001 101 111 011
    constexpr int DX[8] = {0, 1, 1, 0, 0, 1, 1, 0}, DY[8] = {0, 0, 1, 1, 0, 0, 1, 1}, DZ[8] = {0, 0, 0, 0, 1, 1, 1, 1};
    c.cube = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int x = i - 1 + DX[m], y = j - 1 + DY[m], z = k - 1 + DZ[m];
        const bool in = (unsigned)x < (unsigned)d.nx && (unsigned)y < (unsigned)d.ny && (unsigned)z < (unsigned)d.nz;
        c.v[m] = in ? g[((size_t)x * d.ny + y) * d.nz + z] : MESH_PAD;
        c.cube |= (c.v[m] <= isof ? 1u : 0u) << m;
    }
    const unsigned b6 = c.cube >> 6 & 1;
    c.flags = (b6 ^ (c.cube >> 7 & 1)) | (b6 ^ (c.cube >> 5 & 1)) << 1 | (b6 ^ (c.cube >> 2 & 1)) << 2;
    return c;
}

// exclusive prefix over the workgroup's cells, in cell order, of both counts of a cell: x = the number of set flags, y = ntri
__device__ __forceinline__ uint2 cell_prefix(unsigned flags, unsigned nt, uint2* wsum, uint2& total) {
    const unsigned lane = threadIdx.x & 63;
    unsigned sv, st;
    const unsigned pv = wave_excl_bits3<1, 1>(flags, lane, sv), pt = wave_excl_bits3<2, 4>(nt, lane, st);
    return block_combine<MESH_WAVES>(make_uint2(pv, pt), make_uint2(sv, st), lane == 0, wsum, total);
}

__global__ __launch_bounds__(MESH_BLOCK) void mesh_classify_kernel(const float* __restrict__ grids, MeshDims d, float isof,
                                                                   unsigned* __restrict__ words, uint2* __restrict__ blk) {
    __shared__ unsigned char s_ntri[256];
    __shared__ uint2 wsum[MESH_WAVES];
    s_ntri[threadIdx.x] = GIGA_MC_NTRI[threadIdx.x];
    __syncthreads();
    const unsigned cell = blockIdx.x * MESH_BLOCK + threadIdx.x, scene = blockIdx.y;
    unsigned flags = 0, nt = 0;
    if (cell < d.cells) {
        const CellRead c = read_cell(grids + (size_t)scene * d.nx * d.ny * d.nz, d, cell, isof);
        flags = c.flags;
        nt = s_ntri[c.cube];
    }
    uint2 total;
    const uint2 pre = cell_prefix(flags, nt, wsum, total);
    if (cell < d.cells) words[(size_t)scene * d.cells + cell] = pre.x << 3 | flags;
    if (threadIdx.x == 0) blk[(size_t)scene * d.nblk + blockIdx.x] = total;
}

// position along an edge in the padded grid, as the reference computes it: (x2 - x1) (iso - f1) / (f2 - f1) + x1, the midpoint
// for f1 == f2 (kept for parity with marchingcubes.cpp:290-297 only: an edge with equal ends is never crossed, so no vertex of
// this kernel takes that branch); then extract_mesh's mapping, one rounding per step like numpy's
__device__ __forceinline__ double edge_point(double iso, double f1, double f2, double x1, double x2) {
    if (f2 == f1) return (x2 + x1) / 2;
    return (x2 - x1) * (iso - f1) / (f2 - f1) + x1;
}
__device__ __forceinline__ float to_model(double padded, int n, double box) {
    double v = padded - 0.5;
    v -= 1.0;
    v /= (double)(n - 1);
    return (float)(box * (v - 0.5));
}

__global__ __launch_bounds__(MESH_BLOCK) void mesh_emit_kernel(const float* __restrict__ grids, MeshDims d, float isof, double iso,
                                                               double box, const unsigned* __restrict__ words,
                                                               const uint2* __restrict__ blk,
                                                               const unsigned long long* __restrict__ bases, int B,
                                                               float* __restrict__ vertices, unsigned long long cap_v,
                                                               int* __restrict__ triangles, unsigned long long cap_t,
                                                               int* __restrict__ shortfall) {
    __shared__ __attribute__((aligned(16))) unsigned char s_tris[256][16];
    __shared__ unsigned char s_ntri[256];
    __shared__ uint2 wsum[MESH_WAVES];
    reinterpret_cast<uint4*>(&s_tris[0][0])[threadIdx.x] = reinterpret_cast<const uint4*>(&GIGA_MC_TRIS[0][0])[threadIdx.x];
    s_ntri[threadIdx.x] = GIGA_MC_NTRI[threadIdx.x];
    __syncthreads();
    const unsigned cell = blockIdx.x * MESH_BLOCK + threadIdx.x, scene = blockIdx.y;
    if (shortfall && blockIdx.x == 0 && scene == 0 && threadIdx.x == 0) {
        shortfall[0] = scan_shortfall(bases[2 * B], cap_v);
        shortfall[1] = scan_shortfall(bases[2 * B + 1], cap_t);
    }
    CellRead c;
    c.cube = 0;
    c.flags = 0;
    unsigned nt = 0;
    const bool live = cell < d.cells;
    if (live) {
        c = read_cell(grids + (size_t)scene * d.nx * d.ny * d.nz, d, cell, isof);
        nt = s_ntri[c.cube];
    }
    uint2 total;
    const uint2 pre = cell_prefix(c.flags, nt, wsum, total);
    const unsigned pv = pre.x, pt = pre.y;
    if (!live || (c.flags == 0 && nt == 0)) return;
    const unsigned* w = words + (size_t)scene * d.cells;
    const uint2* bo = blk + (size_t)scene * d.nblk;
    const uint2 mine = bo[blockIdx.x];
    if (c.flags) {
        const int k = (int)(cell % d.cz);
        const unsigned r = cell / d.cz;
        const int j = (int)(r % d.cy), i = (int)(r / d.cy);
        // padded coordinates of the cell's corners (marchingcubes.h: x = lower + dx i + dx / 2 with dx = 1)
        const double x0 = i + 0.5, y0 = j + 0.5, z0 = k + 0.5, x1 = i + 1.5, y1 = j + 1.5, z1 = k + 1.5;
        unsigned long long at = bases[2 * scene] + mine.x + pv;
        const float fx = to_model(x1, d.nx, box), fy = to_model(y1, d.ny, box), fz = to_model(z1, d.nz, box);
        if (c.flags & 1) {                   // edge 6: corner 6 -> corner 7, from x1 down to x0
            if (at < cap_v) {
                float* o = vertices + 3 * at;
                o[0] = to_model(edge_point(iso, c.v[6], c.v[7], x1, x0), d.nx, box); o[1] = fy; o[2] = fz;
            }
            ++at;
        }
        if (c.flags & 2) {                   // edge 5: corner 5 -> corner 6, from y0 up to y1
            if (at < cap_v) {
                float* o = vertices + 3 * at;
                o[0] = fx; o[1] = to_model(edge_point(iso, c.v[5], c.v[6], y0, y1), d.ny, box); o[2] = fz;
            }
            ++at;
        }
        if (c.flags & 4) {                   // edge 10: corner 2 -> corner 6, from z0 up to z1
            if (at < cap_v) {
                float* o = vertices + 3 * at;
                o[0] = fx; o[1] = fy; o[2] = to_model(edge_point(iso, c.v[2], c.v[6], z0, z1), d.nz, box);
            }
        }
    }
    if (nt) {
        const unsigned long long tbase = bases[2 * scene + 1] + mine.y + pt;
        const unsigned char* tri = s_tris[c.cube];
        for (unsigned m = 0; m < nt; ++m) {
            int idx[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const unsigned o = edge_owner(tri[3 * m + q]);
                const unsigned axis = o & 3;
                const unsigned back = (o >> 2 & 1) * d.cy * d.cz + (o >> 3 & 1) * d.cz + (o >> 4 & 1);
                const unsigned oc = cell >= back ? cell - back : 0;     // (a crossed edge always has its owner inside the grid)
                const unsigned ow = w[oc];
                idx[q] = (int)(bo[oc / MESH_BLOCK].x + (ow >> 3) + __popc(ow & ((1u << axis) - 1u)));
            }
            if (tbase + m < cap_t) {
                int* o = triangles + 3 * (tbase + m);
                o[0] = idx[0]; o[1] = idx[1]; o[2] = idx[2];
            }
        }
    }
}

MeshDims mesh_dims(int nx, int ny, int nz) {
    MeshDims d;
    d.nx = nx; d.ny = ny; d.nz = nz;
    d.cy = (unsigned)ny + 1; d.cz = (unsigned)nz + 1;
    d.cells = (unsigned)(nx + 1) * d.cy * d.cz;
    d.nblk = (d.cells + MESH_BLOCK - 1) / MESH_BLOCK;
    return d;
}

struct MeshWs { size_t words, blk, bases, total; };
static MeshWs mesh_workspace(int B, int nx, int ny, int nz) {
    const MeshDims d = mesh_dims(nx, ny, nz);
    WsLayout L;
    MeshWs w;
    w.words = L.take<unsigned>((size_t)B * d.cells);
    w.blk = L.take<uint2>((size_t)B * d.nblk);
    w.bases = L.take<unsigned long long>((size_t)(B + 1) * 2);
    w.total = L.total;
    return w;
}

// the largest float <= iso: (double)v <= iso  <=>  v <= isof for every float v
static float iso_floor(double iso) {
    float f = (float)iso;
    if ((double)f > iso) f = nextafterf(f, -INFINITY);
    return f;
}

}  // namespace giga

using namespace giga;

extern "C" {

// counts and triangle entries are int32: a scene has at most 3 vertices and 5 triangles per cell
static_assert(5LL * (GIGA_MESH_MAX_N + 1) * (GIGA_MESH_MAX_N + 1) * (GIGA_MESH_MAX_N + 1) < (1LL << 31), "per-scene counts are int32");
// 0 when the shape is supported, else the error code
static int mesh_shape_check(int B, int nx, int ny, int nz) {
    if (B < 0 || nx < 2 || ny < 2 || nz < 2) return -1;
    if (nx > GIGA_MESH_MAX_N || ny > GIGA_MESH_MAX_N || nz > GIGA_MESH_MAX_N) return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    if ((long long)B * (nx + 1) * (ny + 1) * (nz + 1) >= (1LL << 31)) return -1;      // cell numbers are 32-bit
    return 0;
}

size_t giga_mesh_workspace_bytes(int B, int nx, int ny, int nz) {
    if (B <= 0 || mesh_shape_check(B, nx, ny, nz) != 0) return 0;
    return mesh_workspace(B, nx, ny, nz).total;
}

int giga_mesh_count(const float* grids, int B, int nx, int ny, int nz, double iso, void* workspace, size_t workspace_bytes,
                    int32_t* counts, void* stream) {
    if (const int rc = mesh_shape_check(B, nx, ny, nz)) return rc;
    if (B == 0) return 0;
    if (!grids || !workspace || !counts || !(iso == iso)) return -1;
    if (workspace_bytes < giga_mesh_workspace_bytes(B, nx, ny, nz)) return -4;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const MeshDims d = mesh_dims(nx, ny, nz);
    const MeshWs w = mesh_workspace(B, nx, ny, nz);
    unsigned* words = reinterpret_cast<unsigned*>(ws + w.words);
    uint2* blk = reinterpret_cast<uint2*>(ws + w.blk);
    unsigned long long* bases = reinterpret_cast<unsigned long long*>(ws + w.bases);
    GIGA_LAUNCH(mesh_classify_kernel, dim3(d.nblk, B), dim3(MESH_BLOCK), 0, s, grids, d, iso_floor(iso), words, blk);
    GIGA_LAUNCH(scene_offsets_kernel<unsigned long long>, dim3(B), dim3(SCAN_BLOCK), 0, s, reinterpret_cast<unsigned long long*>(blk),
                d.nblk, counts, static_cast<int*>(nullptr));
    GIGA_LAUNCH(scene_bases_kernel<2>, dim3(1), dim3(64), 0, s, counts, B, bases);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int giga_mesh_emit(const float* grids, int B, int nx, int ny, int nz, double iso, double box_size, const void* workspace,
                   size_t workspace_bytes, float* vertices, size_t cap_v, int32_t* triangles, size_t cap_t, int32_t* shortfall,
                   void* stream) {
    if (const int rc = mesh_shape_check(B, nx, ny, nz)) return rc;
    if (B == 0) return 0;
    if (!grids || !workspace || !(iso == iso) || !(box_size == box_size)) return -1;
    if ((cap_v > 0 && !vertices) || (cap_t > 0 && !triangles)) return -6;
    if (workspace_bytes < giga_mesh_workspace_bytes(B, nx, ny, nz)) return -4;
    const uint8_t* ws = static_cast<const uint8_t*>(workspace);
    const MeshDims d = mesh_dims(nx, ny, nz);
    const MeshWs w = mesh_workspace(B, nx, ny, nz);
    GIGA_LAUNCH(mesh_emit_kernel, dim3(d.nblk, B), dim3(MESH_BLOCK), 0, static_cast<hipStream_t>(stream), grids, d, iso_floor(iso), iso,
                box_size, reinterpret_cast<const unsigned*>(ws + w.words), reinterpret_cast<const uint2*>(ws + w.blk),
                reinterpret_cast<const unsigned long long*>(ws + w.bases), B, vertices, (unsigned long long)cap_v, triangles,
                (unsigned long long)cap_t, shortfall);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // extern "C"
