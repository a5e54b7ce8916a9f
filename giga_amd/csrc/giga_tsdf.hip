// Dense export of a sparse TSDF voxel list: the device counterpart of TSDFVolume.get_grid
// (reference src/vgn/perception.py:107-115), the Python loop the reference itself marks "very slow (~35 ms / 50 ms of the
// whole pipeline)":
//     tsdf_grid = np.zeros((1, R, R, R), np.float32)
//     for voxel in voxels:  i, j, k = voxel.grid_index;  tsdf_grid[0, i, j, k] = voxel.color[0]
// for B scenes at once.  HBM-bound byte work (4 B per cell cleared + 16 B per voxel): no MFMA, no LDS.  The loop's
// semantics for a repeated index -- the LAST voxel of the list wins -- are kept deterministically: pass 1 records for every
// cell the highest list position that targets it (atomicMax on an int32 grid), pass 2 lets exactly that voxel write.
// Indices outside [0, R) are ignored on the device (numpy would raise; the Python wrapper checks host-side inputs).
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "giga_check.h"
#include "giga_scan.h"
#include "giga_ws.h"
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace giga {

// scene of global voxel v: largest b with offsets[b] <= v (B is small: binary search in registers)
__device__ __forceinline__ int scene_of(const int* __restrict__ offsets, int B, int v) {
    int lo = 0, hi = B;                       // offsets[lo] <= v < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void tsdf_claim_kernel(const int* __restrict__ index, const int* __restrict__ offsets, int B, int R, int n,
                                  int* __restrict__ winner) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int i = index[3 * v], j = index[3 * v + 1], k = index[3 * v + 2];
    if ((unsigned)i >= (unsigned)R || (unsigned)j >= (unsigned)R || (unsigned)k >= (unsigned)R) return;
    const int b = scene_of(offsets, B, v);
    atomicMax(winner + ((size_t)b * R + i) * R * R + j * R + k, v);
}

__global__ void tsdf_write_kernel(const int* __restrict__ index, const float* __restrict__ value,
                                  const int* __restrict__ offsets, int B, int R, int n, const int* __restrict__ winner,
                                  float* __restrict__ grid) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int i = index[3 * v], j = index[3 * v + 1], k = index[3 * v + 2];
    if ((unsigned)i >= (unsigned)R || (unsigned)j >= (unsigned)R || (unsigned)k >= (unsigned)R) return;
    const int b = scene_of(offsets, B, v);
    const size_t cell = ((size_t)b * R + i) * R * R + j * R + k;
    if (winner[cell] == v) grid[cell] = value[v];
}

// ---------------------------------------------------------------------------------------------------------------------------
// Fusion of depth images into the volume: the device counterpart of vgn.perception.TSDFVolume.integrate / get_grid / get_cloud
// (reference src/vgn/perception.py:63-126), which hand the work to Open3D's UniformTSDFVolume (NoColor).  The arithmetic below
// restates that algorithm operation by operation (include/giga_hip.h spells it out); every operation is one IEEE rounding --
// no contraction from here on -- so that a numpy restatement reproduces the bytes (tests/tsdf_emu.py).
//
//   integrate  one lane per voxel, z fastest across lanes: the state (tsdf, weight) and the exported grid are read and written
//              once per call, coalesced.  The lane loops over its scene's views with tsdf and weight in registers: no atomics,
//              and the result does not depend on the launch shape or on the other scenes of the batch.  The camera of a view is
//              read through a wave-uniform address (scene = blockIdx.y), so it lives in scalar registers; the only divergent
//              access is the depth gather, where neighbouring z-voxels project to the same or neighbouring pixels.
//   cloud      zero crossings between a voxel and its +x, +y, +z neighbour (extract_point_cloud without normals): count
//              (ballot + popcount inside a wave, LDS across the four waves, per-workgroup sums), scan (one workgroup per scene,
//              then one wave over the scenes), emit at (scene base + workgroup offset + prefix).  Order: cell order, then axis
//              0, 1, 2; no atomics decide it (giga_scan.h, the scheme of giga_mesh.hip).
//              The oriented emit adds the normal of every point (GetNormalAt): 48 reads of the stored tsdf around the cell per
//              point, through the caches; neighbouring lanes share most of them.
#pragma clang fp contract(off)

constexpr int TSDF_BLOCK = 256;
constexpr int TSDF_WAVES = TSDF_BLOCK / 64;
constexpr int TSDF_CAM = 20;                  // doubles per view in the workspace: extrinsic [16] row-major, fx, fy, cx, cy

struct TsdfVol {
    double voxel;                             // length / R
    float neg_trunc, inv_trunc;               // -float(sdf_trunc), float(1 / sdf_trunc)
    float depth_scale, depth_trunc;
    int R, W, H;
    unsigned cells;                           // R^3
};

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_integrate_kernel(const float* __restrict__ depth, const int* __restrict__ view_offsets,
                                                                    const double* __restrict__ cams, TsdfVol g,
                                                                    float* __restrict__ tsdf, float* __restrict__ weight,
                                                                    float* __restrict__ grid) {
    const unsigned cell = blockIdx.x * TSDF_BLOCK + threadIdx.x, scene = blockIdx.y;
    if (cell >= g.cells) return;
    const unsigned R = (unsigned)g.R;
    const unsigned z = cell % R, xy = cell / R, y = xy % R, x = xy / R;
    const double px = ((double)x + 0.5) * g.voxel, py = ((double)y + 0.5) * g.voxel, pz = ((double)z + 0.5) * g.voxel;
    const size_t at = (size_t)scene * g.cells + cell;
    float t = tsdf[at], w = weight[at];
    const int v0 = view_offsets[scene], v1 = view_offsets[scene + 1];
    const size_t pixels = (size_t)g.W * g.H;
    const double umax = (double)g.W - 0.0001, vmax = (double)g.H - 0.0001;
    for (int v = v0; v < v1; ++v) {
        const double* __restrict__ c = cams + (size_t)v * TSDF_CAM;          // wave-uniform address: scalar loads
        const double cz = ((c[8] * px + c[9] * py) + c[10] * pz) + c[11];
        if (!(cz > 0.0)) continue;
        const double cx = ((c[0] * px + c[1] * py) + c[2] * pz) + c[3];
        const double cy = ((c[4] * px + c[5] * py) + c[6] * pz) + c[7];
        const double fx = c[16], fy = c[17], ox = c[18], oy = c[19];
        const double uf = (cx * fx / cz + ox) + 0.5, vf = (cy * fy / cz + oy) + 0.5;
        if (!(uf >= 0.0001 && uf < umax && vf >= 0.0001 && vf < vmax)) continue;
        const int u = (int)uf, r = (int)vf;                                   // 0 <= u < W, 0 <= r < H by the test above
        float d = depth[(size_t)v * pixels + (size_t)r * g.W + u] / g.depth_scale;
        if (d >= g.depth_trunc) d = 0.f;
        if (!(d > 0.f)) continue;
        const double a = ((double)u - ox) / fx, b = ((double)r - oy) / fy;
        const float m = (float)sqrt((a * a + b * b) + 1.0);
        const float sdf = (float)(((double)d - cz) * (double)m);
        if (!(sdf > g.neg_trunc)) continue;
        const float s = fminf(1.0f, sdf * g.inv_trunc);
        t = (t * w + s) / (w + 1.0f);
        w += 1.0f;
    }
    tsdf[at] = t;
    weight[at] = w;
    if (grid) grid[at] = (w != 0.f && (double)t >= -0.98 && (double)t < 0.98) ? (float)(((double)t + 1.0) * 0.5) : 0.f;
}

struct IntegrateWs { size_t offs, cams, total; };
static IntegrateWs integrate_workspace(int B, int n_views) {
    WsLayout L;
    IntegrateWs w;
    w.offs = L.take<int>((size_t)B + 1);
    w.cams = L.take<double>((size_t)n_views * TSDF_CAM);
    w.total = L.total;
    return w;
}

static int launch_tsdf_integrate(const float* depth, const int* view_offsets, const double* extrinsics, const double* intrinsics, int B,
                                 int W, int H, double length, int R, double sdf_trunc, double depth_scale, double depth_trunc, float* tsdf,
                                 float* weight, float* grid, uint8_t* ws, hipStream_t s) {
    const int n = view_offsets[B];
    const IntegrateWs w = integrate_workspace(B, n);
    int* offs = reinterpret_cast<int*>(ws + w.offs);
    double* cams = reinterpret_cast<double*>(ws + w.cams);
    // (pageable host memory: the copies have left the caller's arrays when the call returns)
    if (hipMemcpyAsync(offs, view_offsets, (size_t)(B + 1) * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    if (n > 0) {
        std::vector<double> host((size_t)n * TSDF_CAM);
        for (int v = 0; v < n; ++v) {
            std::memcpy(&host[(size_t)v * TSDF_CAM], extrinsics + 16 * (size_t)v, 16 * sizeof(double));
            std::memcpy(&host[(size_t)v * TSDF_CAM + 16], intrinsics + 4 * (size_t)v, 4 * sizeof(double));
        }
        if (hipMemcpyAsync(cams, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    }
    TsdfVol g;
    g.voxel = length / (double)R;
    g.neg_trunc = -(float)sdf_trunc;
    g.inv_trunc = (float)(1.0 / sdf_trunc);
    g.depth_scale = (float)depth_scale;
    g.depth_trunc = (float)depth_trunc;
    g.R = R; g.W = W; g.H = H;
    g.cells = (unsigned)R * R * R;
    GIGA_LAUNCH(tsdf_integrate_kernel, dim3((g.cells + TSDF_BLOCK - 1) / TSDF_BLOCK, B), dim3(TSDF_BLOCK), 0, s, depth, offs, cams, g,
                tsdf, weight, grid);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

// ---- zero-crossing points ----
struct CloudRead { float f0, f1[3]; unsigned flags; unsigned x, y, z; };

__device__ __forceinline__ bool tsdf_valid(float t, float w) { return w != 0.f && (double)t >= -0.98 && (double)t < 0.98; }

// flags bit i: the edge from the cell to its neighbour along axis i holds a point
__device__ __forceinline__ CloudRead cloud_read(const float* __restrict__ tsdf, const float* __restrict__ weight, unsigned R,
                                                unsigned cell) {
    CloudRead c;
    c.z = cell % R;
    const unsigned xy = cell / R;
    c.y = xy % R;
    c.x = xy / R;
    c.flags = 0;
    c.f0 = tsdf[cell];
    c.f1[0] = c.f1[1] = c.f1[2] = 0.f;
    if (!tsdf_valid(c.f0, weight[cell])) return c;
    const unsigned n[3] = {c.x, c.y, c.z}, stride[3] = {R * R, R, 1u};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (n[i] + 1 >= R - 1) continue;
        const unsigned nb = cell + stride[i];
        const float f1 = tsdf[nb];
        if (tsdf_valid(f1, weight[nb]) && c.f0 * f1 < 0.f) { c.flags |= 1u << i; c.f1[i] = f1; }
    }
    return c;
}

// exclusive prefix of the number of set flags over the workgroup's cells, in cell order; the workgroup's total in tot
__device__ __forceinline__ unsigned cloud_prefix(unsigned flags, unsigned* wsum, unsigned& tot) {
    const unsigned lane = threadIdx.x & 63;
    unsigned sum;
    const unsigned pre = wave_excl_bits3<1, 1>(flags, lane, sum);
    return block_combine<TSDF_WAVES>(pre, sum, lane == 0, wsum, tot);
}

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_cloud_count_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                      unsigned R, unsigned cells, unsigned nblk,
                                                                      unsigned* __restrict__ blk) {
    __shared__ unsigned wsum[TSDF_WAVES];
    const unsigned cell = blockIdx.x * TSDF_BLOCK + threadIdx.x, scene = blockIdx.y;
    const size_t base = (size_t)scene * cells;
    const unsigned flags = cell < cells ? cloud_read(tsdf + base, weight + base, R, cell).flags : 0u;
    unsigned tot;
    cloud_prefix(flags, wsum, tot);
    if (threadIdx.x == 0) blk[(size_t)scene * nblk + blockIdx.x] = tot;
}

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_cloud_emit_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                     unsigned R, unsigned cells, unsigned nblk, double voxel,
                                                                     const unsigned* __restrict__ blk,
                                                                     const unsigned long long* __restrict__ bases, int B,
                                                                     float* __restrict__ points, unsigned long long cap,
                                                                     int* __restrict__ shortfall) {
    __shared__ unsigned wsum[TSDF_WAVES];
    const unsigned cell = blockIdx.x * TSDF_BLOCK + threadIdx.x, scene = blockIdx.y;
    if (shortfall && blockIdx.x == 0 && scene == 0 && threadIdx.x == 0) shortfall[0] = scan_shortfall(bases[B], cap);
    const size_t base = (size_t)scene * cells;
    CloudRead c;
    c.flags = 0;
    if (cell < cells) c = cloud_read(tsdf + base, weight + base, R, cell);
    unsigned tot;
    const unsigned pre = cloud_prefix(c.flags, wsum, tot);
    if (!c.flags) return;
    unsigned long long at = bases[scene] + blk[(size_t)scene * nblk + blockIdx.x] + pre;
    const double p0[3] = {((double)c.x + 0.5) * voxel, ((double)c.y + 0.5) * voxel, ((double)c.z + 0.5) * voxel};
    const double a0 = fabs((double)c.f0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (!(c.flags >> i & 1)) continue;
        if (at < cap) {
            const double a1 = fabs((double)c.f1[i]);
            float* o = points + 3 * at;
#pragma unroll
            for (int q = 0; q < 3; ++q) o[q] = (float)p0[q];
            o[i] = (float)((p0[i] * a1 + (p0[i] + voxel) * a0) / (a0 + a1));
        }
        ++at;
    }
}

// ---- zero-crossing points with normals (UniformTSDFVolume::GetNormalAt, restated in include/giga_hip.h) ----
// s = q / voxel - 0.5 along one axis, split into the cell index and the weight of the cell after it
struct TriAxis { int i; double r; };
__device__ __forceinline__ TriAxis tri_axis(double q, double voxel) {
    const double s = q / voxel - 0.5, f = floor(s);
    return TriAxis{(int)f, s - f};
}

// trilinear value of the stored tsdf (the weight is not consulted); a voxel outside the volume counts 0.0
__device__ __forceinline__ double tsdf_trilinear(const float* __restrict__ tsdf, unsigned R, TriAxis x, TriAxis y, TriAxis z) {
    const double wx[2] = {1.0 - x.r, x.r}, wy[2] = {1.0 - y.r, y.r}, wz[2] = {1.0 - z.r, z.r};
    double acc = 0.0;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const int dx = d >> 2, dy = d >> 1 & 1, dz = d & 1;
        const unsigned ix = (unsigned)(x.i + dx), iy = (unsigned)(y.i + dy), iz = (unsigned)(z.i + dz);
        const bool inside = ix < R && iy < R && iz < R;                       // (a negative index wraps to a large one)
        const double f = inside ? (double)tsdf[((size_t)ix * R + iy) * R + iz] : 0.0;
        const double term = ((wx[dx] * wy[dy]) * wz[dz]) * f;
        acc = d == 0 ? term : acc + term;
    }
    return acc;
}

// the normal at the float64 point p: central differences of the trilinear value at -g and +g along every axis
__device__ __forceinline__ void tsdf_normal(const float* __restrict__ vol, unsigned R, double voxel, const double* p, float* nv) {
    const double g = 0.99 * voxel;
    TriAxis mid[3], lo[3], hi[3];                                             // the three axes at p, and each of them moved by -g and +g
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        mid[q] = tri_axis(p[q], voxel);
        lo[q] = tri_axis(p[q] - g, voxel);
        hi[q] = tri_axis(p[q] + g, voxel);
    }
    const double n0 = tsdf_trilinear(vol, R, hi[0], mid[1], mid[2]) - tsdf_trilinear(vol, R, lo[0], mid[1], mid[2]);
    const double n1 = tsdf_trilinear(vol, R, mid[0], hi[1], mid[2]) - tsdf_trilinear(vol, R, mid[0], lo[1], mid[2]);
    const double n2 = tsdf_trilinear(vol, R, mid[0], mid[1], hi[2]) - tsdf_trilinear(vol, R, mid[0], mid[1], lo[2]);
    const double zz = (n0 * n0 + n1 * n1) + n2 * n2;
    if (zz > 0.0) {
        const double len = sqrt(zz);
        nv[0] = (float)(n0 / len); nv[1] = (float)(n1 / len); nv[2] = (float)(n2 / len);
    } else {
        nv[0] = nv[1] = nv[2] = 0.f;
    }
}

// The emit kernel's points, bit for bit -- one lane per cell, the same prefix and the same positions -- and the normal of each.
// A crossing is rare (one cell in a hundred of a fused scene) and a normal is long (48 reads, a dozen float64 divisions), so the
// lanes that hold one would drag their whole wave through the normal for one or two of 64 lanes.  Instead a lane leaves every
// crossing in LDS, at its position inside the workgroup (cell | axis << 30, and the crossing's coordinate in float64), and after
// a barrier the workgroup's first `tot` lanes take one crossing each: dense waves.  Measured in DESIGN section 3w.
constexpr unsigned CLOUD_QUEUE = 3 * TSDF_BLOCK;   // a workgroup's crossings at most
static_assert((unsigned long long)GIGA_TSDF_MAX_R * GIGA_TSDF_MAX_R * GIGA_TSDF_MAX_R <= 1ull << 30, "a cell index and an axis share a word");

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_cloud_emit_oriented_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                              unsigned R, unsigned cells, unsigned nblk, double voxel,
                                                                              const unsigned* __restrict__ blk,
                                                                              const unsigned long long* __restrict__ bases, int B,
                                                                              float* __restrict__ points, float* __restrict__ normals,
                                                                              unsigned long long cap, int* __restrict__ shortfall) {
    __shared__ unsigned wsum[TSDF_WAVES];
    __shared__ unsigned q_cell[CLOUD_QUEUE];
    __shared__ double q_at[CLOUD_QUEUE];
    const unsigned cell = blockIdx.x * TSDF_BLOCK + threadIdx.x, scene = blockIdx.y;
    if (shortfall && blockIdx.x == 0 && scene == 0 && threadIdx.x == 0) shortfall[0] = scan_shortfall(bases[B], cap);
    const size_t base = (size_t)scene * cells;
    CloudRead c;
    c.flags = 0;
    if (cell < cells) c = cloud_read(tsdf + base, weight + base, R, cell);
    unsigned tot;
    unsigned pre = cloud_prefix(c.flags, wsum, tot);
    if (tot == 0) return;                                                     // (the whole workgroup)
    const unsigned long long first = bases[scene] + blk[(size_t)scene * nblk + blockIdx.x];
    if (c.flags) {
        const double p0[3] = {((double)c.x + 0.5) * voxel, ((double)c.y + 0.5) * voxel, ((double)c.z + 0.5) * voxel};
        const double a0 = fabs((double)c.f0);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (!(c.flags >> i & 1)) continue;
            const double a1 = fabs((double)c.f1[i]);
            const double r = (p0[i] * a1 + (p0[i] + voxel) * a0) / (a0 + a1);
            q_cell[pre] = cell | (unsigned)i << 30;
            q_at[pre] = r;
            if (first + pre < cap) {
                float* o = points + 3 * (first + pre);
#pragma unroll
                for (int q = 0; q < 3; ++q) o[q] = (float)p0[q];
                o[i] = (float)r;
            }
            ++pre;
        }
    }
    __syncthreads();
    const float* __restrict__ vol = tsdf + base;
    for (unsigned t = threadIdx.x; t < tot; t += TSDF_BLOCK) {
        if (first + t >= cap) break;
        const unsigned at = q_cell[t] & 0x3fffffffu, axis = q_cell[t] >> 30;
        const unsigned z = at % R, xy = at / R, y = xy % R, x = xy / R;
        double p[3] = {((double)x + 0.5) * voxel, ((double)y + 0.5) * voxel, ((double)z + 0.5) * voxel};
        const double r = q_at[t];
        if (axis == 0) p[0] = r; else if (axis == 1) p[1] = r; else p[2] = r;
        tsdf_normal(vol, R, voxel, p, normals + 3 * (first + t));
    }
}

struct CloudWs { size_t blk, bases, total; unsigned cells, nblk; };
static CloudWs cloud_workspace(int B, int R) {
    WsLayout L;
    CloudWs w;
    w.cells = (unsigned)R * R * R;
    w.nblk = (w.cells + TSDF_BLOCK - 1) / TSDF_BLOCK;
    w.blk = L.take<unsigned>((size_t)B * w.nblk);
    w.bases = L.take<unsigned long long>((size_t)B + 1);
    w.total = L.total;
    return w;
}

}  // namespace giga

using namespace giga;

extern "C" {

size_t giga_tsdf_scatter_workspace_bytes(int B, int R) {
    if (B <= 0 || R <= 0) return 0;
    return (size_t)B * R * R * R * sizeof(int32_t);
}

int giga_tsdf_scatter(const int32_t* voxel_index, const float* voxel_value, const int32_t* scene_offsets, int B, int R,
                      int n_voxels, float* grid, void* workspace, size_t workspace_bytes, void* stream) {
    if (B < 0 || R <= 0 || R > 1024 || n_voxels < 0) return -1;
    if (B == 0) return 0;
    if (!grid || !scene_offsets) return -1;
    if (n_voxels > 0 && (!voxel_index || !voxel_value || !workspace)) return -1;
    if (n_voxels > 0 && workspace_bytes < giga_tsdf_scatter_workspace_bytes(B, R)) return -4;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int* winner = static_cast<int*>(workspace);
    const size_t cells = (size_t)B * R * R * R;
    if (hipMemsetAsync(grid, 0, cells * sizeof(float), s) != hipSuccess) return -10;
    if (n_voxels <= 0) return 0;
    if (hipMemsetAsync(winner, 0xFF, cells * sizeof(int), s) != hipSuccess) return -10;      // -1 everywhere
    const unsigned blocks = (unsigned)((n_voxels + 255) / 256);
    GIGA_LAUNCH(tsdf_claim_kernel, dim3(blocks), dim3(256), 0, s, voxel_index, scene_offsets, B, R, n_voxels, winner);
    GIGA_LAUNCH(tsdf_write_kernel, dim3(blocks), dim3(256), 0, s, voxel_index, voxel_value, scene_offsets, B, R, n_voxels, winner, grid);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

static int tsdf_volume_check(int B, int R) {
    if (B < 0 || R < 2 || R > GIGA_TSDF_MAX_R) return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    return 0;
}

size_t giga_tsdf_integrate_workspace_bytes(int B, int n_views) {
    if (B <= 0 || B > GIGA_MAX_SCENES || n_views < 0) return 0;
    return integrate_workspace(B, n_views).total;
}

int giga_tsdf_integrate(const float* depth, const int32_t* view_offsets, const double* extrinsics, const double* intrinsics, int B,
                        int width, int height, double length, int R, double sdf_trunc, double depth_scale, double depth_trunc,
                        float* tsdf, float* weight, float* grid, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = tsdf_volume_check(B, R)) return rc;
    if (width < 1 || height < 1 || width > GIGA_TSDF_MAX_IMAGE || height > GIGA_TSDF_MAX_IMAGE) return -1;
    if (!finite_f64(length) || !(length > 0.0) || !finite_f64(sdf_trunc) || !(sdf_trunc > 0.0) || !finite_f64(depth_scale) ||
        !(depth_scale > 0.0) || !(depth_trunc == depth_trunc))
        return -1;
    if (B == 0) return 0;
    if (!ragged_ok(view_offsets, B)) return -1;
    const int n = view_offsets[B];
    if ((long long)n * width * height >= (1LL << 40)) return -1;
    if (!camera_check(n, extrinsics, intrinsics) || (n > 0 && !depth)) return -1;
    if (!tsdf || !weight || !workspace) return -1;
    if (workspace_bytes < giga_tsdf_integrate_workspace_bytes(B, n)) return -4;
    return launch_tsdf_integrate(depth, view_offsets, extrinsics, intrinsics, B, width, height, length, R, sdf_trunc, depth_scale,
                                 depth_trunc, tsdf, weight, grid, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

size_t giga_tsdf_cloud_workspace_bytes(int B, int R) {
    if (B <= 0 || tsdf_volume_check(B, R) != 0) return 0;
    return cloud_workspace(B, R).total;
}

int giga_tsdf_cloud_count(const float* tsdf, const float* weight, int B, int R, void* workspace, size_t workspace_bytes,
                          int32_t* counts, void* stream) {
    if (const int rc = tsdf_volume_check(B, R)) return rc;
    if (B == 0) return 0;
    if (!tsdf || !weight || !workspace || !counts) return -1;
    if (workspace_bytes < giga_tsdf_cloud_workspace_bytes(B, R)) return -4;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const CloudWs w = cloud_workspace(B, R);
    unsigned* blk = reinterpret_cast<unsigned*>(ws + w.blk);
    unsigned long long* bases = reinterpret_cast<unsigned long long*>(ws + w.bases);
    GIGA_LAUNCH(tsdf_cloud_count_kernel, dim3(w.nblk, B), dim3(TSDF_BLOCK), 0, s, tsdf, weight, (unsigned)R, w.cells, w.nblk, blk);
    GIGA_LAUNCH(scene_offsets_kernel<unsigned>, dim3(B), dim3(SCAN_BLOCK), 0, s, blk, w.nblk, counts, static_cast<int*>(nullptr));
    GIGA_LAUNCH(scene_bases_kernel<1>, dim3(1), dim3(64), 0, s, counts, B, bases);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int giga_tsdf_cloud_emit(const float* tsdf, const float* weight, int B, int R, double length, const void* workspace,
                         size_t workspace_bytes, float* points, size_t cap, int32_t* shortfall, void* stream) {
    if (const int rc = tsdf_volume_check(B, R)) return rc;
    if (!finite_f64(length) || !(length > 0.0)) return -1;
    if (B == 0) return 0;
    if (!tsdf || !weight || !workspace) return -1;
    if (cap > 0 && !points) return -6;
    if (workspace_bytes < giga_tsdf_cloud_workspace_bytes(B, R)) return -4;
    const uint8_t* ws = static_cast<const uint8_t*>(workspace);
    const CloudWs w = cloud_workspace(B, R);
    GIGA_LAUNCH(tsdf_cloud_emit_kernel, dim3(w.nblk, B), dim3(TSDF_BLOCK), 0, static_cast<hipStream_t>(stream), tsdf, weight, (unsigned)R,
                w.cells, w.nblk, length / (double)R, reinterpret_cast<const unsigned*>(ws + w.blk),
                reinterpret_cast<const unsigned long long*>(ws + w.bases), B, points, (unsigned long long)cap, shortfall);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int giga_tsdf_cloud_emit_oriented(const float* tsdf, const float* weight, int B, int R, double length, const void* workspace,
                                  size_t workspace_bytes, float* points, float* normals, size_t cap, int32_t* shortfall, void* stream) {
    if (const int rc = tsdf_volume_check(B, R)) return rc;
    if (!finite_f64(length) || !(length > 0.0)) return -1;
    if (B == 0) return 0;
    if (!tsdf || !weight || !workspace) return -1;
    if (cap > 0 && (!points || !normals)) return -6;
    if (workspace_bytes < giga_tsdf_cloud_workspace_bytes(B, R)) return -4;
    const uint8_t* ws = static_cast<const uint8_t*>(workspace);
    const CloudWs w = cloud_workspace(B, R);
    GIGA_LAUNCH(tsdf_cloud_emit_oriented_kernel, dim3(w.nblk, B), dim3(TSDF_BLOCK), 0, static_cast<hipStream_t>(stream), tsdf, weight,
                (unsigned)R, w.cells, w.nblk, length / (double)R, reinterpret_cast<const unsigned*>(ws + w.blk),
                reinterpret_cast<const unsigned long long*>(ws + w.bases), B, points, normals, (unsigned long long)cap, shortfall);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // extern "C"
