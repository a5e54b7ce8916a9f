// Depth images of posed triangle meshes: the device counterpart of the depth half of btsim.Camera.render (reference
// src/vgn/utils/btsim.py:276-337), which the reference hands to PyBullet's renderer.  The semantics are this project's own and are
// spelled out in include/giga_hip.h (giga_depth_render): a double-precision, watertight ray / triangle test per pixel centre, the
// minimum accepted camera-space z per pixel, `far` where nothing is hit.  Every operation is one IEEE rounding -- no contraction
// in this file -- so that a numpy restatement reproduces the bytes (tests/render_emu.py).
//
//   one workgroup per (16 x 16 pixel tile, view), one lane per pixel: no atomics decide a pixel.
//   The workgroup walks its scene's triangles 256 at a time, one triangle per lane: the lane transforms the three vertices into
//   the camera frame, forms the three edge normals n = P x Q (they do not depend on the pixel) and decides whether ANY pixel of
//   the tile can accept the triangle.  That decision uses the very numbers the pixels will compute: e(d) = (d.x n.x + d.y n.y) + n.z
//   is, rounding included, monotone in d.x and in d.y (a rounded product or sum is monotone in each operand), and d is monotone in
//   the pixel index, so the smallest and largest e over the tile's pixels are its values at two corner pixels.  A pixel is hit
//   only if U, V, W are all >= 0 or all <= 0; the tile can be skipped when some edge is < 0 on every pixel AND some edge is > 0
//   on every pixel.  No margin is needed, vertices behind the camera need no special case, and a NaN makes every comparison
//   false, which keeps the triangle.  The second reason to skip is depth: an accepted z is a convex combination of the three
//   vertex depths, so all three < near or all three > far cannot be accepted.
//   Survivors are compacted (ballot + popcount inside a wave, LDS across the four waves, as giga_mesh.hip does) into an LDS list
//   of 12 doubles each (three normals, three depths).  When the list cannot take another 256 it is flushed: every lane runs the
//   test of its pixel against each entry; all lanes read the same entry, so the LDS read is a broadcast.
//
// Shaded images (giga_color_render) are the same walk with the winner kept -- smallest z, then smallest triangle index, so the
// image does not depend on the order of the tests -- and one flat, two-sided shade per pixel after it, in double as well
// (tests/shade_emu.py); giga_image_downsample is the exact k x k box filter behind `supersample`.
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "giga_check.h"
#include "giga_ws.h"
#include <cstdint>
#include <cstring>
#include <vector>

namespace giga {

#pragma clang fp contract(off)

constexpr int RENDER_TILE = 16;                   // pixels per tile side
constexpr int RENDER_BLOCK = RENDER_TILE * RENDER_TILE;
constexpr int RENDER_WAVES = RENDER_BLOCK / 64;
constexpr int RENDER_CAP = 384;                   // LDS list: 384 x 96 B = 36 KB, + 384 x 4 B of indices when shading (four workgroups per CU)
constexpr int RENDER_CAM = 20;                    // doubles per view in the workspace: extrinsic [16] row-major, fx, fy, cx, cy
static_assert(RENDER_CAP >= 2 * RENDER_BLOCK - 128 && RENDER_CAP >= RENDER_BLOCK, "a flush leaves room for one more chunk");

struct RenderTri {                                // what a pixel needs of a triangle (a, b, c in the camera frame)
    double nbc[3], nca[3], nab[3];                // b x c, c x a, a x b
    double az, bz, cz;
};

struct RenderArgs {
    const float* vertices;
    const int* triangles;
    const uint32_t* colors;                       // shading only: per-triangle RGBA, lights [view][4], the three images
    const double* lights;
    uint32_t* rgba;
    int* winner;
    double ambient;
    uint32_t background;
    const int* voffs;                             // workspace copies (device)
    const int* toffs;
    const int* view_scene;
    const double* cams;
    unsigned long long* tested;                   // measurement aid: triangle-tile pairs that survived the culling
    float* depth;
    double near, far, pixel_offset;
    int W, H, tiles_x, tiles;                     // tiles per view
};

__device__ __forceinline__ void render_cross(const double* P, const double* Q, double* n) {
    n[0] = P[1] * Q[2] - P[2] * Q[1];
    n[1] = P[2] * Q[0] - P[0] * Q[2];
    n[2] = P[0] * Q[1] - P[1] * Q[0];
}

__device__ __forceinline__ double render_edge(double dx, double dy, const double* n) { return (dx * n[0] + dy * n[1]) + n[2]; }

// smallest and largest e over the pixels of a tile whose directions span [x0, x1] x [y0, y1] (see the head of the file)
__device__ __forceinline__ void render_edge_range(const double* n, double x0, double x1, double y0, double y1, double& lo, double& hi) {
    const bool px = n[0] >= 0.0, py = n[1] >= 0.0;
    lo = render_edge(px ? x0 : x1, py ? y0 : y1, n);
    hi = render_edge(px ? x1 : x0, py ? y1 : y0, n);
}

// floor(k C + 0.5), at most 255: one channel of a shaded face
__device__ __forceinline__ uint32_t render_level(double k, uint32_t C) { return (uint32_t)fmin(floor(k * (double)C + 0.5), 255.0); }

// The tile walk of both kernels.  SHADE keeps the winner (the list entry gains the triangle's index in a second LDS array) and
// shades the pixel once after the walk; without it the code is the depth renderer's as it was.
template <bool SHADE>
__device__ __forceinline__ void render_tile(const RenderArgs& g) {
    __shared__ RenderTri list[RENDER_CAP];
    __shared__ int lidx[SHADE ? RENDER_CAP : 1];  // the entries' triangle indices, relative to the scene
    __shared__ int wcnt[2][RENDER_WAVES];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int view = (int)(blockIdx.x / (unsigned)g.tiles), tile = (int)(blockIdx.x % (unsigned)g.tiles);
    const int u0 = (tile % g.tiles_x) * RENDER_TILE, v0 = (tile / g.tiles_x) * RENDER_TILE;
    const int u = u0 + (int)(tid & (RENDER_TILE - 1)), v = v0 + (int)(tid / RENDER_TILE);
    const double* __restrict__ c = g.cams + (size_t)view * RENDER_CAM;        // wave-uniform address: scalar loads
    const double fx = c[16], fy = c[17], ox = c[18], oy = c[19];
    const double dx = (((double)u + g.pixel_offset) - ox) / fx, dy = (((double)v + g.pixel_offset) - oy) / fy;
    // directions of the tile's first and last pixel inside the image
    const int u1 = min(u0 + RENDER_TILE, g.W) - 1, v1 = min(v0 + RENDER_TILE, g.H) - 1;
    const double xa = (((double)u0 + g.pixel_offset) - ox) / fx, xb = (((double)u1 + g.pixel_offset) - ox) / fx;
    const double ya = (((double)v0 + g.pixel_offset) - oy) / fy, yb = (((double)v1 + g.pixel_offset) - oy) / fy;
    const double x0 = fmin(xa, xb), x1 = fmax(xa, xb), y0 = fmin(ya, yb), y1 = fmax(ya, yb);

    const int scene = g.view_scene[view];
    const int vbase = g.voffs[scene], nv = g.voffs[scene + 1] - vbase;
    const int t0 = g.toffs[scene], t1 = g.toffs[scene + 1];
    const float* __restrict__ vert = g.vertices + 3 * (size_t)vbase;

    double best = __builtin_huge_val();
    int win = -1;                                 // SHADE: the triangle that gave `best`
    int count = 0, parity = 0;                    // entries in the list (the same number in every lane)
    unsigned long long tested = 0;

    auto flush = [&]() {
        __syncthreads();
        for (int s = 0; s < count; ++s) {
            const RenderTri& t = list[s];         // every lane reads the same entry: broadcast
            const double U = render_edge(dx, dy, t.nbc), V = render_edge(dx, dy, t.nca), Wd = render_edge(dx, dy, t.nab);
            const double S = (U + V) + Wd;
            const bool pos = U >= 0.0 && V >= 0.0 && Wd >= 0.0, neg = U <= 0.0 && V <= 0.0 && Wd <= 0.0;
            if (S != 0.0 && (pos || neg)) {
                const double z = ((U * t.az + V * t.bz) + Wd * t.cz) / S;
                if constexpr (SHADE) {
                    const int idx = lidx[s];
                    if (z >= g.near && z <= g.far && (z < best || (z == best && idx < win))) { best = z; win = idx; }
                } else {
                    if (z >= g.near && z <= g.far && z < best) best = z;
                }
            }
        }
        tested += (unsigned long long)count;
        __syncthreads();
        count = 0;
    };

    for (int base = t0; base < t1; base += RENDER_BLOCK) {
        const int tri = base + (int)tid;
        bool keep = false;
        RenderTri t;
        if (tri < t1) {
            const int* __restrict__ f = g.triangles + 3 * (size_t)tri;
            const int ia = f[0], ib = f[1], ic = f[2];
            if ((unsigned)ia < (unsigned)nv && (unsigned)ib < (unsigned)nv && (unsigned)ic < (unsigned)nv) {
                const int idx[3] = {ia, ib, ic};
                double p[3][3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float* __restrict__ q = vert + 3 * (size_t)idx[k];
                    const double x = (double)q[0], y = (double)q[1], z = (double)q[2];
#pragma unroll
                    for (int r = 0; r < 3; ++r) p[k][r] = ((c[4 * r] * x + c[4 * r + 1] * y) + c[4 * r + 2] * z) + c[4 * r + 3];
                }
                render_cross(p[1], p[2], t.nbc);
                render_cross(p[2], p[0], t.nca);
                render_cross(p[0], p[1], t.nab);
                t.az = p[0][2]; t.bz = p[1][2]; t.cz = p[2][2];
                double lo[3], hi[3];
                render_edge_range(t.nbc, x0, x1, y0, y1, lo[0], hi[0]);
                render_edge_range(t.nca, x0, x1, y0, y1, lo[1], hi[1]);
                render_edge_range(t.nab, x0, x1, y0, y1, lo[2], hi[2]);
                const bool never_pos = hi[0] < 0.0 || hi[1] < 0.0 || hi[2] < 0.0;      // some edge is negative on every pixel
                const bool never_neg = lo[0] > 0.0 || lo[1] > 0.0 || lo[2] > 0.0;      // some edge is positive on every pixel
                const bool too_near = t.az < g.near && t.bz < g.near && t.cz < g.near;
                const bool too_far = t.az > g.far && t.bz > g.far && t.cz > g.far;
                keep = !(never_pos && never_neg) && !too_near && !too_far;
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcnt[parity][wave] = __popcll(m);
        __syncthreads();
        int at = count + __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < RENDER_WAVES; ++w) {
            const int n = wcnt[parity][w];
            if (w < (int)wave) at += n;
            total += n;
        }
        if (keep) {                               // at < count + total <= RENDER_CAP
            list[at] = t;
            if constexpr (SHADE) lidx[at] = tri - t0;
        }
        count += total;
        parity ^= 1;
        if (count > RENDER_CAP - RENDER_BLOCK) flush();
    }
    if (count > 0) flush();

    if (u < g.W && v < g.H) {
        const size_t px = ((size_t)view * g.H + v) * g.W + u;
        if (!SHADE || g.depth) g.depth[px] = best <= g.far ? (float)best : (float)g.far;
        if constexpr (SHADE) {
            uint32_t out = g.background;
            if (win >= 0) {                       // the winner's vertices once more, not carried through the list
                const int* __restrict__ f = g.triangles + 3 * (size_t)(t0 + win);
                const int idx[3] = {f[0], f[1], f[2]};
                double p[3][3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float* __restrict__ q = vert + 3 * (size_t)idx[k];
                    const double x = (double)q[0], y = (double)q[1], z = (double)q[2];
#pragma unroll
                    for (int r = 0; r < 3; ++r) p[k][r] = ((c[4 * r] * x + c[4 * r + 1] * y) + c[4 * r + 2] * z) + c[4 * r + 3];
                }
                const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
                const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
                double n[3];
                render_cross(e1, e2, n);
                const double* __restrict__ l = g.lights + 4 * (size_t)view;
                const double L[3] = {l[0] - l[3] * (best * dx), l[1] - l[3] * (best * dy), l[2] - l[3] * best};
                const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2], ll = (L[0] * L[0] + L[1] * L[1]) + L[2] * L[2];
                const double q = nn * ll;
                double k = g.ambient;
                if (q != 0.0 && q - q == 0.0) {
                    const double nl = (n[0] * L[0] + n[1] * L[1]) + n[2] * L[2];
                    k = g.ambient + ((1.0 - g.ambient) * fabs(nl)) / sqrt(q);
                }
                const uint32_t C = g.colors[(size_t)t0 + win];
                out = render_level(k, C & 255u) | render_level(k, (C >> 8) & 255u) << 8 | render_level(k, (C >> 16) & 255u) << 16 | 255u << 24;
            }
            g.rgba[px] = out;
            if (g.winner) g.winner[px] = win;
        }
    }
    if (tid == 0 && tested) atomicAdd(g.tested, tested);
}

__global__ __launch_bounds__(RENDER_BLOCK) void depth_render_kernel(RenderArgs g) { render_tile<false>(g); }
__global__ __launch_bounds__(RENDER_BLOCK) void color_render_kernel(RenderArgs g) { render_tile<true>(g); }

// k x k box filter of RGBA bytes, exact: per channel (sum + k k / 2) / (k k).  One lane per output pixel.
__global__ __launch_bounds__(256) void image_downsample_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int total,
                                                               int W, int H, int k) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= total) return;
    const int u = i % W, v = (i / W) % H, img = i / (W * H);
    const uint32_t* __restrict__ s = src + ((size_t)img * (size_t)(k * H) + (size_t)(k * v)) * (size_t)(k * W) + (size_t)(k * u);
    uint32_t sum[4] = {0, 0, 0, 0};
    for (int y = 0; y < k; ++y)
        for (int x = 0; x < k; ++x) {
            const uint32_t C = s[(size_t)y * (size_t)(k * W) + x];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) sum[ch] += (C >> (8 * ch)) & 255u;
        }
    const uint32_t kk = (uint32_t)(k * k);
    uint32_t out = 0;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) out |= ((sum[ch] + kk / 2) / kk) << (8 * ch);
    dst[i] = out;
}

struct RenderWs { size_t tested, voffs, toffs, view_scene, cams, lights, total; };
static RenderWs render_workspace(int B, int n_views, bool shade = false) {
    WsLayout L;
    RenderWs w;
    w.tested = L.take<unsigned long long>(1);
    w.voffs = L.take<int>((size_t)B + 1);
    w.toffs = L.take<int>((size_t)B + 1);
    w.view_scene = L.take<int>((size_t)n_views);
    w.cams = L.take<double>((size_t)n_views * RENDER_CAM);
    w.lights = shade ? L.take<double>((size_t)n_views * 4) : 0;
    w.total = L.total;
    return w;
}

struct RenderShade {                              // what the colour render takes beside the depth render's arguments
    const uint8_t* face_colors;
    const double* lights;                         // host [n][4], or null: the headlight (0, 0, 0, 1)
    double ambient;
    uint32_t background;
    uint32_t* rgba;
    int* winner;
};

static int launch_render(const float* vertices, const int* vertex_offsets, const int* triangles, const int* triangle_offsets,
                         const int* view_offsets, const double* extrinsics, const double* intrinsics, int B, int W, int H, double near,
                         double far, double pixel_offset, float* depth, const RenderShade* shade, uint8_t* ws, hipStream_t s) {
    const int n = view_offsets[B];
    const RenderWs w = render_workspace(B, n, shade != nullptr);
    // one staging buffer, one copy (pageable host memory: the copy has left it when the call returns)
    std::vector<uint8_t> host(w.total, 0);
    std::memcpy(&host[w.voffs], vertex_offsets, (size_t)(B + 1) * sizeof(int));
    std::memcpy(&host[w.toffs], triangle_offsets, (size_t)(B + 1) * sizeof(int));
    int* view_scene = reinterpret_cast<int*>(&host[w.view_scene]);
    for (int b = 0; b < B; ++b)
        for (int v = view_offsets[b]; v < view_offsets[b + 1]; ++v) view_scene[v] = b;
    for (int v = 0; v < n; ++v) {
        std::memcpy(&host[w.cams + (size_t)v * RENDER_CAM * sizeof(double)], extrinsics + 16 * (size_t)v, 16 * sizeof(double));
        std::memcpy(&host[w.cams + ((size_t)v * RENDER_CAM + 16) * sizeof(double)], intrinsics + 4 * (size_t)v, 4 * sizeof(double));
    }
    if (shade) {
        double* lights = reinterpret_cast<double*>(&host[w.lights]);
        for (int v = 0; v < n; ++v)
            for (int k = 0; k < 4; ++k) lights[4 * (size_t)v + k] = shade->lights ? shade->lights[4 * (size_t)v + k] : (k == 3 ? 1.0 : 0.0);
    }
    if (hipMemcpyAsync(ws, host.data(), w.total, hipMemcpyHostToDevice, s) != hipSuccess) return -10;
    RenderArgs g;
    g.vertices = vertices;
    g.triangles = triangles;
    g.colors = shade ? reinterpret_cast<const uint32_t*>(shade->face_colors) : nullptr;
    g.lights = shade ? reinterpret_cast<const double*>(ws + w.lights) : nullptr;
    g.rgba = shade ? shade->rgba : nullptr;
    g.winner = shade ? shade->winner : nullptr;
    g.ambient = shade ? shade->ambient : 0.0;
    g.background = shade ? shade->background : 0u;
    g.voffs = reinterpret_cast<const int*>(ws + w.voffs);
    g.toffs = reinterpret_cast<const int*>(ws + w.toffs);
    g.view_scene = reinterpret_cast<const int*>(ws + w.view_scene);
    g.cams = reinterpret_cast<const double*>(ws + w.cams);
    g.tested = reinterpret_cast<unsigned long long*>(ws + w.tested);
    g.depth = depth;
    g.near = near; g.far = far; g.pixel_offset = pixel_offset;
    g.W = W; g.H = H;
    g.tiles_x = (W + RENDER_TILE - 1) / RENDER_TILE;
    g.tiles = g.tiles_x * ((H + RENDER_TILE - 1) / RENDER_TILE);
    if (shade)
        GIGA_LAUNCH(color_render_kernel, dim3((unsigned)g.tiles * (unsigned)n), dim3(RENDER_BLOCK), 0, s, g);
    else
        GIGA_LAUNCH(depth_render_kernel, dim3((unsigned)g.tiles * (unsigned)n), dim3(RENDER_BLOCK), 0, s, g);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

// what giga_depth_render and giga_color_render check alike, up to the view count; 1 = nothing to do
static int render_check(const void* vertices, const int32_t* vertex_offsets, const void* triangles, const int32_t* triangle_offsets,
                        const int32_t* view_offsets, int B, int W, int H, double near, double far, double pixel_offset) {
    if (const int rc = ragged_batch_check(B)) return rc;
    if (W < 1 || H < 1 || W > GIGA_RENDER_MAX_IMAGE || H > GIGA_RENDER_MAX_IMAGE) return -1;
    if (!finite_f64(near) || !finite_f64(far) || !(near > 0.0) || !(far > near) || !finite_f64(pixel_offset)) return -1;
    if (B == 0) return 1;
    if (!mesh_batch_check(vertex_offsets, triangle_offsets, B, vertices, triangles) || !ragged_ok(view_offsets, B)) return -1;
    if ((long long)view_offsets[B] * W * H >= (1LL << 31)) return -1;
    return 0;
}

}  // namespace giga

using namespace giga;

extern "C" {

size_t giga_depth_render_workspace_bytes(int B, int n_views, int n_vertices, int n_triangles) {
    if (B <= 0 || B > GIGA_MAX_SCENES || n_views < 0 || n_vertices < 0 || n_triangles < 0) return 0;
    return render_workspace(B, n_views).total;
}

int giga_depth_render(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                      const int32_t* view_offsets, const double* extrinsics, const double* intrinsics, int B, int W, int H, double near,
                      double far, double pixel_offset, float* depth, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = render_check(vertices, vertex_offsets, triangles, triangle_offsets, view_offsets, B, W, H, near, far, pixel_offset))
        return rc < 0 ? rc : 0;
    const int n = view_offsets[B];
    if (n == 0) return 0;
    if (!camera_check(n, extrinsics, intrinsics) || !workspace) return -1;
    if (!depth) return -6;
    if (workspace_bytes < giga_depth_render_workspace_bytes(B, n, vertex_offsets[B], triangle_offsets[B])) return -4;
    return launch_render(vertices, vertex_offsets, triangles, triangle_offsets, view_offsets, extrinsics, intrinsics, B, W, H, near, far,
                         pixel_offset, depth, nullptr, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

size_t giga_color_render_workspace_bytes(int B, int n_views, int n_vertices, int n_triangles) {
    if (B <= 0 || B > GIGA_MAX_SCENES || n_views < 0 || n_vertices < 0 || n_triangles < 0) return 0;
    return render_workspace(B, n_views, true).total;
}

int giga_color_render(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                      const uint8_t* face_colors, const int32_t* view_offsets, const double* extrinsics, const double* intrinsics,
                      const double* lights, double ambient, const uint8_t* background, int B, int W, int H, double near, double far,
                      double pixel_offset, uint32_t* rgba, float* depth, int32_t* triangle_index, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (const int rc = render_check(vertices, vertex_offsets, triangles, triangle_offsets, view_offsets, B, W, H, near, far, pixel_offset))
        return rc < 0 ? rc : 0;
    if (!(ambient >= 0.0 && ambient <= 1.0)) return -1;
    if (triangle_offsets[B] != 0 && (!face_colors || (reinterpret_cast<uintptr_t>(face_colors) & 3u))) return -1;
    const int n = view_offsets[B];
    if (n == 0) return 0;
    if (!camera_check(n, extrinsics, intrinsics) || !workspace) return -1;
    if (lights)
        for (size_t i = 0; i < (size_t)n * 4; ++i)
            if (!finite_f64(lights[i])) return -1;
    if (!rgba) return -6;
    if (workspace_bytes < giga_color_render_workspace_bytes(B, n, vertex_offsets[B], triangle_offsets[B])) return -4;
    const uint32_t bg = background ? (uint32_t)background[0] | (uint32_t)background[1] << 8 | (uint32_t)background[2] << 16 |
                                         (uint32_t)background[3] << 24 : 0xffffffffu;
    const RenderShade shade = {face_colors, lights, ambient, bg, rgba, triangle_index};
    return launch_render(vertices, vertex_offsets, triangles, triangle_offsets, view_offsets, extrinsics, intrinsics, B, W, H, near, far,
                         pixel_offset, depth, &shade, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

int giga_image_downsample(const uint32_t* src, uint32_t* dst, int n, int W, int H, int k, void* stream) {
    if (n < 0 || k < 1 || k > GIGA_DOWNSAMPLE_MAX_K || W < 1 || H < 1 || W > GIGA_RENDER_MAX_IMAGE || H > GIGA_RENDER_MAX_IMAGE) return -1;
    if ((long long)n * W * H * k * k >= (1LL << 31)) return -1;
    if (n == 0) return 0;
    if (!src) return -1;
    if (!dst) return -6;
    const int total = n * W * H;
    GIGA_LAUNCH(image_downsample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), src, dst,
                total, W, H, k);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // extern "C"
