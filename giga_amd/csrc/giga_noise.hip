// Depth-sensor noise on the device: the dex, trans and norm models of the reference's vgn.utils.misc.apply_noise
// (src/vgn/utils/misc.py:18-69), applied to [n][H][W] float32 depth images between giga_depth_render and giga_tsdf_integrate.
// The semantics and the draw layout are spelled out in include/giga_hip.h (giga_depth_noise); tests/noise_emu.py restates them.
//
//   draws   counter-based: one Philox-4x32-10 block per counter (block, image id low, image id high, stream), key = the seed.
//           A block gives two 53-bit uniforms and, through Box-Muller, two normals: element e of a stream is normal (e & 1) of
//           block e >> 1.  Nothing depends on the batch, the launch geometry or the order of calls.
//   shape   one launch, memory bound: a workgroup owns a NOISE_TILE_H x NOISE_TILE_W pixel tile of one image, a lane four
//           consecutive pixels of a row (16-byte loads and stores when W is a multiple of 4; trans gathers its sources with
//           scalar loads, an image stays in L2).  Lane 0 draws the image's scalars (dex: the gamma factor and the GP coin);
//           for dex the coarse normals the tile's bilinear taps can touch -- (tile_h h/H + 3) x (tile_w w/W + 3) of them -- are
//           generated once into LDS at the head of the tile.
// Every operation is one IEEE rounding (no contraction); log, cos, sin and pow are the only places a device and numpy may differ.
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "giga_check.h"
#include "giga_philox.h"
#include "giga_ws.h"
#include <cmath>
#include <cstdint>

#include "../../include/giga_hip.h"

#pragma clang fp contract(off)

namespace giga {

constexpr int NOISE_BLOCK = 256;
constexpr int NOISE_TILE_W = 128;             // 32 lanes x 4 pixels
constexpr int NOISE_TILE_H = 32;              // 8 rows per pass, 4 passes
constexpr int NOISE_ROWS = NOISE_BLOCK / (NOISE_TILE_W / 4);
constexpr unsigned NOISE_MAX_BLOCKS = 1u << 22;      // per launch (256 lanes each: below HIP's 2^32 lanes per grid)
enum { NOISE_STREAM_IMAGE = 0, NOISE_STREAM_GP = 1, NOISE_STREAM_ROW = 2, NOISE_STREAM_COL = 3, NOISE_STREAM_PIXEL = 4 };

struct NoiseArgs {
    const float* in;
    float* out;
    const unsigned long long* ids;            // device [n] (workspace), or null: the id of image i is i
    double p[5];                              // the model's parameters (include/giga_hip.h)
    double sy, sx;                            // dex: coarse / fine size, h / H and w / W
    int W, H, tiles_x, tiles;
    int ch, cw, nr, nc;                       // dex: coarse grid h x w; rows and columns of the LDS window
    int image0;                               // first image of this launch
    int vec;                                  // 16-byte accesses are aligned
    unsigned k0, k1;
};

// the normals of elements e0 .. e0 + 3: two blocks, three when e0 is odd
__device__ __forceinline__ void noise_normals4(unsigned e0, unsigned id_lo, unsigned id_hi, unsigned stream, unsigned k0, unsigned k1,
                                               double z[4]) {
    const unsigned b = e0 >> 1;
    const NoisePair q0 = noise_pair(b, id_lo, id_hi, stream, k0, k1), q1 = noise_pair(b + 1, id_lo, id_hi, stream, k0, k1);
    if (e0 & 1u) {
        const NoisePair q2 = noise_pair(b + 2, id_lo, id_hi, stream, k0, k1);
        z[0] = q0.z1; z[1] = q1.z0; z[2] = q1.z1; z[3] = q2.z0;
    } else {
        z[0] = q0.z0; z[1] = q0.z1; z[2] = q1.z0; z[3] = q1.z1;
    }
}

// Marsaglia-Tsang (2000) in double.  Attempt k reads the normal of block 1 + 2k and the uniform of block 2 + 2k of the image
// stream; after GIGA_NOISE_GAMMA_ATTEMPTS rejections the result is the sampler's value at x = 0, (a - 1/3) scale.  shape < 1
// draws shape + 1 and multiplies by u^(1 / shape), u the second uniform of block 0.
__device__ double noise_gamma(double shape, double scale, double u_boost, unsigned id_lo, unsigned id_hi, unsigned k0, unsigned k1) {
    const double a = shape < 1.0 ? shape + 1.0 : shape;
    const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double g = d;
    for (int k = 0; k < GIGA_NOISE_GAMMA_ATTEMPTS; ++k) {
        const double x = noise_pair(1u + 2u * k, id_lo, id_hi, NOISE_STREAM_IMAGE, k0, k1).z0;
        const Philox r = philox4x32_10(2u + 2u * k, id_lo, id_hi, NOISE_STREAM_IMAGE, k0, k1);
        const double u = noise_u53(r.x[0], r.x[1]);
        double v = 1.0 + c * x;
        if (!(v > 0.0)) continue;
        v = (v * v) * v;
        const double x2 = x * x;
        if (u < 1.0 - 0.0331 * (x2 * x2) || log(u) < 0.5 * x2 + d * ((1.0 - v) + log(v))) {
            g = d * v;
            break;
        }
    }
    if (shape < 1.0) g = g * pow(u_boost, 1.0 / shape);
    return g * scale;
}

template <int MODEL>
__global__ __launch_bounds__(NOISE_BLOCK) void depth_noise_kernel(NoiseArgs a) {
    extern __shared__ double s_gp[];          // dex: the coarse normals (times gp_sigma) under this tile, nr x nc
    __shared__ float s_gamma;
    __shared__ int s_on;
    const unsigned image = (unsigned)a.image0 + blockIdx.x / (unsigned)a.tiles, tile = blockIdx.x % (unsigned)a.tiles;
    const int r0 = (int)(tile / (unsigned)a.tiles_x) * NOISE_TILE_H, c0 = (int)(tile % (unsigned)a.tiles_x) * NOISE_TILE_W;
    const unsigned long long id = a.ids ? a.ids[image] : (unsigned long long)image;
    const unsigned id_lo = (unsigned)id, id_hi = (unsigned)(id >> 32);
    const size_t base = (size_t)image * a.H * a.W;
    const float* __restrict__ in = a.in + base;
    float* __restrict__ out = a.out + base;

    float gamma = 1.f;
    bool on = false;
    int y_lo = 0, x_lo = 0;
    if (MODEL == 1) {
        if (threadIdx.x == 0) {
            const Philox r = philox4x32_10(0u, id_lo, id_hi, NOISE_STREAM_IMAGE, a.k0, a.k1);
            s_on = noise_u53(r.x[0], r.x[1]) < a.p[4];
            s_gamma = (float)noise_gamma(a.p[0], a.p[1], noise_u53(r.x[2], r.x[3]), id_lo, id_hi, a.k0, a.k1);
        }
        __syncthreads();
        gamma = s_gamma;
        on = s_on != 0;
        if (on) {                             // (uniform over the workgroup)
            y_lo = (int)floor(((double)r0 + 0.5) * a.sy - 0.5);
            x_lo = (int)floor(((double)c0 + 0.5) * a.sx - 0.5);
            for (int i = threadIdx.x; i < a.nr * a.nc; i += NOISE_BLOCK) {
                const int y = y_lo + i / a.nc, x = x_lo + i % a.nc;
                double v = 0.0;               // a tap outside the coarse grid reads 0
                if (y >= 0 && y < a.ch && x >= 0 && x < a.cw)
                    v = noise_normal((unsigned)(y * a.cw + x), id_lo, id_hi, NOISE_STREAM_GP, a.k0, a.k1) * a.p[2];
                s_gp[i] = v;
            }
            __syncthreads();
        }
    }

    const int lx = threadIdx.x % (NOISE_TILE_W / 4), ly = threadIdx.x / (NOISE_TILE_W / 4);
    const int c = c0 + 4 * lx;
    if (c >= a.W) return;
    const int m = a.W - c < 4 ? a.W - c : 4;
    for (int r = r0 + ly; r < r0 + NOISE_TILE_H && r < a.H; r += NOISE_ROWS) {
        const size_t at = (size_t)r * a.W + c;
        const unsigned e0 = (unsigned)at;     // n W H < 2^31
        const bool wide = a.vec && m == 4;
        float x[4] = {0.f, 0.f, 0.f, 0.f}, y[4];
        if (MODEL != 2) {
            if (wide) {
                const float4 q = *reinterpret_cast<const float4*>(in + at);
                x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
            } else {
                for (int j = 0; j < m; ++j) x[j] = in[at + j];
            }
        }
        if (MODEL == 1) {
            double wy = 0.0;
            int iy = 0;
            if (on) {
                const double sy = ((double)r + 0.5) * a.sy - 0.5, fy = floor(sy);
                wy = sy - fy;
                iy = (int)fy - y_lo;
                iy = iy < 0 ? 0 : (iy < a.nr - 2 ? iy : a.nr - 2);      // (never taken: the window covers the tile's taps)
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float scaled = x[j] * gamma;
                if (on) {
                    const double sx = ((double)(c + j) + 0.5) * a.sx - 0.5, fx = floor(sx), wx = sx - fx;
                    int ix = (int)fx - x_lo;
                    ix = ix < 0 ? 0 : (ix < a.nc - 2 ? ix : a.nc - 2);
                    const double* g = s_gp + iy * a.nc + ix;
                    const double top = (1.0 - wx) * g[0] + wx * g[1], bot = (1.0 - wx) * g[a.nc] + wx * g[a.nc + 1];
                    y[j] = (float)((double)scaled + ((1.0 - wy) * top + wy * bot));
                } else {
                    y[j] = scaled;
                }
            }
        } else if (MODEL == 2) {
            double zr[4], zc[4], zd[4];
            noise_normals4(e0, id_lo, id_hi, NOISE_STREAM_ROW, a.k0, a.k1, zr);
            noise_normals4(e0, id_lo, id_hi, NOISE_STREAM_COL, a.k0, a.k1, zc);
            noise_normals4(e0, id_lo, id_hi, NOISE_STREAM_PIXEL, a.k0, a.k1, zd);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double rr = rint((double)r + zr[j] * a.p[0]), cc = rint((double)(c + j) + zc[j] * a.p[0]);     // half to even
                rr = fmin(fmax(rr, 0.0), (double)(a.H - 1));
                cc = fmin(fmax(cc, 0.0), (double)(a.W - 1));
                const float src = j < m ? in[(size_t)(int)rr * a.W + (int)cc] : 0.f;
                y[j] = (float)((double)src + zd[j] * a.p[1]);
            }
        } else {
            double z[4];
            noise_normals4(e0, id_lo, id_hi, NOISE_STREAM_PIXEL, a.k0, a.k1, z);
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = (float)((double)x[j] + z[j] * a.p[0]);
        }
        if (wide) {
            *reinterpret_cast<float4*>(out + at) = make_float4(y[0], y[1], y[2], y[3]);
        } else {
            for (int j = 0; j < m; ++j) out[at + j] = y[j];
        }
    }
}

static size_t depth_noise_workspace_bytes(int n) { return ws_align((size_t)(n > 0 ? n : 1) * sizeof(unsigned long long)); }

static int launch_depth_noise(const float* in, float* out, int n, int W, int H, int model, const double* p, unsigned long long seed,
                              const unsigned long long* image_ids, uint8_t* ws, hipStream_t s) {
    NoiseArgs a{};
    a.in = in; a.out = out;
    a.ids = nullptr;
    if (image_ids) {
        // (pageable host memory: the copy has left the caller's array when the call returns)
        if (hipMemcpyAsync(ws, image_ids, (size_t)n * sizeof(unsigned long long), hipMemcpyHostToDevice, s) != hipSuccess) return -10;
        a.ids = reinterpret_cast<const unsigned long long*>(ws);
    }
    for (int i = 0; i < 5; ++i) a.p[i] = p[i];
    a.W = W; a.H = H;
    a.tiles_x = (W + NOISE_TILE_W - 1) / NOISE_TILE_W;
    a.tiles = a.tiles_x * ((H + NOISE_TILE_H - 1) / NOISE_TILE_H);
    a.k0 = (unsigned)seed; a.k1 = (unsigned)(seed >> 32);
    a.vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    size_t lds = 0;
    if (model == 1) {
        a.ch = (int)((double)H / p[3]); a.cw = (int)((double)W / p[3]);          // int(h / gp_scale), as the reference
        a.sy = (double)a.ch / (double)H; a.sx = (double)a.cw / (double)W;
        a.nr = (int)floor(NOISE_TILE_H * a.sy) + 3; a.nc = (int)floor(NOISE_TILE_W * a.sx) + 3;
        lds = (size_t)a.nr * a.nc * sizeof(double);                              // gp_scale >= 1: at most 35 x 131 doubles
    }
    const int per = (int)(NOISE_MAX_BLOCKS / (unsigned)a.tiles) > 0 ? (int)(NOISE_MAX_BLOCKS / (unsigned)a.tiles) : 1;
    for (int first = 0; first < n; first += per) {
        a.image0 = first;
        const unsigned blocks = (unsigned)(n - first < per ? n - first : per) * (unsigned)a.tiles;
        if (model == 1) GIGA_LAUNCH(depth_noise_kernel<1>, dim3(blocks), dim3(NOISE_BLOCK), lds, s, a);
        else if (model == 2) GIGA_LAUNCH(depth_noise_kernel<2>, dim3(blocks), dim3(NOISE_BLOCK), 0, s, a);
        else GIGA_LAUNCH(depth_noise_kernel<3>, dim3(blocks), dim3(NOISE_BLOCK), 0, s, a);
        if (hipGetLastError() != hipSuccess) return -10;
    }
    return 0;
}

}  // namespace giga

using namespace giga;

extern "C" {

static bool noise_positive(double x) { return finite_f64(x) && x > 0.0; }

static bool noise_shape_ok(int n, int W, int H, int model) {
    if (n < 0 || W < 1 || H < 1 || W > GIGA_TSDF_MAX_IMAGE || H > GIGA_TSDF_MAX_IMAGE) return false;
    if ((long long)n * W * H >= (1LL << 31)) return false;
    return model >= GIGA_NOISE_DEX && model <= GIGA_NOISE_NORM;
}

size_t giga_depth_noise_workspace_bytes(int n_images, int width, int height, int model) {
    if (!noise_shape_ok(n_images, width, height, model) || n_images == 0) return 0;
    return depth_noise_workspace_bytes(n_images);
}

int giga_depth_noise(const float* depth_in, float* depth_out, int n_images, int width, int height, int model, const double* params,
                     unsigned long long seed, const unsigned long long* image_ids, void* workspace, size_t workspace_bytes,
                     void* stream) {
    if (!noise_shape_ok(n_images, width, height, model)) return -1;
    static const double defaults[3][5] = {{1000.0, 0.001, 0.005, 4.0, 0.5}, {1.0, 0.005, 0, 0, 0}, {0.005, 0, 0, 0, 0}};
    static const int count[3] = {5, 2, 1};
    double p[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < count[model - 1]; ++i) p[i] = params ? params[i] : defaults[model - 1][i];
    if (model == GIGA_NOISE_DEX) {
        if (!noise_positive(p[0]) || !noise_positive(p[1]) || !noise_positive(p[2]) || !noise_positive(p[3])) return -1;
        if (!(p[4] >= 0.0 && p[4] <= 1.0)) return -1;
        if (p[3] < 1.0 || (double)height < p[3] || (double)width < p[3]) return -1;
    } else {
        for (int i = 0; i < count[model - 1]; ++i)
            if (!noise_positive(p[i])) return -1;
    }
    if (n_images == 0) return 0;
    if (!depth_in || !depth_out || !workspace) return -1;
    const size_t bytes = (size_t)n_images * width * height * sizeof(float);
    const uintptr_t a = reinterpret_cast<uintptr_t>(depth_in), b = reinterpret_cast<uintptr_t>(depth_out);
    if (a < b + bytes && b < a + bytes) return -1;                               // out of place: trans is a gather
    if (workspace_bytes < giga_depth_noise_workspace_bytes(n_images, width, height, model)) return -4;
    return launch_depth_noise(depth_in, depth_out, n_images, width, height, model, p, seed, image_ids,
                              static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

}  // extern "C"
