// Mesh refinement on the device: the reference's Generator3D.refine_mesh (conv_onet/generation.py:457-519) without an autograd
// graph.  A step is four launches: giga_refine_face_points, giga_decoder_point_hess (giga_decoder_pgrad.hip: logit f, grad f and
// the three off-diagonal Hessian entries at the face points), giga_refine_face_grad and giga_refine_vertex_step.  The semantics
// are spelled out in include/giga_hip.h; tests/refine_emu.py restates the formulas, tests/refine_ref.py the reference's loss.
//
//   face points   one lane per face: barycentric weights given, or Dirichlet(1/2, 1/2, 1/2) as z_i^2 / sum z_j^2 from three
//                 counter-based standard normals (Gamma(1/2, 2) is the square of a normal: no rejection loop), Philox counter
//                 (block, face, step, 0), key = the seed; q = sum eps_i v_i.
//   face grad     one lane per face: with sigma = sigmoid(f), g = sigma' grad f, t = -g / (|g| + 1e-10), c = e1 x e2,
//                 n = c / (|c| + 1e-10) the loss is mean (sigma - tau)^2 + 0.01 mean |n - t|^2, and its gradient w.r.t. the three
//                 corners is closed-form 3 x 3 arithmetic (the Hessian enters through D t = d t / d q).  Per-face arithmetic
//                 runs in double: the kernel is a few hundred flops per 100 bytes and the 1e-10 guards sit next to |g| ~ 1e-3.
//   vertex step   one lane per vertex: the incident corner gradients summed in the order of a CSR list (no float atomics: bit
//                 reproducible), then torch's RMSprop defaults in place.
// An index outside its array is never followed: a face with a corner outside [0, V) gets NaN outputs, a corner entry outside
// [0, 3F) is skipped.
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "giga_philox.h"
#include <cmath>
#include <cstdint>

#include "../../include/giga_hip.h"

namespace giga {

constexpr int REFINE_BLOCK = 256;
constexpr unsigned REFINE_STREAM = 0;         // Philox stream of the barycentric draws
constexpr double REFINE_EPS = 1e-10;          // the reference's guard in both normalisations
constexpr double REFINE_NORMAL_WEIGHT = 0.01; // loss = loss_target + 0.01 loss_normal
constexpr double REFINE_LR = 1e-4, REFINE_ALPHA = 0.99, REFINE_RMS_EPS = 1e-8;      // optim.RMSprop([v], lr=1e-4) defaults

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 operator*(double s, D3 a) { return D3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ D3 load3(const float* p, int i) { return D3{(double)p[3 * (size_t)i], (double)p[3 * (size_t)i + 1], (double)p[3 * (size_t)i + 2]}; }
__device__ __forceinline__ void store3(float* p, size_t i, D3 a) { p[3 * i] = (float)a.x; p[3 * i + 1] = (float)a.y; p[3 * i + 2] = (float)a.z; }

// J(a) y for J = d (a / (|a| + eps)) / d a = I / (|a| + eps) - a a^T / (|a| (|a| + eps)^2), symmetric; the second term is 0 at
// a = 0 (torch's subgradient of norm at the origin)
__device__ __forceinline__ D3 normalize_jvp(D3 a, double na, D3 y) {
    const double d = na + REFINE_EPS;
    const double k = na > 0.0 ? dot(a, y) / (na * d * d) : 0.0;
    return (1.0 / d) * y - k * a;
}

__global__ __launch_bounds__(REFINE_BLOCK) void refine_face_points_kernel(const float* __restrict__ vertices, const int* __restrict__ faces,
                                                                          const float* __restrict__ eps_in, float* __restrict__ eps,
                                                                          float* __restrict__ points, int V, int F, unsigned k0,
                                                                          unsigned k1, unsigned step) {
    const int f = blockIdx.x * REFINE_BLOCK + threadIdx.x;
    if (f >= F) return;
    float e0, e1, e2;
    if (eps_in) {
        e0 = eps_in[3 * (size_t)f]; e1 = eps_in[3 * (size_t)f + 1]; e2 = eps_in[3 * (size_t)f + 2];
    } else {
        const NoisePair a = noise_pair(0u, (unsigned)f, step, REFINE_STREAM, k0, k1);
        const double z2 = noise_pair(1u, (unsigned)f, step, REFINE_STREAM, k0, k1).z0;
        const double g0 = a.z0 * a.z0, g1 = a.z1 * a.z1, g2 = z2 * z2, sum = g0 + g1 + g2;
        const double inv = sum > 0.0 ? 1.0 / sum : 0.0;
        e0 = sum > 0.0 ? (float)(g0 * inv) : 1.0f / 3.0f;
        e1 = sum > 0.0 ? (float)(g1 * inv) : 1.0f / 3.0f;
        e2 = sum > 0.0 ? (float)(g2 * inv) : 1.0f / 3.0f;
    }
    eps[3 * (size_t)f] = e0; eps[3 * (size_t)f + 1] = e1; eps[3 * (size_t)f + 2] = e2;
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) {
        const float nan = __builtin_nanf("");
        points[3 * (size_t)f] = nan; points[3 * (size_t)f + 1] = nan; points[3 * (size_t)f + 2] = nan;
        return;
    }
    // (face_vertex * eps[:, :, None]).sum(dim=1) in fp32, as the reference forms the decoder's input
    const float* v0 = vertices + 3 * (size_t)i0; const float* v1 = vertices + 3 * (size_t)i1; const float* v2 = vertices + 3 * (size_t)i2;
#pragma unroll
    for (int j = 0; j < 3; ++j) points[3 * (size_t)f + j] = (v0[j] * e0 + v1[j] * e1) + v2[j] * e2;
}

__global__ __launch_bounds__(REFINE_BLOCK) void refine_face_grad_kernel(const float* __restrict__ vertices, const int* __restrict__ faces,
                                                                        const float* __restrict__ eps, const float* __restrict__ logit,
                                                                        const float* __restrict__ dp, const float* __restrict__ hess,
                                                                        double tau, float* __restrict__ floss, float* __restrict__ fgrad,
                                                                        int V, int F) {
    const int f = blockIdx.x * REFINE_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) {
        const float nan = __builtin_nanf("");
        floss[2 * (size_t)f] = nan; floss[2 * (size_t)f + 1] = nan;
        for (int j = 0; j < 9; ++j) fgrad[9 * (size_t)f + j] = nan;
        return;
    }
    const double invF = 1.0 / (double)F;
    const D3 v0 = load3(vertices, i0), v1 = load3(vertices, i1), v2 = load3(vertices, i2);
    const D3 df = load3(dp, f);
    const double hxy = hess[3 * (size_t)f], hxz = hess[3 * (size_t)f + 1], hyz = hess[3 * (size_t)f + 2];
    const double z = logit[f];
    // both tails of the sigmoid: sigma' = sigma (1 - sigma) and 1 - 2 sigma without cancellation
    const double sp = 1.0 / (1.0 + exp(-z)), sm = 1.0 / (1.0 + exp(z));
    const double s1 = sp * sm, s2 = s1 * (sm - sp);
    const D3 g = s1 * df;
    const double ng = sqrt(dot(g, g));
    const D3 t = (-1.0 / (ng + REFINE_EPS)) * g;
    const D3 e1 = v1 - v0, e2 = v2 - v1, c = cross(e1, e2);
    const double nc = sqrt(dot(c, c));
    const D3 n = (1.0 / (nc + REFINE_EPS)) * c;
    const D3 r = n - t;                                            // n - t
    floss[2 * (size_t)f] = (float)((sp - tau) * (sp - tau));
    floss[2 * (size_t)f + 1] = (float)dot(r, r);
    // dL/dq = (2/F)(sigma - tau) sigma' grad f + M Jt y,  y = (0.02/F)(n - t),  M = d g / d q = sigma'' grad f grad f^T + sigma' H:
    // dL/dt = -y and D t = -Jt M, both factors symmetric
    const double wn = 2.0 * REFINE_NORMAL_WEIGHT * invF;
    const D3 y = wn * r;
    const D3 u = normalize_jvp(g, ng, y);
    const D3 Hu = D3{hxy * u.y + hxz * u.z, hxy * u.x + hyz * u.z, hxz * u.x + hyz * u.y};
    const D3 dq = (2.0 * invF * (sp - tau) * s1 + s2 * dot(df, u)) * df + s1 * Hu;
    const D3 w = normalize_jvp(c, nc, y);
    const D3 de1 = cross(e2, w), de2 = cross(w, e1);
    const double b0 = eps[3 * (size_t)f], b1 = eps[3 * (size_t)f + 1], b2 = eps[3 * (size_t)f + 2];
    store3(fgrad, 3 * (size_t)f + 0, b0 * dq - de1);
    store3(fgrad, 3 * (size_t)f + 1, b1 * dq + de1 - de2);
    store3(fgrad, 3 * (size_t)f + 2, b2 * dq + de2);
}

__global__ __launch_bounds__(REFINE_BLOCK) void refine_vertex_step_kernel(const float* __restrict__ fgrad, const int* __restrict__ corner_order,
                                                                          const int* __restrict__ vertex_offsets, float* __restrict__ vertices,
                                                                          float* __restrict__ square_avg, float* __restrict__ grad, int V,
                                                                          int F) {
    const int v = blockIdx.x * REFINE_BLOCK + threadIdx.x;
    if (v >= V) return;
    const long long C = 3LL * F;
    long long k0 = vertex_offsets[v], k1 = vertex_offsets[v + 1];
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > C ? C : k1;
    D3 g = D3{0.0, 0.0, 0.0};
    for (long long k = k0; k < k1; ++k) {
        const int corner = corner_order[k];
        if ((unsigned)corner >= (unsigned long long)C) continue;
        g = g + load3(fgrad, corner);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float gj = (float)(j == 0 ? g.x : j == 1 ? g.y : g.z);
        const size_t at = 3 * (size_t)v + j;
        grad[at] = gj;
        // square_avg.mul_(alpha).addcmul_(g, g, value=1 - alpha); v.addcdiv_(g, square_avg.sqrt().add_(eps), value=-lr)
        const float sq = (float)(REFINE_ALPHA * (double)square_avg[at] + (1.0 - REFINE_ALPHA) * ((double)gj * (double)gj));
        square_avg[at] = sq;
        // (g = 0 moves nothing: an unreferenced vertex stays where it is)
        vertices[at] = (float)((double)vertices[at] - REFINE_LR * ((double)gj / (sqrt((double)sq) + REFINE_RMS_EPS)));
    }
}

}  // namespace giga

using namespace giga;

extern "C" {

// 3 F corner indices and 9 F gradient floats are indexed with int / 32-bit products of the face count
static bool refine_sizes_ok(int n_vertices, int n_faces) {
    return n_vertices >= 0 && n_faces >= 0 && n_vertices <= GIGA_REFINE_MAX_VERTICES && n_faces <= GIGA_REFINE_MAX_FACES;
}

static unsigned refine_blocks(int n) { return (unsigned)((n + REFINE_BLOCK - 1) / REFINE_BLOCK); }

int giga_refine_face_points(const float* vertices, const int* faces, const float* eps_in, float* eps, float* points,
                            int n_vertices, int n_faces, unsigned long long seed, int step, void* stream) {
    if (!refine_sizes_ok(n_vertices, n_faces) || step < 0) return -1;
    if (n_faces == 0) return 0;
    if (!vertices || !faces) return -1;
    if (!eps || !points) return -6;
    GIGA_LAUNCH(refine_face_points_kernel, dim3(refine_blocks(n_faces)), dim3(REFINE_BLOCK), 0, static_cast<hipStream_t>(stream),
                vertices, faces, eps_in, eps, points, n_vertices, n_faces, (unsigned)seed, (unsigned)(seed >> 32), (unsigned)step);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int giga_refine_face_grad(const float* vertices, const int* faces, const float* eps, const float* logit, const float* dp,
                          const float* hess, double threshold, float* face_loss, float* face_grad, int n_vertices, int n_faces,
                          void* stream) {
    if (!refine_sizes_ok(n_vertices, n_faces) || !(threshold > 0.0 && threshold < 1.0)) return -1;
    if (n_faces == 0) return 0;
    if (!vertices || !faces || !eps || !logit || !dp || !hess) return -1;
    if (!face_loss || !face_grad) return -6;
    GIGA_LAUNCH(refine_face_grad_kernel, dim3(refine_blocks(n_faces)), dim3(REFINE_BLOCK), 0, static_cast<hipStream_t>(stream),
                vertices, faces, eps, logit, dp, hess, threshold, face_loss, face_grad, n_vertices, n_faces);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int giga_refine_vertex_step(const float* face_grad, const int* corner_order, const int* vertex_offsets, float* vertices,
                            float* square_avg, float* grad, int n_vertices, int n_faces, void* stream) {
    if (!refine_sizes_ok(n_vertices, n_faces)) return -1;
    if (n_vertices == 0) return 0;
    if (!vertex_offsets || !vertices || !square_avg || (n_faces > 0 && (!face_grad || !corner_order))) return -1;
    if (!grad) return -6;
    GIGA_LAUNCH(refine_vertex_step_kernel, dim3(refine_blocks(n_vertices)), dim3(REFINE_BLOCK), 0, static_cast<hipStream_t>(stream),
                face_grad, corner_order, vertex_offsets, vertices, square_avg, grad, n_vertices, n_faces);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // extern "C"
