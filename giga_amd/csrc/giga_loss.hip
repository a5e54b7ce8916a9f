// Fused training loss of the joint GIGA objective and its gradient with respect to the four head outputs.
//
// Replaces the caller-side torch code of the reference's training step for the literal call shape (one grasp query per
// scene): `select` (scripts/train_giga.py:154-158: squeeze + sigmoid(occ)) followed by `loss_fn` (train_giga.py:161-195):
//   loss_qual  = BCE(qual, label)                                  (:177-178; F.binary_cross_entropy clamps log at -100)
//   loss_rot   = min_k (1 - |<rot, rotations[:, k]>|), k = 0, 1    (:181-188)
//   loss_width = (40 width - 40 width_t)^2                         (:191-192, F.mse_loss(40 w, 40 w_t, 'none'))
//   loss_occ   = mean_M BCE(sigmoid(occ_logit), occ_t)             (:194-195)
//   loss       = mean_B (loss_qual + label * (loss_rot + 0.01 loss_width) + loss_occ)
// As ~20 tiny ATen kernels forward and as many backward that is a visible part of a 3 ms training step; here it is
// three launches: per-scene losses (one workgroup per scene, block reduction over the M occupancy queries), a fixed-order
// mean over the scenes (deterministic), and the gradient kernel.  HBM-bound elementwise work: 8 B read + 4 B written
// per occupancy query.  The arithmetic follows ATen's fp32 formulas (sigmoid as 1/(1+exp(-z)), logs clamped at -100,
// the BCE gradient (p - y) / max(p (1 - p), 1e-12)) so that losses and gradients agree with autograd through the
// reference's helpers to fp32 rounding (tests/test_gpu_training.py, golden G11).
#include <hip/hip_runtime.h>
#include "giga_launch.h"
#include "../../include/giga_hip.h"
#include <cmath>

namespace giga {

__device__ __forceinline__ float bce_term(float p, float y) {
    const float lp = fmaxf(logf(p), -100.0f), lq = fmaxf(logf(1.0f - p), -100.0f);
    return -(y * lp + (1.0f - y) * lq);
}
__device__ __forceinline__ float bce_grad(float p, float y) {        // d BCE / d p   (ATen binary_cross_entropy_backward)
    return (p - y) / fmaxf((1.0f - p) * p, 1e-12f);
}

// scene_loss [B][5]: qual, rot, width, occ, all
__global__ __launch_bounds__(256) void loss_scene_kernel(const float* __restrict__ qual, const float* __restrict__ rot,
                                                         const float* __restrict__ width, const float* __restrict__ occ,
                                                         const float* __restrict__ label, const float* __restrict__ rot_t,
                                                         const float* __restrict__ width_t, const float* __restrict__ occ_t,
                                                         int M, float* __restrict__ scene_loss) {
    __shared__ float part[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    float s = 0.f;
    for (int i = tid; i < M; i += 256) {
        const float z = occ[(size_t)b * M + i];
        const float p = 1.0f / (1.0f + expf(-z));
        s += bce_term(p, occ_t[(size_t)b * M + i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const float locc = M > 0 ? ((part[0] + part[1]) + (part[2] + part[3])) / (float)M : 0.f;
        const float y = label[b];
        const float lq = bce_term(qual[b], y);
        float lr = 0.f;
        {
            const float* r = rot + 4 * b;
            const float* t0 = rot_t + 8 * b;
            const float d0 = r[0] * t0[0] + r[1] * t0[1] + r[2] * t0[2] + r[3] * t0[3];
            const float d1 = r[0] * t0[4] + r[1] * t0[5] + r[2] * t0[6] + r[3] * t0[7];
            lr = fminf(1.0f - fabsf(d0), 1.0f - fabsf(d1));
        }
        const float dw = 40.0f * width[b] - 40.0f * width_t[b];
        const float lw = dw * dw;
        float* o = scene_loss + 5 * b;
        o[0] = lq; o[1] = lr; o[2] = lw; o[3] = locc;
        o[4] = lq + y * (lr + 0.01f * lw) + locc;
    }
}

// losses [5] = mean over the scenes, summed in scene order by one wave (fixed order: run-to-run identical)
__global__ __launch_bounds__(64) void loss_mean_kernel(const float* __restrict__ scene_loss, int B, float* __restrict__ losses) {
    const int k = threadIdx.x;
    if (k >= 5) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += scene_loss[5 * b + k];
    losses[k] = s / (float)B;
}

// The mean launch of a training loop (giga_train_loss_metrics): the same five means, and the epoch accumulator of
// include/giga_hip.h updated from this batch -- uint64 words 0-6 (batches, examples, correct, tp, fp, fn, invalid), double
// words 8-12 (running sums of the batch means); words 7 and 13-15 are not touched.  One workgroup of four waves.  Lanes 0-4 of
// wave 0 compute the means exactly as loss_mean_kernel does (same loop, same fp32 sum); that serial loop is the launch's critical
// path, so wave 0 does nothing else beside it: lane 0 loads the twelve accumulator words first (their latency passes under the
// loop), and waves 1-3 classify the scenes meanwhile, b = lane, lane + 192, ... (a uniform trip count, so each ballot sees whole
// waves): prediction qual > 0.5f (torch.round of a sigmoid output, half to even), valid when 0 <= qual <= 1 and label is exactly
// 0 or 1.  Counts are popcounts of ballots per wave, summed over the three waves through LDS in wave order by lane 0, which alone
// reads, updates and writes `acc`.  Integer counts and one double addition per sum: no atomics and nothing whose order could
// vary, so the accumulator is a pure function of the calls.
__global__ __launch_bounds__(256) void loss_mean_metrics_kernel(const float* __restrict__ scene_loss, const float* __restrict__ qual,
                                                                const float* __restrict__ label, int B, float* losses,
                                                                unsigned long long* acc) {
    __shared__ unsigned cnt[3][6];                              // per counting wave: examples, correct, tp, fp, fn, invalid
    __shared__ float mean[5];
    const int tid = threadIdx.x;
    // thread 0's view of `acc`: + 0 as a per-lane value (every lane is active here), so that its accesses are vector loads and
    // stores, not reads through the scalar cache; no other thread uses it
    unsigned long long* const words = acc + __builtin_amdgcn_mbcnt_lo(~0u, 0u);
    unsigned long long old[7];
    double old_sum[5];
    if (tid == 0) {
        for (int k = 0; k < 7; ++k) old[k] = words[k];
        for (int k = 0; k < 5; ++k) old_sum[k] = reinterpret_cast<const double*>(words)[8 + k];
    }
    if (tid < 64) {
        if (tid < 5) {
            float s = 0.f;
            for (int b = 0; b < B; ++b) s += scene_loss[5 * b + tid];
            const float m = s / (float)B;
            losses[tid] = m;
            mean[tid] = m;
        }
    } else {
        const int lane = tid - 64;
        unsigned c[6] = {0, 0, 0, 0, 0, 0};
        for (long long base = 0; base < B; base += 192) {       // (64-bit: base + 192 passes INT_MAX for the largest B)
            const long long b = base + lane;
            const bool in = b < B;
            const float q = in ? qual[b] : 0.f, y = in ? label[b] : 0.f;
            const bool valid = in && q >= 0.f && q <= 1.f && (y == 0.f || y == 1.f);
            const bool pred = q > 0.5f, pos = y == 1.f;
            c[0] += __popcll(__ballot(valid));
            c[1] += __popcll(__ballot(valid && pred == pos));
            c[2] += __popcll(__ballot(valid && pred && pos));
            c[3] += __popcll(__ballot(valid && pred && !pos));
            c[4] += __popcll(__ballot(valid && !pred && pos));
            c[5] += __popcll(__ballot(in && !valid));
        }
        if ((lane & 63) == 0)
            for (int k = 0; k < 6; ++k) cnt[lane >> 6][k] = c[k];
    }
    __syncthreads();
    if (tid == 0) {
        words[0] = old[0] + 1ull;
        for (int k = 0; k < 6; ++k) words[1 + k] = old[1 + k] + ((unsigned long long)cnt[0][k] + cnt[1][k] + cnt[2][k]);
        for (int k = 0; k < 5; ++k) reinterpret_cast<double*>(words)[8 + k] = old_sum[k] + (double)mean[k];
    }
}

// gradients of `loss` (times the upstream scalar *gout) with respect to the head outputs
__global__ __launch_bounds__(256) void loss_grad_kernel(const float* __restrict__ qual, const float* __restrict__ rot,
                                                        const float* __restrict__ width, const float* __restrict__ occ,
                                                        const float* __restrict__ label, const float* __restrict__ rot_t,
                                                        const float* __restrict__ width_t, const float* __restrict__ occ_t,
                                                        const float* __restrict__ gout, int B, int M,
                                                        float* __restrict__ dqual, float* __restrict__ drot,
                                                        float* __restrict__ dwidth, float* __restrict__ docc) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float g = gout[0] / (float)B;
    const float gm = M > 0 ? g / (float)M : 0.f;
    for (int i = tid; i < M; i += 256) {
        const float z = occ[(size_t)b * M + i];
        const float p = 1.0f / (1.0f + expf(-z));
        // autograd's chain: BCE'(p) * sigmoid'(z) = (p - y) / max(p(1-p), 1e-12) * p(1-p)
        docc[(size_t)b * M + i] = gm * bce_grad(p, occ_t[(size_t)b * M + i]) * ((1.0f - p) * p);
    }
    if (tid == 0) {
        const float y = label[b];
        dqual[b] = g * bce_grad(qual[b], y);
        const float* r = rot + 4 * b;
        const float* t0 = rot_t + 8 * b;
        const float d0 = r[0] * t0[0] + r[1] * t0[1] + r[2] * t0[2] + r[3] * t0[3];
        const float d1 = r[0] * t0[4] + r[1] * t0[5] + r[2] * t0[6] + r[3] * t0[7];
        const float l0 = 1.0f - fabsf(d0), l1 = 1.0f - fabsf(d1);
        // torch.min(a, b): the gradient goes to the smaller argument (split evenly on an exact tie)
        const float w0 = l0 < l1 ? 1.0f : (l0 == l1 ? 0.5f : 0.0f), w1 = 1.0f - w0;
        const float s0 = d0 > 0.f ? 1.0f : (d0 < 0.f ? -1.0f : 0.0f), s1 = d1 > 0.f ? 1.0f : (d1 < 0.f ? -1.0f : 0.0f);
#pragma unroll
        for (int k = 0; k < 4; ++k) drot[4 * b + k] = -g * y * (w0 * s0 * t0[k] + w1 * s1 * t0[4 + k]);
        dwidth[b] = g * y * 0.01f * 2.0f * (40.0f * width[b] - 40.0f * width_t[b]) * 40.0f;
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// The occupancy-only objective of giga_geo (scripts/train_giga_geo.py:152-165: loss = mean_B mean_M BCE(sigmoid(z), t)) and its
// epoch metrics (:52-57: ignite's binary Accuracy / Precision / Recall over EVERY occupancy point of the epoch).  The arithmetic
// is the occupancy term's of the kernels above, restated: the same p, the same bce_term, the same per-thread order (i = tid,
// tid + 256, ...), the same wave and LDS tree, the same serial sum over the scenes -- `loss` equals losses[3] of giga_train_loss
// and `docc` equals its docc, bit for bit (tests/test_gpu_geo_trainer.py).  HBM-bound: one read of each input per launch.
//
// One workgroup per scene.  The loop's trip count is uniform (ceil(M / 256) rounds for every thread; a thread past M adds nothing),
// so each ballot sees whole waves; a point's prediction is p > 0.5f on the p the loss uses (torch.round(sigmoid(z)): half to even,
// p == 0.5 rounds to 0), and it is valid when p is not NaN and the target is exactly 0 or 1.  With `scene_counts` (the metrics
// form) thread 0 writes the scene's six counts -- examples, correct, tp, fp, fn, invalid -- as 32-bit words [b][6].
__global__ __launch_bounds__(256) void occ_scene_kernel(const float* __restrict__ occ, const float* __restrict__ occ_t, int M,
                                                        float* __restrict__ scene_loss, unsigned* __restrict__ scene_counts) {
    __shared__ float part[4];
    __shared__ unsigned cnt[4][6];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* z_row = occ + (size_t)b * M;
    const float* t_row = occ_t + (size_t)b * M;
    float s = 0.f;
    unsigned c[6] = {0, 0, 0, 0, 0, 0};
    for (long long base = 0; base < M; base += 256) {           // (64-bit: base + 256 passes INT_MAX for the largest M)
        const long long i = base + tid;
        const bool in = i < M;
        const float z = in ? z_row[i] : 0.f, t = in ? t_row[i] : 0.f;
        const float p = 1.0f / (1.0f + expf(-z));
        if (in) s += bce_term(p, t);
        const bool valid = in && p == p && (t == 0.f || t == 1.f);
        const bool pred = p > 0.5f, pos = t == 1.f;
        c[0] += __popcll(__ballot(valid));
        c[1] += __popcll(__ballot(valid && pred == pos));
        c[2] += __popcll(__ballot(valid && pred && pos));
        c[3] += __popcll(__ballot(valid && pred && !pos));
        c[4] += __popcll(__ballot(valid && !pred && pos));
        c[5] += __popcll(__ballot(in && !valid));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) {
        part[tid >> 6] = s;
        for (int k = 0; k < 6; ++k) cnt[tid >> 6][k] = c[k];
    }
    __syncthreads();
    if (tid == 0) {
        scene_loss[b] = ((part[0] + part[1]) + (part[2] + part[3])) / (float)M;
        if (scene_counts)
            for (int k = 0; k < 6; ++k) scene_counts[6 * (size_t)b + k] = (cnt[0][k] + cnt[1][k]) + (cnt[2][k] + cnt[3][k]);
    }
}

// loss [1] = mean over the scenes, summed in scene order by one lane
__global__ __launch_bounds__(64) void occ_mean_kernel(const float* __restrict__ scene_loss, int B, float* __restrict__ loss) {
    if (threadIdx.x != 0) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += scene_loss[b];
    loss[0] = s / (float)B;
}

// The mean launch of the giga_geo loop (giga_train_occ_loss_metrics), in the manner of loss_mean_metrics_kernel: lane 0 of wave 0
// loads the accumulator words it will update and then runs the serial fp32 sum exactly as occ_mean_kernel does; lanes 0-5 of wave 1
// meanwhile sum the per-scene counts over the scenes as 64-bit integers, one count each.  Lane 0 alone reads, updates and writes
// `acc`: words 0-6 (batches + 1; examples, correct, tp, fp, fn, invalid in points) and the doubles 8 + 3 and 8 + 4 (both
// += (double)loss: the occupancy mean is the whole objective here); words 7, 8-10 and 13-15 are not touched.  No atomics.
__global__ __launch_bounds__(128) void occ_mean_metrics_kernel(const float* __restrict__ scene_loss,
                                                               const unsigned* __restrict__ scene_counts, int B, float* loss,
                                                               unsigned long long* acc) {
    __shared__ unsigned long long total[6];
    const int tid = threadIdx.x;
    // thread 0's view of `acc`, + 0 as a per-lane value: vector loads and stores (see loss_mean_metrics_kernel)
    unsigned long long* const words = acc + __builtin_amdgcn_mbcnt_lo(~0u, 0u);
    unsigned long long old[7];
    double old_sum[2];
    float m = 0.f;
    if (tid == 0) {
        for (int k = 0; k < 7; ++k) old[k] = words[k];
        for (int k = 0; k < 2; ++k) old_sum[k] = reinterpret_cast<const double*>(words)[8 + 3 + k];
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += scene_loss[b];
        m = s / (float)B;
        loss[0] = m;
    } else if (tid >= 64 && tid < 64 + 6) {
        const int k = tid - 64;
        unsigned long long n = 0;
        for (int b = 0; b < B; ++b) n += scene_counts[6 * (size_t)b + k];
        total[k] = n;
    }
    __syncthreads();
    if (tid == 0) {
        words[0] = old[0] + 1ull;
        for (int k = 0; k < 6; ++k) words[1 + k] = old[1 + k] + total[k];
        for (int k = 0; k < 2; ++k) reinterpret_cast<double*>(words)[8 + 3 + k] = old_sum[k] + (double)m;
    }
}

// docc = (g / B / M) * BCE'(p) * sigmoid'(z), the occupancy line of loss_grad_kernel
__global__ __launch_bounds__(256) void occ_grad_kernel(const float* __restrict__ occ, const float* __restrict__ occ_t,
                                                       const float* __restrict__ gout, int B, int M, float* __restrict__ docc) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float g = gout[0] / (float)B;
    const float gm = g / (float)M;
    for (int i = tid; i < M; i += 256) {
        const float z = occ[(size_t)b * M + i];
        const float p = 1.0f / (1.0f + expf(-z));
        docc[(size_t)b * M + i] = gm * bce_grad(p, occ_t[(size_t)b * M + i]) * ((1.0f - p) * p);
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// Adam over ONE flat fp32 parameter buffer (the module's flattened parameters, 581 863 elements): torch.optim.Adam's update
// (scripts/train_giga.py:49 builds `torch.optim.Adam(net.parameters(), lr)`; no amsgrad, not maximize) in one launch that
// uses the whole chip.  torch's fused multi-tensor kernel gives one tensor one workgroup per 65 536 elements: nine workgroups
// for this buffer, 98 us per step (tools/gpu_train_kernels.py); this takes ~5 us.  Same formulas in the same order as
// torch/optim/adam.py (_single_tensor_adam): m = lerp(m, g, 1 - b1); v = b2 v + (1 - b2) g g;
// p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps); L2 weight decay adds wd * p to g first.
__global__ __launch_bounds__(256) void adam_flat_kernel(float4* __restrict__ p, const float4* __restrict__ g, float4* __restrict__ m,
                                                        float4* __restrict__ v, size_t n4, size_t n, float step_size, float b2,
                                                        float omb1, float omb2, float eps, float wd, float bc2_sqrt) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    auto upd = [&](float& pp, float gg, float& mm, float& vv) {
        if (wd != 0.f) gg = fmaf(wd, pp, gg);
        mm = mm + (gg - mm) * omb1;                            // exp_avg.lerp_(grad, 1 - beta1)
        vv = vv * b2 + omb2 * gg * gg;                         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        const float denom = sqrtf(vv) / bc2_sqrt + eps;
        pp = pp - step_size * (mm / denom);                    // param.addcdiv_(exp_avg, denom, value=-step_size)
    };
    if (i < n4) {
        float4 P = p[i], M = m[i], V = v[i];
        const float4 G = g[i];
        upd(P.x, G.x, M.x, V.x); upd(P.y, G.y, M.y, V.y); upd(P.z, G.z, M.z, V.z); upd(P.w, G.w, M.w, V.w);
        p[i] = P; m[i] = M; v[i] = V;
    } else if (i == n4) {                                      // the (n % 4) tail elements
        float* ps = reinterpret_cast<float*>(p); const float* gs = reinterpret_cast<const float*>(g);
        float* ms = reinterpret_cast<float*>(m); float* vs = reinterpret_cast<float*>(v);
        for (size_t k = 4 * n4; k < n; ++k) upd(ps[k], gs[k], ms[k], vs[k]);
    }
}

}  // namespace giga

using namespace giga;

extern "C" {

int giga_train_loss(const float* qual, const float* rot, const float* width, const float* occ_logits, const float* label,
                    const float* rot_targets, const float* width_target, const float* occ_target, int B, int M,
                    float* losses, float* scene_losses, void* stream) {
    if (B < 0 || M < 0) return -1;
    if (B == 0) return 0;
    if (!qual || !rot || !width || !label || !rot_targets || !width_target || !losses || !scene_losses) return -1;
    if (M > 0 && (!occ_logits || !occ_target)) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    GIGA_LAUNCH(loss_scene_kernel, dim3(B), dim3(256), 0, s, qual, rot, width, occ_logits, label, rot_targets, width_target, occ_target,
                M, scene_losses);
    GIGA_LAUNCH(loss_mean_kernel, dim3(1), dim3(64), 0, s, scene_losses, B, losses);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int giga_train_loss_metrics(const float* qual, const float* rot, const float* width, const float* occ_logits, const float* label,
                            const float* rot_targets, const float* width_target, const float* occ_target, int B, int M,
                            float* losses, float* scene_losses, void* acc, void* stream) {
    if (B < 0 || M < 0) return -1;
    if (!acc || (reinterpret_cast<uintptr_t>(acc) & 7)) return -1;
    if (B == 0) return 0;
    if (!qual || !rot || !width || !label || !rot_targets || !width_target || !losses || !scene_losses) return -1;
    if (M > 0 && (!occ_logits || !occ_target)) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    GIGA_LAUNCH(loss_scene_kernel, dim3(B), dim3(256), 0, s, qual, rot, width, occ_logits, label, rot_targets, width_target, occ_target,
                M, scene_losses);
    GIGA_LAUNCH(loss_mean_metrics_kernel, dim3(1), dim3(256), 0, s, scene_losses, qual, label, B, losses,
                static_cast<unsigned long long*>(acc));
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int giga_train_loss_backward(const float* qual, const float* rot, const float* width, const float* occ_logits,
                             const float* label, const float* rot_targets, const float* width_target,
                             const float* occ_target, const float* grad_loss, int B, int M, float* dqual, float* drot,
                             float* dwidth, float* docc, void* stream) {
    if (B < 0 || M < 0) return -1;
    if (B == 0) return 0;
    if (!qual || !rot || !width || !label || !rot_targets || !width_target || !grad_loss || !dqual || !drot || !dwidth)
        return -1;
    if (M > 0 && (!occ_logits || !occ_target || !docc)) return -1;
    GIGA_LAUNCH(loss_grad_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), qual, rot, width, occ_logits, label,
                rot_targets, width_target, occ_target, grad_loss, B, M, dqual, drot, dwidth, docc);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

// the occupancy objective: with `acc` the epoch metrics too (scene_counts is read only then)
static int launch_train_occ_loss(const float* occ, const float* occ_t, int B, int M, float* loss, float* scene_loss, unsigned* scene_counts,
                                 void* acc, hipStream_t s) {
    GIGA_LAUNCH(occ_scene_kernel, dim3(B), dim3(256), 0, s, occ, occ_t, M, scene_loss, acc ? scene_counts : nullptr);
    if (acc)
        GIGA_LAUNCH(occ_mean_metrics_kernel, dim3(1), dim3(128), 0, s, scene_loss, scene_counts, B, loss,
                    static_cast<unsigned long long*>(acc));
    else
        GIGA_LAUNCH(occ_mean_kernel, dim3(1), dim3(64), 0, s, scene_loss, B, loss);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int giga_train_occ_loss(const float* occ_logits, const float* occ_target, int B, int M, float* loss, float* scene_losses,
                        void* stream) {
    if (B < 0 || M < 0) return -1;
    if (B == 0) return 0;
    if (M == 0) return -1;                                  // the loss of a scene is a mean over its points
    if (!occ_logits || !occ_target || !loss || !scene_losses) return -1;
    return launch_train_occ_loss(occ_logits, occ_target, B, M, loss, scene_losses, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int giga_train_occ_loss_metrics(const float* occ_logits, const float* occ_target, int B, int M, float* loss, float* scene_losses,
                                uint32_t* scene_counts, void* acc, void* stream) {
    if (B < 0 || M < 0) return -1;
    if (!acc || (reinterpret_cast<uintptr_t>(acc) & 7)) return -1;
    if (B == 0) return 0;
    if (M == 0) return -1;
    if (!occ_logits || !occ_target || !loss || !scene_losses || !scene_counts) return -1;
    return launch_train_occ_loss(occ_logits, occ_target, B, M, loss, scene_losses, scene_counts, acc, static_cast<hipStream_t>(stream));
}

int giga_train_occ_loss_backward(const float* occ_logits, const float* occ_target, const float* grad_loss, int B, int M, float* docc,
                                 void* stream) {
    if (B < 0 || M < 0) return -1;
    if (B == 0) return 0;
    if (M == 0) return -1;
    if (!occ_logits || !occ_target || !grad_loss || !docc) return -1;
    GIGA_LAUNCH(occ_grad_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), occ_logits, occ_target, grad_loss, B, M, docc);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int giga_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                   double beta2, double eps, double weight_decay, int step, void* stream) {
    if (n == 0) return 0;
    if (!params || !grads || !exp_avg || !exp_avg_sq || step < 1) return -1;
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0)) return -1;
    // the kernel moves float4: all four buffers must be 16-byte aligned (whole torch allocations are; a view at an odd offset is not)
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15) return -1;
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);     // (hyper-parameters stay double on the host, as in torch)
    const size_t n4 = n / 4;
    GIGA_LAUNCH(adam_flat_kernel, dim3((unsigned)((n4 + 1 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                reinterpret_cast<float4*>(params), reinterpret_cast<const float4*>(grads), reinterpret_cast<float4*>(exp_avg),
                reinterpret_cast<float4*>(exp_avg_sq), n4, n, (float)(lr / bc1), (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                (float)eps, (float)weight_decay, (float)sqrt(bc2));
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

}  // extern "C"
