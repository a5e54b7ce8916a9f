// extern "C" entry points of libgiga_hip.so (declared in include/giga_hip.h).
#include <hip/hip_runtime.h>
#include "giga_launch.h"

#include "../../include/giga_hip.h"
#include "giga_layout.h"
#include "giga_conv32_geom.h"
#include "giga_dect.h"
#include "giga_args.h"
#include "giga_side.h"

namespace giga {
// giga_pack.cpp
size_t packed_bytes();
int pack_weights_host(const float* P, size_t n_params, int head_present, uint8_t* blob, size_t blob_bytes);
int pack_map_host(int head_present, int32_t* map, size_t nwords);
size_t bwd_packed_bytes();
int pack_bwd_host(const float* P, size_t n_params, int head_present, uint8_t* blob, size_t blob_bytes);
int pack_bwd_map_host(int head_present, int32_t* map, size_t nwords);
int packed_check_host(const uint8_t* blob, size_t bytes, int backward);
// giga_encoder_bwd.hip / giga_decoder_bwd.hip
void persistent_forget();
int launch_encoder_backward(const float* tsdf, const uint8_t* blob, const uint8_t* bwd_blob, const uint8_t* fws,
                            float* gplanes, uint8_t* gws, float* grads, int head_present, int B, hipStream_t s, bool bf16_convs, bool convin_mask,
                            SideScope& side);
size_t dec_bwd_scratch_floats(long long P, int nheads);
bool dec_bwd_writes_planes(int nheads, int B, int N);
int launch_decoder_backward(const float* planes, const float* p, const uint8_t* blob, const uint8_t* bwd_blob,
                            int head_mask, const float* const* outs, const float* const* douts, float* gplanes,
                            float* grads, int head_present, float* scratch, int B, int N, hipStream_t s, bool writes_planes,
                            SideScope* side);
int launch_plane_gather(const float* dcbuf, const float* p, float* gplanes, int B, int N, hipStream_t s);
// giga_decoder_pgrad.hip
int launch_decoder_point_grad(const float* planes, const float* p, const uint8_t* blob, const uint8_t* bwd_blob, int head_mask,
                              const float* const* douts, float* const* outs, float* dp, int B, int N, hipStream_t s);
int launch_decoder_point_hess(const float* planes, const float* p, const uint8_t* blob, const uint8_t* bwd_blob, float* logit,
                              float* dp, float* hess, int B, int N, hipStream_t s);
// giga_refine.hip
int launch_refine_face_points(const float* vertices, const int* faces, const float* eps_in, float* eps, float* points, int V, int F,
                              unsigned long long seed, int step, hipStream_t s);
int launch_refine_face_grad(const float* vertices, const int* faces, const float* eps, const float* logit, const float* dp,
                            const float* hess, double threshold, float* floss, float* fgrad, int V, int F, hipStream_t s);
int launch_refine_vertex_step(const float* fgrad, const int* corner_order, const int* vertex_offsets, float* vertices,
                              float* square_avg, float* grad, int V, int F, hipStream_t s);
// giga_decoder_train16.hip (bf16 decoder of the bf16 training step)
int launch_dect_forward(const float* planes, const float* p, const uint8_t* blob, int head_mask, float* const* outs, int B, int N,
                        int post, hipStream_t s);
size_t dect_partial_floats(long long P, int nheads);
int launch_dect_backward(const float* planes, const float* p, const uint8_t* blob, const uint8_t* bwd_blob, int head_mask,
                         const float* const* outs, const float* const* douts, float* gplanes, float* dcbuf, float* scratch, int B,
                         int N, hipStream_t s, DectPending* pend);
int launch_dect_reduce(const DectPending& pend, float* grads, int head_present, hipStream_t s);
// giga_loss.hip
int launch_train_loss(const float* qual, const float* rot, const float* width, const float* occ, const float* label,
                      const float* rot_t, const float* width_t, const float* occ_t, int B, int M, float* losses,
                      float* scene_loss, hipStream_t s);
int launch_train_loss_metrics(const float* qual, const float* rot, const float* width, const float* occ, const float* label,
                              const float* rot_t, const float* width_t, const float* occ_t, int B, int M, float* losses,
                              float* scene_loss, void* acc, hipStream_t s);
int launch_train_loss_backward(const float* qual, const float* rot, const float* width, const float* occ,
                               const float* label, const float* rot_t, const float* width_t, const float* occ_t,
                               const float* gout, int B, int M, float* dqual, float* drot, float* dwidth, float* docc,
                               hipStream_t s);
int launch_train_occ_loss(const float* occ, const float* occ_t, int B, int M, float* loss, float* scene_loss, unsigned* scene_counts,
                          void* acc, hipStream_t s);
int launch_train_occ_loss_backward(const float* occ, const float* occ_t, const float* gout, int B, int M, float* docc, hipStream_t s);
// giga_tsdf.hip
int launch_tsdf_scatter(const int* index, const float* value, const int* offsets, int B, int R, int n, float* grid,
                        int* winner, hipStream_t s);
size_t tsdf_integrate_workspace_bytes(int B, int n_views);
int launch_tsdf_integrate(const float* depth, const int* view_offsets, const double* extrinsics, const double* intrinsics, int B,
                          int W, int H, double length, int R, double sdf_trunc, double depth_scale, double depth_trunc, float* tsdf,
                          float* weight, float* grid, uint8_t* ws, hipStream_t s);
size_t tsdf_cloud_workspace_bytes(int B, int R);
int launch_tsdf_cloud_count(const float* tsdf, const float* weight, int B, int R, uint8_t* ws, int* counts, hipStream_t s);
int launch_tsdf_cloud_emit(const float* tsdf, const float* weight, int B, int R, double length, const uint8_t* ws, float* points,
                           size_t cap, int* shortfall, hipStream_t s);
// giga_render.hip
size_t depth_render_workspace_bytes(int B, int n_views);
int launch_depth_render(const float* vertices, const int* vertex_offsets, const int* triangles, const int* triangle_offsets,
                        const int* view_offsets, const double* extrinsics, const double* intrinsics, int B, int W, int H, double near,
                        double far, double pixel_offset, float* depth, uint8_t* ws, hipStream_t s);
// giga_noise.hip
size_t depth_noise_workspace_bytes(int n);
int launch_depth_noise(const float* in, float* out, int n, int W, int H, int model, const double* p, unsigned long long seed,
                       const unsigned long long* image_ids, uint8_t* ws, hipStream_t s);
// giga_batch.hip
int launch_batch_draw(const GigaBatchSet& set, const int32_t* ordinals, const int32_t* rows, int B, int M, int epoch,
                      unsigned long long seed, int32_t* quarter, double* u, int32_t* file, int32_t* index, hipStream_t s);
int launch_batch_assemble(const GigaBatchSet& set, const int32_t* rows, const int32_t* quarter, const double* u, const int32_t* file,
                          const int32_t* index, int B, int M, int augment, float* x, float* pos, float* pos_occ, float* label,
                          float* rotations, float* width, float* occ, hipStream_t s);
// giga_mesh.hip
size_t mesh_workspace_bytes(int B, int nx, int ny, int nz);
int launch_mesh_count(const float* grids, int B, int nx, int ny, int nz, double iso, uint8_t* ws, int* counts, hipStream_t s);
int launch_mesh_emit(const float* grids, int B, int nx, int ny, int nz, double iso, double box, const uint8_t* ws, float* vertices,
                     size_t cap_v, int* triangles, size_t cap_t, int* shortfall, hipStream_t s);
// giga_simplify.hip
long long simplify_ref_capacity(int n_triangles_of_mesh, int ref_extra);
size_t simplify_workspace_bytes(int B, long long n_vertices, long long n_triangles, long long ref_total);
int launch_mesh_simplify(const void* vertices, int vertices_f64, const int* vertex_offsets, const int* triangles,
                         const int* triangle_offsets, const int* targets, int B, double agressiveness, int ref_extra,
                         double* out_vertices, int* out_triangles, int* out_counts, int* stats, uint8_t* ws, hipStream_t st);
// giga_mise.hip
size_t mise_workspace_bytes(int B, int res0, int depth);
int launch_mise_init(int B, int res0, int depth, uint8_t* ws, hipStream_t s);
int launch_mise_count(int B, int res0, int depth, uint8_t* ws, int* counts, hipStream_t s);
int launch_mise_emit(int B, int res0, int depth, const uint8_t* ws, int* query, size_t cap, int* shortfall, const float* lin,
                     float* points, hipStream_t s);
int launch_mise_update(const float* values, const int* query, size_t cap, int B, int res0, int depth, double thr, uint8_t* ws,
                       hipStream_t s);
int launch_mise_to_dense(int B, int res0, int depth, const uint8_t* ws, float* grid, hipStream_t s);
// giga_eval.hip
size_t nn_workspace_bytes(int B, int n_src);
int launch_nn_query(const float* src, const int* src_offsets, const float* tgt, const int* tgt_offsets, int B, float* dist,
                    int* idx, uint8_t* ws, hipStream_t s);
size_t sample_workspace_bytes(int B, int n_tri);
int launch_mesh_sample(const float* vertices, const int* vertex_offsets, const int* triangles, const int* triangle_offsets, int B,
                       int n, unsigned long long seed, int first_scene, float* points, int* face, float* normals, int* counts,
                       uint8_t* ws, hipStream_t s);
size_t contains_workspace_bytes(int B, int n_tri, int n_pts);
int launch_mesh_contains(const float* vertices, const int* vertex_offsets, const int* triangles, const int* triangle_offsets,
                         const double* points, const int* point_offsets, int B, int resolution, uint8_t* inside, uint8_t* ws,
                         hipStream_t s);
// giga_collide.hip
size_t collide_workspace_bytes(int M, int P);
int launch_mesh_collide(const float* vertices, const int* vertex_offsets, const int* triangles, const int* triangle_offsets, int M,
                        const int* pairs, int P, uint8_t* hit, uint8_t* ws, hipStream_t s);
// giga_geometry.hip
size_t roi_workspace_bytes(int G);
int launch_roi_points(const double* grasps, const int* offsets, const int* scene, const int* first, int G, unsigned long long seed,
                      double extent, double size, double* world, float* normalised, uint8_t* ws, hipStream_t s);
size_t confusion_workspace_bytes(int B);
int launch_occ_confusion(const float* logits, const uint8_t* pred, double th, const uint8_t* target, const int* offsets, int B,
                         unsigned long long* counts, uint8_t* ws, hipStream_t s);
// giga_affordance.hip
size_t affordance_workspace_bytes(int B, int R);
void affordance_colormap(uint8_t* rgba);
int launch_affordance_points(const float* qual, const float* rot, int B, int R, const GigaAffordanceParams* prm, double* points,
                             int* counts, uint8_t* ws, hipStream_t s);
int launch_affordance_faces(const float* vertices, const int* vertex_offsets, const int* triangles, const int* triangle_offsets,
                            const double* points, const int* counts, int B, int R, const GigaAffordanceParams* prm,
                            double* affordance, uint8_t* rgba, uint8_t* ws, hipStream_t s);
// giga_encoder.hip
EncWs enc_workspace(int B, int precision);
int launch_encoder(const float* tsdf, const uint8_t* blob, void* planes_nhwc, float* planes_nchw, int B,
                   int precision, uint8_t* ws, hipStream_t s, int probe_stage, void* ev0, void* ev1);
// giga_decoder.hip
int launch_decoder(const DecArgs& a, int precision, hipStream_t s, void* ev0, void* ev1);
int launch_adam_flat(float* p, const float* g, float* m, float* v, size_t n, double lr, double b1, double b2, double eps, double wd,
                     int step, hipStream_t s);
int launch_planes_pack(const float* xz, const float* xy, const float* yz, void* dst, int B, int precision, hipStream_t s);
int launch_lattice_resample(const void* planes, const float* lin, void* out, int B, int R, int precision, hipStream_t s,
                            bool planes_fp32 = false);
int launch_planes_unpack(const void* src, float* dst, int B, int precision, hipStream_t s);
}  // namespace giga

using namespace giga;

std::atomic<unsigned long long> giga::g_launch_count{0};
std::atomic<unsigned long long> giga::g_probe_target{0};
void* giga::g_probe_ev[2] = {nullptr, nullptr};
const char* volatile giga::g_probe_name = "";

// byte offset of head h's weight image for a precision (0 fp32, 1 f16, 2 f16x3 split), plain or with conv_final folded in
static size_t head_image_offset(const PackOff& ko, int h, int precision, bool fold) {
    if (precision == 2) return fold ? ko.dec16sf[h] : ko.dec16s[h];
    if (precision == 1) return fold ? ko.dec16f[h] : ko.dec16[h];
    return fold ? ko.dec32f[h] : ko.dec32[h];
}

// blob word w <- params[map[w]] (map >= 0) | 0 (map == -1) | untouched (map == -2)
__global__ void repack_kernel(const float* __restrict__ params, const int32_t* __restrict__ map,
                              float* __restrict__ words, size_t nwords) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwords) return;
    const int m = map[i];
    if (m >= 0) words[i] = params[m];
    else if (m == -1) words[i] = 0.f;
}

// bf16 fragment images (f16 fragment layout: lane (j, g) holds channels 8g..8g+7 of k-group kg32) from the fp32 fragments
// (lane (j, g') holds channels 4g'..4g'+3 of k-group kg16 = 2*kg32 + h): one workgroup per bf16 fragment.
struct BfRegions { size_t src[2 * NCONV], dst[2 * NCONV]; int first[2 * NCONV + 1]; int n; };
__device__ __forceinline__ void derive_bf16_block(uint8_t* fwd, uint8_t* bwd, const BfRegions& r, int blk) {
    int reg = 0;
    while (reg + 1 < r.n && blk >= r.first[reg + 1]) ++reg;
    const int i16 = blk - r.first[reg], lane = threadIdx.x;
    uint8_t* base = reg < NCONV ? fwd : bwd;
    if (!base) return;
    const float* f32 = reinterpret_cast<const float*>(base + r.src[reg]);
    __bf16* out = reinterpret_cast<__bf16*>(base + r.dst[reg]) + ((size_t)i16 * 64 + lane) * 8;
    const int j = lane & 15, g = lane >> 4;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = 8 * g + e;
        out[e] = (__bf16)f32[((size_t)(2 * i16 + c / 16) * 64 + ((c % 16) / 4) * 16 + j) * 4 + c % 4];
    }
}

// bf16 conv32 images (A operands of v_mfma_f32_32x32x16_bf16, giga_pack.cpp: lane (i, hi), element e -> W[32 cs + c32_row_cout(i)][16 kc +
// 8 hi + e][tap], fragment order [sub][cs][tap][kc]) from the fp32 conv16 fragments of the same layer (lane (j, g), element e ->
// W[16 nb + j][16 kg + 4 g + e][tap], order [sub][nb][tap][kg]): one workgroup per conv32 fragment.
struct C32bRegions { size_t src[NCONV], dst[NCONV]; int first[NCONV + 1]; int nbt[NCONV], taps[NCONV], kg[NCONV]; };
__device__ __forceinline__ void derive_c32b_block(uint8_t* fwd, const C32bRegions& r, int blk) {
    int l = 0;
    while (l + 1 < NCONV && blk >= r.first[l + 1]) ++l;
    const int f = blk - r.first[l], lane = threadIdx.x;
    const int KG = r.kg[l], TAPS = r.taps[l], NBT = r.nbt[l], CS = NBT / 2;
    const int kc = f % KG, tap = (f / KG) % TAPS, cs = (f / (KG * TAPS)) % CS, sub = f / (KG * TAPS * CS);
    const int i = lane & 31, hi = lane >> 5;
    const int co = 32 * cs + c32_row_cout(i), nb = co >> 4, j = co & 15;
    const float* f32 = reinterpret_cast<const float*>(fwd + r.src[l]);
    const size_t i32 = ((size_t)(sub * NBT + nb) * TAPS + tap) * KG + kc;
    __bf16* out = reinterpret_cast<__bf16*>(fwd + r.dst[l]) + ((size_t)f * 64 + lane) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int rr = 8 * hi + e;
        out[e] = (__bf16)f32[(i32 * 64 + (rr >> 2) * 16 + j) * 4 + (rr & 3)];
    }
}

// Winograd F(2x2, 3x3) images (giga_wino.h; giga_pack.cpp::pack_wino) from the fp32 conv16 fragments of the same layer: one workgroup per
// 512-byte piece [grp][kpass][pos][chunk][half] = 64 lanes x 2 floats, U = G g G^T accumulated in double in the packer's order, so the
// device image equals the host's bit for bit.
struct WinoRegions { size_t src[NCONV], dst[NCONV]; int first[NCONV + 1]; int cin[NCONV]; };
__device__ __forceinline__ void derive_wino_block(uint8_t* fwd, const WinoRegions& r, int blk) {
    int l = 0;
    while (l + 1 < NCONV && blk >= r.first[l + 1]) ++l;
    const int f = blk - r.first[l], lane = threadIdx.x;
    const int cin = r.cin[l], kp = cin > 64 ? cin / 64 : 1, cinp = cin / kp, nchunk = cinp / 16, KG = cin / 16;
    const int h = f & 1, cc = (f >> 1) % nchunk, pos = (f / (2 * nchunk)) & 15, k = (f / (32 * nchunk)) % kp, grp = f / (32 * nchunk * kp);
    const int j = lane & 15, g = lane >> 4, xi = pos >> 2, nu = pos & 3;
    const float* f32 = reinterpret_cast<const float*>(fwd + r.src[l]);           // [nb][tap][kg][lane (j, g')][e']: W[16 nb + j][16 kg + 4 g' + e'][tap]
    float* out = reinterpret_cast<float*>(fwd + r.dst[l]) + ((size_t)f * 64 + lane) * 2;
    const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int ci = cinp * k + 16 * cc + 4 * g + 2 * h + e;
        double u = 0.0;
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) {
                const float w = f32[((((size_t)grp * 9 + ky * 3 + kx) * KG + ci / 16) * 64 + ((ci % 16) / 4) * 16 + j) * 4 + ci % 4];
                u += G[xi][ky] * G[nu][kx] * (double)w;
            }
        out[e] = (float)u;
    }
}

constexpr int DECT_DERIVE_BLOCKS = (59 + 51) * NHEADS;
struct DeriveArgs {
    BfRegions r; C32bRegions c; int n16, n32;
    size_t dec32_0, dec32_stride, dectf_0, dectf_stride, decb_0, decb_stride, dectb_0, dectb_stride;
    size_t convin_w, convin_ws;
};
__global__ __launch_bounds__(64) void derive_all_kernel(uint8_t* fwd, uint8_t* bwd, DeriveArgs d) {
    const int b = blockIdx.x;
    if (b < d.n16) derive_bf16_block(fwd, bwd, d.r, b);
    else if (b < d.n16 + d.n32) derive_c32b_block(fwd, d.c, b - d.n16);
    else if (b == d.n16 + d.n32 + DECT_DERIVE_BLOCKS) {
        // f16x3 split conv_in operands (giga_pack.cpp): [2 channel halves][hi | lo][lane (j, g)][8 halfs e] <- W[16 h + j][ci16_tap(g, e)],
        // from the fp32 image [h][K-step s of 4 taps][lane (j, k)] = W[16 h + j][4 s + k]
        if (!fwd) return;
        const float* cw = reinterpret_cast<const float*>(fwd + d.convin_w);
        _Float16* cs = reinterpret_cast<_Float16*>(fwd + d.convin_ws);
        const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
        for (int h = 0; h < 2; ++h)
            for (int e = 0; e < 8; ++e) {
                const int tap = ci16_tap(g, e);
                const float w = tap >= 0 ? cw[(h * 7 + tap / 4) * 64 + (tap % 4) * 16 + j] : 0.f;
                const _Float16 hi = (_Float16)w;
                cs[((2 * h) * 64 + lane) * 8 + e] = hi;
                cs[((2 * h + 1) * 64 + lane) * 8 + e] = (_Float16)(w - (float)hi);
            }
    } else {
        const int k = b - d.n16 - d.n32;
        dect_derive_block(fwd, bwd, k % (59 + 51), k / (59 + 51), d.dec32_0, d.dec32_stride, d.dectf_0, d.dectf_stride, d.decb_0,
                          d.decb_stride, d.dectb_0, d.dectb_stride);
    }
}
__global__ void repack2_kernel(const float* __restrict__ params, const int32_t* __restrict__ map_a, float* __restrict__ words_a, size_t na,
                               const int32_t* __restrict__ map_b, float* __restrict__ words_b, size_t nb) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t* map = map_a; float* words = words_a;
    if (i >= na) { i -= na; if (i >= nb) return; map = map_b; words = words_b; }
    const int m = map[i];
    if (m >= 0) words[i] = params[m];
    else if (m == -1) words[i] = 0.f;
}

// one launch for both blobs: blocks [0, nf) derive the forward blob's images, the rest the backward blob's
__global__ __launch_bounds__(64) void derive_wino_kernel(uint8_t* fwd, WinoRegions wf, int nf, uint8_t* bwd, WinoRegions wb) {
    const int b = (int)blockIdx.x;
    if (b < nf) derive_wino_block(fwd, wf, b);
    else derive_wino_block(bwd, wb, b - nf);
}

extern "C" {

/* Winograd images of the fp32 3x3 layers (giga_wino.h) from the fp32 fragments of the same DEVICE blob, after giga_repack_device:
 * the forward blob's (the layers themselves) and / or the backward blob's (their data-gradient convolutions: the same fragment layout
 * with the channels swapped) -- either pointer may be NULL */
int giga_derive_winograd(void* packed_dev, void* bwd_packed_dev, void* stream) {
    if (!packed_dev && !bwd_packed_dev) return -1;
    const PackOff ko = pack_offsets();
    const BwdPackOff bo = bwd_pack_offsets();
    WinoRegions w[2] = {};
    int n[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        if (!(pass ? bwd_packed_dev : packed_dev)) continue;
        int nw = 0;
        for (int l = 0; l < NCONV; ++l) {
            const ConvLayerDesc& cd = kConv[l];
            w[pass].src[l] = pass ? bo.conv[l] : ko.conv[l].w32; w[pass].dst[l] = pass ? bo.wino[l] : ko.conv[l].wino; w[pass].first[l] = nw;
            w[pass].cin[l] = pass ? cd.cout : cd.cin0 + cd.cin1;                      // channels IN of the convolution the image is for
            if (cd.kind == CONV3) nw += (cd.cin0 + cd.cin1) * cd.cout / 8;           // 512-byte pieces of the layer's image
        }
        w[pass].first[NCONV] = nw;
        n[pass] = nw;
    }
    GIGA_LAUNCH(derive_wino_kernel, dim3(n[0] + n[1]), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<uint8_t*>(packed_dev), w[0], n[0],
                static_cast<uint8_t*>(bwd_packed_dev), w[1]);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

int giga_derive_bf16_fragments(void* packed_dev, void* bwd_packed_dev, void* stream) {
    if (!packed_dev && !bwd_packed_dev) return -1;
    const PackOff ko = pack_offsets();
    const BwdPackOff bo = bwd_pack_offsets();
    DeriveArgs d{};
    int at = 0;
    for (int l = 0; l < NCONV; ++l) { d.r.src[l] = ko.conv[l].w32; d.r.dst[l] = ko.conv[l].wbf; d.r.first[l] = at; at += ko.conv[l].nfrag16; }
    for (int l = 0; l < NCONV; ++l) {
        d.r.src[NCONV + l] = bo.conv[l]; d.r.dst[NCONV + l] = bo.convbf[l]; d.r.first[NCONV + l] = at; at += bo.nfrag[l] / 2;
    }
    d.r.first[2 * NCONV] = at;
    d.r.n = 2 * NCONV;
    d.n16 = at;
    int n32 = 0;
    for (int l = 0; l < NCONV; ++l) {
        const ConvLayerDesc& cd = kConv[l];
        d.c.src[l] = ko.conv[l].w32; d.c.dst[l] = ko.conv[l].c32b; d.c.first[l] = n32; n32 += ko.conv[l].nfragc32;
        d.c.nbt[l] = cd.cout / 16; d.c.taps[l] = conv_taps(cd); d.c.kg[l] = (cd.cin0 + cd.cin1) / 16;
    }
    d.c.first[NCONV] = n32;
    d.n32 = packed_dev ? n32 : 0;
    d.dec32_0 = ko.dec32[0]; d.dec32_stride = ko.dec32[1] - ko.dec32[0]; d.dectf_0 = ko.dect[0]; d.dectf_stride = ko.dect[1] - ko.dect[0];
    d.decb_0 = bo.dec[0]; d.decb_stride = bo.dec[1] - bo.dec[0]; d.dectb_0 = bo.dect[0]; d.dectb_stride = bo.dect[1] - bo.dect[0];
    d.convin_w = ko.convin_w; d.convin_ws = ko.convin_ws;
    // ONE launch: the bf16 conv16 fragments of both blobs, the bf16 conv32 images, the bf16 decoder images (giga_dect.h), the f16x3 conv_in operands
    GIGA_LAUNCH(derive_all_kernel, dim3(d.n16 + d.n32 + DECT_DERIVE_BLOCKS + 1), dim3(64), 0, static_cast<hipStream_t>(stream),
                static_cast<uint8_t*>(packed_dev), static_cast<uint8_t*>(bwd_packed_dev), d);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

/* both weight images in ONE launch (training: every step) */
int giga_repack_device2(const float* params_dev, const int32_t* map_fwd_dev, void* packed_dev, size_t nwords_fwd,
                        const int32_t* map_bwd_dev, void* bwd_packed_dev, size_t nwords_bwd, void* stream) {
    if (!params_dev || !map_fwd_dev || !packed_dev || !map_bwd_dev || !bwd_packed_dev) return -1;
    const size_t n = nwords_fwd + nwords_bwd;
    if (n == 0) return 0;
    GIGA_LAUNCH(repack2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), params_dev,
                map_fwd_dev, static_cast<float*>(packed_dev), nwords_fwd, map_bwd_dev, static_cast<float*>(bwd_packed_dev), nwords_bwd);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

static_assert(GIGA_ABI_VERSION == PACK_ABI_VERSION, "the blob stamp carries the ABI version");
int giga_abi_version(void) { return GIGA_ABI_VERSION; }

int giga_packed_check(const void* packed_host, size_t bytes, int backward) {
    if (!packed_host) return -1;
    return packed_check_host(static_cast<const uint8_t*>(packed_host), bytes, backward ? 1 : 0);
}

const char* giga_strerror(int code) {
    switch (code) {
        case 0: return "ok";
        case -1: return "invalid argument";
        case -2: return "parameter count does not match the head set";
        case -3: return "packed buffer too small";
        case -4: return "workspace too small";
        case -5: return "unsupported precision";
        case -6: return "null pointer for a requested output";
        case -7: return "more than GIGA_MAX_SCENES scenes in one call";
        case -8: return "packed blob was not produced by this version of the library (repack the weights)";
        case -10: return "HIP launch failed";
        case -11: return "a face index lies outside its mesh's vertex range";
        case -12: return "mesh simplification: a pass exceeded its round bound, or the reference-list capacity is too small for one collapse";
        default: return "unknown error";
    }
}

size_t giga_param_count(int head_present) { return param_offsets(head_present & 15).total; }

size_t giga_packed_bytes(void) { return packed_bytes(); }

int giga_pack_weights(const float* params_host, size_t n_params, int head_present, void* packed_host,
                      size_t packed_bytes_) {
    if (!params_host || !packed_host) return -1;
    return pack_weights_host(params_host, n_params, head_present & 15, static_cast<uint8_t*>(packed_host),
                             packed_bytes_);
}

int giga_pack_map(int head_present, int32_t* map_host, size_t nwords) {
    if (!map_host) return -1;
    return pack_map_host(head_present & 15, map_host, nwords);
}

int giga_repack_device(const float* params_dev, const int32_t* map_dev, void* packed_dev, size_t nwords,
                       void* stream) {
    if (!params_dev || !map_dev || !packed_dev) return -1;
    if (nwords == 0) return 0;
    GIGA_LAUNCH(repack_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), params_dev, map_dev, static_cast<float*>(packed_dev), nwords);
    return hipGetLastError() == hipSuccess ? 0 : -10;
}

size_t giga_encoder_workspace_bytes(int B, int precision) {
    precision &= ~GIGA_ENCODER_FLAGS;
    if (B <= 0) return 0;
    return enc_workspace(B, precision).total;
}

int giga_encoder_workspace_layout(int B, int precision, size_t* offsets) {
    if (B <= 0 || !offsets) return -1;
    precision &= ~GIGA_ENCODER_FLAGS;
    if (precision < 0 || precision > 3) return -5;
    const EncWs w = enc_workspace(B, precision);
    const size_t v[17] = {w.P0, w.A0, w.S0, w.Q0, w.A1, w.S1, w.Q1, w.A2, w.S2, w.U0, w.A3, w.A4, w.U1, w.A5, w.A6,
                          w.YZ, w.XZ};
    for (int i = 0; i < 17; ++i) offsets[i] = v[i];
    return 0;
}

int giga_encoder_forward_probe(const float* tsdf, const void* packed, void* planes_nhwc, float* planes_nchw,
                               int B, int precision, void* workspace, size_t workspace_bytes, void* stream,
                               int probe_stage, void* ev_start, void* ev_stop) {
    if (B < 0 || (B > 0 && (!tsdf || !packed || !planes_nhwc || !workspace))) return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    const bool fold = (precision & GIGA_FOLD_FINAL) != 0;     // stop before conv_final (folded decoder images)
    const int persist = precision & (GIGA_PERSIST_UNET | GIGA_LAYERWISE_UNET | GIGA_CONV32_UNET | GIGA_CONV16_UNET | GIGA_CONVIN_MASK | GIGA_DIRECT_CONV);   // U-Net launch form and kernels (see the header)
    precision &= ~GIGA_ENCODER_FLAGS;
    if (precision < 0 || precision > 3) return -5;
    // only the fp32 and bf16 encoders store conv_in's ReLU mask: a precision 1 / 2 forward that claims to would leave giga_backward
    // (GIGA_CONVIN_MASK_BWD) reading workspace bytes nobody wrote
    if ((persist & GIGA_CONVIN_MASK) && (precision == 1 || precision == 2)) return -5;
    if (fold && planes_nchw) return -1;                       // the reference-layout copy is the FINAL planes only
    if (workspace_bytes < giga_encoder_workspace_bytes(B, precision)) return -4;
    return launch_encoder(tsdf, static_cast<const uint8_t*>(packed), planes_nhwc, planes_nchw, B,
                          precision | (fold ? GIGA_FOLD_FINAL : 0) | persist,
                          static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream), probe_stage,
                          ev_start, ev_stop);
}

int giga_encoder_forward(const float* tsdf, const void* packed, void* planes_nhwc, float* planes_nchw, int B,
                         int precision, void* workspace, size_t workspace_bytes, void* stream) {
    return giga_encoder_forward_probe(tsdf, packed, planes_nhwc, planes_nchw, B, precision, workspace,
                                      workspace_bytes, stream, -1, nullptr, nullptr);
}

unsigned long long giga_launch_count(void) { return g_launch_count.load(std::memory_order_relaxed); }

int giga_launch_probe(unsigned long long ordinal, void* ev_start, void* ev_stop) {
    if (ordinal != 0 && (!ev_start || !ev_stop)) return -1;
    g_probe_target.store(0, std::memory_order_relaxed);
    g_probe_ev[0] = ev_start; g_probe_ev[1] = ev_stop;
    g_probe_target.store(ordinal, std::memory_order_release);
    return 0;
}
const char* giga_launch_probe_name(void) { return g_probe_name; }

void giga_forget_device_state(void) {
    giga::dyn_lds_forget();
    giga::persistent_forget();
    giga::side_streams_forget();
}

void* giga_event_create(void) {
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? static_cast<void*>(e) : nullptr;
}
void giga_event_destroy(void* ev) { if (ev) (void)hipEventDestroy(static_cast<hipEvent_t>(ev)); }
int giga_event_record(void* ev, void* stream) {
    if (!ev) return -1;
    return hipEventRecord(static_cast<hipEvent_t>(ev), static_cast<hipStream_t>(stream)) == hipSuccess ? 0 : -10;
}
int giga_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms) {
    if (!ev_start || !ev_stop || !ms) return -1;
    if (hipEventSynchronize(static_cast<hipEvent_t>(ev_stop)) != hipSuccess) return -10;
    return hipEventElapsedTime(ms, static_cast<hipEvent_t>(ev_start), static_cast<hipEvent_t>(ev_stop)) == hipSuccess
               ? 0 : -10;
}

int giga_planes_pack(const float* xz, const float* xy, const float* yz, void* planes_nhwc, int B, int precision,
                     void* stream) {
    if (B < 0 || (B > 0 && (!xz || !xy || !yz || !planes_nhwc))) return -1;
    if (precision < 0 || precision > 2) return -5;
    return launch_planes_pack(xz, xy, yz, planes_nhwc, B, precision, static_cast<hipStream_t>(stream));
}

int giga_planes_unpack(const void* planes_nhwc, float* planes_nchw, int B, int precision, void* stream) {
    if (B < 0 || (B > 0 && (!planes_nhwc || !planes_nchw))) return -1;
    if (precision < 0 || precision > 2) return -5;
    return launch_planes_unpack(planes_nhwc, planes_nchw, B, precision, static_cast<hipStream_t>(stream));
}

// the head list of a decoder launch: the heads of `head_mask` in order, each with its image in the packed blob and its output.
// -6: a requested head has no output
static int dec_args_heads(DecArgs& a, int head_mask, float* const (&outs)[NHEADS], const PackOff& ko, int precision, bool fold) {
    a.nheads = 0;
    for (int h = 0; h < NHEADS; ++h) {
        if (!(head_mask >> h & 1)) continue;
        if (!outs[h]) return -6;
        a.head_id[a.nheads] = h;
        a.head_off[a.nheads] = head_image_offset(ko, h, precision, fold);
        a.out[a.nheads] = outs[h];
        ++a.nheads;
    }
    return 0;
}

int giga_decoder_forward_probe(const void* planes_nhwc, const float* p, const void* packed, int head_mask,
                               float* qual, float* rot, float* width, float* occ, int B, int N, int precision,
                               int post, void* stream, void* ev_start, void* ev_stop);

int giga_decoder_forward(const void* planes_nhwc, const float* p, const void* packed, int head_mask, float* qual,
                         float* rot, float* width, float* occ, int B, int N, int precision, int post,
                         void* stream) {
    return giga_decoder_forward_probe(planes_nhwc, p, packed, head_mask, qual, rot, width, occ, B, N, precision,
                                      post, stream, nullptr, nullptr);
}

int giga_decoder_forward_probe(const void* planes_nhwc, const float* p, const void* packed, int head_mask,
                               float* qual, float* rot, float* width, float* occ, int B, int N, int precision,
                               int post, void* stream, void* ev_start, void* ev_stop) {
    if (B < 0 || N < 0) return -1;
    const bool fold = (precision & GIGA_FOLD_FINAL) != 0;     // planes are the encoder output BEFORE conv_final
    precision &= ~GIGA_FOLD_FINAL;
    if (precision < 0 || precision > 3 || (precision == 3 && fold)) return -5;
    if ((long long)B * N == 0 || (head_mask & 15) == 0) return 0;
    if (!planes_nhwc || !p || !packed) return -1;
    if (precision == 3) {                                     // bf16 operands / fp32 accumulate on fp32 planes: the bf16 training forward
        float* outs3[NHEADS] = {qual, rot, width, occ};
        for (int h = 0; h < NHEADS; ++h)
            if ((head_mask >> h & 1) && !outs3[h]) return -6;
        hipStream_t s3 = static_cast<hipStream_t>(stream);
        if (ev_start && hipEventRecord(static_cast<hipEvent_t>(ev_start), s3) != hipSuccess) return -10;
        const int rc3 = launch_dect_forward(static_cast<const float*>(planes_nhwc), p, static_cast<const uint8_t*>(packed), head_mask & 15,
                                            outs3, B, N, post, s3);
        if (ev_stop && hipEventRecord(static_cast<hipEvent_t>(ev_stop), s3) != hipSuccess) return -10;
        return rc3;
    }
    DecArgs a{};
    a.planes = planes_nhwc; a.p = p; a.blob = static_cast<const uint8_t*>(packed);
    float* outs[NHEADS] = {qual, rot, width, occ};
    if (const int rc = dec_args_heads(a, head_mask, outs, pack_offsets(), precision, fold)) return rc;
    a.B = B; a.N = N; a.P = (long long)B * N; a.post = post;
    return launch_decoder(a, precision, static_cast<hipStream_t>(stream), ev_start, ev_stop);
}

size_t giga_lattice_workspace_bytes(int B, int R, int precision) {
    precision &= ~(GIGA_FOLD_FINAL | GIGA_PLANES_FP32);
    if (B <= 0 || R <= 0) return 0;
    return (size_t)3 * B * R * R * CD * (precision == 1 ? 2 : 4);
}

int giga_decoder_forward_lattice(const void* planes_nhwc, const float* lin, const void* packed, int head_mask,
                                 float* qual, float* rot, float* width, float* occ, int B, int R, int precision,
                                 int post, void* workspace, size_t workspace_bytes, void* stream, void* ev_start,
                                 void* ev_stop) {
    if (B < 0 || R < 0 || R > 64) return -1;
    const bool fold = (precision & GIGA_FOLD_FINAL) != 0;
    const bool planes32 = (precision & GIGA_PLANES_FP32) != 0;        // fp32 planes into the plain-f16 decoder
    precision &= ~(GIGA_FOLD_FINAL | GIGA_PLANES_FP32);
    if (precision < 0 || precision > 2 || (planes32 && precision != 1)) return -5;
    if (B == 0 || R == 0 || (head_mask & 15) == 0) return 0;
    if (!planes_nhwc || !lin || !packed || !workspace) return -1;
    if (workspace_bytes < giga_lattice_workspace_bytes(B, R, precision)) return -4;
    float* outs[NHEADS] = {qual, rot, width, occ};
    DecArgs a{};
    int rc = dec_args_heads(a, head_mask, outs, pack_offsets(), precision, fold);      // (-6 before anything is enqueued)
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = launch_lattice_resample(planes_nhwc, lin, workspace, B, R, precision, s, planes32);
    if (rc) return rc;
    a.planes = workspace; a.p = nullptr; a.blob = static_cast<const uint8_t*>(packed);
    a.B = B; a.N = R * R * R; a.P = (long long)B * a.N; a.post = post; a.lin = lin; a.R = R;
    return launch_decoder(a, precision, s, ev_start, ev_stop);
}

// ---------------------------------------------------------------------------------------------------------
// training path (fp32)
size_t giga_bwd_packed_bytes(void) { return bwd_packed_bytes(); }

int giga_pack_bwd_weights(const float* params_host, size_t n_params, int head_present, void* packed_host,
                          size_t packed_bytes_) {
    if (!params_host || !packed_host) return -1;
    return pack_bwd_host(params_host, n_params, head_present & 15, static_cast<uint8_t*>(packed_host), packed_bytes_);
}

int giga_pack_bwd_map(int head_present, int32_t* map_host, size_t nwords) {
    if (!map_host) return -1;
    return pack_bwd_map_host(head_present & 15, map_host, nwords);
}

static size_t train_dec_scratch_bytes(int B, int N, int M, int head_present) {
    const int ng = __builtin_popcount(head_present & 7), nt = (head_present >> 3) & 1;
    const size_t a = ng ? dec_bwd_scratch_floats((long long)B * N, ng) : 0;
    const size_t b = nt && M > 0 ? dec_bwd_scratch_floats((long long)B * M, 1) : 0;
    // bf16 decoder (GIGA_BF16_DECODER): the dc rows of the occupancy head + the partial gradient tiles of both calls (they are
    // reduced together at the end); far below the fp32 path's row arrays except for a handful of points
    const size_t c = (nt && M > 0 ? (size_t)B * M * 96 + dect_partial_floats((long long)B * M, 1) : 0) +
                     (ng ? dect_partial_floats((long long)B * N, ng) : 0);
    const size_t m = a + b;                          // (both: the occupancy call's weight gradients run beside the grasp call, giga_side.h)
    return align_up((m > c ? m : c) * sizeof(float), 256);
}

size_t giga_backward_workspace_bytes(int B, int N, int M, int head_present) {
    if (B <= 0) return 0;
    head_present &= 15;
    return align_up((size_t)3 * B * RES * RES * CD * sizeof(float), 256) + enc_bwd_workspace(B).total +
           train_dec_scratch_bytes(B, N, M, head_present);
}

int giga_backward_workspace_layout(int B, size_t* offsets) {
    if (B <= 0 || !offsets) return -1;
    const BwdWs g = enc_bwd_workspace(B);
    const size_t base = align_up((size_t)3 * B * RES * RES * CD * sizeof(float), 256);     // the plane gradients come first
    const size_t o[15] = {g.gA6, g.gA5, g.gC1, g.gA4, g.gA3, g.gC0, g.gS2, g.gA2, g.gQ1, g.gS1, g.gA1, g.gQ0, g.gS0, g.gA0, g.gP0};
    for (int i = 0; i < 15; ++i) offsets[i] = base + o[i];
    return 0;
}

int giga_backward(const float* tsdf, const void* packed, const void* bwd_packed, const void* enc_workspace_fwd,
                  const void* planes_nhwc, const float* p, const float* p_tsdf, const float* const* outs,
                  const float* const* douts, float* grads, size_t n_params, int head_present, int B, int N, int M,
                  void* workspace, size_t workspace_bytes, void* stream) {
    if (B <= 0) return 0;
    if (!tsdf || !packed || !bwd_packed || !enc_workspace_fwd || !planes_nhwc || !outs || !douts || !grads ||
        !workspace)
        return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    const bool detach_occ = (head_present & GIGA_DETACH_OCC) != 0;     // detach_tsdf, models/__init__.py:61-63
    const bool bf16_convs = (head_present & GIGA_BF16_CONVS) != 0;     // data-gradient convolutions on bf16 MFMA
    const bool bf16_dec = (head_present & GIGA_BF16_DECODER) != 0;     // decoder backward on the fused bf16 kernel
    const bool convin_mask = (head_present & GIGA_CONVIN_MASK_BWD) != 0;   // the forward kept conv_in's ReLU mask (GIGA_CONVIN_MASK)
    head_present &= 15;
    if (N < 0 || M < 0) return -1;
    if (n_params != param_offsets(head_present).total) return -2;
    for (int h = 0; h < NHEADS; ++h) {                                  // every head that will run needs out and dout
        const bool runs = (head_present >> h & 1) && (h < 3 ? N > 0 : (M > 0 && p_tsdf != nullptr));
        if (runs && (!outs[h] || !douts[h])) return -6;
    }
    if ((head_present & 7) && N > 0 && !p) return -1;                   // (every argument is checked before anything is enqueued)
    if (workspace_bytes < giga_backward_workspace_bytes(B, N, M, head_present)) return -4;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const size_t gp_bytes = align_up((size_t)3 * B * RES * RES * CD * sizeof(float), 256);
    float* gplanes = reinterpret_cast<float*>(ws);
    uint8_t* gws = ws + gp_bytes;
    float* scratch = reinterpret_cast<float*>(gws + enc_bwd_workspace(B).total);
    const uint8_t* blob = static_cast<const uint8_t*>(packed);
    const uint8_t* bblob = static_cast<const uint8_t*>(bwd_packed);
    const bool occ_runs = (head_present & 8) && M > 0 && p_tsdf;
    // The occupancy head with many queries per scene WRITES the plane gradients (plane_gather_kernel: a gather over binned points
    // instead of global atomics), so it runs first and nothing needs clearing; the grasp heads then add theirs with atomics.
    const bool occ_writes = occ_runs && !detach_occ && dec_bwd_writes_planes(1, B, M);
    if (!occ_writes && hipMemsetAsync(gplanes, 0, gp_bytes, s) != hipSuccess) return -10;
    if (hipMemsetAsync(grads, 0, n_params * sizeof(float), s) != hipSuccess) return -10;
    int rc = 0;
    // work that waits for ONE launch of the caller's stream only goes to the device's side stream (giga_side.h; GIGA_WGRAD_STREAM=0: none)
    SideScope side(s, [] { const char* e = getenv("GIGA_WGRAD_STREAM"); return !e || atoi(e) != 0; }());
    if (bf16_dec) {
        // one fused launch per call (recompute, gradient chain, weight gradients), ONE reduce for every head of the step
        DectPending pend{};
        float* sc = scratch;
        if (occ_runs) {
            float* dcbuf = occ_writes ? sc : nullptr;
            if (dcbuf) sc += (size_t)B * M * 96;
            rc |= launch_dect_backward(static_cast<const float*>(planes_nhwc), p_tsdf, blob, bblob, 8, outs, douts,
                                       detach_occ ? nullptr : gplanes, dcbuf, sc, B, M, s, &pend);
            sc += dect_partial_floats((long long)B * M, 1);
            if (dcbuf) rc |= launch_plane_gather(dcbuf, p_tsdf, gplanes, B, M, s);
        }
        if ((head_present & 7) && N > 0)
            rc |= launch_dect_backward(static_cast<const float*>(planes_nhwc), p, blob, bblob, head_present & 7, outs, douts,
                                       gplanes, nullptr, sc, B, N, s, &pend);
        // (on the caller's stream: moved to the side stream it delays the first weight gradients there, 894 -> 899 us per step)
        rc |= launch_dect_reduce(pend, grads, head_present, s);
    } else {
    float* sc = scratch;
    if (occ_runs) {
        rc |= launch_decoder_backward(static_cast<const float*>(planes_nhwc), p_tsdf, blob, bblob, 8, outs, douts,
                                      detach_occ ? nullptr : gplanes, grads, head_present, sc, B, M, s, occ_writes, &side);
        sc += dec_bwd_scratch_floats((long long)B * M, 1);       // (its weight gradients may still be reading their rows)
    }
    if ((head_present & 7) && N > 0) {
        rc |= launch_decoder_backward(static_cast<const float*>(planes_nhwc), p, blob, bblob, head_present & 7, outs,
                                      douts, gplanes, grads, head_present, sc, B, N, s, false, &side);
    }
    }
    rc |= launch_encoder_backward(tsdf, blob, bblob, static_cast<const uint8_t*>(enc_workspace_fwd), gplanes, gws,
                                  grads, head_present, B, s, bf16_convs, convin_mask, side);
    return rc;
}

int giga_decoder_point_grad(const void* planes_nhwc, const float* p, const void* packed, const void* bwd_packed,
                            int head_mask, const float* dqual, const float* drot, const float* dwidth, const float* dtsdf,
                            float* dp, float* out_qual, float* out_rot, float* out_width, float* out_tsdf,
                            int B, int N, int flags, void* stream) {
    if (head_mask <= 0 || (head_mask & ~15) != 0) return -1;
    if (B <= 0 || N <= 0) return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    if ((long long)B * N >= (1LL << 31)) return -1;         // split_scene's point index is exact below 2^31
    if (flags != 0) return -5;
    if (!planes_nhwc || !p || !packed || !bwd_packed || !dp) return -1;
    const float* douts[NHEADS] = {dqual, drot, dwidth, dtsdf};
    float* outs[NHEADS] = {out_qual, out_rot, out_width, out_tsdf};
    for (int h = 0; h < NHEADS; ++h)
        if ((head_mask >> h & 1) && !douts[h]) return -6;
    return launch_decoder_point_grad(static_cast<const float*>(planes_nhwc), p, static_cast<const uint8_t*>(packed),
                                     static_cast<const uint8_t*>(bwd_packed), head_mask, douts, outs, dp, B, N,
                                     static_cast<hipStream_t>(stream));
}

int giga_decoder_point_hess(const void* planes_nhwc, const float* p, const void* packed, const void* bwd_packed, float* logit,
                            float* dp, float* hess, int B, int N, void* stream) {
    if (B <= 0 || N <= 0) return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    if ((long long)B * N >= (1LL << 31)) return -1;         // split_scene's point index is exact below 2^31
    if (!planes_nhwc || !p || !packed || !bwd_packed || !logit || !dp || !hess) return -1;
    return launch_decoder_point_hess(static_cast<const float*>(planes_nhwc), p, static_cast<const uint8_t*>(packed),
                                     static_cast<const uint8_t*>(bwd_packed), logit, dp, hess, B, N,
                                     static_cast<hipStream_t>(stream));
}

// 3 F corner indices and 9 F gradient floats are indexed with int / 32-bit products of the face count
static bool refine_sizes_ok(int n_vertices, int n_faces) {
    return n_vertices >= 0 && n_faces >= 0 && n_vertices <= GIGA_REFINE_MAX_VERTICES && n_faces <= GIGA_REFINE_MAX_FACES;
}

int giga_refine_face_points(const float* vertices, const int* faces, const float* eps_in, float* eps, float* points,
                            int n_vertices, int n_faces, unsigned long long seed, int step, void* stream) {
    if (!refine_sizes_ok(n_vertices, n_faces) || step < 0) return -1;
    if (n_faces == 0) return 0;
    if (!vertices || !faces) return -1;
    if (!eps || !points) return -6;
    return launch_refine_face_points(vertices, faces, eps_in, eps, points, n_vertices, n_faces, seed, step,
                                     static_cast<hipStream_t>(stream));
}

int giga_refine_face_grad(const float* vertices, const int* faces, const float* eps, const float* logit, const float* dp,
                          const float* hess, double threshold, float* face_loss, float* face_grad, int n_vertices, int n_faces,
                          void* stream) {
    if (!refine_sizes_ok(n_vertices, n_faces) || !(threshold > 0.0 && threshold < 1.0)) return -1;
    if (n_faces == 0) return 0;
    if (!vertices || !faces || !eps || !logit || !dp || !hess) return -1;
    if (!face_loss || !face_grad) return -6;
    return launch_refine_face_grad(vertices, faces, eps, logit, dp, hess, threshold, face_loss, face_grad, n_vertices, n_faces,
                                   static_cast<hipStream_t>(stream));
}

int giga_refine_vertex_step(const float* face_grad, const int* corner_order, const int* vertex_offsets, float* vertices,
                            float* square_avg, float* grad, int n_vertices, int n_faces, void* stream) {
    if (!refine_sizes_ok(n_vertices, n_faces)) return -1;
    if (n_vertices == 0) return 0;
    if (!vertex_offsets || !vertices || !square_avg || (n_faces > 0 && (!face_grad || !corner_order))) return -1;
    if (!grad) return -6;
    return launch_refine_vertex_step(face_grad, corner_order, vertex_offsets, vertices, square_avg, grad, n_vertices, n_faces,
                                     static_cast<hipStream_t>(stream));
}

/* page-lock (and map for DMA) a host range the caller owns, e.g. a shared-memory batch ring written by reader processes */
int giga_host_register(void* ptr, size_t bytes) {
    if (!ptr || bytes == 0) return -1;
    return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? 0 : -10;
}
int giga_host_unregister(void* ptr) {
    if (!ptr) return -1;
    return hipHostUnregister(ptr) == hipSuccess ? 0 : -10;
}

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
    return launch_tsdf_scatter(voxel_index, voxel_value, scene_offsets, B, R, n_voxels, grid, static_cast<int*>(workspace),
                               static_cast<hipStream_t>(stream));
}

int giga_train_loss(const float* qual, const float* rot, const float* width, const float* occ_logits, const float* label,
                    const float* rot_targets, const float* width_target, const float* occ_target, int B, int M,
                    float* losses, float* scene_losses, void* stream) {
    if (B < 0 || M < 0) return -1;
    if (B == 0) return 0;
    if (!qual || !rot || !width || !label || !rot_targets || !width_target || !losses || !scene_losses) return -1;
    if (M > 0 && (!occ_logits || !occ_target)) return -1;
    return launch_train_loss(qual, rot, width, occ_logits, label, rot_targets, width_target, occ_target, B, M, losses,
                             scene_losses, static_cast<hipStream_t>(stream));
}

int giga_train_loss_metrics(const float* qual, const float* rot, const float* width, const float* occ_logits, const float* label,
                            const float* rot_targets, const float* width_target, const float* occ_target, int B, int M,
                            float* losses, float* scene_losses, void* acc, void* stream) {
    if (B < 0 || M < 0) return -1;
    if (!acc || (reinterpret_cast<uintptr_t>(acc) & 7)) return -1;
    if (B == 0) return 0;
    if (!qual || !rot || !width || !label || !rot_targets || !width_target || !losses || !scene_losses) return -1;
    if (M > 0 && (!occ_logits || !occ_target)) return -1;
    return launch_train_loss_metrics(qual, rot, width, occ_logits, label, rot_targets, width_target, occ_target, B, M, losses,
                                     scene_losses, acc, static_cast<hipStream_t>(stream));
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
    return launch_train_loss_backward(qual, rot, width, occ_logits, label, rot_targets, width_target, occ_target, grad_loss,
                                      B, M, dqual, drot, dwidth, docc, static_cast<hipStream_t>(stream));
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
    return launch_train_occ_loss_backward(occ_logits, occ_target, grad_loss, B, M, docc, static_cast<hipStream_t>(stream));
}

int giga_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                   double beta2, double eps, double weight_decay, int step, void* stream) {
    if (n == 0) return 0;
    if (!params || !grads || !exp_avg || !exp_avg_sq || step < 1) return -1;
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0)) return -1;
    // the kernel moves float4: all four buffers must be 16-byte aligned (whole torch allocations are; a view at an odd offset is not)
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(exp_avg) |
         reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15) return -1;
    return launch_adam_flat(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step,
                            static_cast<hipStream_t>(stream));
}

// ---- marching cubes (giga_mesh.hip) ----
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
    return mesh_workspace_bytes(B, nx, ny, nz);
}

int giga_mesh_count(const float* grids, int B, int nx, int ny, int nz, double iso, void* workspace, size_t workspace_bytes,
                    int32_t* counts, void* stream) {
    if (const int rc = mesh_shape_check(B, nx, ny, nz)) return rc;
    if (B == 0) return 0;
    if (!grids || !workspace || !counts || !(iso == iso)) return -1;
    if (workspace_bytes < giga_mesh_workspace_bytes(B, nx, ny, nz)) return -4;
    return launch_mesh_count(grids, B, nx, ny, nz, iso, static_cast<uint8_t*>(workspace), counts, static_cast<hipStream_t>(stream));
}

int giga_mesh_emit(const float* grids, int B, int nx, int ny, int nz, double iso, double box_size, const void* workspace,
                   size_t workspace_bytes, float* vertices, size_t cap_v, int32_t* triangles, size_t cap_t, int32_t* shortfall,
                   void* stream) {
    if (const int rc = mesh_shape_check(B, nx, ny, nz)) return rc;
    if (B == 0) return 0;
    if (!grids || !workspace || !(iso == iso) || !(box_size == box_size)) return -1;
    if ((cap_v > 0 && !vertices) || (cap_t > 0 && !triangles)) return -6;
    if (workspace_bytes < giga_mesh_workspace_bytes(B, nx, ny, nz)) return -4;
    return launch_mesh_emit(grids, B, nx, ny, nz, iso, box_size, static_cast<const uint8_t*>(workspace), vertices, cap_v, triangles,
                            cap_t, shortfall, static_cast<hipStream_t>(stream));
}

// ---- MISE (giga_mise.hip) ----
// 0 when the tree shape is supported, else the error code
static int mise_shape_check(int B, int res0, int depth) {
    if (B < 0 || res0 < 1 || depth < 1 || depth > 30) return -1;
    if (((long long)res0 << depth) + 1 > GIGA_MISE_MAX_N) return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    const long long N = ((long long)res0 << depth) + 1;
    if ((long long)B * N * N * N >= (1LL << 31)) return -1;                           // sample numbers are 32-bit
    return 0;
}

size_t giga_mise_workspace_bytes(int B, int resolution0, int depth) {
    if (B <= 0 || mise_shape_check(B, resolution0, depth) != 0) return 0;
    return mise_workspace_bytes(B, resolution0, depth);
}

int giga_mise_init(int B, int resolution0, int depth, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = mise_shape_check(B, resolution0, depth)) return rc;
    if (B == 0) return 0;
    if (!workspace) return -1;
    if (workspace_bytes < giga_mise_workspace_bytes(B, resolution0, depth)) return -4;
    return launch_mise_init(B, resolution0, depth, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

int giga_mise_count(int B, int resolution0, int depth, void* workspace, size_t workspace_bytes, int32_t* counts, void* stream) {
    if (const int rc = mise_shape_check(B, resolution0, depth)) return rc;
    if (B == 0) return 0;
    if (!workspace || !counts) return -1;
    if (workspace_bytes < giga_mise_workspace_bytes(B, resolution0, depth)) return -4;
    return launch_mise_count(B, resolution0, depth, static_cast<uint8_t*>(workspace), counts, static_cast<hipStream_t>(stream));
}

int giga_mise_emit(int B, int resolution0, int depth, const void* workspace, size_t workspace_bytes, int32_t* query, size_t cap,
                   int32_t* shortfall, const float* lin, float* points, void* stream) {
    if (const int rc = mise_shape_check(B, resolution0, depth)) return rc;
    if (B == 0) return 0;
    if (!workspace || (points && !lin)) return -1;
    if (cap > 0 && !query) return -6;
    if ((unsigned long long)B * cap >= (1ull << 31)) return -1;
    if (workspace_bytes < giga_mise_workspace_bytes(B, resolution0, depth)) return -4;
    return launch_mise_emit(B, resolution0, depth, static_cast<const uint8_t*>(workspace), query, cap, shortfall, lin, points,
                            static_cast<hipStream_t>(stream));
}

int giga_mise_update(const float* values, const int32_t* query, size_t cap, int B, int resolution0, int depth, double threshold,
                     void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = mise_shape_check(B, resolution0, depth)) return rc;
    if (!(threshold == threshold)) return -1;
    if (B == 0) return 0;
    if (!workspace || (cap > 0 && (!values || !query))) return -1;
    if ((unsigned long long)B * cap >= (1ull << 31)) return -1;
    if (workspace_bytes < giga_mise_workspace_bytes(B, resolution0, depth)) return -4;
    return launch_mise_update(values, query, cap, B, resolution0, depth, threshold, static_cast<uint8_t*>(workspace),
                              static_cast<hipStream_t>(stream));
}

int giga_mise_to_dense(int B, int resolution0, int depth, const void* workspace, size_t workspace_bytes, float* grid, void* stream) {
    if (const int rc = mise_shape_check(B, resolution0, depth)) return rc;
    if (B == 0) return 0;
    if (!workspace || !grid) return -1;
    if (workspace_bytes < giga_mise_workspace_bytes(B, resolution0, depth)) return -4;
    return launch_mise_to_dense(B, resolution0, depth, static_cast<const uint8_t*>(workspace), grid, static_cast<hipStream_t>(stream));
}

// ---- mesh evaluation (giga_eval.hip) ----
// offsets of a ragged batch (host array of B + 1 entries): starts at 0 and never decreases
static bool ragged_ok(const int32_t* offs, int B) {
    if (!offs || offs[0] != 0) return false;
    for (int b = 0; b < B; ++b)
        if (offs[b + 1] < offs[b]) return false;
    return true;
}
static int ragged_batch_check(int B) { return B < 0 ? -1 : (B > GIGA_MAX_SCENES ? -7 : 0); }

// a ragged batch of B meshes: both offset arrays are well formed, and data that is not empty has a pointer
static bool mesh_batch_check(const int32_t* vertex_offsets, const int32_t* triangle_offsets, int B, const void* vertices,
                             const void* triangles) {
    if (!ragged_ok(vertex_offsets, B) || !ragged_ok(triangle_offsets, B)) return false;
    return (vertex_offsets[B] == 0 || vertices) && (triangle_offsets[B] == 0 || triangles);
}

static bool finite_f64(double x) { return x - x == 0.0; }

// n cameras (extrinsics [n][16], intrinsics [n][4] = fx, fy, cx, cy): every number finite, no focal length zero
static bool camera_check(int n, const double* extrinsics, const double* intrinsics) {
    if (n > 0 && (!extrinsics || !intrinsics)) return false;
    for (size_t i = 0; i < (size_t)n * 16; ++i)
        if (!finite_f64(extrinsics[i])) return false;
    for (size_t i = 0; i < (size_t)n * 4; ++i)
        if (!finite_f64(intrinsics[i])) return false;
    for (int v = 0; v < n; ++v)
        if (intrinsics[4 * (size_t)v] == 0.0 || intrinsics[4 * (size_t)v + 1] == 0.0) return false;
    return true;
}

// ---- mesh simplification (giga_simplify.hip) ----
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
    return simplify_workspace_bytes(B, n_vertices, n_triangles, simplify_ref_total(B, n_triangles, ref_extra));
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

size_t giga_nn_query_workspace_bytes(int B, int n_src) {
    if (B <= 0 || B > GIGA_MAX_SCENES || n_src < 0) return 0;
    return nn_workspace_bytes(B, n_src);
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
    return sample_workspace_bytes(B, n_triangles);
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
    return contains_workspace_bytes(B, n_triangles, n_points);
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

// ---- mesh against mesh (giga_collide.hip) ----
size_t giga_mesh_collide_workspace_bytes(int M, int P) {
    if (M <= 0 || M > GIGA_MAX_SCENES || P < 0) return 0;
    return collide_workspace_bytes(M, P);
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

// ---- geometry scoring (giga_geometry.hip) ----
size_t giga_roi_points_workspace_bytes(int n_grasps) {
    if (n_grasps <= 0) return 0;
    return roi_workspace_bytes(n_grasps);
}

int giga_roi_points(const double* grasps, const int32_t* point_offsets, const int32_t* grasp_scene, const int32_t* grasp_first,
                    int n_grasps, uint64_t seed, double finger_depth, double roi_scale, double size, double* world,
                    float* normalised, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_grasps < 0) return -1;
    if (!finite_f64(finger_depth) || !finite_f64(roi_scale) || !finite_f64(size) || size == 0.0) return -1;
    if (n_grasps == 0) return 0;
    if (!ragged_ok(point_offsets, n_grasps)) return -1;
    if (point_offsets[n_grasps] == 0) return 0;
    if (!grasps || !grasp_scene || !grasp_first || !workspace) return -1;
    for (int g = 0; g < n_grasps; ++g) {
        // (the point index inside the scene is one 32-bit counter word)
        if (grasp_scene[g] < 0 || grasp_first[g] < 0 ||
            (long long)grasp_first[g] + (point_offsets[g + 1] - point_offsets[g]) > 0x7fffffffLL)
            return -1;
        for (int q = 0; q < 13; ++q)
            if (!finite_f64(grasps[13 * (size_t)g + q])) return -1;
    }
    if (!world || !normalised) return -6;
    if (workspace_bytes < giga_roi_points_workspace_bytes(n_grasps)) return -4;
    return launch_roi_points(grasps, point_offsets, grasp_scene, grasp_first, n_grasps, seed, finger_depth * roi_scale, size, world,
                             normalised, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

size_t giga_occ_confusion_workspace_bytes(int B) {
    if (B <= 0 || B > GIGA_MAX_SCENES) return 0;
    return confusion_workspace_bytes(B);
}

int giga_occ_confusion(const float* logits, const uint8_t* pred, double logit_threshold, const uint8_t* target,
                       const int32_t* offsets, int B, uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = ragged_batch_check(B)) return rc;
    if (B == 0) return 0;
    if (!ragged_ok(offsets, B)) return -1;
    if ((logits != nullptr) == (pred != nullptr) && offsets[B] > 0) return -1;         // exactly one form of the prediction
    if ((offsets[B] > 0 && !target) || !workspace) return -1;
    if (logits && !(logit_threshold == logit_threshold)) return -1;
    if (!counts) return -6;
    if (workspace_bytes < giga_occ_confusion_workspace_bytes(B)) return -4;
    return launch_occ_confusion(logits, pred, logit_threshold, target, offsets, B, reinterpret_cast<unsigned long long*>(counts),
                                static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

// ---- depth fusion (giga_tsdf.hip) ----
static int tsdf_volume_check(int B, int R) {
    if (B < 0 || R < 2 || R > GIGA_TSDF_MAX_R) return -1;
    if (B > GIGA_MAX_SCENES) return -7;
    return 0;
}

size_t giga_tsdf_integrate_workspace_bytes(int B, int n_views) {
    if (B <= 0 || B > GIGA_MAX_SCENES || n_views < 0) return 0;
    return tsdf_integrate_workspace_bytes(B, n_views);
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
    return tsdf_cloud_workspace_bytes(B, R);
}

int giga_tsdf_cloud_count(const float* tsdf, const float* weight, int B, int R, void* workspace, size_t workspace_bytes,
                          int32_t* counts, void* stream) {
    if (const int rc = tsdf_volume_check(B, R)) return rc;
    if (B == 0) return 0;
    if (!tsdf || !weight || !workspace || !counts) return -1;
    if (workspace_bytes < giga_tsdf_cloud_workspace_bytes(B, R)) return -4;
    return launch_tsdf_cloud_count(tsdf, weight, B, R, static_cast<uint8_t*>(workspace), counts, static_cast<hipStream_t>(stream));
}

int giga_tsdf_cloud_emit(const float* tsdf, const float* weight, int B, int R, double length, const void* workspace,
                         size_t workspace_bytes, float* points, size_t cap, int32_t* shortfall, void* stream) {
    if (const int rc = tsdf_volume_check(B, R)) return rc;
    if (!finite_f64(length) || !(length > 0.0)) return -1;
    if (B == 0) return 0;
    if (!tsdf || !weight || !workspace) return -1;
    if (cap > 0 && !points) return -6;
    if (workspace_bytes < giga_tsdf_cloud_workspace_bytes(B, R)) return -4;
    return launch_tsdf_cloud_emit(tsdf, weight, B, R, length, static_cast<const uint8_t*>(workspace), points, cap, shortfall,
                                  static_cast<hipStream_t>(stream));
}

// ---- depth rendering (giga_render.hip) ----
size_t giga_depth_render_workspace_bytes(int B, int n_views, int n_vertices, int n_triangles) {
    if (B <= 0 || B > GIGA_MAX_SCENES || n_views < 0 || n_vertices < 0 || n_triangles < 0) return 0;
    return depth_render_workspace_bytes(B, n_views);
}

int giga_depth_render(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                      const int32_t* view_offsets, const double* extrinsics, const double* intrinsics, int B, int W, int H, double near,
                      double far, double pixel_offset, float* depth, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = ragged_batch_check(B)) return rc;
    if (W < 1 || H < 1 || W > GIGA_RENDER_MAX_IMAGE || H > GIGA_RENDER_MAX_IMAGE) return -1;
    if (!finite_f64(near) || !finite_f64(far) || !(near > 0.0) || !(far > near) || !finite_f64(pixel_offset)) return -1;
    if (B == 0) return 0;
    if (!mesh_batch_check(vertex_offsets, triangle_offsets, B, vertices, triangles) || !ragged_ok(view_offsets, B)) return -1;
    const int n = view_offsets[B];
    if ((long long)n * W * H >= (1LL << 31)) return -1;
    if (n == 0) return 0;
    if (!camera_check(n, extrinsics, intrinsics) || !workspace) return -1;
    if (!depth) return -6;
    if (workspace_bytes < giga_depth_render_workspace_bytes(B, n, vertex_offsets[B], triangle_offsets[B])) return -4;
    return launch_depth_render(vertices, vertex_offsets, triangles, triangle_offsets, view_offsets, extrinsics, intrinsics, B, W, H, near,
                               far, pixel_offset, depth, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

// ---- grasp affordance of a scene mesh (giga_affordance.hip) ----
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
    return affordance_workspace_bytes(B, R);
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

// ---- depth noise (giga_noise.hip) ----
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

// ---- training batches from a resident set (giga_batch.hip) ----
// everything about the set that can be checked on the host; `all`: giga_batch_assemble reads every array, giga_batch_draw the tables
// behind the file sizes only
static int batch_set_check(const GigaBatchSet* set, bool all) {
    if (!set) return -1;
    if (set->n_scenes < 0 || set->n_rows < 0 || set->n_files < 0 || set->n_points < 0) return -1;
    if (!set->row_scene || !set->scene_files || !set->file_points) return -1;
    if (all) {
        if (!set->grids || !set->row_pos || !set->row_quat || !set->row_rotations || !set->row_width || !set->row_label ||
            !set->points || !set->occ)
            return -1;
        if (set->point_dtype != GIGA_BATCH_POINTS_F32 && set->point_dtype != GIGA_BATCH_POINTS_F16) return -1;
        if (!finite_f64(set->size) || !(set->size > 0.0)) return -1;
        if (reinterpret_cast<uintptr_t>(set->grids) % 16 != 0) return -1;
    }
    if (set->scene_files_host) {
        const int32_t* f = set->scene_files_host;
        if (f[0] != 0 || f[set->n_scenes] != set->n_files) return -1;
        for (int i = 0; i < set->n_scenes; ++i)
            if (f[i + 1] < f[i]) return -1;
    }
    if (set->file_points_host) {
        const int64_t* p = set->file_points_host;
        if (p[0] != 0 || p[set->n_files] != set->n_points) return -1;
        for (int i = 0; i < set->n_files; ++i)
            if (p[i + 1] < p[i] || p[i + 1] - p[i] >= (1LL << 31)) return -1;
    }
    return 0;
}

static bool batch_shape_ok(int B, int M) {
    return B >= 0 && M >= 0 && B <= GIGA_BATCH_MAX_ITEMS && (long long)B * M < (1LL << 31);
}

int giga_batch_draw(const GigaBatchSet* set, const int32_t* ordinals, const int32_t* rows, int B, int M, int epoch,
                    unsigned long long seed, int32_t* quarter, double* u, int32_t* file, int32_t* index, void* stream) {
    if (!batch_shape_ok(B, M) || epoch < 0) return -1;
    if (const int rc = batch_set_check(set, false)) return rc;
    if (B == 0) return 0;
    if (!ordinals || !rows) return -1;
    if (!quarter || !u || !file || (M > 0 && !index)) return -6;
    return launch_batch_draw(*set, ordinals, rows, B, M, epoch, seed, quarter, u, file, index, static_cast<hipStream_t>(stream));
}

int giga_batch_assemble(const GigaBatchSet* set, const int32_t* rows, const int32_t* quarter, const double* u, const int32_t* file,
                        const int32_t* index, int B, int M, int augment, float* x, float* pos, float* pos_occ, float* label,
                        float* rotations, float* width, float* occ, void* stream) {
    if (!batch_shape_ok(B, M)) return -1;
    if (const int rc = batch_set_check(set, true)) return rc;
    if (B == 0) return 0;
    if (!rows || !file || (M > 0 && !index) || (augment && (!quarter || !u))) return -1;
    if (!x || !pos || !label || !rotations || !width || (M > 0 && (!pos_occ || !occ))) return -6;
    if (reinterpret_cast<uintptr_t>(x) % 16 != 0) return -1;
    return launch_batch_assemble(*set, rows, quarter, u, file, index, B, M, augment, x, pos, pos_occ, label, rotations, width, occ,
                                 static_cast<hipStream_t>(stream));
}

}  // extern "C"
