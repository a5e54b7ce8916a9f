/* giga_hip.h -- C ABI of the MI355X-native GIGA hot path (libgiga_hip.so).
 *
 * The reference (UT-Austin-RPL/GIGA) has no FFI layer: the boundary it exposes for this path is the
 * nn.Module surface consumed by scripts/train_giga.py:204 and src/vgn/detection_implicit.py:107.
 * `giga_amd/` keeps that Python surface (same class names, kwargs, tensor layouts and state-dict
 * keys) and calls the functions below underneath; each entry point cites the reference code it
 * replaces (paths relative to /root/reference/src/vgn).  See INTEGRATION.md for the binding.
 *
 * Conventions
 *   - plain pointers and sizes only; every device buffer is owned by the caller (PyTorch);
 *     the library never allocates device memory and is re-entrant per (stream, workspace).  Its only
 *     process-wide mutable state is bookkeeping, never read by the arithmetic: the launch counter
 *     (giga_launch_count), the per-kernel record of raised dynamic-LDS limits, and per device the
 *     completion events of the streams' last persistent U-Net launches (see GIGA_PERSIST_UNET);
 *   - every launch is asynchronous on the caller's HIP stream `stream` (a hipStream_t);
 *   - return value 0 = success, negative = error (giga_strerror); nothing throws across the ABI;
 *   - at most GIGA_MAX_SCENES scenes per encoder / training call (the convolution kernels address activations with
 *     24-bit pixel indices and 32-bit byte offsets); larger batches return -7, split them;
 *   - `precision`: 0 = exact fp32 (v_mfma_f32_32x32x2_f32, bitwise fp32 fma chains),
 *                  1 = f16 operands / fp32 accumulate (v_mfma_f32_32x32x16_f16);
 *                  2 = f16x3 split operands / fp32 accumulate: every operand is the pair hi = f16(v), lo = f16(v - hi)
 *                      and every product W_lo*x_hi + W_hi*x_lo + W_hi*x_hi on the f16 MFMA (~22-bit operands, results
 *                      within 1e-5 of the fp32 path).  Decoder entry points only change arithmetic; planes are fp32
 *                      (as for precision 0); the encoder runs its convolutions (conv_in and the U-Net) in the same split
 *                      arithmetic.  Range: the split carries an operand to 2^-22 relative for 2^-3 <= |v| < 65520; below
 *                      2^-3 lo is subnormal and the error is 2^-25 absolute; from 65520 up hi = inf.  Measured on He-uniform
 *                      weights (planes of range ~3 at TSDF scale 1): planes within 3.5e-5 of their range against float64 for
 *                      TSDF inputs scaled by 2^-8 .. 2^14, decoders for planes of range ~6 scaled by 2^-10 .. 2^12; below,
 *                      the error doubles per halving of the scale.  Precisions 1 and 2: an activation past the f16 range
 *                      (65504) gives NaN / inf outputs, never a finite wrong value (the f16-class ReLUs and max-pools
 *                      propagate NaN; a qual logit of +-inf gives a NaN quality);
 *                  3 = bf16 operands / fp32 accumulate, fp32 activations and planes in memory: the forward of the bf16 training
 *                      step.  Encoder entry points: the U-Net convolutions (fp32 conv_in; see GIGA_BF16_CONVS); giga_decoder_forward:
 *                      every linear layer of the heads (see GIGA_BF16_DECODER; not with GIGA_FOLD_FINAL, not the lattice entry point);
 *   - "NHWC planes": one buffer [3 (xz,xy,yz)][B][40 (H)][40 (W)][32 (C)] of float (precision 0 and 2) or
 *     _Float16 (precision 1).  H/W follow the reference's plane indexing (ConvONets/common.py:246-251,
 *     303-318): xz -> (H=z, W=x), xy -> (H=y, W=x), yz -> (H=z, W=y).
 */
#ifndef GIGA_HIP_H_
#define GIGA_HIP_H_

#define GIGA_MAX_SCENES 3072

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GIGA_ABI_VERSION 3   /* 3: the forward blob grew (Winograd-domain images of the fp32 3x3 layers, round 6); 2: bf16 decoder images: repack */

#define GIGA_HEAD_QUAL 1   /* decoder_qual  (out_dim 1, sigmoid epilogue)     */
#define GIGA_HEAD_ROT 2    /* decoder_rot   (out_dim 4, L2-normalise epilogue) */
#define GIGA_HEAD_WIDTH 4  /* decoder_width (out_dim 1)                        */
#define GIGA_HEAD_TSDF 8   /* decoder_tsdf  (out_dim 1, raw logits)            */

int giga_abi_version(void);
const char* giga_strerror(int code);

/* Number of fp32 parameters expected for a head set (bitmask of GIGA_HEAD_*): the reference
 * state-dict flattened in its own key order (networks.py:21-35 load_network / state-dict keys of
 * conv_onet/models/__init__.py:15-40).  giga: 581863 for all four heads. */
size_t giga_param_count(int head_present);

/* Size of the packed-weight blob produced by giga_pack_weights. */
size_t giga_packed_bytes(void);

/* HOST function: repack the flat fp32 parameters (host pointer) into MFMA operand fragments
 * (host pointer, giga_packed_bytes() bytes).  The caller uploads the blob to the device.
 * Replaces the weight ownership of nn.Module.load_state_dict (networks.py:33-34). */
int giga_pack_weights(const float* params_host, size_t n_params, int head_present,
                      void* packed_host, size_t packed_bytes);

/* The blob layout belongs to the ABI version: new images are appended and slot orders change between versions, and the compute entry
 * points take no blob size -- a blob packed by another version would be read at the wrong offsets, silently.  Blobs are not
 * portable across versions: REPACK from the parameters after an upgrade.  Both packers stamp the last 256 bytes of their blob (magic,
 * ABI version, size); giga_packed_check validates a HOST copy (`backward` != 0: a giga_pack_bwd_weights blob) before it is uploaded:
 * 0, or -8 for a foreign / truncated / stale blob.  (A blob rebuilt on the device by giga_repack_device carries no stamp.) */
int giga_packed_check(const void* packed_host, size_t bytes, int backward);

/* Training support (scripts/train_giga.py:198-211: weights change every optimizer step): the fp32
 * words of the blob are pure gathers of single parameters.  giga_pack_map fills a HOST int32 map with one
 * entry per 4-byte blob word (>= 0 parameter index, -1 constant zero, -2 not an fp32 word);
 * giga_repack_device rewrites the fp32 words of a DEVICE blob from a DEVICE flat parameter buffer
 * (asynchronous on `stream`; f16 fragments are left untouched). nwords = giga_packed_bytes() / 4. */
int giga_pack_map(int head_present, int32_t* map_host, size_t nwords);
int giga_repack_device(const float* params_dev, const int32_t* map_dev, void* packed_dev, size_t nwords,
                       void* stream);
/* the forward and the backward blob in ONE launch (the training step rebuilds both every step) */
int giga_repack_device2(const float* params_dev, const int32_t* map_fwd_dev, void* packed_dev, size_t nwords_fwd,
                        const int32_t* map_bwd_dev, void* bwd_packed_dev, size_t nwords_bwd, void* stream);

/* Scratch bytes giga_encoder_forward needs for a batch of B scenes. */
size_t giga_encoder_workspace_bytes(int B, int precision);

/* Introspection for tests: byte offsets of the 17 intermediate activations inside the encoder
 * workspace, in order P0 (projected planes, U-Net input) A0 S0 Q0 A1 S1 Q1 A2 S2 U0 A3 A4 U1 A5 A6
 * YZ XZ (csrc/giga_enc_plan.h: enc_workspace).  All NHWC [3B][H][W][C] in the precision's element type
 * (YZ/XZ: fp32 partial sums).  offsets must have room for 17 entries. */
int giga_encoder_workspace_layout(int B, int precision, size_t* offsets);

/* LocalVoxelEncoder.forward (encoder/voxels.py:89-121) + UNet.forward (encoder/unet.py:225-239):
 * tsdf [B][40][40][40] fp32  ->  feature planes.
 *   planes_nhwc : NHWC planes in the precision's element type (consumed by giga_decoder_forward)
 *   planes_nchw : optional (may be NULL) fp32 [3][B][32][40][40], i.e. the reference's
 *                 {'xz','xy','yz'} dict of (B,32,40,40) tensors stacked. */
int giga_encoder_forward(const float* tsdf, const void* packed, void* planes_nhwc, float* planes_nchw,
                         int B, int precision, void* workspace, size_t workspace_bytes, void* stream);

/* Repack reference-layout planes (three fp32 (B,32,40,40) tensors) into NHWC planes; used when
 * LocalDecoder.forward(p, c_plane) (conv_onet/models/decoder.py:133) is handed foreign planes. */
int giga_planes_pack(const float* xz, const float* xy, const float* yz, void* planes_nhwc, int B,
                     int precision, void* stream);
/* Inverse: NHWC planes -> fp32 [3][B][32][40][40]. */
int giga_planes_unpack(const void* planes_nhwc, float* planes_nchw, int B, int precision, void* stream);

/* Fused LocalDecoder.forward for every head in `head_mask` (decoder.py:133-176; ResnetBlockFC
 * layers.py:39-47) over p [B][N][3] fp32 in [-0.5,0.5]^3 (any value is clamped like
 * common.py:238-261).  Point g uses the planes of scene g / N.
 *   qual [B*N], rot [B*N][4], width [B*N], occ [B*N]; a pointer may be NULL iff its head is not
 *   in head_mask.
 *   post != 0 applies the epilogues of ConvolutionalOccupancyNetwork.decode
 *   (conv_onet/models/__init__.py:111-124): sigmoid(qual), F.normalize(rot, dim=2). */
int giga_decoder_forward(const void* planes_nhwc, const float* p, const void* packed, int head_mask,
                         float* qual, float* rot, float* width, float* occ, int B, int N,
                         int precision, int post, void* stream);

/* GIGA_FOLD_FINAL, OR-ed into `precision` of giga_encoder_forward* AND of the giga_decoder_forward* call that consumes its
 * planes: the encoder stops before its last layer, conv_final (a 1x1 convolution without activation, encoder/unet.py:238),
 * and the decoder uses head images in which that layer is folded into fc_c -- bilinear sampling (decoder.py:117-122)
 * commutes with a per-pixel linear map, so fc_c(sample(Wf x + bf)) = (Wc blockdiag(Wf)) sample(x) + (bc + Wc bf).  Same
 * outputs (fp32 rounding-level differences), one layer less.  planes_nchw must be NULL with this flag: the planes it
 * produces are NOT LocalVoxelEncoder's return value and are only meaningful to a decoder call carrying the flag. */
#define GIGA_FOLD_FINAL 16
/* How the twelve (thirteen) U-Net layers are launched.  DEFAULT: ONE persistent launch in which groups of 8 workgroups, each
 * group inside one XCD, walk their share of the 3 * B plane images through all layers with a barrier among those 8 only
 * (csrc/giga_encoder.hip::unet_mega_kernel) -- for every batch size in precisions 1 and 2, from 8 scenes up in precisions 0
 * and 3.  Same results as one launch per layer: bit for bit in the f16-class modes, to fp32 rounding (<= 2e-6 relative) in
 * precision 0, where the summation order of a layer's ragged last round follows the work distribution.  A layer boundary then
 * costs a 1-us barrier instead of a launch: the whole encoder takes 75 instead of 94 us for one scene in precision 1 (the
 * planner of detection_implicit.py:99-113 runs one scene at a time), 130 instead of 150 us at 32 scenes, 361 instead of 378 in
 * precision 0.  The workgroups of a group find each other by ticket among the workgroups already resident on their XCD, so
 * such launches may be in flight on several streams of one device without waiting on each other's CUs -- UP TO FOUR of them: a
 * launch can hold one unfilled group (<= 7 workgroups) per XCD, an XCD has 32 slots for these workgroups, and 5 x 7 > 32 could
 * park every slot in groups that never fill.  The library enforces the bound inside a process: per device it tracks the
 * completion event of every stream's last persistent launch, and a call on a stream that would be the fifth with an unfinished one
 * takes one launch per layer instead (same results; launches queued on one stream run one after the other and count once).  It cannot see OTHER PROCESSES that share the device, nor replays of captured hipGraphs on several streams at
 * once: keep those to four concurrent encoder calls, or pass GIGA_LAYERWISE_UNET.  The kernel also assumes that every XCD
 * receives an eighth of the grid (no CU mask on the stream, a whole MI355X: 256 CUs -- checked -- in one partition).  A barrier
 * that is not released within 20 s of wall clock (s_memrealtime) traps instead of returning stale data or hanging the device.
 *   GIGA_LAYERWISE_UNET, OR-ed into `precision` of giga_encoder_forward*: one launch per layer (A/B comparisons).
 *   GIGA_PERSIST_UNET: the persistent launch also where the default keeps per-layer launches (precisions 0 / 3 below 8 scenes). */
#define GIGA_PERSIST_UNET 32
#define GIGA_LAYERWISE_UNET 64
/* Which convolution kernels run the U-Net of the f16-class precisions (1 and 2):
 *   conv32 (csrc/giga_conv32.h; round 4; the default up to 16 scenes): v_mfma_f32_32x32x16, a member of a group owns a band of ROWS of the
 *     group's images -- staged once per layer into LDS -- and one LDS-DMA copy of its weights; register tiles fed by conflict-free
 *     ds_read_b128 at `base + immediate`, no VALU in the MFMA loop; at up to two images per group the same-resolution layer
 *     pairs (0,1), (2,3), (10,11) of plain f16 run without the group barrier between them (the second layer reads the first one's
 *     output from LDS; one halo row recomputed per side; bit-identical to the unfused form).
 *   conv16 (csrc/giga_conv16.h): 16x16x32, wave-private haloed patches; the only kernels of precisions 0 and 3.
 * Same arithmetic per layer (f16 / f16x3 operands, fp32 accumulation, outputs within one rounding of each other), same launch
 * forms, same workspace.  Default: conv32 up to 16 scenes (48 images), conv16 beyond.  Measured: conv32's
 * encoder is 3-9 % faster up to 32 scenes, but with every CU busy (from ~24 scenes) the chip holds a 3-5 % lower shader clock while
 * and after the conv32 launch runs, which costs sustained large-batch steps more than the kernel gains.  A scene's low-order bits
 * therefore depend on whether its batch has more than 16 scenes -- force one kernel where that matters:
 *   GIGA_CONV32_UNET / GIGA_CONV16_UNET, OR-ed into `precision` (1 or 2) of giga_encoder_forward*: force the one or the other for
 *   this call. */
#define GIGA_CONV32_UNET 128
#define GIGA_CONV16_UNET 256
/* GIGA_CONVIN_MASK, OR-ed into `precision` (0 or 3) of giga_encoder_forward*: a TRAINING forward -- conv_in also stores its ReLU mask, one
 * bit per pre-activation z set when !(z > 0) (10 MB at 32 scenes, in the encoder workspace), and giga_backward called with GIGA_CONVIN_MASK_BWD on that workspace
 * takes the ReLU mask of conv_in from them instead of recomputing the convolution (8 instead of 15 MFMAs per unit). */
#define GIGA_CONVIN_MASK 512
/* The stride-1 3x3 layers of the U-Net in precision 0 (exact fp32; encoder/unet.py:14-23) run as Winograd F(2x2, 3x3) on the fp32
 * MFMA by default (csrc/giga_wino.h: 16 instead of 36 multiplies per 2x2 outputs; transforms in registers, Winograd-domain weights
 * from the packed blob).  fp32 Winograd is not the direct form's bitwise fma chain: planes differ from it by a few 1e-6 relative
 * (the suite holds both to 1e-4 of the oracle).  GIGA_DIRECT_CONV, OR-ed into `precision` (0) of giga_encoder_forward*, keeps the
 * direct convolutions for this call; the environment variable GIGA_WINOGRAD=0 does so for every call made while it is set (a layer bit
 * mask otherwise; read on every call).  A blob rebuilt by giga_repack_device (the training path) needs giga_derive_winograd before such a forward:
 * giga_repack_device gathers parameters, and the Winograd image is not a gather. */
#define GIGA_DIRECT_CONV 1024
/* The launch plan giga_encoder_forward* would use for B scenes and this `precision` word (the precision 0..3 with the flags above)
 * on a device of `cus` compute units (<= 0: assume 256, a whole MI355X), decided NOW: the tuning variables GIGA_WINOGRAD (the layer
 * mask of the Winograd stages of precision 0) and GIGA_C32_FUSE (0 / 1: the fused pairs of the persistent conv32 launch off / on) are
 * read on every call, as a launch reads them.  probe_stage: the stage a giga_encoder_forward_probe call would bracket (-1: none; a
 * probed layer, stages 2..14, gets its own launch).  Host only: no device is touched.  The plan assumes that the device has room for
 * one more persistent launch (see GIGA_PERSIST_UNET); GIGA_ENCODER_PLAN_NO_SLOT, OR-ed into the word of THIS function only, asks for
 * the plan of a call that finds four others in flight.  Error codes as giga_encoder_forward_probe's for the same arguments: -1
 * (B < 0, NULL plan_words), -7 (B > GIGA_MAX_SCENES), -5 (precision, GIGA_CONVIN_MASK with precision 1 / 2); B == 0: all words zero.
 * plan_words[GIGA_ENCODER_PLAN_WORDS], in order (csrc/giga_enc_plan.h, struct EncPlan):
 *   nimg (3 B), nlayers (12 with GIGA_FOLD_FINAL, else 13);
 *   conv_in: nxp (x-parts), ci_f16 (f16 operand image), ci_lo (f16x3 split operands), ci_mask (stores the ReLU mask), ci_sxw (slices
 *   per wave), ci_nw (waves), ci_grid_x, ci_grid_y, ci_grid_z, ci_block;  plane_finalize: fin_grid, fin_block;
 *   form (GIGA_ENC_FORM_*), persistent, conv32, fused, wino_mask (bit l: layer l is a Winograd stage / an up-GEMM), groups (of 8
 *   workgroups), grid, block (the persistent launch; 0: one launch per layer), layer_kernel[13] (GIGA_ENC_LAYER_*; 0: not launched),
 *   launches (kernel launches of the call), path (the GIGA_PATH_* word giga_encoder_last_path reports after the call). */
#define GIGA_ENCODER_PLAN_WORDS 37
#define GIGA_ENCODER_PLAN_NO_SLOT 2048
#define GIGA_ENC_FORM_LAYERS_CONV16 1    /* one launch per layer: conv16_kernel (precision 0: wino_kernel / up_kernel where wino_mask says) */
#define GIGA_ENC_FORM_LAYERS_CONV32 2    /* one launch per layer: conv32_kernel */
#define GIGA_ENC_FORM_PERSIST_CONV16 3   /* unet_mega_kernel<T, MATH, false> */
#define GIGA_ENC_FORM_PERSIST_WINO 4     /* unet_mega_kernel<float, MATH_NATIVE, true> */
#define GIGA_ENC_FORM_PERSIST_CONV32 5   /* unet32_mega_kernel<MODE, fused> */
#define GIGA_ENC_LAYER_CONV16 1
#define GIGA_ENC_LAYER_CONV32 2
#define GIGA_ENC_LAYER_WINO 3
#define GIGA_ENC_LAYER_UP 4
int giga_encoder_plan(int B, int precision_word, int cus, int probe_stage, int32_t* plan_words);

/* Inference fast path for the FIXED QUERY LATTICE of VGNImplicit (detection_implicit.py:28-31,107):
 * the R^3 points meshgrid(lin, lin, lin, 'ij') with z fastest, shared by all B scenes.  Each plane is
 * sampled at only R*R distinct positions, so the planes are first resampled at the lattice coordinates
 * (same arithmetic as sample_plane_feature, decoder.py:117-122) into `workspace`
 * (giga_lattice_workspace_bytes) and the fused decoder then reads three pixels per point instead of
 * twelve bilinear taps.  lin: device pointer to the R lattice coordinates (R <= 64).
 * Outputs as giga_decoder_forward with N = R^3; ev_start/ev_stop (may be NULL) bracket the decoder launch. */
/* GIGA_PLANES_FP32, OR-ed into `precision` 1 of giga_decoder_forward_lattice: planes_nhwc are FP32 planes (an encoder at precision 0 or
 * 2); the resampling reads them and writes the f16 lattice planes the plain-f16 decoder consumes.  The throughput decoder under an
 * fp32-grade encoder: most of plain f16's error against the fp32 reference comes from its ENCODER (tests/test_f16_error_budget.py). */
#define GIGA_PLANES_FP32 1024
size_t giga_lattice_workspace_bytes(int B, int R, int precision);
int giga_decoder_forward_lattice(const void* planes_nhwc, const float* lin, const void* packed, int head_mask,
                                 float* qual, float* rot, float* width, float* occ, int B, int R, int precision,
                                 int post, void* workspace, size_t workspace_bytes, void* stream,
                                 void* ev_start, void* ev_stop);
/* The launch plan giga_decoder_forward* (R == 0: B x N generic queries) or giga_decoder_forward_lattice (R > 0; N is ignored)
 * would use for `nheads` heads at `precision` (0..2; GIGA_FOLD_FINAL / GIGA_PLANES_FP32 are ignored), decided NOW: the tuning
 * variables GIGA_DEC_LAT, GIGA_DEC16_RESIDENT, GIGA_DEC32_TILE and GIGA_DEC32_POINT are read on every call, as a launch reads them.
 * Host only: no device is touched.  -1 / -5 on the arguments those calls reject.  plan_words[GIGA_DECODER_PLAN_WORDS], in order
 * (csrc/giga_dec_plan.h, struct DecPlan):
 *   kernel (GIGA_DEC_KERNEL_*; 0: nothing is launched), T (32-point tiles per wave), NW (waves per workgroup), split (operands are
 *   [hi, lo] f16 pairs), dbuf (two line buffers), grid_x, grid_y, block, lds (dynamic LDS bytes), nbatch, heads_per_wg, lat_parts,
 *   slots (workgroups per head of the head-resident kernels), xcd_remap (their XCD-contiguous workgroup map applies). */
#define GIGA_DECODER_PLAN_WORDS 14
#define GIGA_DEC_KERNEL_F16 1        /* decoder_f16_kernel: shared features */
#define GIGA_DEC_KERNEL_F16S 2       /* decoder_f16s_kernel: head-resident */
#define GIGA_DEC_KERNEL_LAT 3        /* decoder_lat_kernel: separable fc_c on the lattice */
#define GIGA_DEC_KERNEL_F32 4        /* decoder_f32_kernel: general exact kernel */
#define GIGA_DEC_KERNEL_F32_TILE 5   /* decoder_f32_tile_kernel */
#define GIGA_DEC_KERNEL_F32_POINT 6  /* decoder_f32_point_kernel */
int giga_decoder_plan(int B, int N, int R, int nheads, int precision, int32_t* plan_words);

/* ---- training path, fp32 (scripts/train_giga.py:198-211: forward, loss.backward(), optimizer.step()) -----
 * The forward is giga_encoder_forward + giga_decoder_forward at precision 0 with the encoder workspace
 * kept alive (it holds every U-Net activation).  giga_backward computes the gradient of a scalar loss with
 * respect to EVERY parameter, given the gradients of the four head outputs:
 *   outs / douts : arrays of 4 device pointers (qual [B*N], rot [B*N][4], width [B*N], occ [B*M]); entries of
 *                  absent heads are ignored, a NULL entry of a head that runs (grasp heads: N > 0; occupancy head:
 *                  M > 0 and p_tsdf given) is GIGA -6.  outs are the forward results (post sigmoid / normalize).
 *                  Every argument is validated before anything is enqueued on the stream.
 *   grads        : flat fp32 buffer in reference state-dict order (giga_param_count), overwritten.
 *   head_present : head bits, optionally | GIGA_DETACH_OCC: the occupancy head then reads detached planes, i.e. its
 *                  loss does not reach the encoder (detach_tsdf of `giga_detach`, models/__init__.py:61-63,
 *                  networks.py:143-169); the three grasp heads are unaffected.
 * It replaces autograd through conv_onet/models/__init__.py:42-67 (decoder.py:117-176, encoder/voxels.py:89-121,
 * encoder/unet.py:225-239).  Data-gradient convolutions and the decoder's gradient chain run on MFMA with the
 * transposed weights of the BACKWARD blob (giga_bwd_packed_bytes / giga_pack_bwd_weights, host; or
 * giga_pack_bwd_map + giga_repack_device on the device every step).  Weight gradients are reduced with fp32
 * atomics (run-to-run differences at rounding level, as in PyTorch's own GPU backward). */
#define GIGA_DETACH_OCC 16
/* GIGA_BF16_CONVS, OR-ed into giga_backward's head_present: the thirteen data-gradient convolutions of the U-Net (from the
 * backward blob's bf16 images) and the weight gradients of its eleven 3x3 layers run on bf16 MFMA (operands rounded to bf16,
 * fp32 accumulate, fp32 gradients in memory); pairs with an encoder forward at precision 3.  ConvTranspose / 1x1 weight
 * gradients, the decoder and conv_in stay fp32.  BASELINE config c5 ("bf16"). */
#define GIGA_BF16_CONVS 32
/* GIGA_BF16_DECODER, OR-ed into giga_backward's head_present: the decoder heads' backward runs as ONE fused bf16 kernel per call
 * (csrc/giga_decoder_train16.hip): the forward chain recomputed on bf16 MFMA, the gradient chain with the transposed bf16 matrices,
 * and the weight gradients dW = dY^T X in the same kernel (tiles handed over through LDS and read back transposed with
 * ds_read_b64_tr_b16; gradient tiles resident in registers across the workgroup's points) -- no [P][32] row arrays, no separate
 * weight-gradient launch; one reduce launch for every head of the step.  Pairs with giga_decoder_forward at precision 3 (the same
 * bf16 arithmetic; the backward recomputes it bit for bit).  Operands (features, activations, gradients, weights) are rounded to
 * bf16 once, accumulation and the residual stream are fp32, fc_p / the biases are carried as hi + lo bf16 pairs. */
#define GIGA_BF16_DECODER 64
/* GIGA_CONVIN_MASK_BWD, OR-ed into giga_backward's head_present: enc_workspace_fwd comes from a forward with GIGA_CONVIN_MASK. */
#define GIGA_CONVIN_MASK_BWD 128
/* bf16 images of the convolution fragments, derived ON THE DEVICE from the fp32 fragments of the same blob(s) after
 * giga_repack_device (either pointer may be NULL).  giga_pack_weights / giga_pack_bwd_weights fill them on the host too. */
int giga_derive_bf16_fragments(void* packed_dev, void* bwd_packed_dev, void* stream);
/* The Winograd-domain images of the fp32 3x3 layers (csrc/giga_wino.h), derived ON THE DEVICE from the fp32 fragments of the same blob
 * after giga_repack_device: U = G g G^T accumulated in double in the host packer's order -- bit-identical to giga_pack_weights' /
 * giga_pack_bwd_weights'.  packed_dev: the forward blob (a precision-0 forward on a device-repacked blob needs it unless the call carries
 * GIGA_DIRECT_CONV); bwd_packed_dev: the backward blob (the fp32 data-gradient chain of giga_backward runs its 3x3 layers as Winograd
 * too unless GIGA_WINOGRAD_BWD=0 is set in the environment).  Either may be NULL. */
int giga_derive_winograd(void* packed_dev, void* bwd_packed_dev, void* stream);
size_t giga_bwd_packed_bytes(void);
int giga_pack_bwd_weights(const float* params_host, size_t n_params, int head_present, void* packed_host,
                          size_t packed_bytes);
int giga_pack_bwd_map(int head_present, int32_t* map_host, size_t nwords);
size_t giga_backward_workspace_bytes(int B, int N, int M, int head_present);
/* Introspection for tests: byte offsets, inside the backward workspace, of the 15 activation-gradient tensors the encoder backward
 * leaves there (fp32 NHWC [3B][H][W][C], in order gA6 gA5 gC1 gA4 gA3 gC0 gS2 gA2 gQ1 gS1 gA1 gQ0 gS0 gA0 gP0: g<X> = gradient of
 * the loss w.r.t. activation X of giga_encoder_workspace_layout; gC1 / gC0 = w.r.t. the concatenated inputs of up1.conv1 /
 * up0.conv1).  gA6 gA5 gA4 gA3 gS2 gA2 gS1 gA1 gS0 gA0 are, with the ReLU mask already applied, the dY operands of the weight
 * gradients of layers 11, 10, 8, 7, 5, 4, 3, 2, 1, 0.  offsets must have room for 15 entries. */
int giga_backward_workspace_layout(int B, size_t* offsets);
/* What the decoder part of giga_backward(..., head_present, B, N, M, ...) would do: which calls run and in which order, every launch
 * shape and every region of the decoder scratch (csrc/giga_dec_bwd_plan.h; giga_backward and giga_backward_workspace_bytes read the same
 * plan).  head_present carries giga_backward's flag bits GIGA_DETACH_OCC and GIGA_BF16_DECODER (the others are ignored); an occupancy
 * head with M > 0 is planned as if p_tsdf were given.  Host only: no device is touched.  Error codes as giga_backward's for the same
 * arguments: -1 (N < 0, M < 0, NULL plan_words), -7 (B > GIGA_MAX_SCENES); B <= 0: all words zero.
 * plan_words[GIGA_DECODER_BACKWARD_PLAN_WORDS], in order (struct TrainDecPlan; a 64-bit field is two words, low first):
 *   bf16, clear_planes (the plane-gradient buffer is cleared first), reduce (dect_reduce_kernel ends the decoder part), launches (kernel
 *   launches of the decoder part), order[GIGA_DECODER_BACKWARD_MAX_LAUNCHES] (their GIGA_DEC_BWD_KERNEL_*, as enqueued);
 *   64-bit: occ_base, grasp_base (the calls' scratch bases in floats), scratch_floats (the step's decoder scratch at this precision);
 *   then the occupancy call and the grasp call, GIGA_DECODER_BACKWARD_CALL_WORDS each (struct DecBwdCall):
 *   runs, kernel, nheads, planes, gather, nbatch, grid_x, grid_y, block, lds, heads_per_wg, wgrad_merged, wgrad_launches, nb_total,
 *   ksplit_cap, ksplit, pts_per_block, launches, fwd_grid_x, fwd_block, fwd_lds, bf16;
 *   64-bit: P, tiles, head_off, head_stride, cbuf_off, pbuf_off, dcbuf_off (floats from the call's base, -1: none), scratch_floats. */
#define GIGA_DECODER_BACKWARD_MAX_LAUNCHES 8
#define GIGA_DECODER_BACKWARD_CALL_WORDS 38
#define GIGA_DECODER_BACKWARD_PLAN_WORDS 94
#define GIGA_DEC_BWD_KERNEL_DECODER_BWD 1    /* decoder_bwd_kernel */
#define GIGA_DEC_BWD_KERNEL_PLANE_GATHER 2   /* plane_gather_kernel */
#define GIGA_DEC_BWD_KERNEL_LINEAR_WGRAD 3   /* linear_wgrad_kernel */
#define GIGA_DEC_BWD_KERNEL_DECT 4           /* dect_kernel<true, 4> */
#define GIGA_DEC_BWD_KERNEL_DECT_REDUCE 5    /* dect_reduce_kernel */
int giga_decoder_backward_plan(int B, int N, int M, int head_present, int32_t* plan_words);
int giga_backward(const float* tsdf, const void* packed, const void* bwd_packed, const void* enc_workspace_fwd,
                  const void* planes_nhwc, const float* p, const float* p_tsdf, const float* const* outs,
                  const float* const* douts, float* grads, size_t n_params, int head_present, int B, int N, int M,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- gradient with respect to the QUERY POINTS (fp32; added within ABI 3) -----------------------------------------------
 * dp [B*N][3] = d/dp of sum_h <dout_h, head_h(p)> over the heads of head_mask, the planes held constant: what autograd of the
 * reference LocalDecoder (decoder.py:117-176) gives for p, as ConvolutionalOccupancyNetwork.grad_refine (models/__init__.py:136-164)
 * and Generator3D.estimate_normals (conv_onet/generation.py:430-455) use it.  The upstream gradients refer to the POST-epilogue
 * outputs of giga_decoder_forward(..., post = 1): dqual of sigmoid(qual), drot of F.normalize(rot), dwidth / dtsdf of the raw
 * outputs; [B*N] each ([B*N][4] for drot), non-NULL for every head in head_mask.  A coordinate that common.py:255-260 clamps
 * contributes no bilinear term (only fc_p's).  dp is overwritten.
 *   planes_nhwc: fp32 FINAL planes (after conv_final: an encoder call WITHOUT GIGA_FOLD_FINAL, or giga_planes_pack precision 0);
 *   packed / bwd_packed: the forward and backward blobs of the same weights (giga_pack_weights / giga_pack_bwd_weights);
 *   out_*: optional (may be NULL) post-epilogue head outputs, bit for bit those of the precision-0 forward kernel;
 *   flags: reserved, must be 0 (GIGA_FOLD_FINAL is rejected with -5).
 * One launch (csrc/giga_decoder_pgrad.hip): per 32-point tile the forward chain is recomputed and the gradient chain run in
 * registers, ending in Wp^T DN0 plus the spatial derivative of the bilinear sample.  Errors before anything is enqueued: -1
 * (head_mask 0 or outside 0xF, B <= 0, N <= 0, B*N >= 2^31, a NULL plane / point / blob pointer or dp), -6 (a head in head_mask with a
 * NULL upstream gradient), -7 (B > GIGA_MAX_SCENES), -5 (flags != 0). */
int giga_decoder_point_grad(const void* planes_nhwc, const float* p, const void* packed, const void* bwd_packed,
                            int head_mask, const float* dqual, const float* drot, const float* dwidth, const float* dtsdf,
                            float* dp, float* out_qual, float* out_rot, float* out_width, float* out_tsdf,
                            int B, int N, int flags, void* stream);

/* ---- occupancy logit, gradient and Hessian at query points (fp32; added within ABI 3) ------------------------------------
 * giga_decoder_point_grad for the occupancy head alone with upstream gradient 1, plus the second derivative of the logit f with
 * respect to p.  The decoder is piecewise linear in (p, c) and c(p) is a bilinear sample of three planes, so almost everywhere
 * the Hessian of f has a zero diagonal and one entry per plane, d2f/du dv = s_u s_v sum_ch dc[ch] (f00 - f01 - f10 + f11)[ch] (dc:
 * the gradient w.r.t. the sampled features, s = 39 / 1.00001, or 0 along an axis that common.py:255-260 clamps).
 *   logit [B*N]: the raw occupancy output, bit for bit giga_decoder_point_grad's out_tsdf;  dp [B*N][3]: bit for bit its dp for
 *   head_mask 8 and dtsdf = 1;  hess [B*N][3] = (H_xy, H_xz, H_yz).  All three are overwritten; planes and blobs as above.
 * One launch (the HESS instantiation of the same kernel).  Errors before anything is enqueued: -1 (B <= 0, N <= 0, B*N >= 2^31, a
 * NULL plane / point / blob pointer, logit, dp or hess), -7 (B > GIGA_MAX_SCENES). */
int giga_decoder_point_hess(const void* planes_nhwc, const float* p, const void* packed, const void* bwd_packed, float* logit,
                            float* dp, float* hess, int B, int N, void* stream);

/* ---- mesh refinement: Generator3D.refine_mesh (conv_onet/generation.py:457-519) as closed-form per-face arithmetic ------------
 * One refinement step of a triangle mesh (vertices [V][3] float32, faces [F][3] int32, both on the device) is
 *   giga_refine_face_points -> giga_decoder_point_hess at the face points (B = 1, N = F) -> giga_refine_face_grad ->
 *   giga_refine_vertex_step,
 * and minimises mean_f (sigmoid(f(q_f)) - threshold)^2 + 0.01 mean_f |n_f - t_f|^2 over the vertices, q_f = sum_i eps_fi v_fi the
 * face point, n_f = c / (|c| + 1e-10) with c = (v1 - v0) x (v2 - v1), t_f = -g / (|g| + 1e-10) with g = grad_q sigmoid(f(q_f)).
 *
 * giga_refine_face_points: eps [F][3] and points [F][3] are written.  eps_in [F][3] non-NULL: eps = eps_in.  NULL: eps is drawn,
 *   Dirichlet(1/2, 1/2, 1/2) as z_i^2 / sum_j z_j^2 from the normals z_0, z_1 (Box-Muller pair of block 0) and z_2 (first normal of
 *   block 1) of the Philox counter (block, face, step, 0), key = seed (blocks, uniforms and normals as in giga_depth_noise).
 *   points = (v0 eps_0 + v1 eps_1) + v2 eps_2 in fp32.
 * giga_refine_face_grad: logit [F], dp [F][3], hess [F][3] are giga_decoder_point_hess's outputs at `points`.  face_loss [F][2] =
 *   ((sigma - threshold)^2, |n - t|^2) (the caller takes the means); face_grad [F][3][3] = d loss / d (corner i of face f), with
 *   the 1/F of the means folded in.  Where |g| or |c| is exactly 0 the a a^T / |a| term of the normalisation's Jacobian is 0
 *   (torch's subgradient of norm at the origin).  The arithmetic runs in double on the fp32 inputs.
 * giga_refine_vertex_step: corner_order [3F] lists the corners (3 * face + i) sorted by their vertex, vertex_offsets [V+1] is the
 *   CSR row table into it.  grad [V][3] = the sum of the vertex's corner gradients in list order (no atomics: bit reproducible),
 *   then torch.optim.RMSprop's defaults in place: square_avg = 0.99 square_avg + 0.01 grad^2,
 *   vertices -= 1e-4 grad / (sqrt(square_avg) + 1e-8).  A vertex without corners has grad 0 and does not move.
 * A face with a corner index outside [0, V) gets NaN outputs and an entry of corner_order outside [0, 3F) is skipped: no index
 * is followed out of its array.  Errors before anything is enqueued: -1 (negative counts, V > GIGA_REFINE_MAX_VERTICES,
 * F > GIGA_REFINE_MAX_FACES, step < 0, threshold outside (0, 1), a NULL input), -6 (a NULL output).  F = 0 (face kernels) and
 * V = 0 (vertex step) return 0 without a launch. */
#define GIGA_REFINE_MAX_VERTICES 0x0FFFFFFF
#define GIGA_REFINE_MAX_FACES 0x0FFFFFFF
int giga_refine_face_points(const float* vertices, const int* faces, const float* eps_in, float* eps, float* points,
                            int n_vertices, int n_faces, unsigned long long seed, int step, void* stream);
int giga_refine_face_grad(const float* vertices, const int* faces, const float* eps, const float* logit, const float* dp,
                          const float* hess, double threshold, float* face_loss, float* face_grad, int n_vertices, int n_faces,
                          void* stream);
int giga_refine_vertex_step(const float* face_grad, const int* corner_order, const int* vertex_offsets, float* vertices,
                            float* square_avg, float* grad, int n_vertices, int n_faces, void* stream);

/* ---- input side: page-locking of caller-owned host memory (hipHostRegister / hipHostUnregister), so that batches which
 * reader processes assemble in a shared-memory ring are DMA-ed to the device without a staging copy
 * (giga_amd/feed.py; replaces the pageable `.to(device)` of train_giga.py:141-151). */
int giga_host_register(void* ptr, size_t bytes);
int giga_host_unregister(void* ptr);

/* ---- input side: dense export of a sparse TSDF (src/vgn/perception.py:107-115, TSDFVolume.get_grid) -----
 * voxel_index [n][3] int32 (grid_index i, j, k) and voxel_value [n] float32 (voxel.color[0]) list the observed voxels of B
 * scenes back to back; scene b owns voxels scene_offsets[b] .. scene_offsets[b+1]-1 (scene_offsets [B+1], device).
 * grid [B][R][R][R] float32 receives 0 for unobserved cells and the value of the LAST voxel of the list that targets a
 * cell (the Python loop's semantics; Open3D's lists have unique indices).  Indices outside [0, R) are ignored.
 * workspace: giga_tsdf_scatter_workspace_bytes(B, R) bytes of device scratch. */
size_t giga_tsdf_scatter_workspace_bytes(int B, int R);
int giga_tsdf_scatter(const int32_t* voxel_index, const float* voxel_value, const int32_t* scene_offsets, int B, int R,
                      int n_voxels, float* grid, void* workspace, size_t workspace_bytes, void* stream);

/* ---- input side: fusion of depth images into the volume (src/vgn/perception.py:63-126: TSDFVolume.integrate, get_grid,
 * get_cloud, which the reference hands to Open3D's UniformTSDFVolume with NoColor) -----
 * giga_tsdf_integrate fuses, for B scenes in one launch, scene b's views view_offsets[b] .. view_offsets[b+1]-1 into that scene's
 * state.  depth [n_views][height][width] float32 (device) holds the images of all scenes back to back.  HOST arrays, read (and
 * copied into the workspace) before the call returns: view_offsets [B+1] int32, extrinsics [n_views][16] double (task -> camera,
 * row-major 4x4), intrinsics [n_views][4] double (fx, fy, cx, cy).  The volume is the cube [0, length]^3 with R cells per axis,
 * voxel_length = length / R; the reference passes sdf_trunc = 4 voxel_length, depth_scale = 1, depth_trunc = 2.  State: tsdf and
 * weight [B][R][R][R] float32 (device), cell (x, y, z) at x R R + y R + z, read and updated in place (zeros = a new volume; a
 * later call with further views continues the running average).  Per voxel and view, in view order (E the extrinsic):
 *     p   = (x + 0.5, y + 0.5, z + 0.5) voxel_length                                          double
 *     pc  = E[:3,:3] p + E[:3,3], every row ((e0 p.x + e1 p.y) + e2 p.z) + e3                  double; skip unless pc.z > 0
 *     u_f = pc.x fx / pc.z + cx + 0.5, v_f = pc.y fy / pc.z + cy + 0.5                        double
 *     skip unless 0.0001 <= u_f < width - 0.0001 and 0.0001 <= v_f < height - 0.0001;  u, v = (int) u_f, (int) v_f
 *     d   = depth[v][u] / float(depth_scale); d = 0 if d >= float(depth_trunc)                float32; skip unless d > 0
 *     m   = float(sqrt((((u - cx) / fx)^2 + ((v - cy) / fy)^2) + 1))                          double, rounded once
 *     sdf = float((double(d) - pc.z) double(m));  skip unless sdf > -float(sdf_trunc)
 *     t   = min(1, sdf float(1 / sdf_trunc));  tsdf = (tsdf weight + t) / (weight + 1);  weight += 1       float32
 * with one IEEE rounding per operation (no fused multiply-add).  grid [B][R][R][R] float32 (device, may be NULL) receives in the
 * same pass the network input that get_grid builds from extract_voxel_grid: float((double(tsdf) + 1) 0.5) where weight != 0 and
 * -0.98 <= tsdf < 0.98 (compared in double), 0 elsewhere.  One lane per voxel with the views looped inside: no atomics, equal
 * input gives equal bytes, and a batch gives scene b the bytes of a call on scene b alone.
 * Every argument is checked before the first HIP call.  Errors: -1 negative B, R outside 2 .. GIGA_TSDF_MAX_R, width or height
 * outside 1 .. GIGA_TSDF_MAX_IMAGE, length / sdf_trunc / depth_scale not finite or <= 0, NaN depth_trunc, offsets that do not
 * start at 0 or decrease, a non-finite camera entry, fx or fy equal to 0, null depth / cameras (with views) / state / workspace;
 * -4 workspace too small (giga_tsdf_integrate_workspace_bytes(B, view_offsets[B])); -7 B > GIGA_MAX_SCENES.  B = 0 returns 0.
 *
 * giga_tsdf_cloud_count / giga_tsdf_cloud_emit: the points of extract_point_cloud (no normals, no colours).  A voxel is valid when
 * weight != 0 and -0.98 <= tsdf < 0.98.  A valid voxel with value f0 at p0 = (x + 0.5, y + 0.5, z + 0.5) voxel_length gives, for
 * each axis i whose neighbour index n_i + 1 < R - 1, whose neighbour is valid with value f1, and f0 f1 < 0 (float32 product), the
 * point p0 with component i replaced by (p0_i |f1| + (p0_i + voxel_length) |f0|) / (|f0| + |f1|), evaluated in double and stored
 * as float32.  Two phases like giga_mesh_count / giga_mesh_emit: count writes counts [B] int32 (device) and keeps the offsets in
 * the workspace (giga_tsdf_cloud_workspace_bytes(B, R)), which must reach emit unchanged together with the same state; emit
 * writes points [cap][3] float32, scenes back to back, in cell order and then axis order inside a scene.  Nothing is written at or
 * beyond cap; shortfall [1] int32 (device, may be NULL) receives the number of points that did not fit.
 * Errors: -1 as above or null state / workspace / counts; -4; -6 null points with cap > 0; -7.
 *
 * giga_tsdf_cloud_emit_oriented (added within ABI 3): giga_tsdf_cloud_emit plus normals [cap][3] float32 (device), one per point.
 * It reads the workspace that giga_tsdf_cloud_count filled and writes the same points in the same order (bit for bit), with the
 * same cap / shortfall rule for both arrays; -6 also for null normals with cap > 0.  The normal of a point restates Open3D's
 * UniformTSDFVolume::GetNormalAt (agreement with Open3D itself is unverified, as for the points).  All of it in float64, one
 * rounding per operation, no fused multiply-add.  p is the point in float64 BEFORE it is rounded to float32 (p0 with component i
 * replaced by the quotient above), v = voxel_length = length / R, g = 0.99 v.
 *     T(q)   s_c = q_c / v - 0.5, i_c = floor(s_c), r_c = s_c - i_c for c = x, y, z.  With w_c(0) = 1 - r_c and w_c(1) = r_c, T is
 *            the sum over (dx, dy, dz) in the order 000, 001, 010, 011, 100, 101, 110, 111 (dz fastest) of
 *                ((w_x(dx) w_y(dy)) w_z(dz)) double(tsdf[i_x + dx][i_y + dy][i_z + dz]),
 *            the first term taken as it is and the others added to it from left to right.  The weight array is NOT consulted: an
 *            unobserved voxel contributes its stored value (0 in a volume that integrate built).  A voxel with an index outside
 *            [0, R) on any axis contributes the value 0.0: this library's choice -- Open3D reads out of bounds there.
 *     n_c    = T(p + g e_c) - T(p - g e_c), c = x, y, z (only component c of p changes: p_c + g, p_c - g)
 *     z      = (n_x n_x + n_y n_y) + n_z n_z;  normal = n / sqrt(z) per component if z > 0, else (0, 0, 0) (Eigen's normalized());
 *            every component is rounded once to float32.
 * One lane per cell as in giga_tsdf_cloud_emit; 48 four-byte reads per normal. */
#define GIGA_TSDF_MAX_R 512
#define GIGA_TSDF_MAX_IMAGE 16384
size_t giga_tsdf_integrate_workspace_bytes(int B, int n_views);
int giga_tsdf_integrate(const float* depth, const int32_t* view_offsets, const double* extrinsics, const double* intrinsics, int B,
                        int width, int height, double length, int R, double sdf_trunc, double depth_scale, double depth_trunc,
                        float* tsdf, float* weight, float* grid, void* workspace, size_t workspace_bytes, void* stream);
size_t giga_tsdf_cloud_workspace_bytes(int B, int R);
int giga_tsdf_cloud_count(const float* tsdf, const float* weight, int B, int R, void* workspace, size_t workspace_bytes,
                          int32_t* counts, void* stream);
int giga_tsdf_cloud_emit(const float* tsdf, const float* weight, int B, int R, double length, const void* workspace,
                         size_t workspace_bytes, float* points, size_t cap, int32_t* shortfall, void* stream);
int giga_tsdf_cloud_emit_oriented(const float* tsdf, const float* weight, int B, int R, double length, const void* workspace,
                                  size_t workspace_bytes, float* points, float* normals, size_t cap, int32_t* shortfall, void* stream);

/* ---- input side: depth images of posed triangle meshes (the depth half of btsim.Camera.render, src/vgn/utils/btsim.py:276-337,
 * which the reference hands to PyBullet) -----
 * B scenes packed back to back in the ragged layout giga_mesh_emit produces: vertices [.][3] float32 and triangles [.][3] int32
 * (device), a scene's triangles counting from its OWN first vertex.  HOST arrays, validated before the first HIP call and copied
 * into the workspace before the call returns: vertex_offsets, triangle_offsets, view_offsets [B+1] int32 (start at 0, never
 * decrease), extrinsics [n][16] double (task -> camera, row-major 4x4), intrinsics [n][4] double (fx, fy, cx, cy), n =
 * view_offsets[B].  View k of scene b is image view_offsets[b] + k of depth [n][H][W] float32 (device): the layout
 * giga_tsdf_integrate consumes.  Everything below is evaluated in double with one IEEE rounding per operation (no fused
 * multiply-add); E is the view's extrinsic:
 *   camera-space vertex  a = E (x, y, z, 1) from the float32 vertex, every row ((e0 x + e1 y) + e2 z) + e3.
 *   pixel ray            pixel (row v, column u) has direction d = ((u + pixel_offset - cx) / fx, (v + pixel_offset - cy) / fy, 1),
 *                        the numerators evaluated left to right.  pixel_offset = 0 is the convention of giga_tsdf_integrate (pixel u
 *                        is centred on image coordinate u); 0.5 is OpenGL's.
 *   edge function        for an ordered vertex pair (P, Q): n = P x Q = (Py Qz - Pz Qy, Pz Qx - Px Qz, Px Qy - Py Qx) and
 *                        e(P, Q) = (d.x n.x + d.y n.y) + n.z.  e(P, Q) == -e(Q, P) exactly, so two triangles that share an edge
 *                        decide a ray through that edge consistently.
 *   hit test             U = e(b, c), V = e(c, a), W = e(a, b), S = (U + V) + W.  The triangle (a, b, c) is hit iff S != 0 and
 *                        (U, V, W all >= 0 or all <= 0): zero counts as inside (watertight: no cracks on shared edges or
 *                        vertices), and both faces are visible.
 *   depth of a hit       z = ((U a.z + V b.z) + W c.z) / S; the hit is accepted iff near <= z <= far.
 *   output               depth[v][u] = float(min accepted z), or float(far) when no triangle is accepted (with far = 2 = the
 *                        fusion's depth_trunc, giga_tsdf_integrate ignores such pixels).
 * A triangle with a vertex index outside its scene is skipped; a triangle with a non-finite vertex is never accepted (its
 * comparisons are false).  The minimum does not depend on the order: equal input gives equal bytes, and a batch gives scene b
 * the bytes of a call on scene b alone.  No allocation; asynchronous on `stream`.
 * Not reproduced: PyBullet's TinyRenderer fill rule at silhouettes, its z-buffer quantisation (RGB: giga_color_render below).
 * Measurement aid: the first 8 bytes of the workspace hold, after the call, the number of (triangle, 16x16 pixel tile) pairs that
 * survived the kernel's culling (uint64).
 * Errors: -1 negative B, W or H outside 1 .. GIGA_RENDER_MAX_IMAGE, near / far / pixel_offset not finite, near <= 0, far <= near,
 * offsets that are null, do not start at 0 or decrease, n W H >= 2^31, null vertices / triangles (with a non-zero count), null
 * cameras or workspace (with views), a non-finite camera entry, fx or fy equal to 0; -6 null depth (with views); -4 workspace
 * smaller than giga_depth_render_workspace_bytes(B, n, vertex_offsets[B], triangle_offsets[B]); -7 B > GIGA_MAX_SCENES.
 * B = 0 and n = 0 return 0. */
#define GIGA_RENDER_MAX_IMAGE 4096
size_t giga_depth_render_workspace_bytes(int B, int n_views, int n_vertices, int n_triangles);
int giga_depth_render(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                      const int32_t* view_offsets, const double* extrinsics, const double* intrinsics, int B, int W, int H,
                      double near, double far, double pixel_offset, float* depth, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---- output side: shaded images of coloured meshes (render_mesh of src/vgn/utils/visual.py:147-164, pyrender there, and the RGB
 * half of btsim.Camera.render) -----
 * giga_color_render takes giga_depth_render's ragged mesh batch and cameras (the same layouts, HOST arrays and checks) and in
 * addition face_colors [.][4] uint8 RGBA (device, 4-byte aligned), one per triangle in the order of `triangles`; lights [n][4]
 * double (HOST, per view, camera frame: (lx, ly, lz, lw); NULL = (0, 0, 0, 1) for every view); ambient in [0, 1]; background [4] uint8
 * RGBA (HOST; NULL = opaque white).  Outputs (device), per pixel: rgba [n][H][W] uint32 = R | G << 8 | B << 16 | A << 24 (in memory
 * the bytes R, G, B, A); depth [n][H][W] float32, may be NULL; triangle_index [n][H][W] int32, the winning triangle counted from
 * its scene's first triangle, or -1, may be NULL.
 *   visibility   giga_depth_render's hit test and depth z, operation for operation.  Among the accepted triangles the winner is
 *                the one with the smallest z, and among equal z the one with the smallest index: the image does not depend on the
 *                order in which triangles are tested.  depth = float(z of the winner) or float(far): giga_depth_render's bytes.
 *   shading      flat and two-sided, in double, one IEEE rounding per operation, sums of three left to right
 *                ((x0 y0 + x1 y1) + x2 y2), with the winner's camera-space vertices a, b, c, its z and the pixel's direction d:
 *                  p = (z d.x, z d.y, z)
 *                  n = (b - a) x (c - a)          (the cross product as in the edge function)
 *                  L = (lx - lw p.x, ly - lw p.y, lz - lw p.z): lw = 1 is a point light at (lx, ly, lz), (0, 0, 0, 1) the
 *                      headlight at the camera; lw = 0 a direction towards the light
 *                  q = (n . n) (L . L)
 *                  k = ambient + ((1 - ambient) |n . L|) / sqrt(q);  k = ambient when q is 0 or not finite
 *                  each of the face's R, G, B bytes C becomes min(floor(k C + 0.5), 255); alpha is 255.
 *                A pixel without a winner gets `background`, all four bytes.
 * This is the project's own shading model, not pyrender's metallic-roughness one; no smooth shading, textures, shadows or
 * transparency (the face's alpha is not used).  Equal input gives equal bytes; a batch gives scene b the bytes of a call on
 * scene b alone.  No allocation; asynchronous on `stream`.  The first 8 bytes of the workspace count the surviving (triangle,
 * tile) pairs as for giga_depth_render.
 * Errors: giga_depth_render's, and -1 ambient outside [0, 1] (or NaN), a non-finite light, null or misaligned face_colors with a
 * non-zero triangle count; -6 null rgba (with views); -4 workspace smaller than giga_color_render_workspace_bytes(...).
 *
 * giga_image_downsample: k x k box filter of RGBA bytes, k in 1 .. GIGA_DOWNSAMPLE_MAX_K, in integers: src [n][k H][k W] uint32,
 * dst [n][H][W] uint32 (device), per channel dst = (sum of the k k samples + (k k) / 2) / (k k), integer division.  Rendering at
 * k W x k H with fx' = k fx, fy' = k fy, cx' = k cx, cy' = k cy, pixel_offset' = k (pixel_offset - 0.5) + 0.5 puts the k k samples
 * on a regular grid inside each pixel's footprint, symmetric about its centre.
 * Errors: -1 negative n, k outside 1 .. 4, W or H outside 1 .. GIGA_RENDER_MAX_IMAGE, n W H k k >= 2^31, null src; -6 null dst. */
#define GIGA_DOWNSAMPLE_MAX_K 4
size_t giga_color_render_workspace_bytes(int B, int n_views, int n_vertices, int n_triangles);
int giga_color_render(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                      const uint8_t* face_colors, const int32_t* view_offsets, const double* extrinsics, const double* intrinsics,
                      const double* lights, double ambient, const uint8_t* background, int B, int W, int H, double near, double far,
                      double pixel_offset, uint32_t* rgba, float* depth, int32_t* triangle_index, void* workspace,
                      size_t workspace_bytes, void* stream);
int giga_image_downsample(const uint32_t* src, uint32_t* dst, int n, int W, int H, int k, void* stream);

/* ---- input side: depth-sensor noise, the dex, trans and norm models of vgn.utils.misc.apply_noise (src/vgn/utils/misc.py:18-69),
 * which the reference applies to every depth image before fusion (scripts/construct_dataset_parallel.py:21, simulation.py:176) -----
 * depth_in, depth_out [n][H][W] float32 (device): the layout giga_depth_render writes and giga_tsdf_integrate reads.  Out of
 * place (trans is a gather): overlapping buffers are an error, depth_in is never written.  model: GIGA_NOISE_DEX / _TRANS / _NORM.
 * params (HOST, NULL = the reference's defaults): dex {gamma_shape 1000, gamma_scale 0.001, gp_sigma 0.005, gp_scale 4, gp_rate
 * 0.5}, trans {sigma_p 1, sigma_d 0.005}, norm {sigma 0.005}.  image_ids (HOST [n] uint64, NULL = 0 .. n-1) is copied into the
 * workspace before the call returns.  Asynchronous on `stream`, no allocation, one launch (more only beyond 2^22 tiles).
 * Draws are counter based.  Block (b, id, s) is Philox-4x32-10 on the counter (b, id & 0xffffffff, id >> 32, s) with the key
 * (seed & 0xffffffff, seed >> 32); id the image's id, s the stream: 0 image scalars, 1 GP coarse grid, 2 trans row displacement,
 * 3 trans column displacement, 4 per-pixel depth noise.  A block's words x0..x3 give two uniforms u(x0, x1), u(x2, x3) with
 * u(hi, lo) = k 2^-53, k = (hi >> 5) 2^26 + (lo >> 6) (53 bits; 2^-54 in place of k = 0, so 0 < u < 1) and the Box-Muller pair
 * z0 = rad cos(th), z1 = rad sin(th), rad = sqrt(-2 log u(x0, x1)), th = 6.283185307179586 u(x2, x3).  Element e of a stream is
 * z(e & 1) of block e >> 1; element r w + c belongs to entry (r, c) of the array the reference fills with randn(h, w).  So an
 * image's output depends only on seed, its id, W, H, the model and the parameters: not on the batch it sits in, the launch
 * geometry or the order of calls, and equal input gives equal bytes.  All arithmetic is double with one IEEE rounding per
 * operation unless stated; log, cos, sin (and pow for gamma_shape < 1) are the only operations whose last bits may differ between
 * implementations.
 *   dex    gamma = Marsaglia-Tsang (2000) for shape a, d = a - 1/3, c = 1 / sqrt(9 d): attempt k = 0, 1, .. takes x = z0 of
 *          image-stream block 1 + 2k and u = u(x0, x1) of block 2 + 2k; v = 1 + c x, rejected if v <= 0; v = v^3; accepted if
 *          u < 1 - 0.0331 x^4 or log u < 0.5 x^2 + d ((1 - v) + log v); the draw is d v gamma_scale.  At most
 *          GIGA_NOISE_GAMMA_ATTEMPTS attempts (each accepts with probability > 0.95): after that the draw is d gamma_scale, the
 *          sampler's value at x = 0.  gamma_shape < 1 draws shape + 1 and multiplies by u(x2, x3)^(1 / shape) of block 0.
 *          out = in * float(gamma) in float32.  The coin u(x0, x1) of image-stream block 0 is always drawn; if it is below
 *          gp_rate, a coarse h x w grid, h = int(H / gp_scale), w = int(W / gp_scale), of stream-1 normals times gp_sigma is
 *          upsampled bilinearly to H x W with the pixel-centre mapping src = (dst + 0.5) (h / H) - 0.5 per axis, taps outside the
 *          grid reading 0: f = floor(src), t = src - f, value = (1 - ty) ((1 - tx) g[fy][fx] + tx g[fy][fx+1]) + ty ((1 - tx)
 *          g[fy+1][fx] + tx g[fy+1][fx+1]), and out = float(double(out) + value).  This is skimage.transform.resize(order=1,
 *          mode="constant", anti_aliasing=False) WITHOUT its final clip to the coarse grid's [min, max]: the clip changes nothing
 *          when the grid has both signs (always, for practical purposes, at 120 x 160 coarse cells) and is not reproduced.
 *   trans  r' = clip(rint(r + n1 sigma_p), 0, H - 1), c' = clip(rint(c + n2 sigma_p), 0, W - 1) (rint: half to even; n1, n2
 *          elements r W + c of streams 2 and 3), out[r][c] = float(double(in[r'][c']) + n3 sigma_d), n3 of stream 4.
 *   norm   out = float(double(in) + n sigma), n of stream 4.
 * Every argument is checked before the first HIP call.  Errors: -1 negative n, W or H outside 1 .. GIGA_TSDF_MAX_IMAGE,
 * n W H >= 2^31, unknown model, a sigma / shape / scale parameter that is not finite or not > 0, gp_rate outside [0, 1], gp_scale
 * < 1 or above H or W (the coarse grid would be empty), null images or workspace with n > 0, overlapping images; -4 workspace
 * smaller than giga_depth_noise_workspace_bytes(n, W, H, model).  n = 0 returns 0. */
#define GIGA_NOISE_DEX 1
#define GIGA_NOISE_TRANS 2
#define GIGA_NOISE_NORM 3
#define GIGA_NOISE_GAMMA_ATTEMPTS 16
size_t giga_depth_noise_workspace_bytes(int n_images, int width, int height, int model);
int giga_depth_noise(const float* depth_in, float* depth_out, int n_images, int width, int height, int model, const double* params,
                     unsigned long long seed, const unsigned long long* image_ids, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---- input side: training batches from a device-resident training set (the reference's DatasetVoxelOccFile.__getitem__ with its
 * apply_transform, src/vgn/dataset_voxel.py:55-135, and the DataLoader's collate) -----
 * GigaBatchSet describes the set; every array is the caller's and is only read.  Device arrays: grids [n_scenes][40][40][40]
 * float32 (16-byte aligned); per grasp row r: row_scene int32, row_pos [3] float32 (METRIC position of the grasp table), row_quat
 * [4] float32 (x, y, z, w as in the table), row_rotations [2][4] float32 (the two gripper rotations of the un-augmented item),
 * row_width float32 (metric), row_label float32; scene_files [n_scenes + 1] int32: the files of scene s are scene_files[s] ..
 * scene_files[s + 1] - 1, in the order the host reader lists them; file_points [n_files + 1] INT64: the points of file f are
 * file_points[f] .. file_points[f + 1] - 1 (a set may hold more than 2^31 points; one file holds fewer); points [n_points][3] of
 * point_dtype (GIGA_BATCH_POINTS_F32 / _F16), occ [n_points] uint8.  scene_files_host / file_points_host: HOST copies of the two
 * offset arrays or NULL; where given they are checked (first entry 0, non-decreasing, last entry n_files / n_points) before the
 * first HIP call -- pass them on the first call for a set, NULL afterwards.  size: the workspace edge length of setup.json.
 *
 * giga_batch_draw: the random draws of B items.  ordinals [B] int32 (device): an item's position in its epoch's order; rows [B]
 * int32 (device): its grasp row.  Philox-4x32-10 (as giga_depth_noise) on the counter (block, ordinal, epoch, stream) with the key
 * (seed & 0xffffffff, seed >> 32), so an item's draws depend on (seed, epoch, ordinal) and its scene's file sizes only: not on the
 * batch size, the batch it falls in or the rank.  mulhi(a, b) = (a b) >> 32 on 64-bit integers.
 *   stream 0, block 0, words x0..x3:  quarter [B] int32 = x0 >> 30;  u [B] FLOAT64 = 6 + 28 (x1 2^-32) in double;  file [B] int32 =
 *     mulhi(x3, number of files of the row's scene): the index into the scene's file list.
 *   stream 1: index [B][M] int32 into the drawn file of n points.
 *     M > n   with replacement: word (m & 3) of block (m >> 2) gives index[m] = mulhi(word, n).
 *     M <= n  M distinct indices index[m] = pi(m), pi a keyed bijection of [0, n): n = 1 gives 0; otherwise a balanced Feistel
 *             network on b bits, b the smallest even number >= 2 with 2^b >= n, halves of h = b / 2 bits, v = m = (L << h) | R,
 *             GIGA_BATCH_FEISTEL_ROUNDS rounds (L, R) <- (R, L ^ (fmix32(R ^ k_r) & (2^h - 1))) with k_r = x[r & 3] + r 0x9E3779B9
 *             (mod 2^32), x the words of block 0, and fmix32 MurmurHash3's finaliser (h ^= h >> 16, h *= 0x85ebca6b, h ^= h >> 13,
 *             h *= 0xc2b2ae35, h ^= h >> 16).  The network is applied again while v >= n (cycle walking: it is a bijection of
 *             [0, 2^b), so the walk returns below n after at most 2^b - n + 1 < 3 n + 2 applications, the bound of the loop; each
 *             application ends the walk with probability n / 2^b > 1/4).  Each m is evaluated on its own.
 * giga_batch_assemble: the batch of B items from forced draws (quarter, u, file, index as above, device).  For item b with row r
 * and scene s = row_scene[r]:
 *   x [B][40][40][40] (16-byte aligned)  augment == 0: grids[s].  Otherwise z_off = u - double(row_pos[r][2]) and output voxel
 *     (i, j, k) reads source (s_i, s_j, s_k): (s_i, s_j) = (i, j), (j, 40 - i), (40 - i, 40 - j), (40 - j, i) for quarter 0..3;
 *     c = double(k) - z_off, s_k = floor(c + 0.5); the value is grids[s][s_i][s_j][s_k] where 0 <= s_i, s_j <= 39 and 0 <= c <= 39
 *     and 0 elsewhere: scipy.ndimage.affine_transform(order=0, mode="constant") about the centre (20, 20, 20), with exact integers
 *     in x and y (scipy's own in-range test of a source index of exactly 0 or 39 hangs on the rounding of its rotation matrix).
 *   pos [B][3]  augment == 0: float32 arithmetic, row_pos / float(size) - 0.5.  Otherwise in double: d = (x - 20, y - 20) turned to
 *     (dx, dy), (-dy, dx), (-dx, -dy), (dy, -dx) for quarter 0..3, plus 20; z' = z + z_off; then p' / size - 0.5, rounded once to
 *     float32 (the reference transforms the metric position with these voxel-unit offsets; restated as it is).
 *   rotations [B][2][4]  augment == 0: row_rotations.  Otherwise in double: o = row_quat / sqrt(((x^2 + y^2) + z^2) + w^2), then
 *     rot[0] = q_aug (x) o = (c o.x - s o.y, c o.y + s o.x, c o.z + s o.w, c o.w - s o.z) with (s, c) = (sin, cos)(quarter pi / 4) the
 *     doubles (0, 1), (0.7071067811865475, 0.7071067811865476), (1, 6.123233995736766e-17), (0.7071067811865476,
 *     -0.7071067811865475); rot[1] = rot[0] (x) (0, 0, 1, 0) = (r.y, -r.x, r.w, -r.z); each rounded once to float32.
 *   width [B] = row_width / float(size) in float32; label [B] = row_label.
 *   pos_occ [B][M][3] = points[file_points[scene_files[s] + file] + index[m]] / size - 0.5 in the points' own type, then widened:
 *     float32 points: (p / float(size)) - 0.5f.  float16 points: size rounded to float16, the quotient of the two as float32 rounded
 *     to float16, minus 0.5 as float32 rounded to float16 (what numpy computes).  occ [B][M] = the byte as float.
 * All double arithmetic is one IEEE rounding per operation (compiled without contraction); equal input gives equal bytes (no
 * atomics).  A row, file or index outside its range (possible only with inconsistent input) yields zeros, never an access outside
 * the set.  Both calls are asynchronous on `stream`, allocate nothing, and are one launch each.
 * Every argument is checked before the first HIP call.  Errors: -1 null set, rows, ordinals or draws, a null array of the set,
 * negative B, M, epoch or counts, B > GIGA_BATCH_MAX_ITEMS, unknown point_dtype, size not finite or not > 0, misaligned grids or x,
 * host offsets that do not start at 0, decrease, or end elsewhere than n_files / n_points; -6 a null output (index, pos_occ and occ
 * may be null when M = 0).  B = 0 returns 0. */
#define GIGA_BATCH_RES 40
#define GIGA_BATCH_POINTS_F32 0
#define GIGA_BATCH_POINTS_F16 1
#define GIGA_BATCH_FEISTEL_ROUNDS 8
#define GIGA_BATCH_MAX_ITEMS 65535
typedef struct GigaBatchSet {
    const float* grids;
    const int32_t* row_scene;
    const float* row_pos;
    const float* row_quat;
    const float* row_rotations;
    const float* row_width;
    const float* row_label;
    const int32_t* scene_files;
    const int64_t* file_points;
    const void* points;
    const uint8_t* occ;
    const int32_t* scene_files_host;
    const int64_t* file_points_host;
    int64_t n_points;
    int32_t n_scenes, n_rows, n_files, point_dtype;
    double size;
} GigaBatchSet;
int giga_batch_draw(const GigaBatchSet* set, const int32_t* ordinals, const int32_t* rows, int B, int M, int epoch,
                    unsigned long long seed, int32_t* quarter, double* u, int32_t* file, int32_t* index, void* stream);
int giga_batch_assemble(const GigaBatchSet* set, const int32_t* rows, const int32_t* quarter, const double* u, const int32_t* file,
                        const int32_t* index, int B, int M, int augment, float* x, float* pos, float* pos_occ, float* label,
                        float* rotations, float* width, float* occ, void* stream);

/* ---- fused training loss (scripts/train_giga.py:154-195: `select` + `loss_fn`, literal call shape N = 1) -----
 * Inputs are the head outputs of the model's forward for one grasp query per scene -- qual [B] (post sigmoid), rot [B][4]
 * (unit), width [B], occ_logits [B][M] (raw; the sigmoid of `select` is part of this function) -- and the labels of
 * `prepare_batch` (train_giga.py:141-151): label [B], rot_targets [B][2][4], width_target [B], occ_target [B][M].
 *   giga_train_loss          : losses [5] (device) = means over the batch of loss_qual, loss_rot, loss_width, loss_occ and
 *                              loss_all = mean(loss_qual + label (loss_rot + 0.01 loss_width) + loss_occ), the `loss_dict`
 *                              of train_giga.py:169-173; scene_losses [B][5] (device, scratch and per-scene values).
 *   giga_train_loss_backward : d loss_all / d(qual, rot, width, occ_logits), scaled by the device scalar *grad_loss.
 * Arithmetic follows ATen's fp32 formulas (BCE logs clamped at -100, BCE gradient (p-y)/max(p(1-p),1e-12)); the mean
 * over scenes is summed in scene order (deterministic). */
int giga_train_loss(const float* qual, const float* rot, const float* width, const float* occ_logits, const float* label,
                    const float* rot_targets, const float* width_target, const float* occ_target, int B, int M,
                    float* losses, float* scene_losses, void* stream);
int giga_train_loss_backward(const float* qual, const float* rot, const float* width, const float* occ_logits,
                             const float* label, const float* rot_targets, const float* width_target,
                             const float* occ_target, const float* grad_loss, int B, int M, float* dqual, float* drot,
                             float* dwidth, float* docc, void* stream);

/* giga_train_loss with the metrics of a training epoch (scripts/train_giga.py:53-59: ignite's Accuracy, Precision, Recall and five
 * Averages) accumulated by the mean launch itself: still two launches, and `losses` / `scene_losses` get the bytes giga_train_loss
 * writes.  `acc`: GIGA_TRAIN_METRICS_BYTES of device memory owned by the caller, 8-byte aligned, sixteen 8-byte words:
 *   words 0-6  uint64  batches, examples, correct, tp, fp, fn, invalid
 *   word  7            reserved, left as found
 *   words 8-12 double  running sums of the batch means, in the order of scene_losses' columns (qual, rot, width, occ, all)
 *   words 13-15        reserved, left as found
 * The prediction of a scene is torch.round(qual), i.e. qual > 0.5f (half to even: 0.5 itself rounds to 0).  A scene is valid when
 * 0 <= qual <= 1 (so not NaN) and label is exactly 0 or 1; a valid scene adds to `examples` and to `correct` (pred == label), `tp`
 * (pred 1, label 1), `fp` (pred 1, label 0), `fn` (pred 0, label 1); any other scene adds 1 to `invalid` only.  Each call adds 1 to
 * `batches` and (double)losses[k] to sum k.  One workgroup, one lane updates `acc` with plain loads and stores: no atomics, so the
 * accumulator after a sequence of calls on one stream is a pure function of the inputs in call order.  The caller zeroes `acc` at
 * the start of an epoch.  Checks: those of giga_train_loss, and `acc` non-null and 8-byte aligned (-1); B == 0 returns 0 and leaves
 * `acc` untouched. */
#define GIGA_TRAIN_METRICS_BYTES 128
int giga_train_loss_metrics(const float* qual, const float* rot, const float* width, const float* occ_logits, const float* label,
                            const float* rot_targets, const float* width_target, const float* occ_target, int B, int M,
                            float* losses, float* scene_losses, void* acc, void* stream);

/* ---- the occupancy-only objective of the model giga_geo, scripts/train_giga_geo.py:152-165, and its epoch metrics (:52-57) -----
 * occ_logits [B][M] (raw; the sigmoid of `select` is part of these functions), occ_target [B][M].
 *   giga_train_occ_loss          : scene_losses [B] = mean_M BCE(sigmoid(z), t); loss [1] = their mean over the scenes.  The
 *                                  arithmetic is the occupancy term's of giga_train_loss: for the same logits and targets `loss`
 *                                  equals its losses[3] bit for bit.
 *   giga_train_occ_loss_backward : docc [B][M] = d loss / d occ_logits scaled by the device scalar *grad_loss; equals the docc of
 *                                  giga_train_loss_backward bit for bit.
 *   giga_train_occ_loss_metrics  : giga_train_occ_loss (the same bytes in `loss` and `scene_losses`, still two launches) that also
 *                                  adds the batch to the epoch accumulator `acc` (GIGA_TRAIN_METRICS_BYTES, 8-byte aligned, the
 *                                  layout above) -- counted in occupancy POINTS, B * M per call, as ignite's binary metrics over
 *                                  (round(sigmoid(z)), t) count them:
 *     word  0            batches, + 1
 *     words 1-6          examples, correct, tp, fp, fn, invalid, in points
 *     words 8 + 3, 8 + 4 double, both += (double)loss (the occupancy mean and the whole objective)
 *     words 7, 8-10, 13-15  left as found
 *   A point's prediction is p > 0.5f on the p = 1 / (1 + expf(-z)) the loss uses (half to even: p == 0.5 rounds to 0).  A point is
 *   valid when p is not NaN and t is exactly 0 or 1; any other point adds 1 to `invalid` only.  `scene_counts`: scratch of the
 *   caller, B * 6 32-bit words (per scene: examples, correct, tp, fp, fn, invalid).  One lane updates `acc` with plain loads and
 *   stores: no atomics, so the accumulator after a sequence of calls on one stream is a pure function of the inputs in call order.
 * Checks: B < 0 or M < 0, a null pointer, `acc` null or not 8-byte aligned: -1.  B == 0 returns 0 and leaves everything untouched;
 * M == 0 with B > 0 is -1 (an empty mean). */
int giga_train_occ_loss(const float* occ_logits, const float* occ_target, int B, int M, float* loss, float* scene_losses,
                        void* stream);
int giga_train_occ_loss_metrics(const float* occ_logits, const float* occ_target, int B, int M, float* loss, float* scene_losses,
                                uint32_t* scene_counts, void* acc, void* stream);
int giga_train_occ_loss_backward(const float* occ_logits, const float* occ_target, const float* grad_loss, int B, int M, float* docc,
                                 void* stream);

/* Adam over ONE flat fp32 buffer (the flattened parameters of the module, `net.flatten_parameters()`), in place: the update of
 * torch.optim.Adam (the reference's optimiser, scripts/train_giga.py:49; no amsgrad), formulas and order of torch/optim/adam.py:
 * m = lerp(m, g, 1 - beta1); v = beta2 v + (1 - beta2) g^2; p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps);
 * weight_decay (L2) adds weight_decay * p to g first.  `step` counts from 1.  One launch over the whole chip: torch's fused
 * multi-tensor kernel gives a single tensor one workgroup per 65 536 elements (98 us for these 581 863 parameters, this: ~5 us).
 * All four buffers must be 16-byte aligned (-1 otherwise). */
int giga_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                   double beta2, double eps, double weight_decay, int step, void* stream);

/* ---- grasp post-processing (src/vgn/detection_implicit.py:115-143 process, :87-97 bound, :146-174 select) -----
 * Replaces the host-side scipy stage that follows `predict` in VGNImplicit.__call__ (detection_implicit.py:55-58)
 * for B scenes at once; every volume is [B][R][R][R] float32 (rot: [B][R^3][4]) on the device.
 *   process : gaussian_filter(qual, sigma, mode="nearest"); qual = 0 where the voxel is not in the 2-iteration
 *             masked binary dilation of (tsdf > out_th) with mask ~(1e-3 < tsdf < out_th), or where
 *             width < min_width or width > max_width                      (detection_implicit.py:126-141)
 *   bound   : qual = 0 for x < lim_x, x >= R-lim_x, y < lim_y, y >= R-lim_y, z < lim_z; the caller computes
 *             lim = int(limit / voxel_size) as detection_implicit.py:89-91 does.  The limits are geometric: lim 0 means
 *             no margin on that axis, lim >= R zeroes the scene.  The reference differs at 0: its far margin is the slice
 *             qual_vol[-x_lim:] (detection_implicit.py:92-95), which for x_lim == 0 (voxel_size > 0.02) is the whole array,
 *             so its volume comes out all zero.  A caller that wants the reference's result passes lim = R on an x or y
 *             axis whose int(limit / voxel_size) is 0, as giga_amd/detection.py does; lim_z == 0 needs no such care
 *   select  : qual < low_th -> 0; if force_detection and no voxel >= threshold the scene is "best only" and
 *             the threshold is skipped, else qual < threshold -> 0; NMS with maximum_filter(size =
 *             max_filter_size, mode reflect); survivors are appended (unordered) to the candidate lists.
 * Outputs: qual_out [B][R^3] = the volume after process+bound (what the reference hands to select and to its
 * visualiser); counters [B][2] = {#voxels >= threshold (0 => best-only when force_detection), #candidates};
 * cand_index/score/width [B][cap], cand_rot [B][cap][4] hold the first min(#candidates, cap) survivors: flat
 * voxel index (x*R+y)*R+z, score, quaternion and width.  The caller sorts by descending score
 * (detection_implicit.py:166-171) and keeps one entry for a best-only scene. */
typedef struct GigaGraspParams {
    double gaussian_sigma;     /* 1.0 */
    float min_width;           /* 0.033 */
    float max_width;           /* 0.233 */
    float out_th;              /* VGNImplicit(out_th=0.5) */
    float low_th;              /* LOW_TH = 0.5, detection_implicit.py:15 */
    float threshold;           /* VGNImplicit(qual_th=0.9) */
    int lim_x, lim_y, lim_z;   /* int(0.02/voxel_size), int(0.02/voxel_size), int(0.055/voxel_size) */
    int max_filter_size;       /* 4 (8 when visualising) */
    int force_detection;
} GigaGraspParams;
size_t giga_grasp_workspace_bytes(int B, int R);
int giga_grasp_select(const float* tsdf, const float* qual, const float* rot, const float* width, int B, int R,
                      const GigaGraspParams* params, float* qual_out, int* counters, int cap, int* cand_index,
                      float* cand_score, float* cand_rot, float* cand_width, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- mesh extraction: marching cubes on B dense value grids (conv_onet/generation.py:360-393, extract_mesh with
 * vol_bound None; libmcubes.marching_cubes on the grid padded with -1e6) -----
 * grids [B][nx][ny][nz] float32 (occupancy logits), 2 <= n <= GIGA_MESH_MAX_N per axis (513 = 32 * 2^4 + 1, the largest MISE grid;
 * cell numbers, per-scene vertex and triangle numbers are 32-bit, the positions in the packed outputs 64-bit).  The padding by one sample of -1e6
 * on every side is virtual.  A corner counts as set when value <= iso; every crossed edge of the padded grid gives ONE
 * vertex at (iso - f1) / (f2 - f1) along it (evaluated in double, stored as float32), already in model coordinates
 * box_size * (g / (n - 1) - 0.5) with g the fractional grid index in [-1, n].  Triangles are wound as the reference's (the
 * normal points towards values <= iso).  Two phases, both asynchronous on `stream`, no allocation:
 *   count : classify + scan.  counts [B][2] int32 (device) = {#vertices, #triangles} of every scene; the workspace keeps
 *           the offsets and must reach the emit call unchanged (same grids, shape and iso).
 *   emit  : scenes packed back to back in scene order: vertices [cap_v][3] float32, triangles [cap_t][3] int32 whose
 *           entries count from the scene's OWN first vertex.  Within a scene the order is cell order (z fastest; edges
 *           along x, y, z inside a cell), so equal input gives equal bytes.  Nothing is written at or beyond a capacity;
 *           shortfall [2] int32 (device, may be NULL) receives the number of vertices and triangles that did not fit
 *           (0, 0 when everything was written).
 * Errors: -1 null grid / workspace / counts, n < 2 or n > GIGA_MESH_MAX_N, NaN iso, B (nx+1)(ny+1)(nz+1) >= 2^31;
 * -4 workspace too small; -6 null output with a non-zero capacity; -7 B > GIGA_MAX_SCENES. */
#define GIGA_MESH_MAX_N 513
size_t giga_mesh_workspace_bytes(int B, int nx, int ny, int nz);
int giga_mesh_count(const float* grids, int B, int nx, int ny, int nz, double iso, void* workspace, size_t workspace_bytes,
                    int32_t* counts, void* stream);
int giga_mesh_emit(const float* grids, int B, int nx, int ny, int nz, double iso, double box_size, const void* workspace,
                   size_t workspace_bytes, float* vertices, size_t cap_v, int32_t* triangles, size_t cap_t, int32_t* shortfall,
                   void* stream);

/* ---- mesh simplification: the greedy quadric edge collapse of utils/libsimplify/Simplify.h, as conv_onet/generation.py:417-420
 * calls it (simplify_mesh(mesh, simplify_nfaces, 5.)); added within ABI 3 -----
 * B meshes packed back to back in the layout giga_mesh_emit produces: vertices [.][3] float32 (vertices_f64 = 0; widened exactly)
 * or float64 (vertices_f64 = 1) and triangles [.][3] int32 (device), a mesh's triangles counting from its OWN first vertex;
 * vertex_offsets, triangle_offsets [B+1] int32 and targets [B] int32 are HOST arrays.  Mesh b is simplified to at most targets[b]
 * faces exactly as `Simplify::simplify_mesh(targets[b], agressiveness)` on value-initialised records does it -- float64 in the
 * header's order of operations, no fused multiply-add; up to 100 iterations, a mesh that cannot reach its target ends above it;
 * a mesh with no more faces than its target only loses its unreferenced vertices.  All meshes of a call share their rounds (a
 * batch costs the rounds of its slowest mesh).  Outputs (device, caller-owned, at least as large as the inputs): out_vertices
 * [.][3] float64 and out_triangles [.][3] int32, meshes back to back, faces counting from the mesh's own first vertex;
 * out_counts [B][2] int32 = {#vertices, #triangles}.  stats (HOST, may be NULL) [B][4] int32 = {iterations, rounds, passes run
 * again to meet the face budget exactly, rebuilds of the reference lists}.  ref_extra: entries of the per-vertex reference lists
 * beyond the 3 F a mesh starts with, per mesh; < 0 = the default 3 F + GIGA_SIMPLIFY_MIN_REF_EXTRA; a smaller value (at least
 * GIGA_SIMPLIFY_MIN_REF_EXTRA) only makes the lists be rebuilt more often, the result is the same.
 * The call drives the rounds itself: it synchronises `stream` (the pending counts are read back every few rounds) and has
 * returned its result when it returns.  No allocation: everything lives in the workspace.
 * Errors: -1 negative B, offsets that do not start at 0 or decrease, a target < 0, NaN agressiveness, vertices_f64 not 0 / 1,
 * 0 <= ref_extra < GIGA_SIMPLIFY_MIN_REF_EXTRA, more than GIGA_SIMPLIFY_MAX_FACES vertices or faces in the call, null inputs /
 * targets / workspace; -4 workspace too small; -6 null output; -7 B > GIGA_MAX_SCENES; -11 a face index outside its mesh's
 * vertex range (found by a check launch before anything else runs, nothing is written to the outputs); -12 a pass exceeded its
 * bound of one round per candidate, or ref_extra is too small for a single collapse.  B = 0 returns 0. */
#define GIGA_SIMPLIFY_MIN_REF_EXTRA 64
#define GIGA_SIMPLIFY_MAX_FACES 0x0FFFFFFF
size_t giga_simplify_workspace_bytes(int B, int n_vertices, int n_triangles, int ref_extra);
int giga_mesh_simplify(const void* vertices, int vertices_f64, const int32_t* vertex_offsets, const int32_t* triangles,
                       const int32_t* triangle_offsets, const int32_t* targets, int B, double agressiveness, int ref_extra,
                       double* out_vertices, int32_t* out_triangles, int32_t* out_counts, int32_t* stats, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- MISE: the sparse value grid of conv_onet/generation.py:125-142 (utils/libmise/mise.pyx), B independent octrees (added within
 * ABI 3) -----
 * R = resolution0 << depth, N = R + 1 <= GIGA_MISE_MAX_N samples per axis, depth >= 1; sample (i, j, k) has the linear index
 * (i N + j) N + k.  The workspace (giga_mise_workspace_bytes(B, resolution0, depth)) holds the whole state: a known / unknown mark
 * and a value per sample, and the leaves of the octree (a voxel of level l has edge 1 << (depth - l)).  All calls are asynchronous
 * on `stream` and allocate nothing; scene b of a batch gives the bytes of a call on b alone.
 *   init     : the resolution0^3 voxels of level 0 are leaves, the (resolution0 + 1)^3 coarse lattice points unknown.
 *   count    : counts [B] int32 (device) = number of unknown points of every scene (MISE.query()'s length).  The workspace keeps
 *              the offsets and must reach emit and update unchanged.
 *   emit     : query [B][cap] int32 = the unknown points of scene b as linear indices in ASCENDING order (count / scan / emit, no
 *              atomic append: equal state gives equal bytes).  Nothing is written at or beyond cap; shortfall [B] int32 (device,
 *              may be NULL) receives the number of indices of each scene that did not fit.  With `points` [B][cap][3] float32 not
 *              NULL, entry i of scene b also receives (lin[x], lin[y], lin[z]) of its sample, `lin` [N] float32 (device) being the
 *              caller's per-axis table; entries at and beyond the scene's count repeat its first point (sample 0 when it has
 *              none), so that one decoder launch over [B][cap] reads valid points only.
 *   update   : values [B][cap] float32 are the values of the list that emit wrote (the first min(count, cap) of each scene count):
 *              those points become known.  Then every leaf of level < depth for which a known point p of its CLOSED cube
 *              (loc <= p <= loc + edge on all three axes) has (double)v >= threshold and one has (double)v <= threshold --
 *              judged on all known points, before any subdivision of this round -- becomes an inner node with 8 leaf children, and
 *              those of the children's 27 lattice points that did not exist are created unknown (mise.pyx:87-128, 184-280).
 *   to_dense : grid [B][N][N][N] float32: the value of every created point (0 for one that is still unknown); then a sample without
 *              value takes that of i-1 along x, then those still without take j-1 along y, then k-1 along z (mise.pyx:130-164).
 * The caller loops count -> (copy of the B counts: the only device-to-host traffic of a round) -> emit -> decoder -> update until
 * every count is 0, even if a leaf created in the last round would be subdivided by the next: that is what the reference does.
 * Errors: -1 resolution0 < 1, depth < 1, N > GIGA_MISE_MAX_N, B N^3 >= 2^31, B cap >= 2^31, NaN threshold, null workspace / counts /
 * grid / values / lin with points; -4 workspace too small; -6 null query with cap > 0; -7 B > GIGA_MAX_SCENES.  B = 0 returns 0. */
#define GIGA_MISE_MAX_N 513
size_t giga_mise_workspace_bytes(int B, int resolution0, int depth);
int giga_mise_init(int B, int resolution0, int depth, void* workspace, size_t workspace_bytes, void* stream);
int giga_mise_count(int B, int resolution0, int depth, void* workspace, size_t workspace_bytes, int32_t* counts, void* stream);
int giga_mise_emit(int B, int resolution0, int depth, const void* workspace, size_t workspace_bytes, int32_t* query, size_t cap,
                   int32_t* shortfall, const float* lin, float* points, void* stream);
int giga_mise_update(const float* values, const int32_t* query, size_t cap, int B, int resolution0, int depth, double threshold,
                     void* workspace, size_t workspace_bytes, void* stream);
int giga_mise_to_dense(int B, int resolution0, int depth, const void* workspace, size_t workspace_bytes, float* grid, void* stream);

/* ---- mesh evaluation on ragged batches (vgn/ConvONets/eval.py:28-232, utils/libmesh/inside_mesh.py) -----
 * B scenes packed back to back, the layout giga_mesh_emit produces: every `*_offsets` argument is a HOST array of B + 1 int32
 * that starts at 0 and never decreases; scene b owns rows offsets[b] .. offsets[b+1]-1 of the DEVICE array it belongs to, and a
 * scene's triangles [.][3] int32 count from the scene's OWN first vertex.  The offsets are read (and copied into the workspace)
 * before a call returns.  Caller-owned buffers, no allocation, asynchronous on `stream`; every argument is checked before the
 * first HIP call.  No floating-point atomics: equal input gives equal bytes, and a batch gives scene b the bytes of a call on
 * scene b alone.
 * Errors (all three): -1 negative B / count, null input or workspace, offsets that do not start at 0 or decrease, resolution
 * outside 2 .. GIGA_CONTAINS_MAX_RESOLUTION, B n >= 2^31; -4 workspace too small; -6 null output; -7 B > GIGA_MAX_SCENES.
 *
 * giga_nn_query: for every source point [.][3] float32 the nearest target point of the SAME scene, exact brute force on float32
 * differences, d2 = (dx*dx + dy*dy) + dz*dz with one rounding per operation.  dist [n_src] float32 = sqrt(d2) (Euclidean),
 * idx [n_src] int32 relative to the scene's first target; ties go to the lowest index; a scene without targets (or whose
 * distances are all NaN) gives dist = +inf, idx = -1.  workspace: giga_nn_query_workspace_bytes(B, src_offsets[B]).
 *
 * giga_mesh_sample: n points per scene, uniform over the scene's surface.  Sample i of scene b draws one Philox-4x32-10 block
 * with counter (i, first_scene + b, 0, 0) (first_scene >= 0: a call on scene b alone with first_scene = b repeats the batch's
 * bytes) and key (seed & 0xffffffff, seed >> 32); r0, r1, r2 = words 0, 1, 2 times 2^-32 (double).  Face
 * areas 0.5 |cross(v1 - v0, v2 - v0)| and their inclusive prefix sums inside the scene are double; the sample lies on the first
 * face whose prefix sum exceeds r0 * total (a face without area is never chosen; neither is one with an index outside the
 * scene's vertices or a non-finite area) at (1 - sqrt r1) v0 + sqrt r1 (1 - r2) v1 + sqrt r1 r2 v2, evaluated in double.
 * Outputs at row b * n + i: points [B n][3] float32, face [B n] int32 (relative to the scene's first face), normals [B n][3]
 * float32 = cross(v1 - v0, v2 - v0) normalised in double.  counts [B] int32 (device) = n, or 0 for a scene without faces or with
 * total area 0 (or not finite): NOTHING is written to that scene's rows.  workspace:
 * giga_mesh_sample_workspace_bytes(B, triangle_offsets[B]).
 *
 * giga_mesh_contains: inside [n_points] uint8 = 1 where the query point (points [.][3] FLOAT64, so that float32 and float64 callers
 * both get the reference's arithmetic) lies inside its scene's mesh, as MeshIntersector(mesh, resolution).query decides it, in
 * double and in the reference's operand order without fused multiply-adds: triangles and points rescaled by scale =
 * (resolution - 1) / (bbox_max - bbox_min), translate = 0.5 - scale bbox_min (the scene's own box over the vertices its faces
 * use); candidates = the triangles whose clamped cell range holds the point's cell (triangle_hash.pyx); a candidate is hit when
 * det != 0 and 0 < u, v, u + v < |det|; inside = both (#hits with depth >= p.z |n.z|) and (#hits with depth < p.z |n.z|) odd.  A
 * scene without faces has no inside.  workspace: giga_mesh_contains_workspace_bytes(B, triangle_offsets[B], point_offsets[B]). */
#define GIGA_CONTAINS_MAX_RESOLUTION 32768
size_t giga_nn_query_workspace_bytes(int B, int n_src);
int giga_nn_query(const float* src, const int32_t* src_offsets, const float* tgt, const int32_t* tgt_offsets, int B, float* dist,
                  int32_t* idx, void* workspace, size_t workspace_bytes, void* stream);
size_t giga_mesh_sample_workspace_bytes(int B, int n_triangles);
int giga_mesh_sample(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                     int B, int n, uint64_t seed, int first_scene, float* points, int32_t* face, float* normals, int32_t* counts,
                     void* workspace, size_t workspace_bytes, void* stream);
size_t giga_mesh_contains_workspace_bytes(int B, int n_triangles, int n_points);
int giga_mesh_contains(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                       const double* points, const int32_t* point_offsets, int B, int resolution, uint8_t* inside, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- mesh against mesh: do two bodies' surfaces intersect? (src/vgn/simulation.py:118-143 needs it; added within ABI 3) -----
 * M bodies packed back to back in the ragged layout of the mesh-evaluation entries above: vertices [.][3] float32 in world space
 * and triangles [.][3] int32 counting from the body's OWN first vertex, both on the device; vertex_offsets and triangle_offsets
 * are HOST arrays of M + 1 int32, read (and copied into the workspace) before the call returns.  pairs is a HOST array
 * [P][2] int32 of body indices, copied into the workspace before the call returns.  hit [P] uint8 (device) is the output.
 * Caller-owned buffers, no allocation, asynchronous on `stream`; every argument is checked before the first HIP call.
 * workspace: giga_mesh_collide_workspace_bytes(M, P) (0 for arguments the call rejects).
 * Errors: -1 negative count, null input or workspace, offsets that do not start at 0 or decrease, a pair index outside
 * 0 .. M-1, a pair with a == b; -4 workspace too small; -6 null hit with P > 0; -7 M > GIGA_MAX_SCENES.  M = 0 or P = 0 returns 0.
 *
 * All arithmetic is in double with one IEEE rounding per operation and no contraction.
 *   Orientation.  orient(a, b, c, d) uses u = b - a, v = c - a, w = d - a.  These differences are exact, because the vertices
 *     are float32.  Its value is (u.x*(v.y*w.z - v.z*w.y) - u.y*(v.x*w.z - v.z*w.x)) + u.z*(v.x*w.y - v.y*w.x), in exactly this
 *     order.
 *   Segment against triangle.  Segment (p, q) hits triangle (a, b, c) under these rules, with sp = orient(a,b,c,p) and
 *     sq = orient(a,b,c,q): it misses when sp and sq are both > 0 or both < 0; it misses when both are exactly 0 (a segment in
 *     the triangle's plane: coplanar contact is not detected); it misses when either is NaN; otherwise it hits iff
 *     orient(p,q,a,b), orient(p,q,b,c) and orient(p,q,c,a) are all >= 0 or all <= 0.  Zero counts as touching, which is
 *     giga_depth_render's watertight rule.
 *   Triangle against triangle.  Triangles A and B intersect iff one of A's edges (v0,v1), (v1,v2), (v2,v0) hits B, or one of B's
 *     edges hits A.  A triangle with an index outside its body or a non-finite vertex intersects nothing.
 *   Pair.  hit[p] = 1 iff some triangle of body a intersects some triangle of body b, else 0.  The rule is symmetric, so
 *     hit(a,b) == hit(b,a).  There are no floating-point atomics.  Equal input gives equal bytes.  A pair's byte does not depend on
 *     the other pairs of the call or on their order.  Surface intersection only: a body that lies wholly inside another is not
 *     detected (giga_mesh_contains on one of its vertices answers that).
 * Culling, part of the definition: a body's box is the float32 box over the vertices of its triangles that can intersect
 * anything (exact: min and max do not round).  A pair whose boxes are disjoint (or one of whose bodies has no such triangle) is
 * 0, and only triangles whose own box meets the intersection of the two bodies' boxes (closed intervals) are tested against each
 * other.  Triangles that are left out cannot meet the other body's surface; the determinants of such a pair are never taken. */
size_t giga_mesh_collide_workspace_bytes(int M, int P);
int giga_mesh_collide(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                      int M, const int32_t* pairs, int P, uint8_t* hit, void* workspace, size_t workspace_bytes, void* stream);

/* ---- geometry scoring (scripts/eval_geometry_voxel.py, src/vgn/dataset_voxel_occ.py:109-128; added within ABI 3) -----
 * Caller-owned buffers, no allocation, asynchronous on `stream`, every argument checked before the first HIP call, no
 * floating-point atomics: equal input gives equal bytes.  Errors: -1 negative count, null input or workspace, offsets that do not
 * start at 0 or decrease, a number that is not finite, size 0, a negative scene or first index, a NaN threshold, both or neither of
 * logits / pred; -4 workspace too small; -6 null output; -7 B > GIGA_MAX_SCENES.
 *
 * giga_roi_points: the query points of DatasetVoxelOccGeoROI.__getitem__ for a ragged batch of scenes.  All grasp arrays are HOST
 * arrays (copied into the workspace before the call returns): grasps [G][13] float64 = the rotation matrix R row-major (9), the
 * box origin pos = xyz + R (0,0,1) finger_depth (3) and the width; point_offsets [G + 1] int32, the prefix of the per-grasp point
 * counts over the whole call (a grasp with count 0 emits nothing); grasp_scene [G] the index of the grasp's scene in the data set;
 * grasp_first [G] the index inside its scene of the grasp's first point.  Point j of a scene (j counts through the scene's grasps)
 * draws two Philox-4x32-10 blocks with counters (j, scene, 0, 0x524F49) and (j, scene, 1, 0x524F49) and key (seed & 0xffffffff,
 * seed >> 32); u0, u1 = words (0,1), (2,3) of the first block and u2 = words (0,1) of the second, each 53 bits in (0, 1)
 * (((hi >> 5) << 26 | lo >> 6) 2^-53, 2^-54 in place of 0).  So a point depends on (seed, scene, j) alone, not on the batch, the
 * launch or the chunking.  In float64, one rounding per operation, no fused multiply-add:
 *     x = (u0 - 1) e,  y = (u1 - 0.5) width,  z = (u2 - 1) e,  e = finger_depth * roi_scale
 *     world [n][3] float64 = ((R[.][0] x + R[.][1] y) + R[.][2] z) + pos          (what the containment test sees)
 *     normalised [n][3] float32 = float32(world / size - 0.5), rounded once
 * n = point_offsets[G].  workspace: giga_roi_points_workspace_bytes(G).
 *
 * giga_occ_confusion: counts [B][4] uint64 (device) = [tp, fp, fn, tn] of every scene of a ragged batch (offsets: HOST, B + 1
 * int32); an empty scene leaves zeros.  target [n] uint8: occupied where not 0.  The prediction is EITHER pred [n] uint8 (occupied
 * where not 0; logits null) OR logits [n] float32 (pred null) with
 *     predicted = (double)logit > logit_threshold,      logit_threshold = log(th / (1 - th)) computed by the caller in float64.
 * A NaN logit predicts false.  This is the library's own definition of "sigmoid(logit) > th": the reference evaluates
 * torch.sigmoid in float32 and compares with th, which decides differently only for logits within float32 rounding of the
 * boundary (sigmoid(logit) rounds onto or across th there).  Integer atomics: the counts do not depend on the order of the
 * additions.  workspace: giga_occ_confusion_workspace_bytes(B). */
size_t giga_roi_points_workspace_bytes(int n_grasps);
int giga_roi_points(const double* grasps, const int32_t* point_offsets, const int32_t* grasp_scene, const int32_t* grasp_first,
                    int n_grasps, uint64_t seed, double finger_depth, double roi_scale, double size, double* world,
                    float* normalised, void* workspace, size_t workspace_bytes, void* stream);
size_t giga_occ_confusion_workspace_bytes(int B);
int giga_occ_confusion(const float* logits, const uint8_t* pred, double logit_threshold, const uint8_t* target,
                       const int32_t* offsets, int B, uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---- grasp candidates from the oriented cloud (scripts/generate_data_parallel.py:133-161: sample_grasp_point and the frame and yaw
 * angles of evaluate_grasp_point; added within ABI 3) -----
 * giga_grasp_candidates draws K candidates for each of B scenes.  points, normals [n][3] float32 (device) are what
 * giga_tsdf_cloud_emit_oriented wrote, scenes back to back.  HOST arrays, validated before the first HIP call and copied into the
 * workspace before the call returns: offsets [B + 1] int32 (start at 0, never decrease; n = offsets[B]), scene_ids [B] uint32,
 * lower [3] and upper [3] float64, yaw_table [Y][2] float64 with row j = (sin(yaw_j / 2), cos(yaw_j / 2)), 1 <= Y <= 32: the caller
 * computes it (the reference's angles are np.linspace(0, pi, Y)), so that no sine or cosine is evaluated on the device.
 * Everything below is float64 with one rounding per operation and no fused multiply-add; P and N are a point and its normal widened
 * to float64.
 *
 * Eligible points.  A point is eligible when lower_c <= P_c <= upper_c for c = x, y, z (both ends included, Open3D's crop),
 * N_z > -0.1 (generate_data_parallel.py:141), d = (N_x N_x + N_y N_y) + N_z N_z > 0, and all six numbers are finite.  The eligible
 * points of a scene are counted and listed in ascending point order by prefix sums, without atomics; counts [B] int32 (device)
 * receives the number E_b.
 *
 * Draw of candidate k of scene b: one Philox-4x32-10 block with counter (k, scene_ids[b], 0, 0x47525350) and key
 * (seed & 0xffffffff, seed >> 32).  e = (uint64(word 0) E_b) >> 32 picks the e-th eligible point; index [B][K] int32 (device)
 * receives its index inside the scene.  u = words (2, 3) as 53 bits in (0, 1): ((w2 >> 5) << 26 | w3 >> 6) 2^-53, 2^-54 in place
 * of 0.  lo = -(eps finger_depth), hi = (1 + eps) finger_depth, depth = lo + (hi - lo) u, pos [B][K][3] float64 (device) =
 * P + N depth per component.  The reference redraws until N_z > -0.1; a uniform draw over the eligible points has the same
 * distribution and always ends.  A scene with E_b = 0 gets counts[b] = 0 and its rows of pos, quat and index are left as they were.
 * A candidate depends on (seed, scene id, k) and on the scene's own cloud alone, not on the batch or the launch.
 *
 * Frame (generate_data_parallel.py:149-155).  z = (-N) / sqrt(d) per component.  x = (1, 0, 0); if
 * | |x . z| - 1 | <= 1e-8 + 1e-4 (np.isclose(.., 1.0, 1e-4); x . z = (x_0 z_0 + x_1 z_1) + x_2 z_2), x = (0, 1, 0).  y = z cross x,
 * then x = y cross z, a cross b = (a_1 b_2 - a_2 b_1, a_2 b_0 - a_0 b_2, a_0 b_1 - a_1 b_0).  The reference hands the matrix with the
 * columns (x, y, z) to scipy's Rotation.from_matrix although x and y are orthogonal but not of unit length; scipy (1.15.3) returns
 * the rotation of the matrix with every column normalised, so x and y are each divided by sqrt((a_0 a_0 + a_1 a_1) + a_2 a_2) here
 * and the grasp's z axis is -N / |N|.  With M[r][0] = x_r, M[r][1] = y_r, M[r][2] = z_r and t = (M00 + M11) + M22, the
 * quaternion (xyzw) takes the branch of the first largest of (M00, M11, M22, t):
 *     M00:  ((1 - t) + 2 M00,  M10 + M01,  M20 + M02,  M21 - M12)
 *     M11:  (M01 + M10,  (1 - t) + 2 M11,  M21 + M12,  M02 - M20)
 *     M22:  (M02 + M20,  M12 + M21,  (1 - t) + 2 M22,  M10 - M01)
 *     t:    (M21 - M12,  M02 - M20,  M10 - M01,  1 + t)
 * and is divided by sqrt(((q_0 q_0 + q_1 q_1) + q_2 q_2) + q_3 q_3).  Its sign is not canonicalised.
 * Yaw j with (s, c) = yaw_table[j]:  quat [B][K][Y][4] float64 (device) =
 *     (q_0 c + q_1 s,  q_1 c - q_0 s,  q_2 c + q_3 s,  q_3 c - q_2 s)          the product q (0, 0, s, c).
 *
 * One workgroup per scene; caller-owned buffers, asynchronous on `stream`, equal input gives equal bytes.  workspace:
 * giga_grasp_candidates_workspace_bytes(B, offsets[B], Y).  Errors: -1 negative B or K, Y outside 1 .. 32, a bound, finger_depth,
 * eps or table entry that is not finite, offsets that do not start at 0 or decrease, null host array, null points or normals with
 * n > 0, null workspace; -4 workspace too small; -6 null output; -7 B > GIGA_MAX_SCENES.  B = 0 or K = 0 returns 0. */
#define GIGA_CANDIDATES_MAX_ROTATIONS 32
size_t giga_grasp_candidates_workspace_bytes(int B, int n_points, int n_rotations);
int giga_grasp_candidates(const float* points, const float* normals, const int32_t* offsets, const uint32_t* scene_ids, int B, int K,
                          const double* lower, const double* upper, double finger_depth, double eps, const double* yaw_table,
                          int n_rotations, uint64_t seed, double* pos, double* quat, int32_t* index, int32_t* counts, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- output side: grasp affordance of a scene mesh (src/vgn/utils/visual.py:22-98, affordance_visual; added within ABI 3) -----
 * Colours every face of B scene meshes by the grasp quality predicted near it.  qual [B][R^3] float32 is the volume after process
 * and bound (the qual_out of giga_grasp_select), rot [B][R^3][4] float32 the quaternions (xyzw), voxel (i, j, k) at i R^2 + j R + k.
 * Two calls, both asynchronous on `stream`, without allocation and without atomics; equal input gives equal bytes, and a batch
 * gives scene b the bytes of a call on scene b alone.
 *
 * giga_affordance_points: the voxels with qual > float(th) (a float32 comparison), in ascending voxel order, as points [B][R^3][4]
 * double (x, y, z, q); counts[b] rows of scene b are written, the rest is left as it was.
 *   position   (lin[i], lin[j], lin[k]) in double, lin = np.linspace(0, size, R): lin[t] = t (size / (R - 1)), lin[R - 1] = size.  (The
 *              spacing is size / (R - 1), not the planner lattice's size / R: the reference's choice, kept.)
 *   move_center != 0 adds the third column of the rotation matrix, computed in float32 with one rounding per operation:
 *              zx = (2 r0) r2 + (2 r1) r3, zy = (2 r1) r2 - (2 r0) r3, zz = (1 - (2 r0) r0) - (2 r1) r1,
 *              off = (z float(finger_depth)) float(finger_offset); off is widened to double and added to the position.
 *   q          the float32 quality widened to double.
 *
 * giga_affordance_faces: the meshes are packed back to back in the ragged layout of giga_depth_render (vertices [.][3] float32,
 * triangles [.][3] int32 counting from the scene's own first vertex, both on the device; vertex_offsets and triangle_offsets
 * [B+1] int32 on the HOST, copied into the workspace before the call returns).  points and counts are what
 * giga_affordance_points wrote (device).  Per face, in double, one rounding per operation:
 *   centre     ((v0 + v1) + v2) / 3 from the float32 vertices;
 *   dist       sqrt(((dx dx) + (dy dy)) + (dz dz)), d = centre - point, the root correctly rounded;
 *   over the P = counts[b] points of the scene
 *     GIGA_AFFORDANCE_MAX      a = max_p (dist <= rad ? q_p : 0)
 *     GIGA_AFFORDANCE_SOFTMAX  w_p = dist <= rad ? exp(q_p temp) : 0,  a = (sum w_p q_p) / (sum w_p + 1e-5)
 *     GIGA_AFFORDANCE_MEAN     w_p = exp(-dist temp),                   a = (sum w_p q_p) / (sum w_p)       (0 / 0 = NaN)
 *              the sums taken in ascending point order;
 *   affordance a = (min(max(a, th), 1) - th) / (1 - th), NaN staying NaN -> affordance [F] double;
 *   colour     matplotlib's 'Reds' with its 256 entries at x = (a a) (a a): entry min(int(256 x), 255) as rint(255 c), alpha 255;
 *              NaN gives (0, 0, 0, 0) -> rgba [F][4] uint8.  giga_affordance_colormap writes the table ([256][4], host memory).
 * A scene without points (P = 0) gets affordance NaN and the colour (102, 102, 102, 255) on every face; a face with a vertex
 * index outside its scene gets NaN and (0, 0, 0, 0).
 * GIGA_AFFORDANCE_MAX walks a uniform cell grid over the points instead of all of them when that grid has at least 3 cells per
 * axis and R^3 <= 2^20; the results are the same bytes.  GIGA_AFFORDANCE_DENSE, OR-ed into `aggregation`, keeps the dense form
 * (what the tests compare the grid against).
 * workspace: giga_affordance_workspace_bytes(B, R, n_faces_total) for both calls (0 for arguments the calls reject).
 * Errors: -1 null params, B < 0, R < 2 or R > GIGA_TSDF_MAX_R, an unknown aggregation, a parameter that is not finite, offsets
 * that are null, do not start at 0 or decrease, a null pointer to a non-empty array, null workspace; -4 workspace too small;
 * -7 B > GIGA_MAX_SCENES.  B = 0 returns 0. */
#define GIGA_AFFORDANCE_MAX 0
#define GIGA_AFFORDANCE_SOFTMAX 1
#define GIGA_AFFORDANCE_MEAN 2
#define GIGA_AFFORDANCE_DENSE 256
typedef struct GigaAffordanceParams {
    double size, th, temp, rad, finger_depth, finger_offset;
    int32_t move_center;
    int32_t aggregation;
} GigaAffordanceParams;
size_t giga_affordance_workspace_bytes(int B, int R, int n_faces_total);
int giga_affordance_points(const float* qual, const float* rot, int B, int R, const GigaAffordanceParams* params, double* points,
                           int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int giga_affordance_faces(const float* vertices, const int32_t* vertex_offsets, const int32_t* triangles, const int32_t* triangle_offsets,
                          const double* points, const int32_t* counts, int B, int R, const GigaAffordanceParams* params,
                          double* affordance, uint8_t* rgba, void* workspace, size_t workspace_bytes, void* stream);
void giga_affordance_colormap(uint8_t* rgba);

/* Number of kernel launches the library has enqueued in this process so far (all streams): the difference around a call is
 * that call's launch count.  Diagnostic only. */
unsigned long long giga_launch_count(void);
/* Measurement hook for ANY launch of the library (bench.py: the kernels of the training step): the launch whose ordinal -- the value
 * giga_launch_count() returns right after it was enqueued -- equals `ordinal` is bracketed by ev_start / ev_stop (giga_event_create)
 * on the stream it is launched on; giga_launch_probe_name() then returns the kernel expression of that launch site.  ordinal 0
 * disarms.  One probe per process; not for concurrent use from several host threads. */
int giga_launch_probe(unsigned long long ordinal, void* ev_start, void* ev_stop);
const char* giga_launch_probe_name(void);
/* The library's per-device bookkeeping -- which kernels have had their dynamic-LDS limit raised, which streams have a persistent
 * U-Net launch in flight -- outlives a hipDeviceReset(), the state it describes does not.  A host that resets a device calls this
 * before its next call into the library (no GPU work is enqueued; safe to call at any time when no call is in progress). */
void giga_forget_device_state(void);
/* How the LAST encoder call of this process ran its U-Net (diagnostic: tests pin the launch-form and kernel flags to it):
 * an OR of GIGA_PATH_PERSISTENT (one persistent launch; else one launch per layer), GIGA_PATH_CONV32 (conv32 kernels; else
 * conv16), GIGA_PATH_FUSED_PAIRS (the persistent conv32 launch ran its same-resolution layer pairs fused) and GIGA_PATH_WINOGRAD
 * (precision 0: 3x3 layers ran as Winograd F(2x2, 3x3)). */
#define GIGA_PATH_PERSISTENT 1
#define GIGA_PATH_CONV32 2
#define GIGA_PATH_FUSED_PAIRS 4
#define GIGA_PATH_WINOGRAD 8
int giga_encoder_last_path(void);
/* How the LAST giga_backward call of this process ran the U-Net's data-gradient chain (diagnostic, read-only: tests pin the launch
 * form to it; the chain is always one launch per stage): an OR of GIGA_BWD_PATH_WINOGRAD (fp32: the 3x3 layers' data gradients as
 * Winograd F(2x2, 3x3)) and GIGA_BWD_PATH_BF16 (GIGA_BF16_CONVS: bf16 operands).  0 before the first call.
 * GIGA_BWD_PATH_PERSISTENT is no longer reported (the chain as one persistent launch was removed); its value stays reserved. */
#define GIGA_BWD_PATH_PERSISTENT 1
#define GIGA_BWD_PATH_WINOGRAD 2
#define GIGA_BWD_PATH_BF16 4
int giga_backward_last_path(void);
/* ---- measurement hooks (bench.py roofline): HIP events recorded on `stream` right before and
 * after ONE kernel launch, so the kernel's duration is measured live on the stream it runs on.
 * probe_stage: 0 conv_in+project, 1 plane_finalize, 2..14 = U-Net layers 0..12 (giga_layout.h kConv), 15 = the whole U-Net.
 * The decoder variant brackets the single fused decoder launch. */
void* giga_event_create(void);
void giga_event_destroy(void* ev);
int giga_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);   /* synchronises on ev_stop */
int giga_event_record(void* ev, void* stream);   /* bench.py: an EMPTY bracket measures what the two records themselves cost */
int giga_encoder_forward_probe(const float* tsdf, const void* packed, void* planes_nhwc, float* planes_nchw,
                               int B, int precision, void* workspace, size_t workspace_bytes, void* stream,
                               int probe_stage, void* ev_start, void* ev_stop);
int giga_decoder_forward_probe(const void* planes_nhwc, const float* p, const void* packed, int head_mask,
                               float* qual, float* rot, float* width, float* occ, int B, int N,
                               int precision, int post, void* stream, void* ev_start, void* ev_stop);

#ifdef __cplusplus
}
#endif
#endif /* GIGA_HIP_H_ */
