// The launchers of the training decoder (giga_decoder_bwd.hip, giga_decoder_train16.hip) as their callers (giga_capi.hip's
// giga_backward, giga_decoder.hip's forward entry point) see them: ONE declaration, which the defining files include too.  Each
// launches what its DecBwdCall (giga_dec_bwd_plan.h) says; `scratch` is the call's scratch base.
#pragma once
#include <hip/hip_runtime.h>

#include "giga_dec_bwd_plan.h"
#include "giga_side.h"

namespace giga {

// partial weight-gradient tiles of the fused bf16 backward launches of one step, waiting for dect_reduce_kernel
struct DectPending { const float* partial[NHEADS]; int nwg[NHEADS]; int head_id[NHEADS]; int n; };

// fp32: decoder_bwd_kernel on the caller's stream, then the weight-gradient launches (they wait for its row arrays only) on the
// device's side stream where `side` is given.  gplanes: added to with atomics; nullptr = the head is detached from the planes;
// with dcbuf (the plan's gather) the kernel leaves its dc rows there instead and launch_plane_gather follows it, in front of the
// weight gradients as the plan's order has it.
int launch_decoder_backward(const DecBwdCall& c, const float* planes, const float* p, const uint8_t* blob, const uint8_t* bwd_blob,
                            int head_mask, const float* const* outs, const float* const* douts, float* gplanes, float* dcbuf,
                            float* grads, int head_present, float* scratch, int B, int N, hipStream_t s, SideScope* side);
// plane gradients of a one-head call from its dc rows [B * N][96]: WRITTEN, so the call runs before those that add with atomics
int launch_plane_gather(const float* dcbuf, const float* p, float* gplanes, int B, int N, hipStream_t s);
// bf16: one fused launch per call; the reduce is enqueued by launch_dect_reduce once all calls of the step have run
int launch_dect_forward(const float* planes, const float* p, const uint8_t* blob, int head_mask, float* const* outs, int B, int N,
                        int post, hipStream_t s);
int launch_dect_backward(const DecBwdCall& c, const float* planes, const float* p, const uint8_t* blob, const uint8_t* bwd_blob,
                         int head_mask, const float* const* outs, const float* const* douts, float* gplanes, float* dcbuf,
                         float* scratch, int B, int N, hipStream_t s, DectPending* pend);
int launch_dect_reduce(const DectPending& pend, float* grads, int head_present, hipStream_t s);

}  // namespace giga
