"""Depth-sensor noise on the device: the dex, trans and norm models of the reference's `vgn.utils.misc.apply_noise`
(reference src/vgn/utils/misc.py:18-69), which the reference applies to every depth image before fusion
(scripts/construct_dataset_parallel.py:21, simulation.py:176), through `giga_depth_noise` (csrc/giga_noise.hip; semantics and the
draw layout in include/giga_hip.h).

The reference draws from numpy's global generator.  Here every draw is a counter-based Philox block keyed by `seed` and
addressed by the image's 64-bit id, so an image's noise depends only on (seed, id, shape, model, parameters): not on the batch it
sits in, and a data set can be rebuilt scene by scene.  `DepthNoise` objects are what the `noise=` arguments of
`perception.construct_dataset`, `render.acquire_tsdf(s)` and `VGNImplicit.plan_from_depth` take.  There is no CPU path: CPU
tensors raise `GigaHipError`."""
import numpy as np
import torch

from . import _capi

PARAMS = {"dex": (("gamma_shape", 1000), ("gamma_scale", 0.001), ("gp_sigma", 0.005), ("gp_scale", 4.0), ("gp_rate", 0.5)),
          "trans": (("sigma_p", 1), ("sigma_d", 0.005)),
          "norm": (("sigma", 0.005),)}


class DepthNoise(object):
    """One noise model with its seed and parameters (the reference's names and defaults: apply_dex_noise,
    apply_translational_noise, apply_gaussian_noise)."""

    def __init__(self, kind, seed=0, **params):
        if kind not in PARAMS:
            raise ValueError(f"kind is one of {sorted(PARAMS)}, not {kind!r}")
        names = [k for k, _ in PARAMS[kind]]
        unknown = sorted(set(params) - set(names))
        if unknown:
            raise TypeError(f"{kind} noise has the parameters {names}, not {unknown}")
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError("seed is an unsigned 64-bit integer")
        self.kind, self.seed = kind, int(seed)
        self.params = {k: float(params.get(k, default)) for k, default in PARAMS[kind]}

    def __repr__(self):
        return "DepthNoise(%r, seed=%d, %s)" % (self.kind, self.seed, ", ".join("%s=%r" % kv for kv in self.params.items()))

    def apply(self, depth, image_ids=None):
        """depth: (n, H, W) or (H, W) device tensor; image_ids: n unsigned 64-bit ids (default 0 .. n-1).  Returns a NEW float32
        device tensor of the same shape; `depth` is not modified.  Asynchronous on the current stream."""
        if not torch.is_tensor(depth):
            raise _capi.GigaHipError("depth noise runs on a HIP device: pass a device tensor; there is no CPU fallback")
        dev = _capi.device_of(depth)
        if depth.dim() not in (2, 3):
            raise ValueError("depth is an (n, H, W) or (H, W) tensor")
        src = depth.to(torch.float32).contiguous().reshape((-1,) + tuple(depth.shape[-2:]))
        n, H, W = (int(d) for d in src.shape)
        ids = None
        if image_ids is not None:
            ids = [int(i) for i in np.asarray(image_ids, dtype=object).reshape(-1)]
            if len(ids) != n or any(not 0 <= i < 1 << 64 for i in ids):
                raise ValueError("image_ids holds one unsigned 64-bit id per image")
            ids = np.array(ids, np.uint64)
        out = torch.empty_like(src)
        if n == 0 or H == 0 or W == 0:
            return out.reshape(depth.shape)
        p = np.array([self.params[k] for k, _ in PARAMS[self.kind]], np.float64)
        model = _capi.NOISE_MODEL[self.kind]
        ws = _capi.workspace("giga_depth_noise", dev, n, W, H, model)
        _capi.call("giga_depth_noise", dev, src, out, n, W, H, model, p, self.seed, ids, ws, ws.numel())
        return out.reshape(depth.shape)


def apply_noise(img, noise_type, seed=0, image_ids=None):
    """misc.apply_noise (misc.py:18-26) with the reference's default parameters: 'dex', 'trans' or 'norm'; an empty or unknown
    type returns `img` unchanged."""
    if noise_type not in PARAMS:
        return img
    return DepthNoise(noise_type, seed).apply(img, image_ids)
