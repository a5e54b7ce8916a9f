"""Write tests/golden/g18_depth_noise.npz: the reference's own vgn.utils.misc noise models on this project's draw streams.

    python tools/make_noise_goldens.py

Needs the reference checkout (oracle/ref_bootstrap.py: REFERENCE_SRC) and scipy; runs only where that checkout is present.  The reference's
utils/misc.py is loaded by path and run as it is.  Two things are supplied around it:

  skimage.transform.resize   scikit-image need not be installed: the stand-in evaluates resize(order=1, mode="constant",
                             anti_aliasing=False) as scipy.ndimage.zoom(order=1, mode="grid-constant", cval=0, grid_mode=True),
                             the routine scikit-image itself calls, WITHOUT resize's final clip to the input's [min, max].  The
                             kernel does not clip either (include/giga_hip.h).  The clip is the identity when the coarse grid has
                             both signs, which is asserted below for every grid of more than one cell; the 4 x 4 image's 1 x 1 grid
                             cannot have both signs, and there the fixture pins the unclipped definition.
  np.random.gamma/rand/randn replaced, for the duration of a call, by functions that hand out the draws of tests/noise_emu.py in
                             the reference's call order (and check the requested shapes), so the reference's code consumes this
                             project's streams: image-stream gamma and coin, GP grid, row / column / depth normals.

Only arrays, seeds and ids are stored.  The inputs are regenerated from a seed by noise_emu.depth_images (a checksum is stored).
Per shape HxW of noise_emu.SMALL_SHAPES: ids, dex / trans / norm outputs (float32), the rounded trans source indices (int16) and the
dex coin outcome; for 480x640 the rows and columns noise_emu.BIG_STRIDE apart plus float64 sums of every output image.
Asserted here, because the tests rely on it: among the dex ids of each shape the GP branch is taken and not taken; every coarse
grid of more than one cell has both signs; no displaced trans coordinate lies within 1e-9 of a half-integer (so the rounded
index cannot depend on the last bits of log / cos / sin); the gamma sampler accepted within its attempt cap.
"""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import scipy.ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import noise_emu as N  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g18_depth_noise.npz")


def _resize(image, output_shape, order=None, anti_aliasing=None, mode=None, **kw):
    assert order == 1 and mode == "constant" and anti_aliasing is False and not kw, (order, mode, anti_aliasing, kw)
    zoom = [o / i for o, i in zip(output_shape, image.shape)]
    out = scipy.ndimage.zoom(image, zoom, order=1, mode="grid-constant", cval=0.0, grid_mode=True)
    assert out.shape == tuple(output_shape)
    return out


def reference_misc():
    from oracle import ref_bootstrap
    if not ref_bootstrap.reference_available():
        raise SystemExit("the reference checkout is not present: fixtures can only be made where it is")
    skimage, transform = types.ModuleType("skimage"), types.ModuleType("skimage.transform")
    transform.resize = _resize
    skimage.transform = transform
    saved = {k: sys.modules.get(k) for k in ("skimage", "skimage.transform")}
    sys.modules.update({"skimage": skimage, "skimage.transform": transform})
    try:
        spec = importlib.util.spec_from_file_location("reference_misc", os.path.join(ref_bootstrap.REFERENCE_SRC, "vgn", "utils", "misc.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


class Feed(object):
    """np.random.gamma / rand / randn for one reference call: hands out `draws` [(kind, value), ...] in order"""

    def __init__(self, draws):
        self.draws = list(draws)

    def _next(self, kind, shape=()):
        k, v = self.draws.pop(0)
        assert k == kind and np.shape(v) == tuple(shape), (k, kind, np.shape(v), shape)
        return v

    def __enter__(self):
        self.saved = (np.random.gamma, np.random.rand, np.random.randn)
        np.random.gamma = lambda shape, scale: float(self._next("gamma"))          # a Python float, like the generator's
        np.random.rand = lambda: float(self._next("rand"))
        np.random.randn = lambda *shape: self._next("randn", shape).copy()
        return self

    def __exit__(self, *exc):
        np.random.gamma, np.random.rand, np.random.randn = self.saved


def reference_outputs(misc, img, image_id, seed):
    """-> dict(dex, trans, norm, r, c, on) of one image from the reference's three functions on this project's draws"""
    H, W = img.shape
    out = {}
    g, u, z = N.dex_parts(H, W, image_id, seed)
    assert N.gamma(image_id, seed)[1] < N.GAMMA_ATTEMPTS
    on = u < 0.5
    if on and z.size > 1:
        assert z.min() < 0 < z.max(), ("coarse grid of one sign", H, W, image_id)
    with Feed([("gamma", g), ("rand", u), ("randn", z)]) as f:
        out["dex"] = misc.apply_noise(img.copy(), "dex")
        assert len(f.draws) == (0 if on else 1)
    zr, zc, zd = N.trans_parts(H, W, image_id, seed)
    fr, fc, r, c = N.trans_coords(H, W, image_id, seed)
    for v in (fr, fc):
        assert np.abs(np.abs(v - np.floor(v)) - 0.5).min() > 1e-9, ("a displaced coordinate at a half-integer", H, W, image_id)
    with Feed([("randn", zr), ("randn", zc), ("randn", zd)]) as f:
        out["trans"] = misc.apply_noise(img.copy(), "trans")
        assert not f.draws
    with Feed([("randn", zd)]) as f:
        out["norm"] = misc.apply_noise(img.copy(), "norm")
        assert not f.draws
    for k in ("dex", "trans", "norm"):
        assert out[k].dtype == np.float32 and out[k].shape == (H, W), (k, out[k].dtype)
    out.update(r=r.astype(np.int16), c=c.astype(np.int16), on=on)
    return out


def checksum(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def build():
    misc = reference_misc()
    seed = N.FIXTURE_SEED
    fix = {"seed": np.uint64(seed), "image_seed": np.int64(N.IMAGE_SEED)}
    for H, W in N.SMALL_SHAPES + [N.BIG_SHAPE]:
        ids = N.IDS[(H, W)]
        imgs = N.depth_images(len(ids), H, W, N.IMAGE_SEED)
        outs = [reference_outputs(misc, img, i, seed) for img, i in zip(imgs, ids)]
        on = np.array([o["on"] for o in outs])
        assert on.any() and not on.all(), ("the dex ids must take both GP branches", H, W, on)
        tag = "%dx%d" % (H, W)
        fix["ids_" + tag] = np.array(ids, np.uint64)
        fix["in_sha_" + tag] = checksum(imgs)
        fix["dex_on_" + tag] = on
        sub = (slice(None),) * 2 if (H, W) != N.BIG_SHAPE else (slice(None, None, N.BIG_STRIDE[0]), slice(None, None, N.BIG_STRIDE[1]))
        for k in ("dex", "trans", "norm", "r", "c"):
            fix[k + "_" + tag] = np.stack([o[k][sub] for o in outs])
        if (H, W) == N.BIG_SHAPE:
            for k in ("dex", "trans", "norm"):
                fix[k + "_sum_" + tag] = np.array([o[k].astype(np.float64).sum() for o in outs])
    return fix


if __name__ == "__main__":
    fix = build()
    if os.path.exists(OUT) and "--check" in sys.argv:
        old = np.load(OUT)
        assert set(old.files) == set(fix), set(old.files) ^ set(fix)
        for k in fix:
            assert np.array_equal(old[k], fix[k]), k
        print("g18_depth_noise.npz regenerates array for array (%d arrays)" % len(fix))
    else:
        np.savez_compressed(OUT, **fix)
        print(OUT, os.path.getsize(OUT), "bytes")
