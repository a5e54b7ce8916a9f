"""numpy restatement of the depth-noise kernel (csrc/giga_noise.hip; semantics and draw layout in include/giga_hip.h,
giga_depth_noise): the Philox draw streams, the three models of the reference's vgn.utils.misc.apply_noise, and the seeded test
images of tests/golden/g18_depth_noise.npz (tools/make_noise_goldens.py feeds these draws to the reference's own code)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eval_emu import philox4x32_10  # noqa: E402

STREAM_IMAGE, STREAM_GP, STREAM_ROW, STREAM_COL, STREAM_PIXEL = 0, 1, 2, 3, 4
GAMMA_ATTEMPTS = 16                      # GIGA_NOISE_GAMMA_ATTEMPTS
DEFAULTS = {"dex": dict(gamma_shape=1000, gamma_scale=0.001, gp_sigma=0.005, gp_scale=4.0, gp_rate=0.5),
            "trans": dict(sigma_p=1, sigma_d=0.005), "norm": dict(sigma=0.005)}
FAR = 2.0


# -------------------------------------------------------------------------------------------------------------------- draws
def blocks(block, image_id, stream, seed):
    """the four words of Philox blocks (block, id low, id high, stream) under the key `seed`; block and image_id broadcast"""
    image_id = np.asarray(image_id, np.uint64)
    return philox4x32_10(np.asarray(block, np.uint64), image_id & np.uint64(0xffffffff), image_id >> np.uint64(32), stream,
                         int(seed) & 0xffffffff, int(seed) >> 32)


def u53(hi, lo):
    k = ((hi.astype(np.uint64) >> np.uint64(5)) << np.uint64(26)) | (lo.astype(np.uint64) >> np.uint64(6))
    return np.where(k == 0, 2.0 ** -54, k.astype(np.float64) * 2.0 ** -53)


def uniform_pairs(block, image_id, stream, seed):
    w = blocks(block, image_id, stream, seed)
    return u53(w[0], w[1]), u53(w[2], w[3])


def normal_pairs(block, image_id, stream, seed):
    u1, u2 = uniform_pairs(block, image_id, stream, seed)
    rad, th = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    return rad * np.cos(th), rad * np.sin(th)


def normals(n, image_id, stream, seed):
    """elements 0 .. n-1 of a stream: element e is normal (e & 1) of block e >> 1"""
    z0, z1 = normal_pairs(np.arange((n + 1) // 2), image_id, stream, seed)
    return np.stack([z0, z1], axis=1).reshape(-1)[:n]


def coin(image_id, seed):
    """the always-drawn uniform of dex (compared with gp_rate) for one id or an array of ids"""
    return uniform_pairs(0, image_id, STREAM_IMAGE, seed)[0]


def gamma(image_id, seed, shape=1000.0, scale=0.001, attempts=GAMMA_ATTEMPTS):
    """Marsaglia-Tsang with a bounded number of attempts, for one id or an array of ids -> (draw, attempts used)"""
    ids = np.atleast_1d(np.asarray(image_id, np.uint64))
    shape, scale = float(shape), float(scale)
    a = shape + 1.0 if shape < 1.0 else shape
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    g, used, open_ = np.full(len(ids), d), np.full(len(ids), attempts), np.ones(len(ids), bool)
    for k in range(attempts):
        x = normal_pairs(1 + 2 * k, ids, STREAM_IMAGE, seed)[0]
        u = uniform_pairs(2 + 2 * k, ids, STREAM_IMAGE, seed)[0]
        v = 1.0 + c * x
        pos = v > 0.0
        v = (v * v) * v
        x2 = x * x
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = pos & ((u < 1.0 - 0.0331 * (x2 * x2)) | (np.log(u) < 0.5 * x2 + d * ((1.0 - v) + np.log(np.where(pos, v, 1.0)))))
        take = open_ & ok
        g[take], used[take] = (d * v)[take], k + 1
        open_ &= ~ok
    if shape < 1.0:
        g = g * np.power(uniform_pairs(0, ids, STREAM_IMAGE, seed)[1], 1.0 / shape)
    g = g * scale
    return (g, used) if np.ndim(image_id) else (float(g[0]), int(used[0]))


# ------------------------------------------------------------------------------------------------------------------- models
def coarse_shape(H, W, gp_scale):
    return int(H / gp_scale), int(W / gp_scale)


def upsample(grid, H, W):
    """bilinear, pixel centres, src = (dst + 0.5) (h / H) - 0.5, taps outside the grid read 0, no clip; double"""
    h, w = grid.shape
    pad = np.zeros((h + 2, w + 2))
    pad[1:-1, 1:-1] = grid
    sy, sx = (np.arange(H) + 0.5) * (h / H) - 0.5, (np.arange(W) + 0.5) * (w / W) - 0.5
    fy, fx = np.floor(sy), np.floor(sx)
    ty, tx = (sy - fy)[:, None], (sx - fx)[None, :]
    iy, ix = fy.astype(int)[:, None] + 1, fx.astype(int)[None, :] + 1
    top = (1.0 - tx) * pad[iy, ix] + tx * pad[iy, ix + 1]
    bot = (1.0 - tx) * pad[iy + 1, ix] + tx * pad[iy + 1, ix + 1]
    return (1.0 - ty) * top + ty * bot


def dex_parts(H, W, image_id, seed, gamma_shape=1000, gamma_scale=0.001, gp_sigma=0.005, gp_scale=4.0, gp_rate=0.5):
    """(gamma, coin, coarse randn grid (h, w)): the draws in the reference's call order gamma(), rand(), randn(h, w)"""
    h, w = coarse_shape(H, W, gp_scale)
    return (gamma(image_id, seed, gamma_shape, gamma_scale)[0], float(coin(image_id, seed)),
            normals(h * w, image_id, STREAM_GP, seed).reshape(h, w))


def dex(img, image_id, seed, gamma_shape=1000, gamma_scale=0.001, gp_sigma=0.005, gp_scale=4.0, gp_rate=0.5):
    img = np.asarray(img, np.float32)
    H, W = img.shape
    g, u, z = dex_parts(H, W, image_id, seed, gamma_shape, gamma_scale, gp_sigma, gp_scale, gp_rate)
    out = img * np.float32(g)
    if u < gp_rate:
        out = (out.astype(np.float64) + upsample(z * gp_sigma, H, W)).astype(np.float32)
    return out


def trans_parts(H, W, image_id, seed):
    """the three randn(H, W) arrays in the reference's call order: rows, columns, depth"""
    return tuple(normals(H * W, image_id, s, seed).reshape(H, W) for s in (STREAM_ROW, STREAM_COL, STREAM_PIXEL))


def trans_coords(H, W, image_id, seed, sigma_p=1):
    """(displaced row, displaced column) before rounding, and the rounded, clipped source indices"""
    zr, zc, _ = trans_parts(H, W, image_id, seed)
    ww, hh = np.meshgrid(np.arange(W), np.arange(H))
    fr, fc = hh + zr * sigma_p, ww + zc * sigma_p
    return fr, fc, np.clip(np.round(fr), 0, H - 1).astype(int), np.clip(np.round(fc), 0, W - 1).astype(int)


def trans(img, image_id, seed, sigma_p=1, sigma_d=0.005):
    img = np.asarray(img, np.float32)
    H, W = img.shape
    _, _, r, c = trans_coords(H, W, image_id, seed, sigma_p)
    zd = trans_parts(H, W, image_id, seed)[2]
    return (img[r, c].astype(np.float64) + zd * sigma_d).astype(np.float32)


def norm(img, image_id, seed, sigma=0.005):
    img = np.asarray(img, np.float32)
    H, W = img.shape
    return (img.astype(np.float64) + normals(H * W, image_id, STREAM_PIXEL, seed).reshape(H, W) * sigma).astype(np.float32)


MODELS = {"dex": dex, "trans": trans, "norm": norm}


def apply(kind, imgs, image_ids, seed, **params):
    """(n, H, W) images with their ids -> (n, H, W) float32"""
    return np.stack([MODELS[kind](img, int(i), seed, **params) for img, i in zip(imgs, image_ids)])


# ------------------------------------------------------------------------------------------------------------------- inputs
def depth_images(n, H, W, seed):
    """n float32 depth images: a smooth ramp, a step edge and a `far`-valued background patch, so that a wrong gather shows"""
    rng = np.random.default_rng([seed, n, H, W])
    out = np.empty((n, H, W), np.float32)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for i in range(n):
        a, base = rng.uniform(0.05, 0.2, 2) / max(H, W), rng.uniform(0.4, 0.6)
        img = base + a[0] * r + a[1] * c                                            # the ramp
        edge = rng.integers(1, max(2, W))
        img = np.where(c >= edge, img + rng.uniform(0.1, 0.3), img)               # the step
        r0, c0 = rng.integers(0, H), rng.integers(0, W)
        img[r0:r0 + max(1, H // 3), c0:c0 + max(1, W // 4)] = FAR                   # the background patch
        out[i] = img
    return out


def ulp32(x):
    """the spacing of float32 at |x| (of the smallest normal below it)"""
    x = np.maximum(np.abs(np.asarray(x, np.float32)), np.float32(2.0 ** -126))
    return np.spacing(x).astype(np.float64)


# shapes, seeds and ids of the fixture (tools/make_noise_goldens.py asserts what the tests rely on: see its docstring)
SMALL_SHAPES = [(24, 36), (30, 45), (4, 4), (5, 67), (65, 130)]
BIG_SHAPE = (480, 640)
FIXTURE_SEED = 18
IMAGE_SEED = 5
IDS = {(24, 36): [0, 1, 2, 3], (30, 45): [1, 2, 3], (4, 4): [0, 1, 2, 3], (5, 67): [0, 1, 2], (65, 130): [0, 1],
       (480, 640): [0, 1, (1 << 40) + 3]}
BIG_STRIDE = (16, 16)                     # the stored subset of the 480 x 640 case: every 16th row and column
