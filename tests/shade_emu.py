"""numpy restatement of the colour renderer (include/giga_hip.h, giga_color_render and giga_image_downsample) on top of
tests/render_emu.py's hit test, written from the header's text and not from the kernel, in two forms: `render` is vectorised over
the pixels (numpy float64, one IEEE rounding per operation, never fused), `render_scalar` takes one pixel and one triangle at a
time in Python floats (IEEE doubles, math.sqrt and math.floor correctly rounded / exact).  The two agree byte for byte on every
scene of CASES (tests/test_shade_host.py), which is what lets the GPU comparison (tests/test_gpu_shade.py) be strict.  Also the
scenes both test files share."""
import math

import numpy as np

import render_emu as remu
import tsdf_emu as emu

F32 = np.float32
SIZE = 0.3
HEADLIGHT = (0.0, 0.0, 0.0, 1.0)
WHITE = (255, 255, 255, 255)


def _pixel_dirs(intrinsic, pixel_offset):
    W, H, fx, fy, cx, cy = intrinsic
    fx, fy, cx, cy, po = (np.float64(v) for v in (fx, fy, cx, cy, pixel_offset))
    dx = ((np.arange(int(W), dtype=np.float64) + po) - cx) / fx
    dy = ((np.arange(int(H), dtype=np.float64) + po) - cy) / fy
    return dx, dy


def render(vertices, faces, face_colors, extrinsic, intrinsic, light=HEADLIGHT, ambient=0.3, background=WHITE, near=0.1, far=2.0,
           pixel_offset=0.0, order=None):
    """(rgba (H, W, 4) uint8, depth (H, W) float32, index (H, W) int32).  order: the order in which the triangles are tested (the
    result must not depend on it)."""
    W, H = int(intrinsic[0]), int(intrinsic[1])
    near, far, ambient = np.float64(near), np.float64(far), np.float64(ambient)
    cam = remu.camera_vertices(vertices, extrinsic)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    colors = np.asarray(face_colors, np.uint8).reshape(-1, 4)
    dx, dy = _pixel_dirs(intrinsic, pixel_offset)
    DX, DY = np.meshgrid(dx, dy)
    best = np.full((H, W), np.inf)
    win = np.full((H, W), -1, np.int64)
    with np.errstate(all="ignore"):
        for i in (range(len(faces)) if order is None else order):
            ia, ib, ic = faces[i]
            if min(ia, ib, ic) < 0 or max(ia, ib, ic) >= len(cam):
                continue
            a, b, c = cam[ia], cam[ib], cam[ic]
            nbc, nca, nab = remu.cross(b, c), remu.cross(c, a), remu.cross(a, b)
            U = (DX * nbc[0] + DY * nbc[1]) + nbc[2]
            V = (DX * nca[0] + DY * nca[1]) + nca[2]
            Wd = (DX * nab[0] + DY * nab[1]) + nab[2]
            S = (U + V) + Wd
            hit = (S != 0) & (((U >= 0) & (V >= 0) & (Wd >= 0)) | ((U <= 0) & (V <= 0) & (Wd <= 0)))
            z = ((U * a[2] + V * b[2]) + Wd * c[2]) / S
            take = hit & (z >= near) & (z <= far) & ((z < best) | ((z == best) & (i < win)))
            best = np.where(take, z, best)
            win = np.where(take, i, win)
        depth = np.where(best <= far, best, far).astype(F32)
        rgba = np.empty((H, W, 4), np.uint8)
        rgba[:] = np.asarray(background, np.uint8)
        got = win >= 0
        if got.any():
            w = win[got]
            a, b, c = (cam[faces[w, k]] for k in range(3))                   # (m, 3) each
            e1, e2 = b - a, c - a
            n = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
            z = best[got]
            p = [z * DX[got], z * DY[got], z]
            lx, ly, lz, lw = (np.float64(v) for v in light)
            L = [lx - lw * p[0], ly - lw * p[1], lz - lw * p[2]]
            nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
            ll = (L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]
            q = nn * ll
            nl = (n[0] * L[0] + n[1] * L[1]) + n[2] * L[2]
            k = np.where((q != 0) & np.isfinite(q), ambient + ((1.0 - ambient) * np.abs(nl)) / np.sqrt(q), ambient)
            C = colors[w, :3].astype(np.float64)
            out = np.full((len(w), 4), 255, np.uint8)
            out[:, :3] = np.minimum(np.floor(k[:, None] * C + 0.5), 255.0).astype(np.uint8)
            rgba[got] = out
    return rgba, depth, win.astype(np.int32)


def render_scalar(vertices, faces, face_colors, extrinsic, intrinsic, light=HEADLIGHT, ambient=0.3, background=WHITE, near=0.1, far=2.0,
                  pixel_offset=0.0, pixels=None):
    """The same, one Python float operation after the other.  pixels: the (row, column) pairs to compute (default: all); the
    others keep background, float32(far) and -1."""
    W, H, fx, fy, cx, cy = intrinsic
    W, H = int(W), int(H)
    fx, fy, cx, cy, near, far, po, ambient = (float(v) for v in (fx, fy, cx, cy, near, far, pixel_offset, ambient))
    lx, ly, lz, lw = (float(v) for v in light)
    E = [[float(x) for x in row] for row in np.asarray(extrinsic, np.float64).reshape(4, 4)]
    verts = [[float(x) for x in row] for row in np.asarray(vertices, F32).reshape(-1, 3)]
    cam = [[((E[r][0] * x + E[r][1] * y) + E[r][2] * z) + E[r][3] for r in range(3)] for x, y, z in verts]
    faces = [[int(i) for i in row] for row in np.asarray(faces, np.int64).reshape(-1, 3)]
    colors = np.asarray(face_colors, np.uint8).reshape(-1, 4)

    def cross(P, Q):
        return (P[1] * Q[2] - P[2] * Q[1], P[2] * Q[0] - P[0] * Q[2], P[0] * Q[1] - P[1] * Q[0])
    tris = []
    for i, (ia, ib, ic) in enumerate(faces):
        if min(ia, ib, ic) < 0 or max(ia, ib, ic) >= len(cam):
            continue
        a, b, c = cam[ia], cam[ib], cam[ic]
        tris.append((i, cross(b, c), cross(c, a), cross(a, b), a[2], b[2], c[2]))
    rgba = np.empty((H, W, 4), np.uint8)
    rgba[:] = np.asarray(background, np.uint8)
    depth = np.full((H, W), F32(far), F32)
    index = np.full((H, W), -1, np.int32)
    for v, u in (pixels if pixels is not None else ((v, u) for v in range(H) for u in range(W))):
        dx, dy = ((u + po) - cx) / fx, ((v + po) - cy) / fy
        best, win = math.inf, -1
        for i, nbc, nca, nab, az, bz, cz in tris:
            U = (dx * nbc[0] + dy * nbc[1]) + nbc[2]
            V = (dx * nca[0] + dy * nca[1]) + nca[2]
            Wd = (dx * nab[0] + dy * nab[1]) + nab[2]
            if not ((U >= 0 and V >= 0 and Wd >= 0) or (U <= 0 and V <= 0 and Wd <= 0)):
                continue
            S = (U + V) + Wd
            if S == 0 or S != S:
                continue
            num = (U * az + V * bz) + Wd * cz
            if math.isinf(num) and math.isinf(S):
                continue                                           # inf / inf is NaN: never accepted
            z = num / S
            if near <= z <= far and (z < best or (z == best and i < win)):
                best, win = z, i
        if win < 0:
            continue
        depth[v, u] = F32(best)
        index[v, u] = win
        a, b, c = (cam[j] for j in faces[win])
        n = cross([b[0] - a[0], b[1] - a[1], b[2] - a[2]], [c[0] - a[0], c[1] - a[1], c[2] - a[2]])
        p = (best * dx, best * dy, best)
        L = (lx - lw * p[0], ly - lw * p[1], lz - lw * p[2])
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        ll = (L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]
        q = nn * ll
        k = ambient
        if q != 0 and math.isfinite(q):
            k = ambient + ((1.0 - ambient) * abs((n[0] * L[0] + n[1] * L[1]) + n[2] * L[2])) / math.sqrt(q)
        rgba[v, u] = [min(math.floor(k * float(C) + 0.5), 255) for C in colors[win, :3]] + [255]
    return rgba, depth, index


def render_views(vertices, faces, face_colors, extrinsics, intrinsic, lights=None, form=render, **kw):
    """stacked (rgba (n, H, W, 4), depth (n, H, W), index (n, H, W)); lights: None, one light, or one per view"""
    lights = np.asarray(HEADLIGHT if lights is None else lights, np.float64)
    lights = np.tile(lights, (len(extrinsics), 1)) if lights.ndim == 1 else lights
    out = [form(vertices, faces, face_colors, e, intrinsic, light=l, **kw) for e, l in zip(extrinsics, lights)]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def supersample_camera(intrinsic, pixel_offset, k):
    """the header's supersampling parameters: (k W, k H, k fx, k fy, k cx, k cy), k (pixel_offset - 0.5) + 0.5"""
    W, H, fx, fy, cx, cy = intrinsic
    return (k * int(W), k * int(H), k * float(fx), k * float(fy), k * float(cx), k * float(cy)), k * (float(pixel_offset) - 0.5) + 0.5


def downsample(rgba, k):
    """(..., k H, k W, 4) uint8 -> (..., H, W, 4): per channel (sum + k k / 2) / (k k) in integers"""
    a = np.asarray(rgba, np.uint8).astype(np.int64)
    Hk, Wk = a.shape[-3], a.shape[-2]
    a = a.reshape(a.shape[:-3] + (Hk // k, k, Wk // k, k, 4)).sum(axis=(-4, -2))
    return ((a + (k * k) // 2) // (k * k)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the shared scenes
PIXEL_CAM = (32, 16, 64.0, 64.0, 16.0, 8.0)
SMALL = emu.SMALL_INTRINSIC                                        # 37 rows x 53 columns: ragged 16 x 16 tiles


def random_colors(n, seed):
    c = np.random.default_rng(seed).integers(0, 256, size=(n, 4), dtype=np.uint8)
    c[:, 3] = 255
    return c


def plane_boxes(seed):
    return remu.scene_to_mesh(emu.make_scene(seed))


def tile_icosphere():
    """the 1280-triangle icosphere, seen from view 0 of the circle small enough to sit inside one 16 x 16 tile of SMALL: more
    survivors than the kernel's LDS list holds (384), so the flush runs more than once and carries indices"""
    return remu.icosphere((0.15, 0.15, 0.14), 0.03, 3)             # rows 10 .. 14, columns 24 .. 29 (tests/test_shade_host.py)


def tie_squares(swap, flip):
    """two coplanar 4 x 4-pixel squares at z = 0.5 under PIXEL_CAM that share the edge through the pixel centres of column 16, a
    red one (columns 12 .. 16) and a blue one (columns 16 .. 20), rows 4 .. 8; swap puts the blue one first.  Returns the mesh,
    the colours and the (H, W) bool masks (left only, shared edge, right only)."""
    left = remu.grid_square((12 - 16) / 128.0, (4 - 8) / 128.0, 4 / 128.0, 1, 1, 0.5, flip)
    right = remu.grid_square((16 - 16) / 128.0, (4 - 8) / 128.0, 4 / 128.0, 1, 1, 0.5, flip)
    red, blue = np.tile(np.array([200, 10, 20, 255], np.uint8), (2, 1)), np.tile(np.array([10, 20, 200, 255], np.uint8), (2, 1))
    mesh = remu.merge(right, left) if swap else remu.merge(left, right)
    colors = np.concatenate((blue, red) if swap else (red, blue))
    masks = [np.zeros((16, 32), bool) for _ in range(3)]
    masks[0][4:9, 12:16] = True
    masks[1][4:9, 16] = True
    masks[2][4:9, 17:21] = True
    return mesh, colors, masks


def _nan_and_bad_index():
    v, f = remu.plane_mesh(0.5, 4 / 128.0)
    v = np.concatenate([v, [[np.nan, 0, 0.4], [0.1, 0.1, 0.4], [-0.1, 0.1, 0.4], [np.inf, 0.0, 0.3]]]).astype(F32)
    f = np.concatenate([[[4, 5, 6]], [[0, 1, 8]], f, [[0, -1, 2]], [[7, 5, 6]]]).astype(np.int32)
    return v, f


BEHIND = (np.array([[-1, 0.0625, 2], [1, 0.0625, 2], [0, 0.0625, -1]], F32), np.array([[0, 1, 2]], np.int32))
EMPTY = (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32))
EYE = np.eye(4)[None]


def _case(mesh, K, ext, seed=1, colors=None, **kw):
    return mesh, (random_colors(len(mesh[1]), seed) if colors is None else colors), K, ext, kw


# name -> (mesh, face colours, intrinsic, extrinsics, keyword arguments of render): every scene the GPU tests compare
CASES = {
    "six-37x53-plane-boxes": lambda: _case(plane_boxes(0), SMALL, emu.six_views(SIZE)),
    "tile-icosphere-1280": lambda: _case(tile_icosphere(), SMALL, emu.six_views(SIZE, 1, 6), seed=2),
    "tie-squares": lambda: _case(tie_squares(False, False)[0], PIXEL_CAM, EYE, colors=tie_squares(False, False)[1]),
    "tie-squares-flipped-swapped": lambda: _case(tie_squares(True, True)[0], PIXEL_CAM, EYE, colors=tie_squares(True, True)[1]),
    "point-light": lambda: _case(plane_boxes(1), SMALL, emu.six_views(SIZE, 2, 6), lights=(0.2, -0.3, 0.1, 1.0)),
    "directional-light": lambda: _case(plane_boxes(1), SMALL, emu.six_views(SIZE, 2, 6), lights=(0.3, -0.5, -1.0, 0.0)),
    "ambient-0": lambda: _case(plane_boxes(2), SMALL, emu.six_views(SIZE, 1, 6), ambient=0.0),
    "ambient-1": lambda: _case(plane_boxes(2), SMALL, emu.six_views(SIZE, 1, 6), ambient=1.0),
    "behind-the-camera": lambda: _case(BEHIND, PIXEL_CAM, EYE, background=(1, 2, 3, 4)),
    "empty-mesh": lambda: _case(EMPTY, PIXEL_CAM, EYE, background=(9, 8, 7, 0)),
    "nan-vertex-bad-index": lambda: _case(_nan_and_bad_index(), PIXEL_CAM, EYE),
    "near-far": lambda: _case(remu.box_mesh((-0.05, -0.05, 0.05), (0.05, 0.05, 0.3)), PIXEL_CAM, EYE, near=0.1, far=0.25),
    "pixel-offset-half": lambda: _case(plane_boxes(3), SMALL, emu.six_views(SIZE, 2, 6), pixel_offset=0.5),
}
FULL = lambda: _case(plane_boxes(0), emu.SIM_INTRINSIC, emu.six_views(SIZE, 1, 6))           # noqa: E731  one 480 x 640 view
SUPER = lambda: _case(plane_boxes(4), SMALL, emu.six_views(SIZE, 2, 6), seed=3)              # noqa: E731  supersample 2 and 3


def render_case(case, form=render, **extra):
    """(rgba, depth, index) of every view of a case"""
    (v, f), colors, K, ext, kw = case
    kw = dict(kw, **extra)
    return render_views(v, f, colors, ext, K, lights=kw.pop("lights", None), form=form, **kw)
