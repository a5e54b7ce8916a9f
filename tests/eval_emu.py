"""numpy float64 restatements of the mesh-evaluation kernels (csrc/giga_eval.hip) and of the reference's metrics
(vgn/ConvONets/eval.py), plus the seeded inputs of tests/golden/g17_eval.npz (tools/make_eval_goldens.py regenerates the
same inputs; the fixture stores a checksum of each)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_emu  # noqa: E402

CASES = {"A": 20000, "B": 3000}          # points per cloud
N_IOU = 20000
THRESHOLDS = np.linspace(1. / 1000, 1, 1000)


# ------------------------------------------------------------------------------------------------------------------- inputs
def fixture_mesh(g16, name):
    """(vertices float32, faces int64) of g16's fixture `name` through the marching-cubes restatement."""
    v, f = mesh_emu.marching_cubes(g16[name + "_grid"], float(g16[name + "_iso"]), float(g16[name + "_box_size"]))
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int64)


def target_mesh(v, f):
    """the "ground truth" of the fixture: the same mesh scaled by 1.02 and shifted by 0.003"""
    return (v.astype(np.float64) * 1.02 + 0.003).astype(np.float32), f


def face_normals(v, f):
    v = v.astype(np.float64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    with np.errstate(invalid="ignore"):                  # (a face without area has no normal, and is never sampled)
        return n / np.linalg.norm(n, axis=1, keepdims=True)


def numpy_cloud(v, f, n, seed):
    """n points (float32) with face normals (float32) from a float64 sampler on default_rng(seed)"""
    rng = np.random.default_rng(seed)
    v64 = v.astype(np.float64)
    nr = np.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]])
    area = 0.5 * np.linalg.norm(nr, axis=1)
    face = rng.choice(len(f), size=n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.random(n))[:, None], rng.random(n)[:, None]
    a, b, c = v64[f[face, 0]], v64[f[face, 1]], v64[f[face, 2]]
    p = (1 - r1) * a + r1 * (1 - r2) * b + r1 * r2 * c
    return p.astype(np.float32), face_normals(v, f)[face].astype(np.float32)


def iou_points(seed):
    return (np.random.default_rng(seed).random((N_IOU, 3)) - 0.5).astype(np.float32)


def case_inputs(g16, name, seed):
    v, f = fixture_mesh(g16, name)
    tv, tf = target_mesh(v, f)
    n = CASES[name]
    pred, n_pred = numpy_cloud(v, f, n, seed)
    tgt, n_tgt = numpy_cloud(tv, tf, n, seed + 1)
    pts = iou_points(seed + 2)
    occ_tgt = np.linalg.norm(pts.astype(np.float64), axis=1) < 0.3          # the "second bit vector" of compute_iou
    return dict(v=v, f=f, tv=tv, pred=pred, n_pred=n_pred, tgt=tgt, n_tgt=n_tgt, pts=pts, occ_tgt=occ_tgt)


def checksum(inp):
    h = hashlib.sha256()
    for k in ("v", "f", "tv", "pred", "n_pred", "tgt", "n_tgt", "pts", "occ_tgt"):
        h.update(np.ascontiguousarray(inp[k]).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


# -------------------------------------------------------------------------------------------------------- nearest neighbour
def nn_brute(src, tgt, chunk=512):
    """float64 brute force: (dist, idx with the lowest index on a tie, second-nearest distance)"""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    n = len(src)
    dist, idx, second = np.full(n, np.inf), np.full(n, -1, np.int64), np.full(n, np.inf)
    if len(tgt) == 0:
        return dist, idx, second
    chunk = max(1, min(chunk, 4_000_000 // len(tgt)))
    for s in range(0, n, chunk):
        d = src[s:s + chunk, None, :] - tgt[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        i = d2.argmin(axis=1)
        r = np.arange(len(i))
        dist[s:s + chunk] = np.sqrt(d2[r, i])
        idx[s:s + chunk] = i
        if len(tgt) > 1:
            d2[r, i] = np.inf
            second[s:s + chunk] = np.sqrt(d2.min(axis=1))
    return dist, idx, second


def near_tie(dist, second, rel=1e-6):
    return second - dist <= rel * dist


# ------------------------------------------------------------------------------------------------------------------ sampler
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32 with 10 rounds (Salmon et al. 2011) on uint32 arrays; returns the four output words"""
    c = [np.asarray(x, np.uint64) & 0xffffffff for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & 0xffffffff), np.uint64(k1 & 0xffffffff)
    m = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m
        k1 = (k1 + np.uint64(0xBB67AE85)) & m
    return [x.astype(np.uint32) for x in c]


def uniforms(n, seed, scene=0):
    w = philox4x32_10(np.arange(n), scene, 0, 0, seed & 0xffffffff, seed >> 32)
    return [x.astype(np.float64) * 2.0 ** -32 for x in w[:3]]


def face_areas(v, f):
    v = np.asarray(v, np.float32).astype(np.float64)
    ok = ((f >= 0) & (f < len(v))).all(axis=1) if len(f) else np.zeros(0, bool)
    g = np.where(ok[:, None], f, 0)
    e1, e2 = v[g[:, 1]] - v[g[:, 0]], v[g[:, 2]] - v[g[:, 0]]
    n = np.cross(e1, e2)
    with np.errstate(invalid="ignore", over="ignore"):
        area = 0.5 * np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return np.where(ok & (area > 0) & np.isfinite(area), area, 0.0)


def sample_surface(v, f, n, seed, scene=0):
    """-> dict(points float32, face, normals float32, r (3 uniforms), x = r0 * total, cum, total); empty for a mesh without area"""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    cum = np.cumsum(face_areas(v, f))
    total = cum[-1] if len(cum) else 0.0
    if not (total > 0 and np.isfinite(total)):
        return dict(points=np.zeros((0, 3), np.float32), face=np.zeros(0, np.int64), normals=np.zeros((0, 3), np.float32))
    r = uniforms(n, seed, scene)
    x = r[0] * total
    face = np.minimum(np.searchsorted(cum, x, side="right"), len(f) - 1)        # first face with cum > x
    p, nr = points_on_faces(v, f, face, r[1], r[2])
    return dict(points=p, face=face, normals=nr, r=r, x=x, cum=cum, total=total)


def points_on_faces(v, f, face, r1, r2):
    v64 = np.asarray(v, np.float32).astype(np.float64)
    a, b, c = v64[f[face, 0]], v64[f[face, 1]], v64[f[face, 2]]
    sr = np.sqrt(r1)
    wa, wb, wc = (1.0 - sr)[:, None], (sr * (1.0 - r2))[:, None], (sr * r2)[:, None]
    p = (wa * a + wb * b) + wc * c
    nr = np.cross(b - a, c - a)
    ln = np.sqrt((nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2])
    return p.astype(np.float32), (nr / ln[:, None]).astype(np.float32)


# -------------------------------------------------------------------------------------------------------------- containment
def mesh_contains(v, f, points, resolution=512, chunk=256):
    """MeshIntersector(mesh, resolution).query(points) restated over ALL triangles (the reference's hash only culls)"""
    tri = np.asarray(v)[np.asarray(f)].astype(np.float64)
    pts = np.asarray(points)
    out = np.zeros(len(pts), bool)
    if len(tri) == 0 or len(pts) == 0:
        return out
    lo, hi = tri.reshape(-1, 3).min(axis=0), tri.reshape(-1, 3).max(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = (resolution - 1) / (hi - lo)
        translate = 0.5 - scale * lo
        tri = scale * tri + translate
        pts = scale * pts + translate
        inside = np.all((0 <= pts) & (pts <= resolution), axis=1)
        A = (tri[:, :2, :2] - tri[:, 2:, :2]).transpose([0, 2, 1])
        det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
        sdet, adet = np.sign(det), np.abs(det)
        t1, t2, t3 = tri[:, 0], tri[:, 1], tri[:, 2]
        nrm = np.cross(t3 - t1, t2 - t1)
        an, sn = np.abs(nrm[:, 2]), np.sign(nrm[:, 2])
        for s in range(0, len(pts), chunk):
            p = pts[s:s + chunk]
            y0, y1 = p[:, None, 0] - tri[None, :, 2, 0], p[:, None, 1] - tri[None, :, 2, 1]
            u = (A[None, :, 1, 1] * y0 - A[None, :, 0, 1] * y1) * sdet
            w = (-A[None, :, 1, 0] * y0 + A[None, :, 0, 0] * y1) * sdet
            uw = u + w
            hit = (adet != 0) & (0 < u) & (u < adet) & (0 < w) & (w < adet) & (0 < uw) & (uw < adet)
            alpha = nrm[None, :, 0] * (t1[None, :, 0] - p[:, None, 0]) + nrm[None, :, 1] * (t1[None, :, 1] - p[:, None, 1])
            depth = np.where(an != 0, t1[None, :, 2] * an + alpha * sn, np.nan)
            ref = p[:, None, 2] * an
            n0 = (hit & (depth >= ref)).sum(axis=1)
            n1 = (hit & (depth < ref)).sum(axis=1)
            out[s:s + chunk] = inside[s:s + chunk] & (n0 % 2 == 1) & (n1 % 2 == 1)
    return out


# ------------------------------------------------------------------------------------------------------------------ metrics
def compute_iou(occ1, occ2):
    occ1, occ2 = np.asarray(occ1) >= 0.5, np.asarray(occ2) >= 0.5
    return (occ1 & occ2).astype(np.float32).sum(axis=-1) / (occ1 | occ2).astype(np.float32).sum(axis=-1)


def threshold_percentage(dist, thresholds=THRESHOLDS):
    return [(dist <= t).mean() for t in thresholds]


def normal_dots(idx, n_src, n_tgt):
    n_src = n_src / np.linalg.norm(n_src, axis=-1, keepdims=True)
    n_tgt = n_tgt / np.linalg.norm(n_tgt, axis=-1, keepdims=True)
    return np.abs((n_tgt[idx] * n_src).sum(axis=-1))


def eval_pointcloud(pred, tgt, n_pred, n_tgt):
    """the reference's eval_pointcloud on float64 brute-force neighbours"""
    comp, ci, _ = nn_brute(tgt, pred)
    acc, ai, _ = nn_brute(pred, tgt)
    cn = normal_dots(ci, n_tgt.astype(np.float64), n_pred.astype(np.float64)).mean()
    an = normal_dots(ai, n_pred.astype(np.float64), n_tgt.astype(np.float64)).mean()
    recall, precision = threshold_percentage(comp), threshold_percentage(acc)
    with np.errstate(invalid="ignore", divide="ignore"):
        F = [2 * np.float64(precision[i]) * recall[i] / (precision[i] + recall[i]) for i in range(len(precision))]
    return {"completeness": comp.mean(), "accuracy": acc.mean(), "normals completeness": cn, "normals accuracy": an,
            "normals": 0.5 * cn + 0.5 * an, "completeness2": (comp ** 2).mean(), "accuracy2": (acc ** 2).mean(),
            "chamfer-L2": 0.5 * ((comp ** 2).mean() + (acc ** 2).mean()), "chamfer-L1": 0.5 * (comp.mean() + acc.mean()),
            "f-score": F[9], "f-score-15": F[14], "f-score-20": F[19]}


# key -> (kind, bound): the bounds of the metric comparison (relative for distances, absolute for normals and F-scores)
METRIC_BOUNDS = {"completeness": ("rel", 5e-6), "accuracy": ("rel", 5e-6), "chamfer-L1": ("rel", 5e-6),
                 "completeness2": ("rel", 1e-5), "accuracy2": ("rel", 1e-5), "chamfer-L2": ("rel", 1e-5),
                 "normals completeness": ("abs", 1e-5), "normals accuracy": ("abs", 1e-5), "normals": ("abs", 1e-5),
                 "f-score": ("abs", 1e-12), "f-score-15": ("abs", 1e-12), "f-score-20": ("abs", 1e-12)}


def assert_metrics(got, want, what=""):
    assert set(METRIC_BOUNDS) <= set(got), sorted(got)
    for k, (kind, bound) in METRIC_BOUNDS.items():
        g, w = float(got[k]), float(want[k])
        err = abs(g - w) / (abs(w) if kind == "rel" else 1.0)
        print(what, k, g, w, "err %.3g (bound %.1g %s)" % (err, bound, kind))
        assert err <= bound, (what, k, g, w)
