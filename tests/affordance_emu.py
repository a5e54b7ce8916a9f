"""numpy restatement of the affordance of a scene mesh (giga_affordance_points / giga_affordance_faces, include/giga_hip.h),
written from that description: the voxels above th become points, every face aggregates the quality of the points near its
centre, matplotlib's 'Reds' colours the result.  Two forms of the exact part -- vectorised, and one scalar operation after the
other in the order the description gives -- which tests/test_affordance_host.py holds against each other bit for bit."""
import numpy as np

F32, F64 = np.float32, np.float64
DEFAULTS = dict(size=0.3, th=0.5, temp=150, rad=0.02, finger_depth=0.05, finger_offset=0.5, move_center=True, aggregation="max")
GREY = np.array([102, 102, 102, 255], np.uint8)
REDS_ANCHORS = ("fff5f0", "fee0d2", "fcbba1", "fc9272", "fb6a4a", "ef3b2c", "cb181d", "a50f15", "67000d")


# ---------------------------------------------------------------------------------------------------------------- points
def lin(size, R):
    t = np.arange(R, dtype=F64) * (F64(size) / F64(R - 1))
    t[R - 1] = size
    return t


def points(qual, rot, size=0.3, th=0.5, finger_depth=0.05, finger_offset=0.5, move_center=True):
    """qual (R,R,R) float32, rot (R,R,R,4) float32 -> (P,4) float64 (x, y, z, q), ascending voxel order"""
    qual, rot = np.asarray(qual, F32), np.asarray(rot, F32).reshape(qual.shape + (4,))
    R = qual.shape[0]
    t = lin(size, R)
    pos = np.stack(np.meshgrid(t, t, t, indexing="ij"), -1)
    if move_center:
        r0, r1, r2, r3 = (rot[..., i] for i in range(4))
        two = F32(2)
        z = np.stack(((two * r0) * r2 + (two * r1) * r3, (two * r1) * r2 - (two * r0) * r3,
                      (F32(1) - (two * r0) * r0) - (two * r1) * r1), -1)
        assert z.dtype == F32
        off = (z * F32(finger_depth)) * F32(finger_offset)
        assert off.dtype == F32
        pos = pos + off.astype(F64)
    keep = qual > F32(th)
    return np.concatenate((pos[keep], qual[keep].astype(F64)[:, None]), 1)


def points_scalar(qual, rot, size=0.3, th=0.5, finger_depth=0.05, finger_offset=0.5, move_center=True):
    qual, rot = np.asarray(qual, F32), np.asarray(rot, F32).reshape(np.shape(qual) + (4,))
    R = qual.shape[0]
    step = F64(size) / F64(R - 1)
    out = []
    for i in range(R):
        for j in range(R):
            for k in range(R):
                q = qual[i, j, k]
                if not q > F32(th):
                    continue
                p = [F64(size) if a == R - 1 else F64(a) * step for a in (i, j, k)]
                if move_center:
                    r0, r1, r2, r3 = rot[i, j, k]
                    z = (F32(F32(F32(2) * r0) * r2) + F32(F32(F32(2) * r1) * r3), F32(F32(F32(2) * r1) * r2) - F32(F32(F32(2) * r0) * r3),
                         F32(F32(1) - F32(F32(F32(2) * r0) * r0)) - F32(F32(F32(2) * r1) * r1))
                    p = [p[a] + F64(F32(F32(F32(z[a]) * F32(finger_depth)) * F32(finger_offset))) for a in range(3)]
                out.append(p + [F64(q)])
    return np.asarray(out, F64).reshape(-1, 4)


# ----------------------------------------------------------------------------------------------------------------- faces
def centres(vertices, faces):
    v = np.asarray(vertices, F32).astype(F64)[np.asarray(faces, np.int64)]
    return ((v[:, 0] + v[:, 1]) + v[:, 2]) / 3.0


def distances(c, pts):
    """(F,P) float64"""
    d = c[:, None, :] - pts[None, :, :3]
    return np.sqrt(((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2]))


def distances_scalar(c, pts):
    out = np.empty((len(c), len(pts)), F64)
    for f in range(len(c)):
        for p in range(len(pts)):
            dx, dy, dz = c[f, 0] - pts[p, 0], c[f, 1] - pts[p, 1], c[f, 2] - pts[p, 2]
            out[f, p] = np.sqrt(F64(F64(dx * dx) + F64(dy * dy)) + F64(dz * dz))
    return out


def aggregate(dist, q, aggregation="max", temp=150, rad=0.02):
    """(F,P) distances, (P,) qualities -> the aggregate of every face, before the clip"""
    with np.errstate(invalid="ignore", divide="ignore"):
        if aggregation == "max":
            return np.where(dist <= rad, q[None, :], 0.0).max(1)
        if aggregation == "softmax":
            w = np.where(dist <= rad, np.exp(q * F64(temp))[None, :], 0.0)
            return (w * q[None, :]).sum(1) / (w.sum(1) + 1e-5)
        if aggregation == "mean":
            w = np.exp(-dist * F64(temp))
            return (w * q[None, :]).sum(1) / w.sum(1)
    raise ValueError(aggregation)


def max_scalar(dist, q, rad=0.02):
    out = np.empty(len(dist), F64)
    for f in range(len(dist)):
        best = -np.inf
        for p in range(len(q)):
            v = q[p] if dist[f, p] <= rad else 0.0
            best = v if v > best else best
        out[f] = best
    return out


def normalise(a, th=0.5):
    with np.errstate(invalid="ignore"):
        return (np.minimum(np.maximum(a, F64(th)), 1.0) - F64(th)) / (1.0 - F64(th))


# ---------------------------------------------------------------------------------------------------------------- colour
def reds_table():
    a = np.array([[int(h[i:i + 2], 16) / 255.0 for i in (0, 2, 4)] for h in REDS_ANCHORS])
    return np.stack([np.interp(np.arange(256) / 255.0, np.arange(9) / 8.0, a[:, c]) for c in range(3)] + [np.ones(256)], 1)


def colour_index(a):
    """entry of the table for an affordance a in [0, 1] (not NaN): int(256 x), 256 -> 255, with x = (a a) (a a) -- within an ulp
    or two of the reference's a ** 4, which only a knife-edge face (below) could tell apart"""
    return np.minimum((((a * a) * (a * a)) * 256.0).astype(np.int64), 255)


def colours(a):
    """(F,) affordance -> (F,4) uint8"""
    bad = np.isnan(a)
    c = np.rint(255.0 * reds_table()[colour_index(np.where(bad, 0.0, a))]).astype(np.uint8)
    c[bad] = 0
    return c


def knife_edge_colours(a, eps=1e-6):
    """faces whose 256 a^4 lies within eps of one of the integers 1 .. 255, where a last-bit difference of a changes the entry (0 and
    256 are no edges: below 1 the entry is 0 and from 255 on it is 255, whichever side a falls on)"""
    a = np.where(np.isnan(a), 0.5, a)
    x = ((a * a) * (a * a)) * 256.0
    k = np.rint(x)
    return (np.abs(x - k) < eps) & (k >= 1) & (k <= 255)


# ------------------------------------------------------------------------------------------------------------------ whole
def affordance(qual, rot, vertices, faces, chunk=512, **kw):
    """-> (points (P,4), normalised affordance (F,) or None, colours (F,4) uint8, (F,P) pairs within 1e-9 of rad)"""
    p = dict(DEFAULTS, **kw)
    pts = points(qual, rot, p["size"], p["th"], p["finger_depth"], p["finger_offset"], p["move_center"])
    F = len(faces)
    if len(pts) == 0:
        return pts, None, np.tile(GREY, (F, 1)), 0
    c = centres(vertices, faces)
    raw, near = np.empty(F, F64), 0
    for a in range(0, F, chunk):
        d = distances(c[a:a + chunk], pts)
        near += int((np.abs(d - p["rad"]) < 1e-9).sum())
        raw[a:a + chunk] = aggregate(d, pts[:, 3], p["aggregation"], p["temp"], p["rad"])
    a = normalise(raw, p["th"])
    return pts, a, colours(a), near
