"""numpy restatement of the oriented cloud (giga_tsdf_cloud_emit_oriented) and of the grasp candidates (giga_grasp_candidates),
written from the text of include/giga_hip.h and not from the kernels.  Every step is a float64 numpy operation (one IEEE rounding;
numpy never fuses a multiply with an add); the points themselves are tsdf_emu.cloud's."""
import numpy as np

import tsdf_emu
from eval_emu import philox4x32_10
from noise_emu import u53

F32 = np.float32
STREAM = 0x47525350


# ------------------------------------------------------------------------------------------------ oriented cloud
def cloud_points64(tsdf, weight, length):
    """(m, 3) float64: the crossings before they are rounded to float32, in cell order and then axis order."""
    R = tsdf.shape[0]
    voxel = float(length) / R
    ok = tsdf_emu.valid(tsdf, weight)
    idx = np.stack(np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij"), -1)
    p0 = (idx.astype(np.float64) + 0.5) * voxel
    flags = np.zeros((R, R, R, 3), bool)
    pts = np.zeros((R, R, R, 3, 3), np.float64)
    for i in range(3):
        f1 = np.roll(tsdf, -1, axis=i)
        flags[..., i] = ok & (idx[..., i] + 1 < R - 1) & np.roll(ok, -1, axis=i) & ((tsdf * f1) < 0)
        a0, a1 = np.abs(tsdf.astype(np.float64)), np.abs(f1.astype(np.float64))
        with np.errstate(invalid="ignore", divide="ignore"):
            r = (p0[..., i] * a1 + (p0[..., i] + voxel) * a0) / (a0 + a1)
        q = p0.copy()
        q[..., i] = r
        pts[..., i, :] = q
    return pts[flags]


def trilinear(tsdf, q, voxel):
    """T(q) for q (m, 3) float64: the stored values only; a voxel outside the volume counts 0.0."""
    R = tsdf.shape[0]
    s = q / voxel - 0.5
    i = np.floor(s)
    r = s - i
    i = i.astype(np.int64)
    w = (1.0 - r, r)
    acc = None
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                ix, iy, iz = i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz
                inside = (ix >= 0) & (ix < R) & (iy >= 0) & (iy < R) & (iz >= 0) & (iz < R)
                f = np.where(inside, tsdf[np.clip(ix, 0, R - 1), np.clip(iy, 0, R - 1), np.clip(iz, 0, R - 1)].astype(np.float64), 0.0)
                term = ((w[dx][:, 0] * w[dy][:, 1]) * w[dz][:, 2]) * f
                acc = term if acc is None else acc + term
    return acc


def gradient_at(tsdf, p, length):
    """(m, 3) float64: n_c = T(p + g e_c) - T(p - g e_c) at the float64 points p, before it is normalised."""
    voxel = float(length) / tsdf.shape[0]
    g = 0.99 * voxel
    n = np.zeros((len(p), 3), np.float64)
    for c in range(3):
        hi, lo = p.copy(), p.copy()
        hi[:, c] = p[:, c] + g
        lo[:, c] = p[:, c] - g
        n[:, c] = trilinear(tsdf, hi, voxel) - trilinear(tsdf, lo, voxel)
    return n


def normals64_at(tsdf, p, length):
    """(m, 3) float64: the normals before they are rounded to float32."""
    if len(p) == 0:
        return np.zeros((0, 3))
    n = gradient_at(tsdf, p, length)
    z = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = n / np.sqrt(z)[:, None]
    return np.where((z > 0)[:, None], unit, 0.0)


def normals_at(tsdf, p, length):
    """(m, 3) float32 normals of the float64 points p."""
    return normals64_at(tsdf, p, length).astype(F32)


def cloud_oriented(tsdf, weight, length):
    """(points (m, 3) float32 -- tsdf_emu.cloud's --, normals (m, 3) float32)"""
    p = cloud_points64(tsdf, weight, length)
    points = tsdf_emu.cloud(tsdf, weight, length)
    assert np.array_equal(p.astype(F32).view(np.uint32), points.view(np.uint32))
    return points, normals_at(tsdf, p, length)


# ------------------------------------------------------------------------------------------------ candidates
def yaw_table(Y):
    yaws = np.linspace(0.0, np.pi, Y)
    return np.stack((np.sin(yaws / 2.0), np.cos(yaws / 2.0)), axis=1)


def eligible(points, normals, lower, upper):
    P, N = points.astype(np.float64), normals.astype(np.float64)
    lower, upper = np.asarray(lower, np.float64), np.asarray(upper, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
        return (np.isfinite(P).all(1) & np.isfinite(N).all(1) & (P >= lower).all(1) & (P <= upper).all(1) & (N[:, 2] > -0.1) & (d > 0))


def cross(a, b):
    return np.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), 1)


def unit(a):
    return a / np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])[:, None]


def frame_axes(N):
    """the columns (x, y, z) of the frame of the float64 normals N (m, 3)"""
    d = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
    z = (-N) / np.sqrt(d)[:, None]
    x = np.tile([1.0, 0.0, 0.0], (len(N), 1))
    dot = (x[:, 0] * z[:, 0] + x[:, 1] * z[:, 1]) + x[:, 2] * z[:, 2]
    x[np.abs(np.abs(dot) - 1.0) <= 1e-8 + 1e-4] = [0.0, 1.0, 0.0]
    y = cross(z, x)
    x = cross(y, z)
    return unit(x), unit(y), z


def frame_quat(N):
    """(m, 4) xyzw, normalised, sign as it comes"""
    x, y, z = frame_axes(N)
    M = np.stack((x, y, z), axis=2)                                        # M[:, r, c]
    t = (M[:, 0, 0] + M[:, 1, 1]) + M[:, 2, 2]
    choice = np.argmax(np.stack((M[:, 0, 0], M[:, 1, 1], M[:, 2, 2], t), 1), axis=1)       # the first largest
    q = np.zeros((len(N), 4))
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        m = choice == i
        q[m, i] = (1.0 - t[m]) + 2.0 * M[m, i, i]
        q[m, j] = M[m, j, i] + M[m, i, j]
        q[m, k] = M[m, k, i] + M[m, i, k]
        q[m, 3] = M[m, k, j] - M[m, j, k]
    m = choice == 3
    q[m, 0] = M[m, 2, 1] - M[m, 1, 2]
    q[m, 1] = M[m, 0, 2] - M[m, 2, 0]
    q[m, 2] = M[m, 1, 0] - M[m, 0, 1]
    q[m, 3] = 1.0 + t[m]
    return q / np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])[:, None]


def yaw_quats(q, table):
    """(m, Y, 4): q (0, 0, s, c) for every row (s, c) of the table"""
    s, c = table[None, :, 0], table[None, :, 1]
    q0, q1, q2, q3 = (q[:, i, None] for i in range(4))
    return np.stack((q0 * c + q1 * s, q1 * c - q0 * s, q2 * c + q3 * s, q3 * c - q2 * s), axis=2)


def candidates(points, normals, K, lower, upper, scene_id, seed, finger_depth=0.05, eps=0.1, Y=6):
    """One scene.  Returns (pos (K, 3), quat (K, Y, 4), index (K,) int32, E, depth (K,)); None in place of the arrays if E = 0."""
    idx = np.nonzero(eligible(points, normals, lower, upper))[0]
    E = len(idx)
    if E == 0:
        return None, None, None, 0, None
    w = philox4x32_10(np.arange(K), scene_id, 0, STREAM, seed & 0xffffffff, seed >> 32)
    e = (w[0].astype(np.uint64) * np.uint64(E)) >> np.uint64(32)
    index = idx[e.astype(np.int64)]
    lo, hi = -eps * finger_depth, (1.0 + eps) * finger_depth
    depth = lo + (hi - lo) * u53(w[2], w[3])
    P, N = points[index].astype(np.float64), normals[index].astype(np.float64)
    pos = P + N * depth[:, None]
    return pos, yaw_quats(frame_quat(N), yaw_table(Y)), index.astype(np.int32), E, depth


# ------------------------------------------------------------------------------------------------ inputs the tests share
def frame_normals():
    """random normals of any length, +-x and +-z exactly, and normals at 0.9999, 0.99989 and 0.99991 of |x . z|: the three
    straddle np.isclose(|x . z|, 1, 1e-4), which switches at 1 - (1e-8 + 1e-4) = 0.99989999"""
    rng = np.random.default_rng(5)
    n = [rng.normal(size=(500, 3)) * rng.uniform(0.2, 3.0, (500, 1))]
    n.append(np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 0, 1.0], [0, 0, -1.0], [0, 1.0, 0], [0, -1.0, 0]]))
    for c in (0.9999, 0.99989, 0.99991):
        for sign in (1.0, -1.0):
            for phi in (0.3, 2.1, 4.4):
                s = np.sqrt(1.0 - c * c)
                n.append(np.array([[sign * c, s * np.cos(phi), s * np.sin(phi)]]))
    return np.concatenate(n)


LOWER, UPPER = np.r_[0.02, 0.02, 0.05 + 0.005], np.r_[0.3 - 0.02, 0.3 - 0.02, 0.3]      # simulation.py:92-96 at size 0.3, table 0.05


def sampler_cloud(rng, n, eligible_at):
    """n points, of which exactly those at `eligible_at` are eligible: the others lie outside the box, point down, have a zero
    normal or hold a NaN"""
    points = rng.uniform(LOWER, UPPER, (n, 3)).astype(np.float32)
    normals = rng.normal(size=(n, 3))
    normals[:, 2] = np.abs(normals[:, 2])
    normals = (normals / np.linalg.norm(normals, axis=1)[:, None]).astype(np.float32)
    keep = np.zeros(n, bool)
    keep[list(eligible_at)] = True
    for k, i in enumerate(np.nonzero(~keep)[0]):
        kind = k % 5
        if kind == 0:
            points[i, k % 3] = np.float32(UPPER[k % 3]) + np.float32(1e-3)
        elif kind == 1:
            points[i, 2] = np.float32(0.054)
        elif kind == 2:
            normals[i] = (0.6, 0.0, -0.8)
        elif kind == 3:
            normals[i] = 0.0
        else:
            normals[i, k % 3] = np.nan
    return points, normals


def fake_execute(scene, pos, quat, max_opening_width):
    """an executor without physics: deterministic outcomes scrambled from the candidates' own numbers, about one success in four"""
    K, Y = quat.shape[:2]
    bits = (np.floor(np.abs(pos[:, :1]) * 1e6).astype(np.int64) * (2 * np.arange(Y)[None, :] + 3) // 7 + scene) % 4
    outcomes = (bits == 0).astype(np.int64)
    widths = max_opening_width * (0.25 + 0.5 * np.abs(quat[:, :, 3]))
    return outcomes, widths
