"""numpy restatement of the depth fusion (include/giga_hip.h, giga_tsdf_integrate / giga_tsdf_cloud_*), float64 and float32
exactly where the header says so, written from the header's text and not from the kernel; plus a small analytic depth renderer
(float64 ray casting of a ground plane, spheres and boxes) that gives the tests their images from seeds.

Every float32 step below is a numpy float32 operation (one IEEE rounding), every float64 step a float64 one; numpy never fuses
a multiply with an add, which is what the kernel is compiled to match."""
import numpy as np

F32 = np.float32


def integrate(tsdf, weight, depth_imgs, extrinsics, intrinsic, length, sdf_trunc=None, depth_scale=1.0, depth_trunc=2.0, stats=None):
    """tsdf, weight (R, R, R) float32, updated in place and returned; depth_imgs (n, H, W) float32; extrinsics (n, 4, 4) float64;
    intrinsic = (fx, fy, cx, cy).  stats (a dict) receives 'voxel_views' and 'knife_edge': the voxel-views whose u_f or v_f lies
    within 1e-9 of an integer or of a bound of the image test, or whose sdf lies within one ulp of -sdf_trunc."""
    R = tsdf.shape[0]
    assert tsdf.shape == weight.shape == (R, R, R) and tsdf.dtype == weight.dtype == F32
    depth_imgs = np.asarray(depth_imgs, F32)
    n = len(depth_imgs)
    H, W = depth_imgs.shape[1:] if n else (1, 1)
    fx, fy, cx, cy = (float(v) for v in intrinsic)
    voxel = float(length) / R
    if sdf_trunc is None:
        sdf_trunc = 4 * voxel
    neg_trunc, inv_trunc = -F32(sdf_trunc), F32(1.0 / sdf_trunc)
    c = (np.arange(R, dtype=np.float64) + 0.5) * voxel
    px, py, pz = (a.reshape(-1) for a in np.meshgrid(c, c, c, indexing="ij"))
    t, w = tsdf.reshape(-1), weight.reshape(-1)
    knife = views = 0
    for k in range(n):
        E = np.asarray(extrinsics[k], np.float64).reshape(4, 4)
        zc = ((E[2, 0] * px + E[2, 1] * py) + E[2, 2] * pz) + E[2, 3]
        i0 = np.nonzero(zc > 0.0)[0]
        zc = zc[i0]
        xc = ((E[0, 0] * px[i0] + E[0, 1] * py[i0]) + E[0, 2] * pz[i0]) + E[0, 3]
        yc = ((E[1, 0] * px[i0] + E[1, 1] * py[i0]) + E[1, 2] * pz[i0]) + E[1, 3]
        uf = (xc * fx / zc + cx) + 0.5
        vf = (yc * fy / zc + cy) + 0.5
        if stats is not None:
            views += len(i0)
            near = np.zeros(len(i0), bool)
            for f, hi in ((uf, W - 0.0001), (vf, H - 0.0001)):
                near |= np.abs(f - np.rint(f)) < 1e-9
                near |= (np.abs(f - 0.0001) < 1e-9) | (np.abs(f - hi) < 1e-9)
        inside = (uf >= 0.0001) & (uf < W - 0.0001) & (vf >= 0.0001) & (vf < H - 0.0001)
        if stats is not None:
            near &= np.isfinite(uf) & np.isfinite(vf)
            knife += int(near.sum())
        i1 = np.nonzero(inside)[0]
        u, v = uf[i1].astype(np.int64), vf[i1].astype(np.int64)
        d = depth_imgs[k][v, u] / F32(depth_scale)
        d = np.where(d >= F32(depth_trunc), F32(0), d)
        i2 = np.nonzero(d > 0)[0]
        u, v, d, z2 = u[i2], v[i2], d[i2], zc[i1][i2]
        a, b = (u.astype(np.float64) - cx) / fx, (v.astype(np.float64) - cy) / fy
        m = np.sqrt((a * a + b * b) + 1.0).astype(F32)
        sdf = ((d.astype(np.float64) - z2) * m.astype(np.float64)).astype(F32)
        if stats is not None:
            knife += int((np.abs(sdf - neg_trunc) <= np.spacing(np.abs(neg_trunc))).sum())
        i3 = np.nonzero(sdf > neg_trunc)[0]
        cell = i0[i1][i2][i3]
        s = np.minimum(F32(1.0), sdf[i3] * inv_trunc)
        assert s.dtype == F32
        t[cell] = (t[cell] * w[cell] + s) / (w[cell] + F32(1.0))
        w[cell] = w[cell] + F32(1.0)
    if stats is not None:
        stats["voxel_views"] = stats.get("voxel_views", 0) + views
        stats["knife_edge"] = stats.get("knife_edge", 0) + knife
    return tsdf, weight


def valid(tsdf, weight):
    t = tsdf.astype(np.float64)
    return (weight != 0) & (t >= -0.98) & (t < 0.98)


def export_grid(tsdf, weight):
    """get_grid through extract_voxel_grid: (tsdf + 1) / 2 in double where the voxel is valid, 0 elsewhere; float32."""
    g = ((tsdf.astype(np.float64) + 1.0) * 0.5).astype(F32)
    return np.where(valid(tsdf, weight), g, F32(0))


def fuse(depth_imgs, extrinsics, intrinsic, length, R, stats=None):
    """A new volume with all views: (tsdf, weight, grid)."""
    t, w = np.zeros((R, R, R), F32), np.zeros((R, R, R), F32)
    integrate(t, w, depth_imgs, extrinsics, intrinsic, length, stats=stats)
    return t, w, export_grid(t, w)


def cloud(tsdf, weight, length):
    """(n, 3) float32 zero-crossing points, in cell order and then axis order."""
    R = tsdf.shape[0]
    voxel = float(length) / R
    ok = valid(tsdf, weight)
    idx = np.stack(np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij"), -1)      # (R, R, R, 3)
    p0 = (idx.astype(np.float64) + 0.5) * voxel
    flags = np.zeros((R, R, R, 3), bool)
    pts = np.zeros((R, R, R, 3, 3), F32)
    for i in range(3):
        f1 = np.roll(tsdf, -1, axis=i)
        ok1 = np.roll(ok, -1, axis=i)
        has = idx[..., i] + 1 < R - 1
        flags[..., i] = ok & has & ok1 & ((tsdf * f1) < 0)
        a0, a1 = np.abs(tsdf.astype(np.float64)), np.abs(f1.astype(np.float64))
        with np.errstate(invalid="ignore", divide="ignore"):
            r = (p0[..., i] * a1 + (p0[..., i] + voxel) * a0) / (a0 + a1)
        q = p0.copy()
        q[..., i] = r
        pts[..., i, :] = q.astype(F32)
    return pts[flags]


# ------------------------------------------------------------------------------------------------ poses and scenes
def quat_matrix(pose):
    """4x4 of the 7-list [qx, qy, qz, qw, x, y, z] (scipy's from_quat normalises the quaternion)."""
    x, y, z, w = np.asarray(pose[:4], np.float64) / np.linalg.norm(np.asarray(pose[:4], np.float64))
    m = np.eye(4)
    m[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    m[:3, 3] = pose[4:]
    return m


def six_views(size, n=6, N=None):
    """The extrinsics of simulation.py's acquire_tsdf (top view branch): n of N cameras on a circle at theta = pi / 6,
    radius 2 size, about (size / 2, size / 2, 0)."""
    from giga_amd.perception import camera_on_sphere
    origin = np.eye(4)
    origin[:3, 3] = [size / 2, size / 2, 0.0]
    N = N if N else n
    return np.stack([camera_on_sphere(origin, 2.0 * size, np.pi / 6.0, 2.0 * np.pi * k / N) for k in range(n)])


SIM_INTRINSIC = (640, 480, 540.0, 540.0, 320.0, 240.0)       # width, height, fx, fy, cx, cy of the reference's simulated camera
SMALL_INTRINSIC = (53, 37, 45.0, 44.0, 26.25, 18.5)


def make_scene(seed, size=0.3):
    """Ground plane z = 0.05 plus spheres and axis-aligned boxes resting on it, from a seed."""
    rng = np.random.default_rng(seed)
    spheres, boxes = [], []
    for _ in range(int(rng.integers(1, 4))):
        r = rng.uniform(0.02, 0.045)
        spheres.append((np.r_[rng.uniform(0.07, size - 0.07, 2), 0.05 + r * rng.uniform(0.6, 1.0)], r))
    for _ in range(int(rng.integers(1, 3))):
        h = rng.uniform(0.015, 0.04, 3)
        c = np.r_[rng.uniform(0.07, size - 0.07, 2), 0.05 + h[2]]
        boxes.append((c - h, c + h))
    return {"plane_z": 0.05, "spheres": spheres, "boxes": boxes}


def render(scene, extrinsic, intrinsic):
    """Depth image (H, W) float32 of the scene: the camera-frame z of the first hit of the ray through each pixel centre, 0
    where nothing is hit.  float64 inside."""
    W, H, fx, fy, cx, cy = intrinsic
    E = np.asarray(extrinsic, np.float64)
    Rm, tv = E[:3, :3], E[:3, 3]
    o = -Rm.T @ tv                                               # camera centre in the task frame
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dc = np.stack(((u - cx) / fx, (v - cy) / fy, np.ones_like(u)), -1)          # camera-frame direction with z = 1
    d = dc @ Rm                                                  # R^T dc, row-wise
    best = np.full((H, W), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (scene["plane_z"] - o[2]) / d[..., 2]
        best = np.where((s > 0) & (s < best), s, best)
        for c, r in scene["spheres"]:
            oc = o - c
            a = (d * d).sum(-1)
            b = d @ oc
            disc = b * b - a * (oc @ oc - r * r)
            s = (-b - np.sqrt(np.where(disc >= 0, disc, np.nan))) / a
            best = np.where((s > 0) & (s < best), s, best)
        for lo, hi in scene["boxes"]:
            t0, t1 = (lo - o) / d, (hi - o) / d
            near, far = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
            best = np.where((near <= far) & (near > 0) & (near < best), near, best)
    return np.where(np.isfinite(best), best, 0.0).astype(F32)


def render_views(scene, extrinsics, intrinsic):
    return np.stack([render(scene, e, intrinsic) for e in extrinsics]) if len(extrinsics) else np.zeros((0, intrinsic[1], intrinsic[0]), F32)
