"""numpy restatement of the depth renderer (include/giga_hip.h, giga_depth_render), float64 throughout, brute force (every
triangle against every pixel), written from the header's text and not from the kernel; plus the mesh generators the tests use.

Every step below is a numpy float64 operation (one IEEE rounding); numpy never fuses a multiply with an add, which is what the
kernel is compiled to match."""
import numpy as np

F32 = np.float32


def camera_vertices(vertices, E):
    """a = E (x, y, z, 1) from the float32 vertices, every row ((e0 x + e1 y) + e2 z) + e3: (n, 3) float64"""
    v = np.asarray(vertices, F32).reshape(-1, 3).astype(np.float64)
    E = np.asarray(E, np.float64).reshape(4, 4)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((E[r, 0] * x + E[r, 1] * y) + E[r, 2] * z) + E[r, 3] for r in range(3)], 1)


def cross(P, Q):
    return (P[1] * Q[2] - P[2] * Q[1], P[2] * Q[0] - P[0] * Q[2], P[0] * Q[1] - P[1] * Q[0])


def render(vertices, faces, extrinsic, intrinsic, near=0.1, far=2.0, pixel_offset=0.0, stats=None):
    """Depth image (H, W) float32.  intrinsic = (W, H, fx, fy, cx, cy).  stats (a dict) receives 'knife_edge': the pixels where
    some triangle has |U|, |V| or |W| below 1e-12 (|U| + |V| + |W|) without being exactly 0, or an accepted z within one double
    ulp of near or far; and 'hits', the accepted (pixel, triangle) pairs."""
    W, H, fx, fy, cx, cy = intrinsic
    W, H = int(W), int(H)
    fx, fy, cx, cy, near, far, po = (np.float64(v) for v in (fx, fy, cx, cy, near, far, pixel_offset))
    cam = camera_vertices(vertices, extrinsic)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    dx = ((np.arange(W, dtype=np.float64) + po) - cx) / fx
    dy = ((np.arange(H, dtype=np.float64) + po) - cy) / fy
    DX, DY = np.meshgrid(dx, dy)                                   # (H, W): row v, column u
    best = np.full((H, W), np.inf)
    knife = np.zeros((H, W), bool)
    hits = 0
    with np.errstate(all="ignore"):
        for ia, ib, ic in faces:
            if min(ia, ib, ic) < 0 or max(ia, ib, ic) >= len(cam):
                continue                                           # an index outside the scene: skipped
            a, b, c = cam[ia], cam[ib], cam[ic]
            nbc, nca, nab = cross(b, c), cross(c, a), cross(a, b)
            U = (DX * nbc[0] + DY * nbc[1]) + nbc[2]
            V = (DX * nca[0] + DY * nca[1]) + nca[2]
            Wd = (DX * nab[0] + DY * nab[1]) + nab[2]
            S = (U + V) + Wd
            hit = (S != 0) & (((U >= 0) & (V >= 0) & (Wd >= 0)) | ((U <= 0) & (V <= 0) & (Wd <= 0)))
            z = ((U * a[2] + V * b[2]) + Wd * c[2]) / S
            ok = hit & (z >= near) & (z <= far)
            best = np.where(ok & (z < best), z, best)
            if stats is not None:
                hits += int(ok.sum())
                mag = 1e-12 * ((np.abs(U) + np.abs(V)) + np.abs(Wd))
                for e in (U, V, Wd):
                    knife |= (e != 0) & (np.abs(e) < mag)
                knife |= ok & ((np.abs(z - near) <= np.spacing(near)) | (np.abs(z - far) <= np.spacing(far)))
    if stats is not None:
        stats["knife_edge"] = stats.get("knife_edge", 0) + int(knife.sum())
        stats["hits"] = stats.get("hits", 0) + hits
    return np.where(best <= far, best, far).astype(F32)


def render_views(vertices, faces, extrinsics, intrinsic, near=0.1, far=2.0, pixel_offset=0.0, stats=None):
    if not len(extrinsics):
        return np.zeros((0, int(intrinsic[1]), int(intrinsic[0])), F32)
    return np.stack([render(vertices, faces, e, intrinsic, near, far, pixel_offset, stats) for e in extrinsics])


# ------------------------------------------------------------------------------------------------ meshes
def _mesh(v, f):
    return np.asarray(v, F32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)


def merge(*meshes):
    """one (vertices, faces) pair of several, faces re-based"""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return _mesh(np.concatenate(vs), np.concatenate(fs))


def box_mesh(lo, hi):
    """axis-aligned box, 8 vertices, 12 triangles (outward winding)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = [[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)]      # index 4 i + 2 j + k
    f = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]
    return _mesh(v, f)


def plane_mesh(z, extent):
    """the rectangle extent = (x0, x1, y0, y1) (or [-e, e]^2 for a number) at height z, 2 triangles"""
    x0, x1, y0, y1 = (-extent, extent, -extent, extent) if np.isscalar(extent) else extent
    return _mesh([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], [[0, 1, 2], [0, 2, 3]])


def icosphere(c, r, subdiv):
    """20 4^subdiv triangles on the sphere of radius r about c"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        mid, out = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c_ in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c_), midpoint(c_, a)
            out += [[a, ab, ca], [b, bc, ab], [c_, ca, bc], [ab, bc, ca]]
        f = out
    return _mesh(np.asarray(c, np.float64) + r * np.asarray(v), f)


def grid_square(x0, y0, step, nx, ny, z, flip=False):
    """(nx x ny) cells of side `step` from (x0, y0) at depth z, two triangles per cell; flip reverses the orientation of every
    second triangle"""
    v = [[x0 + i * step, y0 + j * step, z] for j in range(ny + 1) for i in range(nx + 1)]
    f = []
    for j in range(ny):
        for i in range(nx):
            p = j * (nx + 1) + i
            f.append([p, p + 1, p + nx + 2])
            f.append([p, p + nx + 1, p + nx + 2] if flip else [p, p + nx + 2, p + nx + 1])
    return _mesh(v, f)


PLANE_EXTENT = (-3.0, 3.3, -3.0, 3.3)         # covers every ray of the six-view circle about a 0.3 m workspace


def scene_to_mesh(scene, extent=PLANE_EXTENT):
    """the ground plane and the boxes (not the spheres) of a tsdf_emu.make_scene scene"""
    return merge(plane_mesh(scene["plane_z"], extent), *[box_mesh(lo, hi) for lo, hi in scene["boxes"]])
