"""numpy restatement of giga_mesh_collide (include/giga_hip.h, "mesh against mesh"): float64, one rounding per operation -- numpy's
elementwise operations do not fuse, and nothing here goes through BLAS (`@`, np.dot) -- plus the same decision in exact rational
arithmetic (fractions.Fraction on the float32 inputs), and the bodies the tests share."""
from fractions import Fraction

import numpy as np

from render_emu import box_mesh, grid_square, icosphere, merge, plane_mesh  # noqa: F401  (re-exported mesh makers)

F32, F64 = np.float32, np.float64


# ----------------------------------------------------------------------------------------------------------- the restatement
def orient(a, b, c, d):
    """(..., 3) float64 arrays -> the header's determinant, in its order"""
    ux, uy, uz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
    vx, vy, vz = c[..., 0] - a[..., 0], c[..., 1] - a[..., 1], c[..., 2] - a[..., 2]
    wx, wy, wz = d[..., 0] - a[..., 0], d[..., 1] - a[..., 1], d[..., 2] - a[..., 2]
    return (ux * (vy * wz - vz * wy) - uy * (vx * wz - vz * wx)) + uz * (vx * wy - vy * wx)


def _decide(sp, sq, d0, d1, d2):
    """the segment rule from its five determinants (arrays of float64, or of exact integers)"""
    miss = ((sp > 0) & (sq > 0)) | ((sp < 0) & (sq < 0)) | ((sp == 0) & (sq == 0)) | (sp != sp) | (sq != sq)
    return ~miss & (((d0 >= 0) & (d1 >= 0) & (d2 >= 0)) | ((d0 <= 0) & (d1 <= 0) & (d2 <= 0)))


def seg_tri(p, q, a, b, c):
    """does segment (p, q) hit triangle (a, b, c)?  (..., 3) arrays, broadcast against each other"""
    p, q, a, b, c = np.broadcast_arrays(*[np.asarray(x, F64) for x in (p, q, a, b, c)])
    with np.errstate(invalid="ignore", over="ignore"):
        return _decide(orient(a, b, c, p), orient(a, b, c, q), orient(p, q, a, b), orient(p, q, b, c), orient(p, q, c, a))


def tri_tri(A, B):
    """(..., 3, 3) triangles (corner, coordinate), broadcast against each other -> bool: an edge of either hits the other"""
    A, B = np.asarray(A, F64), np.asarray(B, F64)
    out = np.zeros(np.broadcast_shapes(A.shape[:-2], B.shape[:-2]), bool)
    for X, Y in ((A, B), (B, A)):
        for i, j in ((0, 1), (1, 2), (2, 0)):
            out |= seg_tri(X[..., i, :], X[..., j, :], Y[..., 0, :], Y[..., 1, :], Y[..., 2, :])
    return out


def usable_triangles(v, f):
    """(k, 3, 3) float32 corners of the faces whose indices lie in the body and whose coordinates are finite, and their face ids"""
    v, f = np.asarray(v, F32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    if not ok.any():
        return np.zeros((0, 3, 3), F32), np.zeros(0, np.int64)
    tri = v[np.where(ok[:, None], f, 0)]
    ok &= np.isfinite(tri).all(axis=(1, 2))
    return tri[ok], np.nonzero(ok)[0]


def body_box(v, f):
    """(lo, hi) float32 over the usable triangles; (+inf, -inf) without any"""
    tri = usable_triangles(v, f)[0].reshape(-1, 3)
    if not len(tri):
        return np.full(3, np.inf, F32), np.full(3, -np.inf, F32)
    return tri.min(axis=0), tri.max(axis=0)


def culled(mesh_a, mesh_b):
    """the triangles of either body that take part: (A (ka, 3, 3), B (kb, 3, 3)) float32, both empty for disjoint boxes"""
    (la, ha), (lb, hb) = body_box(*mesh_a), body_box(*mesh_b)
    lo, hi = np.maximum(la, lb), np.minimum(ha, hb)
    none = np.zeros((0, 3, 3), F32)
    if not (lo <= hi).all():
        return none, none
    out = []
    for mesh in (mesh_a, mesh_b):
        tri = usable_triangles(*mesh)[0]
        out.append(tri[((tri.min(axis=1) <= hi) & (tri.max(axis=1) >= lo)).all(axis=1)])
    return out[0], out[1]


def pair_hit(mesh_a, mesh_b, chunk=1 << 16):
    A, B = culled(mesh_a, mesh_b)
    if not len(A) or not len(B):
        return False
    rows = max(1, chunk // len(B))
    for at in range(0, len(A), rows):
        if tri_tri(A[at:at + rows, None], B[None]).any():
            return True
    return False


def mesh_collide(meshes, pairs):
    """the decision function `giga_amd.scenes.generate_packed_scenes(collide=...)` takes: surface test only, (P,) bool"""
    meshes = [(np.asarray(v, F32).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)) for v, f in meshes]
    memo, out = {}, []
    for a, b in np.asarray(pairs, np.int64).reshape(-1, 2):
        key = (min(a, b), max(a, b))                        # the rule is symmetric by construction
        if key not in memo:
            memo[key] = pair_hit(meshes[key[0]], meshes[key[1]])
        out.append(memo[key])
    return np.asarray(out, bool)


# ------------------------------------------------------------------------------------------------------------- exact decision
def exact_integers(*arrays):
    """float32 arrays -> object arrays of Python integers, all scaled by one power of two (exact: through fractions.Fraction)"""
    fr = [[Fraction(float(x)) for x in np.asarray(a, F32).ravel()] for a in arrays]
    den = max([x.denominator for row in fr for x in row] or [1])          # denominators are powers of two: the largest is the lcm
    out = []
    for a, row in zip(arrays, fr):
        ints = np.empty(len(row), object)
        ints[:] = [int(x * den) for x in row]
        out.append(ints.reshape(np.shape(a)))
    return out


def tri_tri_exact(A, B):
    """(ka, 3, 3), (kb, 3, 3) float32 -> (ka, kb) bool: the header's rule with every determinant's sign exact"""
    A, B = exact_integers(A, B)
    out = np.zeros((len(A), len(B)), bool)
    for X, Y, flip in ((A, B, False), (B, A, True)):
        # plane determinants of every corner of X against every triangle of Y: (kx, 3, ky)
        s = orient(Y[None, None, :, 0], Y[None, None, :, 1], Y[None, None, :, 2], X[:, :, None, :])
        for i, j in ((0, 1), (1, 2), (2, 0)):
            sp, sq = s[:, i], s[:, j]
            cand = ~(((sp > 0) & (sq > 0)) | ((sp < 0) & (sq < 0)) | ((sp == 0) & (sq == 0))).astype(bool)
            ix, iy = np.nonzero(cand)
            if not len(ix):
                continue
            p, q, y = X[ix, i], X[ix, j], Y[iy]
            d0, d1, d2 = orient(p, q, y[:, 0], y[:, 1]), orient(p, q, y[:, 1], y[:, 2]), orient(p, q, y[:, 2], y[:, 0])
            hit = (((d0 >= 0) & (d1 >= 0) & (d2 >= 0)) | ((d0 <= 0) & (d1 <= 0) & (d2 <= 0))).astype(bool)
            if flip:
                out[iy[hit], ix[hit]] = True
            else:
                out[ix[hit], iy[hit]] = True
    return out


# --------------------------------------------------------------------------------------------------------------------- bodies
def transform(mesh, R=None, t=(0, 0, 0), scale=1.0):
    v, f = mesh
    v = np.asarray(v, F64) * scale
    if R is not None:
        v = np.stack([v[:, 0] * R[k, 0] + v[:, 1] * R[k, 1] + v[:, 2] * R[k, 2] for k in range(3)], axis=1)
    return (v + np.asarray(t, F64)).astype(F32), np.asarray(f, np.int32)


def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def random_bodies(seed):
    """8 randomly posed boxes (12 triangles each) and 4 icospheres of subdivision 1 (80 each), crowded into a 0.3 m cube"""
    rng = np.random.default_rng([20261, seed])
    out = []
    for _ in range(8):
        half = rng.uniform(0.02, 0.07, 3)
        out.append(transform(box_mesh(-half, half), random_rotation(rng), rng.uniform(0.05, 0.25, 3)))
    for _ in range(4):
        out.append(transform(icosphere((0, 0, 0), rng.uniform(0.03, 0.07), 1), random_rotation(rng), rng.uniform(0.05, 0.25, 3)))
    return out


def gpu_bodies(seed):
    """random_bodies plus an icosphere of subdivision 2 (320 triangles: more than one tile), a body of exactly 257 triangles, one
    of 1 triangle and one of 0"""
    rng = np.random.default_rng([20262, seed])
    out = random_bodies(seed)
    out.append(transform(icosphere((0, 0, 0), 0.09, 2), random_rotation(rng), rng.uniform(0.1, 0.2, 3)))
    sheet = merge(grid_square(-0.1, -0.1, 0.0125, 16, 8, 0.0), (np.array([[0, 0, -0.05], [0.05, 0.01, 0.05], [-0.03, 0.04, 0.06]], F32),
                                                                 np.array([[0, 1, 2]], np.int32)))
    assert len(sheet[1]) == 257
    out.append(transform(sheet, random_rotation(rng), rng.uniform(0.1, 0.2, 3)))
    out.append(transform((np.array([[-0.2, -0.1, 0.0], [0.2, -0.1, 0.01], [0.0, 0.2, -0.02]]), np.array([[0, 1, 2]])),
                         random_rotation(rng), rng.uniform(0.1, 0.2, 3)))
    out.append((np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32), np.zeros((0, 3), np.int32)))
    return out


def l_prism(size=0.1, notch=0.06, height=0.05):
    """a non-convex L-shaped prism: the square [0, size]^2 without the notch (size - notch, size]^2, extruded to `height`.
    12 vertices, 20 triangles, closed."""
    s, c = size, size - notch
    ring = [(0, 0), (s, 0), (s, c), (c, c), (c, s), (0, s)]                # counter-clockwise
    v = [[x, y, 0.0] for x, y in ring] + [[x, y, height] for x, y in ring]
    cap = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)]                     # a fan about the corner (0, 0): inside the L
    f = [[k, j, i] for i, j, k in cap] + [[i + 6, j + 6, k + 6] for i, j, k in cap]
    for i in range(6):
        j = (i + 1) % 6
        f += [[i, j, j + 6], [i, j + 6, i + 6]]
    return np.asarray(v, F32), np.asarray(f, np.int32)


# ---------------------------------------------------------------------------------------------------------------- object sets
OBJECT_MAKERS = {
    "box_a": lambda: box_mesh((-0.025, -0.02, -0.03), (0.025, 0.02, 0.03)),
    "box_b": lambda: box_mesh((-0.03, -0.015, -0.02), (0.03, 0.015, 0.02)),
    "box_c": lambda: box_mesh((-0.02, -0.02, -0.035), (0.02, 0.02, 0.035)),
    "sphere": lambda: icosphere((0, 0, 0), 0.03, 1),
    "prism": lambda: transform(l_prism(0.07, 0.04, 0.05), t=(-0.035, -0.035, -0.025)),
    "prism_sunk": lambda: transform(l_prism(0.07, 0.04, 0.05), t=(-0.035, -0.035, -0.04)),   # (its origin lies above its centre)
}
BOX_HALF = {"box_a": (0.025, 0.02, 0.03), "box_b": (0.03, 0.015, 0.02), "box_c": (0.02, 0.02, 0.035)}


def write_obj(path, v, f):
    with open(path, "w") as fh:
        for p in np.asarray(v, F64):
            fh.write("v %r %r %r\n" % tuple(float(x) for x in p))
        for t in np.asarray(f, np.int64):
            fh.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


def write_object_set(root, names, urdf=True):
    """<root>/<name>.obj for every name, and with urdf=True a one-link <name>.urdf beside it"""
    import os
    os.makedirs(root, exist_ok=True)
    for name in names:
        write_obj(os.path.join(str(root), name + ".obj"), *OBJECT_MAKERS[name]())
        if urdf:
            with open(os.path.join(str(root), name + ".urdf"), "w") as fh:
                fh.write('<?xml version="1.0"?>\n<robot name="%s"><link name="base"><visual><geometry><mesh filename="%s.obj" '
                         'scale="1 1 1"/></geometry></visual></link></robot>\n' % (name, name))
    return root
