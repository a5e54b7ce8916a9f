"""Test-side numpy restatement of csrc/giga_refine.hip (float64): the closed-form gradient of the refinement loss per face from
(f, grad f, H) at the face points, the CSR corner sum, torch's RMSprop step, and the hand-made test mesh.  Test infrastructure
only."""
import numpy as np

EPS = 1e-10
LR, ALPHA, RMS_EPS = 1e-4, 0.99, 1e-8


def hand_mesh(n_faces, seed):
    """(vertices (V,3) float32, faces (F,3) int64), V = n_faces + 4, small triangles inside the cube.  Faces 0 .. min(F-1, 48)-1
    fan around vertex 0 (valence >= 40 from 41 faces on), the last face has zero area (two of its vertices coincide), the rest
    are random triples; the last vertex is referenced by no face."""
    rng = np.random.RandomState(seed)
    V = n_faces + 4
    centre = rng.uniform(-0.3, 0.3, size=3)
    v = (centre + 0.06 * rng.standard_normal((V, 3))).astype(np.float32)
    f = np.zeros((n_faces, 3), np.int64)
    fan = min(n_faces - 1, 48)
    for k in range(n_faces - 1):
        if k < fan:
            f[k] = (0, 1 + k, 2 + k)
        else:
            f[k] = rng.choice(V - 2, size=3, replace=False)
    a, b = 1, 2
    v[V - 2] = v[b]                                   # a second vertex at the position of b: e2 = 0 exactly, c = 0
    f[n_faces - 1] = (a, b, V - 2)
    return v, f


def degenerate(v, f):
    """Faces whose fp32 vertices give c = e1 x e2 = 0 exactly."""
    v = np.asarray(v, np.float64)
    c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 1]])
    return (c == 0).all(axis=1)


def dirichlet(n_faces, seed):
    """Given barycentric weights for the teacher-forced tests: numpy's Dirichlet(1/2,1/2,1/2), float32, rows renormalised."""
    e = np.random.RandomState(seed).dirichlet((0.5, 0.5, 0.5), size=n_faces).astype(np.float32)
    return e


def _normalize_jvp(a, na, y):
    d = na + EPS
    k = np.where(na > 0, (a * y).sum(-1, keepdims=True) / np.where(na > 0, na * d * d, 1.0), 0.0)
    return y / d - k * a


def face_grad(v, faces, eps, f, df, hess, tau=0.5, weight=0.01):
    """include/giga_hip.h, giga_refine_face_grad: -> (face_loss (F,2), face_grad (F,3,3)), float64.  hess (F,3) = (H_xy, H_xz,
    H_yz), the diagonal being zero."""
    v, eps, f, df, hess = (np.asarray(t, np.float64) for t in (v, eps, f, df, hess))
    F = faces.shape[0]
    v0, v1, v2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    sp, sm = 1.0 / (1.0 + np.exp(-f)), 1.0 / (1.0 + np.exp(f))
    s1 = (sp * sm)[:, None]
    s2 = s1 * (sm - sp)[:, None]
    g = s1 * df
    ng = np.linalg.norm(g, axis=1, keepdims=True)
    t = -g / (ng + EPS)
    e1, e2 = v1 - v0, v2 - v1
    c = np.cross(e1, e2)
    nc = np.linalg.norm(c, axis=1, keepdims=True)
    n = c / (nc + EPS)
    r = n - t
    loss = np.stack(((sp - tau) ** 2, (r * r).sum(1)), axis=1)
    y = (2 * weight / F) * r
    u = _normalize_jvp(g, ng, y)
    hxy, hxz, hyz = hess[:, 0:1], hess[:, 1:2], hess[:, 2:3]
    Hu = np.concatenate((hxy * u[:, 1:2] + hxz * u[:, 2:3], hxy * u[:, 0:1] + hyz * u[:, 2:3], hxz * u[:, 0:1] + hyz * u[:, 1:2]), axis=1)
    dq = ((2.0 / F) * (sp - tau)[:, None] * s1 + s2 * (df * u).sum(1, keepdims=True)) * df + s1 * Hu
    w = _normalize_jvp(c, nc, y)
    de1, de2 = np.cross(e2, w), np.cross(w, e1)
    out = np.stack((eps[:, 0:1] * dq - de1, eps[:, 1:2] * dq + de1 - de2, eps[:, 2:3] * dq + de2), axis=1)
    return loss, out


def csr(faces, n_vertices):
    """(corner_order (3F,), vertex_offsets (V+1,)): corners 3 face + i in a stable sort by vertex."""
    flat = np.asarray(faces).reshape(-1)
    order = np.argsort(flat, kind="stable")
    offsets = np.concatenate(([0], np.cumsum(np.bincount(flat, minlength=n_vertices))))
    return order, offsets


def vertex_grad(fgrad, faces, n_vertices):
    g = np.zeros((n_vertices, 3))
    np.add.at(g, np.asarray(faces).reshape(-1), np.asarray(fgrad, np.float64).reshape(-1, 3))
    return g


def rmsprop(v, sq, g):
    """torch.optim.RMSprop(lr=1e-4) defaults, float64: -> (v', sq')."""
    v, sq, g = (np.asarray(t, np.float64) for t in (v, sq, g))
    sq = ALPHA * sq + (1 - ALPHA) * g * g
    return v - LR * g / (np.sqrt(sq) + RMS_EPS), sq
