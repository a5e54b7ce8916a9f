"""numpy restatement of csrc/giga_mesh.hip (classify / scan / emit in cell order, reading the case tables from the generated
header) and the mesh invariants that the CPU and GPU mesh tests share.  Not a test module."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "giga_amd", "csrc", "giga_mc_tables.h")
PAD = np.float32(-1e6)
CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))


def parse_tables(path=HEADER):
    """(ntri[256], tris[256][16]) as written in the header."""
    text = open(path).read()
    ntri = re.search(r"GIGA_MC_NTRI\[256\] = \{(.*?)\};", text, re.S).group(1)
    tris = re.search(r"GIGA_MC_TRIS\[256\]\[16\] = \{(.*)\};", text, re.S).group(1)
    ntri = np.array([int(t) for t in re.findall(r"\d+", ntri)], dtype=np.int64)
    tris = np.array([int(t) for t in re.findall(r"\d+", tris)], dtype=np.int64).reshape(256, 16)
    assert ntri.shape == (256,)
    return ntri, tris


def iso_of(threshold):
    return float(np.log(threshold) - np.log(1.0 - threshold))


def _corner_bits(grid, iso):
    """Padded samples and their case bits: value <= iso, compared in double like marchingcubes.h:65-68."""
    pad = np.pad(np.asarray(grid, dtype=np.float32), 1, constant_values=PAD)
    return pad, pad.astype(np.float64) <= iso


def _edge_owner(e):
    a, b = EDGES[e]
    hi = CORNERS[a] if CORNERS[a].sum() > CORNERS[b].sum() else CORNERS[b]
    axis = int(np.nonzero(CORNERS[a] != CORNERS[b])[0][0])
    return axis, 1 - hi                                    # (axis, cells back along x, y, z)


def marching_cubes(grid, iso, box_size=1.0, tables=None):
    """The three passes of giga_mesh.hip for one scene.  Returns (vertices (V,3) float32, triangles (F,3) int32), in the
    kernel's order: cells with z fastest, the owned x / y / z edge inside a cell."""
    ntri, tris = tables if tables is not None else parse_tables()
    pad, bits = _corner_bits(grid, iso)
    n = np.array(grid.shape)
    cx, cy, cz = n + 1
    cube = np.zeros((cx, cy, cz), dtype=np.int64)
    for m, (dx, dy, dz) in enumerate(CORNERS):
        cube |= bits[dx:dx + cx, dy:dy + cy, dz:dz + cz].astype(np.int64) << m
    b = lambda m: (cube >> m) & 1
    flags = np.stack([b(6) ^ b(7), b(6) ^ b(5), b(6) ^ b(2)], axis=-1).reshape(-1, 3)       # owned x, y, z edge crossed
    nv = flags.sum(axis=1)
    voff = np.cumsum(nv) - nv                                                             # exclusive scan, cell order
    nt = ntri[cube.reshape(-1)]
    # ---- vertices
    val = pad.astype(np.float64)
    i, j, k = np.meshgrid(np.arange(cx), np.arange(cy), np.arange(cz), indexing="ij")
    i, j, k = i.reshape(-1), j.reshape(-1), k.reshape(-1)
    v6 = val[i + 1, j + 1, k + 1]
    verts = np.zeros((int(nv.sum()), 3), dtype=np.float32)
    hi = np.stack([i + 1.5, j + 1.5, k + 1.5], axis=-1)

    def to_model(p, axis):
        v = p - 0.5
        v = v - 1.0
        v = v / float(n[axis] - 1)
        return box_size * (v - 0.5)

    for axis in range(3):
        sel = np.nonzero(flags[:, axis])[0]
        d = [0, 0, 0]
        d[axis] = 1
        other = val[i[sel] + 1 - d[0], j[sel] + 1 - d[1], k[sel] + 1 - d[2]]
        c6 = v6[sel]
        x1 = hi[sel, axis]
        # (the f1 == f2 midpoint of marchingcubes.cpp:290-297 is restated for parity; a crossed edge never has equal ends)
        with np.errstate(divide="ignore", invalid="ignore"):
            if axis == 0:       # edge 6: corner 6 -> 7, from x1 down to x1 - 1
                p = np.where(other == c6, (x1 - 1.0 + x1) / 2, (-1.0) * (iso - c6) / (other - c6) + x1)
            else:               # edges 5, 10: corner 5 / 2 -> 6, from x1 - 1 up to x1
                p = np.where(other == c6, (x1 + (x1 - 1.0)) / 2, 1.0 * (iso - other) / (c6 - other) + (x1 - 1.0))
        out = np.stack([to_model(hi[sel, a], a) for a in range(3)], axis=-1)
        out[:, axis] = to_model(p, axis)
        verts[voff[sel] + flags[sel, :axis].sum(axis=1)] = out.astype(np.float32)
    # ---- triangles
    cells = np.nonzero(nt)[0]
    toff = np.cumsum(nt) - nt
    faces = np.zeros((int(nt.sum()), 3), dtype=np.int32)
    owner = [_edge_owner(e) for e in range(12)]
    stride = np.array([cy * cz, cz, 1])
    for c in cells:
        t = tris[cube.reshape(-1)[c]]
        for m in range(nt[c]):
            for q in range(3):
                axis, back = owner[t[3 * m + q]]
                oc = c - int((back * stride).sum())
                assert oc >= 0 and flags[oc, axis]
                faces[toff[c] + m, q] = voff[oc] + flags[oc, :axis].sum()
    return verts, faces


def edges_in_kernel_order(grid, iso):
    """The crossed edges as `crossed_edges` keys them, in the order in which the kernel (and `marching_cubes` above) writes
    their vertices: cells with z fastest, inside a cell the owned x, y, z edge.  Cell (i, j, k) has its corner 6 at padded
    sample (i+1, j+1, k+1); an owned edge's lower end is one sample back along its axis."""
    _, bits = _corner_bits(grid, iso)
    c6 = bits[1:, 1:, 1:]
    flags = np.stack([c6 ^ bits[:-1, 1:, 1:], c6 ^ bits[1:, :-1, 1:], c6 ^ bits[1:, 1:, :-1]], axis=-1)
    out = []
    for i, j, k, axis in np.argwhere(flags):               # C order: i, j, k, then axis
        q = [int(i) + 1, int(j) + 1, int(k) + 1]
        q[axis] -= 1
        out.append((int(axis), q[0], q[1], q[2]))
    return out


def crossed_edges(grid, iso):
    """{(axis, i, j, k)}: the crossed edge from padded sample (i, j, k) to its +axis neighbour."""
    _, bits = _corner_bits(grid, iso)
    out = set()
    for axis in range(3):
        a = np.swapaxes(bits, 0, axis)
        x = np.swapaxes(a[:-1] ^ a[1:], 0, axis)
        out |= {(axis, int(p[0]), int(p[1]), int(p[2])) for p in np.argwhere(x)}
    return out


def ambiguous_faces(grid, iso):
    """Number of cell faces of the padded grid with exactly two set corners on a diagonal."""
    _, bits = _corner_bits(grid, iso)
    n = 0
    for axis in range(3):
        b = np.moveaxis(bits, axis, 0)
        a00, a01, a10, a11 = b[:, :-1, :-1], b[:, :-1, 1:], b[:, 1:, :-1], b[:, 1:, 1:]
        n += int(((a00 == a11) & (a01 == a10) & (a00 != a01)).sum())
    return n


def near_threshold_edges(grid, iso, eps=1e-4):
    """The crossed edges with an endpoint within eps of iso (a value grid within eps may cross them or not)."""
    pad, _ = _corner_bits(grid, iso)
    near = np.abs(pad.astype(np.float64) - iso) <= eps
    out = set()
    for e in crossed_edges(grid, iso):
        axis, i, j, k = e
        q = [i, j, k]
        q[axis] += 1
        if near[i, j, k] or near[q[0], q[1], q[2]]:
            out.add(e)
    return out


def signed_volume(v, f):
    v = np.asarray(v, dtype=np.float64)
    if len(f) == 0:
        return 0.0
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def euler_characteristic(nv, f):
    if len(f) == 0:
        return 0
    f = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.unique(np.sort(e, axis=1), axis=0)
    return int(nv - len(e) + len(f))


def closed_and_oriented(nv, f):
    """Every undirected edge in exactly two triangles, once in each direction; every vertex used."""
    f = np.asarray(f, dtype=np.int64)
    if len(f) == 0:
        return nv == 0
    if f.min() < 0 or f.max() >= nv or len(np.unique(f)) != nv:
        return False
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    if (e[:, 0] == e[:, 1]).any():
        return False
    d = e[:, 0] * nv + e[:, 1]
    r = e[:, 1] * nv + e[:, 0]
    if len(np.unique(d)) != len(d):                      # a directed edge twice
        return False
    return bool(np.array_equal(np.sort(d), np.sort(r)))   # every directed edge has its reverse


def sort_rows(v):
    v = np.asarray(v)
    return v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))] if len(v) else v
