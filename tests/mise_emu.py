"""Dict / set restatement of the reference's utils/libmise/mise.pyx (MISE: query, update, to_dense), the yardstick of the device
kernels (csrc/giga_mise.hip).  Pinned to the reference's own compiled libmise by tests/golden/g19_mise.npz
(tools/make_mise_goldens.py, tests/test_mise_host.py).

A lattice point is its (i, j, k) on the (resolution + 1)^3 lattice, resolution = resolution0 << depth; a voxel is
(level, vx, vy, vz) with edge 1 << (depth - level).  Values are float64 and compared with `>=` / `<=` against a float64 threshold,
as mise.pyx does (a float32 value is widened first)."""
import numpy as np


class MISE:
    def __init__(self, resolution0, depth, threshold):
        self.resolution0, self.depth, self.threshold = int(resolution0), int(depth), float(threshold)
        self.resolution = self.resolution0 << self.depth
        r0, s = self.resolution0, 1 << self.depth
        # True: leaf, False: inner node (mise.pyx:57-72)
        self.voxels = {(0, i, j, k): True for i in range(r0) for j in range(r0) for k in range(r0)}
        # value, or None while unknown; insertion order is mise.pyx's grid_points order (mise.pyx:76-85)
        self.points = {(i * s, j * s, k * s): None for i in range(r0 + 1) for j in range(r0 + 1) for k in range(r0 + 1)}

    def linear(self, p):
        n = self.resolution + 1
        return (p[0] * n + p[1]) * n + p[2]

    def query(self):
        """(n, 3) int64 array of the unknown points, in the reference's order (mise.pyx:106-128)."""
        pts = [p for p, v in self.points.items() if v is None]
        return np.array(pts, dtype=np.int64).reshape(-1, 3)

    def query_linear(self):
        """The same set as sorted int32 linear indices (the device's order)."""
        q = self.query()
        n = self.resolution + 1
        return np.sort((q[:, 0] * n + q[:, 1]) * n + q[:, 2]).astype(np.int32)

    def _leaf_of(self, x, y, z):
        """The leaf voxel that contains unit cell (x, y, z), or None outside the grid (mise.pyx:283-347)."""
        r = self.resolution
        if not (0 <= x < r and 0 <= y < r and 0 <= z < r):
            return None
        for level in range(self.depth + 1):
            sh = self.depth - level
            key = (level, x >> sh, y >> sh, z >> sh)
            if self.voxels[key]:
                return key
        raise AssertionError("an inner node at the last level")

    def update(self, points, values):
        """mise.pyx:87-104, 184-235."""
        points, values = np.asarray(points), np.asarray(values, dtype=np.float64)
        assert points.shape == (len(values), 3)
        for p, v in zip(map(tuple, points.tolist()), values.tolist()):
            if p not in self.points:
                raise ValueError("Point not in grid!")
            self.points[p] = v
        pos, neg = set(), set()
        for (x, y, z), v in self.points.items():
            if v is None:
                continue
            for i in (-1, 0):
                for j in (-1, 0):
                    for k in (-1, 0):
                        leaf = self._leaf_of(x + i, y + j, z + k)
                        if leaf is None:
                            continue
                        if v >= self.threshold:
                            pos.add(leaf)
                        if v <= self.threshold:
                            neg.add(leaf)
        for key in [k for k, is_leaf in self.voxels.items() if is_leaf and k[0] < self.depth and k in pos and k in neg]:
            self._subdivide(key)

    def _subdivide(self, key):
        """mise.pyx:237-280."""
        level, vx, vy, vz = key
        self.voxels[key] = False
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    self.voxels[(level + 1, 2 * vx + i, 2 * vy + j, 2 * vz + k)] = True
        size = 1 << (self.depth - level)
        half = size >> 1
        for i in range(3):
            for j in range(3):
                for k in range(3):
                    self.points.setdefault((vx * size + i * half, vy * size + j * half, vz * size + k * half), None)

    def to_dense(self):
        """mise.pyx:130-164; an unknown point holds 0 (mise.pyx:350-355).  float64, NaN where nothing could be copied."""
        n = self.resolution + 1
        out = np.full((n, n, n), np.nan)
        for p, v in self.points.items():
            out[p] = 0.0 if v is None else v
        for i in range(1, n):
            hole = np.isnan(out[i])
            out[i][hole] = out[i - 1][hole]
        for j in range(1, n):
            hole = np.isnan(out[:, j])
            out[:, j][hole] = out[:, j - 1][hole]
        for k in range(1, n):
            hole = np.isnan(out[:, :, k])
            out[:, :, k][hole] = out[:, :, k - 1][hole]
        return out


def run(field, resolution0, depth, threshold, max_rounds=64):
    """Drive MISE with lookups into `field` ((R+1)^3, any float dtype; widened to float64 like generation.py:137-139).
    Returns (list of per-round sorted int32 linear query indices, to_dense() as float32)."""
    field = np.asarray(field)
    m = MISE(resolution0, depth, threshold)
    assert field.shape == (m.resolution + 1,) * 3
    rounds = []
    q = m.query()
    while len(q):
        assert len(rounds) < max_rounds
        rounds.append(m.query_linear())
        m.update(q, field[q[:, 0], q[:, 1], q[:, 2]].astype(np.float64))
        q = m.query()
    return rounds, m.to_dense().astype(np.float32)
