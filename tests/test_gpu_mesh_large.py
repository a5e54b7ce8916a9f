"""GPU tests of marching cubes beyond 256 samples per axis (GIGA_MESH_MAX_N = 513, the largest MISE grid): thin grids that are
long along one axis against the numpy restatement of tests/mesh_emu.py, bit for bit as tests/test_gpu_mesh.py compares, and a
257^3 sphere by its invariants."""
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import _capi
from giga_amd.mesh import marching_cubes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_emu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RADIUS = 0.3


def _run(grid, iso, box):
    v, t, counts = marching_cubes(grid[None], iso, box)
    torch.cuda.synchronize()
    assert tuple(v.shape) == (int(counts[0, 0]), 3) and tuple(t.shape) == (int(counts[0, 1]), 3)
    return v.cpu().numpy(), t.cpu().numpy()


@pytest.mark.parametrize("shape", [(300, 5, 6), (5, 300, 6), (6, 5, 300)])
def test_long_thin_grids_equal_the_emulation(shape):
    assert max(shape) > 256 and max(shape) <= _capi.MESH_MAX_N
    i, j, k = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    long_axis = (i, j, k)[int(np.argmax(shape))]
    others = i + j + k - long_axis
    grid = (np.cos(0.37 * long_axis) + 0.5 * np.sin(0.9 * others + 0.3) - 0.1).astype(np.float32)    # crossings along the whole axis
    v, f = _run(torch.from_numpy(grid).to(DEV), 0.05, 1.2)
    ev, ef = mesh_emu.marching_cubes(grid, 0.05, 1.2)
    far = np.argmax(shape)
    assert len(v) > 0 and (v[:, far] > 1.2 * (257 / (max(shape) - 1) - 0.5)).any()      # vertices beyond sample 256
    assert np.array_equal(f, ef)                                   # same cells, same order, same indices
    assert ev.dtype == v.dtype and v.tobytes() == ev.tobytes()     # ... and the same vertex bits
    assert mesh_emu.closed_and_oriented(len(v), f) and len(v) == len(mesh_emu.crossed_edges(grid, 0.05))


def _sphere_mesh(n):
    """The mesh of RADIUS - |x| on n^3 samples of the unit box (box_size 1: x = index / (n - 1) - 0.5), field made on the device."""
    c = torch.arange(n, dtype=torch.float64, device=DEV) / (n - 1) - 0.5
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    grid = (RADIUS - torch.sqrt(x * x + y * y + z * z)).float()
    return _run(grid, 0.0, 1.0)


def _volume_bound(n):
    """Every vertex lies on a crossed edge and every triangle inside a crossed cell, so the mesh stays within one cell diagonal
    d = sqrt(3) h, h = 1 / (n - 1), of the sphere: its volume differs from the ball's by at most that of the shell of
    thickness d on either side, 4/3 pi ((r + d)^3 - r^3)."""
    d = np.sqrt(3.0) / (n - 1)
    return 4.0 / 3.0 * np.pi * ((RADIUS + d) ** 3 - RADIUS ** 3)


def test_sphere_on_257_samples_is_watertight_with_the_volume_of_the_ball():
    ball = 4.0 / 3.0 * np.pi * RADIUS ** 3
    errors = {}
    for n in (129, 257):
        v, f = _sphere_mesh(n)
        assert len(v) > 0 and mesh_emu.closed_and_oriented(len(v), f), n          # watertight, consistently oriented
        assert mesh_emu.euler_characteristic(len(v), f) == 2, n
        errors[n] = abs(abs(mesh_emu.signed_volume(v, f)) - ball)
        print(n, "samples:", len(v), "vertices", len(f), "faces, volume error", errors[n], "bound", _volume_bound(n))
        assert errors[n] <= _volume_bound(n), n
    assert errors[257] <= _volume_bound(129)                      # the bound the 129^3 mesh meets
