"""Coordinate vectors `lin` of the product grids the lattice tests run (tests/test_lattice_host.py on the CPU,
tests/test_gpu_lattice_shapes.py on the device), and the grid meshgrid(lin, lin, lin, 'ij') itself.  Test infrastructure only.

a  the planner recipe (detection_implicit.py:28-31): linspace(-0.5, 0.5 - 1/R, R);
b  the mesh recipe (Generator3D._mesh_points with the default padding): (1 + 0.1) * linspace(-0.5, 0.5, R) in fp32 -- both ends lie
   outside the cube, so both coordinate clamps are hit;
c  an unsorted vector drawn with a fixed seed from [-0.6, 0.6] that holds the exact values -0.5, 0.5 and 0.0 and one duplicated
   entry, at seeded positions (needs R >= 5)."""
import numpy as np
import torch

FAMILIES = ("a", "b", "c")


def lin_family(fam, R):
    """(R,) float32 CPU tensor."""
    if fam == "a":
        return torch.linspace(-0.5, 0.5 - 1.0 / R, R)
    if fam == "b":
        return ((1 + 0.1) * torch.linspace(-0.5, 0.5, R)).float()
    if fam == "c":
        if R < 5:
            raise ValueError("family c needs five entries: -0.5, 0.5, 0.0 and a duplicated pair")
        rng = np.random.default_rng(1000 + R)
        v = rng.uniform(-0.6, 0.6, R).astype(np.float32)
        at = rng.permutation(R)[:5]
        v[at[0]], v[at[1]], v[at[2]] = -0.5, 0.5, 0.0
        v[at[4]] = v[at[3]]
        return torch.from_numpy(v)
    raise ValueError(fam)


def grid_points(lin):
    """(1, R^3, 3) float32: meshgrid(lin, lin, lin, indexing='ij') flattened with z fastest."""
    x, y, z = torch.meshgrid(lin, lin, lin, indexing="ij")
    return torch.stack((x, y, z), dim=-1).float().reshape(1, lin.numel() ** 3, 3).contiguous()
