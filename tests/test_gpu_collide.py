"""GPU tests of giga_mesh_collide (csrc/giga_collide.hip) and giga_amd.collision.  The bytes are compared with the numpy restatement
of tests/collide_emu.py, which tests/test_collide_host.py holds to exact arithmetic on these very inputs, and with decisions that
are known analytically."""
import functools

import numpy as np
import pytest
import torch

import collide_emu as cemu
from giga_amd import _capi, collision

pytestmark = pytest.mark.gpu
F32 = np.float32
TILE = 256                                    # CO_BLOCK: triangles of the larger body per workgroup, and per step of the walk


def dev():
    return torch.device("cuda:0")


def collide(meshes, pairs, containment=False):
    return collision.mesh_collide(meshes, pairs, containment=containment, device=dev()).cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference():
    """the bodies, all ordered pairs and the restatement's decisions: computed once, shared, never changed"""
    bodies = cemu.gpu_bodies(0)
    assert [len(f) for _, f in bodies] == [12] * 8 + [80] * 4 + [320, 257, 1, 0]
    pairs = np.array([(a, b) for a in range(len(bodies)) for b in range(len(bodies)) if a != b], np.int64)
    want = cemu.mesh_collide(bodies, pairs)
    want.setflags(write=False)
    pairs.setflags(write=False)
    return bodies, pairs, want


def test_hit_equals_the_restatement_in_both_orders_permuted_and_twice():
    bodies, pairs, want = reference()
    assert 20 < want.sum() < len(want) - 20                                # both answers occur
    for big in (12, 13):                                                   # the bodies that cross the tile take part in hits and misses
        mine = want[(pairs == big).any(axis=1)]
        assert mine.any() and not mine.all()
    got = collide(bodies, pairs)
    assert got.dtype == bool and np.array_equal(got, want)
    swapped = collide(bodies, pairs[:, ::-1])
    assert np.array_equal(swapped, want)                                   # hit(a, b) == hit(b, a)
    order = np.random.default_rng(5).permutation(len(pairs))
    assert np.array_equal(collide(bodies, pairs[order]), want[order])      # a byte does not depend on the other pairs
    assert np.array_equal(collide(bodies, pairs), got)                     # equal input, equal bytes
    one = np.array([pairs[3]])
    assert np.array_equal(collide(bodies, one), want[3:4])
    # device tensors in, and objects with .vertices / .faces
    from giga_amd.mesh import Mesh
    as_tensors = [(torch.from_numpy(v).to(dev()), torch.from_numpy(f).to(dev())) for v, f in bodies]
    assert np.array_equal(collide(as_tensors, pairs[:40]), want[:40])
    assert np.array_equal(collide([Mesh(v, f) for v, f in bodies], pairs[:40]), want[:40])


def test_unusable_triangles_intersect_nothing():
    A = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32), np.array([[0, 1, 2]], np.int32))
    B = np.array([[0.2, 0.2, -0.5], [0.2, 0.2, 0.5], [0.9, 0.9, 0.5]], F32)
    bad = B.copy()
    bad[1, 2] = np.nan
    inf = B.copy()
    inf[2, 0] = np.inf
    f = np.array([[0, 1, 2]], np.int32)
    bodies = [A, (B, f), (bad, f), (inf, f), (B, np.array([[0, 1, 3]], np.int32)), (B, np.array([[0, -1, 2]], np.int32)),
              (np.concatenate((bad, B)), np.array([[0, 1, 2], [3, 4, 5]], np.int32)), (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32))]
    pairs = [(0, k) for k in range(1, len(bodies))]
    want = [True, False, False, False, False, True, False]
    assert cemu.mesh_collide(bodies, pairs).tolist() == want
    assert collide(bodies, pairs).tolist() == want
    assert collide(bodies, pairs, containment=True).tolist() == want


def test_analytic_boxes():
    base = cemu.box_mesh((0, 0, 0), (1, 1, 1))
    partial = cemu.box_mesh((0.5, 0.4, 0.3), (1.5, 1.4, 1.3))
    apart = cemu.box_mesh((2, 0, 0), (3, 1, 1))
    nested = cemu.box_mesh((0.25, 0.3125, 0.25), (0.75, 0.5, 0.625))     # (its corners lie off the diagonals of base's faces)
    flush = cemu.box_mesh((1, 0, 0), (2, 1, 1))
    bodies = [base, partial, apart, nested, flush]
    pairs = [(0, 1), (0, 2), (0, 3), (0, 4), (3, 0)]
    got = collide(bodies, pairs)
    assert got[:3].tolist() == [True, False, False]
    assert got[3] == cemu.mesh_collide(bodies, [(0, 4)])[0]
    assert not got[4]
    with_containment = collide(bodies, pairs, containment=True)
    assert with_containment[[0, 1, 2, 4]].tolist() == [True, False, True, True]
    # an object inside a hollow open mesh (a box without its lid) is no collision
    v, f = base
    open_box = (v, f[~(v[f][:, :, 2] == 1).all(axis=1)])
    assert len(open_box[1]) == 10
    assert collide([open_box, nested], [(0, 1), (1, 0)], containment=True).tolist() == [False, False]


def _inscribed(mesh, centre):
    v, f = mesh
    a, b, c = (v[f[:, k]].astype(np.float64) - centre for k in range(3))
    n = np.cross(b - a, c - a)
    return float((np.abs((n * a).sum(axis=1)) / np.sqrt((n * n).sum(axis=1))).min())


def test_analytic_spheres():
    r1, r2 = 0.05, 0.04
    one = cemu.icosphere((0, 0, 0), r1, 2)
    rin2 = _inscribed(cemu.icosphere((0, 0, 0), r2, 2), 0)
    rin = _inscribed(one, 0) + rin2
    assert 0.9 * (r1 + r2) < rin < r1 + r2
    direction = np.array([0.48, -0.6, 0.64])                               # a unit vector
    distances = [1.001 * (r1 + r2), 1.2 * (r1 + r2), 0.999 * rin, 0.06, 0.02, 0.013]
    want = [False, False, True, True, True, True]
    # below rin the solids overlap; above r1 - rin2 (a little more than |r1 - r2|: these are polyhedra) the smaller one's
    # inscribed ball reaches outside the larger one's circumscribed ball, so neither solid holds the other: the surfaces meet
    assert all(max(abs(r1 - r2), r1 - rin2) < d < rin for d, w in zip(distances, want) if w)
    bodies = [one] + [cemu.icosphere(direction * d, r2, 2) for d in distances]
    assert collide(bodies, [(0, k + 1) for k in range(len(distances))]).tolist() == want


def test_full_walk_without_an_early_stop():
    """Concentric icospheres of subdivision 3: the boxes are nested, so all 1280 triangles of the inner sphere and the 1004 of the
    outer one that reach into the inner box survive the box test; none of the 1.3 M pairs intersects, so every workgroup walks
    the whole other body and its list overflows several times."""
    outer, inner = cemu.icosphere((0, 0, 0), 1.0, 3), cemu.icosphere((0, 0, 0), 0.9, 3)
    assert len(outer[1]) == 1280 == 5 * TILE and _inscribed(outer, 0) > 0.9
    assert [len(t) for t in cemu.culled(outer, inner)] == [1004, 1280]
    shifted = cemu.icosphere((0.3, 0, 0), 1.0, 3)
    got = collide([outer, inner, shifted], [(0, 1), (1, 0), (0, 2), (2, 0)])
    assert got.tolist() == [False, False, True, True]
    assert collide([outer, inner], [(0, 1)], containment=True).tolist() == [True]


def test_l_prism_with_a_box_in_its_notch():
    prism = cemu.l_prism()
    in_notch = cemu.box_mesh((0.05, 0.05, 0.01), (0.09, 0.09, 0.04))        # bounding boxes overlap, surfaces do not
    across = cemu.box_mesh((0.03, 0.05, 0.01), (0.09, 0.09, 0.04))
    assert collide([prism, in_notch, across], [(0, 1), (0, 2)]).tolist() == [False, True]
    assert collide([prism, in_notch], [(0, 1)], containment=True).tolist() == [False]


def test_cpu_tensors_and_bad_pairs_raise():
    v, f = cemu.box_mesh((0, 0, 0), (1, 1, 1))
    with pytest.raises(_capi.GigaHipError):
        collision.mesh_collide([(torch.from_numpy(v), torch.from_numpy(f))] * 2, [(0, 1)])
    with pytest.raises(ValueError):
        collision.mesh_collide([(v, f)] * 2, [(0, 0)], device=dev())
    with pytest.raises(ValueError):
        collision.mesh_collide([(v, f)] * 2, [(0, 2)], device=dev())
    assert collision.mesh_collide([(v, f)] * 2, np.zeros((0, 2), int), device=dev()).shape == (0,)
