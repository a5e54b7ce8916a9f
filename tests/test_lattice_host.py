"""CPU tests of the lattice recognition (giga_amd.convonet._detect_lattice / register_lattice): which query tensors are promoted
to the lattice decoder without the caller asking, and which are not.  _detect_lattice runs on CPU tensors as it is (only
_lattice_of asks for a device tensor), so nothing here needs a GPU.  Also the proof, from the restated launch formula, that the cases
of tests/test_gpu_lattice_shapes.py reach every dispatch branch of the lattice decoders."""
import os
import sys

import pytest
import torch

from giga_amd import convonet

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_lattice_shapes as G  # noqa: E402  (its case tables and the restated launch formula; nothing in it runs here)
from lattice_lins import FAMILIES, grid_points, lin_family  # noqa: E402


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("R", [8, 9, 40, 64])
def test_product_grids_are_detected(R, fam):
    """Sorted, clamped-at-both-ends and unsorted / duplicated coordinate vectors alike: the grid is recognised, with the right
    R and `lin` bit-equal to the vector it was built from."""
    lin = lin_family(fam, R)
    before = convonet.LATTICE_STATS["detected"]
    res = convonet._detect_lattice(grid_points(lin))
    assert res is not None
    got, r = res
    assert r == R and got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (R,)
    assert torch.equal(_bits(got), _bits(lin))
    assert convonet.LATTICE_STATS["detected"] == before + 1


def test_cube_root_is_exact_for_every_admitted_size():
    """R = round(n ** (1/3)) must give back R for every cube from 8^3 to 64^3, and every one of those grids is detected."""
    for R in range(8, 65):
        n = R ** 3
        assert round(n ** (1.0 / 3.0)) == R, R
        lin = lin_family("a", R)
        res = convonet._detect_lattice(grid_points(lin))
        assert res is not None and res[1] == R and torch.equal(_bits(res[0]), _bits(lin)), R


@pytest.mark.parametrize("R", [7, 65])
def test_sizes_outside_8_to_64_are_declined(R):
    assert convonet._detect_lattice(grid_points(lin_family("a", R))) is None


@pytest.mark.parametrize("n", [511, 513, 63999, 64001])
def test_point_counts_that_are_no_cube_are_declined(n):
    R = round(n ** (1.0 / 3.0))
    full = grid_points(lin_family("a", R))[0]
    p = full[:n] if n < R ** 3 else torch.cat([full, full[:n - R ** 3]])
    assert tuple(p.shape) == (n, 3)
    assert convonet._detect_lattice(p.unsqueeze(0).contiguous()) is None


@pytest.mark.parametrize("fam", FAMILIES)
def test_near_lattices_are_declined(fam):
    R = 9
    lin = lin_family(fam, R)
    p = grid_points(lin)
    assert convonet._detect_lattice(p) is not None                            # the control: everything below changes ONE property
    assert convonet._detect_lattice(p.double()) is None                       # float64
    wide = torch.zeros(1, 2 * R ** 3, 3)
    wide[:, ::2] = p
    view = wide[:, ::2]
    assert torch.equal(view, p) and not view.is_contiguous()
    assert convonet._detect_lattice(view) is None                             # a non-contiguous view of the very same points
    assert convonet._detect_lattice(p.expand(2, -1, -1).contiguous()) is None  # (2, R^3, 3)
    for idx, axis, toward in ((0, 0, 1.0), (R ** 3 // 2 + 1, 1, -1.0), (R ** 3 - 1, 2, 1.0)):
        bent = p.clone()
        bent[0, idx, axis] = torch.nextafter(bent[0, idx, axis], torch.tensor(toward))
        assert not torch.equal(bent, p)
        assert convonet._detect_lattice(bent) is None, (idx, axis)            # one coordinate, one ulp
    x_fastest = p.view(R, R, R, 3).permute(2, 1, 0, 3).reshape(1, R ** 3, 3).contiguous()
    assert convonet._detect_lattice(x_fastest) is None                        # the same grid flattened with x fastest


def test_registration_is_tied_to_the_tensor_version():
    """register_lattice stores the entry under the tensor's version counter; an in-place edit bumps the counter, so _lattice_of
    must not trust the entry any more (on the device it then re-detects: tests/test_gpu_parity.py, R = 40)."""
    lin = lin_family("c", 9)
    p = grid_points(lin)
    assert convonet.register_lattice(p, lin) is p
    ent = convonet._LATTICES[id(p)]
    assert ent[0]() is p and ent[1] == p._version and ent[2][1] == 9 and torch.equal(_bits(ent[2][0]), _bits(lin))
    p[0, 5, 1] += 0.25
    assert convonet._LATTICES[id(p)][1] != p._version
    assert convonet._lattice_of(p) is None                                     # (a CPU tensor never takes the lattice path)
    del p


def test_dispatch_cases_cover_every_branch():
    """The coverage proof of tests/test_gpu_lattice_shapes.py, which needs no device.  From launch_decoder's formula alone
    (G.dispatch restates it): the decoder_lat_kernel cases take lat_parts 1 and 2 at every R and 5 at R = 40, each
    of the three `slots` branches, the XCD remap on and off, and plain fp16 (two line buffers) at every R; the other cases never
    reach decoder_lat_kernel and run every LATTICE = true kernel in both tile counts."""
    parts, branches, xcd, dbuf = {}, set(), set(), set()
    for R, B, mask, _, _, _, precs in G.LAT_CASES:
        for prec in precs:
            for nh in G.MASKS[mask][1]:
                d = G.dispatch(G.PREC_CODE[prec], B, R, nh)
                assert d["kernel"] == "lat", (R, B, mask, prec)
                parts.setdefault(R, set()).add(d["parts"])
                branches.add(d["branch"])
                xcd.add(d["xcd"])
                if G.PREC_CODE[prec] == 1:
                    dbuf.add(R)
    assert parts == {8: {1, 2}, 16: {1, 2}, 24: {1, 2}, 32: {1, 2}, 40: {1, 2, 5}}, parts
    assert branches == {"nslab", "cap", "cap8"} and xcd == {True, False} and dbuf == {8, 16, 24, 32, 40}
    seen = set()
    for R, B, mask, _, _, _, precs in G.GEN_CASES:
        for prec in precs:
            for nh in G.MASKS[mask][1]:
                d = G.dispatch(G.PREC_CODE[prec], B, R, nh)
                assert d["kernel"] != "lat", (R, B, mask, prec)
                seen.add((d["kernel"], d["T"], d.get("split")))
    assert seen == {("f32", 1, True), ("f32", 1, False), ("f32", 2, None), ("f16s", 1, None), ("f16s", 2, None), ("f16", 2, None)}, seen
    assert {c[0] for c in G.GEN_CASES} == {1, 2, 7, 9, 17, 33, 41, 48, 63, 64}
    assert G.dispatch(1, 2, 48, 3)["kernel"] == "f16" and G.dispatch(1, 2, 48, 1)["kernel"] == "f16s"
    # the batch-versus-single-scene check of the shared-feature kernel: one scene of 64^3 points is already past its threshold
    assert G.dispatch(1, 2, 64, 4)["kernel"] == "f16" and G.dispatch(1, 1, 64, 4)["kernel"] == "f16"
