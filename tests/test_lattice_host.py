"""CPU tests of the lattice recognition (giga_amd.convonet._detect_lattice / register_lattice): which query tensors are promoted
to the lattice decoder without the caller asking, and which are not.  _detect_lattice runs on CPU tensors as it is (only
_lattice_of asks for a device tensor), so nothing here needs a GPU.  Also the proof, from the library's own launch plan
(giga_decoder_plan: host only, it needs the built library and no device), that the cases of tests/test_gpu_lattice_shapes.py reach
every dispatch branch of the lattice decoders, and that the plan equals the hand-written table of those cases."""
import os
import sys

import pytest
import torch

from giga_amd import convonet

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_lattice_shapes as G  # noqa: E402  (its case tables and its `plan`; none of its tests runs here)
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


@pytest.fixture(autouse=True)
def _no_decoder_knobs(monkeypatch):
    for k in ("GIGA_DEC_LAT", "GIGA_DEC16_RESIDENT", "GIGA_DEC32_TILE", "GIGA_DEC32_POINT"):
        monkeypatch.delenv(k, raising=False)


def test_lat_table_equals_the_plan():
    """G.LAT_TABLE, written by hand, against the library's plan, field for field, for every launch of G.LAT_CASES in every
    precision the case runs: ntile (lat_parts divides it), lat_parts, nslab, slots and its branch, the XCD remap -- and the grid,
    the two line buffers of plain fp16 and the operand form, which follow from them."""
    rows = {(r[0], r[1], r[3]): r for r in G.LAT_TABLE}
    assert len(rows) == len(G.LAT_TABLE) == 23
    launches = set()
    for R, B, mask, _, _, _, precs in G.LAT_CASES:
        for nh in G.MASKS[mask][1]:
            launches.add((R, B, nh))
            _, _, tmask, _, ntile, parts, nslab, slots, branch, remap = rows[(R, B, nh)]
            assert tmask == mask and ntile == (R // 4) * (R // 8) and nslab == B * R * parts
            assert slots == {"nslab": nslab, "cap": 256 // nh, "cap8": 256 // (8 * nh) * 8}[branch]
            for prec in precs:
                code = G.PREC_CODE[prec]
                d = G.plan(code, B, R, nh)
                assert d["kernel"] == "lat", (R, B, nh, prec)
                assert ntile % d["lat_parts"] == 0
                assert (d["lat_parts"], B * R * d["lat_parts"], d["slots"], d["xcd_remap"]) == (parts, nslab, slots, remap), (R, B, nh, prec, d)
                assert (d["grid_x"], d["grid_y"], d["nbatch"], d["block"], d["NW"]) == (slots * nh, 1, slots, 1024, 16), d
                assert (d["split"], d["dbuf"]) == (code == 2, code == 1), d
    assert launches == set(rows)


def test_dispatch_cases_cover_every_branch():
    """The coverage proof of tests/test_gpu_lattice_shapes.py, which needs no device.  From the library's plan (G.plan; the branch
    of `slots` from G.LAT_TABLE, which test_lat_table_equals_the_plan holds to the plan): the decoder_lat_kernel cases take
    lat_parts 1 and 2 at every R and 5 at R = 40, each of the three `slots` branches, the XCD remap on and off, and plain fp16 (two
    line buffers) at every R; the other cases never reach decoder_lat_kernel and run every LATTICE = true kernel in both tile
    counts."""
    branch_of = {(r[0], r[1], r[3]): r[8] for r in G.LAT_TABLE}
    parts, branches, xcd, dbuf = {}, set(), set(), set()
    for R, B, mask, _, _, _, precs in G.LAT_CASES:
        for prec in precs:
            for nh in G.MASKS[mask][1]:
                d = G.plan(G.PREC_CODE[prec], B, R, nh)
                assert d["kernel"] == "lat", (R, B, mask, prec)
                parts.setdefault(R, set()).add(d["lat_parts"])
                branches.add(branch_of[(R, B, nh)])
                xcd.add(d["xcd_remap"])
                if d["dbuf"]:
                    assert G.PREC_CODE[prec] == 1
                    dbuf.add(R)
    assert parts == {8: {1, 2}, 16: {1, 2}, 24: {1, 2}, 32: {1, 2}, 40: {1, 2, 5}}, parts
    assert branches == {"nslab", "cap", "cap8"} and xcd == {True, False} and dbuf == {8, 16, 24, 32, 40}
    seen = set()
    for R, B, mask, _, _, _, precs in G.GEN_CASES:
        for prec in precs:
            for nh in G.MASKS[mask][1]:
                d = G.plan(G.PREC_CODE[prec], B, R, nh)
                assert d["kernel"] != "lat", (R, B, mask, prec)
                # fp32, one tile per wave: whether every head gets its own workgroups (blockIdx.y)
                per_head = (d["heads_per_wg"] == 1 and d["grid_y"] == nh) if (d["kernel"], d["T"]) == ("f32", 1) else None
                if per_head is False:
                    assert (d["heads_per_wg"], d["grid_y"]) == (nh, 1)
                seen.add((d["kernel"], d["T"], per_head))
    assert seen == {("f32", 1, True), ("f32", 1, False), ("f32", 2, None), ("f16s", 1, None), ("f16s", 2, None), ("f16", 2, None)}, seen
    assert {c[0] for c in G.GEN_CASES} == {1, 2, 7, 9, 17, 33, 41, 48, 63, 64}
    assert G.plan(1, 2, 48, 3)["kernel"] == "f16" and G.plan(1, 2, 48, 1)["kernel"] == "f16s"
    # the batch-versus-single-scene check of the shared-feature kernel: one scene of 64^3 points is already past its threshold
    assert G.plan(1, 2, 64, 4)["kernel"] == "f16" and G.plan(1, 1, 64, 4)["kernel"] == "f16"
