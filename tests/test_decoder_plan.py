"""CPU tests of the decoder's launch policy (csrc/giga_dec_plan.h) through giga_decoder_plan / convonet.decoder_plan: host only, the
built library and no device.  launch_decoder launches what this plan says (tests/test_gpu_decoder_plan.py holds it to that on the
device), so each threshold of the policy is pinned here from both sides, with the figures of the code as it stands, and each
environment knob in every form its parser distinguishes."""
import ctypes

import pytest

from giga_amd import _capi
from giga_amd.convonet import DECODER_PLAN_FIELDS, decoder_plan

KNOBS = ("GIGA_DEC_LAT", "GIGA_DEC16_RESIDENT", "GIGA_DEC32_TILE", "GIGA_DEC32_POINT")
F16, F16S, LAT = "decoder_f16_kernel", "decoder_f16s_kernel", "decoder_lat_kernel"
F32, TILE, POINT = "decoder_f32_kernel", "decoder_f32_tile_kernel", "decoder_f32_point_kernel"


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def kernel(B, N, R, nh, prec):
    return decoder_plan(B, N, R, nh, prec)["kernel"]


def _tiles(B, N):
    return (B * N + 31) // 32


def test_arguments():
    """The codes of giga_decoder_forward* for the same arguments; no points or no heads: nothing is launched, all words zero."""
    L = _capi.lib()
    w = (ctypes.c_int32 * len(DECODER_PLAN_FIELDS))()
    assert L.giga_decoder_plan(1, 100, 0, 3, 1, None) == -1
    for args in ((-1, 1, 0, 1, 0), (1, -1, 0, 1, 0), (1, 1, -1, 1, 0), (1, 1, 65, 1, 0), (1, 1, 0, 5, 0), (1, 1, 0, -1, 0)):
        assert L.giga_decoder_plan(*args, w) == -1, args
    for prec in (-1, 3, 4):
        assert L.giga_decoder_plan(1, 100, 0, 3, prec, w) == -5
    assert L.giga_decoder_plan(1, 100, 0, 3, 1 | _capi.FOLD_FINAL, w) == 0 and L.giga_decoder_plan(4, 0, 8, 3, 1 | _capi.PLANES_FP32, w) == 0
    for args in ((0, 100, 0, 3, 0), (3, 0, 0, 3, 1), (3, 100, 0, 0, 2)):
        d = decoder_plan(*args)
        assert d["kernel"] is None and not any(v for k, v in d.items() if k != "kernel"), d
    assert decoder_plan(2, 12345, 9, 3, 2) == decoder_plan(2, 0, 9, 3, 2)          # a lattice launch has N = R^3


def test_plain_f16_leaves_the_head_resident_kernel_at_its_tile_counts(monkeypatch):
    """tiles * nheads < 6000 (generic) / 16000 (lattice) runs the head-resident kernel, from there on the shared-feature one."""
    for nh, tiles in ((1, 6000), (2, 3000), (3, 2000), (4, 1500)):
        below = decoder_plan(1, 32 * (tiles - 1), 0, nh, 1)
        at = decoder_plan(1, 32 * tiles, 0, nh, 1)
        assert (below["kernel"], at["kernel"]) == (F16S, F16), (nh, below, at)
        assert (at["T"], at["NW"], at["block"], at["lds"]) == (2, 8, 512, 2 * 59 * 1024)
        assert at["nbatch"] == (tiles + 15) // 16 and at["grid_x"] == min(at["nbatch"], 256) and at["grid_y"] == 1
    assert decoder_plan(1, 32 * 5999, 0, 1, 1)["kernel"] == F16S                   # 5999 / 6000
    # the lattice: B R^3 points fix the reachable tile counts.  Every lattice the shared-feature kernel can see (GIGA_DEC_LAT=0 in
    # a second pass, so that R % 8 == 0 counts too) sits on the right side of 16000; 16000 itself is reached, and the largest count
    # below it is named
    best_below = 0
    for lat_off in (False, True):
        if lat_off:
            monkeypatch.setenv("GIGA_DEC_LAT", "0")
        for R in range(1, 65):
            for B in (1, 2, 3, 4, 5, 8, 13, 32):
                for nh in (1, 2, 3, 4):
                    d = decoder_plan(B, 0, R, nh, 1)
                    if d["kernel"] == LAT:
                        assert not lat_off
                        continue
                    load = _tiles(B, R ** 3) * nh
                    assert d["kernel"] == (F16S if load < 16000 else F16), (R, B, nh, load, d)
                    if load < 16000:
                        best_below = max(best_below, load)
                    elif d["kernel"] == F16:
                        assert (d["T"], d["NW"], d["lds"]) == (2, 12, 2 * 59 * 1024)
    assert decoder_plan(2, 0, 40, 4, 1)["kernel"] == F16 and _tiles(2, 40 ** 3) * 4 == 16000     # (GIGA_DEC_LAT=0 is still set)
    assert best_below == 15994, best_below       # the nearest ceil(B R^3 / 32) * nheads below 16000 over these B; 15999 is out of reach


@pytest.mark.parametrize("prec", [2, 1])
@pytest.mark.parametrize("nh", [1, 2, 3, 4])
def test_two_tiles_per_wave_of_the_head_resident_kernel(monkeypatch, prec, nh):
    """tiles >= 2 * cap * 8 * 2, cap = 256 / nheads: two tiles per wave; plain f16 then runs 8 waves instead of 12."""
    if prec == 1:
        monkeypatch.setenv("GIGA_DEC16_RESIDENT", "1")                              # (generic plain f16 leaves the kernel at 6000)
    bound = 2 * (256 // nh) * 8 * 2
    below, at = decoder_plan(1, 32 * (bound - 1), 0, nh, prec), decoder_plan(1, 32 * bound, 0, nh, prec)
    assert below["kernel"] == at["kernel"] == F16S
    assert (below["T"], below["NW"]) == (1, 8 if prec == 2 else 12) and (at["T"], at["NW"]) == (2, 8)
    for d in (below, at):
        assert d["split"] == (prec == 2) and d["lds"] == (111 if prec == 2 else 59) * 1024 and d["block"] == 64 * d["NW"]
        assert d["grid_x"] == d["slots"] * nh <= 256 and d["nbatch"] == d["slots"] and d["xcd_remap"] == (d["slots"] % 8 == 0)


def test_fp32_one_query_kernels():
    """N == 1: the point kernel up to 256 points, then the tile kernel while tiles * nheads <= 96, then the general kernel; never
    with more than one query per scene."""
    for nh in (1, 3, 4):
        d = decoder_plan(256, 1, 0, nh, 0)
        assert (d["kernel"], d["grid_x"], d["grid_y"], d["block"]) == (POINT, 256, nh, 256), d
        d = decoder_plan(257, 1, 0, nh, 0)
        assert (d["kernel"], d["grid_x"], d["grid_y"], d["block"]) == (TILE, 9, nh, 256), d
    assert kernel(3072, 1, 0, 1, 0) == TILE and kernel(3073, 1, 0, 1, 0) == F32                 # 96 / 97 tiles, one head
    assert kernel(1024, 1, 0, 3, 0) == TILE and kernel(1025, 1, 0, 3, 0) == F32                 # 32 / 33 tiles x 3 heads = 96 / 99
    assert kernel(768, 1, 0, 4, 0) == TILE and kernel(769, 1, 0, 4, 0) == F32                   # 24 / 25 tiles x 4 heads = 96 / 100
    assert kernel(1, 2, 0, 3, 0) == F32 and kernel(128, 2, 0, 1, 0) == F32                      # N == 2
    assert kernel(1, 0, 1, 3, 0) == F32                                                          # a one-point lattice is no such call


def test_fp32_general_kernel_tiles_and_head_split():
    """tiles >= 2048: two tiles per wave.  One tile per wave: every head gets its own workgroups (blockIdx.y) while
    grid * nheads <= 256."""
    for nh in (1, 3):
        below, at = decoder_plan(2047, 32, 0, nh, 0), decoder_plan(2048, 32, 0, nh, 0)
        assert (below["kernel"], below["T"], below["nbatch"], below["grid_x"]) == (F32, 1, 512, 256)
        assert (at["kernel"], at["T"], at["nbatch"], at["grid_x"], at["grid_y"], at["heads_per_wg"]) == (F32, 2, 256, 256, 1, nh)
    # grid = ceil(tiles / 4).  256 / 257 itself is out of reach (257 is prime and one head's grid ends at 256): the nearest products
    for nh, grid in ((2, 128), (3, 85), (4, 64)):
        assert grid * nh <= 256 < (grid + 1) * nh
        yes, no = decoder_plan(4 * grid, 32, 0, nh, 0), decoder_plan(4 * grid + 1, 32, 0, nh, 0)
        assert (yes["grid_x"], yes["grid_y"], yes["heads_per_wg"]) == (grid, nh, 1), yes
        assert (no["grid_x"], no["grid_y"], no["heads_per_wg"]) == (grid + 1, 1, nh), no
    one = decoder_plan(2047, 32, 0, 1, 0)
    assert (one["grid_x"], one["grid_y"], one["heads_per_wg"]) == (256, 1, 1)                   # 256 * 1 <= 256
    for d in (decoder_plan(3, 43, 0, 3, 0), decoder_plan(2048, 32, 0, 3, 0)):
        assert (d["block"], d["NW"], d["lds"], d["split"]) == (256, 4, 111 * 1024 + 4 * 32 * 96 * 4, False)


def test_lattice_kernel_sizes_and_scenes():
    """decoder_lat_kernel: f16-class, R % 8 == 0 and R <= 40; f16x3 always, plain f16 from 4 scenes up; never fp32."""
    for R in range(1, 65):
        ok = R % 8 == 0 and R <= 40
        assert (kernel(1, 0, R, 3, 2) == LAT) == ok, R
        assert (kernel(4, 0, R, 3, 1) == LAT) == ok, R
        assert kernel(4, 0, R, 3, 0) == F32, R
    assert kernel(1, 0, 40, 3, 2) == LAT and kernel(1, 0, 41, 3, 2) == F16S and kernel(1, 0, 48, 3, 2) == F16S
    for R, below4 in ((8, F16S), (40, F16)):                # (three scenes of 40^3 points x 3 heads: 18000 tiles)
        assert kernel(3, 0, R, 3, 1) == below4 and kernel(4, 0, R, 3, 1) == LAT
    d2, d1 = decoder_plan(4, 0, 40, 3, 2), decoder_plan(4, 0, 40, 3, 1)
    assert (d2["split"], d2["dbuf"], d2["lds"]) == (True, False, 65 * 1024 + 11 * 10 * 512 + 16)
    assert (d1["split"], d1["dbuf"], d1["lds"]) == (False, True, 33 * 1024 + 2 * 11 * 10 * 512 + 16)


@pytest.mark.parametrize("value,bound", [(None, 256), ("0", 0), ("1", 256), ("-3", 256), ("x", 256), ("300", 300), ("5000", 3072)])
def test_knob_dec32_point(monkeypatch, value, bound):
    if value is not None:
        monkeypatch.setenv("GIGA_DEC32_POINT", value)
    if bound:
        assert kernel(bound, 1, 0, 1, 0) == POINT and kernel(1, 1, 0, 4, 0) == POINT
    else:
        assert kernel(1, 1, 0, 1, 0) == TILE
    assert kernel(bound + 1, 1, 0, 1, 0) == (TILE if bound + 1 <= 3072 else F32)
    monkeypatch.setenv("GIGA_DEC32_TILE", "0")                                       # neither one-query kernel, whatever the bound
    assert kernel(1, 1, 0, 1, 0) == F32 and kernel(max(bound, 1), 1, 0, 3, 0) == F32


def test_knob_dec32_tile(monkeypatch):
    assert kernel(3, 1, 0, 3, 0) == POINT and kernel(300, 1, 0, 1, 0) == TILE
    monkeypatch.setenv("GIGA_DEC32_TILE", "0")
    d = decoder_plan(3, 1, 0, 3, 0)
    assert (d["kernel"], d["T"], d["grid_x"], d["grid_y"], d["heads_per_wg"]) == (F32, 1, 1, 3, 1) and kernel(300, 1, 0, 1, 0) == F32
    monkeypatch.setenv("GIGA_DEC32_TILE", "1")
    assert kernel(3, 1, 0, 3, 0) == POINT


def test_knob_dec_lat(monkeypatch):
    assert kernel(1, 0, 8, 3, 1) == F16S and kernel(1, 0, 8, 3, 2) == LAT and kernel(32, 0, 40, 3, 1) == LAT
    monkeypatch.setenv("GIGA_DEC_LAT", "1")
    assert kernel(1, 0, 8, 3, 1) == LAT and kernel(1, 0, 8, 3, 2) == LAT
    assert kernel(1, 0, 9, 3, 2) == F16S and kernel(1, 0, 48, 3, 1) == F16S and kernel(4, 0, 8, 3, 0) == F32    # only where it can run
    monkeypatch.setenv("GIGA_DEC_LAT", "0")
    assert kernel(1, 0, 8, 3, 2) == F16S and kernel(32, 0, 40, 3, 1) == F16 and kernel(4, 0, 8, 3, 1) == F16S


def test_knob_dec16_resident_is_read_per_call(monkeypatch):
    """Set AFTER a first call of the process has planned without it: the next call sees it (it was read once per process before
    the plan existed)."""
    assert kernel(1, 100, 0, 3, 1) == F16S and kernel(32, 2048, 0, 3, 1) == F16
    monkeypatch.setenv("GIGA_DEC16_RESIDENT", "0")
    d = decoder_plan(1, 100, 0, 3, 1)
    assert (d["kernel"], d["T"], d["NW"], d["grid_x"], d["nbatch"]) == (F16, 2, 8, 1, 1)
    assert kernel(1, 0, 9, 3, 1) == F16 and kernel(1, 100, 0, 3, 2) == F16S          # (f16x3 has no other kernel)
    monkeypatch.setenv("GIGA_DEC16_RESIDENT", "1")
    assert kernel(1, 100, 0, 3, 1) == F16S and kernel(32, 2048, 0, 3, 1) == F16S and kernel(2, 0, 64, 4, 1) == F16S
    monkeypatch.delenv("GIGA_DEC16_RESIDENT")
    assert kernel(32, 2048, 0, 3, 1) == F16
