"""CPU tests of the encoder forward's launch policy (csrc/giga_enc_plan.h) through giga_encoder_plan / convonet.encoder_plan: host only,
the built library and no device.  launch_encoder launches what this plan says (tests/test_gpu_encoder_plan.py holds it to that on the
device), so each threshold of the policy is pinned here from both sides, with the figures of the code as it stands, and both
environment knobs in every form their parser distinguishes.  An image count is 3 B, so the steps of the group count (8 | 9, 16 | 17,
24 | 25 images) are pinned at the nearest scene counts; tools/enc_plan_check.cpp holds mega_groups itself to those image counts."""
import ctypes
import json
import os

import pytest

from giga_amd import _capi
from giga_amd.convonet import ENCODER_PLAN_WORDS, encoder_plan

KNOBS = ("GIGA_WINOGRAD", "GIGA_C32_FUSE")
PRECISIONS = ("fp32", "fp16", "fp16x3", "bf16")
P, C32, FUSED, WINO = _capi.PATH_PERSISTENT, _capi.PATH_CONV32, _capi.PATH_FUSED_PAIRS, _capi.PATH_WINOGRAD
CONV3 = (0, 1, 2, 3, 4, 5, 7, 8, 10, 11)     # the 3x3 layers of giga_layout.h::kConv; 6 and 9 are the ConvTransposes, 12 is the 1x1


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _raw(B, word, cus=256, stage=-1):
    w = (ctypes.c_int32 * ENCODER_PLAN_WORDS)()
    return _capi.lib().giga_encoder_plan(B, word, cus, stage, w), list(w)


def test_arguments():
    """The codes of giga_encoder_forward_probe for the same arguments; no scenes: nothing is launched, all words zero."""
    assert _capi.lib().giga_encoder_plan(1, 0, 256, -1, None) == -1
    assert _raw(-1, 0)[0] == -1
    assert _raw(_capi.MAX_SCENES + 1, 0)[0] == -7 and _raw(_capi.MAX_SCENES, 0)[0] == 0
    for word in (-1, 4, 5, 15, 4 | _capi.FOLD_FINAL, 4096):
        assert _raw(1, word)[0] == -5, word
    for prec in (1, 2):
        assert _raw(1, prec | _capi.CONVIN_MASK)[0] == -5
    for prec in (0, 3):
        assert _raw(1, prec | _capi.CONVIN_MASK)[0] == 0
    for prec in range(4):
        rc, words = _raw(0, prec)
        assert rc == 0 and not any(words)
    d = encoder_plan(0, "fp16")
    assert d["form"] is None and d["launches"] == 0 and d["layers"] == ["none"] * 13
    assert encoder_plan(3, "fp16x3") == encoder_plan(3, 2)                                   # a name or the encoder's code
    assert _raw(5, 1, cus=0)[1] == _raw(5, 1, cus=256)[1] == _raw(5, 1, cus=-3)[1]           # cus <= 0: assume 256


def test_conv_in_parts_and_grid():
    for prec in PRECISIONS:
        below, at = encoder_plan(31, prec), encoder_plan(32, prec)
        assert (below["nxp"], below["ci_sxw"], below["ci_grid_x"], below["ci_grid_y"], below["ci_grid_z"]) == (5, 1, 5, 8, 31)
        assert (at["nxp"], at["ci_sxw"], at["ci_grid_x"], at["ci_grid_y"], at["ci_grid_z"]) == (1, 5, 8 * 32, 1, 1)
        for d in (below, at):
            assert (d["ci_nw"], d["ci_block"], d["fin_block"]) == (8, 512, 256)
        assert below["fin_grid"] == 31 * 40 * 40 * 32 // 4 // 256 and at["fin_grid"] == 32 * 40 * 40 * 32 // 4 // 256
    assert encoder_plan(1, "fp32")["fin_grid"] == 50 and encoder_plan(3072, "fp32")["ci_grid_x"] == 8 * 3072


def test_conv_in_instantiation_per_mode():
    def inst(prec, **kw):
        d = encoder_plan(2, prec, **kw)
        return d["ci_f16"], d["ci_lo"], d["ci_mask"]
    assert inst("fp32") == (False, False, False)
    assert inst("fp32", convin_mask=True) == (False, False, True)
    assert inst("fp16") == (True, False, False)
    assert inst("fp16x3") == (True, True, False)
    assert inst("bf16") == (True, True, False)
    assert inst("bf16", convin_mask=True) == (True, False, True)


def test_persistent_by_default():
    for prec in ("fp16", "fp16x3"):
        for B in (1, 2, 7, 8, 33, 3072):
            assert encoder_plan(B, prec)["persistent"], (prec, B)
    for prec in ("fp32", "bf16"):
        assert not encoder_plan(7, prec)["persistent"] and encoder_plan(8, prec)["persistent"]          # 21 | 24 images
        assert encoder_plan(7, prec, persistent=True)["persistent"]
        assert not encoder_plan(8, prec, persistent="layers")["persistent"]
    assert not encoder_plan(1, "fp16", persistent="layers")["persistent"]
    # GIGA_LAYERWISE_UNET beats GIGA_PERSIST_UNET
    rc, words = _raw(8, 1 | _capi.PERSIST_UNET | _capi.LAYERWISE_UNET)
    assert rc == 0 and words == _raw(8, 1 | _capi.LAYERWISE_UNET)[1] and words != _raw(8, 1 | _capi.PERSIST_UNET)[1]
    for cus in (64, 255, 257, 304):                            # not a whole MI355X: one launch per layer, whatever is asked for
        assert not encoder_plan(8, "fp16", cus=cus)["persistent"] and not encoder_plan(8, "fp32", cus=cus, persistent=True)["persistent"]
    for stage in range(-1, 17):
        assert encoder_plan(8, "fp16", probe_stage=stage)["persistent"] == (not 2 <= stage <= 14), stage
    # no room for a fifth persistent launch on the device: the same call, one launch per layer
    busy = encoder_plan(8, "fp16", slot_free=False)
    assert not busy["persistent"] and busy == encoder_plan(8, "fp16", persistent="layers")
    assert encoder_plan(7, "fp32", slot_free=False) == encoder_plan(7, "fp32")


def test_conv32_choice():
    for prec in ("fp16", "fp16x3", "bf16"):
        assert encoder_plan(16, prec)["conv32"] and not encoder_plan(17, prec)["conv32"]                 # 48 | 51 images
    for prec in ("fp16", "fp16x3"):
        assert encoder_plan(17, prec, unet_kernel="conv32")["conv32"] and not encoder_plan(16, prec, unet_kernel="conv16")["conv32"]
    for prec in (1, 2, 3):                                     # the C flags, precision 3 too; GIGA_CONV32_UNET beats GIGA_CONV16_UNET
        both = _raw(17, prec | _capi.CONV32_UNET | _capi.CONV16_UNET)[1]
        assert both == _raw(17, prec | _capi.CONV32_UNET)[1] != _raw(17, prec | _capi.CONV16_UNET)[1]
        assert _raw(16, prec | _capi.CONV16_UNET)[1] != _raw(16, prec)[1] == _raw(16, prec | _capi.CONV32_UNET)[1]
    for B in (1, 16, 17):                                      # precision 0 has conv16 only
        for flag in (_capi.CONV32_UNET, _capi.CONV16_UNET):
            assert _raw(B, 0 | flag)[1] == _raw(B, 0)[1]
        assert not encoder_plan(B, "fp32")["conv32"]
    d = encoder_plan(16, "fp16")
    assert d["form"] == "persistent_conv32" and d["layers"] == ["conv32"] * 13 and d["block"] == 512
    assert encoder_plan(16, "fp16", persistent="layers")["form"] == "layers_conv32"
    d = encoder_plan(17, "fp16")
    assert d["form"] == "persistent_conv16" and d["layers"] == ["conv16"] * 13 and d["block"] == 768


def test_fused_pairs(monkeypatch):
    """Only with the persistent conv32 launch; up to two images per group."""
    assert encoder_plan(21, "fp16", unet_kernel="conv32")["fused"]                      # 63 images over 32 groups
    assert not encoder_plan(22, "fp16", unet_kernel="conv32")["fused"]                  # 66
    assert encoder_plan(1, "fp16")["fused"] and encoder_plan(16, "fp16x3")["fused"]
    assert encoder_plan(16, "fp16")["path"] == P | C32 | FUSED and encoder_plan(22, "fp16", unet_kernel="conv32")["path"] == P | C32
    for kw in (dict(persistent="layers"), dict(unet_kernel="conv16"), dict(cus=64), dict(slot_free=False), dict(probe_stage=2)):
        assert not encoder_plan(4, "fp16", **kw)["fused"], kw
    assert not encoder_plan(8, "fp32")["fused"]
    monkeypatch.setenv("GIGA_C32_FUSE", "0")
    assert not encoder_plan(1, "fp16")["fused"] and encoder_plan(1, "fp16")["path"] == P | C32
    monkeypatch.setenv("GIGA_C32_FUSE", "1")
    assert encoder_plan(22, "fp16", unet_kernel="conv32")["fused"] and encoder_plan(3072, "fp16x3", unet_kernel="conv32")["fused"]
    assert not encoder_plan(22, "fp16")["fused"] and not encoder_plan(1, "fp16", persistent="layers")["fused"]


def test_groups_and_grid():
    for B, groups in ((1, 8), (2, 8), (3, 16), (5, 16), (6, 24), (8, 24), (9, 32), (32, 32), (3072, 32)):     # 6 | 9, 15 | 18, 24 | 27 images
        d = encoder_plan(B, "fp16")
        assert d["nimg"] == 3 * B and d["groups"] == groups and d["grid"] == 8 * groups <= 256, (B, d)
        assert encoder_plan(B, "fp16", persistent="layers")["grid"] == 0
    assert encoder_plan(8, "fp32")["block"] == 512 and encoder_plan(8, "fp32", unet_kernel="direct")["block"] == 768


def test_wino_mask(monkeypatch):
    for B in (1, 8):
        d = encoder_plan(B, "fp32")
        assert d["wino_mask"] == 0xFFF and bool(d["path"] & WINO)
        for prec in ("fp16", "fp16x3", "bf16"):
            d = encoder_plan(B, prec)
            assert d["wino_mask"] == 0 and not d["path"] & WINO
    d = encoder_plan(8, "fp32", unet_kernel="direct")          # GIGA_DIRECT_CONV
    assert d["wino_mask"] == 0 and d["path"] == P and d["form"] == "persistent_conv16" and d["layers"] == ["conv16"] * 13
    assert encoder_plan(8, "fp32")["form"] == "persistent_winograd" and encoder_plan(8, "fp32")["path"] == P | WINO
    for text, mask in (("0x1FFF", 0xFFF), ("0xFFFFFFFF", 0xFFF), ("0", 0), ("3", 3), ("0x3", 3), ("0x40", 0x40), ("010", 8), ("x", 0)):
        monkeypatch.setenv("GIGA_WINOGRAD", text)
        for B in (1, 8):
            d = encoder_plan(B, "fp32")
            assert d["wino_mask"] == mask and bool(d["path"] & WINO) == (mask != 0), (text, d)
        assert encoder_plan(8, "fp32")["form"] == ("persistent_winograd" if mask else "persistent_conv16")
        assert encoder_plan(1, "fp16")["wino_mask"] == 0 and encoder_plan(8, "fp32", unet_kernel="direct")["wino_mask"] == 0


def test_layer_families(monkeypatch):
    want = ["winograd" if l in CONV3 else "up_gemm" if l in (6, 9) else "conv16" for l in range(13)]
    for B in (1, 8):
        assert encoder_plan(B, "fp32")["layers"] == want
    monkeypatch.setenv("GIGA_WINOGRAD", "0x45")                # layers 0, 2 and 6
    assert encoder_plan(1, "fp32")["layers"] == ["winograd", "conv16", "winograd"] + ["conv16"] * 3 + ["up_gemm"] + ["conv16"] * 6
    monkeypatch.delenv("GIGA_WINOGRAD")
    for prec in PRECISIONS:
        for B in (1, 17):
            full, fold = encoder_plan(B, prec), encoder_plan(B, prec, fold_final=True)
            assert full["nlayers"] == 13 and fold["nlayers"] == 12
            assert fold["layers"] == full["layers"][:12] + ["none"] and "none" not in full["layers"]


def test_launch_counts():
    for prec in PRECISIONS:
        for B in (1, 8, 17):
            for fold in (False, True):
                for form in (False, True, "layers"):
                    d = encoder_plan(B, prec, fold_final=fold, persistent=form)
                    assert d["launches"] == (3 if d["persistent"] else 2 + d["nlayers"]), d
    assert encoder_plan(1, "fp32")["launches"] == 15 and encoder_plan(1, "fp32", fold_final=True)["launches"] == 14
    assert encoder_plan(1, "fp16")["launches"] == 3


def test_workspace_is_the_parents():
    """giga_encoder_workspace_bytes and the 17 offsets of giga_encoder_workspace_layout against the figures recorded from the build
    before the carve moved into giga_enc_plan.h (tests/golden/encoder_workspace.json: "B,precision" -> [bytes, 17 offsets])."""
    L = _capi.lib()
    with open(os.path.join(os.path.dirname(__file__), "golden", "encoder_workspace.json")) as f:
        rows = json.load(f)
    assert sorted(rows) == sorted(f"{B},{p}" for B in (1, 7, 31, 32, 33, 3072) for p in range(4))
    off = (ctypes.c_size_t * 17)()
    for key, row in rows.items():
        B, prec = map(int, key.split(","))
        assert L.giga_encoder_workspace_layout(B, prec, off) == 0
        assert [L.giga_encoder_workspace_bytes(B, prec)] + list(off) == row, key
        assert L.giga_encoder_workspace_bytes(B, prec | _capi.FOLD_FINAL | _capi.CONV16_UNET | _capi.CONVIN_MASK) == row[0]
    assert rows["1,0"][0] == 7951360 and rows["1,1"][0] == 5071360 and rows["1,0"][16:] == [5760000, 5760000]      # (XZ is YZ)
    assert L.giga_encoder_workspace_bytes(0, 0) == 0 and L.giga_encoder_workspace_layout(0, 0, off) == -1
    assert L.giga_encoder_workspace_layout(1, 4, off) == -5


def test_knobs_are_read_on_every_call(monkeypatch):
    a = encoder_plan(1, "fp32")
    monkeypatch.setenv("GIGA_WINOGRAD", "0")
    b = encoder_plan(1, "fp32")
    monkeypatch.delenv("GIGA_WINOGRAD")
    assert a["wino_mask"] == 0xFFF and b["wino_mask"] == 0 and encoder_plan(1, "fp32") == a
    a = encoder_plan(1, "fp16")
    monkeypatch.setenv("GIGA_C32_FUSE", "0")
    b = encoder_plan(1, "fp16")
    monkeypatch.delenv("GIGA_C32_FUSE")
    assert a["fused"] and not b["fused"] and encoder_plan(1, "fp16") == a
