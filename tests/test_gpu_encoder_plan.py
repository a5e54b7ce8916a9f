"""What is planned is what runs: for the smallest encoder calls that reach each branch of the launch policy, giga_launch_count rises by
the plan's `launches`, giga_encoder_last_path() is the plan's `path`, and the library's launch probe -- armed on conv_in, on the
persistent U-Net launch or on one layer's own launch -- names the kernel family and the integer and boolean template arguments of
convonet.encoder_plan (csrc/giga_enc_plan.h).  One encoder call per case; the plans are also written out by hand, so the test fails
when the policy moves as well as when launch and plan part."""
import torch

import pytest

from giga_amd import _capi, convonet, networks, synth, weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P, C32, FUSED, WINO = _capi.PATH_PERSISTENT, _capi.PATH_CONV32, _capi.PATH_FUSED_PAIRS, _capi.PATH_WINOGRAD
F32, F16 = ("float", "f"), ("_Float16", "DF16_")          # a type argument as the runtime may spell it: demangled, Itanium-mangled
# the MATH_* of giga_conv16.h and the C32_* modes of giga_conv32_geom.h
NATIVE, SPLIT, BF16 = 0, 1, 2
# (id, precision, B, keywords of encoder_plan, {knob: value}, the launch to probe: "conv_in", "unet" (the persistent launch) or a layer,
#  the kernel and template arguments expected there (None: the family's name alone), the plan's fields the case is about)
CASES = [
    ("fp32-1-layers-wino-layer0", "fp32", 1, {}, {}, 0, ("wino_kernel", [32, 0, 32, 40, 40, False, True]),
     dict(form="layers_conv16", launches=15, path=WINO, wino_mask=0xFFF)),
    ("fp32-1-layers-up-layer6", "fp32", 1, {}, {}, 6, ("up_kernel", [128, 64, 10, 10]), dict(form="layers_conv16", launches=15, path=WINO)),
    ("fp32-1-layers-final-layer12", "fp32", 1, {}, {}, 12, ("conv16_kernel", None), dict(form="layers_conv16", launches=15)),
    ("fp32-7-layers", "fp32", 7, {}, {}, 1, ("wino_kernel", [32, 0, 32, 40, 40, True, True]), dict(persistent=False, launches=15, path=WINO)),
    ("fp32-8-persistent-wino", "fp32", 8, {}, {}, "unet", ("unet_mega_kernel", [F32, NATIVE, True]),
     dict(form="persistent_winograd", launches=3, path=P | WINO, grid=192, block=512)),
    ("fp32-8-direct", "fp32", 8, dict(unet_kernel="direct"), {}, "unet", ("unet_mega_kernel", [F32, NATIVE, False]),
     dict(form="persistent_conv16", launches=3, path=P, grid=192, block=768, wino_mask=0)),
    ("fp32-1-knob-direct-layer0", "fp32", 1, {}, {"GIGA_WINOGRAD": "0"}, 0, ("conv16_kernel", None), dict(launches=15, path=0, wino_mask=0)),
    ("fp16-1-conv32-fused", "fp16", 1, {}, {}, "unet", ("unet32_mega_kernel", [NATIVE, True]),
     dict(form="persistent_conv32", launches=3, path=P | C32 | FUSED, grid=64, block=512)),
    ("fp16-16-conv32-fused", "fp16", 16, {}, {}, "unet", ("unet32_mega_kernel", [NATIVE, True]), dict(launches=3, path=P | C32 | FUSED, grid=256)),
    ("fp16-17-conv16", "fp16", 17, {}, {}, "unet", ("unet_mega_kernel", [F16, NATIVE, False]),
     dict(form="persistent_conv16", launches=3, path=P, grid=256, block=768)),
    ("fp16x3-1-conv16", "fp16x3", 1, dict(unet_kernel="conv16"), {}, "unet", ("unet_mega_kernel", [F32, SPLIT, False]), dict(launches=3, path=P)),
    ("fp16x3-1-conv32", "fp16x3", 1, {}, {}, "unet", ("unet32_mega_kernel", [SPLIT, True]), dict(launches=3, path=P | C32 | FUSED)),
    ("fp16-22-conv32-unfused", "fp16", 22, dict(unet_kernel="conv32"), {}, "unet", ("unet32_mega_kernel", [NATIVE, False]),
     dict(launches=3, path=P | C32, fused=False)),
    ("fp16-1-knob-unfused", "fp16", 1, {}, {"GIGA_C32_FUSE": "0"}, "unet", ("unet32_mega_kernel", [NATIVE, False]), dict(launches=3, path=P | C32)),
    ("fp16-1-layers", "fp16", 1, dict(persistent="layers"), {}, 0, ("conv32_kernel", None), dict(form="layers_conv32", launches=15, path=C32)),
    ("fp16-2-folded", "fp16", 2, dict(fold_final=True), {}, "unet", ("unet32_mega_kernel", [NATIVE, True]), dict(nlayers=12, launches=3)),
    ("fp16-1-layers-folded", "fp16", 1, dict(persistent="layers", fold_final=True), {}, 11, ("conv32_kernel", None), dict(nlayers=12, launches=14)),
    ("fp16-1-conv_in", "fp16", 1, {}, {}, "conv_in", ("convin_project_kernel", [F16, 1, True, 8, False, False]), dict(ci_grid_x=5, ci_grid_z=1)),
    ("fp16x3-1-conv_in", "fp16x3", 1, {}, {}, "conv_in", ("convin_project_kernel", [F32, 1, True, 8, True, False]), dict(nxp=5)),
    ("bf16-1-conv_in", "bf16", 1, {}, {}, "conv_in", ("convin_project_kernel", [F32, 1, True, 8, True, False]),
     dict(form="layers_conv32", launches=15, path=C32)),
    ("bf16-1-conv_in-mask", "bf16", 1, dict(convin_mask=True), {}, "conv_in", ("convin_project_kernel", [F32, 1, True, 8, False, True]),
     dict(ci_mask=True, launches=15)),
    ("fp32-1-conv_in-mask", "fp32", 1, dict(convin_mask=True), {}, "conv_in", ("convin_project_kernel", [F32, 1, False, 8, False, True]), dict(ci_mask=True)),
    ("fp32-31-conv_in", "fp32", 31, {}, {}, "conv_in", ("convin_project_kernel", [F32, 1, False, 8, False, False]),
     dict(nxp=5, ci_grid_x=5, ci_grid_y=8, ci_grid_z=31)),
    ("fp32-32-conv_in", "fp32", 32, {}, {}, "conv_in", ("convin_project_kernel", [F32, 5, False, 8, False, False]),
     dict(nxp=1, ci_grid_x=256, ci_grid_y=1, ci_grid_z=1)),
]


def _planned_instantiation(plan, prec, probe):
    """The template arguments the PLAN gives the probed launch (None where the plan names the family only: a layer's own launch)."""
    T = F16 if prec == "fp16" else F32
    mode = {"fp32": NATIVE, "fp16": NATIVE, "fp16x3": SPLIT, "bf16": BF16}[prec]
    if probe == "conv_in":
        return "convin_project_kernel", [T, plan["ci_sxw"], plan["ci_f16"], plan["ci_nw"], plan["ci_lo"], plan["ci_mask"]]
    if probe == "unet":
        if plan["form"] == "persistent_conv32":
            return "unet32_mega_kernel", [mode, plan["fused"]]
        return "unet_mega_kernel", [T, mode, plan["form"] == "persistent_winograd"]
    return {"conv16": "conv16_kernel", "conv32": "conv32_kernel", "winograd": "wino_kernel", "up_gemm": "up_kernel"}[plan["layers"][probe]], None


def _spellings(kernel, targs):
    """The kernel's name as the runtime may give it: demangled, or the Itanium-mangled instantiation."""
    if targs is None:
        return kernel + "<", kernel + "I"
    plain = [a[0] if isinstance(a, tuple) else str(a).lower() for a in targs]
    mangled = [a[1] if isinstance(a, tuple) else f"Lb{int(a)}E" if isinstance(a, bool) else f"Li{a}E" for a in targs]
    return kernel + "<" + ", ".join(plain) + ">", kernel + "I" + "".join(mangled) + "E"


@pytest.fixture(scope="module")
def setup():
    net = networks.get_network("giga")
    net.load_state_dict(weights.make_state_dict(7))
    net = net.to(DEV).eval()
    L = _capi.lib()
    ev = (L.giga_event_create(), L.giga_event_create())
    yield net.packed_blob(DEV), ev
    L.giga_event_destroy(ev[0])
    L.giga_event_destroy(ev[1])


@pytest.mark.parametrize("cid,prec,B,kw,knobs,probe,kernel,fields", CASES, ids=[c[0] for c in CASES])
def test_planned_launches_are_the_ones_made(setup, monkeypatch, cid, prec, B, kw, knobs, probe, kernel, fields):
    blob, ev = setup
    for k in ("GIGA_WINOGRAD", "GIGA_C32_FUSE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    L = _capi.lib()
    code = _capi.ENCODER_PRECISION[_capi.PRECISION[prec]]
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    plan = convonet.encoder_plan(B, prec, cus=cus, **kw)
    assert {k: plan[k] for k in fields} == fields, plan
    name, targs = _planned_instantiation(plan, prec, probe)
    assert name == kernel[0] and (targs == kernel[1] if probe in ("conv_in", "unet") else targs is None), plan
    x = torch.from_numpy(synth.tsdf_batch(3, B)).to(DEV)
    nhwc = torch.empty((3, B, 40, 40, 32), device=DEV, dtype=_capi.PLANE_DTYPE[code])
    ws = torch.empty(L.giga_encoder_workspace_bytes(B, code), device=DEV, dtype=torch.uint8)
    word = convonet.encoder_precision_word(code, **kw)
    ordinal = 1 if probe == "conv_in" else 3 if probe == "unet" else 3 + probe
    assert ordinal <= plan["launches"] and (probe != "unet" or plan["persistent"])
    before = L.giga_launch_count()
    L.giga_launch_probe(before + ordinal, ev[0], ev[1])
    try:
        with torch.cuda.device(DEV):
            rc = L.giga_encoder_forward(_capi.ptr(x), _capi.ptr(blob), _capi.ptr(nhwc), None, B, word, _capi.ptr(ws), ws.numel(),
                                        _capi.stream_ptr(DEV))
        torch.cuda.synchronize()
        got = (L.giga_launch_probe_name() or b"").decode().replace("(int)", "").replace("(bool)", "")
    finally:
        L.giga_launch_probe(0, None, None)
    assert rc == 0
    assert L.giga_launch_count() - before == plan["launches"]
    assert L.giga_encoder_last_path() == plan["path"]
    assert any(s in got for s in _spellings(*kernel)), (got, plan)
    assert bool(torch.isfinite(nhwc.float()).all())
