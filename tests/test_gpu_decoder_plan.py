"""What is planned is what runs: for ten small decoder launches, one per kernel family and operand form, the library's launch probe
names the kernel and template arguments of convonet.decoder_plan (csrc/giga_dec_plan.h), and giga_launch_count rises by the
launches of the call.  The shapes are the smallest that still reach each family; the plans are also written out by hand, so the
test fails when the policy moves as well as when launch and plan part."""
import torch

import pytest

from giga_amd import _capi, convonet, networks, weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CODE = {"fp32": 0, "fp16": 1, "fp16x3": 2}
F16, F16S, LAT = "decoder_f16_kernel", "decoder_f16s_kernel", "decoder_lat_kernel"
F32, TILE, POINT = "decoder_f32_kernel", "decoder_f32_tile_kernel", "decoder_f32_point_kernel"
# (id, precision, B, N (generic) or 0, R (lattice) or 0, {knob: value}, the plan's kernel, the fields the case is about)
CASES = [
    ("fp32-point", "fp32", 3, 1, 0, {}, POINT, dict(grid_x=3, grid_y=3)),
    ("fp32-tile", "fp32", 3, 1, 0, {"GIGA_DEC32_POINT": "0"}, TILE, dict(grid_x=1, grid_y=3)),
    ("fp32-general", "fp32", 3, 43, 0, {}, F32, dict(T=1, heads_per_wg=1, grid_x=2, grid_y=3)),
    ("fp16-resident", "fp16", 1, 100, 0, {}, F16S, dict(T=1, NW=12, split=False)),
    ("fp16x3-resident", "fp16x3", 1, 100, 0, {}, F16S, dict(T=1, NW=8, split=True)),
    ("fp16-shared", "fp16", 1, 100, 0, {"GIGA_DEC16_RESIDENT": "0"}, F16, dict(T=2, NW=8, grid_x=1)),
    ("lat-fp16x3", "fp16x3", 1, 0, 8, {}, LAT, dict(NW=16, split=True, dbuf=False)),
    ("lat-fp16-dbuf", "fp16", 4, 0, 8, {}, LAT, dict(NW=16, split=False, dbuf=True)),
    ("fp16-resident-lattice", "fp16", 1, 0, 8, {}, F16S, dict(T=1, NW=12, split=False)),
    ("fp16x3-resident-lattice", "fp16x3", 1, 0, 9, {}, F16S, dict(T=1, NW=8, split=True)),
    ("fp32-general-lattice", "fp32", 1, 0, 8, {}, F32, dict(T=1, heads_per_wg=1, grid_y=3)),
]


def _template_args(plan, lattice):
    k = plan["kernel"]
    if k == F16:
        return [plan["T"], lattice, plan["NW"]]
    if k == F16S:
        return [plan["T"], lattice, plan["NW"], plan["split"]]
    if k == LAT:
        return [plan["split"], plan["NW"], plan["dbuf"]]
    if k == F32:
        return [plan["T"], lattice]
    return []


def _names(kernel, targs):
    """The kernel's name as the runtime may give it: demangled, or the Itanium-mangled instantiation."""
    if not targs:
        return (kernel,)
    plain = kernel + "<" + ", ".join(str(a).lower() if isinstance(a, bool) else str(a) for a in targs) + ">"
    mangled = kernel + "I" + "".join(f"Lb{int(a)}E" if isinstance(a, bool) else f"Li{a}E" for a in targs) + "E"
    return plain, mangled


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


@pytest.mark.parametrize("cid,prec,B,N,R,knobs,kernel,fields", CASES, ids=[c[0] for c in CASES])
def test_planned_kernel_is_the_one_launched(setup, monkeypatch, cid, prec, B, N, R, knobs, kernel, fields):
    blob, ev = setup
    for k in ("GIGA_DEC_LAT", "GIGA_DEC16_RESIDENT", "GIGA_DEC32_TILE", "GIGA_DEC32_POINT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    nheads = 3
    plan = convonet.decoder_plan(B, N, R, nheads, CODE[prec])
    assert plan["kernel"] == kernel and {k: plan[k] for k in fields} == fields, plan
    g = torch.Generator().manual_seed(B + N + R)
    nhwc = torch.randn(3, B, 40, 40, 32, generator=g).to(DEV).to(_capi.PLANE_DTYPE[CODE[prec]])
    if R:
        lin = torch.linspace(-0.5, 0.5, R)
        grid = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(1, -1, 3).contiguous()
        p = convonet.register_lattice(grid.to(DEV), lin.to(DEV))
    else:
        p = (torch.rand(B, N, 3, generator=g) - 0.5).to(DEV)
    launches = 2 if R else 1                                   # a lattice call resamples the planes first
    L = _capi.lib()
    before = L.giga_launch_count()
    L.giga_launch_probe(before + launches, ev[0], ev[1])       # the call's last launch: the decoder
    try:
        out = convonet.decode_heads(nhwc, p, blob, 7, prec, True)
        torch.cuda.synchronize()
        name = (L.giga_launch_probe_name() or b"").decode().replace("(int)", "").replace("(bool)", "")
    finally:
        L.giga_launch_probe(0, None, None)
    assert L.giga_launch_count() - before == launches
    assert any(n in name for n in _names(kernel, _template_args(plan, bool(R)))), (name, plan)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
