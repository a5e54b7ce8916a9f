"""HIP-event times of the one-query fp32 grasp-head launch (N = 1, mask 7): decoder_f32_point_kernel against
decoder_f32_tile_kernel (GIGA_DEC32_POINT=0) at the same P, and beyond the tile kernel's own rule against whatever the
dispatch takes there.  Each number is a median of seven; the empty bracket (two events, nothing between) is printed beside
them, taken with the same events.  DEC32_POINT_MAX_P of csrc/giga_decoder.hip is set from this table
(profiles/dec_point/sweep.txt).  GIGA_DIAG_B=1,32,... replaces the list of sizes.
    PYTHONPATH=. python tools/gpu_dec_point_sweep.py"""
import ctypes
import os

import numpy as np
import torch

from giga_amd import _capi, networks, synth, weights
from giga_amd.convonet import decode_heads

BS = [int(b) for b in os.environ.get("GIGA_DIAG_B", "1,8,32,64,128,256,384,512,768,1024").split(",")]
dev = torch.device("cuda:0")
net = networks.get_network("giga")
net.load_state_dict(weights.make_state_dict(7))
net = net.to(dev).eval().set_precision("fp32")
blob = net.packed_blob(dev)
L = _capi.lib()
ev = (L.giga_event_create(), L.giga_event_create())
ms = ctypes.c_float()


def elapsed():
    torch.cuda.synchronize()
    _capi.check(L.giga_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)), "event")
    return ms.value * 1e3


def empty_bracket():
    """The same two events, on the same stream and read the same way as the launch probe's, with nothing between them."""
    stream = _capi.stream_ptr(dev)
    t = []
    for _ in range(3 + 7):
        _capi.check(L.giga_event_record(ev[0], stream), "event")
        _capi.check(L.giga_event_record(ev[1], stream), "event")
        t.append(elapsed())
    return float(np.median(t[3:])), float(np.min(t[3:]))


def timed(c, p, knob):
    if knob is None:
        os.environ.pop("GIGA_DEC32_POINT", None)
    else:
        os.environ["GIGA_DEC32_POINT"] = knob
    t, name = [], ""
    with torch.no_grad():
        for _ in range(3):
            decode_heads(c.nhwc, p, blob, 7, "fp32", True)
        for _ in range(7):
            L.giga_launch_probe(L.giga_launch_count() + 1, ev[0], ev[1])
            decode_heads(c.nhwc, p, blob, 7, "fp32", True)
            t.append(elapsed())
            name = (L.giga_launch_probe_name() or b"").decode()
        L.giga_launch_probe(0, None, None)
    os.environ.pop("GIGA_DEC32_POINT", None)
    short = "point" if "point_kernel" in name else "tile" if "tile_kernel" in name else "general"
    return float(np.median(t)), float(np.min(t)), short


print("empty bracket (the probe's events, nothing between): %.1f / %.1f us" % empty_bracket())
print("    B   forced point kernel      GIGA_DEC32_POINT=0        default dispatch   (median / min of seven, us)")
for B in BS:
    x = torch.from_numpy(synth.tsdf_batch(0, min(B, 64))).to(dev)
    with torch.no_grad():
        c = net.encode_inputs(x)
    if B > 64:                                            # planes of 64 scenes repeated: the decoder's work does not depend on them
        class C:
            nhwc = c.nhwc.repeat(1, (B + 63) // 64, 1, 1, 1)[:, :B].contiguous()
        c = C
    p = torch.from_numpy(synth.query_points(0, B, 1, stream=2)).to(dev)
    row = [timed(c, p, k) for k in ("3072", "0", None)]
    print(f"{B:5d}   " + "   ".join(f"{m:7.1f} / {lo:7.1f} {nm:8s}" for m, lo, nm in row))
print("empty bracket again: %.1f / %.1f us" % empty_bracket())
