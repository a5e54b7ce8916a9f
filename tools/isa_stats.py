#!/usr/bin/env python
"""Per-kernel ISA statistics of a hipcc -save-temps gfx950 .s file: VGPR/AGPR use, scratch, MFMA and VALU mix.
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -c X.hip -save-temps=obj -o /tmp/x.o ; python tools/isa_stats.py /tmp/X-hip-amdgcn-amd-amdhsa-gfx950.s [filter] [--runs]
--runs adds, per kernel, the run-length histogram of VALU instructions between consecutive MFMAs ({VALU in the gap: number of
gaps}; an fp32 MFMA does not co-execute with VALU work and a lone VALU instruction costs ≈3x one in a run) and the
MFMA ordinals (0-based, in program order) in front of which a gap of 1-3 VALU instructions sits."""
import collections
import re
import sys

args = [a for a in sys.argv[1:] if a != "--runs"]
runs = "--runs" in sys.argv[1:]
s = open(args[0]).read()
flt = args[1] if len(args) > 1 else ""


def valu_runs(body):
    """({VALU instructions in a gap: gaps}, [ordinal of the MFMA behind each gap of 1-3]) over consecutive MFMAs of body."""
    hist, short, n, gap = collections.Counter(), [], 0, None
    for line in body.split("\n"):
        op = line.split(None, 1)[0] if line.strip() else ""
        if op.startswith("v_mfma"):
            if gap is not None:
                hist[gap] += 1
                if 1 <= gap <= 3:
                    short.append(n)
            n, gap = n + 1, 0
        elif op.startswith("v_") and gap is not None:
            gap += 1
    return dict(sorted(hist.items())), short


for m in re.finditer(r'^(_Z\w+):.*?\n(.*?)\.Lfunc_end\d+:', s, re.S | re.M):
    name, body = m.group(1), m.group(2)
    if flt not in name:
        continue
    def setv(k):
        r = re.search(r'\.set ' + re.escape(name) + r'\.' + k + r', (\d+)', s)
        return int(r.group(1)) if r else None
    pats = {"mfma": r"v_mfma", "fma_mix": r"v_fma_mix", "cvt_pk_f16": r"v_cvt_pk_f16_f32|v_cvt_pkrtz", "cvt_f16": r"v_cvt_f16_f32",
            "cvt_f32_f16": r"v_cvt_f32_f16", "max_i32": r"v_max_i32", "ds_read": r"ds_read", "ds_write": r"ds_write",
            "global_load": r"global_load", "scratch": r"scratch_", "s_nop": r"s_nop", "waitcnt": r"s_waitcnt", "accvgpr": r"v_accvgpr"}
    cnt = {k: len(re.findall(v, body)) for k, v in pats.items()}
    valu = len(re.findall(r'^\s+v_(?!mfma)', body, re.M))
    print(f"{name[:90]}\n   vgpr {setv('num_vgpr')} agpr {setv('num_agpr')} sgpr {setv('numbered_sgpr')} scratch {setv('private_seg_size')} "
          f"lines {body.count(chr(10))} valu {valu} " + " ".join(f"{k} {v}" for k, v in cnt.items() if v))
    if runs:
        hist, short = valu_runs(body)
        spans = []                                              # consecutive ordinals as first-last
        for n in short:
            if spans and n == spans[-1][1] + 1:
                spans[-1][1] = n
            else:
                spans.append([n, n])
        where = " ".join(str(a) if a == b else f"{a}-{b}" for a, b in spans) or "none"
        print(f"   VALU between consecutive MFMAs {hist}\n   gaps of 1-3 VALU in front of MFMA # {where}")
