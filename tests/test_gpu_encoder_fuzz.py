"""Encoder planes at many batch sizes and input seeds, in all three precisions and both U-Net launch forms, against the CPU
oracle (first four, middle and last scene) and against the same scenes encoded alone.  The first four scenes of every batch
from 4 up are adversarial: empty, all ones, a single voxel, a checkerboard."""
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import networks, synth
from oracle import giga_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref64  # noqa: E402

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 9, 16, 17, 33, 48, 65)


@pytest.fixture(scope="module")
def net(sd7):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    n = networks.get_network("giga")
    n.load_state_dict(sd7)
    return n.to(torch.device("cuda:0")).eval()


@pytest.mark.parametrize("B", BATCHES)
def test_encoder_fuzz_against_oracle_and_alone(net, sd7, B):
    dev = torch.device("cuda:0")
    seed = int(np.random.default_rng(B).integers(0, 5000))
    x = torch.from_numpy(synth.tsdf_batch(seed, B))
    if B >= 4:
        x[:4] = torch.from_numpy(ref64.adversarial_scenes())
    xd = x.to(dev)
    ks = sorted({0, 1, 2, 3, B // 2, B - 1} & set(range(B)))
    refs = {k: O.encoder_forward(sd7, x[k:k + 1]) for k in ks}
    fails = []
    try:
        for prec, tol in (("fp32", 1e-4), ("fp16x3", 1e-4), ("fp16", 2e-2)):
            net.set_precision(prec)
            for persist in (False, True):
                net.set_persistent_unet(persist)
                with torch.no_grad():
                    pl = net.encode_inputs(xd)
                    for k in ks:
                        one = net.encode_inputs(xd[k:k + 1].contiguous())
                        for key in O.PLANES:
                            scale = max(1.0, float(refs[k][key].abs().max()))
                            e_or = (pl[key][k:k + 1].float().cpu() - refs[k][key]).abs().max().item() / scale
                            e_al = (pl[key][k:k + 1].float() - one[key].float()).abs().max().item() / scale
                            if e_or > tol or e_al > (1e-5 if prec != "fp16" else 1e-2) or not np.isfinite(e_or):
                                fails.append((prec, persist, k, key, e_or, e_al))
    finally:
        net.set_precision("fp32")
        net.set_persistent_unet(False)
    assert not fails, fails
