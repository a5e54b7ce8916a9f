"""The oracle against the reference network itself, through golden G14 (oracle/make_goldens.py g14): the reference's
state-dict layout, its forward and encoder planes (a fixed sample and per-image sums) on seeded realistic scenes, and the plane-cell indices its
coordinate2index / normalize_coordinate assign to the 40^3 voxel centres."""
import numpy as np
import pytest
import torch

from giga_amd import synth, weights
from oracle import giga_oracle as O
from oracle.make_goldens import plane_sample, plane_sums


@pytest.fixture(scope="module")
def g14(golden):
    return golden("g14_reference_network.npz")


def test_state_dict_keys_match_reference(g14):
    names = [str(k) for k in g14["param_names"]]
    assert names == list(weights.giga_param_shapes().keys())
    for k, row in zip(names, g14["param_shapes"]):
        assert tuple(int(d) for d in row[1:1 + row[0]]) == weights.giga_param_shapes()[k], k


def test_forward_matches_reference(g14):
    sd = weights.make_state_dict(int(g14["weight_seed"]))
    s0, n, B = int(g14["first_scene"]), int(g14["n_points"]), g14["qual"].shape[0]
    x = torch.from_numpy(synth.tsdf_batch(s0, B, realistic=True))
    p = torch.from_numpy(synth.query_points(s0, B, n, stream=int(g14["stream"]), half_width=float(g14["half_width"])))
    with torch.no_grad():
        got = O.model_forward(sd, x, p, p_tsdf=p)
        got_c = O.encoder_forward(sd, x)
    for name, b in zip(("qual", "rot", "width", "tsdf"), got):
        a = torch.from_numpy(g14[name])
        assert a.shape == b.shape, name
        assert (a - b).abs().max().item() < 2e-5, name
    for k in O.PLANES:                                  # a fixed 1/8 of every plane, and each (scene, channel) image's sums
        a = torch.from_numpy(g14[f"plane_{k}_sample"])
        assert (a - torch.from_numpy(plane_sample(got_c[k]))).abs().max().item() < 2e-5, k
        ref, sums = g14[f"plane_{k}_sums"], plane_sums(got_c[k])
        assert ref.shape == sums.shape == (B, 32, 2), k
        assert (np.abs(sums - ref) <= 2e-6 * np.maximum(1.0, ref[..., 1:])).all(), k


def test_scatter_mean_is_axis_mean(g14):
    """The closed form of SURVEY 8a/a4: every plane cell receives exactly the 40 voxels along the
    projected axis, independent of the scatter stub's arithmetic."""
    ijk = torch.stack(torch.meshgrid(*(torch.arange(40),) * 3, indexing="ij"), -1).reshape(-1, 3)
    for plane, (a0, a1) in (("xz", (0, 2)), ("xy", (0, 1)), ("yz", (1, 2))):
        idx = torch.from_numpy(g14[f"index_{plane}"].astype("int64"))
        assert torch.equal(idx, ijk[:, a0] + 40 * ijk[:, a1])
        assert torch.equal(torch.bincount(idx, minlength=1600), torch.full((1600,), 40))
