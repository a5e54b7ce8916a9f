"""GPU tests of giga_amd.scenes: packed scenes decided by giga_mesh_collide, and the geometry data set they make."""
import json

import numpy as np
import pytest
import torch

import collide_emu as cemu
from giga_amd import geometry, perception, render, scenes

pytestmark = pytest.mark.gpu
BOXES = ("box_a", "box_b", "box_c")
MIXED = ("box_a", "prism", "sphere")
SEED, N_SCENES = 2, 8                         # chosen on the host: see the box test's last assertion


def dev():
    return torch.device("cuda:0")


def object_set(tmp_path_factory, names):
    return scenes.ObjectSet(cemu.write_object_set(tmp_path_factory.mktemp("objects") / "set", names))


def _same(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and x[1] == y[1] and np.array_equal(x[2], y[2]) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ boxes: a 2-D oracle
def _rect_gap(a, b):
    """separating-axis test of two rectangles (centre, half extents, yaw) in float64: the largest gap over the four axes;
    positive = apart, negative = overlapping"""
    gap = -np.inf
    for p in (a, b):
        for k in range(2):
            axis = np.array([np.cos(p[2] + k * np.pi / 2), np.sin(p[2] + k * np.pi / 2)])
            reach = 0.0
            for q in (a, b):
                ux = np.array([np.cos(q[2]), np.sin(q[2])])
                uy = np.array([-ux[1], ux[0]])
                reach += q[1][0] * abs(ux[0] * axis[0] + ux[1] * axis[1]) + q[1][1] * abs(uy[0] * axis[0] + uy[1] * axis[1])
            d = (b[0][0] - a[0][0]) * axis[0] + (b[0][1] - a[0][1]) * axis[1]
            gap = max(gap, abs(d) - reach)
    return gap


def test_box_scenes_equal_the_rectangle_oracle(tmp_path_factory):
    """Boxes yawed about z standing on one table overlap iff their rectangles do."""
    objects = object_set(tmp_path_factory, BOXES)
    got = scenes.generate_packed_scenes(objects, N_SCENES, seed=SEED, batch=4, device=dev())
    half = [np.abs(objects.mesh(k)[0]).max(axis=0) for k in range(3)]      # (the files' own numbers)
    closest, turned_away = np.inf, 0
    for s in range(N_SCENES):
        count, attempts = scenes.packed_candidates(objects, SEED, s)
        rects = [((a["x"], a["y"]), half[a["index"]][:2] * a["scale"], a["yaw"]) for a in attempts]
        hit = np.zeros((12, 12), bool)
        for i in range(12):
            for j in range(i):
                gap = _rect_gap(rects[i], rects[j])
                closest = min(closest, abs(gap))
                hit[i, j] = hit[j, i] = gap < 0
        kept = scenes.resolve_packed(hit, np.zeros(12, bool), count)
        assert [e[0] for e in got[s]] == [a["path"] for a, k in zip(attempts, kept) if k]
        assert all(np.array_equal(e[2], a["pose"]) for e, a in zip(got[s], [a for a, k in zip(attempts, kept) if k]))
        turned_away += min(count, 12) - int(kept.sum())
    assert closest > 1e-6 and turned_away > 0      # no rectangle pair near touching (checked on the host), and collisions did occur


# ------------------------------------------------------------------------------------------------------------ mixed set
def test_mixed_scenes_equal_the_restatement_and_do_not_depend_on_the_batch(tmp_path_factory):
    objects = object_set(tmp_path_factory, MIXED)
    by4 = scenes.generate_packed_scenes(objects, N_SCENES, seed=SEED, batch=4, device=dev())
    by1 = scenes.generate_packed_scenes(objects, N_SCENES, seed=SEED, batch=1, device=dev())
    host = scenes.generate_packed_scenes(objects, N_SCENES, seed=SEED, batch=3, collide=cemu.mesh_collide)
    assert all(_same(a, b) and _same(a, c) for a, b, c in zip(by4, by1, host))
    kinds = set()
    for s, kept in enumerate(by4):
        count = scenes.packed_candidates(objects, SEED, s)[0]
        assert 1 <= len(kept) <= count
        bodies = [render.scene_mesh([(*geometry.default_mesh_loader(p), sc, pose)]) for p, sc, pose in kept]
        assert not cemu.mesh_collide(bodies, [(i, j) for i in range(len(bodies)) for j in range(i)]).any()
        kinds |= {p.rsplit("/", 1)[1] for p, _, _ in kept}
    assert kinds == {"box_a.urdf", "prism.urdf", "sphere.urdf"}


# ------------------------------------------------------------------------------------------------------------- data set
@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """two scenes of the box set, written once and shared"""
    objects = object_set(tmp_path_factory, BOXES)
    base = tmp_path_factory.mktemp("geo_set")
    raw, root = base / "raw", base / "data"
    ids = scenes.write_geo_dataset(objects, raw, root, 2, seed=SEED, batch=2, num_point_per_file=512, num_file=2, device=dev())
    return objects, raw, root, ids


def test_write_geo_dataset_files(written):
    objects, raw, root, ids = written
    assert ids == [scenes.scene_id(SEED, 0), scenes.scene_id(SEED, 1)]
    for sid in ids:
        assert (raw / "mesh_pose_list" / (sid + ".npz")).exists() and (raw / "scenes" / (sid + ".npz")).exists()
        assert sorted(p.name for p in (raw / "occ" / sid).iterdir()) == ["0000.npz", "0001.npz"]
        assert (root / "scenes" / (sid + ".npz")).exists() and (root / "point_clouds" / (sid + ".npz")).exists()
        with np.load(raw / "scenes" / (sid + ".npz")) as d:
            assert d["depth_imgs"].shape == (6, 480, 640) and d["extrinsics"].shape == (6, 7)
            assert d["extrinsics"].dtype == np.float64 and d["depth_imgs"].dtype == np.float32
            assert 0.3 < d["depth_imgs"].min() < 0.6 and (d["depth_imgs"] < 2.0).mean() > 0.5      # objects and table in view
        with np.load(raw / "occ" / sid / "0000.npz") as d:
            assert d["points"].shape == (512, 3) and d["points"].dtype == np.float16 and d["occ"].shape == (512,)
    with (raw / "setup.json").open() as fh:
        setup = json.load(fh)
    assert setup["size"] == 0.3 and setup["finger_depth"] == 0.05 and setup["max_opening_width"] == 0.08 and "intrinsic" in setup
    rows = open(raw / "grasps.csv").read().splitlines()
    assert rows[0] == "scene_id,qx,qy,qz,qw,x,y,z,width,label"
    assert rows[1:] == [sid + ",0.0,0.0,0.0,1.0,0.15,0.15,0.15,0.0,0" for sid in ids]
    lists = scenes.generate_packed_scenes(objects, 2, seed=SEED, batch=2, collide=cemu.mesh_collide)
    for sid, want in zip(ids, lists):
        entries, mesh_list = geometry.read_mesh_pose_list(raw, sid)
        assert len(entries) == len(want) and all(np.array_equal(e[3], w[2]) and e[2] == w[1] for e, w in zip(entries, want))


def test_geo_dataset_item_and_analytic_box_labels(written):
    objects, raw, root, ids = written
    ds = geometry.VoxelOccGeoDataset(root, raw, num_point_occ=20000, seed=1, device=dev())
    assert len(ds) == 2 and ds.scene_list == ids
    item = ds.item(0)
    assert item["grid"].shape == (40, 40, 40) and item["grid"].min() < item["grid"].max()
    assert len(item["mesh_list"]) == len(geometry.read_mesh_pose_list(raw, ids[0])[0]) >= 1
    # the labels are the analytic inside-some-box test on the returned points (normalised: world / size - 0.5, float32)
    occ = item["occ"]
    assert item["points"].shape == (20000, 3) and item["points"].dtype == torch.float32 and occ.shape == (20000,)
    p = (item["points"].double().cpu().numpy() + 0.5) * ds.size
    inside = np.zeros(len(p), bool)
    margin = np.full(len(p), np.inf)
    for path, scale, pose in np.load(raw / "mesh_pose_list" / (ids[0] + ".npz"), allow_pickle=True)["pc"]:
        half = np.abs(geometry.default_mesh_loader(path)[0]).max(axis=0) * scale
        local = (p - pose[:3, 3])
        local = np.stack([local[:, 0] * pose[0, k] + local[:, 1] * pose[1, k] + local[:, 2] * pose[2, k] for k in range(3)], axis=1)
        d = (np.abs(local) - half).max(axis=1)                              # < 0 inside
        inside |= d < 0
        margin = np.minimum(margin, np.abs(d))
    # the mesh the kernel sees has float32 vertices and the points were normalised in float32 (each within 3e-8 here): a point closer than 1e-6 to a face may fall on
    # either side and is left out; the others must agree
    clear = margin > 1e-6
    assert clear.mean() > 0.999 and 200 < inside.sum() < len(p) - 200
    assert np.array_equal(occ.cpu().numpy()[clear], inside[clear])
    # ... and the files hold labels of the same kind
    with np.load(raw / "occ" / ids[0] / "0001.npz") as d:
        assert d["occ"].dtype == bool and 0 < d["occ"].sum() < 512


def test_written_grids_equal_acquire_tsdfs_on_the_scene_meshes_plus_table(written):
    """The grids construct_dataset wrote against acquire_tsdfs on the same scene meshes plus table, byte for byte."""
    objects, raw, root, ids = written
    table = scenes.table_mesh()
    meshes = []
    for sid in ids:
        v, f = render.scene_mesh(geometry.read_mesh_pose_list(raw, sid)[0])
        meshes.append((np.concatenate((v, table[0])), np.concatenate((f, table[1] + len(v)))))
    want = render.acquire_tsdfs(meshes, 6, device=dev()).cpu().numpy()
    for b, sid in enumerate(ids):
        got = np.load(root / "scenes" / (sid + ".npz"))["grid"]
        assert got.shape == (1, 40, 40, 40) and got.dtype == np.float32
        differ = int((got[0].view(np.uint32) != want[b].view(np.uint32)).sum())
        print("scene", sid, "voxels that differ:", differ, "largest difference:", float(np.abs(got[0] - want[b]).max()))
        assert differ == 0


def test_one_geo_trainer_step_on_the_written_set(written):
    from giga_amd import networks, resident, trainer, weights
    from giga_amd.dataset import GraspOccDataset
    objects, raw, root, ids = written
    rset = resident.ResidentTrainingSet(GraspOccDataset(str(root), str(raw), num_point_occ=64), device=str(dev()))
    assert len(rset) == 2
    batches = resident.ResidentBatches(rset, 2, shuffle=False, seed=0, drop_last=True)
    net = networks.get_network("giga_geo")
    net.load_state_dict(weights.make_state_dict(7, heads=("decoder_tsdf",)))
    tr = trainer.GeoTrainer(net.to(dev()), batches, quiet=True)
    loss = tr.train_step(next(iter(batches)))
    assert torch.isfinite(loss).all() and float(loss.detach()) > 0
