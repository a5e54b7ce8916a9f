"""giga_amd.scenes on the host: the draws, the acceptance rule, the scene lists and their files.  The collision decision is the
numpy restatement (tests/collide_emu.py) passed as `collide=`; object sets are a few small files written into tmp_path."""
import numpy as np
import pytest

import collide_emu as cemu
from giga_amd import geometry, render, scenes

MIXED = ("box_a", "prism_sunk", "sphere")


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    return scenes.ObjectSet(cemu.write_object_set(tmp_path_factory.mktemp("objects") / "mixed", MIXED))


def test_object_set_lists_urdfs_sorted_or_obj_files(tmp_path, mixed):
    assert [p.rsplit("/", 1)[1] for p in mixed.paths] == ["box_a.urdf", "prism_sunk.urdf", "sphere.urdf"] and len(mixed) == 3
    assert mixed.global_scaling == 1.0
    v, f = mixed.mesh(1)
    assert v.dtype == np.float64 and f.dtype == np.int64 and v.shape == (12, 3) and f.shape == (20, 3) and mixed.mesh(1)[0] is v
    objs = scenes.ObjectSet(cemu.write_object_set(tmp_path / "blocks", ("box_b", "box_a"), urdf=False))
    assert [p.rsplit("/", 1)[1] for p in objs.paths] == ["box_a.obj", "box_b.obj"]
    assert objs.global_scaling == 1.67                                     # the reference's table, by directory name
    assert scenes.ObjectSet(tmp_path / "blocks", global_scaling=0.5).global_scaling == 0.5
    assert scenes.GLOBAL_SCALING == {"blocks": 1.67, "google": 0.7, "google_pile": 0.7, "google_packed": 0.7}
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError):
        scenes.ObjectSet(tmp_path / "empty")


def test_packed_candidates_follow_the_stated_draws(mixed):
    for seed, scene in ((0, 0), (0, 1), (3, 7)):
        count, attempts = scenes.packed_candidates(mixed, seed, scene)
        again = scenes.packed_candidates(mixed, seed, scene)
        assert count == again[0] and all(np.array_equal(a["pose"], b["pose"]) and a["path"] == b["path"] for a, b in zip(attempts, again[1]))
        rng = np.random.default_rng([seed, scene])                         # the stated order, restated
        assert count == rng.poisson(4) + 1 and len(attempts) == 12
        for a in attempts:
            assert a["index"] == rng.integers(3) and a["path"] == mixed.paths[a["index"]]
            assert a["x"] == rng.uniform(0.08, 0.22) and a["y"] == rng.uniform(0.08, 0.22)
            assert a["yaw"] == rng.uniform(0.0, 2.0 * np.pi) and a["draw"] == rng.uniform(0.7, 0.9)
            assert 0.08 <= a["x"] < 0.22 and 0.08 <= a["y"] < 0.22 and 0 <= a["yaw"] < 2 * np.pi and 0.7 <= a["draw"] < 0.9
            assert a["scale"] == mixed.global_scaling * a["draw"]
            vz = mixed.mesh(a["index"])[0][:, 2] * a["scale"]
            c, s = np.cos(a["yaw"]), np.sin(a["yaw"])
            want = np.array([[c, -s, 0, a["x"]], [s, c, 0, a["y"]], [0, 0, 1, 0.05 + 0.5 * (vz.max() - vz.min()) + 0.002], [0, 0, 0, 1]])
            assert np.array_equal(a["pose"], want)
            # this prism's origin lies above its centre, so it ends up sunk into the table; the centred objects clear it by 2 mm
            assert a["table_hit"] == (a["index"] == 1)
            placed = render.scene_mesh([(*mixed.mesh(a["index"]), a["scale"], a["pose"])])[0]
            assert (placed[:, 2].min() < 0.05) == a["table_hit"]
    assert scenes.packed_candidates(mixed, 0, 0)[1][0]["pose"].tolist() != scenes.packed_candidates(mixed, 0, 1)[1][0]["pose"].tolist()
    assert scenes.packed_candidates(mixed, 0, 1)[1][0]["pose"].tolist() != scenes.packed_candidates(mixed, 1, 1)[1][0]["pose"].tolist()


def test_resolve_packed_on_hand_made_matrices():
    n = 5
    none, free = np.zeros((n, n), bool), np.zeros(n, bool)
    assert scenes.resolve_packed(none, free, 9).tolist() == [True] * 5
    assert scenes.resolve_packed(none, free, 3).tolist() == [True, True, True, False, False]      # the object_count stop
    assert scenes.resolve_packed(none, free, 0).tolist() == [False] * 5
    table = np.array([True, False, False, True, False])
    assert scenes.resolve_packed(none, table, 9).tolist() == [False, True, True, False, True]     # the table rejection
    assert scenes.resolve_packed(none, table, 2).tolist() == [False, True, True, False, False]    # ... does not use up the count
    hit = none.copy()
    hit[0, 1] = hit[1, 0] = True           # 1 collides with the kept 0: rejected
    hit[1, 2] = hit[2, 1] = True           # 2 collides only with the rejected 1: kept
    hit[2, 4] = hit[4, 2] = True           # 4 collides with the kept 2: rejected
    assert scenes.resolve_packed(hit, free, 9).tolist() == [True, False, True, True, False]
    assert scenes.resolve_packed(hit, np.array([True, False, False, False, False]), 9).tolist() == [False, True, False, True, True]
    assert scenes.resolve_packed(np.zeros((0, 0), bool), np.zeros(0, bool), 3).tolist() == []


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """six scenes of a centred object set (nothing touches the table), batch 4: computed once, shared"""
    objects = scenes.ObjectSet(cemu.write_object_set(tmp_path_factory.mktemp("objects") / "set", ("box_a", "box_b", "sphere")))
    return objects, scenes.generate_packed_scenes(objects, 6, seed=2, batch=4, collide=cemu.mesh_collide)


def _same(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and x[1] == y[1] and np.array_equal(x[2], y[2]) for x, y in zip(a, b))


def test_generate_packed_scenes_batch_1_equals_batch_4(generated):
    objects, by4 = generated
    by1 = scenes.generate_packed_scenes(objects, 6, seed=2, batch=1, collide=cemu.mesh_collide)
    assert len(by1) == len(by4) == 6 and all(_same(a, b) for a, b in zip(by1, by4))
    shifted = scenes.generate_packed_scenes(objects, 3, seed=2, first_scene=2, batch=2, collide=cemu.mesh_collide)
    assert all(_same(a, b) for a, b in zip(shifted, by4[2:5]))             # (seed, scene) alone
    rejected = 0
    for s, kept in enumerate(by4):
        count, attempts = scenes.packed_candidates(objects, 2, s)
        assert 1 <= len(kept) <= count
        assert kept[0][0] == attempts[0]["path"]                           # the first attempt meets an empty table
        bodies = [render.scene_mesh([(*geometry.default_mesh_loader(p), sc, pose)]) for p, sc, pose in kept]
        pairs = [(i, j) for i in range(len(bodies)) for j in range(i)]
        assert not cemu.mesh_collide(bodies, pairs).any()
        rejected += min(count, 12) - len(kept)
    assert rejected > 0                                                    # some attempt was turned away by a collision
    calls = []
    scenes.generate_packed_scenes(objects, 5, seed=2, batch=2, collide=lambda m, p: calls.append((len(m), len(p))) or np.zeros(len(p), bool))
    assert calls == [(24, 132), (24, 132), (12, 66)]                       # 12 bodies and 66 pairs per scene, one call per batch


def test_mesh_pose_list_file_loads_through_the_geometry_reader(generated, tmp_path):
    objects, lists = generated
    scenes.write_mesh_pose_list(tmp_path, "abc", lists[0])
    scenes.write_mesh_pose_list(tmp_path, "none", [])
    pc = np.load(tmp_path / "mesh_pose_list" / "abc.npz", allow_pickle=True)["pc"]
    assert pc.dtype == object and pc.shape == (len(lists[0]), 3)
    entries, mesh_list = geometry.read_mesh_pose_list(tmp_path, "abc")
    assert len(entries) == len(mesh_list) == len(lists[0])
    for (v, f, scale, pose), (path, want_scale, want_pose), mesh in zip(entries, lists[0], mesh_list):
        assert scale == want_scale and np.array_equal(pose, want_pose)
        assert np.array_equal(mesh[0], render.scene_mesh([(*geometry.default_mesh_loader(path), want_scale, want_pose)])[0])
    assert geometry.read_mesh_pose_list(tmp_path, "none") == ([], [])


def test_table_mesh_corners_and_height():
    v, f = scenes.table_mesh()
    assert v.dtype == np.float32 and f.dtype == np.int32 and f.tolist() == [[0, 1, 2], [0, 2, 3]]
    assert np.allclose(v, [[-0.15, -0.15, 0.05], [0.45, -0.15, 0.05], [0.45, 0.45, 0.05], [-0.15, 0.45, 0.05]], atol=1e-7)
    n = np.cross(v[1] - v[0], v[2] - v[0])
    assert n[2] > 0 and n[0] == n[1] == 0                                   # facing up
    v, _ = scenes.table_mesh(size=0.4, height=0.1, extent=1.0)
    assert np.allclose(v[[0, 2]], [[-0.3, -0.3, 0.1], [0.7, 0.7, 0.1]], atol=1e-7)


def test_command_line_flags_and_defaults():
    from pathlib import Path

    from giga_amd import generate_scenes
    args = generate_scenes.build_parser().parse_args(["--object-set", "o", "--raw", "r", "--dataset", "d"])
    assert (args.object_set, args.raw, args.dataset) == (Path("o"), Path("r"), Path("d"))
    assert (args.num_scenes, args.seed, args.batch, args.first_scene, args.views) == (100, 0, 32, 0, 6)
    args = generate_scenes.build_parser().parse_args("--object-set o --raw r --dataset d --num-scenes 7 --seed 3 --batch 2".split())
    assert (args.num_scenes, args.seed, args.batch) == (7, 3, 2)
    with pytest.raises(SystemExit):
        generate_scenes.build_parser().parse_args(["--raw", "r", "--dataset", "d"])
    assert "no grasp labels" in scenes.write_geo_dataset.__doc__ and "WITHOUT `--ROI`" in scenes.write_geo_dataset.__doc__


def test_exports():
    import giga_amd
    for name in ("ObjectSet", "packed_candidates", "resolve_packed", "generate_packed_scenes", "table_mesh", "write_geo_dataset"):
        assert getattr(giga_amd, name) is getattr(scenes, name)
