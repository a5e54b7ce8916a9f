"""Packed scenes from a directory of object meshes, and the geometry data set they make: the device counterpart of the reference's
`ClutterRemovalSim.generate_packed_scene` (src/vgn/simulation.py:118-143), which needs no dynamics to decide anything -- up to
12 attempts, each drawing an object, a position, a yaw and a scale, setting the object upright on the table and keeping it if and
only if it touches nothing.  "Touches" is `giga_amd.collision.mesh_collide` here (PyBullet there).  The draws of the 12 attempts
do not depend on which earlier attempts were kept, so all candidates of all scenes of a batch are tested in one launch and the
host resolves acceptance in attempt order.

    objects = ObjectSet("data/urdfs/packed/train")
    scenes = generate_packed_scenes(objects, 100, seed=0)          # per scene [(mesh_path, scale, pose 4x4)]
    write_geo_dataset(objects, "data/set_raw", "data/set", 100)     # everything train_geo / eval_geometry read

Not reproduced:
  * PyBullet's collision margins and contact distances: bodies collide when their surfaces intersect (or one holds a vertex of
    the other), not when they come within a margin;
  * `remove_and_wait`, the settling after each kept object: objects stay 2 mm above the table, and an unstable object does not
    topple;
  * inertial-frame offsets of URDFs: the pose is that of the mesh's own origin;
  * pile scenes (`generate_pile_scene` needs rigid-body dynamics) and the execution of a grasp: `write_geo_dataset` writes grasp
    labels only for the outcomes of an executor that the caller brings (`giga_amd.candidates` makes the candidates);
  * the extent of the reference's `plane.urdf` (the file is not part of this project): `table_mesh` takes an `extent`;
  * agreement with PyBullet itself is unverified.
The random stream is this module's own (`np.random.default_rng([seed, scene])`), so a scene depends on (seed, scene) alone."""
import json
import os
from pathlib import Path

import numpy as np

from . import geometry, render

MAX_ATTEMPTS = 12                              # simulation.py:120
TABLE_HEIGHT = 0.05                            # the gripper's finger_depth (simulation.py:68)
FINGER_DEPTH, MAX_OPENING_WIDTH = 0.05, 0.08   # what the reference's Gripper writes into setup.json
GLOBAL_SCALING = {"blocks": 1.67, "google": 0.7, "google_pile": 0.7, "google_packed": 0.7}     # simulation.py:23-29
ATTEMPT_PAIRS = np.array([(i, j) for i in range(MAX_ATTEMPTS) for j in range(i + 1, MAX_ATTEMPTS)], np.int64)    # 66 pairs


class ObjectSet:
    """The object files of a directory: its `*.urdf` files, sorted (simulation.py:45-47), or, without any, its `*.obj` files.
    Meshes are loaded through `geometry.default_mesh_loader` and cached.  global_scaling: the reference's table keyed by the
    directory's name (1.0 for other names) unless given."""

    def __init__(self, root, global_scaling=None):
        self.root = Path(root)
        files = sorted(f for f in self.root.iterdir() if f.suffix == ".urdf")
        if not files:
            files = sorted(f for f in self.root.iterdir() if f.suffix == ".obj")
        if not files:
            raise ValueError(f"{root}: no .urdf or .obj files")
        self.paths = [str(f) for f in files]
        self.global_scaling = float(GLOBAL_SCALING.get(self.root.name, 1.0) if global_scaling is None else global_scaling)
        self._meshes = {}

    def __len__(self):
        return len(self.paths)

    def mesh(self, index):
        """(vertices (V, 3) float64, faces (F, 3) int64) of object `index`, in its own frame and unscaled"""
        if index not in self._meshes:
            v, f = geometry.default_mesh_loader(self.paths[index])
            self._meshes[index] = (np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3))
        return self._meshes[index]


def packed_candidates(object_set, seed, scene, table_height=TABLE_HEIGHT):
    """The draws of one scene, all from np.random.default_rng([seed, scene]) in this order: object_count = poisson(4) + 1
    (scripts/generate_data_parallel.py:18,46); then for each of the 12 attempts the object index, x and y in U(0.08, 0.22), the yaw
    in U(0, 2 pi) and the scale in U(0.7, 0.9).  All 12 attempts are always drawn.  Returns (object_count, attempts); an attempt is
    a dict with `index`, `path`, `x`, `y`, `yaw`, `draw` (the drawn scale), `scale` (global_scaling * draw, what the mesh is
    scaled by), `pose` (4x4: the yaw about z; the centre at height table_height + 0.5 (zmax - zmin) + 0.002 of the scaled mesh,
    simulation.py:133-135) and `table_hit` (its lowest vertex ends up below the table)."""
    rng = np.random.default_rng([int(seed), int(scene)])
    object_count = int(rng.poisson(4)) + 1
    attempts = []
    for _ in range(MAX_ATTEMPTS):
        index = int(rng.integers(len(object_set)))
        x, y = float(rng.uniform(0.08, 0.22)), float(rng.uniform(0.08, 0.22))
        yaw = float(rng.uniform(0.0, 2.0 * np.pi))
        draw = float(rng.uniform(0.7, 0.9))
        scale = object_set.global_scaling * draw
        vz = object_set.mesh(index)[0][:, 2]
        zmin, zmax = (float(vz.min()) * scale, float(vz.max()) * scale) if len(vz) else (0.0, 0.0)
        z = table_height + 0.5 * (zmax - zmin) + 0.002
        c, s = np.cos(yaw), np.sin(yaw)
        pose = np.array([[c, -s, 0.0, x], [s, c, 0.0, y], [0.0, 0.0, 1.0, z], [0.0, 0.0, 0.0, 1.0]])
        attempts.append(dict(index=index, path=object_set.paths[index], x=x, y=y, yaw=yaw, draw=draw, scale=scale, pose=pose,
                             table_hit=bool(z + zmin < table_height)))
    return object_count, attempts


def resolve_packed(hit, table_hit, object_count):
    """hit (n, n) bool, symmetric: do attempts i and j collide; table_hit (n,) bool.  Attempt k is kept iff fewer than
    object_count attempts are kept so far, it does not touch the table, and it collides with no kept earlier attempt.  Returns
    the (n,) bool array of kept attempts.  Pure host arithmetic."""
    hit, table_hit = np.asarray(hit, bool), np.asarray(table_hit, bool)
    kept = np.zeros(len(table_hit), bool)
    for k in range(len(table_hit)):
        if kept.sum() >= object_count:
            break
        kept[k] = not table_hit[k] and not (hit[k, :k] & kept[:k]).any()
    return kept


def generate_packed_scenes(object_set, n_scenes, seed=0, first_scene=0, batch=32, device=None, collide=None):
    """Scenes first_scene .. first_scene + n_scenes - 1 of `seed`.  Per batch of scenes: the 12 x batch candidate bodies are built
    with `render.scene_mesh([entry])` -- the very float32 vertices that are rendered later -- the 66 pairs inside each scene are
    tested in one `mesh_collide` call, and `resolve_packed` decides on the host.  Returns per scene the list
    [(mesh_path, scale, pose 4x4)] of the kept objects, the form of get_mesh_pose_list_from_world (utils/implicit.py:33-51).
    collide(meshes, pairs) -> (P,) bool is the decision function (default: `collision.mesh_collide` with containment, on
    `device`).  A scene's result depends on (seed, scene) only, not on `batch` or `first_scene`."""
    if int(batch) < 1:
        raise ValueError("batch must be at least 1")
    if collide is None:
        from . import collision
        collide = lambda meshes, pairs: collision.mesh_collide(meshes, pairs, containment=True, device=device).cpu().numpy()  # noqa: E731
    out = []
    for at in range(0, int(n_scenes), int(batch)):
        ids = range(int(first_scene) + at, int(first_scene) + min(at + int(batch), int(n_scenes)))
        drawn = [packed_candidates(object_set, seed, s) for s in ids]
        bodies = [render.scene_mesh([(*object_set.mesh(a["index"]), a["scale"], a["pose"])]) for _, attempts in drawn for a in attempts]
        pairs = np.concatenate([ATTEMPT_PAIRS + MAX_ATTEMPTS * k for k in range(len(drawn))])
        decided = np.asarray(collide(bodies, pairs), bool).reshape(len(drawn), len(ATTEMPT_PAIRS))
        for (object_count, attempts), row in zip(drawn, decided):
            hit = np.zeros((MAX_ATTEMPTS, MAX_ATTEMPTS), bool)
            hit[ATTEMPT_PAIRS[:, 0], ATTEMPT_PAIRS[:, 1]] = row
            kept = resolve_packed(hit | hit.T, [a["table_hit"] for a in attempts], object_count)
            out.append([(a["path"], a["scale"], a["pose"]) for a, k in zip(attempts, kept) if k])
    return out


def table_mesh(size=0.3, height=TABLE_HEIGHT, extent=0.6):
    """(vertices (4, 3) float32, faces (2, 3) int32): a square of side `extent` centred on the workspace [0, size]^2 at `height`,
    facing up.  It stands for the reference's plane.urdf (placed at (0.15, 0.15, height) with scale 0.6, simulation.py:86-89) in
    the mesh that is RENDERED; it is never part of the mesh list that labels occupancy (the reference's exclude_plane=True)."""
    lo, hi = 0.5 * size - 0.5 * extent, 0.5 * size + 0.5 * extent
    v = np.array([[lo, lo, height], [hi, lo, height], [hi, hi, height], [lo, hi, height]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def scene_id(seed, scene):
    return "packed_%d_%06d" % (int(seed), int(scene))


def write_mesh_pose_list(raw_root, sid, mesh_pose_list):
    """<raw_root>/mesh_pose_list/<sid>.npz, key `pc`: the (n, 3) object array of (mesh_path, scale, pose) that numpy makes of the
    reference's list (scripts/generate_data_parallel.py, io.write_point_cloud): what `geometry.read_mesh_pose_list` loads"""
    path = Path(raw_root) / "mesh_pose_list"
    path.mkdir(parents=True, exist_ok=True)
    pc = np.empty((len(mesh_pose_list), 3), object)
    for k, (mesh_path, scale, pose) in enumerate(mesh_pose_list):
        pc[k, 0], pc[k, 1], pc[k, 2] = str(mesh_path), float(scale), np.asarray(pose, np.float64).reshape(4, 4)
    np.savez_compressed(path / (sid + ".npz"), pc=pc)


def write_geo_dataset(object_set, raw_root, dataset_root, n_scenes, seed=0, first_scene=0, batch=32, n_views=6, num_point_per_file=2048,
                      num_file=4, size=0.3, table_extent=0.6, device=None, collide=None, execute=None, grasps_per_scene=120,
                      num_rotations=6):
    """From object meshes to the files `python -m giga_amd.train_geo` and `python -m giga_amd.eval_geometry` read, without leaving
    the package.  For the packed scenes first_scene .. first_scene + n_scenes - 1 of `seed` (a scene in which nothing was kept is
    left out) it writes
        <raw_root>/mesh_pose_list/<id>.npz   the kept objects (`write_mesh_pose_list`)
        <raw_root>/scenes/<id>.npz           n_views depth images of the objects and the table, and <raw_root>/setup.json with
                                             finger_depth 0.05 and max_opening_width 0.08 added (`render.write_raw_scenes`).  The
                                             camera poses are stored as float64 (the reference stores float32), so that the
                                             fused grids are those of `render.acquire_tsdfs` on the same meshes
        <raw_root>/occ/<id>/%04d.npz         num_file files of num_point_per_file occupancy labels of the objects alone, from a
                                             device generator seeded by (seed, scene) (`render.save_occ`)
        <dataset_root>/                      the fused grids and clouds (`perception.construct_dataset`)
        <raw_root>/grasps.csv                ONE PLACEHOLDER ROW per scene: identity rotation, the workspace centre, width 0,
                                             label 0.
    The placeholder exists because the data sets of `giga_amd.dataset` and `giga_amd.geometry` take their scene list from that
    file.  Such a set feeds `train_geo` and `eval_geometry` WITHOUT `--ROI` only: it holds no grasp labels.
    Returns the scene ids that were written.

    execute: a grasp executor (physics: a simulator or a robot; none is part of this package),
        execute(scene_number, pos (K, 3), quat (K, Y, 4) xyzw, max_opening_width) -> (outcomes (K, Y), widths (K, Y)), numpy.
    With one, grasps.csv holds `grasps_per_scene` labelled rows per scene in place of the placeholder, made the way
    scripts/generate_data_parallel.py makes them (`giga_amd.candidates`): six views drawn by `candidates.scene_views(seed, scene)`
    are rendered and fused at resolution 120, the oriented cloud inside `candidates.workspace_bounds(size, TABLE_HEIGHT)` gives the
    candidates with `num_rotations` yaw angles each, `execute` tries them and `candidates.reduce_outcomes` picks the row.  Every
    other file is written as without an executor.  A scene without an eligible cloud point gets no row (the reference skips such a
    scene), and the return value becomes (scene ids, ids of the scenes without rows)."""
    import torch

    from . import perception
    raw_root, dataset_root = Path(raw_root), Path(dataset_root)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    lists = generate_packed_scenes(object_set, n_scenes, seed, first_scene, batch, dev, collide)
    scenes = [(int(first_scene) + k, mpl) for k, mpl in enumerate(lists) if mpl]
    ids = [scene_id(seed, s) for s, _ in scenes]
    table = table_mesh(size, TABLE_HEIGHT, table_extent)
    rendered = []
    for (s, mpl), sid in zip(scenes, ids):
        write_mesh_pose_list(raw_root, sid, mpl)
        entries, mesh_list = geometry.read_mesh_pose_list(raw_root, sid)
        v, f = render.scene_mesh(entries)
        rendered.append((np.concatenate((v, table[0])), np.concatenate((f, table[1] + len(v)))))
        gen = torch.Generator(device=dev)
        gen.manual_seed(geometry._scene_seed(seed, s))
        render.save_occ(raw_root, sid, mesh_list, num_point_per_file, num_file, generator=gen, device=dev)
    render.write_raw_scenes(raw_root, ids, rendered, n_views, size=size, batch=batch, device=dev, extrinsics_dtype=np.float64)
    with (raw_root / "setup.json").open("r") as fh:
        setup = json.load(fh)
    setup.update({"finger_depth": FINGER_DEPTH, "max_opening_width": MAX_OPENING_WIDTH})
    with (raw_root / "setup.json").open("w") as fh:
        json.dump(setup, fh)
    labelled = None
    if execute is not None:
        labelled = label_packed_scenes([s for s, _ in scenes], rendered, execute, seed=seed, size=size, batch=batch,
                                       grasps_per_scene=grasps_per_scene, num_rotations=num_rotations, device=dev)
    unlabelled = write_grasps_csv(raw_root, ids, labelled, size)
    perception.construct_dataset(raw_root, dataset_root, batch=batch, device=dev)
    return ids if labelled is None else (ids, unlabelled)


def write_grasps_csv(raw_root, ids, labelled=None, size=0.3):
    """<raw_root>/grasps.csv.  labelled None: the placeholder row of `write_geo_dataset` for every scene.  Else one
    `candidates.label_scenes` entry per scene: its rows, or none for an entry that is None; returns the ids of those scenes."""
    from . import candidates
    with open(os.path.join(str(raw_root), "grasps.csv"), "w") as fh:
        fh.write("scene_id,qx,qy,qz,qw,x,y,z,width,label\n")
        for k, sid in enumerate(ids):
            if labelled is None:
                fh.write(",".join([sid] + [repr(float(x)) for x in (0.0, 0.0, 0.0, 1.0, 0.5 * size, 0.5 * size, 0.5 * size, 0.0)] + ["0"]) + "\n")
            elif labelled[k] is not None:
                fh.write("\n".join(candidates.grasp_rows(sid, labelled[k])) + "\n")
    return [] if labelled is None else [sid for sid, rows in zip(ids, labelled) if rows is None]


def label_packed_scenes(scene_numbers, meshes, execute, seed=0, size=0.3, batch=32, grasps_per_scene=120, num_rotations=6, device=None):
    """`candidates.label_scenes` on scene meshes (objects plus table): per batch of scenes the six views of
    `candidates.scene_views(seed, scene)` are rendered in one launch and fused at resolution 120 in another.  Returns one
    `label_scenes` entry per scene."""
    from . import candidates, perception
    intrinsic = render.sim_intrinsic()
    out = []
    for at in range(0, len(meshes), int(batch)):
        numbers = list(scene_numbers[at:at + int(batch)])
        views = [candidates.scene_views(seed, s, size) for s in numbers]
        depth, offs = render.render_depth_batch(meshes[at:at + int(batch)], intrinsic, views, device=device)
        tsdf, weight, _ = perception.fuse_scenes(size, candidates.LABEL_RESOLUTION, [depth[offs[b]:offs[b + 1]] for b in range(len(numbers))],
                                                 intrinsic, views, depth.device)
        out += candidates.label_scenes(tsdf, weight, size, numbers, execute, table_height=TABLE_HEIGHT,
                                       grasps_per_scene=grasps_per_scene, num_rotations=num_rotations, seed=seed,
                                       finger_depth=FINGER_DEPTH, max_opening_width=MAX_OPENING_WIDTH)
    return out
