"""Grasp candidates from the fused TSDF: the geometry of the reference's label generator (scripts/generate_data_parallel.py)
around its physics step.

    points, normals, offsets = perception.cloud_batch(tsdf, weight, size, normals=True)          # the oriented cloud
    lower, upper = workspace_bounds(size, table_height)
    pos, quat, index, counts = grasp_candidates(points, normals, offsets, 120, lower=lower, upper=upper)
    outcomes, widths = my_executor(...)                                  # physics: PyBullet, another simulator, a robot
    quat1, width, label = reduce_outcomes(outcomes, widths, quat_b)      # the row generate_data_parallel.py writes

`grasp_candidates` is `sample_grasp_point` (:133-144) and the frame and yaw angles of `evaluate_grasp_point` (:147-161) for a
ragged batch of scenes in one launch (`giga_grasp_candidates`, include/giga_hip.h); `reduce_outcomes` is :168-179 on the host,
where the outcomes of an executor arrive.  The executor itself -- contact, settling, the gripper -- is not part of this package."""
import numpy as np
import torch

from . import _capi

VIEW_STREAM = 0x47525350                       # third word of the view generator's seed (the device draws' counter word, "GRSP")
LABEL_RESOLUTION = 120                         # generate_data_parallel.py:56
N_VIEWS = 6                                    # MAX_VIEWPOINT_COUNT


def workspace_bounds(size, table_height):
    """(lower, upper): the volume grasps are sampled in (simulation.py:92-96)."""
    size, height = float(size), float(table_height)
    return np.r_[0.02, 0.02, height + 0.005], np.r_[size - 0.02, size - 0.02, size]


def yaw_table(num_rotations):
    """(Y, 2) float64: (sin(yaw / 2), cos(yaw / 2)) of the reference's angles np.linspace(0, pi, Y)."""
    Y = int(num_rotations)
    if not 1 <= Y <= _capi.CANDIDATES_MAX_ROTATIONS:
        raise ValueError(f"num_rotations outside 1 .. {_capi.CANDIDATES_MAX_ROTATIONS}")
    yaws = np.linspace(0.0, np.pi, Y)
    return np.ascontiguousarray(np.stack((np.sin(yaws / 2.0), np.cos(yaws / 2.0)), axis=1))


def grasp_candidates(points, normals, offsets, per_scene, *, lower, upper, finger_depth=0.05, eps=0.1, num_rotations=6, seed=0,
                     scene_ids=None):
    """`per_scene` candidates for each scene of an oriented cloud.  points, normals (n, 3) float32 device tensors, scenes back to
    back; offsets B + 1 ints (what `perception.cloud_batch(..., normals=True)` returns); scene_ids B ints below 2^32 (default
    0 .. B - 1): a scene's draws depend on (seed, its id) and its own cloud alone.
    Returns device tensors (pos (B, K, 3) float64, quat (B, K, Y, 4) float64 xyzw, index (B, K) int32 -- the drawn point inside
    its scene --, counts (B,) int32 -- the scene's eligible points).  A scene with count 0 has no candidates: its rows are zeros.
    Asynchronous on the current stream."""
    dev = _capi.device_of(points, normals)
    offs = np.ascontiguousarray(offsets, np.int32)
    B, K = len(offs) - 1, int(per_scene)
    if B < 0 or K < 0:
        raise ValueError("offsets has B + 1 entries and per_scene is not negative")
    n = int(offs[-1])
    for t in (points, normals):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (n, 3):
            raise ValueError("points and normals are contiguous float32 (n, 3) tensors with n = offsets[-1]")
    ids = np.arange(B, dtype=np.int64) if scene_ids is None else np.asarray(scene_ids, np.int64).reshape(-1)
    if len(ids) != B or (B and (ids.min() < 0 or ids.max() >= 1 << 32)):
        raise ValueError("scene_ids: one id in [0, 2^32) per scene")
    ids = np.ascontiguousarray(ids.astype(np.uint32))
    table = yaw_table(num_rotations)
    Y = len(table)
    lower, upper = (np.ascontiguousarray(np.asarray(a, np.float64).reshape(3)) for a in (lower, upper))
    pos = torch.zeros((B, K, 3), dtype=torch.float64, device=dev)
    quat = torch.zeros((B, K, Y, 4), dtype=torch.float64, device=dev)
    index = torch.zeros((B, K), dtype=torch.int32, device=dev)
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    if B == 0 or K == 0:
        return pos, quat, index, counts
    ws = _capi.workspace("giga_grasp_candidates", dev, B, n, Y)
    _capi.call("giga_grasp_candidates", dev, points if n else None, normals if n else None, offs, ids, B, K, lower, upper,
               float(finger_depth), float(eps), table, Y, int(seed) & 0xFFFFFFFFFFFFFFFF, pos, quat, index, counts, ws, ws.numel())
    return pos, quat, index, counts


def reduce_outcomes(outcomes, widths, quat):
    """generate_data_parallel.py:168-179 for K candidates at once, on the host.  outcomes (K, Y) (1 = success), widths (K, Y),
    quat (K, Y, 4).  Returns (quat (K, 4), width (K,), label (K,) int64).  A candidate with a success gets the yaw in the middle
    (rounded down) of its longest run of successes, the first such run on ties -- what find_peaks(x=[0, s, 0], height=1, width=1)
    followed by argmax(widths) selects -- and the label max(outcomes).  A candidate without one gets the LAST yaw's quaternion and
    width (the values the reference's loop variables hold there) and the label 0."""
    outcomes, widths, quat = np.asarray(outcomes), np.asarray(widths, np.float64), np.asarray(quat, np.float64)
    K, Y = outcomes.shape
    if widths.shape != (K, Y) or quat.shape != (K, Y, 4) or Y < 1:
        raise ValueError("outcomes and widths are (K, Y), quat is (K, Y, 4), Y >= 1")
    s = outcomes == 1
    run = np.zeros(K, np.int64)                 # length of the run of successes that ends at the yaw before j
    best_len = np.zeros(K, np.int64)
    best_mid = np.full(K, Y - 1, np.int64)
    for j in range(Y):
        run = np.where(s[:, j], run + 1, 0)
        ends = s[:, j] & (~s[:, j + 1] if j + 1 < Y else True)
        better = ends & (run > best_len)        # strictly longer: the first of equal runs stays
        best_mid = np.where(better, (2 * j - run + 1) // 2, best_mid)
        best_len = np.where(better, run, best_len)
    rows = np.arange(K)
    return quat[rows, best_mid], widths[rows, best_mid], outcomes.max(axis=1).astype(np.int64)


def scene_views(seed, scene, size=0.3, n=N_VIEWS):
    """(n, 4, 4) extrinsics with the distributions of the reference's render_images (generate_data_parallel.py:87-105): per view
    r in U(1.6, 2.4) size, theta in U(0, pi / 4), phi in U(0, 2 pi), about (size / 2, size / 2, 0), drawn in that order from
    np.random.default_rng([seed, scene, 0x47525350]): the views depend on (seed, scene) alone."""
    from .perception import camera_on_sphere
    rng = np.random.default_rng([int(seed), int(scene), VIEW_STREAM])
    origin = np.eye(4)
    origin[:3, 3] = [size / 2, size / 2, 0.0]
    views = []
    for _ in range(int(n)):
        r = rng.uniform(1.6, 2.4) * size
        theta = rng.uniform(0.0, np.pi / 4.0)
        phi = rng.uniform(0.0, 2.0 * np.pi)
        views.append(camera_on_sphere(origin, r, theta, phi))
    return np.stack(views).reshape(-1, 4, 4)


def label_scenes(tsdf, weight, size, scene_numbers, execute, *, table_height=0.05, grasps_per_scene=120, num_rotations=6, seed=0,
                 finger_depth=0.05, eps=0.1, max_opening_width=0.08):
    """Grasp rows of B fused volumes (tsdf, weight (B, R, R, R) float32 device tensors, `perception.fuse_scenes`): the oriented
    cloud, the candidates inside `workspace_bounds(size, table_height)`, then per scene
        execute(scene_number, pos (K, 3), quat (K, Y, 4), max_opening_width) -> (outcomes (K, Y), widths (K, Y))
    (numpy in, numpy out; outcome 1 = success) and `reduce_outcomes`.  scene_numbers[b] is handed to `execute` and is the id of
    the scene's draws.  Returns per scene (pos (K, 3), quat (K, 4), width (K,), label (K,)) or None for a scene without an
    eligible point (the reference skips such a scene)."""
    from . import perception
    B = tsdf.shape[0]
    if len(scene_numbers) != B:
        raise ValueError("one scene number per volume")
    points, normals, offsets = perception.cloud_batch(tsdf, weight, size, normals=True)
    lower, upper = workspace_bounds(size, table_height)
    pos, quat, _, counts = grasp_candidates(points, normals, offsets, grasps_per_scene, lower=lower, upper=upper,
                                            finger_depth=finger_depth, eps=eps, num_rotations=num_rotations, seed=seed,
                                            scene_ids=scene_numbers)
    pos, quat, counts = pos.cpu().numpy(), quat.cpu().numpy(), counts.cpu().numpy()
    out = []
    for b, number in enumerate(scene_numbers):
        if counts[b] == 0:
            out.append(None)
            continue
        outcomes, widths = execute(int(number), pos[b], quat[b], float(max_opening_width))
        q, w, label = reduce_outcomes(outcomes, widths, quat[b])
        out.append((pos[b], q, w, label))
    return out


def grasp_rows(scene_id, labelled):
    """The grasps.csv lines `scene_id,qx,qy,qz,qw,x,y,z,width,label` of one `label_scenes` entry (io.write_grasp's columns)."""
    pos, quat, width, label = labelled
    return [",".join([str(scene_id)] + [repr(float(x)) for x in (*quat[k], *pos[k], width[k])] + [str(int(label[k]))])
            for k in range(len(pos))]


def resolve_executor(spec):
    """The callable named `module:function` (the command line's --executor)."""
    import importlib
    module, _, name = str(spec).partition(":")
    if not module or not name:
        raise ValueError("an executor is named module:function")
    return getattr(importlib.import_module(module), name)
