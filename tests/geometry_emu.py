"""numpy float64 restatements for the geometry scoring (giga_amd.geometry, csrc/giga_geometry.hip): the ROI grasp table and box
points of the reference's DatasetVoxelOccGeoROI.__getitem__ (src/vgn/dataset_voxel_occ.py:96-128), the Philox draws of
giga_roi_points, the occupancy scores of eval_geometry_voxel.py, and the box scenes the GPU tests build in tmp_path."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_emu  # noqa: E402

ROI_STREAM = 0x524F49


# ------------------------------------------------------------------------------------------------------------- the grasp table
def scene_lists(raw_root):
    """(every scene id of grasps.csv in order of first appearance; scene id -> rows with a true label, scenes without one
    dropped, same order)"""
    import pandas as pd
    df = pd.read_csv(os.path.join(str(raw_root), "grasps.csv"))
    everything, positives = [], {}
    for i in range(len(df.index)):
        sid = df.loc[i, "scene_id"]
        if sid not in positives:
            positives[sid] = []
            everything.append(sid)
        if df.loc[i, "label"]:
            positives[sid].append(i)
    return df, everything, {k: v for k, v in positives.items() if len(v) >= 1}


def roi_grasps(df, rows, finger_depth):
    """(R (k,3,3), pos (k,3), width (k,)) float64: the quaternion read as float32, pos = xyz + R (0,0,1) finger_depth"""
    from scipy.spatial.transform import Rotation
    R, pos, width = [], [], []
    for r in rows:
        ori = Rotation.from_quat(df.loc[r, "qx":"qw"].to_numpy(np.single))
        p = df.loc[r, "x":"z"].to_numpy(np.float64)
        p = p + ori.apply(np.array([0, 0, 1])) * finger_depth
        R.append(ori.as_matrix())
        pos.append(p)
        width.append(np.float64(df.loc[r, "width"]))
    return np.array(R), np.array(pos), np.array(width, dtype=float)


def point_counts(widths, n):
    num = n * np.array(widths, dtype=float)
    num = num / np.sum(np.array(widths, dtype=float))
    return np.round(num).astype(int)


# ------------------------------------------------------------------------------------------------------------------ the points
def uniforms(n, seed, scene):
    """(n,3) float64: point j of `scene` draws Philox blocks (j, scene, 0, ROI) and (j, scene, 1, ROI); 53-bit uniforms"""
    j = np.arange(n)
    a = eval_emu.philox4x32_10(j, scene, 0, ROI_STREAM, seed & 0xffffffff, seed >> 32)
    b = eval_emu.philox4x32_10(j, scene, 1, ROI_STREAM, seed & 0xffffffff, seed >> 32)

    def u53(hi, lo):
        k = ((hi.astype(np.uint64) >> np.uint64(5)) << np.uint64(26)) | (lo.astype(np.uint64) >> np.uint64(6))
        return np.where(k != 0, k.astype(np.float64) * 2.0 ** -53, 2.0 ** -54)

    return np.stack([u53(a[0], a[1]), u53(a[2], a[3]), u53(b[0], b[1])], axis=1)


def box_points(u, R, pos, width, finger_depth, roi_scale, size, blas=False):
    """one grasp: uniforms (m,3) -> (world (m,3) float64, normalised (m,3) float32).  blas=True forms the rotation as numpy's
    matrix product does (the reference's expression); otherwise in the kernel's documented order"""
    e = finger_depth * roi_scale
    x, y, z = (u[:, 0] - 1) * e, (u[:, 1] - 0.5) * width, (u[:, 2] - 1) * e
    if blas:
        world = R.dot(np.stack([x, y, z], axis=1).T).T
    else:
        world = (R[None, :, 0] * x[:, None] + R[None, :, 1] * y[:, None]) + R[None, :, 2] * z[:, None]
    world = world + pos
    return world, (world / size - 0.5).astype(np.float32)


def roi_scene(R, pos, width, counts, u, finger_depth, roi_scale, size, blas=False):
    """a scene: its grasps in order, grasp g taking the next counts[g] rows of u"""
    world, norm, at = [], [], 0
    for g, m in enumerate(counts):
        w, nrm = box_points(u[at:at + m], R[g], pos[g], width[g], finger_depth, roi_scale, size, blas)
        world.append(w)
        norm.append(nrm)
        at += m
    return np.concatenate(world), np.concatenate(norm)


def local_coordinates(world, R, pos):
    """world points of one grasp back in its frame: R^T (world - pos)"""
    return (world - pos) @ R


# ------------------------------------------------------------------------------------------------------------------ the scores
def confusion(pred, target):
    pred, target = np.asarray(pred, bool), np.asarray(target, bool)
    return np.array([(pred & target).sum(), (pred & ~target).sum(), (~pred & target).sum(), (~pred & ~target).sum()], np.int64)


def reference_scores(occ_pred, occ, ext=""):
    """eval.py (eval_occ) / eval_geometry_voxel.py:158-161 and common.compute_iou"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"iou" + ext: eval_emu.compute_iou(occ_pred, occ),
                "precision" + ext: 1.0 * np.sum(np.logical_and(occ_pred, occ)) / np.sum(occ_pred),
                "recall" + ext: 1.0 * np.sum(np.logical_and(occ_pred, occ)) / np.sum(occ)}


def same_number(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and ((np.isnan(a) and np.isnan(b)) or a == b)


# ------------------------------------------------------------------------------------------------------------------ box scenes
BOX_FACES = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6], [1, 2, 6], [1, 6, 5],
                      [0, 4, 7], [0, 7, 3]])


def unit_box():
    """the cube [-0.5, 0.5]^3, outward faces"""
    v = np.array([[-.5, -.5, -.5], [.5, -.5, -.5], [.5, .5, -.5], [-.5, .5, -.5], [-.5, -.5, .5], [.5, -.5, .5], [.5, .5, .5],
                  [-.5, .5, .5]])
    return v, BOX_FACES.copy()


def write_obj(path, v, f, quads=False):
    with open(path, "w") as fh:
        fh.write("# a box\n")
        for p in v:
            fh.write("v %r %r %r\n" % tuple(float(x) for x in p))
        if quads:                        # the six sides as quadrilaterals, the a/b/c form, relative indices on one of them
            for q in ([0, 3, 2, 1], [4, 5, 6, 7], [0, 1, 5, 4], [2, 3, 7, 6], [1, 2, 6, 5]):
                fh.write("f " + " ".join("%d/1/1" % (k + 1) for k in q) + "\n")
            fh.write("f " + " ".join("%d//1" % (k - len(v)) for k in [0, 4, 7, 3]) + "\n")
        else:
            for t in f:
                fh.write("f %d %d %d\n" % tuple(int(k) + 1 for k in t))


# (centre, edge lengths) of the boxes of three scenes, on the floor of the 0.3 workspace; and the successful grasps (x, y, z,
# width) placed so that the box below the finger tips cuts through the objects
BOX_SCENES = [
    [((0.10, 0.10, 0.05), (0.06, 0.08, 0.10)), ((0.20, 0.18, 0.04), (0.08, 0.05, 0.08))],
    [((0.08, 0.20, 0.03), (0.05, 0.05, 0.06)), ((0.15, 0.12, 0.06), (0.07, 0.06, 0.12)), ((0.23, 0.07, 0.035), (0.05, 0.09, 0.07))],
    [((0.15, 0.15, 0.045), (0.10, 0.10, 0.09)), ((0.07, 0.07, 0.025), (0.04, 0.06, 0.05))],
]
BOX_GRASPS = [
    [(0.105, 0.12, 0.06, 0.07), (0.20, 0.19, 0.05, 0.06)],
    [(0.15, 0.125, 0.09, 0.08), (0.083, 0.20, 0.07, 0.06), (0.23, 0.075, 0.04, 0.06)],
    [(0.21, 0.15, 0.06, 0.08)],
]


def write_box_set(root, raw_root, grids, size=0.3, finger_depth=0.05):
    """The reference's on-disk layout for the three box scenes: <root>/scenes/<id>.npz (grids[b] (40,40,40)), <raw_root>/
    grasps.csv (the failures first, in reverse scene order, then the successful grasps, which point along -z), setup.json,
    mesh_pose_list/<id>.npz with (mesh_path, scale, pose) per box (one .obj with quads, one through a one-link .urdf).  Returns the
    scene ids in BOX_SCENES order; scene id "boxNN" is BOX_SCENES[NN]."""
    os.makedirs(os.path.join(root, "scenes"), exist_ok=True)
    os.makedirs(os.path.join(raw_root, "mesh_pose_list"), exist_ok=True)
    v, f = unit_box()
    write_obj(os.path.join(raw_root, "box_tri.obj"), v, f)
    write_obj(os.path.join(raw_root, "box_quad.obj"), v, f, quads=True)
    with open(os.path.join(raw_root, "box.urdf"), "w") as fh:
        fh.write('<?xml version="1.0"?>\n<robot name="box"><link name="base"><visual><geometry><mesh filename="box_tri.obj" '
                 'scale="1 1 1"/></geometry></visual></link></robot>\n')
    files = ["box_tri.obj", "box_quad.obj", "box.urdf"]
    ids = ["box%02d" % b for b in range(len(BOX_SCENES))]
    rows = []
    for b, boxes in enumerate(BOX_SCENES):
        pc = np.empty(len(boxes), dtype=object)
        for k, (centre, edges) in enumerate(boxes):
            pose = np.eye(4)
            pose[:3, 3] = centre
            pc[k] = (os.path.join(raw_root, files[(b + k) % 3]), np.array(edges, np.float64), pose)
        np.savez(os.path.join(raw_root, "mesh_pose_list", ids[b] + ".npz"), pc=pc)
        np.savez_compressed(os.path.join(root, "scenes", ids[b] + ".npz"), grid=np.asarray(grids[b], np.float32)[None])
        for (x, y, z, w) in BOX_GRASPS[b]:
            rows.append((ids[b], 1.0, 0.0, 0.0, 0.0, x, y, z, w, 1))                  # a half turn about x: the approach is -z
            rows.append((ids[b], 0.0, 0.0, 0.0, 1.0, x, y, z + 0.1, w, 0))
    rows = rows[1::2][::-1] + rows[0::2]          # the failures first and backwards: the scenes appear as box02, box01, box00
    with open(os.path.join(raw_root, "grasps.csv"), "w") as fh:
        fh.write("scene_id,qx,qy,qz,qw,x,y,z,width,label\n")
        for r in rows:
            fh.write(",".join([r[0]] + [repr(float(x)) for x in r[1:9]] + [str(r[9])]) + "\n")
    with open(os.path.join(raw_root, "setup.json"), "w") as fh:
        json.dump({"size": size, "intrinsic": {"width": 640, "height": 480, "K": [540.0, 0.0, 320.0, 0.0, 540.0, 240.0, 0.0, 0.0, 1.0]},
                   "max_opening_width": 0.08, "finger_depth": finger_depth}, fh)
    return ids


def box_scene_mesh(b):
    """the world-coordinate mesh of box scene b (float64 vertices, faces), for rendering its grid"""
    v0, f0 = unit_box()
    vs, fs, base = [], [], 0
    for centre, edges in BOX_SCENES[b]:
        vs.append(v0 * np.array(edges) + np.array(centre))
        fs.append(f0 + base)
        base += len(v0)
    return np.concatenate(vs), np.concatenate(fs)


def inside_boxes(b, points):
    """(inside any box of scene b, distance to the nearest face plane of any box) for world points; the planes are where the
    float32 vertices of the scene mesh lie"""
    inside, dist = np.zeros(len(points), bool), np.full(len(points), np.inf)
    v0 = unit_box()[0]
    for centre, edges in BOX_SCENES[b]:
        v = (v0 * np.array(edges) + np.array(centre)).astype(np.float32).astype(np.float64)
        lo, hi = v.min(axis=0), v.max(axis=0)
        inside |= ((points > lo) & (points < hi)).all(axis=1)
        dist = np.minimum(dist, np.minimum(np.abs(points - lo), np.abs(points - hi)).min(axis=1))
    return inside, dist
