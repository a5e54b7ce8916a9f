"""numpy restatement of the resident training set's two stages (csrc/giga_batch.hip; semantics in include/giga_hip.h,
giga_batch_draw and giga_batch_assemble): the Philox draws of an item, the keyed bijection behind the occupancy sample, and the
assembly of an item from forced draws.  Shared by tests/test_resident_host.py (against the host reader) and
tests/test_gpu_resident.py (against the kernels)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eval_emu import philox4x32_10  # noqa: E402

STREAM_ITEM, STREAM_OCC = 0, 1
FEISTEL_ROUNDS = 8                       # GIGA_BATCH_FEISTEL_ROUNDS
RES = 40                                 # GIGA_BATCH_RES
# sin and cos of q pi / 4, q = 0..3: the half angles of the quarter turns (the header's constants)
SIN_Q = (0.0, 0.7071067811865475, 1.0, 0.7071067811865476)
COS_Q = (1.0, 0.7071067811865476, 6.123233995736766e-17, -0.7071067811865475)
U32 = np.uint32
M32 = np.uint64(0xffffffff)


# -------------------------------------------------------------------------------------------------------------------- draws
def blocks(block, ordinal, epoch, stream, seed):
    """the four words of the Philox blocks (block, ordinal, epoch, stream) under the key `seed`; arguments broadcast"""
    return philox4x32_10(np.asarray(block, np.uint64), np.asarray(ordinal, np.uint64), np.asarray(epoch, np.uint64), stream,
                         int(seed) & 0xffffffff, int(seed) >> 32)


def mulhi(word, n):
    return ((np.asarray(word, np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def item_draws(ordinal, epoch, seed, n_files):
    """quarter, u, file of one item or an array of items (n_files broadcasts)"""
    x = blocks(0, ordinal, epoch, STREAM_ITEM, seed)
    quarter = (x[0] >> U32(30)).astype(np.int32)
    u = 6.0 + 28.0 * (x[1].astype(np.float64) * 2.0 ** -32)
    file = ((x[3].astype(np.uint64) * np.asarray(n_files, np.uint64)) >> np.uint64(32)).astype(np.int32)
    return quarter, u, file


def fmix32(h):
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & M32
    h ^= h >> np.uint64(16)
    return h


def feistel_bits(n):
    """the even width of the Feistel domain: the smallest b >= 2, b even, with 2^b >= n"""
    b = max(int(n - 1).bit_length(), 2)
    return b + (b & 1)


def permute(m, n, keys, rounds=FEISTEL_ROUNDS, walks=None):
    """pi(m) for an array m of positions in [0, n): the balanced Feistel network on feistel_bits(n) bits, walked until the value
    is below n.  keys: four uint32 words or arrays of them that broadcast against m.  walks (a list) receives the longest walk."""
    m, k0, k1, k2, k3 = np.broadcast_arrays(np.asarray(m, np.uint64), *[np.asarray(k, np.uint64) for k in keys])
    if n == 1:
        return np.zeros(m.shape, np.int64)
    b = feistel_bits(n)
    h = np.uint64(b // 2)
    mask = np.uint64((1 << (b // 2)) - 1)
    rk = [((k0, k1, k2, k3)[r & 3] + np.uint64(r * 0x9E3779B9)) & M32 for r in range(rounds)]
    v = m.copy()
    todo = np.ones(m.shape, bool)
    bound = (1 << b) - n + 1                 # a walk leaves [n, 2^b) after at most this many applications
    it = 0
    while todo.any():
        assert it < bound
        L, R = v[todo] >> h, v[todo] & mask
        for r in range(rounds):
            L, R = R, L ^ (fmix32(R ^ rk[r][todo]) & mask)
        v[todo] = (L << h) | R
        todo &= v >= np.uint64(n)
        it += 1
    if walks is not None:
        walks.append(it)
    return v.astype(np.int64)


def occ_indices(ordinal, epoch, seed, n, M, rounds=FEISTEL_ROUNDS, walks=None):
    """the M occupancy indices into a file of n points: (M,) int32 for one item, (T, M) for an array of T ordinals"""
    o = np.asarray(ordinal, np.uint64)
    m = np.arange(M)
    if M > n:
        w = np.stack(blocks(m >> 2, o[..., None], epoch, STREAM_OCC, seed), axis=-1)     # (.., M, 4): block m >> 2, word m & 3
        return mulhi(np.take_along_axis(w, np.broadcast_to(m & 3, w.shape[:-1])[..., None], axis=-1)[..., 0], n).astype(np.int32)
    keys = [k[..., None] for k in blocks(0, o, epoch, STREAM_OCC, seed)]
    return permute(m, n, keys, rounds, walks).astype(np.int32)


def draw(ordinals, epoch, seed, n_files, n_points, M):
    """the draws of a batch: n_files[b] files of item b's scene, n_points(b, file) points of its drawn file"""
    ordinals = np.asarray(ordinals, np.int64)
    quarter, u, file = item_draws(ordinals, epoch, seed, n_files)
    n = np.array([n_points(b, int(file[b])) for b in range(len(ordinals))], np.int64)
    index = np.zeros((len(ordinals), M), np.int32)
    for size in np.unique(n):
        index[n == size] = occ_indices(ordinals[n == size], epoch, seed, int(size), M)
    return quarter, u, file, index


# ----------------------------------------------------------------------------------------------------------------- assembly
def source_rows(q):
    """source (s_i, s_j) of output (i, j) under quarter turn q, as (40, 40) integer arrays (values 0..40: 40 is outside)"""
    i, j = np.meshgrid(np.arange(RES), np.arange(RES), indexing="ij")
    return ((i, j), (j, RES - i), (RES - i, RES - j), (RES - j, i))[q]


def transform_grid(grid, q, z_off):
    """(40, 40, 40) float32 -> the augmented grid and the mask of voxels whose source lies in range"""
    si, sj = source_rows(q)
    c = np.arange(RES, dtype=np.float64) - np.float64(z_off)
    sk = np.floor(c + 0.5)
    ok_k = (c >= 0.0) & (c <= RES - 1.0)
    ok_ij = (si >= 0) & (si <= RES - 1) & (sj >= 0) & (sj <= RES - 1)
    ok = ok_ij[:, :, None] & ok_k[None, None, :]
    src = grid[np.clip(si, 0, RES - 1)[:, :, None], np.clip(sj, 0, RES - 1)[:, :, None],
               np.where(ok_k, sk, 0).astype(np.int64)[None, None, :]]
    return np.where(ok, src, np.float32(0)).astype(np.float32), ok


def border_set(q):
    """(40, 40) mask of the output rows whose source x or y index is exactly 0 or 39 under q != 0: where scipy's in-range test
    hangs on the rounding noise of its rotation matrix"""
    if q == 0:
        return np.zeros((RES, RES), bool)
    si, sj = source_rows(q)
    return (si == 0) | (si == RES - 1) | (sj == 0) | (sj == RES - 1)


def pose(pos_metric, quat, q, z_off, size):
    """augmented pose: pos (3,) float32, rot (2, 4) float32; every operation one rounding in double, one rounding to float32"""
    p = np.asarray(pos_metric, np.float32).astype(np.float64)
    dx, dy = p[0] - 20.0, p[1] - 20.0
    rx, ry = ((dx, dy), (-dy, dx), (-dx, -dy), (dy, -dx))[q]
    out = np.array([rx + 20.0, ry + 20.0, p[2] + np.float64(z_off)], np.float64)
    pos = (out / np.float64(size) - 0.5).astype(np.float32)
    b = np.asarray(quat, np.float32).astype(np.float64)
    norm = np.sqrt(((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]) + b[3] * b[3])
    b = b / norm
    s, c = np.float64(SIN_Q[q]), np.float64(COS_Q[q])
    r0 = np.array([c * b[0] - s * b[1], c * b[1] + s * b[0], c * b[2] + s * b[3], c * b[3] - s * b[2]], np.float64)
    r1 = np.array([r0[1], -r0[0], r0[3], -r0[2]], np.float64)
    return pos, np.stack([r0, r1]).astype(np.float32)


def occupancy(points, occ, index, size):
    """pos_occ (M, 3) float32 and occ (M,) float32 of one file: numpy's own arithmetic in the file's dtype"""
    idx = np.asarray(index, np.int64)
    return (points[idx] / size - 0.5).astype(np.float32), np.asarray(occ)[idx].astype(np.float32)


def assemble_item(grid, pos_metric, quat, rotations, width_metric, label, points, occ, size, q, u, index, augment, z_off=None):
    """one item from forced draws.  z_off overrides u - pos_z (the tests' exact shifts).  Returns x, pos (3,), pos_occ, (label,
    rot (2, 4), width, occ) as float32, and the in-range mask of x (None without augmentation)."""
    pos_metric = np.asarray(pos_metric, np.float32)
    width = np.float32(width_metric) / np.float32(size)
    pocc, o = occupancy(points, occ, index, size)
    if not augment:
        pos = pos_metric / np.float32(size) - np.float32(0.5)
        return grid.astype(np.float32), pos, pocc, (np.float32(label), np.asarray(rotations, np.float32), width, o), None
    if z_off is None:
        z_off = np.float64(u) - np.float64(pos_metric[2])
    x, ok = transform_grid(grid, int(q), z_off)
    pos, rot = pose(pos_metric, quat, int(q), z_off, size)
    return x, pos, pocc, (np.float32(label), rot, width, o), ok


def file_range(tables, row, file):
    """[first, first + n) of the points of file `file` of the scene of grasp row `row`"""
    f = int(tables["scene_files"][int(tables["row_scene"][row])]) + int(file)
    return int(tables["file_points"][f]), int(tables["file_points"][f + 1])


def files_of(tables, rows):
    s = tables["row_scene"][np.asarray(rows, np.int64)]
    return (tables["scene_files"][s + 1] - tables["scene_files"][s]).astype(np.int64)


def draw_batch(tables, ordinals, epoch, seed, rows, M):
    """`draw` on the host tables of a set (giga_amd.resident.host_tables)"""
    def n_points(b, file):
        lo, hi = file_range(tables, rows[b], file)
        return hi - lo
    return draw(ordinals, epoch, seed, files_of(tables, rows), n_points, M)


def assemble_batch(tables, size, rows, draws, M, augment, z_offs=None):
    """the batch of grasp rows `rows` under forced draws, in the shapes giga_batch_assemble writes; also the in-range masks"""
    quarter, u, file, index = draws
    items = []
    for b, r in enumerate(rows):
        lo, hi = file_range(tables, r, file[b])
        items.append(assemble_item(tables["grids"][tables["row_scene"][r]], tables["row_pos"][r], tables["row_quat"][r],
                                   tables["row_rotations"][r], tables["row_width"][r], tables["row_label"][r], tables["points"][lo:hi],
                                   tables["occ"][lo:hi], size, quarter[b], u[b], np.asarray(index[b]).reshape(M), augment,
                                   None if z_offs is None else z_offs[b]))
    stack = lambda f, shape: np.stack([f(it) for it in items]).astype(np.float32).reshape(shape)  # noqa: E731
    B = len(rows)
    return (stack(lambda it: it[0], (B, RES, RES, RES)), stack(lambda it: it[1], (B, 1, 3)), stack(lambda it: it[2], (B, M, 3)),
            (stack(lambda it: it[3][0], (B,)), stack(lambda it: it[3][1], (B, 2, 4)), stack(lambda it: it[3][2], (B,)),
             stack(lambda it: it[3][3], (B, M)))), [it[4] for it in items]


# --------------------------------------------------------------------------------------------------------------- tiny sets
FILE_SIZES = (300, 1, 5, 2049)           # the sizes of the tiny sets' occupancy files, in turn
SAMPLER_SIZES = (1, 2, 3, 5, 64, 65, 97, 2047, 2048, 2049)


def resize_occ_files(raw_root, dtype=np.float32, sizes=FILE_SIZES, seed=0, size=0.3):
    """rewrite the occupancy files under raw_root/occ so that their sizes run through `sizes`, with points of `dtype`"""
    rng = np.random.default_rng([707, seed])
    k = 0
    for d in sorted(os.listdir(os.path.join(raw_root, "occ"))):
        for f in sorted(os.listdir(os.path.join(raw_root, "occ", d))):
            n = sizes[k % len(sizes)]
            k += 1
            np.savez(os.path.join(raw_root, "occ", d, f), points=(rng.random((n, 3)) * size).astype(dtype), occ=rng.random(n) < 0.3)
    return k


def write_set(root, raw_root, file_sizes, dtype, grasps_per_scene=5, seed=0, size=0.3, res=RES):
    """a training set in the reference's layout written here: scene s has one occupancy file per entry of file_sizes[s], points of
    `dtype`; every fourth grasp has a z that is a multiple of 1/8, so that u = z_off + z reaches exact shifts"""
    rng = np.random.default_rng([808, seed])
    os.makedirs(os.path.join(root, "scenes"), exist_ok=True)
    os.makedirs(raw_root, exist_ok=True)
    lines = []
    for s, sizes in enumerate(file_sizes):
        sid = f"w{seed:02d}_{s:04d}"
        np.savez_compressed(os.path.join(root, "scenes", sid + ".npz"), grid=rng.random((1, res, res, res), dtype=np.float32))
        os.makedirs(os.path.join(raw_root, "occ", sid), exist_ok=True)
        for f, n in enumerate(sizes):
            np.savez(os.path.join(raw_root, "occ", sid, f"{f:04d}.npz"), points=(rng.random((n, 3)) * size).astype(dtype),
                     occ=rng.random(n) < 0.3)
        for g in range(grasps_per_scene):
            q = rng.normal(size=4)
            q /= np.linalg.norm(q)
            p = rng.random(3) * size
            if g % 4 == 0:
                p[2] = int(rng.integers(0, 3)) / 8.0
            lines.append(",".join([sid] + [repr(float(v)) for v in (*q, *p, rng.uniform(0.02, 0.08))] + [str(int(rng.random() < 0.5))]))
    with open(os.path.join(raw_root, "grasps.csv"), "w") as f:
        f.write("scene_id,qx,qy,qz,qw,x,y,z,width,label\n")
        for i in rng.permutation(len(lines)):
            f.write(lines[i] + "\n")
    with open(os.path.join(raw_root, "setup.json"), "w") as f:
        json.dump({"size": size}, f)
    return len(lines)


def tiny_sets(base):
    """the tests' sets under directory `base` -> {name: (root, raw_root)}: "f32" synth.write_training_set's six scenes with 1-3
    float32 files each, resized to FILE_SIZES; "f16" six scenes with 1-3 float16 files of the same sizes; "sizes" one float32 file
    of every size in SAMPLER_SIZES, one scene each"""
    from giga_amd import synth
    out = {}
    for name in ("f32", "f16", "sizes"):
        out[name] = (os.path.join(base, name, "data"), os.path.join(base, name, "raw"))
    synth.write_training_set(*out["f32"], n_scenes=6, grasps_per_scene=5, occ_files=(1, 3), n_occ_points=300, seed=3)
    resize_occ_files(out["f32"][1])
    counts, k, sizes = (1, 3, 2, 1, 2, 3), 0, []
    for c in counts:
        sizes.append([FILE_SIZES[(k + i) % len(FILE_SIZES)] for i in range(c)])
        k += c
    write_set(*out["f16"], sizes, np.float16, grasps_per_scene=7, seed=1)
    write_set(*out["sizes"], [[n] for n in SAMPLER_SIZES], np.float32, grasps_per_scene=4, seed=2)
    return out


def ulp32(x):
    """the spacing of float32 at |x| (of the smallest normal below it)"""
    x = np.maximum(np.abs(np.asarray(x, np.float32)), np.float32(2.0 ** -126))
    return np.spacing(x).astype(np.float64)
