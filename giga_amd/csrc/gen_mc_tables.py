"""Generate the 256-case marching-cubes tables of giga_mesh.hip:  python giga_amd/csrc/gen_mc_tables.py [--check]

Nothing here is copied from a published table: every case is derived from the cube's geometry.

Numbering (the customary one): corner m sits at CORNERS[m]; edge e joins EDGES[e]; bit m of the case index is set when
the value at corner m is <= iso.

Per case:
  1. every cube face is cut into directed segments between its crossed edges.  Seen from outside the cube with the face's
     corners counter-clockwise, every maximal run of set corners gets ONE segment, from the crossed edge that ends the run
     to the crossed edge that begins it: the set corners lie to the segment's left.  A face with two diagonal set corners
     therefore gets two segments that cut each set corner off on its own.  The rule reads only the face's four bits, so the
     two cells that share a face draw the same segments (in opposite directions), and the surface has no cracks;
  2. every crossed edge is the head of one segment and the tail of one other: the segments chain into closed loops;
  3. a loop is fan-triangulated from the first apex (in loop order) for which no fan diagonal joins two points of one cube
     face (such a diagonal could coincide with a segment or a diagonal of the neighbouring cell and make an edge with four
     triangles); the triangles keep the loop's direction;
  4. FLIP reverses every triangle: it is the one global choice, set so that the normals point towards the set corners
     (values <= iso), the orientation of the reference implementation this package is compared with.
"""
import math
import os
import sys

CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
FLIP = False
MAX_TRIS = 5
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "giga_mc_tables.h")


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def faces():
    """The six faces as 4 corner numbers, counter-clockwise seen from outside.  Order: -x, +x, -y, +y, -z, +z."""
    out = []
    for axis in range(3):
        for side in (0, 1):
            cs = [m for m, c in enumerate(CORNERS) if c[axis] == side]
            u, v = [a for a in range(3) if a != axis]
            cs.sort(key=lambda m: math.atan2(CORNERS[m][v] - 0.5, CORNERS[m][u] - 0.5))
            # make it counter-clockwise about the outward normal
            a, b, c = (CORNERS[cs[0]], CORNERS[cs[1]], CORNERS[cs[2]])
            n = _cross([b[i] - a[i] for i in range(3)], [c[i] - b[i] for i in range(3)])
            if (n[axis] > 0) != (side == 1):
                cs.reverse()
            out.append(tuple(cs))
    return tuple(out)


FACES = faces()
EDGE_OF = {frozenset(e): i for i, e in enumerate(EDGES)}


def face_edges(face):
    return tuple(EDGE_OF[frozenset((face[i], face[(i + 1) % 4]))] for i in range(4))


def face_segments(face, case):
    """Directed segments (edge_from, edge_to) of one face for a case index (rule 1 of the module docstring)."""
    bits = [(case >> m) & 1 for m in face]
    if sum(bits) in (0, 4):
        return []
    fe = face_edges(face)
    segs = []
    for i in range(4):
        if bits[i] and not bits[(i - 1) % 4]:           # a run of set corners begins at i (edge i-1 is crossed)
            j = i
            while bits[(j + 1) % 4]:
                j = (j + 1) % 4
            segs.append((fe[j], fe[(i - 1) % 4]))        # from the edge that ends the run to the edge that begins it
    return segs


def crossed_edges(case):
    return [e for e, (a, b) in enumerate(EDGES) if ((case >> a) ^ (case >> b)) & 1]


def _on_one_face(e1, e2):
    for f in FACES:
        fe = face_edges(f)
        if e1 in fe and e2 in fe:
            return True
    return False


def loops(case):
    nxt = {}
    for f in FACES:
        for a, b in face_segments(f, case):
            assert a not in nxt
            nxt[a] = b
    assert sorted(nxt) == crossed_edges(case) and sorted(nxt.values()) == sorted(nxt)
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3
        out.append(loop)
    return out


def triangulate(loop):
    n = len(loop)
    for apex in range(n):
        r = loop[apex:] + loop[:apex]
        if all(not _on_one_face(r[0], r[i]) for i in range(2, n - 1)):
            return [(r[0], r[i], r[i + 1]) for i in range(1, n - 1)]
    raise AssertionError("no admissible fan for loop %r" % (loop,))


def case_triangles(case):
    tris = []
    for loop in loops(case):
        tris += triangulate(loop)
    if FLIP:
        tris = [(a, c, b) for a, b, c in tris]
    assert len(tris) <= MAX_TRIS
    return tris


def tables():
    return [case_triangles(c) for c in range(256)]


def render():
    t = tables()
    lines = [
        "// generated by giga_amd/csrc/gen_mc_tables.py -- do not edit; tests/test_mesh_host.py regenerates and compares.",
        "// Marching-cubes case tables: bit m of a case is set when the value at corner m is <= iso; corners and edges in the",
        "// customary numbering (see the generator).  GIGA_MC_TRIS[c] holds GIGA_MC_NTRI[c] triangles as edge numbers, padded with 255.",
        "// Define GIGA_MC_QUAL (e.g. `__device__`) before including to place the arrays; the default is `static`.",
        "#pragma once",
        "#ifndef GIGA_MC_QUAL",
        "#define GIGA_MC_QUAL static",
        "#endif",
        "#define GIGA_MC_MAX_TRIS %d" % MAX_TRIS,
        "GIGA_MC_QUAL const unsigned char GIGA_MC_NTRI[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t[c])) for c in range(r, r + 32)) + ",")
    lines.append("};")
    lines.append("GIGA_MC_QUAL const unsigned char GIGA_MC_TRIS[256][%d] = {" % (3 * MAX_TRIS + 1))
    for c in range(256):
        flat = [e for tri in t[c] for e in tri]
        flat += [255] * (3 * MAX_TRIS + 1 - len(flat))
        lines.append("    {" + ", ".join("%3d" % e for e in flat) + "},")
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        sys.exit(0 if open(HEADER).read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", HEADER)
