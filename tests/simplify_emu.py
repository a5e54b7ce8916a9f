"""Float64 restatement of the reference's quadric edge collapse (utils/libsimplify/Simplify.h, `simplify_mesh(target, agressiveness)`
on value-initialised records) in two forms:

  simplify         the header's sequential loop;
  simplify_rounds  the schedule of csrc/giga_simplify.hip: per pass, parallel rounds of deterministic reservations (every pending
                   triangle claims, with its index, every vertex of every live face around its three vertices; the triangles that
                   hold all their claims run the header's loop body), the face budget met by a repeated pass, the reference lists
                   rebuilt when their appended region is full.

Python floats are IEEE doubles and every expression below keeps the header's order of operations (no fused multiply-add), so both
forms give the header's bytes.  Vertices (V,3) and faces (F,3) in, (vertices float64, faces int32) out."""
import math

import numpy as np

NAN, INF = math.nan, math.inf


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def _fmin(a, b):                                   # C fmin: a NaN operand is ignored
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN       # (NaN and negative arguments give NaN)


def _normalize(x, y, z):
    s = _sqrt(x * x + y * y + z * z)
    return _div(x, s), _div(y, s), _div(z, s)


def _cross(a, b):
    return a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]


def _det(m, a11, a12, a13, a21, a22, a23, a31, a32, a33):
    return m[a11] * m[a22] * m[a33] + m[a13] * m[a21] * m[a32] + m[a12] * m[a23] * m[a31] \
        - m[a13] * m[a22] * m[a31] - m[a11] * m[a23] * m[a32] - m[a12] * m[a21] * m[a33]


def _vertex_error(q, x, y, z):
    return q[0] * x * x + 2 * q[1] * x * y + 2 * q[2] * x * z + 2 * q[3] * x + q[4] * y * y \
        + 2 * q[5] * y * z + 2 * q[6] * y + q[7] * z * z + 2 * q[8] * z + q[9]


class State:
    """The header's globals: vertices (p, q, border, list), triangles (v, err, n, deleted, dirty)."""

    def __init__(self, vertices, faces):
        v = np.asarray(vertices, dtype=np.float64)
        f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        self.P = [[float(x) for x in row] for row in v]
        self.Q = [[0.0] * 10 for _ in self.P]
        self.border = [0] * len(self.P)
        self.lists = [[] for _ in self.P]          # per vertex: (triangle, corner) pairs
        self.tv = [[int(x) for x in row] for row in f]
        self.terr = [[0.0] * 4 for _ in self.tv]
        self.tn = [(0.0, 0.0, 0.0) for _ in self.tv]
        self.tdel = [0] * len(self.tv)
        self.tdirty = [0] * len(self.tv)
        self.ref_used = 0                          # entries of the shared reference array in use (`simplify_rounds` only)

    def clone(self):
        c = State.__new__(State)
        c.P, c.Q, c.border = [p[:] for p in self.P], [q[:] for q in self.Q], self.border[:]
        c.lists = [lst[:] for lst in self.lists]
        c.tv, c.terr, c.tn = [v[:] for v in self.tv], [e[:] for e in self.terr], self.tn[:]
        c.tdel, c.tdirty, c.ref_used = self.tdel[:], self.tdirty[:], self.ref_used
        return c

    # ---- calculate_error -------------------------------------------------------------------------------------------------
    def calculate_error(self, a, b):
        qa, qb = self.Q[a], self.Q[b]
        q = [qa[i] + qb[i] for i in range(10)]
        border = self.border[a] & self.border[b]
        det = _det(q, 0, 1, 2, 1, 4, 5, 2, 5, 7)
        if det != 0 and not border:
            x = _div(-1.0, det) * _det(q, 1, 2, 3, 4, 5, 6, 5, 7, 8)
            y = _div(1.0, det) * _det(q, 0, 2, 3, 1, 5, 6, 2, 7, 8)
            z = _div(-1.0, det) * _det(q, 0, 1, 3, 1, 4, 6, 2, 5, 8)
            return _vertex_error(q, x, y, z), (x, y, z)
        p1, p2 = self.P[a], self.P[b]
        p3 = ((p1[0] + p2[0]) / 2, (p1[1] + p2[1]) / 2, (p1[2] + p2[2]) / 2)
        e1, e2, e3 = _vertex_error(q, *p1), _vertex_error(q, *p2), _vertex_error(q, *p3)
        error = _fmin(e1, _fmin(e2, e3))
        p = (0.0, 0.0, 0.0)                        # (the header leaves p unset when all three are NaN)
        if e1 == error:
            p = tuple(p1)
        if e2 == error:
            p = tuple(p2)
        if e3 == error:
            p = p3
        return error, p

    def _errors(self, t):
        v, e = self.tv[t], self.terr[t]
        e[0] = self.calculate_error(v[0], v[1])[0]
        e[1] = self.calculate_error(v[1], v[2])[0]
        e[2] = self.calculate_error(v[2], v[0])[0]
        e[3] = _fmin(e[0], _fmin(e[1], e[2]))

    # ---- update_mesh -----------------------------------------------------------------------------------------------------
    def build_lists(self):
        self.lists = [[] for _ in self.P]
        for t, v in enumerate(self.tv):
            for j in range(3):
                self.lists[v[j]].append((t, j))
        self.ref_used = 3 * len(self.tv)

    def rebuild_lists_of_live_faces(self):
        """The overflow path: the lists from the live faces, without the compaction."""
        self.lists = [[] for _ in self.P]
        live = 0
        for t, v in enumerate(self.tv):
            if not self.tdel[t]:
                live += 1
                for j in range(3):
                    self.lists[v[j]].append((t, j))
        self.ref_used = 3 * live

    def update_mesh(self, iteration):
        if iteration > 0:
            keep = [t for t in range(len(self.tv)) if not self.tdel[t]]
            for name in ("tv", "terr", "tn", "tdel", "tdirty"):
                arr = getattr(self, name)
                setattr(self, name, [arr[t] for t in keep])
        if iteration == 0:
            P = self.P
            self.Q = [[0.0] * 10 for _ in P]
            for t, v in enumerate(self.tv):
                p0, p1, p2 = P[v[0]], P[v[1]], P[v[2]]
                n = _cross((p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]), (p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]))
                n = _normalize(*n)
                self.tn[t] = n
                a, b, c = n
                d = -(p0[0] * a + p0[1] * b + p0[2] * c)
                plane = (a * a, a * b, a * c, a * d, b * b, b * c, b * d, c * c, c * d, d * d)
                for j in range(3):
                    q = self.Q[v[j]]
                    self.Q[v[j]] = [q[i] + plane[i] for i in range(10)]
            for t in range(len(self.tv)):          # (before the boundary is identified: these errors see border = 0 everywhere)
                self._errors(t)
        self.build_lists()
        if iteration == 0:
            self.border = [0] * len(self.P)
            for i in range(len(self.P)):
                vids, vcount = [], []
                for t, _ in self.lists[i]:
                    for k in range(3):
                        w = self.tv[t][k]
                        if w in vids:
                            vcount[vids.index(w)] += 1
                        else:
                            vids.append(w)
                            vcount.append(1)
                for w, c in zip(vids, vcount):
                    if c == 1:
                        self.border[w] = 1

    # ---- flipped / the loop body -----------------------------------------------------------------------------------------
    def flipped(self, p, i0, i1, deleted):
        P = self.P
        for k, (t, s) in enumerate(self.lists[i0]):
            if self.tdel[t]:
                continue
            v = self.tv[t]
            id1, id2 = v[(s + 1) % 3], v[(s + 2) % 3]
            if id1 == i1 or id2 == i1:
                deleted[k] = 1
                continue
            a, b = P[id1], P[id2]
            d1 = _normalize(a[0] - p[0], a[1] - p[1], a[2] - p[2])
            d2 = _normalize(b[0] - p[0], b[1] - p[1], b[2] - p[2])
            if abs(d2[0] * d1[0] + d2[1] * d1[1] + d2[2] * d1[2]) > 0.999:
                return True
            n = _normalize(*_cross(d1, d2))
            deleted[k] = 0
            tn = self.tn[t]
            if tn[0] * n[0] + tn[1] * n[1] + tn[2] * n[2] < 0.2:
                return True
        return False

    def _update_triangles(self, i0, lst, deleted, out):
        n_deleted = 0
        for k, (t, s) in enumerate(lst):
            if self.tdel[t]:
                continue
            if deleted[k]:
                self.tdel[t] = 1
                n_deleted += 1
                continue
            self.tv[t][s] = i0
            self.tdirty[t] = 1
            self._errors(t)
            out.append((t, s))
        return n_deleted

    def body(self, i, threshold, deleted0, deleted1, ref_capacity=None):
        """The header's loop body for triangle i (already known to be a candidate).  Returns the number of faces the collapse
        deleted (0: no edge was collapsed), or -1 when the new list did not fit into `ref_capacity` (nothing was changed)."""
        v, err = self.tv[i], self.terr[i]
        for j in range(3):
            if not err[j] < threshold:
                continue
            i0, i1 = v[j], v[(j + 1) % 3]
            if self.border[i0] != self.border[i1]:
                continue
            p = self.calculate_error(i0, i1)[1]
            l0, l1 = self.lists[i0], self.lists[i1]
            _resize(deleted0, len(l0))
            _resize(deleted1, len(l1))
            if self.flipped(p, i0, i1, deleted0):
                continue
            if self.flipped(p, i1, i0, deleted1):
                continue
            if ref_capacity is not None:
                count = sum(1 for k, (t, _) in enumerate(l0) if not self.tdel[t] and not deleted0[k]) + \
                    sum(1 for k, (t, _) in enumerate(l1) if not self.tdel[t] and not deleted1[k])
                if count > len(l0):                # (else the list is rewritten in place)
                    if self.ref_used + count > ref_capacity:
                        return -1
                    self.ref_used += count
            self.P[i0] = list(p)
            q0, q1 = self.Q[i0], self.Q[i1]
            self.Q[i0] = [q1[m] + q0[m] for m in range(10)]
            out = []
            n = self._update_triangles(i0, l0, deleted0, out)
            n += self._update_triangles(i0, l1, deleted1, out)
            self.lists[i0] = out
            return n
        return 0

    def candidate(self, i, threshold):
        return not self.terr[i][3] > threshold and not self.tdel[i] and not self.tdirty[i]

    # ---- compact_mesh ----------------------------------------------------------------------------------------------------
    def compact(self):
        faces = [self.tv[t] for t in range(len(self.tv)) if not self.tdel[t]]
        used = [0] * len(self.P)
        for f in faces:
            for w in f:
                used[w] = 1
        new, verts = [0] * len(self.P), []
        for i, u in enumerate(used):
            if u:
                new[i] = len(verts)
                verts.append(self.P[i])
        return np.array(verts, dtype=np.float64).reshape(-1, 3), \
            np.array([[new[w] for w in f] for f in faces], dtype=np.int32).reshape(-1, 3)


def _resize(lst, n):                               # std::vector::resize: kept entries keep their values, new ones are 0
    if len(lst) > n:
        del lst[n:]
    else:
        lst.extend([0] * (n - len(lst)))


def threshold_of(iteration, agressiveness):
    return 0.000000001 * math.pow(float(iteration + 3), agressiveness)


def simplify(vertices, faces, target, agressiveness=7.0, stats=None):
    """The header's `simplify_mesh(target, agressiveness)` followed by the read-out of vertices and triangles."""
    st = State(vertices, faces)
    count, deleted = len(st.tv), 0
    d0, d1 = [], []
    iterations = 0
    for iteration in range(100):
        if count - deleted <= target:
            break
        iterations += 1
        if iteration % 5 == 0:
            st.update_mesh(iteration)
        st.tdirty = [0] * len(st.tv)
        thr = threshold_of(iteration, agressiveness)
        for i in range(len(st.tv)):
            if not st.candidate(i, thr):
                continue
            deleted += st.body(i, thr, d0, d1)
            if count - deleted <= target:
                break
    if stats is not None:
        stats.update(iterations=iterations, deleted=deleted)
    return st.compact()


# ---- the schedule of the device kernels ----------------------------------------------------------------------------------
def _claim_set(st, i):
    out = set()
    for w in st.tv[i]:
        for t, _ in st.lists[w]:
            if not st.tdel[t]:
                out.update(st.tv[t])
    return out


def run_pass(st, threshold, limit, order, ref_capacity, counters):
    """One pass in rounds over the candidates with index <= limit.  Returns {triangle: faces deleted} of the collapses."""
    pending = [i for i in range(len(st.tv)) if i <= limit and st.candidate(i, threshold)]
    candidates, rounds, log, sets = len(pending), 0, {}, {}
    while True:
        pending = [i for i in pending if not st.tdel[i] and not st.tdirty[i]]
        if not pending:
            break
        rounds += 1
        if rounds > candidates + counters["rebuilds"]:
            raise RuntimeError("a pass took more rounds than it has candidates")
        for i in pending:
            if i not in sets:
                sets[i] = _claim_set(st, i)
        # atomicMin(claim[vertex], index) over all pending triangles: i holds all its claims iff no lower pending triangle
        # claims one of its vertices (pending is ascending)
        claimed, winners, touched = set(), [], set()
        for i in pending:
            if claimed.isdisjoint(sets[i]):
                winners.append(i)
                assert touched.isdisjoint(sets[i])              # winners' claim sets are disjoint
                touched |= sets[i]
            claimed |= sets[i]
        assert winners and winners[0] == pending[0]
        retired, overflow = set(), False
        for i in (winners if order == "ascending" else winners[::-1]):
            n = st.body(i, threshold, [], [], ref_capacity)
            if n < 0:
                overflow = True                                 # stays pending, the lists are rebuilt, the round is repeated
                continue
            retired.add(i)
            if n:
                log[i] = n
        if overflow:
            if not retired and counters.get("just_rebuilt"):
                raise RuntimeError("the reference-list capacity is too small for one collapse")
            st.rebuild_lists_of_live_faces()
            counters["rebuilds"] += 1
        counters["just_rebuilt"] = overflow
        # a collapse changes faces only inside its claim set: the claim sets that do not meet a winner's stay as they are
        pending = [i for i in pending if i not in retired]
        for i in pending:
            if not touched.isdisjoint(sets[i]):
                del sets[i]
    counters["rounds"] += rounds
    counters["max_rounds_over_candidates"] = max(counters.get("max_rounds_over_candidates", 0), rounds - candidates)
    counters["longest_pass"] = max(counters.get("longest_pass", 0), rounds)
    return log


def simplify_rounds(vertices, faces, target, agressiveness=7.0, order="ascending", ref_extra=None, stats=None):
    """`simplify` by the schedule of the device kernels.  order: "ascending" or "descending" execution of a round's winners (the
    result does not depend on it).  ref_extra: room of the reference array beyond 3 F entries (None: unbounded).  stats (a dict)
    receives iterations, rounds, repeats (passes run again for the face budget), rebuilds and longest_pass."""
    st = State(vertices, faces)
    count, deleted = len(st.tv), 0
    cap = None if ref_extra is None else 3 * count + ref_extra
    counters = dict(rounds=0, rebuilds=0)
    iterations = repeats = 0
    for iteration in range(100):
        if count - deleted <= target:
            break
        iterations += 1
        if iteration % 5 == 0:
            st.update_mesh(iteration)
        st.tdirty = [0] * len(st.tv)
        thr = threshold_of(iteration, agressiveness)
        before = st.clone()
        log = run_pass(st, thr, len(st.tv), order, cap, counters)
        total = sum(log.values())
        if count - (deleted + total) <= target:
            need, run = (count - deleted) - target, 0
            for i in sorted(log):
                run += log[i]
                if run >= need:
                    break
            if i != max(log):
                st = before
                log = run_pass(st, thr, i, order, cap, counters)
                total = sum(log.values())
                repeats += 1
        deleted += total
    if stats is not None:
        stats.update(iterations=iterations, rounds=counters["rounds"], repeats=repeats, rebuilds=counters["rebuilds"],
                     longest_pass=counters.get("longest_pass", 0), deleted=deleted,
                     max_rounds_over_candidates=counters.get("max_rounds_over_candidates", 0))
    return st.compact()
