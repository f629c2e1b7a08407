"""Helpers for the box-record elision of the scene compiler (csrc/scene_compile.cpp elide_box_nodes), shared by tests/test_elide_host.py,
tests/test_gpu_elide.py and scripts/cpu_elide_counts.py: the tree behind a dumped threaded array, the compiler's cost model restated, and
which records of the full array (RT_LAYOUT_ALL_BOX_NODES) the default array kept."""
import numpy as np


def boxed(nodes):
    return np.isfinite(nodes["mn"]).all(axis=1) & np.isfinite(nodes["mx"]).all(axis=1)


def parents(nodes):
    """parent[i] of every record of a pre-order threaded array (-1: top level). A record's subtree ends at its skip link."""
    n = len(nodes)
    parent, stack = np.full(n, -1, dtype=np.int64), []
    for i in range(n):
        while stack and stack[-1][1] <= i:
            stack.pop()
        parent[i] = stack[-1][0] if stack else -1
        if int(nodes["skip"][i]) > i + 1:
            stack.append((i, int(nodes["skip"][i])))
    return parent


def inner_records(nodes, every_child_boxed=True):
    """The records the pass may leave out: a finite box, no leaf word, at least one child — and, the library's own addition to that rule,
    every child boxed (False: the rule without the addition; on a tree whose records all have finite boxes the two are the same set)."""
    par, bx = parents(nodes), boxed(nodes)
    kids, bare = np.zeros(len(nodes), int), np.zeros(len(nodes), int)
    for i, p in enumerate(par):
        if p >= 0:
            kids[p] += 1
            bare[p] += 0 if bx[i] else 1
    ok = bx & (nodes["leaf"] == 0) & (kids > 0)
    return np.flatnonzero(ok & (bare == 0) if every_child_boxed else ok)


def half_area(nodes):
    e = nodes["mx"].astype(np.float64) - nodes["mn"].astype(np.float64)
    return e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]


def model_cost(nodes, kept):
    """The compiler's model: every kept boxed record costs P(entered) of its nearest kept boxed ancestor, 1 without one;
    P(entered Z) = min(1, A(Z) / A(R)), R the outermost record above Z. A record whose box is not finite is no box test; what lies below
    it starts trees of its own."""
    par, bx = parents(nodes), boxed(nodes)
    area = half_area(nodes)
    cost = 0.0
    for i in range(len(nodes)):
        if not (bx[i] and kept[i]):
            continue
        a = par[i]
        while a >= 0 and bx[a] and not kept[a]:
            a = par[a]
        if a < 0 or not bx[a]:
            cost += 1.0
            continue
        top = a
        while par[top] >= 0 and bx[par[top]]:
            top = par[top]
        cost += min(1.0, area[a] / area[top]) if area[top] > 0 else 1.0
    return cost


def _leaves_below(nodes):
    """Records with a leaf word in every record's subtree, itself included."""
    has = np.concatenate([[0], np.cumsum(nodes["leaf"] != 0)])
    i = np.arange(len(nodes))
    return has[np.maximum(nodes["skip"].astype(np.int64), i + 1).clip(max=len(nodes))] - has[i]


def kept_mask(full, elided):
    """Which records of `full` are in `elided` — which must be `full` minus some records without a leaf word, in order. Matched on
    structure, not on boxes alone (a parent may have its child's box): a record with a leaf word always stays; one without is the
    record at hand in `elided` when that has none either, holds as many leaves below it and the same box bytes (NaN included). A parent
    and its only child with equal boxes cannot be told apart, and need not be: they have the same links."""
    lf, le = _leaves_below(full), _leaves_below(elided)
    box = lambda a, k: a["mn"][k].tobytes() + a["mx"][k].tobytes()
    kept, j = np.zeros(len(full), bool), 0
    for i in range(len(full)):
        if j >= len(elided):
            break
        if full["leaf"][i] != 0:
            assert elided["leaf"][j] == full["leaf"][i] and box(full, i) == box(elided, j), f"leaf record {i} is missing or changed"
        elif elided["leaf"][j] != 0 or le[j] != lf[i] or box(full, i) != box(elided, j):
            continue
        kept[i] = True
        j += 1
    assert j == len(elided) and np.all(full["leaf"][~kept] == 0), "the elided array is not the full array minus some records"
    return kept


def check_links(full, elided, kept):
    """Every link of a kept record leads where it led: to the first kept record at or after its old target."""
    new_index = np.concatenate([[0], np.cumsum(kept)])           # new_index[x]: kept records before x = where a link to x goes now
    assert np.array_equal(elided["skip"], new_index[full["skip"][kept]])
    assert np.all(elided["skip"] > np.arange(len(elided))) and elided["skip"].max() == len(elided)


def first_spheres(info):
    return [k for w in info["first"] for k in range(w & 0xFFFFFF, (w & 0xFFFFFF) + ((w >> 24) & 15))]


class Walk:
    """The walk of tests/test_compile.py::traverse on plain floats (the script walks 10^5 segments): (t, sphere, box visits, sphere tests)."""

    def __init__(self, nodes, spheres, first=()):
        self.n = len(nodes)
        bx = boxed(nodes)
        self.rec = [(bool(bx[i]), tuple(float(v) for v in nodes["mn"][i]), tuple(float(v) for v in nodes["mx"][i]), int(nodes["skip"][i]), int(nodes["leaf"][i]))
                    for i in range(self.n)]
        self.sph = [tuple(float(v) for v in s) for s in spheres]
        self.first = list(first)

    def _sphere(self, k, o, d, a, tmin, best):
        cx, cy, cz, r = self.sph[k]
        ox, oy, oz = o[0] - cx, o[1] - cy, o[2] - cz
        hb = ox * d[0] + oy * d[1] + oz * d[2]
        det = hb * hb - a * (ox * ox + oy * oy + oz * oz - r * r)
        if det < 0:
            return None
        sq = det ** 0.5
        root = (-hb - sq) / a
        if root < tmin or best < root:
            root = (-hb + sq) / a
            if root < tmin or best < root:
                return None
        return root

    def __call__(self, o, d, tmin=0.001):
        inf = float("inf")
        best, hit, visits, tests = inf, -1, 0, 0
        a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        inv = [(1.0 / v if v != 0.0 else inf) for v in d]
        for k in self.first:
            tests += 1
            root = self._sphere(k, o, d, a, tmin, best)
            if root is not None:
                best, hit = root, k
        i, n, rec = 0, self.n, self.rec
        while i < n:
            bx, mn, mx, skip, leaf = rec[i]
            if bx:
                visits += 1
                lo, hi, ok = tmin, best, True
                for ax in range(3):
                    t0, t1 = (mn[ax] - o[ax]) * inv[ax], (mx[ax] - o[ax]) * inv[ax]
                    if inv[ax] < 0:
                        t0, t1 = t1, t0
                    lo = lo if lo > t0 else t0
                    hi = hi if hi < t1 else t1
                    if hi <= lo:
                        ok = False
                        break
                if not ok:
                    i = skip
                    continue
            if leaf:
                assert leaf >> 28 == 1
                f, c = leaf & 0xFFFFFF, (leaf >> 24) & 15
                for k in range(f, f + c):
                    tests += 1
                    root = self._sphere(k, o, d, a, tmin, best)
                    if root is not None:
                        best, hit = root, k
            i += 1
        return best, hit, visits, tests
