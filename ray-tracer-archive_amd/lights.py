"""light_reference: a numpy restatement of the device's light sampler (csrc/kernels.hip lights_random / lights_pdf_value) for every light
kind and wrapper of RT_SCENE_LIGHTS_ALL_SHAPES (include/rt_hip.h), and of the reference's kinds with the flag clear.

It restates the ARITHMETIC, operation for operation and in the device's order, in a dtype of the caller's choice: float64 is the yardstick
the tests hold rt_sample_lights to, float32 shows how far that arithmetic alone moves a result (the device's bound is a multiple of it). The
inputs are the device's: light parameters and wrapper maps rounded to f32 as the scene compiler rounds them, points and directions as f32.
A division is a * (1 / b), as the device forms it (v_rcp_f32); in f64 that is a division to the last bit or two.

Draw orders (one SplitMix64 stream per query, seeded with the query's state, as kernels.hip Rng):
    pick        next64() % n_lights; with RT_SCENE_LIGHTS_MANY one rnd() u, the first member k with cdf_k > u (light_weights)
    rect        range(a0, a1), range(b0, b1); the point has k on the rect's axis
    triangle    r1, r2; s = sqrt(r1); (1 - s) v0 + s (1 - r2) v1 + s r2 v2   (pdf: the kernel's tri_hit, closed edges included)
    box         next64() % 6 picks a side in boxes.rs order (z1 z0 y1 y0 x1 x0), then that rect's two draws
    sphere      r1, r2 of random_to_sphere (pdf.rs:82-91)
A member under Translate / RotateY / FlipFace: the chain is one rigid map (world -> the member's space); the point goes there, the drawn
direction is rotated back, the pdf is evaluated there.

RT_SCENE_LIGHTS_MANY: the list's pdf is sum_k p_k pdf_k with the f32 weights of light_weights, summed here in LIST order (the device sums in
the leaf order of its light tree, light_tree: the same terms, another order of rounding)."""
import ctypes as C
import math

import numpy as np

from . import _abi as A

GAMMA = np.uint64(0x9E3779B97F4A7C15)
T_MIN = 0.001
TRI_SLACK_MAX = 0.0009765625      # kernels.hip kTriSlackMax
MAX_WRAP_OPS = 6


def _fin(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


class _Rng:
    """n independent SplitMix64 streams (kernels.hip Rng); `live` masks the queries that draw."""

    def __init__(self, states, dtype):
        self.s = np.array(states, dtype=np.uint64).copy()
        self.n = np.zeros(self.s.shape, dtype=np.uint32)
        self.dtype = dtype

    def next64(self, live):
        with np.errstate(over="ignore"):
            self.s = np.where(live, self.s + GAMMA, self.s)
            self.n = self.n + live.astype(np.uint32)
            return _fin(self.s)

    def rnd(self, live):
        return ((self.next64(live) >> np.uint64(40)).astype(np.float64) * (1.0 / 16777216.0)).astype(self.dtype)

    def range(self, lo, hi, live):
        return lo + (hi - lo) * self.rnd(live)


def lights_of(desc):
    """The lights list of an RtSceneDesc as records: dict(kind, p (f32 values), theta_sin, theta_cos, off, has_xform), as
    scene_compile.cpp compile_lights builds them. Raises ValueError for what RT_SCENE_LIGHTS_ALL_SHAPES refuses."""
    if desc.lights < 0:
        return []
    H = desc.hittables
    L = H[desc.lights]
    ids = [desc.children[L.first_child + c] for c in range(L.n_children)] if L.kind == A.RT_HIT_LIST else [desc.lights]
    all_shapes = bool(desc.scene_flags & A.RT_SCENE_LIGHTS_ALL_SHAPES)
    f32 = lambda v: float(np.float32(v))
    out = []
    for hid in ids:
        h = H[hid]
        if not all_shapes:
            if h.kind == A.RT_HIT_XZ_RECT:
                out.append(dict(kind="rect", p=[f32(h.p[i]) for i in range(5)] + [1.0], has_xform=False))
            elif h.kind == A.RT_HIT_SPHERE:
                out.append(dict(kind="sphere", p=[f32(h.p[i]) for i in range(4)], has_xform=False))
            else:
                out.append(dict(kind="default", p=[], has_xform=False))
            continue
        theta, off, ops, identity = 0.0, [0.0, 0.0, 0.0], 0, True
        while h.kind in (A.RT_HIT_TRANSLATE, A.RT_HIT_ROTATE_Y, A.RT_HIT_FLIP_FACE):
            if h.kind == A.RT_HIT_TRANSLATE:                 # scene_compile.cpp apply_translate
                s, k = math.sin(theta), math.cos(theta)
                off = [off[0] + k * h.p[0] + s * h.p[2], off[1] + h.p[1], off[2] - s * h.p[0] + k * h.p[2]]
                identity = False
            elif h.kind == A.RT_HIT_ROTATE_Y:
                theta += h.p[0] * math.pi / 180.0
                identity = False
            ops += 1
            h = H[h.first_child]
        if ops > MAX_WRAP_OPS:
            raise ValueError("a chain of more than 6 wrappers")
        p = h.p
        if h.kind in (A.RT_HIT_XY_RECT, A.RT_HIT_XZ_RECT, A.RT_HIT_YZ_RECT):
            if (p[1] - p[0]) * (p[3] - p[2]) == 0.0:
                raise ValueError("a rect of zero area")
            kaxis = {A.RT_HIT_XY_RECT: 2.0, A.RT_HIT_XZ_RECT: 1.0, A.RT_HIT_YZ_RECT: 0.0}[h.kind]
            rec = dict(kind="rect", p=[f32(p[i]) for i in range(5)] + [kaxis], area=abs((p[1] - p[0]) * (p[3] - p[2])))
        elif h.kind == A.RT_HIT_TRIANGLE:
            v = np.array([p[i] for i in range(9)]).reshape(3, 3)
            if not np.any(np.cross(v[1] - v[0], v[2] - v[0]) != 0.0):
                raise ValueError("a triangle of zero area")
            rec = dict(kind="tri", p=[f32(p[i]) for i in range(9)], area=0.5 * math.sqrt(float(np.sum(np.cross(v[1] - v[0], v[2] - v[0]) ** 2))))
        elif h.kind == A.RT_HIT_BOX:
            if any(p[3 + a] - p[a] == 0.0 for a in range(3)):
                raise ValueError("a box with sides of zero area")
            dx, dy, dz = abs(p[3] - p[0]), abs(p[4] - p[1]), abs(p[5] - p[2])
            rec = dict(kind="box", p=[f32(p[0]), f32(p[3]), f32(p[1]), f32(p[4]), f32(p[2]), f32(p[5])], area=2.0 * (dx * dy + dy * dz + dz * dx))
        elif h.kind == A.RT_HIT_SPHERE:
            rec = dict(kind="sphere", p=[f32(p[i]) for i in range(4)], area=4.0 * math.pi * p[3] * p[3])
        else:
            raise ValueError(f"hittable kind {h.kind} cannot be sampled as a light")
        rec.update(has_xform=not identity, sin=f32(math.sin(theta)), cos=f32(math.cos(theta)), off=[f32(x) for x in off])
        out.append(rec)
    return out


def light_weights(desc, dtype=np.float32):
    """(p, cdf), arrays by member: the area-weighted pick of RT_SCENE_LIGHTS_MANY as include/rt_hip.h states it. Areas from the desc's f64
    parameters; in f64 and list order total = the sequential sum, p_k = (float)(A_k / total), cdf_k = (float)((A_0 + .. + A_k) / total) with a
    sequential running sum, cdf_{n-1} = 1.0f exactly. dtype float32: the device's table, to the bit; float64: the same rule without the
    final rounding, the yardstick's weights."""
    T = np.dtype(dtype).type
    areas = [float(l["area"]) for l in lights_of(desc)]
    total = 0.0
    for a in areas:
        total += a
    if not (total > 0.0 and math.isfinite(total)):
        raise ValueError("the lights' total area is not a positive finite number")
    p, cdf, run = np.empty(len(areas), T), np.empty(len(areas), T), 0.0
    for k, a in enumerate(areas):
        run += a
        p[k], cdf[k] = T(a / total), T(run / total)
    cdf[-1] = T(1.0)
    return p, cdf


LIGHT_NODE_DTYPE = np.dtype([("cx", np.float32), ("cy", np.float32), ("hx", np.float32), ("hy", np.float32), ("cz", np.float32), ("hz", np.float32),
                             ("skip", np.uint32), ("leaf", np.uint32)])


def light_tree(desc):
    """rt_scene_light_tree_dump: dict(nodes (LIGHT_NODE_DTYPE, 2n - 1 records in pre-order: box = centre -+ half extent, skip = index of the first
    record after the subtree, leaf = 0 or 1 + slot), slot_member (uint32, n: the member in table slot s), p, cdf (float32, n, by member)) of a
    scene with RT_SCENE_LIGHTS_MANY. Host only."""
    from .api import _check, lib
    n, m = C.c_uint64(), C.c_uint64()
    _check(lib().rt_scene_light_tree_dump(C.byref(desc), None, 0, None, None, None, 0, C.byref(n), C.byref(m)))
    nodes = np.zeros(m.value, dtype=LIGHT_NODE_DTYPE)
    slot_member, p, cdf = np.zeros(n.value, np.uint32), np.zeros(n.value, np.float32), np.zeros(n.value, np.float32)
    fp = C.POINTER(C.c_float)
    _check(lib().rt_scene_light_tree_dump(C.byref(desc), nodes.ctypes.data_as(C.c_void_p), len(nodes), slot_member.ctypes.data_as(C.POINTER(C.c_uint32)),
                                          p.ctypes.data_as(fp), cdf.ctypes.data_as(fp), n.value, C.byref(n), C.byref(m)))
    return dict(nodes=nodes, slot_member=slot_member, p=p, cdf=cdf)


def _box_side(p, s):
    """(a0, a1, b0, b1, k, kaxis) of side s in boxes.rs order; p = x0 x1 y0 y1 z0 z1"""
    return [(p[0], p[1], p[2], p[3], p[5], 2), (p[0], p[1], p[2], p[3], p[4], 2), (p[0], p[1], p[4], p[5], p[3], 1),
            (p[0], p[1], p[4], p[5], p[2], 1), (p[2], p[3], p[4], p[5], p[1], 0), (p[2], p[3], p[4], p[5], p[0], 0)][s]


class _Ops:
    """vector arithmetic in one dtype, in the device's operation order (kernels.hip V3 helpers; -ffp-contract=off: nothing is fused)"""

    def __init__(self, dtype):
        self.T = dtype

    def c(self, v):
        return self.T(v)

    def div(self, a, b):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            return a * (self.T(1.0) / b)

    def dot(self, a, b):
        return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]

    def cross(self, u, v):
        return [u[1] * v[2] - u[2] * v[1], -(u[0] * v[2] - u[2] * v[0]), u[0] * v[1] - u[1] * v[0]]

    def len2(self, a):
        return self.dot(a, a)

    def len(self, a):
        return np.sqrt(self.len2(a))

    def unit(self, a):
        r = self.T(1.0) / np.sqrt(self.len2(a))
        return [a[0] * r, a[1] * r, a[2] * r]

    def sub(self, a, b):
        return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _rect_pdf(M, o, v, a0, a1, b0, b1, k, kaxis, diag):
    T = M.T
    ia, ib = (1 if kaxis == 0 else 0), (1 if kaxis == 2 else 2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = M.div(T(k) - o[kaxis], v[kaxis])
        ok = ~(t < T(T_MIN)) & np.isfinite(t)
        a, b = o[ia] + t * v[ia], o[ib] + t * v[ib]
        hit = ok & ~((a < T(a0)) | (a > T(a1)) | (b < T(b0)) | (b > T(b1)))
        area = (T(a1) - T(a0)) * (T(b1) - T(b0))
        d2 = t * t * M.len2(v)
        cosine = np.abs(M.div(v[kaxis], M.len(v)))
        pdf = M.div(M.div(d2, cosine), area)
        edge = np.minimum(np.minimum(np.abs(a - T(a0)), np.abs(T(a1) - a)), np.minimum(np.abs(b - T(b0)), np.abs(T(b1) - b)))
    near = ok & (a > T(a0) - T(1e-4)) & (a < T(a1) + T(1e-4)) & (b > T(b0) - T(1e-4)) & (b < T(b1) + T(1e-4))     # within reach of the rect
    diag["edge"] = np.where(near, np.minimum(diag["edge"], edge), diag["edge"])
    diag["cos"] = np.where(hit, np.minimum(diag["cos"], cosine), diag["cos"])
    diag["tmin"] = np.where(ok, np.minimum(diag["tmin"], np.abs(t - T(T_MIN))), diag["tmin"])
    return np.where(hit, pdf, T(0.0))


def _tri_pdf(M, o, v, p, diag):
    T = M.T
    v0, v1, v2 = [T(x) for x in p[0:3]], [T(x) for x in p[3:6]], [T(x) for x in p[6:9]]
    e1, e2 = M.sub(v1, v0), M.sub(v2, v0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pv = M.cross(v, e2)
        det = M.dot(e1, pv)
        inv = M.div(T(1.0), det)
        tv = M.sub(o, v0)
        u = M.dot(tv, pv) * inv
        qv = M.cross(tv, e1)
        w = M.dot(v, qv) * inv
        t = M.dot(e2, qv) * inv
        ok = (det != T(0.0)) & ~(t < T(T_MIN)) & np.isfinite(t)
        # the kernel's closed edges (kernels.hip tri_close_edges): a barycentric outside [0, 1] by no more than the f32 test's own rounding bound
        # counts as inside. The bound is the DEVICE's (eps = 2^-24) in either dtype: it is part of the rule, not of the arithmetic.
        n1 = lambda a: np.abs(a[0]) + np.abs(a[1]) + np.abs(a[2])
        sl = T(TRI_SLACK_MAX)
        bound = n1(v) * (n1(e2) * (n1(tv) + n1(e1)) + n1(tv) * n1(e1))
        tol = np.minimum(T(8.0) * T(5.9604645e-8) * (bound * np.abs(inv) + T(1.0)), sl)
        outside = (u < T(0.0)) | (u > T(1.0)) | (w < T(0.0)) | (u + w > T(1.0))
        closed = ~((u < -sl) | (u > T(1.0) + T(2.0) * sl) | (w < -sl) | (u + w > T(1.0) + sl)) & (u >= -tol) & (w >= -tol) & (u + w <= T(1.0) + tol)
        hit = ok & (~outside | closed)
        nn = M.cross(e1, e2)
        ln = M.len(nn)
        d2 = t * t * M.len2(v)
        cosine = np.abs(M.div(M.dot(v, nn), M.len(v) * ln))
        pdf = M.div(M.div(d2, cosine), T(0.5) * ln)
        # distance from the nearest line that decides hit or miss: the edge itself, and the edge moved out by the rule's bound
        edge = np.minimum(np.minimum(np.abs(u), np.abs(w)), np.abs(T(1.0) - (u + w)))
        edge = np.minimum(edge, np.minimum(np.minimum(np.abs(u + tol), np.abs(w + tol)), np.abs(T(1.0) + tol - (u + w))))
    near = ok & (u > -tol - T(1e-4)) & (w > -tol - T(1e-4)) & (u + w < T(1.0 + 1e-4) + tol)
    diag["edge"] = np.where(near, np.minimum(diag["edge"], edge), diag["edge"])
    diag["cos"] = np.where(hit, np.minimum(diag["cos"], cosine), diag["cos"])
    diag["tmin"] = np.where(ok, np.minimum(diag["tmin"], np.abs(t - T(T_MIN))), diag["tmin"])
    return np.where(hit, pdf, T(0.0))


def _sphere_pdf(M, o, v, p, diag):
    T = M.T
    c, r = [T(x) for x in p[0:3]], T(p[3])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # the device decides the hit with f64 FMAs from its f32 inputs (kernels.hip sphere_two_roots): the yardstick is the exact quadratic
        oc = [x.astype(np.float64) - np.float64(cc) for x, cc in zip(o, c)]
        vd = [x.astype(np.float64) for x in v]
        a = sum(x * x for x in vd)
        hb = sum(x * y for x, y in zip(oc, vd))
        cc = sum(x * x for x in oc) - np.float64(r) * np.float64(r)
        det = hb * hb - a * cc
        sq = np.sqrt(np.maximum(det, 0.0))
        t0, t1 = (-hb - sq) / a, (-hb + sq) / a
        root = np.where(t0 >= T_MIN, t0, t1)
        hit = (det >= 0.0) & (root >= T_MIN)
        cos_theta_max = np.sqrt(T(1.0) - M.div(r * r, M.len2(M.sub(c, o))))
        solid_angle = T(2.0) * T(math.pi) * (T(1.0) - cos_theta_max)
        pdf = M.div(T(1.0), solid_angle)
        # how squarely the ray meets the sphere: |cos| between the ray and the normal at the hit = sqrt(det / a) / r
        cosine = np.sqrt(np.maximum(det, 0.0) / a) / abs(float(r))
    grazing = np.abs(det) / (a * float(r) * float(r)) < 1e-4                      # near the silhouette: hit or miss is not decidable
    diag["cos"] = np.where(hit | grazing, np.minimum(diag["cos"], np.where(grazing, 0.0, cosine)), diag["cos"])
    diag["tmin"] = np.where(hit, np.minimum(diag["tmin"], np.abs(root - T_MIN)), diag["tmin"])
    return np.where(hit, pdf, T(0.0)).astype(T)


def _to_local(M, l, o, v):
    if not l["has_xform"]:
        return o, v
    s, c = M.T(l["sin"]), M.T(l["cos"])
    m = [o[0] - M.T(l["off"][0]), o[1] - M.T(l["off"][1]), o[2] - M.T(l["off"][2])]
    ol = [c * m[0] - s * m[2], m[1], s * m[0] + c * m[2]]
    vl = None if v is None else [c * v[0] - s * v[2], v[1], s * v[0] + c * v[2]]
    return ol, vl


def _light_pdf(M, l, o, v, diag):
    if l["kind"] == "default":
        return np.zeros(o[0].shape, dtype=M.T)
    o, v = _to_local(M, l, o, v)
    p = l["p"]
    if l["kind"] == "rect":
        return _rect_pdf(M, o, v, p[0], p[1], p[2], p[3], p[4], int(p[5]), diag)
    if l["kind"] == "tri":
        return _tri_pdf(M, o, v, p, diag)
    if l["kind"] == "box":
        total = np.zeros(o[0].shape, dtype=M.T)
        for s in range(6):
            a0, a1, b0, b1, k, kaxis = _box_side(p, s)
            total = total + M.T(M.T(1.0) / M.T(6.0)) * _rect_pdf(M, o, v, a0, a1, b0, b1, k, kaxis, diag)
        return total
    return _sphere_pdf(M, o, v, p, diag)


def _rect_random(M, o, a0, a1, b0, b1, k, kaxis, g, live):
    T = M.T
    ra = g.range(T(a0), T(a1), live)
    rb = g.range(T(b0), T(b1), live)
    kk = np.full(ra.shape, T(k), dtype=T)
    pt = [kk, ra, rb] if kaxis == 0 else ([ra, kk, rb] if kaxis == 1 else [ra, rb, kk])
    return M.sub(pt, o)


def _light_random(M, l, o, g, live):
    T = M.T
    n = o[0].shape
    if l["kind"] == "default":
        return [np.ones(n, dtype=T), np.zeros(n, dtype=T), np.zeros(n, dtype=T)]
    o, _ = _to_local(M, l, o, None)
    p = l["p"]
    if l["kind"] == "rect":
        d = _rect_random(M, o, p[0], p[1], p[2], p[3], p[4], int(p[5]), g, live)
    elif l["kind"] == "tri":
        r1, r2 = g.rnd(live), g.rnd(live)
        s = np.sqrt(r1)
        w0, w1, w2 = T(1.0) - s, s * (T(1.0) - r2), s * r2
        pt = [(w0 * T(p[i]) + w1 * T(p[3 + i])) + w2 * T(p[6 + i]) for i in range(3)]
        d = M.sub(pt, o)
    elif l["kind"] == "box":
        side = (g.next64(live) % np.uint64(6)).astype(np.int64)
        ra_u, rb_u = g.rnd(live), g.rnd(live)
        d = [np.zeros(n, dtype=T) for _ in range(3)]
        for s in range(6):
            a0, a1, b0, b1, k, kaxis = _box_side(p, s)
            ra, rb = T(a0) + (T(a1) - T(a0)) * ra_u, T(b0) + (T(b1) - T(b0)) * rb_u
            kk = np.full(n, T(k), dtype=T)
            pt = [kk, ra, rb] if kaxis == 0 else ([ra, kk, rb] if kaxis == 1 else [ra, rb, kk])
            ds = M.sub(pt, o)
            d = [np.where(side == s, ds[i], d[i]) for i in range(3)]
    else:                                                   # sphere.rs:85-90, pdf.rs:82-91, onb.rs:19-42
        direction = M.sub([T(p[0]), T(p[1]), T(p[2])], o)
        dist2 = M.len2(direction)
        w = M.unit(direction)
        big = np.abs(w[0]) > T(0.9)
        a = [np.where(big, T(0.0), T(1.0)), np.where(big, T(1.0), T(0.0)), np.zeros(n, dtype=T)]
        vv = M.unit(M.cross(w, a))
        uu = M.cross(w, vv)
        r1, r2 = g.rnd(live), g.rnd(live)
        with np.errstate(invalid="ignore"):
            z = T(1.0) + r2 * (np.sqrt(T(1.0) - M.div(T(p[3]) * T(p[3]), dist2)) - T(1.0))
            phi = (T(2.0) * T(math.pi)) * r1
            q = np.sqrt(T(1.0) - z * z)
        x, y = np.cos(phi).astype(T) * q, np.sin(phi).astype(T) * q
        d = [(x * uu[i] + y * vv[i]) + z * w[i] for i in range(3)]
    if l["has_xform"]:
        s, c = T(l["sin"]), T(l["cos"])
        d = [c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]]
    return d


def light_reference(desc, points, states=None, dirs=None, dtype=np.float64, env=None):
    """What rt_sample_lights returns for (points, states) — or, with `dirs`, for RT_LIGHTQ_DIRECTION_GIVEN queries — restated in `dtype`
    (np.float64 or np.float32). points, dirs: (n, 3), read as f32; states: n uint64. env: the environment.EnvMap the scene was uploaded with;
    a sampled one is member n of a list of n + 1 (include/rt_hip.h RT_ENV_SAMPLED), also of a scene without a lights list. Its results carry
    env_border and env_sin_theta (environment.env_reference: border, sin_theta) of the direction as well.

    Returns dict(d (n, 3), pdf (n), light (n, int32), n_draws (n, uint32)) plus what decides whether a query can be held to the yardstick at
    all: pick_gap (RT_SCENE_LIGHTS_MANY: the distance of the pick's draw from the nearest inner cdf edge; else inf), cos_min (the smallest |cos|
    at which the ray meets a light), edge_min (the smallest distance of a crossing from a rect's edge, in
    scene units, or from a triangle's edge, in barycentrics — near misses count) and tmin_gap (distance of the nearest crossing from t_min)."""
    T = np.dtype(dtype).type
    M = _Ops(T)
    lights = lights_of(desc)
    env_member = env is not None and env.sampled
    if not lights and not env_member:
        raise ValueError("the scene has no lights list")
    n_members = len(lights) + (1 if env_member else 0)
    many = bool(desc.scene_flags & A.RT_SCENE_LIGHTS_MANY)
    if env_member:
        from . import environment as E
        if many:
            raise ValueError("RT_ENV_SAMPLED together with RT_SCENE_LIGHTS_MANY")
        e_marg, e_cond, _ = E.tables_reference(env.rgb)
    if many:
        p_k, cdf = light_weights(desc, T)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    n = pts.shape[0]
    o = [pts[:, i].astype(T) for i in range(3)]
    light = np.full(n, -1, dtype=np.int32)
    n_draws = np.zeros(n, dtype=np.uint32)
    pick_gap = np.full(n, np.inf)
    if dirs is None:
        g = _Rng(np.asarray(states, dtype=np.uint64).reshape(-1), T)
        every = np.ones(n, dtype=bool)
        if many:                                            # one rnd(): 24 bits, exact in either dtype; the first member whose cdf (in T) exceeds it
            u = g.rnd(every).astype(np.float64)
            light = np.searchsorted(cdf.astype(np.float64), u, side="right").astype(np.int32)
            pick_gap = np.abs(u[:, None] - cdf.astype(np.float64)[None, :-1]).min(axis=1) if len(lights) > 1 else pick_gap
        else:
            light = (g.next64(every) % np.uint64(n_members)).astype(np.int32)
        d = [np.zeros(n, dtype=T) for _ in range(3)]
        for k, l in enumerate(lights):
            live = light == k
            if not live.any():
                continue
            dk = _light_random(M, l, o, g, live)
            d = [np.where(live, dk[i], d[i]) for i in range(3)]
        if env_member and (light == len(lights)).any():
            live = light == len(lights)
            dk, _, _ = E._draw(M, env.width, env.height, e_marg, e_cond, g, live)
            d = [np.where(live, dk[i], d[i]) for i in range(3)]
        n_draws = g.n.copy()
        # the direction the device hands on is its f32 result: the pdf of the yardstick is evaluated for the direction in its own dtype
    else:
        dd = np.asarray(dirs, dtype=np.float32).reshape(-1, 3)
        d = [dd[:, i].astype(T) for i in range(3)]
    diag = dict(cos=np.full(n, np.inf), edge=np.full(n, np.inf), tmin=np.full(n, np.inf))
    weight = T(T(1.0) / T(n_members))
    lsum = np.zeros(n, dtype=T)
    for k, l in enumerate(lights):
        lsum = lsum + (T(p_k[k]) if many else weight) * _light_pdf(M, l, o, d, diag)
    if env_member:
        e_pdf, _, _, e_border, e_sin = E._pdf(M, env.width, env.height, e_marg, e_cond, d)
        lsum = lsum + weight * e_pdf
        return dict(d=np.stack(d, axis=1), pdf=lsum, light=light, n_draws=n_draws, pick_gap=pick_gap, cos_min=diag["cos"], edge_min=diag["edge"],
                    tmin_gap=diag["tmin"], env_border=e_border, env_sin_theta=e_sin)
    return dict(d=np.stack(d, axis=1), pdf=lsum, light=light, n_draws=n_draws, pick_gap=pick_gap, cos_min=diag["cos"], edge_min=diag["edge"], tmin_gap=diag["tmin"])


def solid_angle_triangle(p, a, b, c):
    """Solid angle of the triangle (a, b, c) seen from p (van Oosterom and Strackee 1983), f64."""
    ra, rb, rc = np.asarray(a, float) - p, np.asarray(b, float) - p, np.asarray(c, float) - p
    la, lb, lc = np.linalg.norm(ra), np.linalg.norm(rb), np.linalg.norm(rc)
    num = abs(float(np.dot(ra, np.cross(rb, rc))))
    den = la * lb * lc + np.dot(ra, rb) * lc + np.dot(ra, rc) * lb + np.dot(rb, rc) * la
    return 2.0 * math.atan2(num, den)
