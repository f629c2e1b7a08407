"""Scenes, answers and bounds for the normal-map tests (tests/test_normal_maps_host.py, tests/test_gpu_normal_maps.py): the meshes and ray
sets of tests/mesh_attrs.py with a normal map (include/rt_hip.h RtNormalMap) bound to the material of their attribute triangles, and for
every ray the f64 answer — the set's own checker records put through mesh.normal_map_reference and the wrapper replay of mesh_attrs.
Nothing here comes from a GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_attrs as M  # noqa: E402
import rays as R  # noqa: E402

SCENES = ["ico1", "big", "wrapped"]
MAP_W, MAP_H = 16, 8
# The numpy statement at f32 over the checker's precision-32 records against the same at f64 over its precision-64 records, on the decidable
# non-edge rays whose texel is the same at both precisions and under a move of (u, v) by the scene's uv bound: worst |dn| per scene. The
# device is allowed 2 x each figure (the project's factor). Produced on a CPU by
#     python -m pytest tests/test_normal_maps_host.py -k f32_figure -s
# which measures them again and holds them to this table within 1 %.
MEASURED_F32 = {
    "ico1": dict(n=1.240e-06),
    "big": dict(n=4.318e-07),
    "wrapped": dict(n=2.455e-06),
    "wrapped_lone": dict(n=1.978e-07),      # the one triangle of `wrapped` that has the mapped material and no attributes (lone_set below)
}
# front_face of a mapped hit is the sign of dot(d, ns). Its f32 evaluation is off by the error of ns (below 1e-5 in every scene above, x 2 on
# the device) plus three roundings of the products, so a ray whose |dot(unit(d), ns)| is above 1e-4 has the same sign at every precision;
# the others are left out as undecidable.
FF_MARGIN = 1e-4
TEXEL_CAP = 0.02               # the project's allowance for hits on a texel boundary


def bound_of(name):
    return {q: 2.0 * v for q, v in MEASURED_F32[name].items()}


def random_map(seed=7):
    """A seeded random 16 x 8 map: red and green anywhere in 0..255 (tilts up to 45 degrees and more), blue in 128..255 (ns stays on N's side)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (MAP_H, MAP_W, 3)).astype(np.uint8)
    img[..., 2] = 128 + img[..., 2] // 2
    return img


def bind(pkg, mesh, image, strength=1.0, flip_green=False):
    """The scene of `mesh` (a fresh mesh_attrs.build_scene: its builder is this call's alone) with `image` bound to the material of its
    attribute triangles; returns (desc, normal_maps). The hittable ids are the unmapped scene's."""
    b, old = mesh.built.keep, mesh.built.desc
    mat = old.hittables[min(mesh.tris)].material
    b.normal_map(mat, image, strength, flip_green)
    before = b._keep                                   # (desc() below replaces the arrays `old` points into)
    desc = b.desc(old.world, old.lights)
    mesh.built.desc, mesh.unmapped = desc, (old, before)
    return desc, b.normal_maps()


def expected(pkg, mesh, chains, rays, ans, tri, image, T, strength=1.0, flip_green=False):
    """mesh_attrs.expected with the map applied: (n, ff, u, v, texel) for the rays whose hit lies on attribute triangle tri[i] >= 0 (other
    rows: the checker's own, texel -1), every operation in T."""
    n, ff, u, v = ans["n"].astype(T), ans["ff"].copy(), ans["u"].astype(T), ans["v"].astype(T)
    texel = np.full(len(rays), -1, np.int64)
    k = np.flatnonzero(tri >= 0)
    key = lambda h: tuple((w[0], tuple(w[1])) for w in chains[int(h)])
    for chain in {key(h) for h in np.unique(tri[k])}:
        m = k[[key(h) == chain for h in tri[k]]]
        chain = list(chain)
        dk = M.local_directions(pkg, chain, rays["d"][m], T)
        nl, fl, u[m], v[m], texel[m] = pkg.normal_map_reference(mesh.tris, mesh.attrs, tri[m], ans["u"][m], ans["v"][m], image, strength, flip_green, T, d=dk[-1])
        n[m], ff[m] = M.replay(pkg, chain, dk, nl, fl, T)
    return n, ff, u, v, texel


_cache = {}


def mapped_set(pkg, orc, name, seed=7):
    """mesh_attrs.ray_set(name) with the random map bound: dict(base = that set, mesh, desc, maps, image, n, ff, u, v, texel — the f64 answer —
    and use: the decidable, non-edge rays on a mapped attribute triangle whose texel does not change when (u, v) moves by the scene's uv
    bound (mesh_attrs.bound_of) and whose mapped front_face is decided by FF_MARGIN; boundary: the share of rays the texel rule left out)."""
    if (name, seed) in _cache:
        return _cache[(name, seed)]
    s = M.ray_set(pkg, orc, name)
    mesh = M.build_scene(pkg, name)
    image = random_map(seed)
    desc, maps = bind(pkg, mesh, image)
    n, ff, u, v, texel = expected(pkg, mesh, s["chains"], s["rays"], s["ref"], s["tri"], image, np.float64)
    on = s["decidable"] & ~s["edge"] & (s["tri"] >= 0)
    delta = M.bound_of(name)["uv"]
    steady = np.ones(len(n), bool)
    for su in (-delta, delta):
        for sv in (-delta, delta):
            i, j = pkg.texel_of(u + su, v + sv, MAP_W, MAP_H)
            steady &= (j * MAP_W + i) == texel
    # the sign of the mapped front_face: dot(unit(d), ns) in the triangle's space = -|dot(unit(d), n)| after the replay, which turns n against the ray
    d = s["rays"]["d"].astype(np.float64)
    cosine = np.abs(np.einsum("ij,ij->i", d / np.linalg.norm(d, axis=1, keepdims=True), n))
    firm = cosine > FF_MARGIN
    out = dict(base=s, mesh=mesh, desc=desc, maps=maps, image=image, n=n, ff=ff, u=u, v=v, texel=texel, use=on & steady & firm, firm=firm,
               boundary=float((on & ~steady).sum()) / max(1, int(on.sum())), grazing=int((on & ~firm).sum()))
    _cache[(name, seed)] = out
    return out


def f32_figures(pkg, orc, name):
    """Worst |dn| of the f32 statement over the checker's precision-32 records against the set's f64 answer on the rays of mapped_set's `use`
    which the f32 checker answers as the f64 one does and whose f32 texel is the f64 one; returns (figures, ray, front_face differences,
    compared, share left out for their texel among the rays otherwise compared)."""
    ms = mapped_set(pkg, orc, name)
    s = ms["base"]
    a = R.ask(orc, s["mesh"].built.desc, s["rays"], precision=32, limit=R.limits(s["rays"]))
    same = s["decidable"] & ~s["edge"] & (s["tri"] >= 0) & a["hit"] & ~R.changed(a, s["ref"])
    tri = np.where(same, s["tri"], -1)
    n, ff, u, v, texel = expected(pkg, ms["mesh"], s["chains"], s["rays"], a, tri, ms["image"], np.float32)
    k = np.flatnonzero(same & ms["use"] & (texel == ms["texel"]))
    left_out = 1.0 - len(k) / max(1, int((same & ms["firm"]).sum()))
    dn = np.linalg.norm(n[k].astype(np.float64) - ms["n"][k], axis=1)
    return dict(n=float(dn.max())), int(k[dn.argmax()]), int((ff[k] != ms["ff"][k]).sum()), len(k), left_out


def lone_set(pkg, orc, T=np.float64):
    """The triangle of `wrapped` that carries the mapped material and no RtTriangleAttrs (no wrapper above it): uv_k = (0,0), (1,0), (0,1)
    and (u, v) the barycentrics. dict(hittable, k = the decidable non-edge rays of the set whose hit lies on it, away from a texel boundary
    (the scene's uv bound) and from grazing the mapped normal (FF_MARGIN), left_out = the share the texel rule left out, n, ff = the answer
    for those rays in T, from the checker's records of that precision)."""
    ms = mapped_set(pkg, orc, "wrapped")
    s, desc = ms["base"], ms["desc"]
    mat = ms["maps"][0].material
    lone = [i for i in range(desc.n_hittables) if desc.hittables[i].kind == pkg._abi.RT_HIT_TRIANGLE and desc.hittables[i].material == mat and i not in ms["mesh"].tris]
    assert len(lone) == 1
    h = lone[0]
    P = {h: np.array(list(desc.hittables[h].p)[:9]).reshape(3, 3)}
    rays, ref = s["rays"], s["ref"]
    ids, on = R.objects_at(pkg, desc, ref["p"], np.zeros(len(rays)), s["mesh"].built.extent)
    mine = s["decidable"] & ~s["edge"] & ref["hit"] & (on.sum(axis=1) == 1) & (ids[on.argmax(axis=1)] == h)
    q = np.flatnonzero(mine)
    n, ff, u, v, texel = pkg.normal_map_reference(P, None, np.full(len(q), h), ref["u"][q], ref["v"][q], ms["image"], d=rays["d"][q].astype(np.float64))
    delta = M.bound_of("wrapped")["uv"]
    steady = np.ones(len(q), bool)
    for su in (-delta, delta):
        for sv in (-delta, delta):
            i, j = pkg.texel_of(u + su, v + sv, MAP_W, MAP_H)
            steady &= (j * MAP_W + i) == texel
    d = rays["d"][q].astype(np.float64)
    firm = np.abs(np.einsum("ij,ij->i", d / np.linalg.norm(d, axis=1, keepdims=True), n)) > FF_MARGIN
    keep = steady & firm
    out = dict(hittable=h, k=q[keep], n=n[keep], ff=ff[keep], left_out=float((~steady).sum()) / max(1, len(q)))
    if T is not np.float64:
        a = R.ask(orc, s["mesh"].built.desc, rays, precision=32, limit=R.limits(rays))
        same = a["hit"] & ~R.changed(a, ref)
        k = out["k"][same[out["k"]]]
        n32, ff32, _, _, tx32 = pkg.normal_map_reference(P, None, np.full(len(k), h), a["u"][k], a["v"][k], ms["image"], dtype=T, d=rays["d"][k])
        _, _, _, _, tx64 = pkg.normal_map_reference(P, None, np.full(len(k), h), ref["u"][k], ref["v"][k], ms["image"])
        sel = tx32 == tx64
        n64 = out["n"][same[out["k"]]][sel]
        out.update(k32=k[sel], dn32=np.linalg.norm(n32[sel].astype(np.float64) - n64, axis=1), ff32_differs=int((ff32[sel] != out["ff"][same[out["k"]]][sel]).sum()))
    return out
