"""Scenes, ray sets and bounds for the triangle-attribute tests (tests/test_mesh_attrs_host.py, tests/test_gpu_mesh_attrs.py): meshes whose
triangles carry per-vertex normals and texture coordinates (include/rt_hip.h RtTriangleAttrs), per scene a fixed list of f32 rays — a camera
fan plus random point-to-point segments — and for every ray the f64 answer: the CPU checker's world.hit (t, p, the barycentrics it reports
as u, v, and — through tests/rays.py objects_at — the triangle the point lies on), put through mesh.interpolate_reference at f64 and the
wrapper replay below. Decidability is tests/rays.py's R-ulp rule, imported, applied to the checker's answer AND to the interpolated
front_face; an EDGE ray is one whose hit point lies on more than one primitive (which triangle reports it, and with it n, u, v, is either
side's to choose). Nothing here comes from a GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays as R  # noqa: E402

SCENES = ["ico1", "ico2", "big", "wrapped"]
FAN = (48, 32)                 # camera rays: pixel centres of a 48 x 32 frame
N_SEGMENTS = 4096 - FAN[0] * FAN[1]
# The numpy restatement at f32 over the checker's precision-32 records against the same at f64 over its precision-64 records, on the
# decidable non-edge rays both instances answer alike: worst |dn| and worst |d(u, v)| per scene. What plain f32 arithmetic costs here; the
# device is allowed 2 x each figure (the project's factor: tests/rays.py bound_of). Produced on a CPU by
#     python -m pytest tests/test_mesh_attrs_host.py -k f32_figures -s
# which measures them again and holds them to this table within 1 %.
MEASURED_F32 = {
    "ico1": dict(n=1.192e-06, uv=6.441e-07),
    "ico2": dict(n=1.519e-06, uv=6.003e-07),
    "big": dict(n=2.897e-07, uv=1.501e-07),
    "wrapped": dict(n=3.257e-06, uv=1.751e-06),
}
BIG_UV = ((0.2, 0.1), (0.9, 0.3), (0.4, 0.8))
# the large triangle's facet normal is +z; its vertex normals lean 45, 50 and 53 degrees away from it, each another way, none of unit length
BIG_NORMALS = ((2.1, 0.0, 2.1), (-0.5, 0.68, 0.7), (0.0, -2.4, 1.8))
BIG_VERTS = ((-3.0, -2.0, 0.0), (3.0, -2.0, 0.0), (0.0, 3.0, 0.0))
WRAP = dict(offset=(-0.5, 0.2, 0.3), degrees=30.0)


def bound_of(name):
    return {q: 2.0 * v for q, v in MEASURED_F32[name].items()}


class Mesh:
    """A scene (rays.Built), its RtTriangleAttrs array (None: none), and {hittable id: (3, 3) vertices} of the triangles that carry some."""
    def __init__(self, built, attrs, tris):
        self.built, self.attrs, self.tris = built, attrs, tris


def add_sphere_mesh(pkg, b, subdivisions, mat, smooth=True, textured=True, tris_out=None):
    """The unit icosphere's triangles with sphere normals and the sphere's own (u, v) at the vertices; returns their hittable ids."""
    tris, nrm = pkg.icosphere(subdivisions)
    uv = pkg.sphere_uv(nrm)
    ids = []
    for k in range(len(tris)):
        ids.append(b.triangle(tris[k][0], tris[k][1], tris[k][2], mat, normals=nrm[k] if smooth else None, uvs=uv[k] if textured else None))
        if tris_out is not None:
            tris_out[ids[-1]] = tris[k]
    return ids


def build_scene(pkg, name, smooth=True, textured=True):
    A = pkg._abi
    b = pkg.SceneBuilder(background=(0.5, 0.7, 1.0), background_mode=A.RT_BG_SKY_GRADIENT)
    tris = {}
    grey = b.lambertian((0.6, 0.6, 0.6))
    if name in ("ico1", "ico2"):
        world = b.bvh(add_sphere_mesh(pkg, b, 1 if name == "ico1" else 2, grey, smooth, textured, tris))
        cam, extent = pkg.camera_new((0.3, 0.4, 4.0), (0, 0, 0), (0, 1, 0), 32.0, 1.5, 0.0, 4.0, 0.0, 0.0), 1.0
    elif name == "big":
        t = b.triangle(*BIG_VERTS, grey, normals=BIG_NORMALS if smooth else None, uvs=BIG_UV if textured else None)
        tris[t] = np.array(BIG_VERTS)
        world = b.hittable_list([t])
        cam, extent = pkg.camera_new((0.5, 0.3, 6.0), (0, 0, 0), (0, 1, 0), 50.0, 1.5, 0.0, 6.0, 0.0, 0.0), 3.0
    elif name == "wrapped":
        # the subdivision-1 mesh under Translate(RotateY(FlipFace(.))), beside a sphere, rects and triangles WITHOUT attributes: the
        # all-features instance. No two surfaces meet.
        mesh = b.translate(b.rotate_y(b.flip_face(b.bvh(add_sphere_mesh(pkg, b, 1, grey, smooth, textured, tris))), WRAP["degrees"]), WRAP["offset"])
        red = b.lambertian((0.7, 0.2, 0.2))
        others = [b.sphere((2.6, 0.0, 0.0), 0.8, b.metal((0.8, 0.8, 0.8), 0.0)), b.xz_rect(-4.0, 4.0, -4.0, 4.0, -1.6, red), b.xy_rect(-4.0, 4.0, -1.6, 3.0, -3.0, red),
                  b.triangle((-3.5, -1.0, -1.0), (-2.0, -1.0, 0.5), (-2.8, 1.5, -0.4), red), b.triangle((-3.4, 2.0, -2.0), (3.0, 2.2, -2.2), (0.0, 2.9, -1.0), grey)]
        world = b.hittable_list([mesh] + others)
        cam, extent = pkg.camera_new((0.4, 0.6, 6.0), (0, 0, 0), (0, 1, 0), 50.0, 1.5, 0.0, 6.0, 0.0, 0.0), 4.0
    else:
        raise ValueError(name)
    return Mesh(R.Built(b.desc(world), cam, b, extent), b.triangle_attrs(), tris)


def make_rays(built, rng, centre=(0.0, 0.0, 0.0), radius=None):
    """The camera fan, then N_SEGMENTS point-to-point rays d = q - p with t_max = 1, all rounded to f32: three quarters between points of the
    box of half-width 1.6 radius about `centre` (the mesh with attributes; radius None: the scene's extent) — every other one starts well
    inside it, so a closed mesh of that size shows its back faces too — and a quarter between points of the whole scene's box."""
    fan = R.camera_rays(built.cam, FAN[0], FAN[1], rng)
    r = built.extent if radius is None else radius
    p = rng.uniform(-1.6, 1.6, (N_SEGMENTS, 3)) * r
    q = rng.uniform(-1.6, 1.6, (N_SEGMENTS, 3)) * r
    p[::2] *= 0.3
    p, q = p + np.asarray(centre), q + np.asarray(centre)
    wide = np.arange(N_SEGMENTS) % 4 == 3
    p[wide] = rng.uniform(-1.6, 1.6, (int(wide.sum()), 3)) * built.extent
    q[wide] = rng.uniform(-1.6, 1.6, (int(wide.sum()), 3)) * built.extent
    return np.concatenate([fan, R.make_rays(p, q - p, np.zeros(N_SEGMENTS), 1.0)])


def rot_y(v, degrees, back, T):
    """RotateY's map of a direction to its child's space (hittable.rs:154-155), or of a normal back to its own (:169-170), in T."""
    th = np.radians(degrees)
    c, s = T(np.cos(th)), T(np.sin(th))
    if back:
        return np.stack([c * v[:, 0] + s * v[:, 2], v[:, 1], -s * v[:, 0] + c * v[:, 2]], axis=1).astype(T)
    return np.stack([c * v[:, 0] - s * v[:, 2], v[:, 1], s * v[:, 0] + c * v[:, 2]], axis=1).astype(T)


def local_directions(pkg, chain, d, T):
    """The ray direction every wrapper of `chain` (outermost first) hands to its child; the last one is the triangle's own."""
    A = pkg._abi
    dk = [np.asarray(d).astype(T)]
    for kind, prm in chain:
        dk.append(rot_y(dk[-1], prm[0], False, T) if kind == A.RT_HIT_ROTATE_Y else dk[-1])
    return dk


def replay(pkg, chain, dk, n, ff, T):
    """What the wrappers make of the child's (normal, front_face) on the way out, innermost first: Translate and RotateY call
    set_face_normal again — RotateY with the ray of its child space against the normal it has rotated back (hittable.rs:82-83, 169-173) —
    and FlipFace negates front_face (:199). The statement the library replays op by op (csrc/device_types.h Wrap)."""
    A = pkg._abi
    n, ff = n.copy(), ff.copy()
    for k in range(len(chain) - 1, -1, -1):
        kind, prm = chain[k]
        if kind == A.RT_HIT_FLIP_FACE:
            ff = ~ff
            continue
        if kind == A.RT_HIT_ROTATE_Y:
            n = rot_y(n, prm[0], True, T)
        c = dk[k + 1]
        ff = (c[:, 0] * n[:, 0] + c[:, 1] * n[:, 1] + c[:, 2] * n[:, 2]).astype(T) < 0
        n = np.where(ff[:, None], n, -n)
    return n, ff


def expected(pkg, mesh, chains, rays, ans, tri, T):
    """(n, ff, u, v) for the rays whose hit lies on attribute triangle tri[i] >= 0 (other rows: the checker's own), from the checker's
    records `ans` (R.ask: its u, v on a triangle are the barycentrics), every operation in T."""
    n, ff, u, v = ans["n"].astype(T), ans["ff"].copy(), ans["u"].astype(T), ans["v"].astype(T)
    k = np.flatnonzero(tri >= 0)
    if len(k) == 0:
        return n, ff, u, v
    for chain in {tuple(map(lambda w: (w[0], tuple(w[1])), chains[int(h)])) for h in np.unique(tri[k])}:
        chain = list(chain)
        m = k[[tuple(map(lambda w: (w[0], tuple(w[1])), chains[int(h)])) == tuple(chain) for h in tri[k]]]
        dk = local_directions(pkg, chain, rays["d"][m], T)
        nl, fl, u[m], v[m] = pkg.interpolate_reference(mesh.tris, mesh.attrs, tri[m], ans["u"][m], ans["v"][m], dk[-1], T)
        n[m], ff[m] = replay(pkg, chain, dk, nl, fl, T)
    return n, ff, u, v


_cache = {}


def ray_set(pkg, orc, name):
    """dict(mesh, rays, ref, tri, edge, decidable, n, ff, u, v), computed once per process. ref: the checker's f64 records; tri: the
    attribute triangle the hit lies on (-1: none, a miss or an edge ray); n, ff, u, v: the f64 answer (expected()); decidable: the R-ulp
    rule on the checker's answer and on the interpolated front_face."""
    if name in _cache:
        return _cache[name]
    mesh = build_scene(pkg, name)
    built = mesh.built
    rays = make_rays(built, np.random.default_rng(1000 + SCENES.index(name)), *((WRAP["offset"], 1.0) if name == "wrapped" else ()))
    ref = R.ask(orc, built.desc, rays)
    chains = {i: chain for i, _, chain in R.primitives(pkg, built.desc)}

    def on_triangle(ans):
        ids, on = R.objects_at(pkg, built.desc, ans["p"], np.zeros(len(rays)), built.extent)
        edge = ans["hit"] & (on.sum(axis=1) != 1)
        hid = ids[on.argmax(axis=1)]
        return np.where(ans["hit"] & ~edge & np.isin(hid, list(mesh.tris)), hid, -1), edge
    tri, edge = on_triangle(ref)
    n, ff, u, v = expected(pkg, mesh, chains, rays, ref, tri, np.float64)
    und = R.undecidable(orc, built.desc, rays, ref)
    # the same perturbations, for the answer the attributes decide: front_face of the interpolated normal
    d = rays["d"]
    ulp = np.where(np.abs(d) < np.float32(R.SMALL), np.spacing(np.abs(d).max(axis=1, keepdims=True)), np.spacing(np.abs(d)))
    step = np.float32(R.R_ULPS) * ulp.astype(np.float32)
    for s in R.SIGNS:
        q = rays.copy()
        q["d"] = d + np.asarray(s, np.float32) * step
        a = R.ask(orc, built.desc, q)
        t2, _ = on_triangle(a)
        _, ff2, _, _ = expected(pkg, mesh, chains, q, a, t2, np.float64)
        und |= (tri >= 0) & ((t2 < 0) | (ff2 != ff))
    _cache[name] = dict(mesh=mesh, chains=chains, rays=rays, ref=ref, tri=tri, edge=edge, decidable=~und, n=n, ff=ff, u=u, v=v)
    return _cache[name]


def f32_figures(pkg, orc, name):
    """Worst |dn| and |d(u, v)| of the f32 restatement over the checker's precision-32 records against the set's f64 answer, on the decidable
    non-edge hits on attribute triangles which the f32 checker answers as the f64 one does (rays.changed sees no difference)."""
    s = ray_set(pkg, orc, name)
    a = R.ask(orc, s["mesh"].built.desc, s["rays"], precision=32, limit=R.limits(s["rays"]))
    k = s["decidable"] & (s["tri"] >= 0) & a["hit"] & ~R.changed(a, s["ref"])
    tri = np.where(k, s["tri"], -1)
    n, ff, u, v = expected(pkg, s["mesh"], s["chains"], s["rays"], a, tri, np.float32)
    k = np.flatnonzero(k)
    dn = np.linalg.norm(n[k].astype(np.float64) - s["n"][k], axis=1)
    duv = np.maximum(np.abs(u[k].astype(np.float64) - s["u"][k]), np.abs(v[k].astype(np.float64) - s["v"][k]))
    return dict(n=float(dn.max()), uv=float(duv.max())), dict(n=int(k[dn.argmax()]), uv=int(k[duv.argmax()])), int((ff[k] != s["ff"][k]).sum()), len(k)


# ---- the render scenes of tests/test_gpu_mesh_attrs.py ----------------------------------------------------------------------------------
def textured_scene(pkg, earth, mode):
    """Lambertian triangles under a checker, a noise and the earth image texture, and a DiffuseLight triangle. mode: None = no attributes,
    "identity" = uv (0,0), (1,0), (0,1) on every triangle, "flags0" = a record with flags 0 for every triangle. Returns (desc, camera,
    attrs, keep)."""
    A = pkg._abi
    b = pkg.SceneBuilder(background=(0.05, 0.05, 0.08))
    mats = [b.lambertian(texture=b.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))), b.lambertian(texture=b.noise(4.0, np.random.default_rng(5))),
            b.lambertian(texture=b.image(earth)), b.diffuse_light((4.0, 4.0, 4.0))]
    rng = np.random.default_rng(11)
    ids = []
    for k in range(24):
        c = np.array([(k % 6) - 2.5, (k // 6) - 1.5, -0.2 * (k % 5)]) * 1.1
        v = c + rng.uniform(-1.0, 1.0, (3, 3)) * np.array([1.0, 1.0, 0.3])
        if np.cross(v[1] - v[0], v[2] - v[0])[2] < 0:
            v = v[[0, 2, 1]]                                   # all face the camera: the light emits towards it
        ids.append(b.triangle(v[0], v[1], v[2], mats[3 if k == 9 else k % 3], uvs=((0, 0), (1, 0), (0, 1)) if mode == "identity" else None))
    desc = b.desc(b.bvh(ids))
    attrs = b.triangle_attrs()
    if mode == "flags0":
        attrs = (A.RtTriangleAttrs * len(ids))(*[A.RtTriangleAttrs(i, 0) for i in ids])
    return desc, pkg.camera_new((0, 0, 7.0), (0, 0, 0), (0, 1, 0), 40.0, 1.5, 0.0, 7.0, 0.0, 0.0), attrs, b


def rect_pair_scene(pkg, earth, as_mesh):
    """An XyRect at z = 0 with the earth-image Lambertian, seen from z = -5 (its back: a Lambertian scatters on either side), and a second
    XyRect at z = -8, behind the camera, as DiffuseLight: a ray that leaves the picture towards it travels in -z and meets the light's front
    (an XyRect's normal is +z). as_mesh: each rect as two triangles that carry the rect's corner (u, v) and its normal (0, 0, 1) — the same
    surface, affine interpolation being exact. The light's triangles are wound the OTHER way (geometric normal (0, 0, -1)): by their
    geometry they would show the scene their back and emit nothing; only the vertex normals make them emit towards it."""
    b = pkg.SceneBuilder(background=(0.02, 0.02, 0.03))
    img, lamp = b.lambertian(texture=b.image(earth)), b.diffuse_light((6.0, 6.0, 6.0))

    def rect(x0, x1, y0, y1, k, mat, flip):
        if not as_mesh:
            return [b.xy_rect(x0, x1, y0, y1, k, mat)]
        P = {(0, 0): (x0, y0, k), (1, 0): (x1, y0, k), (1, 1): (x1, y1, k), (0, 1): (x0, y1, k)}
        out = []
        for c in (((0, 0), (1, 0), (1, 1)), ((0, 0), (1, 1), (0, 1))):
            c = (c[0], c[2], c[1]) if flip else c
            out.append(b.triangle(P[c[0]], P[c[1]], P[c[2]], mat, normals=[(0, 0, 1)] * 3, uvs=[(float(u), float(v)) for u, v in c]))
        return out
    ids = rect(-2.0, 2.0, -1.5, 1.5, 0.0, img, False) + rect(-4.0, 4.0, -3.0, 4.0, -8.0, lamp, True)
    desc = b.desc(b.hittable_list(ids))
    return desc, pkg.camera_new((0, 0.2, -5.0), (0, 0.2, 0), (0, 1, 0), 50.0, 64 / 48, 0.0, 5.0, 0.0, 0.0), b.triangle_attrs(), b


def sphere_scene(pkg, kind):
    """The unit sphere as Metal (fuzz 0) under the sky gradient, seen from (0, 0, 4) at vfov 14.8 degrees (half-slope 0.13: the sphere
    fills the frame, incidence <= 46 degrees). kind: "sphere" = the true Sphere, "flat" = the subdivision-2 icosphere, "smooth" = that mesh
    with sphere normals."""
    A = pkg._abi
    b = pkg.SceneBuilder(background=(0.5, 0.7, 1.0), background_mode=A.RT_BG_SKY_GRADIENT)
    m = b.metal((0.9, 0.9, 0.9), 0.0)
    if kind == "sphere":
        world = b.hittable_list([b.sphere((0, 0, 0), 1.0, m)])
    else:
        world = b.bvh(add_sphere_mesh(pkg, b, 2, m, smooth=kind == "smooth", textured=False))
    return b.desc(world), pkg.camera_new((0, 0, 4.0), (0, 0, 0), (0, 1, 0), 14.8, 1.0, 0.0, 4.0, 0.0, 0.0), b.triangle_attrs(), b
