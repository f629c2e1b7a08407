"""Scenes, query points and closed forms shared by the light-sampling tests (test_lights_host.py, test_gpu_lights.py).

QUERY CASES (rt_sample_lights against light_reference): a lights list a few units above a cloud of points; every case keeps the share of
queries that are undecidable in f64 under 2 % (checked on the CPU). EMITTER CASES (direct lighting against Lambert's form factor): one
emitter above a grey floor, seen by a camera that looks down at the floor only, and by one that looks at the emitter's front."""
import json
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_QUERIES = 4096
COS_MIN, EDGE_MIN = 1e-2, 1e-4          # a query is undecidable in f64 below these (cosine at a light; distance of a crossing from an edge)
SKIP_SHARE = 0.02

TRI = ((-1.0, 2.5, -1.0), (1.2, 3.0, -0.5), (0.0, 2.2, 1.3))
QUERY_CASES = ("xy_rect", "xz_rect", "yz_rect", "triangle", "box", "wrapped_rect", "wrapped_triangle", "icosphere", "mixed")


def query_case(pkg, name):
    """(desc, builder, (lo, hi) of the points' box). The lights are in the world too, as emitters."""
    b = pkg.SceneBuilder()
    lamp, grey = b.diffuse_light((4.0, 4.0, 4.0)), b.lambertian((0.7, 0.7, 0.7))
    box = ((-2.0, -1.0, -2.0), (2.0, 1.0, 2.0))
    if name == "xy_rect":
        lights, box = [b.xy_rect(-1.0, 1.0, 0.5, 2.0, 3.0, lamp)], ((-2.0, -1.0, -2.0), (2.0, 1.0, 1.0))
    elif name == "xz_rect":
        lights = [b.xz_rect(-1.0, 1.0, -1.0, 1.0, 3.0, lamp)]
    elif name == "yz_rect":
        lights, box = [b.yz_rect(0.0, 2.0, -1.0, 1.0, 3.0, lamp)], ((-2.0, -1.0, -2.0), (1.0, 1.0, 2.0))
    elif name == "triangle":
        lights = [b.triangle(*TRI, lamp)]
    elif name == "box":
        lights = [b.box((-0.5, 2.0, -0.5), (0.7, 3.0, 0.6), lamp)]
    elif name == "wrapped_rect":
        lights = [b.translate(b.rotate_y(b.xz_rect(-1.0, 1.0, -1.0, 1.0, 0.0, lamp), 30.0), (0.5, 3.0, 0.2))]
    elif name == "wrapped_triangle":
        lights = [b.flip_face(b.rotate_y(b.translate(b.triangle(*TRI, lamp), (0.3, 0.0, 0.0)), -40.0))]
    elif name == "icosphere":
        tris, _ = pkg.icosphere(0)
        lights = [b.triangle(*(0.8 * t + np.array([0.0, 3.0, 0.0])), lamp) for t in tris]
    elif name == "mixed":
        lights = [b.xy_rect(-1.0, 1.0, 2.0, 3.0, 3.0, lamp), b.triangle(*TRI, lamp), b.box((1.5, 2.0, -1.5), (2.5, 2.8, -0.5), lamp),
                  b.sphere((-2.0, 3.0, 0.0), 0.5, lamp), b.translate(b.rotate_y(b.yz_rect(2.0, 3.0, -0.5, 0.5, 0.0, lamp), 20.0), (-1.0, 0.0, 2.5))]
    else:
        raise KeyError(name)
    floor = b.xz_rect(-50.0, 50.0, -50.0, 50.0, -2.0, grey)
    world = b.hittable_list([floor] + lights)
    desc = b.desc(world, b.hittable_list(lights), lights_all_shapes=True)
    return desc, b, box


def query_points(name, box, n=N_QUERIES):
    """(points f32 (n, 3), states u64 (n)): seeded by the case's name, the same on every run"""
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    lo, hi = np.array(box[0]), np.array(box[1])
    pts = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    states = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    return pts, states


def decidable(ref64):
    return (ref64["cos_min"] >= COS_MIN) & (ref64["edge_min"] >= EDGE_MIN) & np.isfinite(ref64["pdf"])


def deviations(pkg, desc, pts, states):
    """(ref64, keep, dev_d, dev_pdf): the f64 yardstick, the decidable queries, and how far the f32 restatement moves d (relative to |d|) and
    pdf (relative) on them — the figures the device's bound is twice of."""
    r64 = pkg.light_reference(desc, pts, states, dtype=np.float64)
    r32 = pkg.light_reference(desc, pts, states, dtype=np.float32)
    keep = decidable(r64)
    assert (r32["light"] == r64["light"]).all() and (r32["n_draws"] == r64["n_draws"]).all()
    dd = np.linalg.norm(r32["d"].astype(np.float64) - r64["d"], axis=1) / np.linalg.norm(r64["d"], axis=1)
    dp = np.abs(r32["pdf"].astype(np.float64) - r64["pdf"]) / r64["pdf"]
    return r64, keep, float(dd[keep].max()), float(dp[keep].max())


# ---- direct lighting: one emitter above a floor ------------------------------------------------------------------------------------------------
ALBEDO, LE = 0.7, 4.0
EMITTER_CASES = ("triangle", "xy_rect", "yz_rect", "wrapped_xz_rect", "box", "icosphere")
FRAME, SPP = 32, 256
CAM_FLOOR = ((0.0, 3.0, -2.0), (0.0, 0.0, 0.0))          # looks down at the floor, 36 to 76 degrees below the horizon: every emitter (y >= 1.9, z >= 0) is above its view


def _roty(v, degrees):
    """RotateY's local -> world map (hittable.rs:166-167)"""
    s, c = math.sin(math.radians(degrees)), math.cos(math.radians(degrees))
    v = np.asarray(v, float)
    return np.stack([c * v[..., 0] + s * v[..., 2], v[..., 1], -s * v[..., 0] + c * v[..., 2]], axis=-1)


def emitter_case(pkg, name):
    """(desc, builder, faces, view): faces = the polygons (k, 3) that emit, each wound so that its FRONT (the side a DiffuseLight emits to) is
    the side from which it appears counter-clockwise; for a closed body only the faces whose front is the outside (the others are hidden from
    every outside point by the body itself). view = a camera position on the emitter's front side and the point it looks at."""
    b = pkg.SceneBuilder()
    lamp, grey = b.diffuse_light((LE, LE, LE)), b.lambertian((ALBEDO, ALBEDO, ALBEDO))
    if name == "triangle":
        v = [np.array(x) for x in ((-1.0, 2.6, 0.2), (1.1, 3.0, 0.0), (0.2, 2.2, 1.6))]      # cross(v1 - v0, v2 - v0) points down: the front faces the floor
        world_l = lights = [b.triangle(*v, lamp)]
        faces, view = [np.array(v)], ((0.1, 0.3, -0.4), (0.1, 2.6, 0.6))
    elif name == "xy_rect":                                                                    # front: the +z side (hit with d.z < 0)
        world_l = lights = [b.xy_rect(-1.0, 1.0, 2.0, 3.0, 0.3, lamp)]
        faces, view = [np.array([(-1.0, 2.0, 0.3), (1.0, 2.0, 0.3), (1.0, 3.0, 0.3), (-1.0, 3.0, 0.3)])], ((0.0, 2.5, 3.5), (0.0, 2.5, 0.3))
    elif name == "yz_rect":                                                                    # front: the +x side
        world_l = lights = [b.yz_rect(2.0, 3.0, 0.0, 2.0, -0.4, lamp)]
        faces, view = [np.array([(-0.4, 2.0, 0.0), (-0.4, 3.0, 0.0), (-0.4, 3.0, 2.0), (-0.4, 2.0, 2.0)])], ((3.0, 2.5, 1.0), (-0.4, 2.5, 1.0))
    elif name == "wrapped_xz_rect":
        # Translate::hit ends with set_face_normal on the normal RotateY has already turned against the ray (hittable.rs:82-83, 173): front_face comes
        # out true from either side, so a light under Translate emits to both sides — and under FlipFace(Translate(..)) to neither. It goes into
        # the world as it is; both windings of the rect are faces, and a point sees the front of exactly one.
        inner = b.translate(b.rotate_y(b.xz_rect(-1.0, 1.0, -0.6, 0.6, 0.0, lamp), 30.0), (0.2, 2.4, 1.0))
        world_l = lights = [inner]
        local = np.array([(-1.0, 0.0, -0.6), (1.0, 0.0, -0.6), (1.0, 0.0, 0.6), (-1.0, 0.0, 0.6)])
        face = _roty(local, 30.0) + np.array([0.2, 2.4, 1.0])
        faces, view = [face, face[::-1].copy()], ((0.2, 0.3, 0.0), (0.2, 2.4, 1.0))
    elif name == "box":
        # the sides of a Box are rects with +axis normals (boxes.rs:17-74): seen from outside, the x1, y1 and z1 sides show their front, the
        # x0, y0, z0 sides their back (and hide the fronts behind them)
        p0, p1 = (-0.6, 2.0, 0.2), (0.6, 2.8, 1.4)
        world_l = lights = [b.box(p0, p1, lamp)]
        (x0, y0, z0), (x1, y1, z1) = p0, p1
        faces = [np.array([(x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)]), np.array([(x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)]),
                 np.array([(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)])]
        view = ((3.0, 4.5, 3.8), (0.0, 2.4, 0.8))
    elif name == "icosphere":
        tris, _ = pkg.icosphere(0)                                                             # wound counter-clockwise seen from outside
        tris = 0.7 * tris + np.array([0.0, 2.6, 0.9])
        world_l = lights = [b.triangle(*t, lamp) for t in tris]
        faces, view = [t for t in tris], ((0.0, 2.6, 4.5), (0.0, 2.6, 0.9))
    else:
        raise KeyError(name)
    floor = b.xz_rect(-60.0, 60.0, -60.0, 60.0, 0.0, grey)
    desc = b.desc(b.hittable_list([floor] + world_l), b.hittable_list(lights), lights_all_shapes=True)
    return desc, b, faces, view


def camera(pkg, lookfrom, lookat, vfov=40.0):
    return pkg.camera_new(lookfrom, lookat, (0, 1, 0), vfov, 1.0, 0.0, float(np.linalg.norm(np.subtract(lookfrom, lookat))), 0.0, 0.0)


def form_factor(p, faces):
    """Lambert's polygon form factor of `faces` from the points p (m, 3) of the floor (normal +y): (1 / 2 pi) sum over the edges of gamma_i n . Gamma_i,
    per face, counted only where the face shows p its front. Every face lies above the floor, so no horizon clipping is needed."""
    p = np.asarray(p, float)
    n = np.array([0.0, 1.0, 0.0])
    total = np.zeros(p.shape[0])
    for V in faces:
        V = np.asarray(V, float)
        normal = np.cross(V[1] - V[0], V[2] - V[0])
        front = (V[0] - p) @ normal < 0.0                        # p on the side the normal points to
        R = V[None, :, :] - p[:, None, :]
        R = R / np.linalg.norm(R, axis=2, keepdims=True)
        F = np.zeros(p.shape[0])
        for i in range(V.shape[0]):
            a, c = R[:, i], R[:, (i + 1) % V.shape[0]]
            gamma = np.arccos(np.clip(np.einsum("ij,ij->i", a, c), -1.0, 1.0))
            g = np.cross(a, c)
            g = g / np.linalg.norm(g, axis=1, keepdims=True)
            F += gamma * (g @ n)
        # (the sign of the sum follows the winding as p sees it; the form factor is its magnitude)
        total += np.where(front, np.abs(F) / (2.0 * math.pi), 0.0)
    return total


def expected_frame(cam, faces, sub):
    """albedo * Le * F per pixel of the FRAME x FRAME image, F averaged over a sub x sub grid of the pixel's footprint: the camera's own ray formula
    (camera.rs:61-71 with aperture 0; u = (x + r) / (W - 1), v = (H - 1 - y + r) / (H - 1), main.rs:752-753), met with the floor y = 0."""
    W = H = FRAME
    o = np.array(cam.origin.tuple())
    llc, hor, ver = np.array(cam.lower_left_corner.tuple()), np.array(cam.horizontal.tuple()), np.array(cam.vertical.tuple())
    r = (np.arange(sub) + 0.5) / sub
    ys, xs, ry, rx = np.meshgrid(np.arange(H), np.arange(W), r, r, indexing="ij")
    u, v = (xs + rx) / (W - 1), (H - 1 - ys + ry) / (H - 1)
    d = llc + u[..., None] * hor + v[..., None] * ver - o
    t = -o[1] / d[..., 1]
    assert (d[..., 1] < 0).all()
    p = o + t[..., None] * d
    F = form_factor(p.reshape(-1, 3), faces).reshape(H, W, sub * sub)
    return ALBEDO * LE * F.mean(axis=2)


def z_scores(rgb_sum, sq_sum, expected, spp, channel=0):
    """(z, se): z = (mean - expected) / SE per pixel on one channel; a pixel without variance has z = 0 where its mean is the expected value
    (to 1e-6) and inf where it is not."""
    S, Q = rgb_sum[..., channel].astype(np.float64), sq_sum[..., channel].astype(np.float64)
    mean = S / spp
    se = np.sqrt(np.maximum(Q - S * S / spp, 0.0) / (spp * (spp - 1.0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(se > 0.0, (mean - expected) / se, np.where(np.abs(mean - expected) <= 1e-6, 0.0, np.inf))
    return z, se


def check_z(z):
    """|mean z| <= 6 / sqrt(N) (the mean of N unit normals has sd 1 / sqrt(N)) and at most 1 % of the pixels beyond |z| = 4. A pixel whose z is
    not finite (no variance, and a mean that is not the expected value) counts as beyond 4; the mean is taken over the finite ones."""
    n = z.size
    fin = np.isfinite(z)
    return bool(fin.any()) and abs(float(z[fin].mean())) <= 6.0 / math.sqrt(n) and float(((np.abs(z) > 4.0) | ~fin).mean()) <= 0.01


def surely_dark(expected):
    """pixels whose own footprint and whose eight neighbours' show no front face on the sub-grid: a pixel next to a lit one may catch light in the
    sliver of its footprint beyond the outermost sub-sample"""
    dark = np.pad(expected == 0.0, 1, mode="edge")
    out = np.ones_like(expected, dtype=bool)
    for dy in range(3):
        for dx in range(3):
            out &= dark[dy:dy + expected.shape[0], dx:dx + expected.shape[1]]
    return out


# ---- the Cornell box with its lamp as the reference's rect, or as two triangles ---------------------------------------------------------------
def cornell_doc(lamp_as_triangles):
    doc = json.load(open(os.path.join(ROOT, "examples", "cornell_box.json")))
    if lamp_as_triangles:
        # the lamp's rectangle as two triangles whose front (the side cross(v1 - v0, v2 - v0) points to) faces the floor, as FlipFace(XzRect) does
        doc["objects"]["lamp_a"] = {"triangle": [[213, 554, 227], [343, 554, 332], [213, 554, 332]], "material": "light"}
        doc["objects"]["lamp_b"] = {"triangle": [[213, 554, 227], [343, 554, 227], [343, 554, 332]], "material": "light"}
        doc["world"] = {"list": ["left", "right", "lamp_a", "lamp_b", "floor", "ceiling", "back", "block_placed", "ball"]}
        doc["lights"] = ["lamp_a", "lamp_b", "light_ball"]
        doc["lights_all_shapes"] = True
    return doc


def frame_z(S1, Q1, S2, Q2, spp):
    """per pixel and channel z of the difference of two renders' means, from both renders' squared sums"""
    S1, Q1, S2, Q2 = (np.asarray(a, np.float64) for a in (S1, Q1, S2, Q2))
    v1 = np.maximum(Q1 - S1 * S1 / spp, 0.0) / (spp * (spp - 1.0))
    v2 = np.maximum(Q2 - S2 * S2 / spp, 0.0) / (spp * (spp - 1.0))
    se = np.sqrt(v1 + v2)
    d = S1 / spp - S2 / spp
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(se > 0, d / se, np.where(d == 0, 0.0, np.inf))
