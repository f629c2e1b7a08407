"""Helpers of the radiance-query tests (tests/test_radiance_host.py, tests/test_gpu_radiance.py).

THE LINK TO THE RENDER. A zero-field camera is an RtCamera filled by hand: horizontal = vertical = 0, lens_radius = 0, lower_left_corner =
origin + dir, time0 = time1 = t, with origin, dir and t small dyadic numbers. Every term of new_camera_ray is then exact, and every pixel and
sample of a render traces exactly the ray (origin, dir, t); what differs between samples is the stream (seed, pixel, sample) and the draws the
camera spent on it: 2 for the jitter, 2 per trial of random_in_unit_disk, 1 for the time. draw_counts restates that count from the checker's
RNG stream, with the disk's acceptance test in f32 as tests/features.py::camera_rays forms it. A radiance query over 192 copies of the ray with
first_draw = n0(pixel, sample) and first_stream = 0 must then return the render's samples bit for bit.

BACKGROUND BOUND (background_bound). The sky gradient is three f32 operations on the device: the unit direction's y (|d|^2, a square root, a
division: at most 4 * 2^-24 absolute on |y| <= 1, fast reciprocal forms included), t = 0.5 * (y + 1) (half of that plus one rounding of a sum
in [0, 2]: 3 * 2^-24), and the blend (1 - t) * 1 + t * bg with bg <= 1 (t's error twice, two products and two sums of at most 1 rounded: 1.5 *
2^-24 more): 7.5 * 2^-24, rounded up to 8 * 2^-24 = 4.8e-7 per channel. A constant background is copied: 0."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paths as P  # noqa: E402
import rays as R  # noqa: E402

W, H, SAMPLES = 16, 12, 8
N = W * H
BACKGROUND_BOUND = 8.0 * 2.0 ** -24


def zero_field_camera(pkg, origin, direction, t):
    A = pkg._abi
    cam = A.RtCamera()
    v3 = lambda v: A.RtVec3(float(v[0]), float(v[1]), float(v[2]))
    cam.origin = v3(origin)
    cam.lower_left_corner = v3(np.asarray(origin, float) + np.asarray(direction, float))
    cam.horizontal = cam.vertical = v3((0, 0, 0))
    cam.u, cam.v, cam.w = v3((1, 0, 0)), v3((0, 1, 0)), v3((0, 0, 1))
    cam.lens_radius, cam.time0, cam.time1 = 0.0, float(t), float(t)
    return cam


def draw_count(orc, seed, pixel, sample, n_draws=64):
    """(n0, k, gap): the draws new_camera_ray spends on (seed, pixel, sample) — 2 + 2 k + 1 with k disk trials, the last one accepted — and
    the smallest distance, in f32 ulps of 1 (2^-23), of a trial's px^2 + py^2 from 1."""
    f32 = np.float32
    r = orc.rng_stream(seed, pixel, sample, n_draws)[2]
    k, pos, gap = 0, 2, np.inf
    while True:
        assert pos + 3 <= n_draws, "the disk rejection ran out of draws"
        px, py = f32(-1.0) + f32(2.0) * r[pos], f32(-1.0) + f32(2.0) * r[pos + 1]
        pos += 2
        k += 1
        l2 = f32(f32(px * px) + f32(py * py))
        gap = min(gap, abs(float(l2) - 1.0) / 2.0 ** -23)
        if l2 < f32(1.0):
            return pos + 1, k, gap


_counts = {}


def draw_counts(orc, seed):
    """n0 (N, SAMPLES) uint32, k (N, SAMPLES), and the smallest gap, for every pixel and sample of the W x H frame. Once per seed."""
    if seed not in _counts:
        n0, k, gap = np.zeros((N, SAMPLES), np.uint32), np.zeros((N, SAMPLES), np.int64), np.inf
        for i in range(N):
            for s in range(SAMPLES):
                n0[i, s], k[i, s], g = draw_count(orc, seed, i, s)
                gap = min(gap, g)
        _counts[seed] = (n0, k, gap)
    return _counts[seed]


class Case:
    def __init__(self, name, scene, origin, direction, t=0.0, seed=1, flags=0, layout=0, max_depth=50, tail_paths=0):
        self.name, self.scene, self.origin, self.direction, self.t, self.seed = name, scene, origin, direction, t, seed
        self.flags, self.layout, self.max_depth, self.tail_paths = flags, layout, max_depth, tail_paths


def cases(pkg):
    """The scenes of the exact link, each with a ray aimed at a surface from which light is seen, and the variations of two of them."""
    A = pkg._abi
    cornell = dict(scene="cornell", origin=(278.0, 278.0, 500.0), direction=(-1.0, 0.125, 0.125), seed=7)   # a side wall deep in the box: little of the open front in view
    book1 = dict(scene="book1", origin=(4.0, 3.0, 1.5), direction=(0.25, -1.0, 0.125), flags=A.RT_FLAG_NO_CAMERA_LISTS)
    return [
        Case("cornell", **cornell),
        Case("lights_many", "lights_many", (1.0, 1.5, -0.25), (0.5, -0.75, 0.5), seed=8),                 # the floor between the spheres and the box lamp
        Case("medium", "media", (-1.75, 0.5, 4.0), (0.0, -0.25, -1.0), seed=5),                          # through the dense fog, the floor behind it
        Case("moving", "moving", (0.5, 4.0, 0.5), (0.125, -1.0, 0.25), t=0.375, seed=6),
        Case("book1", seed=3, **book1),                                                                  # the ground sphere: first_in_shade
        Case("smooth_mesh", "smooth_mesh", (-2.0, 0.5, 4.0), (0.0, 0.0, -1.0), seed=4),                   # the textured, smooth-shaded icosphere
        Case("cornell_reference_counters", layout=A.RT_LAYOUT_REFERENCE_COUNTERS, **cornell),
        Case("cornell_scene_in_hbm", layout=A.RT_LAYOUT_SCENE_IN_HBM, **cornell),
        Case("book1_wide_nodes", seed=3, layout=A.RT_LAYOUT_WIDE_NODES, **book1),                        # (the 8-wide tree exists for sphere and mesh scenes with a BVH)
        Case("cornell_never_drain", tail_paths=1, **cornell),
        Case("cornell_depth_8", max_depth=8, **cornell),
    ]


_built = {}


def build(pkg, scene):
    """(desc, attrs, keep) of a case's scene, once per process"""
    if scene not in _built:
        if scene in ("cornell", "book1", "moving"):
            b = R.build_scene(pkg, scene)
            _built[scene] = (b.desc, None, b)
        else:
            b, _ = P.build_scene(pkg, scene, "own")
            _built[scene] = (b.desc, b.attrs, b)
    return _built[scene]


def upload(pkg, ctx, case):
    desc, attrs, _ = build(pkg, case.scene)
    more = dict(triangle_attrs=attrs) if attrs is not None else {}
    return ctx.upload(desc, case.layout, **more)


def lit_scene(pkg):
    return build(pkg, "lights_both")[0]


def varied_rays(pkg, rng, n, lo, hi, timed=True):
    """n PATHRAY rays with origins in the box [lo, hi], directions of every length class between 0.1 and 10, and times in [0, 1]"""
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    d *= (10.0 ** rng.uniform(-1, 1, n) / np.linalg.norm(d, axis=1))[:, None]
    return pkg.path_rays(o, d, time=rng.uniform(0.0, 1.0, n) if timed else 0.0)


def as_query_rays(pkg, rays):
    """the RAY_DTYPE view of PATHRAY rays for trace_rays: the same bytes with t_max = 0 (no limit) where first_draw stands"""
    q = np.zeros(len(rays), dtype=pkg.RAY_DTYPE)
    q["o"], q["d"], q["time"] = rays["o"], rays["d"], rays["time"]
    return q


def emitted(pkg, desc, hits):
    """Per ray of a trace_rays result: what `emitted` returns at the hit — a DiffuseLight's solid colour on the front face, else 0"""
    A = pkg._abi
    out = np.zeros((len(hits), 3))
    hit = (hits["flags"] & A.RT_RAYHIT_HIT) != 0
    ff = (hits["flags"] & A.RT_RAYHIT_FRONT_FACE) != 0
    for m in sorted(set(int(x) for x in hits["material"][hit])):
        mat = desc.materials[m]
        if mat.kind == A.RT_MAT_DIFFUSE_LIGHT:
            tex = desc.textures[mat.texture]
            assert tex.kind == A.RT_TEX_SOLID
            out[hit & ff & (hits["material"] == m)] = tex.color.tuple()
    return out


def furnace(pkg, radiance=2.0, albedo=0.5, half=2.0):
    """A closed cube of Lambertian walls whose floor is an emitter (front face up, towards the inside); no other light, no lights list"""
    b = pkg.SceneBuilder(background=(0.0, 0.0, 0.0))
    wall, lamp, h = b.lambertian((albedo,) * 3), b.diffuse_light((radiance,) * 3), half
    ids = [b.xz_rect(-h, h, -h, h, -h, lamp), b.xz_rect(-h, h, -h, h, h, wall), b.xy_rect(-h, h, -h, h, -h, wall), b.xy_rect(-h, h, -h, h, h, wall),
           b.yz_rect(-h, h, -h, h, -h, wall), b.yz_rect(-h, h, -h, h, h, wall)]
    return b.desc(b.hittable_list(ids)), b


def mean_z(S1, Q1, S2, Q2, n1, n2):
    """(mean z, N) over the values whose variance is not 0 on at least one side, z = (mean1 - mean2) / sqrt(se1^2 + se2^2), in f64; and the mask
    of the values with zero variance on both sides"""
    S1, Q1, S2, Q2 = (np.asarray(a, np.float64).reshape(-1) for a in (S1, Q1, S2, Q2))
    v1 = np.maximum(Q1 - S1 * S1 / n1, 0.0) / (n1 * (n1 - 1.0))
    v2 = np.maximum(Q2 - S2 * S2 / n2, 0.0) / (n2 * (n2 - 1.0))
    some = (v1 + v2) > 0.0
    z = (S1[some] / n1 - S2[some] / n2) / np.sqrt(v1[some] + v2[some])
    return float(z.mean()), int(some.sum()), ~some
