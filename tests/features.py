"""Helpers of the first-hit feature tests (tests/test_features_host.py, tests/test_gpu_features.py): the renderer's camera ray restated in
numpy from the checker's RNG stream, the scenes, and the expected per-pixel features formed from a ray-query hit list.

The rays are built in f64 from the stream's f32 draws (the device's own uniform numbers, exact in f64) and rounded to f32: they differ
from the device's f32 construction by a few ulps, which rays.undecidable (R = 64 ulps) covers."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays as R  # noqa: E402

SCENES = R.SCENES + ["textured"]
GRID = R.GRID
SEED = 5
# The yardstick's own error on these pixel sets: worst |dp| (largest component, absolute) and |d(u, v)| (u modulo 1, hits within 1e-3 of a
# sphere's pole left out) of the ray-query hits against the f64 checker, as measured on an MI355X by tests/test_gpu_features.py, which
# measures them again on every run, moves (u, v, p) by what it finds and holds that to 2 x these. The host test moves by these figures.
YARDSTICK_ERR = {"book1": (1.786e-5, 5.637e-6), "cornell": (1.183e-3, 8.460e-6), "mesh": (1.858e-6, 1.188e-5), "moving": (1.252e-4, 5.608e-6),
                 "rotated_sphere": (2.204e-6, 8.149e-7), "earth": (4.307e-6, 3.022e-6), "textured": (2.562e-6, 1.063e-6)}


def textured_scene(pkg):
    """A checker ground rect, a Perlin sphere, a metal and a glass sphere under the sky gradient. The ground lies at y = -0.1, not 0: the
    checker's sin(10 y) factor would be 0 there and the cell undefined."""
    A = pkg._abi
    b = pkg.SceneBuilder(background=(0.5, 0.7, 1.0), background_mode=A.RT_BG_SKY_GRADIENT)
    ground = b.xz_rect(-5, 5, -5, 5, -0.1, b.lambertian(texture=b.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))))
    marble = b.sphere((0.0, 0.8, 0.0), 0.8, b.lambertian(texture=b.noise(4.0, np.random.default_rng(11))))
    world = b.hittable_list([ground, marble, b.sphere((1.6, 0.4, 0.8), 0.4, b.metal((0.8, 0.6, 0.2), 0.0)), b.sphere((-1.5, 0.45, 1.0), 0.45, b.dielectric(1.5))])
    cam = pkg.camera_new((3.0, 2.0, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 30.0, 1.5, 0.0, 10.0, 0.0, 0.0)
    return R.Built(b.desc(world), cam, b, 6.0)


def build_scene(pkg, name):
    return textured_scene(pkg) if name == "textured" else R.build_scene(pkg, name)


def camera_rays(orc, cam, width, height, seed, sample, jitter=None, n_draws=40):
    """new_camera_ray (csrc/kernels.hip: main.rs:752-753, camera.rs:60-70) for every pixel of the frame, sample `sample`: draws 0, 1 = the
    jitter, then pairs for random_in_unit_disk until one is accepted (drawn whatever the lens radius), then the time. f64 arithmetic on
    the f32 draws; the acceptance test in f32 as the device makes it. jitter: a value to use instead of draws 0 and 1. Returns
    (origins (n, 3), directions (n, 3), times (n,)) in f64, pixel y * width + x."""
    v3 = lambda v: np.array([v.x, v.y, v.z], dtype=np.float64)
    org, llc, hor, ver, cu, cv = v3(cam.origin), v3(cam.lower_left_corner), v3(cam.horizontal), v3(cam.vertical), v3(cam.u), v3(cam.v)
    n = width * height
    o, d, tm = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    f32 = np.float32
    for y in range(height):
        for x in range(width):
            i = y * width + x
            r = orc.rng_stream(seed, i, sample, n_draws)[2]
            ju, jv = (float(r[0]), float(r[1])) if jitter is None else (jitter, jitter)
            u, v = (x + ju) / (width - 1), (height - 1 - y + jv) / (height - 1)
            k = 2
            while True:
                if k + 3 > n_draws:
                    raise RuntimeError("the disk rejection ran out of draws")
                px, py = f32(-1.0) + f32(2.0) * r[k], f32(-1.0) + f32(2.0) * r[k + 1]
                k += 2
                if f32(f32(px * px) + f32(py * py)) < f32(1.0):
                    break
            off = cu * (cam.lens_radius * float(px)) + cv * (cam.lens_radius * float(py))
            o[i] = org + off
            d[i] = llc + hor * u + ver * v - org - off
            tm[i] = cam.time0 + (cam.time1 - cam.time0) * float(r[k])
    return o, d, tm


def background(desc, d):
    """The background radiance of rays with directions d (n, 3), f64 (main.rs:74-76 and the sky gradient of the scene functions)."""
    bg = np.array(desc.background.tuple())
    if desc.background_mode == 0:
        return np.broadcast_to(bg, d.shape).copy()
    t = 0.5 * (d[:, 1] / np.linalg.norm(d, axis=1) + 1.0)
    return (1.0 - t)[:, None] * np.ones(3) + t[:, None] * bg


def texture_values(orc, desc, tex, u, v, p):
    out = np.zeros((len(u), 3))
    L = orc.lib()
    p3, o3 = (C.c_double * 3)(), (C.c_double * 3)()
    for i in range(len(u)):
        p3[0], p3[1], p3[2] = p[i]
        if L.orc_texture_value(C.byref(desc), int(tex), float(u[i]), float(v[i]), p3, o3) != 0:
            raise RuntimeError("checker: " + L.orc_last_error().decode())
        out[i] = o3[0], o3[1], o3[2]
    return out


def expected_albedo(pkg, orc, desc, hit, material, ff, u, v, p, d, err=None):
    """Per ray: the first-hit colour of the contract (include/rt_hip.h, "first-hit features") from a hit list — hit (bool), material index,
    front_face, u, v, p — and the rays' directions d, in f64. With err = (dp, duv) also `unstable`: the textured hits whose colour moves
    by more than 1e-3 when (u, v, p) move by that much in any of 8 sign patterns (texel, checker-cell and Perlin-lattice boundaries)."""
    A = pkg._abi
    n = len(hit)
    out = background(desc, np.asarray(d, np.float64))
    unstable = np.zeros(n, bool)
    u, v, p = np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(p, np.float64)
    for m in sorted(set(int(x) for x in material[hit])):
        k = np.flatnonzero(hit & (material == m))
        mat = desc.materials[m]
        if mat.kind == A.RT_MAT_METAL:
            out[k] = mat.albedo.tuple()
        elif mat.kind == A.RT_MAT_DIELECTRIC:
            out[k] = 1.0
        else:
            t = desc.textures[mat.texture]
            if t.kind == A.RT_TEX_SOLID:
                out[k] = t.color.tuple()
            else:
                out[k] = texture_values(orc, desc, mat.texture, u[k], v[k], p[k])
                if err is not None:
                    for s in R.SIGNS:
                        moved = texture_values(orc, desc, mat.texture, u[k] + s[0] * err[1], v[k] + s[1] * err[1], p[k] + np.array(s) * err[0])
                        unstable[k] |= np.abs(moved - out[k]).max(axis=1) > 1e-3
            if mat.kind == A.RT_MAT_DIFFUSE_LIGHT:
                out[k[~ff[k]]] = 0.0                                  # material.rs:184-190: nothing is emitted from the back face
    return (out, unstable) if err is not None else out


_cache = {}


def pixel_set(pkg, orc, name):
    """dict(built, rays, ref, undecidable) for sample 0 of every pixel of a GRID frame of one scene, seed SEED: the host-made f32 rays,
    the checker's f64 answer and which rays are undecidable (rays.undecidable). Computed once per process."""
    if name not in _cache:
        built = build_scene(pkg, name)
        o, d, tm = camera_rays(orc, built.cam, GRID[0], GRID[1], SEED, 0)
        rays = R.make_rays(o, d, tm)
        ref = R.ask(orc, built.desc, rays)
        _cache[name] = dict(built=built, rays=rays, ref=ref, undecidable=R.undecidable(orc, built.desc, rays, ref))
    return _cache[name]
