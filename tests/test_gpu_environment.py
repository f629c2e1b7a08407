"""Environment maps on the GPU (include/rt_hip.h RtEnvMap). tests/environment.py has the helpers and the quadrature's error.

a. lookup, bit for bit: radiance queries of rays that miss, and the albedo plane of render_features, against env_reference.
b. rt_sample_lights against light_reference(env=...), query by query: the picked member and the draw count exactly, d and pdf within TWICE the
   deviation the f32 restatement shows from the f64 one on the same queries (measured by the test itself, on the CPU; test_gpu_lights.py's
   rule). Measured deviations (f32 against f64, largest over the decidable queries of the 4096; d relative to |d|, pdf relative) and the
   device's own:
       map_alone      restatement 5.3e-07 / 6.5e-06   device 5.3e-07 / 1.4e-06   undecidable 0.5 %
       beside_lights  restatement 5.3e-07 / 5.1e-06   device 5.3e-07 / 1.0e-06   undecidable 1.7 %
   Decidable: test_gpu_lights.py's rule for the area lights, and for the map a direction at least 1e-4 texel from a border between texels
   and with sin(theta) >= 0.1 (the pdf divides by sqrt(1 - y^2): a rounding of y is amplified by 1 / sin^2 next to a pole).
c. unbiased against quadrature, sampled and unsampled, and the sampled standard error is the smaller. Measured: z = +0.36 sampled, +0.15
   unsampled (green channel), standard error unsampled / sampled = 5.9.
d. furnace: a constant map, a convex Lambertian sphere: every sample is albedo * E. Measured: 2.6e-7 relative at the worst pixel.
e. invariances, bit for bit: passes against one render, layouts, kernel forms, pool sizes; no map = the call without the field.
f. rt_scene_upload_multi_ex with a world of 1 renders the same frame."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import environment as EV  # noqa: E402
import lights_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).reshape(-1)


# ---- a. lookup ------------------------------------------------------------------------------------------------------------------------------------
def test_a_miss_returns_the_lookups_texel_bit_for_bit(pkg, gpu):
    """4096 uniform directions and the special ones (along +-y, on the seam with either zero) from the origin of a scene they all miss, one
    sample each at max_depth 1: the sample is scale * texel, to the bit, for every ray at least 1e-4 texel (in f64) from a border between
    texels. A 15 x 8 map: with an odd width the rays along +-y (u = 1/2) lie inside a texel."""
    rgb = EV.random_map(5, W=15, H=8)
    env = pkg.EnvMap(rgb, sampled=False, scale=1.5)
    desc, keep = EV.empty_scene(pkg)
    dirs = np.concatenate([EV.special_dirs(), EV.uniform_dirs(4096)])
    r64 = pkg.env_reference(env, dirs=dirs, dtype=np.float64)
    r32 = pkg.env_reference(env, dirs=dirs, dtype=np.float32)
    ok = r64["border"] >= EV.BORDER
    n_special = len(EV.special_dirs())
    assert ok[:n_special].all()                                   # the special rays are decidable: the clamps and the signed zero decide them
    assert 1.0 - ok.mean() <= 0.02
    scene = gpu.upload(desc, env_map=env)
    try:
        rgb_sum, sq, inv = gpu.radiance(scene, pkg.path_rays((0.0, 0.0, 0.0), dirs), 1, max_depth=1, seed=3)
    finally:
        scene.close()
    assert (inv == 0).all()
    want = r32["radiance"]
    print(f"lookup: {1.0 - ok.mean():.5f} of the rays within {EV.BORDER} texel of a border; device texel != f32 statement's on {int((bits(rgb_sum) != bits(want)).reshape(-1, 3).any(axis=1).sum())} rays in all")
    assert (r32["i"][ok] == r64["i"][ok]).all() and (r32["j"][ok] == r64["j"][ok]).all()
    assert np.array_equal(bits(rgb_sum[ok]), bits(want[ok]))
    # the special rays, spelled out: up = row 0, down = the last row; on the seam +0 -> column 0, -0 -> the last column
    got = rgb_sum[:n_special] / np.float32(1.5)
    assert np.allclose(got[0], rgb[0, 7]) and np.allclose(got[1], rgb[7, 7]) and np.allclose(got[3], rgb[3, 0]) and np.allclose(got[4], rgb[3, 14])


def test_feature_albedo_on_a_miss_is_the_maps_radiance(pkg, gpu):
    """render_features on a scene every camera ray misses: the albedo plane of sample 0 is the 1-spp render's frame at max_depth 1 (the same
    camera ray, the same lookup), bit for bit, and holds many texels."""
    import torch
    env = pkg.EnvMap(EV.random_map(5, W=15, H=8), sampled=True, scale=0.75)
    desc, keep = EV.empty_scene(pkg)
    cam = pkg.camera_new((0, 0, 0), (0.3, 0.2, -1.0), (0, 1, 0), 100.0, 1.0, 0.0, 1.0, 0.0, 0.0)
    prm = pkg.make_params(32, 32, 1, max_depth=1, seed=4)
    scene = gpu.upload(desc, env_map=env)
    try:
        frame, _ = gpu.render(scene, cam, prm)
        albedo, normal, depth, hits = gpu.render_features(scene, cam, prm)
        torch.cuda.synchronize()
    finally:
        scene.close()
    assert int(hits.sum()) == 0 and len(np.unique(frame.reshape(-1, 3), axis=0)) >= 8
    assert np.array_equal(bits(albedo.cpu().numpy()), bits(frame))


# ---- b. the sampler ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["map_alone", "beside_lights"])
def test_samples_match_the_reference_query_by_query(pkg, gpu, name):
    env = pkg.EnvMap(EV.sun_map(), scale=2.0)
    desc, keep = EV.floor_scene(pkg) if name == "map_alone" else EV.lit_scene(pkg)
    n_lights = 0 if name == "map_alone" else 2
    rng = np.random.default_rng(21)
    pts = (rng.uniform(-1.5, 1.5, (4096, 3)) * np.array([1.0, 0.0, 1.0]) + np.array([0.0, 0.25, 0.0])).astype(np.float32)
    states = rng.integers(0, 1 << 63, 4096, dtype=np.uint64)
    r64 = pkg.light_reference(desc, pts, states, dtype=np.float64, env=env)
    r32 = pkg.light_reference(desc, pts, states, dtype=np.float32, env=env)
    ok = LC.decidable(r64) & (r64["env_border"] >= EV.BORDER) & (r64["env_sin_theta"] >= EV.SIN_MIN)
    assert (r32["light"] == r64["light"]).all() and (r32["n_draws"] == r64["n_draws"]).all()
    rel_d = lambda a: np.linalg.norm(a.astype(np.float64) - r64["d"], axis=1) / np.linalg.norm(r64["d"], axis=1)
    rel_p = lambda a: np.abs(a.astype(np.float64) - r64["pdf"]) / r64["pdf"]
    dev_d, dev_pdf = float(rel_d(r32["d"])[ok].max()), float(rel_p(r32["pdf"])[ok].max())
    assert 1.0 - ok.mean() <= 0.05, 1.0 - ok.mean()
    assert set(np.unique(r64["light"])) == set(range(n_lights + 1))
    scene = gpu.upload(desc, env_map=env)
    try:
        got, st = gpu.sample_lights(scene, pts, states, with_stats=True)
        again = gpu.light_pdf(scene, pts, got["d"])
    finally:
        scene.close()
    assert st["samples"] == len(pts)
    assert (got["light"] == r64["light"]).all() and (got["n_draws"] == r64["n_draws"]).all()
    assert (got["n_draws"][got["light"] == n_lights] == 3).all()            # the pick, then the map's two draws
    err_d, err_pdf = rel_d(got["d"]), rel_p(got["pdf"])
    print(f"{name}: device against f64: d {err_d[ok].max():.3e} (f32 restatement {dev_d:.3e}), pdf {err_pdf[ok].max():.3e} (f32 restatement {dev_pdf:.3e}), "
          f"skipped {1.0 - ok.mean():.4f}")
    assert err_d[ok].max() <= 2.0 * dev_d, (name, float(err_d[ok].max()), dev_d)
    assert err_pdf[ok].max() <= 2.0 * dev_pdf, (name, float(err_pdf[ok].max()), dev_pdf)
    assert np.array_equal(again.view(np.uint32), got["pdf"].view(np.uint32))


# ---- c. unbiased ------------------------------------------------------------------------------------------------------------------------------
def test_a_floor_under_the_map_is_the_quadrature(pkg, gpu):
    """One ray straight down onto a large Lambertian XZ rect, the whole scene, 65 536 samples; the map 16 x 8 with texels in [0.1, 1] and one
    of 200 in the upper half. Expected: albedo / pi * integral over y > 0 of E(w) y dw (f64 quadrature, relative error < 1e-5). The mean lies
    within 5 standard errors (from sq_sum) of it with RT_ENV_SAMPLED and without, and the sampled standard error is the smaller. The CPU
    statement alone meets the same bound: test_environment_host.py::test_the_reference_estimators_of_a_floor_are_unbiased."""
    rgb = EV.sun_map()
    expect = EV.FLOOR_ALBEDO / math.pi * EV.floor_irradiance_integral(rgb)
    desc, keep = EV.floor_scene(pkg)
    rays = pkg.path_rays((0.3, 1.0, -0.2), (0.0, -1.0, 0.0))
    N = 65536
    se = {}
    for sampled in (True, False):
        scene = gpu.upload(desc, env_map=pkg.EnvMap(rgb, sampled=sampled))
        try:
            s, q, inv = gpu.radiance(scene, rays, N, max_depth=4, seed=11)
        finally:
            scene.close()
        mean = s[0].astype(np.float64) / N
        err = pkg.standard_error(s, q, N)[0]
        z = (mean - expect) / err
        print(f"sampled={sampled}: mean {mean} expected {expect} standard error {err} z {z}")
        assert np.isfinite(s).all() and (np.abs(z) <= 5.0).all(), (sampled, z)
        se[sampled] = err
    print(f"standard error, unsampled / sampled: {se[False] / se[True]}")
    assert (se[True] < se[False]).all()


# ---- d. furnace -------------------------------------------------------------------------------------------------------------------------------
def test_furnace(pkg, gpu):
    """A constant map E, unsampled, and a convex Lambertian sphere of albedo a: a path hits the sphere at most once, so a sample is E (a miss)
    or T E with T = a * (scattering pdf / sampling pdf). Both pdfs are cos / pi of the same direction, formed from n and from unit(n): two
    three-term dot products that differ by at most 6 eps of their terms' sum (<= 1), so their ratio is 1 within 6 eps / cos; the chain
    a * ratio * E * scale and the reciprocal add 6 roundings. A cosine-distributed direction has cos < c with probability c^2: among the
    4096 samples here none lies below c = 1e-3 but with probability 0.4 %. Bound, relative: 6 eps + 6 eps / 1e-3 = 3.6e-4; sums of 4 samples."""
    E, a = np.float32([0.75, 0.5, 0.375]), (0.5, 0.7, 0.9)                 # (E in few bits: the sum of four misses is exact)
    env = pkg.EnvMap(np.broadcast_to(E, (4, 8, 3)).copy(), sampled=False)
    desc, keep = EV.furnace_scene(pkg, a)
    cam = pkg.camera_new((0, 0, 4), (0, 0, 0), (0, 1, 0), 40.0, 1.0, 0.0, 4.0, 0.0, 0.0)
    prm = pkg.make_params(32, 32, 4, max_depth=8, seed=6)
    scene = gpu.upload(desc, env_map=env)
    try:
        img, st = gpu.render(scene, cam, prm)
    finally:
        scene.close()
    mean = img.astype(np.float64) / 4
    on_sphere = np.zeros((32, 32), bool)
    on_sphere[12:20, 12:20] = True                                       # the sphere's disc has a radius of 11 pixels: these see nothing else
    sky = np.zeros((32, 32), bool)
    sky[:2] = sky[-2:] = True
    assert np.array_equal(bits(img[sky]), bits(np.broadcast_to(E * np.float32(4), img[sky].shape)))
    want = np.float64(np.float32(a)) * np.float64(E)
    rel = np.abs(mean[on_sphere] / want - 1.0).max()
    print(f"furnace: largest relative deviation of a pixel on the sphere {rel:.3e} (bound 3.6e-4)")
    assert rel <= 6 * EPS + 6 * EPS / 1e-3


# ---- e. invariances ---------------------------------------------------------------------------------------------------------------------------
def test_a_map_lit_frame_is_the_same_frame_however_it_is_rendered(pkg, gpu):
    A = pkg._abi
    env = pkg.EnvMap(EV.sun_map(), scale=0.5)
    desc, keep = EV.gallery_scene(pkg)
    cam = EV.gallery_camera(pkg)
    SPP = 8
    prm = pkg.make_params(32, 32, SPP, max_depth=12, seed=9)
    assert pkg.compile_info(desc, env_map=env)["features"] & A.RT_FEATURE_ENV
    scene = gpu.upload(desc, env_map=env)
    try:
        base, st = gpu.render(scene, cam, prm)
        assert np.isfinite(base).all() and base.min() >= 0 and st["segments"] > 2 * st["samples"]
        # passes: 3 + 5 samples, the second accumulating
        n = 32 * 32 * 3
        acc = np.zeros(n, np.float32)
        gpu.render_pass(scene, cam, pkg.make_params(32, 32, 3, max_depth=12, seed=9), 0, SPP, False, rgb_sum=acc)
        gpu.render_pass(scene, cam, pkg.make_params(32, 32, 5, max_depth=12, seed=9), 3, SPP, True, rgb_sum=acc)
        assert np.array_equal(bits(acc), bits(base))
        # the three kernel forms and two pool sizes
        for kw in (dict(flags=A.RT_FLAG_FUSED), dict(tail_paths=1), dict(pool_slots=4096), dict(pool_slots=1024, tail_paths=1)):
            img, _ = gpu.render(scene, cam, pkg.make_params(32, 32, SPP, max_depth=12, seed=9, **kw))
            assert np.array_equal(bits(img), bits(base)), kw
    finally:
        scene.close()
    scene = gpu.upload(desc, A.RT_LAYOUT_LISTS_AS_REFERENCE, env_map=env)
    try:
        img, _ = gpu.render(scene, cam, prm)
    finally:
        scene.close()
    assert np.array_equal(bits(img), bits(base))
    # the map matters: without it the frame differs; and no map = the call without the field (NULL options, a 40-byte record, a NULL field)
    frames = []
    null_field = pkg.upload_options(env_map=env)
    null_field._b_base_.env_map = None
    short = pkg.upload_options(env_map=env)
    short.struct_bytes = 40                                  # the caller's sizeof: the pointer behind it is not read
    for opt in (None, short, null_field):
        sc = pkg.Scene(gpu, desc, opt)
        try:
            frames.append(gpu.render(sc, cam, prm)[0])
        finally:
            sc.close()
    assert np.array_equal(bits(frames[0]), bits(frames[1])) and np.array_equal(bits(frames[0]), bits(frames[2]))
    assert not np.array_equal(bits(frames[0]), bits(base))


# ---- f. multi upload ----------------------------------------------------------------------------------------------------------------------------
def test_multi_upload_with_a_world_of_one_renders_the_same_frame(pkg, gpu):
    env = pkg.EnvMap(EV.sun_map(), scale=0.5)
    desc, keep = EV.gallery_scene(pkg)
    cam = EV.gallery_camera(pkg)
    prm = pkg.make_params(32, 32, 4, max_depth=12, seed=9)
    scene = gpu.upload(desc, env_map=env)
    try:
        base, _ = gpu.render(scene, cam, prm)
    finally:
        scene.close()
    m = pkg.MultiContext([0])
    try:
        ms = m.upload(desc, env_map=env)
        try:
            img, st = m.render(ms, cam, prm)
        finally:
            ms.close()
    finally:
        m.close()
    assert st["n_devices"] == 1 and np.array_equal(bits(img), bits(base))
