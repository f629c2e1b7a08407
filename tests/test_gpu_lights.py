"""Area lights of every shape on the GPU (include/rt_hip.h: RT_SCENE_LIGHTS_ALL_SHAPES, rt_sample_lights).

a. rt_sample_lights against light_reference, query by query: the picked light and the draw count exactly, d and pdf within TWICE the
   deviation the f32 restatement shows from the f64 one on the same queries (measured by the test itself, on the CPU). Measured deviations
   (f32 against f64, largest over the decidable queries of the 4096; d relative to |d|, pdf relative):
       xy_rect 6.8e-08 / 3.9e-07   xz_rect 5.8e-08 / 4.2e-07   yz_rect 5.9e-08 / 3.8e-07   triangle 1.8e-07 / 1.1e-06   box 1.0e-07 / 2.3e-06
       wrapped_rect 1.2e-07 / 4.9e-07   wrapped_triangle 2.2e-07 / 1.6e-06   icosphere 2.1e-07 / 1.5e-05   mixed 6.7e-06 / 8.2e-06
   undecidable share (|cos| < 1e-2 at a light, or a crossing within 1e-4 of an edge, in f64): at most 1.4 % (icosphere).
b. the flag changes nothing for a list of an XzRect and a Sphere: frames and query results equal as arrays; RT_LIGHTQ_LINEAR changes no
   answer of a table without a light tree.
c. direct lighting of a floor by one emitter against Lambert's polygon form factor, in the three kernel forms, bit-identical.
d. the Cornell box with its lamp as two triangles (flag on) against the reference's rect lamp (flag off): the same picture, statistically.
e. a refused lights list uploads nothing; a scene uploaded, destroyed and uploaded again renders the same frame."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lights_cases as LC  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- a. sample by sample ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.QUERY_CASES)
def test_samples_match_the_reference_query_by_query(pkg, gpu, name):
    desc, keep, box = LC.query_case(pkg, name)
    pts, states = LC.query_points(name, box)
    r64, ok, dev_d, dev_pdf = LC.deviations(pkg, desc, pts, states)
    assert 1.0 - ok.mean() <= LC.SKIP_SHARE
    scene = gpu.upload(desc)
    try:
        got, st = gpu.sample_lights(scene, pts, states, with_stats=True)
        assert st["samples"] == len(pts)
        # exact: which light, how many draws
        assert (got["light"] == r64["light"]).all() and (got["n_draws"] == r64["n_draws"]).all()
        err_d = np.linalg.norm(got["d"].astype(np.float64) - r64["d"], axis=1) / np.linalg.norm(r64["d"], axis=1)
        err_pdf = np.abs(got["pdf"].astype(np.float64) - r64["pdf"]) / r64["pdf"]
        print(f"{name}: device against f64: d {err_d[ok].max():.3e} (f32 restatement {dev_d:.3e}), pdf {err_pdf[ok].max():.3e} (f32 restatement {dev_pdf:.3e}), "
              f"skipped {1.0 - ok.mean():.4f}")
        assert err_d[ok].max() <= 2.0 * dev_d, (name, float(err_d[ok].max()), dev_d)
        assert err_pdf[ok].max() <= 2.0 * dev_pdf, (name, float(err_pdf[ok].max()), dev_pdf)
        # DIRECTION_GIVEN: the pdf of the drawn direction, bit for bit
        again = gpu.light_pdf(scene, pts, got["d"])
        assert np.array_equal(again.view(np.uint32), got["pdf"].view(np.uint32))
    finally:
        scene.close()


# ---- b. the flag changes nothing for the reference's own lists ---------------------------------------------------------------------------------------
def test_flag_on_is_flag_off_for_an_xz_rect_and_a_sphere(pkg, gpu):
    doc = json.load(open(os.path.join(LC.ROOT, "examples", "cornell_box.json")))
    off, on = pkg.JsonScene(doc), pkg.JsonScene(dict(doc, lights_all_shapes=True))
    assert on.desc.scene_flags == 1 and off.desc.scene_flags == 0
    prm = pkg.make_params(64, 64, 8, max_depth=50, seed=3)
    rng = np.random.default_rng(2)
    pts = rng.uniform(20.0, 530.0, (4096, 3)).astype(np.float32)
    states = rng.integers(0, 1 << 63, 4096, dtype=np.uint64)
    frames, samples = [], []
    for js in (off, on):
        scene = gpu.upload(js.desc)
        try:
            frames.append(gpu.render(scene, js.camera(1.0), prm)[0])
            samples.append(gpu.sample_lights(scene, pts, states))
        finally:
            scene.close()
    assert np.isfinite(frames[0]).all() and frames[0].max() > 0
    assert np.array_equal(frames[0], frames[1])
    assert np.array_equal(samples[0].view(np.uint8), samples[1].view(np.uint8))
    assert set(samples[0]["light"]) == {0, 1} and (samples[0]["n_draws"] == 3).all()


def test_the_linear_flag_means_nothing_without_a_light_tree(pkg, gpu):
    """RT_LIGHTQ_LINEAR asks a table with a light tree for the plain loop. One kernel body serves every table kind and hands the flag to
    lights_pdf_value always, so on a table without a tree — plain records, and RT_SCENE_LIGHTS_ALL_SHAPES records — the answers must not
    depend on it: 64 queries on the Cornell box (its lamp as a rect, and as two triangles with the flag), half drawing and half with a
    direction towards the lamp given, equal as bytes."""
    A = pkg._abi
    rng = np.random.default_rng(19)
    q = np.zeros(64, dtype=pkg.LIGHTQUERY_DTYPE)
    q["p"] = rng.uniform(20.0, 530.0, (64, 3)).astype(np.float32)
    q["rng_state"] = rng.integers(0, 1 << 63, 64, dtype=np.uint64)
    q["d"][32:] = np.float32([278.0, 554.0, 279.5]) + rng.uniform(-60.0, 60.0, (32, 3)).astype(np.float32) * np.float32([1, 0, 1]) - q["p"][32:]
    q["flags"][32:] = A.RT_LIGHTQ_DIRECTION_GIVEN
    lin = q.copy()
    lin["flags"] |= A.RT_LIGHTQ_LINEAR
    for tri in (False, True):
        js = pkg.JsonScene(LC.cornell_doc(tri))
        assert js.desc.scene_flags == (A.RT_SCENE_LIGHTS_ALL_SHAPES if tri else 0)
        assert bool(pkg.compile_info(js.desc)["features"] & A.RT_FEATURE_LIGHTS_EXT) == tri
        scene = gpu.upload(js.desc)
        try:
            plain, linear = gpu._light_queries(scene, q, False), gpu._light_queries(scene, lin, False)
        finally:
            scene.close()
        assert (plain["pdf"][32:] > 0).any() and (plain["n_draws"][:32] > 0).all() and (plain["n_draws"][32:] == 0).all()
        assert np.array_equal(plain.view(np.uint8), linear.view(np.uint8)), tri


# ---- c. direct lighting against the closed form -----------------------------------------------------------------------------------------------------
def _render_moments(pkg, gpu, scene, cam, **kw):
    prm = pkg.make_params(LC.FRAME, LC.FRAME, LC.SPP, max_depth=2, seed=7, **kw)
    n = LC.FRAME * LC.FRAME * 3
    rgb, sq, st = gpu.render_pass(scene, cam, prm, 0, LC.SPP, False, rgb_sum=np.zeros(n, np.float32), sq_sum=np.zeros(n, np.float32))
    return np.asarray(rgb).reshape(LC.FRAME, LC.FRAME, 3), np.asarray(sq).reshape(LC.FRAME, LC.FRAME, 3)


@pytest.mark.parametrize("name", LC.EMITTER_CASES)
def test_direct_lighting_is_the_form_factor(pkg, gpu, name):
    """max_depth 2, black background, aperture 0, a grey Lambertian floor (albedo 0.7) under one emitter of radiance 4 that the camera does not
    see: a pixel's mean is albedo * Le * F, F = Lambert's polygon form factor of the emitter's front faces, averaged over the pixel's footprint.
    32 x 32 pixels, 256 spp. On one channel: |mean z| <= 6 / sqrt(N); at most 1 % of the pixels beyond |z| = 4. Wavefront, fused and
    tail_paths = 1 renders are bit-identical. A second framing that looks at the emitter's front returns Le exactly."""
    A = pkg._abi
    desc, keep, faces, view = LC.emitter_case(pkg, name)
    cam = LC.camera(pkg, *LC.CAM_FLOOR)
    e8, e4 = LC.expected_frame(cam, faces, 8), LC.expected_frame(cam, faces, 4)
    scene = gpu.upload(desc)
    try:
        rgb, sq = _render_moments(pkg, gpu, scene, cam)
        for kw in (dict(flags=A.RT_FLAG_FUSED), dict(tail_paths=1)):
            rgb2, sq2 = _render_moments(pkg, gpu, scene, cam, **kw)
            assert np.array_equal(rgb, rgb2) and np.array_equal(sq, sq2), kw
        assert np.isfinite(rgb).all()
        z, se = LC.z_scores(rgb, sq, e8, LC.SPP)
        lit = se > 0
        print(f"{name}: mean z {z.mean():+.4f} (bound {6 / math.sqrt(z.size):.4f}), share |z| > 4: {(np.abs(z) > 4).mean():.4f}, lit pixels {lit.mean():.2f}, "
              f"median SE {np.median(se[lit]):.2e}, max |8x8 - 4x4| {np.abs(e8 - e4).max():.2e}")
        assert np.abs(e8 - e4).max() <= 0.1 * np.median(se[lit])            # the footprint average has converged
        assert (rgb[LC.surely_dark(e8)] == 0.0).all()                         # dark where no front face shows: the back of an emitter emits nothing
        assert LC.check_z(z)
        # the emitter seen directly: its radiance, exactly
        direct, _ = _render_moments(pkg, gpu, scene, LC.camera(pkg, *view))
        assert (direct[LC.FRAME // 2, LC.FRAME // 2] == np.float32(LC.LE * LC.SPP)).all(), direct[LC.FRAME // 2, LC.FRAME // 2]
    finally:
        scene.close()


# ---- d. the same picture as the parent's path ---------------------------------------------------------------------------------------------------------
def test_cornell_with_a_triangle_lamp_is_the_cornell_box(pkg, gpu):
    """64 x 64, 64 spp, depth 50: the lamp as the reference's FlipFace(XzRect) with a rect light (flag off) and as two triangles (flag on). Per
    channel, z from both renders' squared sums: |mean z| <= 6 / sqrt(N), at most 1 % of the pixels beyond |z| = 4. (The null case — the
    flag-off scene at two seeds by the f64 oracle — passes with mean z +0.0036, +0.0066, +0.0104 and no pixel beyond 4: test_lights_host.py.)"""
    n = 64 * 64 * 3
    out = []
    for tri in (False, True):
        js = pkg.JsonScene(LC.cornell_doc(tri))
        assert bool(pkg.compile_info(js.desc)["features"] & pkg._abi.RT_FEATURE_LIGHTS_EXT) == tri
        scene = gpu.upload(js.desc)
        try:
            prm = pkg.make_params(64, 64, 64, max_depth=50, seed=5)
            rgb, sq, st = gpu.render_pass(scene, js.camera(1.0), prm, 0, 64, False, rgb_sum=np.zeros(n, np.float32), sq_sum=np.zeros(n, np.float32))
            out.append((np.asarray(rgb).reshape(64, 64, 3).copy(), np.asarray(sq).reshape(64, 64, 3).copy()))
        finally:
            scene.close()
    assert np.isfinite(out[1][0]).all() and not np.array_equal(out[0][0], out[1][0])
    z = LC.frame_z(out[0][0], out[0][1], out[1][0], out[1][1], 64)
    for c in range(3):
        zc = z[..., c]
        print(f"channel {c}: mean z {zc.mean():+.4f} (bound {6 / math.sqrt(zc.size):.4f}), share |z| > 4: {(np.abs(zc) > 4).mean():.4f}")
        assert LC.check_z(zc), c


# ---- e. refusals and lifetimes through the real upload -----------------------------------------------------------------------------------------------
def test_a_refused_lights_list_uploads_nothing_and_a_reupload_renders_the_same(pkg, gpu):
    A = pkg._abi
    b = pkg.SceneBuilder()
    lamp, grey = b.diffuse_light((4, 4, 4)), b.lambertian((0.7, 0.7, 0.7))
    flat = b.triangle((0, 3, 0), (1, 3, 0), (2, 3, 0), lamp)
    bad = b.desc(b.hittable_list([b.xz_rect(-5, 5, -5, 5, 0, grey)]), b.hittable_list([flat]), lights_all_shapes=True)
    with pytest.raises(pkg.RtError) as e:
        gpu.upload(bad)
    assert e.value.code == A.RT_ERR_INVALID and "zero area" in str(e.value)
    handle = C.c_void_p(0xDEAD)                              # the C entry point itself: the refusal comes before any allocation, and no scene comes back
    assert pkg.lib().rt_scene_upload(gpu._h, C.byref(bad), C.byref(handle)) == A.RT_ERR_INVALID and not handle.value
    assert b"lights list member 0" in pkg.lib().rt_last_error(gpu._h)
    bad.scene_flags = 6
    with pytest.raises(pkg.RtError) as e:
        gpu.upload(bad)
    assert e.value.code == A.RT_ERR_INVALID and "scene_flags" in str(e.value)
    # a scene without lights has nothing to sample
    plain = b.desc(b.hittable_list([b.xz_rect(-5, 5, -5, 5, 0, grey)]))
    scene = gpu.upload(plain)
    try:
        with pytest.raises(pkg.RtError) as e:
            gpu.sample_lights(scene, np.zeros((4, 3), np.float32), np.arange(4, dtype=np.uint64))
        assert e.value.code == A.RT_ERR_UNSUPPORTED
    finally:
        scene.close()
    # upload, render, destroy, upload again, render: the same frame; counters name the light tests by kind
    desc, keep, faces, view = LC.emitter_case(pkg, "icosphere")
    cam = LC.camera(pkg, *LC.CAM_FLOOR)
    prm = pkg.make_params(32, 32, 16, max_depth=4, seed=9, flags=A.RT_FLAG_COUNTERS)
    frames = []
    for _ in range(2):
        scene = gpu.upload(desc)
        img, st = gpu.render(scene, cam, prm)
        scene.close()
        frames.append(img)
        assert st["prim_tests"][3] > 0                       # triangle tests: the walk's and the 20 lights'
    assert np.array_equal(frames[0], frames[1]) and frames[0].max() > 0
