"""RT_SCENE_LIGHTS_MANY on the GPU (include/rt_hip.h): the area-weighted pick and the light tree.

a. rt_sample_lights against light_reference, query by query: the picked member and the draw count exactly on the decidable queries (a pick whose
   draw lies within 2^-24 of a cdf edge is not decidable), d and pdf within TWICE the deviation the f32 restatement shows from the f64 one.
b. the tree drops nothing: light_pdf through the tree and by the plain loop (RT_LIGHTQ_LINEAR) are equal as uint32 arrays, on the drawn
   directions, on random directions and on axis-parallel rays whose origins lie in the planes of the tree's box faces and of the mesh.
c. direct lighting by the tessellated lamp and by the icosphere against Lambert's form factor (the untessellated quad's for the lamp), the three
   kernel forms bit-identical.
d. sub-linear work, counted: a 512-triangle lamp costs at most 4 triangle tests per sample with the tree and 512 per floor hit without.
e. a refused list uploads nothing; upload, destroy, upload renders the same frame.

Measured on an MI355X. a: device against f64, d relative to |d| / pdf relative (the f32 restatement's own deviation in brackets):
       one 1.8e-07 / 1.2e-06 (1.8e-07 / 1.1e-06)   two 1.6e-07 / 1.9e-06 (1.7e-07 / 1.1e-06)   three 1.9e-07 / 1.6e-05 (1.9e-07 / 1.6e-05)
       graded_lamp 1.6e-07 / 7.2e-07 (same)   ico2 1.5e-07 / 2.0e-05 (same)   mixed 8.5e-06 / 2.4e-05 (8.5e-06 / 2.0e-05)
   undecidable share at most 1.2 % (ico2). b: no ray differs (up to 26 144 axis rays a case, of which up to 13 326 meet a member).
c: mean z +0.009 (graded_lamp) and -0.034 (ico2) against a bound of 0.1875, no pixel beyond |z| = 4; ico2's mean z stays within +-0.06 up to
   16 384 spp. d: 1.13 triangle tests per sample with the tree, 512 without."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lights_cases as LC  # noqa: E402
import lights_many_cases as LM  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- a. query by query ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LM.CASES)
def test_samples_match_the_reference_query_by_query(pkg, gpu, name):
    desc, keep, box = LM.query_case(pkg, name)
    pts, states = LC.query_points("many_" + name, box)
    r64, ok, dev_d, dev_pdf = LM.deviations(pkg, desc, pts, states)
    assert 1.0 - ok.mean() <= LC.SKIP_SHARE
    scene = gpu.upload(desc)
    try:
        got, st = gpu.sample_lights(scene, pts, states, with_stats=True)
        assert st["samples"] == len(pts)
        assert (got["light"][ok] == r64["light"][ok]).all() and (got["n_draws"][ok] == r64["n_draws"][ok]).all()
        assert (got["light"] >= 0).all() and (got["light"] < pkg.compile_info(desc)["n_lights"]).all()
        err_d = np.linalg.norm(got["d"].astype(np.float64) - r64["d"], axis=1) / np.linalg.norm(r64["d"], axis=1)
        err_pdf = np.abs(got["pdf"].astype(np.float64) - r64["pdf"]) / r64["pdf"]
        print(f"{name}: device against f64: d {err_d[ok].max():.3e} (f32 restatement {dev_d:.3e}), pdf {err_pdf[ok].max():.3e} (f32 restatement {dev_pdf:.3e}), "
              f"skipped {1.0 - ok.mean():.4f}")
        assert err_d[ok].max() <= 2.0 * dev_d, (name, float(err_d[ok].max()), dev_d)
        assert err_pdf[ok].max() <= 2.0 * dev_pdf, (name, float(err_pdf[ok].max()), dev_pdf)
        again = gpu.light_pdf(scene, pts, got["d"])                    # DIRECTION_GIVEN: the pdf of the drawn direction, bit for bit
        assert np.array_equal(again.view(np.uint32), got["pdf"].view(np.uint32))
    finally:
        scene.close()


# ---- b. the tree drops nothing ------------------------------------------------------------------------------------------------------------------------
TINY = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-30, -1e-30], dtype=np.float32)        # zero, -0, subnormal, 1e-30


def _axis_rays(pkg, desc, tree, rng, lamp_plane):
    """axis-parallel rays (one component +-1, the other two from TINY): origins in the planes of the tree's box faces — a point of the face,
    and the same point pushed along the ray's axis out of the box — and on the grid lines through the mesh's vertices"""
    mn, mx = LM.node_boxes(tree["nodes"])
    mn32, mx32 = mn.astype(np.float32), mx.astype(np.float32)
    o, d = [], []

    def ray(origin, axis, sign):
        v = TINY[rng.integers(0, len(TINY), 3)].copy()
        v[axis] = sign
        o.append(np.asarray(origin, np.float32))
        d.append(v)
    pick = np.arange(len(mn)) if len(mn) <= 256 else np.unique(np.concatenate([np.arange(64), rng.integers(0, len(mn), 192)]))
    for i in pick:
        for a in range(3):
            for face in (mn32[i, a], mx32[i, a], np.nextafter(mn32[i, a], np.float32(-np.inf)), np.nextafter(mx32[i, a], np.float32(np.inf))):
                p = (mn[i] + (mx[i] - mn[i]) * rng.random(3)).astype(np.float32)
                p[a] = face
                for m in range(3):
                    if m == a:                                         # leaves the face along its normal, both ways
                        ray(p, m, 1.0), ray(p, m, -1.0)
                    else:                                              # runs in the face's plane: from inside the box, and from 3 units outside it
                        q = p.copy()
                        q[m] = np.float32(mn[i, m] - 3.0)
                        ray(p, m, 1.0), ray(q, m, 1.0), ray(q, m, -1.0)
    for v in LM.world_vertices(pkg, desc):                            # along the mesh's own grid lines (for the lamp: in its plane, along its cell borders)
        if v is None:
            continue
        for vert in v[:: 1 if len(o) < 40000 else 3]:
            for m in range(3):
                q = np.asarray(vert, np.float32).copy()
                q[m] -= np.float32(2.5)
                ray(q, m, 1.0)
    if lamp_plane is not None:
        for _ in range(512):
            q = np.array([rng.uniform(-2.0, 2.0), lamp_plane, rng.uniform(-2.0, 2.0)], np.float32)
            ray(q, int(rng.integers(0, 3)), float(rng.choice([-1.0, 1.0])))
    return np.array(o, np.float32), np.array(d, np.float32)


@pytest.mark.parametrize("name", LM.CASES)
def test_the_tree_drops_no_member(pkg, gpu, name):
    desc, keep, box = LM.query_case(pkg, name)
    pts, states = LC.query_points("many_" + name, box)
    tree = pkg.light_tree(desc)
    rng = np.random.default_rng(sum(map(ord, name)) + 3)
    scene = gpu.upload(desc)
    try:
        drawn = gpu.sample_lights(scene, pts, states)["d"]
        rand = rng.normal(size=(LC.N_QUERIES, 3)).astype(np.float32)
        ao, ad = _axis_rays(pkg, desc, tree, rng, LM.LAMP_Y if name == "graded_lamp" else None)
        for what, o, d in (("drawn", pts, drawn), ("random", pts, rand), ("axis", ao, ad)):
            a = gpu.light_pdf(scene, o, d, linear=False)
            b = gpu.light_pdf(scene, o, d, linear=True)
            differ = a.view(np.uint32) != b.view(np.uint32)
            print(f"{name} {what}: {len(o)} rays, {int((b != 0).sum())} with a pdf, {int(differ.sum())} differ")
            assert not differ.any(), (name, what, o[differ][:4], d[differ][:4], a[differ][:4], b[differ][:4])
            if what != "axis":
                assert (b[np.isfinite(b)] > 0).sum() > (len(o) // 2 if what == "drawn" else 0)
    finally:
        scene.close()


# ---- c. direct lighting against the closed form ---------------------------------------------------------------------------------------------------------
def _render_moments(pkg, gpu, scene, cam, **kw):
    prm = pkg.make_params(LC.FRAME, LC.FRAME, LC.SPP, max_depth=2, seed=7, **kw)
    n = LC.FRAME * LC.FRAME * 3
    rgb, sq, st = gpu.render_pass(scene, cam, prm, 0, LC.SPP, False, rgb_sum=np.zeros(n, np.float32), sq_sum=np.zeros(n, np.float32))
    return np.asarray(rgb).reshape(LC.FRAME, LC.FRAME, 3), np.asarray(sq).reshape(LC.FRAME, LC.FRAME, 3)


@pytest.mark.parametrize("name", ("graded_lamp", "ico2"))
def test_direct_lighting_is_the_form_factor(pkg, gpu, name):
    """lights_cases' floor and camera under the tessellated emitters with scene_flags = 5, 32 x 32 x 256 spp, max_depth 2: a pixel's mean is albedo * Le * F.
    For graded_lamp F is the form factor of the UNTESSELLATED quad. Wavefront, fused and tail_paths = 1 renders are bit-identical."""
    A = pkg._abi
    desc, keep, faces = LM.emitter_case(pkg, name)
    assert desc.scene_flags == 5
    cam = LC.camera(pkg, *LC.CAM_FLOOR)
    fine, coarse = (8, 4) if name == "graded_lamp" else (4, 2)         # (320 faces: the footprint average on the coarser pair of grids)
    e_f, e_c = LC.expected_frame(cam, faces, fine), LC.expected_frame(cam, faces, coarse)
    scene = gpu.upload(desc)
    try:
        rgb, sq = _render_moments(pkg, gpu, scene, cam)
        for kw in (dict(flags=A.RT_FLAG_FUSED), dict(tail_paths=1)):
            rgb2, sq2 = _render_moments(pkg, gpu, scene, cam, **kw)
            assert np.array_equal(rgb, rgb2) and np.array_equal(sq, sq2), kw
        assert np.isfinite(rgb).all()
        z, se = LC.z_scores(rgb, sq, e_f, LC.SPP)
        lit = se > 0
        print(f"{name}: mean z {z.mean():+.4f} (bound {6 / math.sqrt(z.size):.4f}), share |z| > 4: {(np.abs(z) > 4).mean():.4f}, lit pixels {lit.mean():.2f}, "
              f"median SE {np.median(se[lit]):.2e}, max |fine - coarse| {np.abs(e_f - e_c).max():.2e}")
        assert np.abs(e_f - e_c).max() <= 0.1 * np.median(se[lit])     # the footprint average has converged
        assert LC.check_z(z)
    finally:
        scene.close()


@pytest.mark.parametrize("name", ("one", "three", "mixed"))
def test_a_small_table_renders_the_same_in_the_three_forms(pkg, gpu, name):
    """A table of a few lights is staged into k_shade's LDS blob, tree and cdf with it (a big one is read where the upload put it, as in the
    form-factor cases above); the drain form reads it from memory. The frames are bit-identical."""
    A = pkg._abi
    desc, keep, box = LM.query_case(pkg, name)
    cam = LC.camera(pkg, (0.0, 0.5, -6.0), (0.0, 0.5, 0.0))
    scene = gpu.upload(desc)
    try:
        frames = [gpu.render(scene, cam, pkg.make_params(32, 32, 16, max_depth=6, seed=5, **kw))[0] for kw in (dict(), dict(flags=A.RT_FLAG_FUSED), dict(tail_paths=1))]
        assert np.isfinite(frames[0]).all() and frames[0].max() > 0
        assert np.array_equal(frames[0], frames[1]) and np.array_equal(frames[0], frames[2])
    finally:
        scene.close()


# ---- d. sub-linear work, counted not timed ----------------------------------------------------------------------------------------------------------------
def test_a_512_triangle_lamp_costs_a_few_tests_per_sample(pkg, gpu):
    """The world is the floor alone; the lights list is the graded lamp as 16 x 16 cells (512 triangles), not in the world. max_depth 2: every
    camera ray meets the floor, scatters once (the one evaluation of the list's pdf) and leaves. A point of the lamp's plane lies in the boxes
    of its cell's two triangles, and in more only within the pad of a cell border: at most 4 triangle tests per sample with the tree; the
    plain list tests all 512."""
    A = pkg._abi
    counts = {}
    for many in (True, False):
        b = pkg.SceneBuilder()
        lamp, grey = b.diffuse_light((LC.LE, LC.LE, LC.LE)), b.lambertian((LC.ALBEDO, LC.ALBEDO, LC.ALBEDO))
        lights = [b.triangle(*t, lamp) for t in LM.graded_lamp_triangles(16)]
        assert len(lights) == 512
        desc = b.desc(b.hittable_list([b.xz_rect(-60.0, 60.0, -60.0, 60.0, 0.0, grey)]), b.hittable_list(lights), lights_all_shapes=True, lights_many=many)
        scene = gpu.upload(desc)
        try:
            prm = pkg.make_params(32, 32, 16, max_depth=2, seed=11, flags=A.RT_FLAG_COUNTERS)
            img, st = gpu.render(scene, LC.camera(pkg, *LC.CAM_FLOOR), prm)
            counts[many] = (st["prim_tests"][3], st["samples"])
        finally:
            scene.close()
    (tree_tests, samples), (list_tests, samples1) = counts[True], counts[False]
    print(f"triangle tests per sample: {tree_tests / samples:.3f} with the tree, {list_tests / samples1:.1f} without ({samples} samples)")
    assert samples == samples1 == 32 * 32 * 16
    assert 0 < tree_tests <= 4 * samples
    assert list_tests == 512 * samples                                 # one floor hit per sample, 512 tests each


# ---- e. lifetimes ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_refused_list_uploads_nothing_and_a_reupload_renders_the_same(pkg, gpu):
    A = pkg._abi
    b = pkg.SceneBuilder()
    lamp, grey = b.diffuse_light((4, 4, 4)), b.lambertian((0.7, 0.7, 0.7))
    flat = b.triangle((0, 3, 0), (1, 3, 0), (2, 3, 0), lamp)
    bad = b.desc(b.hittable_list([b.xz_rect(-5, 5, -5, 5, 0, grey)]), b.hittable_list([b.triangle((0, 3, 0), (1, 3, 0), (0, 3, 1), lamp), flat]),
                 lights_all_shapes=True, lights_many=True)
    with pytest.raises(pkg.RtError) as e:
        gpu.upload(bad)
    assert e.value.code == A.RT_ERR_INVALID and "zero area" in str(e.value)
    handle = C.c_void_p(0xDEAD)
    assert pkg.lib().rt_scene_upload(gpu._h, C.byref(bad), C.byref(handle)) == A.RT_ERR_INVALID and not handle.value
    assert b"lights list member 1" in pkg.lib().rt_last_error(gpu._h)
    bad.scene_flags = 4
    with pytest.raises(pkg.RtError) as e:
        gpu.upload(bad)
    assert e.value.code == A.RT_ERR_INVALID and "needs RT_SCENE_LIGHTS_ALL_SHAPES" in str(e.value)
    desc, keep, faces = LM.emitter_case(pkg, "ico2")
    cam = LC.camera(pkg, *LC.CAM_FLOOR)
    prm = pkg.make_params(32, 32, 16, max_depth=4, seed=9, flags=A.RT_FLAG_COUNTERS)
    frames = []
    for _ in range(2):
        scene = gpu.upload(desc)
        img, st = gpu.render(scene, cam, prm)
        scene.close()
        frames.append(img)
        assert st["prim_tests"][3] > 0
    assert np.array_equal(frames[0], frames[1]) and frames[0].max() > 0
