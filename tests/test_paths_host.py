"""The per-sample shading net on the CPU (tests/paths.py): the checker's path records against its other entry points and against
answers derived by hand, and for every probe scene, form and depth the cap on undecidable samples, the coverage of every branch, and the
f32 checker standing in for the device: on every decidable sample it must take the f64 path and land within the measured figure."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paths as P  # noqa: E402


def ev(orc, *names):
    return sum(orc.EVENTS[n] for n in names)


# ---- the new entry against the existing ones ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [("textures_wrapped", "all"), ("media", "own"), ("lights_default", "own")])
@pytest.mark.parametrize("precision", [64, 32])
def test_paths_entry_equals_samples_entry(pkg, orc, name, form, precision):
    built, _ = P.scene(pkg, name, form)
    A = pkg._abi
    for policy in (A.RT_NAN_PER_SAMPLE, A.RT_NAN_REFERENCE):
        prm = P.params(pkg, 8, nan_policy=policy)
        rgb, st, ps = orc.render(built.desc, built.cam, prm, precision=precision, n_threads=3, per_sample=True, count=True)
        q = orc.render_paths(built.desc, built.cam, prm, precision=precision, n_threads=2, count=True)
        assert q["radiance"].tobytes() == ps.tobytes() and q["rgb_sum"].tobytes() == rgb.tobytes()
        assert int(q["segments"].sum()) == st["segments"] == q["stats"]["segments"]
        assert {k: v for k, v in q["stats"].items() if k != "seconds"} == {k: v for k, v in st.items() if k != "seconds"}
        if policy == A.RT_NAN_REFERENCE:
            assert ((q["terminal"] == orc.TERM_NONFINITE) == ~np.isfinite(q["radiance"]).all(axis=-1)).all()
        else:
            assert np.isfinite(q["radiance"]).all() and not q["radiance"][q["terminal"] == orc.TERM_NONFINITE].any()
        assert int((q["terminal"] == orc.TERM_NONFINITE).sum()) == st["nonfinite_samples"]
        assert (q["segments"] >= 1).all() and (q["segments"] <= 8).all() and (q["terminal"] <= orc.TERM_NONFINITE).all()
        assert ((q["terminal"] == orc.TERM_DEPTH) <= (q["segments"] == 8)).all()
    # a rectangle of the frame holds the same records
    sub = orc.render_paths(built.desc, built.cam, prm, precision=precision, rect=(5, 3, 12, 9))
    for k in ("radiance", "segments", "terminal", "events", "margin", "tmin_margin"):
        assert sub[k].tobytes() == np.ascontiguousarray(q[k][3:9, 5:12]).tobytes(), k


def test_perturbation_moves_every_ray_by_r_ulps(pkg, orc):
    """Nothing to hit, sky gradient: L = (1 - t) + t * bg with t = (unit(d).y + 1) / 2, so the radiance shows the direction that was traced.
    With +-R ulps per component it is the f32-rounded direction moved by exactly that, for every sign pattern; R = 0 changes nothing."""
    A = pkg._abi
    b = pkg.SceneBuilder(background=(0.5, 0.7, 1.0), background_mode=A.RT_BG_SKY_GRADIENT)
    desc = b.desc(b.hittable_list([b.sphere((0, 0, 50), 1.0, b.lambertian((0.5, 0.5, 0.5)))]))
    cam = pkg.camera_new((0, 0, 0), (0.3, 0.2, -1), (0, 1, 0), 50.0, 4 / 3, 0.0, 1.0, 0.0, 0.0)
    prm = pkg.make_params(4, 3, 2, max_depth=3, seed=5)
    base = orc.render_paths(desc, cam, prm)
    assert (base["segments"] == 1).all() and (base["terminal"] == orc.TERM_MISS).all() and (base["events"] == 0).all()
    # the directions, from the RNG contract (draws 0, 1: jitter; lens radius 0) in f64 as camera.rs:60-70 writes them
    v3 = lambda v: np.array([v.x, v.y, v.z])
    d = np.zeros((3, 4, 2, 3))
    for y in range(3):
        for x in range(4):
            for s in range(2):
                _, u, _ = orc.rng_stream(5, y * 4 + x, s, 2)
                d[y, x, s] = v3(cam.lower_left_corner) + v3(cam.horizontal) * ((x + u[0]) / 3) + v3(cam.vertical) * ((2 - y + u[1]) / 2) - v3(cam.origin)
    sky = lambda dd: (1 - 0.5 * (dd[..., 1] / np.linalg.norm(dd, axis=-1) + 1))[..., None] + (0.5 * (dd[..., 1] / np.linalg.norm(dd, axis=-1) + 1))[..., None] * np.array([0.5, 0.7, 1.0])
    assert np.allclose(base["radiance"], sky(d), rtol=0, atol=1e-14)
    d32 = d.astype(np.float32)
    for sg in P.SIGNS:
        moved = (d32 + np.asarray(sg, np.float32) * (np.float32(P.R_ULPS) * np.spacing(np.abs(d32)))).astype(np.float64)
        q = orc.render_paths(desc, cam, prm, r_ulps=P.R_ULPS, signs=sg)
        assert np.allclose(q["radiance"], sky(moved), rtol=0, atol=1e-14)
        assert not np.allclose(q["radiance"], base["radiance"], rtol=0, atol=1e-9)
        assert (q["events"] == 0).all() and (q["segments"] == 1).all()


# ---- known answers, derived by hand ------------------------------------------------------------------------------------------------------
def test_kat_normal_incidence_through_a_glass_sphere(pkg, orc):
    """A camera 5 units from a glass sphere (ir 1.5, r 1) with a field of view of 0.001 degrees: every ray meets it at normal incidence
    (cos within 1e-10 of 1), where Schlick's reflectance is r0 = ((1 - 1.5) / (1 + 1.5))^2 = 0.04 from outside and from inside alike and
    total internal reflection cannot occur. So a path is decided by its draws alone (RNG contract: 2 jitter, pairs for the lens disk until
    one lies in it, 1 time, then one draw per glass interface): it reflects where draw < 0.04. By hand: outside reflect -> 2 segments,
    {schlick, sphere}, miss; refract in, refract out -> 3 segments, {refract, back face, sphere}, miss, L = background; k internal
    reflections add k segments and the schlick bit; 8 segments without leaving -> depth exhausted, L = 0."""
    b = pkg.SceneBuilder(background=(0.25, 0.5, 1.0))
    desc = b.desc(b.hittable_list([b.sphere((0, 0, 0), 1.0, b.dielectric(1.5))]))
    cam = pkg.camera_new((0, 0, 5), (0, 0, 0), (0, 1, 0), 0.001, 4 / 3, 0.0, 5.0, 0.0, 0.0)
    W, H, SPP, D = 8, 6, 16, 8
    q = orc.render_paths(desc, cam, pkg.make_params(W, H, SPP, max_depth=D, seed=3))
    seen = set()
    for y in range(H):
        for x in range(W):
            for s in range(SPP):
                _, u, _ = orc.rng_stream(3, y * W + x, s, 64)
                k, margin = 2, np.inf
                while True:                                            # random_in_unit_disk: vec3.rs:101-113
                    l2 = (2 * u[k] - 1) ** 2 + (2 * u[k + 1] - 1) ** 2
                    margin, k = min(margin, abs(l2 - 1)), k + 2
                    if l2 < 1:
                        break
                k += 1                                                 # the time
                seg, mask, inside, term, L = 0, ev(orc, "hit_sphere"), False, None, (0.0, 0.0, 0.0)
                while term is None:
                    if seg == D:
                        term = orc.TERM_DEPTH
                        break
                    seg += 1
                    if seg > 1 and not inside:                         # left the sphere: nothing else to hit
                        term, L = orc.TERM_MISS, (0.25, 0.5, 1.0)
                        break
                    if inside:
                        mask |= ev(orc, "dielectric_back_face")
                    draw = u[k]; k += 1
                    margin = min(margin, abs(0.04 - draw))
                    if 0.04 > draw:
                        mask |= ev(orc, "dielectric_reflect_schlick")
                    else:
                        mask |= ev(orc, "dielectric_refract")
                        inside = not inside
                got = (int(q["segments"][y, x, s]), int(q["terminal"][y, x, s]), int(q["events"][y, x, s]))
                assert got == (seg, term, mask), (x, y, s, got, (seg, term, mask))
                assert np.allclose(q["radiance"][y, x, s], L, rtol=1e-12, atol=0)
                assert abs(q["margin"][y, x, s] - margin) <= 1e-9
                seen.add((seg, term))
    assert {(2, orc.TERM_MISS), (3, orc.TERM_MISS), (4, orc.TERM_MISS)} <= seen      # reflected outside, straight through, one internal bounce


def test_kat_emitter_front_and_back(pkg, orc):
    """A lone xy-rect DiffuseLight (normal +z) seen from z = -5 (the ray runs along +z: d . n > 0, the back) and from z = +5 (the front),
    bare and under FlipFace, which swaps the flag only (hittable.rs:199). The back emits nothing and evaluates no texture."""
    for flip in (False, True):
        for z in (-5.0, 5.0):
            b = pkg.SceneBuilder(background=(0.1, 0.1, 0.1))
            q = b.xy_rect(-50, 50, -50, 50, 0.0, b.diffuse_light((2.0, 3.0, 4.0)))
            desc = b.desc(b.hittable_list([b.flip_face(q) if flip else q]))
            cam = pkg.camera_new((0, 0, z), (0, 0, 0), (0, 1, 0), 40.0, 4 / 3, 0.0, 5.0, 0.0, 0.0)
            r = orc.render_paths(desc, cam, pkg.make_params(4, 3, 2, max_depth=5, seed=1))
            front = (z > 0) != flip
            want = ev(orc, "hit_rect") | (ev(orc, "under_flip_face") if flip else 0) | (ev(orc, "tex_solid") if front else 0)
            assert (r["segments"] == 1).all() and (r["events"] == want).all()
            assert (r["terminal"] == (orc.TERM_EMITTER_FRONT if front else orc.TERM_EMITTER_BACK)).all()
            assert (r["radiance"] == (np.array([2.0, 3.0, 4.0]) if front else 0.0)).all()
            # the only threshold on the way is the lens disk's; the rect is met head on 5 units away: (5 / |d| - 0.001) * |d . n| = 5 - 0.001 |d_z|
            assert np.isfinite(r["margin"]).all() and (r["margin"] <= 1.0).all() and (np.abs(r["tmin_margin"] - 5.0) < 0.01).all()


def test_kat_depth_one_on_a_lambertian(pkg, orc):
    """max_depth 1 in front of a Lambertian sphere that fills the view, no lights list: one world.hit, the albedo is evaluated and a
    direction drawn from the cosine pdf alone, and the recursion returns black at depth 0 — L = emitted + albedo * spdf * 0 / pdf = 0.
    With a moving sphere, an aperture and a shutter interval: the hit kind, the lens and the time bits."""
    for moving in (False, True):
        b = pkg.SceneBuilder(background=(0.25, 0.5, 1.0))
        m = b.lambertian((0.5, 0.6, 0.7))
        s = b.moving_sphere((0, 0, 0), (0, 0.1, 0), 0.0, 1.0, 3.0, m) if moving else b.sphere((0, 0, 0), 3.0, m)
        desc = b.desc(b.hittable_list([s]))
        cam = pkg.camera_new((0, 0, 5), (0, 0, 0), (0, 1, 0), 20.0, 4 / 3, 0.2 if moving else 0.0, 5.0, 0.0, 1.0 if moving else 0.0)
        r = orc.render_paths(desc, cam, pkg.make_params(4, 3, 4, max_depth=1, seed=2))
        want = ev(orc, "lambertian_cosine_only", "tex_solid") | (ev(orc, "hit_moving_sphere", "lens_offset", "time") if moving else ev(orc, "hit_sphere"))
        assert (r["segments"] == 1).all() and (r["terminal"] == orc.TERM_DEPTH).all() and (r["events"] == want).all() and (r["radiance"] == 0.0).all()
        # depth 2: the second ray leaves the convex sphere for the background
        r = orc.render_paths(desc, cam, pkg.make_params(4, 3, 4, max_depth=2, seed=2))
        assert (r["segments"] == 2).all() and (r["terminal"] == orc.TERM_MISS).all() and (r["events"] == want).all()
        # L = albedo * (cos / pi) * bg / (cos / pi)
        assert np.allclose(r["radiance"], np.array([0.5, 0.6, 0.7]) * np.array([0.25, 0.5, 1.0]), rtol=1e-12, atol=0)


def test_kat_medium_and_isotropic(pkg, orc):
    """A camera inside a medium of density 1e6 (free paths of 1e-6 in a sphere of radius 2): every world.hit scatters in the medium, the
    Isotropic phase function evaluates its solid albedo (0.5) and draws a direction, 4 segments exhaust the depth. Density 1e-9: every
    ray passes through and leaves for the background."""
    for density, dense in ((1e6, True), (1e-9, False)):
        b = pkg.SceneBuilder(background=(0.25, 0.5, 1.0))
        desc = b.desc(b.hittable_list([b.constant_medium(b.sphere((0, 0, 0), 2.0, b.dielectric(1.5)), density, (0.5, 0.5, 0.5))]))
        cam = pkg.camera_new((0, 0, 0.5), (0, 0, 0), (0, 1, 0), 40.0, 4 / 3, 0.0, 1.0, 0.0, 0.0)
        r = orc.render_paths(desc, cam, pkg.make_params(4, 3, 4, max_depth=4, seed=2))
        if dense:
            assert (r["segments"] == 4).all() and (r["terminal"] == orc.TERM_DEPTH).all() and (r["radiance"] == 0.0).all()
            assert (r["events"] == ev(orc, "medium_scattered", "isotropic", "tex_solid")).all()
        else:
            assert (r["segments"] == 1).all() and (r["terminal"] == orc.TERM_MISS).all() and (r["events"] == ev(orc, "medium_passed")).all()
            assert np.allclose(r["radiance"], [0.25, 0.5, 1.0], rtol=0, atol=0)


# ---- the probe scenes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [(s, f) for s in P.SCENES for f in P.FORMS])
def test_scene_runs_on_the_variant_it_is_meant_for(pkg, name, form):
    """The instance every case runs (pick_variant, with_record_variant and with_shade_variant of csrc/kernels.hip, restated in paths.variant_of),
    from the feature bits rt_scene_compile_info reports. "own" forms of the scenes of scene_flags and triangle attributes:
        lights_shapes, lights_shapes_wrapped            kVariantAllLx       (all+lx)
        lights_many, lights_many_one, lights_many_two   kVariantAllLt       (all+lt)
        smooth_mesh                                     kVariantAllAttr     (all+attr)
        smooth_cancel                                   kVariantMeshAttr    (mesh+attr)
        smooth_lit                                      kVariantAllAttrLx   (all+attr+lx)
        smooth_lit_many                                 kVariantAllAttrLt   (all+attr+lt)
    Their "all" forms run the same instance (smooth_cancel: kVariantAllAttr); the older scenes' run 0, mesh, box or all, and all."""
    built, own = P.scene(pkg, name, form)
    assert P.variant_of(pkg, built) == (own if form == "own" else P.all_form_variant(own))
    new = P.F_TRI_ATTR | P.F_LIGHTS_EXT | P.F_LIGHTS_TREE
    assert P.features_of(pkg, built) & new == P.NEW_FEATURES.get(name, 0)


def test_a_hollow_sphere_is_found_whatever_the_tree(pkg, orc):
    """sphere.rs:66-73 forms a sphere's box as centre -+ radius with the SIGNED radius: for the inner sphere of a hollow glass ball
    (radius < 0) that box is inside out, and which rays then find the sphere depends on the boxes the tree pairs it with — the first
    device run of tests/test_gpu_paths.py showed the oracle's tree and the device's (which lifts the ground out and boxes pair members)
    losing it for different rays. Oracle and scene compiler use |radius|: the BVH is a pure accelerator again. So (1) the oracle renders
    the glass scene the same, record for record, with its spheres in a BVH of any seed and in a plain list, and (2) no box of the compiled
    device tree is inside out, and the record in front of the hollow sphere's own leaf holds it."""
    A = pkg._abi
    gl_at = lambda b: [b.sphere((0, -8.5, 0), 8.0, b.lambertian((0.5, 0.5, 0.5))), b.sphere((0, 0.3, 0), 0.8, b.dielectric(1.5)), b.sphere((0, 0.3, 0), -0.7, b.dielectric(1.5)),
                       b.sphere((1.8, 0.3, 0), 0.8, b.dielectric(0.7)), b.sphere((0.9, 0.0, -1.8), 0.5, b.lambertian((0.7, 0.3, 0.3))), b.sphere((-0.9, 0.0, 1.6), 0.5, b.dielectric(1.5))]
    cam = pkg.camera_new((0, 1.5, 7), (0, 0.2, 0), (0, 1, 0), 40.0, P.W / P.H, 0.0, 7.0, 0.0, 0.0)
    runs = []
    for seed in (None, 1, 2, 3, 4):
        b = pkg.SceneBuilder(background=(0.5, 0.7, 1.0), background_mode=A.RT_BG_SKY_GRADIENT, bvh_seed=seed or 1)
        ids = gl_at(b)
        desc = b.desc(b.hittable_list(ids) if seed is None else b.bvh(ids))
        runs.append(orc.render_paths(desc, cam, P.params(pkg, 8)))
        if seed is not None:
            nodes, spheres, _ = pkg.compile_dump(desc)
            boxed = np.isfinite(nodes["mn"]).all(axis=1) & np.isfinite(nodes["mx"]).all(axis=1)
            assert (nodes["mn"][boxed] <= nodes["mx"][boxed]).all()
            hollow = [k for k, s in enumerate(spheres) if s[3] < 0]
            assert len(hollow) == 1
            for n in nodes[boxed]:
                if n["leaf"] >> 28 == 1 and (n["leaf"] >> 24) & 15 == 1 and n["leaf"] & 0xFFFFFF == hollow[0]:      # a sphere leaf of one: the hollow one
                    c, r = spheres[hollow[0]][:3], abs(spheres[hollow[0]][3])
                    assert (n["mn"] <= c - r).all() and (n["mx"] >= c + r).all()
    assert int((runs[0]["events"] & orc.EVENTS["dielectric_back_face"] != 0).sum()) > 200
    for q in runs[1:]:
        for k in ("radiance", "segments", "terminal", "events"):
            assert q[k].tobytes() == runs[0][k].tobytes(), k


def test_scenes_reach_all_four_variants(pkg):
    assert {P.scene(pkg, s, "own")[1] for s in P.SCENES} == {"0", "mesh", "box", "all"} | set(P.NEW_INSTANCES)        # every instance pick_variant can choose
    assert set(P.MEASURED_F32_ORACLE) == {(s, f) for s in P.SCENES for f in P.FORMS}


@pytest.mark.parametrize("name,form,depth", P.CASES)
def test_cap_on_undecidable_samples(pkg, orc, name, form, depth):
    c = P.decide(pkg, orc, name, form, depth)
    und = int((~c["decidable"]).sum())
    assert und <= P.CAP * c["decidable"].size, (und, c["decidable"].size)


@pytest.mark.parametrize("name,form", [(s, f) for s in P.SCENES for f in P.FORMS])
def test_every_branch_is_covered_by_decidable_samples(pkg, orc, name, form):
    c = P.decide(pkg, orc, name, form, 8)
    need = [n for n in P.REQUIRED[name] if form == "own" or n != "lambertian_cosine_only"] + (P.REQUIRED_ALL_FORM if form == "all" else [])
    got = {n: int((c["decidable"] & ((c["base"]["events"] & orc.EVENTS[n]) != 0)).sum()) for n in need}
    assert all(k >= P.COVERAGE for k in got.values()), got


def test_every_event_bit_is_required_somewhere(orc):
    assert set(orc.EVENT_NAMES) == {n for need in P.REQUIRED.values() for n in need} | set(P.REQUIRED_ALL_FORM) | set(P.MEASURE_ZERO)
    assert not set(P.MEASURE_ZERO) & {n for need in P.REQUIRED.values() for n in need}


def test_nonfinite_samples_are_covered(pkg, orc):
    for form in P.FORMS:
        c = P.decide(pkg, orc, "lights_default", form, 8)
        assert int((c["decidable"] & (c["base"]["terminal"] == orc.TERM_NONFINITE)).sum()) >= P.COVERAGE


@pytest.mark.parametrize("name,form,depth", P.CASES)
def test_f32_checker_follows_every_decidable_sample(pkg, orc, name, form, depth):
    """The f32 checker plays the device: on every decidable sample it has the f64 run's segment count, terminal code and event mask, and
    its radiance is within the figure recorded for the scene (MEASURED_F32_ORACLE, + 10 %: the table was measured with one libm, and an
    ulp of sin / cos / log in an f32 path moves a figure of 1e-5 by a few per cent)."""
    c = P.decide(pkg, orc, name, form, depth)
    dec, a, b = c["decidable"], c["base"], c["f32"]
    for k in ("segments", "terminal", "events"):
        wrong = np.argwhere(dec & (a[k] != b[k]))
        assert len(wrong) == 0, (k, [(tuple(int(v) for v in i), P.describe(orc, int(a["events"][tuple(i)])), P.describe(orc, int(b["events"][tuple(i)]))) for i in wrong[:4]])
    dev = P.deviation(b["radiance"], a["radiance"])
    worst = float(dev[dec].max())
    print(f"{name}/{form}/depth {depth}: {dec.size} samples, {int((~dec).sum())} undecidable, {int(dec.sum())} compared, worst f32-checker figure {worst:.3e}")
    i = np.unravel_index(np.argmax(np.where(dec, dev, -1.0)), dev.shape)
    assert worst <= 1.1 * P.MEASURED_F32_ORACLE[(name, form)], (worst, tuple(int(v) for v in i), P.describe(orc, int(a["events"][i])))
