"""Area lights of every shape, without a GPU (include/rt_hip.h: RtSceneDesc.scene_flags, "light-sample queries").

The ABI (sizes, offsets, symbols, refusals), what the scene compiler makes of a lights list under RT_SCENE_LIGHTS_ALL_SHAPES, and the numpy
restatement light_reference against the oracle's XzRect::pdf_value and against closed-form solid angles. It also checks what the GPU tests
rely on: that their query points leave at most 2 % of the queries undecidable in f64, that the 8 x 8 footprint average of the form factor
has converged, and that the frame criterion of the Cornell comparison passes its null case (the oracle at two seeds)."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lights_cases as LC  # noqa: E402


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_offsets_match_the_header(pkg, tmp_path):
    A = pkg._abi
    src = tmp_path / "sz.c"
    names = ["RtSceneDesc", "RtUploadOptions", "RtLightQuery", "RtLightSample", "RtLightQueryOptions"]
    offs = [("RtSceneDesc", "scene_flags"), ("RtSceneDesc", "hittables"), ("RtSceneDesc", "bvh_seed"), ("RtLightQuery", "flags"), ("RtLightQuery", "rng_state"),
            ("RtLightQuery", "d"), ("RtLightSample", "pdf"), ("RtLightSample", "light"), ("RtLightSample", "n_draws"), ("RtLightQueryOptions", "flags")]
    body = "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names)
    body += "".join(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for s, f in offs)
    body += 'printf("flag %u\\n", (unsigned)RT_SCENE_LIGHTS_ALL_SHAPES); printf("given %u\\n", (unsigned)RT_LIGHTQ_DIRECTION_GIVEN);'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){' + body + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for n in names:
        assert int(got[n]) == C.sizeof(getattr(A, n)), n
    for s, f in offs:
        assert int(got[f"{s}.{f}"]) == getattr(getattr(A, s), f).offset, (s, f)
    # the flag took the place of a padding word: the descriptor and the upload options are the size they were
    assert int(got["RtSceneDesc"]) == 152 and int(got["RtSceneDesc.scene_flags"]) == 4 and int(got["RtUploadOptions"]) == 40
    assert (int(got["RtLightQuery"]), int(got["RtLightSample"]), int(got["RtLightQueryOptions"])) == (40, 24, 8)
    assert int(got["flag"]) == A.RT_SCENE_LIGHTS_ALL_SHAPES == 1 and int(got["given"]) == A.RT_LIGHTQ_DIRECTION_GIVEN == 1
    assert pkg.LIGHTQUERY_DTYPE.itemsize == 40 and pkg.LIGHTSAMPLE_DTYPE.itemsize == 24
    assert pkg.LIGHTQUERY_DTYPE.fields["rng_state"][1] == 16 and pkg.LIGHTSAMPLE_DTYPE.fields["light"][1] == 16


def test_symbols_are_declared_exported_and_bound(pkg):
    A = pkg._abi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_hip.h")).read(), flags=re.S)
    raw = C.CDLL(pkg.lib_path())
    rs = open(os.path.join(ROOT, "docs", "gpu_ffi.rs")).read()
    for name in ("rt_sample_lights", "rt_sample_lights_device"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in A.RT_HIP_SYMBOLS and hasattr(raw, name), name
        assert len(getattr(pkg.lib(), name).argtypes) == 7 and ("pub fn %s(" % name) in rs
    assert "pub scene_flags: u32" in rs and "scene_flags: 0" in open(os.path.join(ROOT, "docs", "scene_flatten.rs")).read()
    assert callable(pkg.Context.sample_lights) and callable(pkg.Context.light_pdf)
    # without a context nothing is touched
    q, out = (A.RtLightQuery * 2)(), (A.RtLightSample * 2)()
    assert pkg.lib().rt_sample_lights(None, None, None, C.cast(q, C.c_void_p), 2, C.cast(out, C.c_void_p), None) == A.RT_ERR_INVALID
    assert b"ctx" in pkg.lib().rt_last_error(None)
    assert pkg.lib().rt_sample_lights_device(None, None, None, None, 0, None, None) == A.RT_ERR_INVALID


def test_the_header_states_the_linear_cost_limit():
    text = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert "linear in the number of lights" in text and "no light BVH" in text


def _simple(pkg, light_of, flag=True, in_world=True):
    """a floor and one light built by light_of(builder, lamp material) -> hittable id"""
    b = pkg.SceneBuilder()
    lamp, grey = b.diffuse_light((4, 4, 4)), b.lambertian((0.7, 0.7, 0.7))
    light = light_of(b, lamp)
    ids = light if isinstance(light, list) else [light]
    world = b.hittable_list([b.xz_rect(-5, 5, -5, 5, 0, grey)] + (ids if in_world else []))
    return b.desc(world, b.hittable_list(ids), lights_all_shapes=flag), b


def test_scene_flags_refusals(pkg):
    A = pkg._abi
    desc, keep = _simple(pkg, lambda b, m: b.xz_rect(-1, 1, -1, 1, 3, m))
    assert desc.scene_flags == A.RT_SCENE_LIGHTS_ALL_SHAPES
    assert pkg.compile_info(desc)["n_lights"] == 1
    for bad in (2, 3, 1 << 31):
        desc.scene_flags = bad
        with pytest.raises(pkg.RtError) as e:
            pkg.compile_info(desc)
        assert e.value.code == A.RT_ERR_INVALID and "scene_flags" in str(e.value) and "unknown bit" in str(e.value)
    desc.scene_flags = 0
    assert pkg.compile_info(desc)["features"] & A.RT_FEATURE_LIGHTS_EXT == 0


# ---- the scene compiler -----------------------------------------------------------------------------------------------------------------------------
TRI = ((-1, 3, -1), (1, 3, -1), (0, 3, 1))
NEEDS_BIT = {
    "xz_rect": (lambda b, m: b.xz_rect(-1, 1, -1, 1, 3, m), False),
    "sphere": (lambda b, m: b.sphere((0, 3, 0), 0.5, m), False),
    "xz_rect_and_sphere": (lambda b, m: [b.xz_rect(-1, 1, -1, 1, 3, m), b.sphere((0, 3, 0), 0.5, m)], False),
    "xy_rect": (lambda b, m: b.xy_rect(-1, 1, 2, 3, 1, m), True),
    "yz_rect": (lambda b, m: b.yz_rect(2, 3, -1, 1, 1, m), True),
    "triangle": (lambda b, m: b.triangle(*TRI, m), True),
    "box": (lambda b, m: b.box((-1, 2, -1), (1, 3, 1), m), True),
    "flipped_xz_rect": (lambda b, m: b.flip_face(b.xz_rect(-1, 1, -1, 1, 3, m)), True),
    "translated_sphere": (lambda b, m: b.translate(b.sphere((0, 3, 0), 0.5, m), (1, 0, 0)), True),
    "six_wrappers": (lambda b, m: b.translate(b.rotate_y(b.flip_face(b.translate(b.rotate_y(b.translate(b.triangle(*TRI, m), (1, 0, 0)), 10), (0, 1, 0))), 20), (0, 0, 1)), True),
    "mixed": (lambda b, m: [b.xz_rect(-1, 1, -1, 1, 3, m), b.triangle(*TRI, m)], True),
}


@pytest.mark.parametrize("name", sorted(NEEDS_BIT))
def test_compile_info_counts_the_lights_and_sets_the_bit_when_needed(pkg, name):
    A = pkg._abi
    make, needs = NEEDS_BIT[name]
    desc, keep = _simple(pkg, make)
    info = pkg.compile_info(desc)
    n = len(keep.children) - (keep.hittables[desc.world].n_children)
    assert info["n_lights"] == n >= 1
    assert bool(info["features"] & A.RT_FEATURE_LIGHTS_EXT) == needs, (name, info["features"])
    assert info["features"] & 64                                        # F_LIGHTS
    # with the flag clear the same list compiles as it always did (LK_DEFAULT for what the reference cannot sample), without the bit
    off, keep2 = _simple(pkg, make, flag=False)
    info_off = pkg.compile_info(off)
    assert info_off["n_lights"] == n and info_off["features"] == info["features"] & ~A.RT_FEATURE_LIGHTS_EXT


REFUSED = {
    "moving_sphere": (lambda b, m: b.moving_sphere((0, 3, 0), (0, 3.5, 0), 0.0, 1.0, 0.5, m), "moving sphere"),
    "medium": (lambda b, m: b.constant_medium(b.sphere((0, 3, 0), 0.5, m), 0.5, (1, 1, 1)), "medium"),
    "nested_list": (lambda b, m: b.hittable_list([b.xz_rect(-1, 1, -1, 1, 3, m)]), "nested list"),
    "bvh": (lambda b, m: b.bvh([b.sphere((0, 3, 0), 0.5, m), b.sphere((2, 3, 0), 0.5, m)]), "BVH"),
    "flat_triangle": (lambda b, m: b.triangle((0, 3, 0), (1, 3, 0), (2, 3, 0), m), "triangle of zero area"),
    "point_triangle": (lambda b, m: b.triangle((0, 3, 0), (0, 3, 0), (0, 3, 0), m), "triangle of zero area"),
    "thin_rect": (lambda b, m: b.xy_rect(-1, 1, 2, 2, 1, m), "rect of zero area"),
    "thin_wrapped_rect": (lambda b, m: b.translate(b.xz_rect(1, 1, -1, 1, 3, m), (0, 1, 0)), "rect of zero area"),
    "seven_wrappers": (lambda b, m: b.flip_face(b.translate(b.rotate_y(b.flip_face(b.translate(b.rotate_y(b.translate(b.triangle(*TRI, m), (1, 0, 0)), 10), (0, 1, 0))), 20),
                                                             (0, 0, 1))), "more than 6"),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_what_the_flag_refuses_is_refused_with_its_reason(pkg, name):
    A = pkg._abi
    make, word = REFUSED[name]
    desc, keep = _simple(pkg, make, in_world=False)          # (the world need not hold it: the refusal is the lights list's)
    with pytest.raises(pkg.RtError) as e:
        pkg.compile_info(desc)
    assert e.value.code == A.RT_ERR_INVALID and word in str(e.value) and "lights list member 0" in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        pkg.lights.lights_of(desc)
    desc.scene_flags = 0                                     # the reference's rule: such a member takes the trait defaults
    assert pkg.compile_info(desc)["n_lights"] == 1


def test_builder_json_and_fingerprint_carry_the_flag(pkg):
    A = pkg._abi
    doc = json.load(open(os.path.join(ROOT, "examples", "cornell_box.json")))
    plain = pkg.JsonScene(doc)
    assert plain.desc.scene_flags == 0
    on = pkg.JsonScene(dict(doc, lights_all_shapes=True))
    assert on.desc.scene_flags == A.RT_SCENE_LIGHTS_ALL_SHAPES
    assert pkg.compile_info(on.desc) == pkg.compile_info(plain.desc)            # an XzRect and a Sphere: nothing changes
    with pytest.raises(ValueError):
        pkg.JsonScene(dict(doc, lights_all_shapes=1))
    fp = pkg.scene_fingerprint(plain.desc)
    assert pkg.scene_fingerprint(on.desc) != fp
    on.desc.scene_flags = 0
    assert pkg.scene_fingerprint(on.desc) == fp
    b = pkg.SceneBuilder()
    w = b.hittable_list([b.sphere((0, 0, 0), 1, b.lambertian((0.5, 0.5, 0.5)))])
    assert b.desc(w).scene_flags == 0 and b.desc(w, -1, True).scene_flags == 1 and b.desc(w, lights_all_shapes=True).scene_flags == 1


# ---- light_reference against the oracle and against closed forms ---------------------------------------------------------------------------------
def _one_light(pkg, make):
    desc, keep = _simple(pkg, make)
    return desc, keep


def _orc_pdf(orc, abk, o, v):
    f = lambda a: (C.c_double * len(a))(*[float(x) for x in a])
    return orc.lib().orc_xzrect_pdf_value(f(abk), f(o), f(v))


def test_rect_pdfs_are_the_oracles_xz_rect_pdf(pkg, orc):
    """Every orientation, and a rect under Translate(RotateY(30)), evaluates XzRect::pdf_value (aarect.rs:107-117) after a change of coordinates:
    a permutation of the axes, or the inverse rigid map. Inputs are f32 values, exact in f64; 1e-12 relative."""
    rng = np.random.default_rng(5)
    abk = (-1.0, 1.5, -0.5, 2.0, 3.0)
    th = math.radians(30.0)
    off = np.array([0.5, 0.25, -0.75])
    mid = np.array([0.25, 3.0, 0.75])                                                                      # the XzRect's centre
    turned = np.array([math.cos(th) * mid[0] + math.sin(th) * mid[2], mid[1], -math.sin(th) * mid[0] + math.cos(th) * mid[2]]) + off
    cases = {
        "xz": (lambda b, m: b.xz_rect(*abk, m), lambda o, v: (o, v), mid),
        "xy": (lambda b, m: b.xy_rect(*abk, m), lambda o, v: (o[[0, 2, 1]], v[[0, 2, 1]]), mid[[0, 2, 1]]),   # (x, y, z) -> (x, z, y): a = x, b = y, k on z
        "yz": (lambda b, m: b.yz_rect(*abk, m), lambda o, v: (o[[1, 0, 2]], v[[1, 0, 2]]), mid[[1, 0, 2]]),   # a = y, b = z, k on x
        "wrapped": (lambda b, m: b.translate(b.rotate_y(b.xz_rect(*abk, m), 30.0), tuple(off)), None, turned),
    }
    n_hit = 0
    for name, (make, to_xz, centre) in cases.items():
        desc, keep = _one_light(pkg, make)
        o = rng.uniform(-2, 2, (400, 3)).astype(np.float32)
        v = (centre + rng.uniform(-2.5, 2.5, (400, 3)) - o).astype(np.float32)                             # towards the rect and past its edges
        got = pkg.light_reference(desc, o, dirs=v)["pdf"]
        for i in range(400):
            oi, vi = o[i].astype(np.float64), v[i].astype(np.float64)
            if to_xz is None:
                # the compiler rounds the composed map to f32 (sin, cos, offset): hand the oracle the ray moved by that same map
                s, c = float(np.float32(math.sin(th))), float(np.float32(math.cos(th)))
                m = oi - off.astype(np.float32).astype(np.float64)
                ol, vl = np.array([c * m[0] - s * m[2], m[1], s * m[0] + c * m[2]]), np.array([c * vi[0] - s * vi[2], vi[1], s * vi[0] + c * vi[2]])
            else:
                ol, vl = to_xz(oi, vi)
            want = _orc_pdf(orc, abk, ol, vl)
            assert got[i] == pytest.approx(want, rel=1e-12, abs=0.0), (name, i, got[i], want)
            n_hit += want > 0
    assert n_hit > 400


def _mean_inverse_pdf(pkg, desc, p, n=200_000):
    rng = np.random.default_rng(11)
    states = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    r = pkg.light_reference(desc, np.tile(np.asarray(p, np.float32), (n, 1)), states)
    w = 1.0 / r["pdf"]
    assert np.isfinite(w).all()
    return float(w.mean()), float(w.std(ddof=1) / math.sqrt(n)), r


def test_triangle_samples_integrate_to_its_solid_angle(pkg):
    tri = ((-1.0, 2.5, -1.0), (1.25, 3.0, -0.5), (0.0, 2.25, 1.25))
    desc, keep = _one_light(pkg, lambda b, m: b.triangle(*tri, m))
    p = (0.25, -0.5, 0.5)
    mean, se, r = _mean_inverse_pdf(pkg, desc, p)
    omega = pkg.solid_angle_triangle(np.array(p), *map(np.array, tri))
    print(f"triangle: mean 1/pdf {mean:.6f} +- {se:.6f}, solid angle {omega:.6f}")
    assert abs(mean - omega) <= 5.0 * se and se < 0.01 * omega
    assert (r["n_draws"] == 3).all() and (r["light"] == 0).all()


def test_box_samples_integrate_to_its_solid_angle(pkg):
    p0, p1 = np.array((-0.5, 2.0, -0.5)), np.array((0.75, 3.0, 0.5))
    desc, keep = _one_light(pkg, lambda b, m: b.box(tuple(p0), tuple(p1), m))
    p = np.array((1.5, -0.5, -1.25))
    mean, se, r = _mean_inverse_pdf(pkg, desc, p)
    # every ray through a box crosses two of its sides: the silhouette's solid angle is half the sum over the six rects
    omega = 0.0
    for axis in range(3):
        u, w = [a for a in range(3) if a != axis]
        for k in (p0[axis], p1[axis]):
            c = np.zeros((4, 3))
            c[:, axis] = k
            c[:, u] = [p0[u], p1[u], p1[u], p0[u]]
            c[:, w] = [p0[w], p0[w], p1[w], p1[w]]
            omega += pkg.solid_angle_triangle(p, c[0], c[1], c[2]) + pkg.solid_angle_triangle(p, c[0], c[2], c[3])
    omega *= 0.5
    print(f"box: mean 1/pdf {mean:.6f} +- {se:.6f}, solid angle {omega:.6f}")
    assert abs(mean - omega) <= 5.0 * se and se < 0.01 * omega
    assert (r["n_draws"] == 4).all()                          # the list's pick, the side, the rect's two


# ---- what the GPU tests rely on ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.QUERY_CASES)
def test_query_points_leave_few_undecidable_queries(pkg, name):
    desc, keep, box = LC.query_case(pkg, name)
    pts, states = LC.query_points(name, box)
    r64, ok, dev_d, dev_pdf = LC.deviations(pkg, desc, pts, states)
    share = 1.0 - ok.mean()
    print(f"{name}: undecidable {share:.4f}, f32 against f64: d {dev_d:.3e} of |d|, pdf {dev_pdf:.3e} relative, lights picked {sorted(set(r64['light']))}")
    assert share <= LC.SKIP_SHARE
    assert (r64["pdf"][ok] > 0).all()                         # a drawn direction meets the light it was drawn on
    assert len(set(r64["light"])) == pkg.compile_info(desc)["n_lights"]
    assert dev_d < 1e-5 and dev_pdf < 1e-3


@pytest.mark.parametrize("name", LC.EMITTER_CASES)
def test_the_footprint_average_of_the_form_factor_has_converged(pkg, name):
    """The expected frame of the direct-lighting test, on an 8 x 8 and a 4 x 4 sub-grid of every pixel's footprint. (The GPU test holds the
    difference to a tenth of the median standard error it measures; here: 2e-3 of the brightest pixel, below any SE 256 samples give.)"""
    desc, keep, faces, view = LC.emitter_case(pkg, name)
    cam = LC.camera(pkg, *LC.CAM_FLOOR)
    e8, e4 = LC.expected_frame(cam, faces, 8), LC.expected_frame(cam, faces, 4)
    print(f"{name}: expected pixel values {e8.min():.4f} .. {e8.max():.4f}, lit pixels {(e8 > 0).mean():.2f}, max |8x8 - 4x4| {np.abs(e8 - e4).max():.2e}")
    assert e8.max() > 0.03 and (e8 > 0).mean() > 0.3
    assert np.abs(e8 - e4).max() <= 2e-3 * e8.max()
    assert pkg.compile_info(desc)["features"] & pkg._abi.RT_FEATURE_LIGHTS_EXT


def test_the_frame_criterion_passes_its_null_case(pkg, orc):
    """The flag-off Cornell box, 64 x 64, 64 spp, depth 50, by the f64 oracle at two seeds: |mean z| <= 6 / sqrt(N) and at most 1 % of the pixels
    beyond |z| = 4, per channel. The oracle's values: mean z +0.0036, +0.0066, +0.0104 (bound 0.0938); share beyond 4: 0.0000 on every channel."""
    js = pkg.JsonScene(LC.cornell_doc(False))
    cam = js.camera(1.0)
    frames = []
    for seed in (1, 2):
        prm = pkg.make_params(64, 64, 64, max_depth=50, seed=seed)
        out = orc.render(js.desc, cam, prm, precision=64, n_threads=8, per_sample=True)
        L = np.nan_to_num(out[2], nan=0.0, posinf=0.0, neginf=0.0)         # RT_NAN_PER_SAMPLE: a non-finite sample counts 0
        frames.append((L.sum(axis=2), (L * L).sum(axis=2)))
    z = LC.frame_z(frames[0][0], frames[0][1], frames[1][0], frames[1][1], 64)
    for c in range(3):
        zc = z[..., c]
        print(f"channel {c}: mean z {zc.mean():+.4f} (bound {6 / math.sqrt(zc.size):.4f}), share |z| > 4: {(np.abs(zc) > 4).mean():.4f}")
        assert LC.check_z(zc)
