"""Environment maps without a device (include/rt_hip.h RtEnvMap): the tables of the upload against the numpy statement, the statement's own
consistency (the pdf integrates to 1, a drawn direction looks up the texel it was drawn from, both estimators of a floor's radiance are
unbiased), every refusal with its pinned text, the struct_bytes rule, the .hdr reader. tests/environment.py has the helpers."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import environment as EV  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusals_env.json")


def _maps():
    one = np.zeros((8, 16, 3), np.float32)
    one[5, 11] = (0.0, 3.0, 0.5)
    zero_row = EV.random_map(9)
    zero_row[3] = 0.0
    zero_row[7] = 0.0                                       # ... and the last row: the marginal reaches 1 before its forced last entry
    return {"random": EV.random_map(), "zero_row": zero_row, "one_by_one": np.full((1, 1, 3), 0.25, np.float32), "one_texel": one,
            "odd": EV.random_map(4, W=15, H=7)}


# ---- 1. the tables ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random", "zero_row", "one_by_one", "one_texel", "odd"])
def test_tables_of_the_upload_are_the_statements(pkg, name):
    rgb = _maps()[name]
    env = pkg.EnvMap(rgb)
    marg, cond = pkg.env_tables(env)
    ref = pkg.env_reference(env, dirs=np.float32([[0, 1, 0]]))
    assert np.array_equal(marg.view(np.uint32), ref["marg"].view(np.uint32)) and np.array_equal(cond.view(np.uint32), ref["cond"].view(np.uint32))
    assert marg[-1] == 1.0 and (cond[:, -1] == 1.0).all() and (np.diff(marg) >= 0).all() and (np.diff(cond, axis=1) >= 0).all()
    if name == "zero_row":
        W = rgb.shape[1]
        assert np.array_equal(cond[3], ((np.arange(W) + 1.0) / W).astype(np.float32)) and marg[3] == marg[2] and marg[6] == 1.0
    if name == "one_texel":                                  # all the mass in one texel: the searches can only end there
        assert marg[4] == 0.0 and marg[5] == 1.0 and cond[5, 10] == 0.0 and cond[5, 11] == 1.0
    # an unsampled map of zero weight is legal and gets uniform tables; sampled, it is refused (test 4)
    if name == "random":
        m0, c0 = pkg.env_tables(pkg.EnvMap(np.zeros((4, 4, 3), np.float32), sampled=False))
        assert np.array_equal(m0, np.float32([0.25, 0.5, 0.75, 1.0])) and np.array_equal(c0[2], m0)


# ---- 2. the pdf integrates to 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random", "zero_row", "one_texel", "odd"])
def test_reference_pdf_integrates_to_one(pkg, name):
    """Midpoint rule on a 24 x 24 grid of every texel, in f64. Inside a texel pdf(w) sin(theta) is the constant mass W H / (2 pi^2), so the rule
    is exact up to rounding: what is left is the f32 rounding of the two cdfs, whose differences telescope — at most (W + H) half ulps of 1,
    1.5e-6 for 16 x 8 — and the f64 arithmetic of 73 728 terms, below 1e-10. Bound: 2e-6."""
    rgb = _maps()[name]
    env = pkg.EnvMap(rgb)
    H, W = rgb.shape[:2]

    def f(TH, PH, j, i):
        r = pkg.env_reference(env, dirs=EV.direction(TH, PH).reshape(-1, 3).astype(np.float32), dtype=np.float64)
        assert (r["i"] == i).all() and (r["j"] == j).all()        # grid points are texel interiors: the lookup finds the texel
        return r["pdf"].reshape(TH.shape)
    # (the directions are rounded to f32 on the way in, so the pdf's own sin(theta) and the quadrature weight's differ by 1e-7 relative, away
    #  from the poles: also inside the bound)
    total = EV.texel_quadrature(W, H, f, n=24).sum()
    print(f"{name}: integral of the reference pdf over the sphere = {total:.9f}")
    assert abs(total - 1.0) <= 2e-6


# ---- 3. a drawn direction looks up its texel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_drawn_direction_looks_up_the_texel_it_was_drawn_from(pkg, dtype):
    env = pkg.EnvMap(EV.sun_map())
    states = np.random.default_rng(2).integers(0, 1 << 63, 65536, dtype=np.uint64)
    r = pkg.env_reference(env, states=states, dtype=dtype)
    inside = r["border"] >= EV.BORDER
    print(f"{np.dtype(dtype).name}: {1.0 - inside.mean():.5f} of the draws within {EV.BORDER} texel of a border")
    assert 1.0 - inside.mean() <= 0.002                      # 2 BORDER per axis and texel, uniformly: 4e-4 expected
    assert (r["drawn_i"][inside] == r["i"][inside]).all() and (r["drawn_j"][inside] == r["j"][inside]).all()
    assert (r["n_draws"] == 2).all() and (r["pdf"][inside] > 0).all()
    # the sun's texel holds 200 / (200 + ~0.55 * 127 * ..) of the weight: it is drawn about that often
    share = ((r["drawn_j"] == 2) & (r["drawn_i"] == 5)).mean()
    m, c = r["marg"].astype(np.float64), r["cond"].astype(np.float64)
    mass = (m[2] - m[1]) * (c[2, 5] - c[2, 4])
    assert abs(share - mass) <= 5.0 * math.sqrt(mass * (1.0 - mass) / len(states)), (share, mass)


def test_the_reference_estimators_of_a_floor_are_unbiased(pkg):
    """GPU test c's premise, on the CPU: with the statement's own draw and pdf, the mixture estimator and the cosine-only one both meet the
    quadrature value (relative error < 1e-5, tests/environment.py) within 5 standard errors, on 262 144 numpy draws; the mixture's standard
    error is the smaller."""
    rgb = EV.sun_map()
    env = pkg.EnvMap(rgb)
    expect = EV.FLOOR_ALBEDO / math.pi * EV.floor_irradiance_integral(rgb)[1]
    est = EV.floor_estimators(pkg, env, EV.FLOOR_ALBEDO, 262144)
    for k, (mean, se) in est.items():
        print(f"{k}: mean {mean:.5f} se {se:.5f} expected {expect:.5f} z {(mean - expect) / se:+.2f}")
        assert abs(mean - expect) <= 5.0 * se + 1e-5 * expect, k
    assert est["sampled"][1] < est["unsampled"][1]


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------
def _refusal_cases(pkg):
    A = pkg._abi
    good = EV.random_map()

    def env(rgb=good, **kw):
        return pkg.EnvMap(rgb, **kw)

    def edit(**fields):
        e = env()
        for k, v in fields.items():
            setattr(e.record, k, v)
        return e
    nan, neg, inf = good.copy(), good.copy(), good.copy()
    nan[2, 3, 1], neg[0, 0, 0], inf[7, 15, 2] = np.nan, -0.5, np.inf
    b = pkg.SceneBuilder()
    lamp = b.xz_rect(-1, 1, -1, 1, 3.0, b.diffuse_light((4,) * 3))
    many = b.desc(b.hittable_list([b.xz_rect(-5, 5, -5, 5, 0.0, b.lambertian((0.5,) * 3)), lamp]), b.hittable_list([lamp]), lights_all_shapes=True, lights_many=True)
    plain = EV.floor_scene(pkg)
    cases = [("struct_bytes=0", edit(struct_bytes=0)), ("struct_bytes=sizeof-8", edit(struct_bytes=C.sizeof(A.RtEnvMap) - 8)), ("flags=2", env(flags=2)),
             ("width=0", edit(width=0)), ("height=0", edit(height=0)), ("width=16385", edit(width=16385)), ("height=16385", edit(height=16385)),
             ("rgb=NULL", edit(rgb=C.POINTER(C.c_float)())), ("texel=nan", env(nan)), ("texel=negative", env(neg)), ("texel=inf", env(inf)),
             ("scale=-1", env(scale=-1.0)), ("scale=nan", env(scale=float("nan"))), ("scale=inf", env(scale=float("inf"))),
             ("sampled,zero-weight", env(np.zeros((8, 16, 3), np.float32))), ("sampled,lights-many", env()), ("unsampled,lights-many", env(sampled=False))]
    return [(name, e, many if "lights-many" in name else plain[0], (many, plain, b)) for name, e in cases]


def test_every_refusal_with_its_text(pkg):
    A, lib = pkg._abi, pkg.lib()
    with open(GOLDEN) as f:
        pinned = json.load(f)
    got = []
    for name, e, desc, keep in _refusal_cases(pkg):
        info = A.RtCompileInfo()
        opt = pkg.upload_options(env_map=e)
        code = lib.rt_scene_compile_info_ex(C.byref(desc), C.byref(opt), C.byref(info))
        got.append(dict(case=name, code=code, error=lib.rt_last_error(None).decode()))
    assert [g["case"] for g in got] == [p["case"] for p in pinned]
    assert len(pinned) == 17 and all(p["code"] == A.RT_ERR_INVALID and p["error"] for p in pinned)
    for g, p in zip(got, pinned):
        assert (g["code"], g["error"]) == (p["code"], p["error"]), p["case"]
    # rt_env_tables makes the same checks (it has no scene: the RT_SCENE_LIGHTS_MANY rule is the upload's)
    for name, e, desc, keep in _refusal_cases(pkg):
        if "lights-many" in name:
            continue
        with pytest.raises(pkg.RtError) as err:
            pkg.env_tables(e)
        assert err.value.code == A.RT_ERR_INVALID, name
    # and the legal neighbours compile: scale 0, a zero map unsampled, 1 x 1
    for e in (pkg.EnvMap(EV.random_map(), scale=0.0), pkg.EnvMap(np.zeros((2, 2, 3), np.float32), sampled=False), pkg.EnvMap(np.ones((1, 1, 3), np.float32))):
        assert pkg.compile_info(EV.floor_scene(pkg)[0], env_map=e)["features"] & A.RT_FEATURE_ENV


# ---- 5. the struct grows at its end -----------------------------------------------------------------------------------------------------------
def test_a_40_byte_options_record_compiles_the_same_scene(pkg):
    """RtUploadOptions stays the 40 bytes its callers compiled; the grown record is RtUploadOptionsEnv, 48, the map's pointer at offset 40. What
    lies behind the caller's struct_bytes is not read, whatever the memory holds."""
    A, lib = pkg._abi, pkg.lib()
    assert C.sizeof(A.RtUploadOptions) == 40 and C.sizeof(A.RtUploadOptionsEnv) == 48 and A.RtUploadOptionsEnv.env_map.offset == 40 and C.sizeof(A.RtEnvMap) == 32
    desc, keep = EV.lit_scene(pkg)
    env = pkg.EnvMap(EV.random_map())
    infos = {}
    for label, nbytes, null_field in (("none", None, False), ("24", 24, False), ("40", 40, False), ("48", 48, False), ("48-null", 48, True)):
        info = A.RtCompileInfo()
        opt = pkg.upload_options(env_map=env)                # 48 bytes of memory, the pointer set
        assert opt.struct_bytes == 48
        if nbytes is not None:
            opt.struct_bytes = nbytes                        # the caller's sizeof
        if null_field:
            opt._b_base_.env_map = None
        assert lib.rt_scene_compile_info_ex(C.byref(desc), C.byref(opt) if nbytes is not None else None, C.byref(info)) == A.RT_OK, label
        infos[label] = bytes(info)
    assert infos["24"] == infos["40"] == infos["48-null"] == infos["none"]
    f = lambda k: A.RtCompileInfo.from_buffer_copy(infos[k]).features
    assert f("48") == f("none") | A.RT_FEATURE_ENV | A.RT_FEATURE_LIGHTS_EXT and not f("none") & A.RT_FEATURE_ENV
    assert pkg.upload_options().struct_bytes == 40          # without a map: the record every caller has always sent
    # a map promotes a list of the reference's own kinds to extended records too, and a scene without a lights list
    plain = EV.floor_scene(pkg)[0]
    assert pkg.compile_info(plain)["features"] & (A.RT_FEATURE_ENV | A.RT_FEATURE_LIGHTS_EXT) == 0
    assert pkg.compile_info(plain, env_map=env)["features"] & (A.RT_FEATURE_ENV | A.RT_FEATURE_LIGHTS_EXT) == A.RT_FEATURE_ENV | A.RT_FEATURE_LIGHTS_EXT


def test_the_fingerprint_covers_the_map(pkg):
    desc, keep = EV.floor_scene(pkg)
    rgb = EV.random_map()
    other = rgb.copy()
    other[1, 2, 0] += 0.5
    prints = [pkg.scene_fingerprint(desc), pkg.scene_fingerprint(desc, env_map=pkg.EnvMap(rgb)), pkg.scene_fingerprint(desc, env_map=pkg.EnvMap(other)),
              pkg.scene_fingerprint(desc, env_map=pkg.EnvMap(rgb, sampled=False)), pkg.scene_fingerprint(desc, env_map=pkg.EnvMap(rgb, scale=2.0))]
    assert len(set(prints)) == 5
    assert prints[1] == pkg.scene_fingerprint(desc, env_map=pkg.EnvMap(rgb.copy()))


# ---- 6. the .hdr reader --------------------------------------------------------------------------------------------------------------------------
def _rgbe(r, g, b, e):
    return bytes([r, g, b, e])


def test_load_hdr_flat_and_run_length_encoded(pkg):
    head = b"#?RADIANCE\n# hand written\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n"
    # flat, 3 x 2: mantissa * 2^(e - 136); e = 0 is black whatever the mantissa holds
    px = [[(128, 64, 32, 129), (255, 0, 0, 136), (1, 2, 3, 0)], [(0, 0, 128, 128), (200, 100, 50, 120), (128, 128, 128, 137)]]
    flat = head + b"-Y 2 +X 3\n" + b"".join(_rgbe(*p) for row in px for p in row)
    img = pkg.load_hdr(flat)
    assert img.shape == (2, 3, 3) and img.dtype == np.float32
    want = np.array([[[m * 2.0 ** (p[3] - 136) if p[3] else 0.0 for m in p[:3]] for p in row] for row in px], dtype=np.float32)
    assert np.array_equal(img, want)
    assert np.array_equal(img[0, 0], np.float32([1.0, 0.5, 0.25])) and np.array_equal(img[0, 2], np.float32([0, 0, 0])) and img[1, 2, 0] == 256.0
    # run-length encoded, 8 x 2: per scanline 2 2 0 8, then each channel as runs (> 128: a run of n - 128 copies; else n literal bytes)
    row0 = bytes([2, 2, 0, 8]) + bytes([128 + 8, 128]) + bytes([128 + 3, 64, 5, 1, 2, 3, 4, 5]) + bytes([8, 0, 1, 2, 3, 4, 5, 6, 7]) + bytes([128 + 8, 129])
    row1 = bytes([2, 2, 0, 8]) + bytes([128 + 4, 10, 128 + 4, 20]) + bytes([128 + 8, 0]) + bytes([4, 9, 8, 7, 6, 128 + 4, 255]) + bytes([128 + 7, 128, 1, 0])
    img = pkg.load_hdr(head + b"-Y 2 +X 8\n" + row0 + row1)
    assert img.shape == (2, 8, 3)
    s = 2.0 ** (129 - 136)
    assert np.array_equal(img[0, :, 0], np.full(8, 128 * s, np.float32))
    assert np.array_equal(img[0, :, 1], np.float32([64, 64, 64, 1, 2, 3, 4, 5]) * np.float32(s))
    assert np.array_equal(img[0, :, 2], np.arange(8, dtype=np.float32) * np.float32(s))
    s1 = 2.0 ** (128 - 136)
    assert np.array_equal(img[1, :, 0], np.float32([10, 10, 10, 10, 20, 20, 20, 0]) * np.float32(s1))     # the last texel has e = 0: black
    assert np.array_equal(img[1, :, 2], np.float32([9, 8, 7, 6, 255, 255, 255, 0]) * np.float32(s1))
    # refused: no signature, another orientation, a truncated scanline, a run past the end of the line
    for bad in (b"P6\n", head + b"+Y 2 +X 3\n" + bytes(24), flat[:-3], head + b"-Y 1 +X 8\n" + bytes([2, 2, 0, 8, 128 + 9, 1])):
        with pytest.raises(ValueError):
            pkg.load_hdr(bad)
    # and such a picture is a map
    env = pkg.EnvMap(pkg.load_hdr(head + b"-Y 2 +X 8\n" + row0 + row1))
    assert pkg.env_tables(env)[0][-1] == 1.0


# ---- scene JSON -----------------------------------------------------------------------------------------------------------------------------------
def test_scene_json_names_a_map(pkg, tmp_path):
    doc = {"materials": {"g": {"lambertian": [0.5, 0.5, 0.5]}}, "objects": {"f": {"xz_rect": [-1, 1, -1, 1, 0], "material": "g"}}, "world": {"list": ["f"]},
           "environment": {"rgb": [[[1, 1, 1], [0.5, 0.5, 0.5]], [[0, 0, 0], [2, 2, 2]]], "sampled": False, "scale": 2.0}}
    js = pkg.JsonScene(doc)
    assert (js.env_map.width, js.env_map.height, js.env_map.scale, js.env_map.sampled) == (2, 2, 2.0, False)
    assert pkg.compile_info(js.desc, env_map=js.env_map)["features"] & pkg._abi.RT_FEATURE_ENV
    assert pkg.JsonScene({k: v for k, v in doc.items() if k != "environment"}).env_map is None
    # a file beside the scene: a flat 2 x 1 Radiance picture
    (tmp_path / "sky.hdr").write_bytes(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 2\n" + bytes([128, 128, 128, 129, 64, 64, 64, 130]))
    js = pkg.JsonScene(dict(doc, environment={"file": "sky.hdr"}), base_dir=str(tmp_path))
    assert js.env_map.sampled and np.array_equal(js.env_map.rgb, np.float32([[[1, 1, 1], [1, 1, 1]]]))
    for bad in ({"rgb": [[1, 2]]}, {"file": "nope.hdr"}, {"rgb": [[[1, 1, 1]]], "file": "x"}, {"rgb": [[[1, 1, 1]]], "sampled": 1}, {"rgb": [[[1, 1, 1]]], "scale": "2"},
                {"rgb": [[[1, 1, 1]]], "rotate": 90}):
        with pytest.raises(ValueError, match="environment"):
            pkg.JsonScene(dict(doc, environment=bad))
