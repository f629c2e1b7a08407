"""Normal maps without a GPU (include/rt_hip.h "normal maps"): the ABI and its refusals on the host-only compile entry points,
mesh.normal_map_reference against answers known by hand, what the scene compiler reports of a mapped mesh, the JSON front-end and the
fingerprint, and the f32 figures that bound the device in tests/test_gpu_normal_maps.py — measured here, from the CPU checker alone."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_attrs as M  # noqa: E402
import normal_maps as NM  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "refusals_normal_maps.json")


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(pkg, tmp_path):
    A = pkg._abi
    body = ('printf("map %zu\\n", sizeof(RtNormalMap)); printf("maps %zu\\n", sizeof(RtUploadOptionsMaps)); printf("env %zu\\n", sizeof(RtUploadOptionsEnv));'
            'printf("options %zu\\n", sizeof(RtUploadOptions)); printf("flip %u\\n", RT_NMAP_FLIP_GREEN);')
    for T, f in (("RtNormalMap", "material"), ("RtNormalMap", "image"), ("RtNormalMap", "strength"), ("RtNormalMap", "flags"),
                 ("RtUploadOptionsMaps", "normal_maps"), ("RtUploadOptionsMaps", "n_normal_maps")):
        body += f'printf("{T}.{f} %zu\\n", offsetof({T}, {f}));'
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){' + body + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["map"] == C.sizeof(A.RtNormalMap) == 16
    assert got["env"] == C.sizeof(A.RtUploadOptionsEnv) == 48 and got["options"] == C.sizeof(A.RtUploadOptions) == 40      # the older records keep their sizes
    assert got["maps"] == C.sizeof(A.RtUploadOptionsMaps) == got["env"] + 16
    for name, off in got.items():
        if "." in name:
            T, f = name.split(".")
            assert getattr(getattr(A, T), f).offset == off, name
    assert got["flip"] == A.RT_NMAP_FLIP_GREEN == 1 and A.RT_FEATURE_NORMAL_MAP == 2048


def info_ex(pkg, desc, opt):
    A, lib = pkg._abi, pkg.lib()
    info = A.RtCompileInfo()
    rc = lib.rt_scene_compile_info_ex(C.byref(desc), C.byref(opt), C.byref(info))
    return rc, info, lib.rt_last_error(None).decode()


def small_scene(pkg):
    """Two triangles of one Lambertian (one with attributes), a sphere, a rect, a box and a medium of materials of their own, a light."""
    b = pkg.SceneBuilder()
    m = dict(tri=b.lambertian((0.5, 0.5, 0.5)), sphere=b.metal((0.8, 0.8, 0.8), 0.0), rect=b.lambertian((0.2, 0.5, 0.2)), box=b.dielectric(1.5),
             moving=b.lambertian((0.1, 0.1, 0.1)), light=b.diffuse_light((4, 4, 4)), unused=b.lambertian((0.9, 0.1, 0.1)))
    ids = [b.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), m["tri"], normals=((0, 0, 1), (0, 0.5, 1), (0.5, 0, 1)), uvs=((0, 0), (1, 0), (0, 1))),
           b.triangle((2, 0, 0), (3, 0, 0), (2, 1, 0), m["tri"]), b.sphere((0, 0, 3), 0.5, m["sphere"]), b.xy_rect(0, 1, 0, 1, -2, m["rect"]),
           b.box((4, 0, 0), (5, 1, 1), m["box"]), b.moving_sphere((0, 3, 0), (0, 3.5, 0), 0.0, 1.0, 0.3, m["moving"]),
           b.triangle((0, 0, 6), (1, 0, 6), (0, 1, 6), m["light"])]
    ids.append(b.constant_medium(b.sphere((8, 0, 0), 1.0, m["sphere"]), 0.5, (1, 1, 1)))
    m["smoke"] = len(b.materials) - 1
    img = b.normal_map(m["tri"], NM.random_map())
    b.nmaps.clear()
    b.images.append(pkg._abi.RtImage(None, 4, 4))          # an image without data (id img + 1)
    return b, b.desc(b.hittable_list(ids)), m, img


def refusal_cases(pkg):
    A = pkg._abi
    b, desc, m, img = small_scene(pkg)
    rec = lambda mat, image=img, strength=1.0, flags=0: A.RtNormalMap(mat, image, strength, flags)
    cases = [("material-out-of-range", [rec(99)]), ("material-negative", [rec(-1)]), ("material-twice", [rec(m["tri"]), rec(m["unused"]), rec(m["tri"])]),
             ("image-out-of-range", [rec(m["tri"], 99)]), ("image-negative", [rec(m["tri"], -1)]), ("image-without-data", [rec(m["tri"], img + 1)]),
             ("strength-negative", [rec(m["tri"], strength=-0.5)]), ("strength-nan", [rec(m["tri"], strength=float("nan"))]), ("strength-inf", [rec(m["tri"], strength=float("inf"))]),
             ("unknown-flag", [rec(m["tri"], flags=2)]), ("diffuse-light", [rec(m["light"])]), ("isotropic", [rec(m["smoke"])]),
             ("on-a-sphere", [rec(m["sphere"])]), ("on-a-rect", [rec(m["rect"])]), ("on-a-box", [rec(m["box"])]), ("on-a-moving-sphere", [rec(m["moving"])])]
    # two cases that need a desc of their own: an image with data and a zero dimension (no scene with one compiles), and a medium whose
    # phase material is not an Isotropic (so that the triangles-only rule is what refuses it)
    bz = pkg.SceneBuilder()
    mz = bz.lambertian((0.5, 0.5, 0.5))
    tz = bz.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), mz)
    iz = bz.normal_map(mz, NM.random_map())
    bz.images[iz].width = 0
    dz = bz.desc(bz.hittable_list([tz]))
    bm = pkg.SceneBuilder()
    mm = bm.lambertian((0.5, 0.5, 0.5))
    tm = bm.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), mm)
    fog = bm._hit(A.RT_HIT_CONSTANT_MEDIUM, mm, bm.sphere((8, 0, 0), 1.0, bm.metal((0.8, 0.8, 0.8), 0.0)), 1, [0.5])
    im = bm.normal_map(mm, NM.random_map())
    dm = bm.desc(bm.hittable_list([tm, fog]))
    cases = [(name, recs, desc) for name, recs in cases] + [("image-zero-dimension", [rec(mz, iz)], dz), ("on-a-medium", [rec(mm, im)], dm)]
    return (b, bz, bm), desc, m, img, cases


def test_every_refusal_with_its_text(pkg):
    A, lib = pkg._abi, pkg.lib()
    b, desc, m, img, cases = refusal_cases(pkg)
    with open(GOLDEN) as f:
        pinned = json.load(f)
    got = []
    for name, recs, d in cases:
        rc, _, err = info_ex(pkg, d, pkg.upload_options(normal_maps=recs))
        got.append(dict(case=name, code=rc, error=err))
        assert lib.rt_scene_compile_dump_ex(C.byref(d), C.byref(pkg.upload_options(normal_maps=recs)), None, 0, None, None, 0) == A.RT_ERR_INVALID, name
    opt = pkg.upload_options(normal_maps=[])
    C.cast(C.byref(opt), C.POINTER(A.RtUploadOptionsMaps)).contents.n_normal_maps = 3
    rc, _, err = info_ex(pkg, desc, opt)
    got.append(dict(case="null-pointer", code=rc, error=err))
    assert [g["case"] for g in got] == [p["case"] for p in pinned]
    assert len(pinned) == 19 and all(p["code"] == A.RT_ERR_INVALID and p["error"] for p in pinned)
    assert got == pinned
    assert all("for now" in p["error"] for p in pinned if p["case"].startswith("on-a-"))
    # the legal neighbours: strength 0, the flip flag, a mapped material no primitive uses (which changes nothing)
    plain = pkg.compile_info(desc)
    rc, info, _ = info_ex(pkg, desc, pkg.upload_options(normal_maps=[A.RtNormalMap(m["tri"], img, 0.0, A.RT_NMAP_FLIP_GREEN)]))
    assert rc == A.RT_OK and info.features & A.RT_FEATURE_NORMAL_MAP
    unused = pkg.compile_info(desc, normal_maps=[A.RtNormalMap(m["unused"], img, 1.0, 0)])
    assert unused == plain and not plain["features"] & (A.RT_FEATURE_NORMAL_MAP | A.RT_FEATURE_TRI_ATTR | 32)


def test_48_byte_options_with_maps_behind_them_have_none(pkg):
    """A caller compiled against RtUploadOptionsEnv: what lies behind its 48 bytes is not read. Neither is a pointer without its count."""
    A = pkg._abi
    b, desc, m, img = small_scene(pkg)
    opt = pkg.upload_options(normal_maps=[A.RtNormalMap(m["tri"], img, 1.0, 0)])
    assert opt.struct_bytes == 64
    rc, info, _ = info_ex(pkg, desc, opt)
    assert rc == A.RT_OK and info.features & A.RT_FEATURE_NORMAL_MAP and info.n_tri_attrs == 2
    C.cast(C.byref(opt), C.POINTER(A.RtUploadOptionsMaps)).contents.normal_maps = C.cast(C.c_void_p(8), C.POINTER(A.RtNormalMap))      # never dereferenced
    for size in (24, 40, 48, 56):
        opt.struct_bytes = size
        rc, info, err = info_ex(pkg, desc, opt)
        assert rc == A.RT_OK and not info.features & A.RT_FEATURE_NORMAL_MAP and info.n_tri_attrs == 0, (size, err)


# ---- what the compiler reports ---------------------------------------------------------------------------------------------------------------
def test_compile_info_of_a_mapped_mesh(pkg):
    """n_tri_attrs counts every device triangle that carries a record — mapped ones without attributes too —, features gets 2048 and F_TEX
    (32: the map is a texture record), with and without attributes, in every copy of an instanced triangle; and a list of no maps is no list."""
    A = pkg._abi
    b, desc, m, img = small_scene(pkg)
    maps = [A.RtNormalMap(m["tri"], img, 1.0, 0)]
    plain = pkg.compile_info(desc)
    assert plain["n_tris"] == 3 and plain["n_tri_attrs"] == 0 and not plain["features"] & 32
    with_attrs = pkg.compile_info(desc, triangle_attrs=b.triangle_attrs())
    assert with_attrs["n_tri_attrs"] == 1 and with_attrs["features"] == plain["features"] | A.RT_FEATURE_TRI_ATTR
    for attrs, n in ((None, 2), (b.triangle_attrs(), 2)):
        info = pkg.compile_info(desc, triangle_attrs=attrs, normal_maps=maps)
        assert info["n_tri_attrs"] == n and info["features"] == plain["features"] | 32 | A.RT_FEATURE_TRI_ATTR | A.RT_FEATURE_NORMAL_MAP, info
    # (128 too: a mapped triangle carries a device record, and the instances with F_TRI_ATTR are the ones that read it); an instanced triangle is mapped in every copy
    b2 = pkg.SceneBuilder()
    mat = b2.lambertian((0.5, 0.5, 0.5))
    t = b2.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), mat)
    other = b2.triangle((0, 0, 5), (1, 0, 5), (0, 1, 5), b2.lambertian((0.1, 0.1, 0.1)))
    b2.normal_map(mat, NM.random_map())
    d2 = b2.desc(b2.hittable_list([t, b2.translate(t, (3, 0, 0)), b2.rotate_y(b2.translate(t, (0, 3, 0)), 20.0), other]))
    for flags in (0, A.RT_LAYOUT_REFERENCE_COUNTERS, A.RT_LAYOUT_SCENE_IN_HBM):
        info = pkg.compile_info(d2, flags, normal_maps=b2.normal_maps())
        assert info["n_tris"] == 4 and info["n_tri_attrs"] == 3 and info["features"] & A.RT_FEATURE_NORMAL_MAP
    # the dump with options at 48 bytes and at 64 with an empty list: the same bytes
    e48, e64 = A.RtUploadOptionsEnv(), pkg.upload_options(normal_maps=[])
    e48.base.struct_bytes = 48
    assert e64.struct_bytes == 64
    dumps = []
    for opt in (e48.base, e64):
        info = A.RtCompileInfo()
        assert pkg.lib().rt_scene_compile_info_ex(C.byref(desc), C.byref(opt), C.byref(info)) == A.RT_OK
        node_t = np.dtype([("mn", np.float32, 3), ("skip", np.uint32), ("mx", np.float32, 3), ("leaf", np.uint32)])
        n_s = max(1, info.n_spheres + info.n_media)
        nodes, spheres, meta = np.zeros(info.n_nodes, node_t), np.zeros((n_s, 4), np.float32), np.zeros(n_s, np.uint32)
        assert pkg.lib().rt_scene_compile_dump_ex(C.byref(desc), C.byref(opt), nodes.ctypes.data_as(C.c_void_p), len(nodes), spheres.ctypes.data_as(C.POINTER(C.c_float)),
                                                  meta.ctypes.data_as(C.POINTER(C.c_uint32)), n_s) == A.RT_OK
        dumps.append(bytes(info) + nodes.tobytes() + spheres.tobytes() + meta.tobytes())
    assert dumps[0] == dumps[1] and len(dumps[0]) > 200


# ---- the numpy statement against answers known by hand ----------------------------------------------------------------------------------------
AXES_UV = ((0.0, 0.0), (1.0, 0.0), (0.5, 1.0))            # on BIG_VERTS: u = (x + 3) / 6, v = (y + 2) / 5 — u along +x, v along +y
MIRROR_UV = ((1.0, 0.0), (0.0, 0.0), (0.5, 1.0))          # u = 1 - (x + 3) / 6: det < 0


def big(pkg, uv):
    A = pkg._abi
    a = A.RtTriangleAttrs(0, A.RT_TRI_UVS if uv is not None else 0)
    for k in range(3):
        for c in range(2):
            a.uv[k][c] = uv[k][c] if uv is not None else 0.0
    return {0: np.array(M.BIG_VERTS)}, [a]


def at(pkg, uv, texel, bu=0.3, bv=0.2, **kw):
    tris, attrs = big(pkg, uv)
    img = np.zeros((1, 1, 3), np.uint8) + np.asarray(texel, np.uint8)
    n, ff, u, v, tx, (t, b, N, ok) = pkg.normal_map_reference(tris, attrs, [0], [bu], [bv], img, frame=True, **kw)
    assert ff is None and tx[0] == 0
    return n[0], t[0], b[0], N[0], bool(ok[0])


def test_known_answers(pkg):
    x, y, z = np.eye(3)
    n, t, b, N, ok = at(pkg, AXES_UV, (255, 128, 128))
    assert ok and np.abs(t - x).max() < 1e-15 and np.abs(b - y).max() < 1e-15 and np.abs(N - z).max() < 1e-15     # red is +u = +x, green is +v = +y
    assert np.linalg.norm(n - t) < 1e-2 and abs(np.linalg.norm(n) - 1.0) < 1e-15
    m = 1.0 / 255.0                                                                         # 128 decodes to 1 / 255
    assert np.allclose(n, np.array([1.0, m, m]) / np.sqrt(1.0 + 2.0 * m * m), atol=1e-15)
    n, *_ = at(pkg, AXES_UV, (128, 255, 128))
    assert np.linalg.norm(n - y) < 1e-2                                                     # green is +v: towards row 0 of the image, here +y
    # an orthonormal frame under vertex normals too, at any hit
    A = pkg._abi
    tris, attrs = big(pkg, M.BIG_UV)
    attrs[0].flags |= A.RT_TRI_NORMALS
    for k in range(3):
        for c in range(3):
            attrs[0].n[k][c] = M.BIG_NORMALS[k][c]
    rng = np.random.default_rng(3)
    bu = rng.uniform(0, 1, 64); bv = rng.uniform(0, 1, 64) * (1 - bu)
    ns, _, _, _, _, (t, b, N, ok) = pkg.normal_map_reference(tris, attrs, np.zeros(64, int), bu, bv, NM.random_map(), frame=True)
    assert ok.all()
    F = np.stack([t, b, N], axis=1)
    assert np.abs(F @ F.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.norm(ns, axis=1) - 1.0).max() < 1e-12
    plain = pkg.interpolate_reference(tris, attrs, np.zeros(64, int), bu, bv, -N)[0]
    assert np.abs(plain - N).max() < 1e-15 and np.linalg.norm(ns - N, axis=1).max() > 0.3  # N is interpolate_reference's, and the map moves it
    # mirrored uv: det < 0 turns t with u, and b = -cross(N, t) keeps green pointing along +v
    n, t, b, N, ok = at(pkg, MIRROR_UV, (255, 128, 128))
    assert ok and np.abs(t + x).max() < 1e-15 and np.abs(b - y).max() < 1e-15 and np.abs(b + np.cross(N, t)).max() < 1e-15 and np.linalg.norm(n + x) < 1e-2
    n0, t0, b0, _, _ = at(pkg, AXES_UV, (128, 255, 128))
    assert np.abs(b0 - np.cross(z, t0)).max() < 1e-15                                      # (unmirrored: b = +cross(N, t))
    # flip_green negates the b component and nothing else
    for uv in (AXES_UV, MIRROR_UV, None):
        n, t, b, N, _ = at(pkg, uv, (200, 90, 230))
        f, *_ = at(pkg, uv, (200, 90, 230), flip_green=True)
        assert np.isclose(f @ b, -(n @ b), atol=1e-15) and np.isclose(f @ t, n @ t, atol=1e-15) and np.isclose(f @ N, n @ N, atol=1e-15) and abs(n @ b) > 0.1
    # without RT_TRI_UVS the vertices' coordinates are (0,0), (1,0), (0,1): t along e1, and (u, v) the barycentrics
    n, t, b, N, ok = at(pkg, None, (255, 128, 128))
    assert ok and np.abs(t - x).max() < 1e-15 and np.abs(b - y).max() < 1e-15
    # strength scales the tangent-plane components: 0 returns +-N (blue below 128 points it the other way)
    assert np.abs(at(pkg, AXES_UV, (255, 0, 200), strength=0.0)[0] - z).max() < 1e-15 and np.abs(at(pkg, AXES_UV, (255, 0, 20), strength=0.0)[0] + z).max() < 1e-15
    half, full = at(pkg, AXES_UV, (255, 128, 255), strength=0.5)[0], at(pkg, AXES_UV, (255, 128, 255))[0]
    assert np.isclose(half[0] / half[2], 0.5 * full[0] / full[2])
    # fallback: collinear uv (det = 0) returns N. (No 8-bit texel decodes to a vector of zero length: 2 c / 255 - 1 is never 0.)
    n, _, _, N, ok = at(pkg, ((0.0, 0.0), (0.5, 0.5), (1.0, 1.0)), (255, 0, 128))
    assert not ok and np.abs(n - z).max() < 1e-15
    n, _, _, N, ok = at(pkg, ((0.25, 0.5), (0.25, 0.5), (0.25, 0.5)), (255, 0, 128))
    assert not ok and np.abs(n - z).max() < 1e-15
    tris, attrs = big(pkg, AXES_UV)
    ns, _, _, _, tx = pkg.normal_map_reference(tris, attrs, [0], [0.3], [0.2], np.full((1, 1, 3), 0, np.uint8) + np.uint8(0), strength=0.0)
    assert np.abs(ns[0] + z).max() < 1e-15                                                 # (0, 0, -1): a legal, inward map
    # the texel index follows the image texture's rule: v = 1 is row 0, u = 1 clamps into the last column
    i, j = pkg.texel_of([0.0, 0.999, 1.0, -3.0, 0.5], [1.0, 0.0, 0.5, 7.0, 0.4999], 16, 8)
    assert list(i) == [0, 15, 15, 0, 8] and list(j) == [0, 7, 4, 0, 4]


def test_height_to_normal_map(pkg):
    """A plane decodes to N; a ramp rising with +u leans the normal to -u, one rising towards row 0 (+v) to -v, by the angle of its slope."""
    flat = pkg.height_to_normal_map(np.zeros((4, 6)), 1.0)
    assert flat.shape == (4, 6, 3) and flat.dtype == np.uint8 and (flat == (128, 128, 255)).all()
    ramp_u = pkg.height_to_normal_map(np.tile(np.arange(6.0), (4, 1)), 1.0)
    ramp_v = pkg.height_to_normal_map(np.tile(np.arange(4.0)[::-1, None], (1, 6)), 1.0)
    s = 255 * (1 - np.sqrt(0.5)) / 2
    assert np.abs(ramp_u[..., 0].astype(float) - s).max() <= 0.5 and (ramp_u[..., 1] == 128).all() and np.abs(ramp_u[..., 2].astype(float) - (255 - s)).max() <= 0.5
    assert np.abs(ramp_v[..., 1].astype(float) - s).max() <= 0.5 and (ramp_v[..., 0] == 128).all()
    tris, attrs = big(pkg, AXES_UV)
    n = pkg.normal_map_reference(tris, attrs, [0], [0.3], [0.2], ramp_u)[0][0]
    assert np.abs(n - np.array([-1.0, 0.0, 1.0]) / np.sqrt(2.0)).max() < 1e-2


# ---- the front-ends --------------------------------------------------------------------------------------------------------------------------
def test_json_and_fingerprint(pkg):
    A = pkg._abi
    doc = {"camera": {"lookfrom": [0, 0, 5], "lookat": [0, 0, 0], "vup": [0, 1, 0], "vfov": 40, "aperture": 0, "focus_dist": 5},
           "materials": {"grey": {"lambertian": [0.5, 0.5, 0.5], "normal_map": {"image": NM.random_map().tolist(), "strength": 0.5, "flip_green": True}},
                         "red": {"lambertian": [0.7, 0.2, 0.2]}},
           "objects": {"a": {"triangle": [[0, 0, 0], [1, 0, 0], [0, 1, 0]], "material": "grey"}, "b": {"triangle": [[0, 0, 1], [1, 0, 1], [0, 1, 1]], "material": "red"}},
           "world": {"list": ["a", "b"]}}
    js = pkg.JsonScene(doc)
    assert len(js.normal_maps) == 1 and js.normal_maps[0].flags == A.RT_NMAP_FLIP_GREEN and js.normal_maps[0].strength == 0.5
    info = pkg.compile_info(js.desc, normal_maps=js.normal_maps)
    assert info["n_tri_attrs"] == 1 and info["features"] & A.RT_FEATURE_NORMAL_MAP
    for bad, word in (({"image": "nowhere.png"}, "image"), ({"image": [[1, 2]]}, "image"), ({"strength": 1.0}, "normal_map"), ({"image": [[[1, 2, 3]]], "strength": "x"}, "strength"),
                      ({"image": [[[1, 2, 3]]], "flip_green": 1}, "flip_green"), ({"image": [[[1, 2, 3]]], "wrap": True}, "normal_map")):
        doc["materials"]["grey"]["normal_map"] = bad
        with pytest.raises(ValueError, match=word):
            pkg.JsonScene(doc)
    del doc["materials"]["grey"]["normal_map"]
    assert pkg.JsonScene(doc).normal_maps is None
    # a checkpoint tells a mapped scene from an unmapped one, and one map from another
    maps = js.normal_maps
    f0, f1 = pkg.scene_fingerprint(js.desc), pkg.scene_fingerprint(js.desc, normal_maps=maps)
    assert f0 != f1 and pkg.scene_fingerprint(js.desc, normal_maps=[]) == f0 == pkg.scene_fingerprint(js.desc, None, None)
    maps[0].strength = 0.25
    f2 = pkg.scene_fingerprint(js.desc, normal_maps=maps)
    js.b._image_arrays[0][0, 0, 0] ^= 1                                                   # a texel of the bound image
    assert len({f0, f1, f2, pkg.scene_fingerprint(js.desc, normal_maps=maps)}) == 4


# ---- the bound for the GPU ray test -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NM.SCENES)
def test_f32_figures(pkg, orc, name):
    """normal_maps.MEASURED_F32[name], which bounds the device (x 2), is what the f32 statement measures against the f64 one here, within 1 %;
    the rays left out for their texel — it differs between the precisions or moves under the scene's uv bound — are at most 2 % of those
    otherwise compared (the reference alone leaves out about 2 delta (W + H) = 2e-4), and the map moves the normal."""
    ms = NM.mapped_set(pkg, orc, name)
    s = ms["base"]
    use = ms["use"]
    flat = s["n"][use]
    moved = np.linalg.norm(ms["n"][use] - flat, axis=1)
    worst, ray, ff_differs, compared, left_out = NM.f32_figures(pkg, orc, name)
    print(f"{name}: {int(use.sum())} rays in use, texel boundary {ms['boundary']:.2e}, grazing {ms['grazing']}; f32 against f64 on {compared}: |dn| {worst['n']:.3e} (ray {ray}), "
          f"front_face differs on {ff_differs}, left out {left_out:.2e}; the map moves n by {np.median(moved):.3f} (median)")
    assert use.sum() >= 800 and np.median(moved) > 0.05
    assert (np.einsum("ij,ij->i", ms["n"][use], s["rays"]["d"][use].astype(np.float64)) <= 0).all()
    assert ms["boundary"] <= NM.TEXEL_CAP and left_out <= NM.TEXEL_CAP and ms["grazing"] <= 0.01 * use.sum()
    assert ff_differs == 0
    for q, v in NM.MEASURED_F32[name].items():
        assert abs(worst[q] - v) <= 0.01 * v, (q, worst[q], v)


def test_f32_figure_of_the_triangle_without_attributes(pkg, orc):
    """The same measurement for the one mapped triangle of `wrapped` that has no RtTriangleAttrs (uv_k = (0,0), (1,0), (0,1), (u, v) the
    barycentrics): MEASURED_F32["wrapped_lone"], within 1 %, on at least 50 rays, the texel rule leaving out at most 2 %."""
    ls = NM.lone_set(pkg, orc, np.float32)
    worst = float(ls["dn32"].max())
    print(f"wrapped, the triangle without attributes (hittable {ls['hittable']}): {len(ls['k'])} rays in use, {len(ls['k32'])} compared, f32 against f64 |dn| {worst:.3e}, "
          f"front_face differs on {ls['ff32_differs']}, left out {ls['left_out']:.2e}")
    assert len(ls["k32"]) >= 50 and ls["left_out"] <= NM.TEXEL_CAP and ls["ff32_differs"] == 0
    v = NM.MEASURED_F32["wrapped_lone"]["n"]
    assert abs(worst - v) <= 0.01 * v, (worst, v)
