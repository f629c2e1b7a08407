"""Triangle attributes without a GPU (include/rt_hip.h "triangle attributes"): the ABI and its refusals on the host-only compile entry
points, mesh.interpolate_reference against answers known by hand, parse_obj_attrs and the JSON front-end, and the f32 figures that bound
the device in tests/test_gpu_mesh_attrs.py — measured here, from the CPU checker alone."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_attrs as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(pkg, tmp_path):
    A = pkg._abi
    body = 'printf("attrs %zu\\n", sizeof(RtTriangleAttrs)); printf("options %zu\\n", sizeof(RtUploadOptions)); printf("info %zu\\n", sizeof(RtCompileInfo));'
    for T, f in (("RtTriangleAttrs", "hittable"), ("RtTriangleAttrs", "flags"), ("RtTriangleAttrs", "n"), ("RtTriangleAttrs", "uv"),
                 ("RtUploadOptions", "list_park_cost"), ("RtUploadOptions", "triangle_attrs"), ("RtUploadOptions", "n_triangle_attrs"), ("RtCompileInfo", "n_tri_attrs")):
        body += f'printf("{T}.{f} %zu\\n", offsetof({T}, {f}));'
    body += 'printf("normals %u\\n", RT_TRI_NORMALS); printf("uvs %u\\n", RT_TRI_UVS); printf("abi %u\\n", RT_ABI_VERSION);'
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){' + body + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["attrs"] == C.sizeof(A.RtTriangleAttrs) == 68
    assert got["options"] == C.sizeof(A.RtUploadOptions) == 40 and got["RtUploadOptions.list_park_cost"] == 20
    assert got["info"] == C.sizeof(A.RtCompileInfo)
    for name, off in got.items():
        if "." in name:
            T, f = name.split(".")
            assert getattr(getattr(A, T), f).offset == off, name
    assert (got["normals"], got["uvs"], got["abi"]) == (A.RT_TRI_NORMALS, A.RT_TRI_UVS, 3) == (1, 2, 3)
    assert A.RT_FEATURE_TRI_ATTR == 128


def info_ex(pkg, desc, opt):
    A, lib = pkg._abi, pkg.lib()
    info = A.RtCompileInfo()
    rc = lib.rt_scene_compile_info_ex(C.byref(desc), C.byref(opt), C.byref(info))
    return rc, info, lib.rt_last_error(None)


def two_triangles(pkg):
    b = pkg.SceneBuilder()
    m = b.lambertian((0.5, 0.5, 0.5))
    t0 = b.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), m, normals=((0, 0, 1), (0, 0.5, 1), (0.5, 0, 1)), uvs=((0, 0), (1, 0), (0, 1)))
    t1 = b.triangle((2, 0, 0), (3, 0, 0), (2, 1, 0), m)
    s = b.sphere((0, 0, 3), 0.5, m)
    return b, b.desc(b.hittable_list([t0, t1, s])), (t0, t1, s)


def test_a_24_byte_options_struct_still_works(pkg):
    """A caller compiled against the options as they were: struct_bytes 24, and whatever lies behind is not read."""
    A = pkg._abi
    b, desc, _ = two_triangles(pkg)
    opt = pkg.upload_options(triangle_attrs=b.triangle_attrs())
    assert opt.n_triangle_attrs == 1
    rc, info, _ = info_ex(pkg, desc, opt)
    assert rc == A.RT_OK and info.n_tri_attrs == 1 and info.features & A.RT_FEATURE_TRI_ATTR
    opt.struct_bytes = 24
    opt.triangle_attrs = C.cast(C.c_void_p(8), C.POINTER(A.RtTriangleAttrs))      # never dereferenced
    rc, info, _ = info_ex(pkg, desc, opt)
    assert rc == A.RT_OK and info.n_tri_attrs == 0 and not info.features & A.RT_FEATURE_TRI_ATTR and info.n_tris == 2
    opt.struct_bytes = 32                                                         # the pointer without its count: not covered either
    rc, info, _ = info_ex(pkg, desc, opt)
    assert rc == A.RT_OK and info.n_tri_attrs == 0


def test_every_refusal(pkg):
    A, lib = pkg._abi, pkg.lib()
    b, desc, (t0, t1, s) = two_triangles(pkg)
    nan, inf = float("nan"), float("inf")

    def rec(h, flags, n=((0, 0, 1),) * 3, uv=((0, 0), (1, 0), (0, 1))):
        a = A.RtTriangleAttrs(h, flags)
        for v in range(3):
            for c in range(3):
                a.n[v][c] = n[v][c]
            for c in range(2):
                a.uv[v][c] = uv[v][c]
        return a
    both = A.RT_TRI_NORMALS | A.RT_TRI_UVS
    cases = [([rec(99, both)], b"out of range"), ([rec(-1, both)], b"out of range"), ([rec(s, both)], b"not an RT_HIT_TRIANGLE"),
             ([rec(t0, both), rec(t1, 0), rec(t0, 0)], b"twice"), ([rec(t0, 4)], b"unknown bit"),
             ([rec(t0, A.RT_TRI_NORMALS, n=((0, 0, 1), (nan, 0, 1), (0, 0, 1)))], b"not finite"), ([rec(t0, A.RT_TRI_NORMALS, n=((0, 0, 1), (0, 0, 1), (inf, 0, 0)))], b"not finite"),
             ([rec(t0, A.RT_TRI_UVS, uv=((0, 0), (1, nan), (0, 1)))], b"not finite"), ([rec(t0, A.RT_TRI_NORMALS, n=((0, 0, 1), (0, 0, 0), (0, 0, 1)))], b"zero length")]
    for recs, word in cases:
        rc, _, err = info_ex(pkg, desc, pkg.upload_options(triangle_attrs=recs))
        assert rc == A.RT_ERR_INVALID and word in err, (word, rc, err)
        assert lib.rt_scene_compile_dump_ex(C.byref(desc), C.byref(pkg.upload_options(triangle_attrs=recs)), None, 0, None, None, 0) == A.RT_ERR_INVALID
    opt = pkg.upload_options()
    opt.n_triangle_attrs = 3
    rc, _, err = info_ex(pkg, desc, opt)
    assert rc == A.RT_ERR_INVALID and b"NULL" in err
    # what a clear flag does not read may hold anything; flags 0 is legal and changes nothing
    ok = [rec(t0, A.RT_TRI_UVS, n=((nan, 0, 0), (0, 0, 0), (inf, 0, 0))), rec(t1, 0, n=((nan,) * 3,) * 3, uv=((nan, nan),) * 3)]
    rc, info, _ = info_ex(pkg, desc, pkg.upload_options(triangle_attrs=ok))
    assert rc == A.RT_OK and info.n_tri_attrs == 1 and info.features & A.RT_FEATURE_TRI_ATTR
    rc, info, _ = info_ex(pkg, desc, pkg.upload_options(triangle_attrs=[rec(t0, 0), rec(t1, 0)]))
    assert rc == A.RT_OK and info.n_tri_attrs == 0 and not info.features & A.RT_FEATURE_TRI_ATTR
    assert pkg.compile_info(desc)["features"] == info.features and pkg.compile_info(desc, triangle_attrs=ok)["n_tri_attrs"] == 1


def test_instanced_copies_count(pkg):
    """A triangle the graph reaches three times is three device records, and each carries the attributes."""
    A = pkg._abi
    b = pkg.SceneBuilder()
    m = b.lambertian((0.5, 0.5, 0.5))
    t = b.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), m, normals=((0, 0, 1),) * 3)
    plain = b.triangle((0, 0, 5), (1, 0, 5), (0, 1, 5), m)
    world = b.hittable_list([t, b.translate(t, (3, 0, 0)), b.rotate_y(b.translate(t, (0, 3, 0)), 20.0), plain])
    info = pkg.compile_info(b.desc(world), triangle_attrs=b.triangle_attrs())
    assert info["n_tris"] == 4 and info["n_tri_attrs"] == 3 and info["features"] & A.RT_FEATURE_TRI_ATTR
    for flags in (0, A.RT_LAYOUT_REFERENCE_COUNTERS, A.RT_LAYOUT_SCENE_IN_HBM):
        assert pkg.compile_info(b.desc(world), flags, leaf_collapse=4, triangle_attrs=b.triangle_attrs())["n_tri_attrs"] == 3


def test_attributes_of_unreached_triangles_attach_to_nothing(pkg):
    """features carries 128 exactly when a DEVICE triangle carries attributes: a record for a triangle the world does not reach is checked
    like any other and then changes nothing."""
    A = pkg._abi
    b = pkg.SceneBuilder()
    m = b.lambertian((0.5, 0.5, 0.5))
    seen = b.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), m)
    b.triangle((0, 0, 2), (1, 0, 2), (0, 1, 2), m, normals=((0, 0, 1),) * 3, uvs=((0, 0), (1, 0), (0, 1)))      # not in the world
    desc = b.desc(b.hittable_list([seen]))
    info = pkg.compile_info(desc, triangle_attrs=b.triangle_attrs())
    assert info["n_tris"] == 1 and info["n_tri_attrs"] == 0 and info["features"] == pkg.compile_info(desc)["features"] == 4
    b.tri_attrs[0].n[1][2] = 0.0
    with pytest.raises(pkg.RtError, match="zero length"):
        pkg.compile_info(desc, triangle_attrs=b.triangle_attrs())


def test_the_scene_fingerprint_covers_the_attributes(pkg):
    """A checkpoint is tied to the scene by scene_fingerprint: the same graph with other normals or uvs is another scene; records that change
    nothing (flags 0), their order, and what a clear flag does not read leave the print alone; no attributes: the print of the graph."""
    A = pkg._abi
    b, desc, (t0, t1, s) = two_triangles(pkg)
    plain = pkg.scene_fingerprint(desc)
    at = b.triangle_attrs()
    fp = pkg.scene_fingerprint(desc, at)
    assert fp != plain and fp == pkg.scene_fingerprint(desc, b.triangle_attrs()) and pkg.scene_fingerprint(desc, None) == plain
    zero = A.RtTriangleAttrs(t1, 0)
    zero.n[0][0] = 7.0
    assert pkg.scene_fingerprint(desc, [zero, at[0]]) == fp and pkg.scene_fingerprint(desc, [zero]) == plain
    at[0].uv[2][1] = 0.75
    assert pkg.scene_fingerprint(desc, at) != fp
    at[0].uv[2][1] = 1.0
    at[0].n[1][0] = 0.25
    assert pkg.scene_fingerprint(desc, at) != fp
    at[0].flags = A.RT_TRI_UVS                                                    # the normals are no longer read
    a = pkg.scene_fingerprint(desc, at)
    at[0].n[1][0] = 0.5
    assert pkg.scene_fingerprint(desc, at) == a != fp


# ---- interpolate_reference at f64: answers known by hand --------------------------------------------------------------------------------
def attrs_of(pkg, hid, normals=None, uvs=None):
    b = pkg.SceneBuilder()
    b.hittables = [None] * hid
    b.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), 0, normals=normals, uvs=uvs)
    return b.tri_attrs


def test_interpolation_known_answers(pkg):
    A = pkg._abi
    rng = np.random.default_rng(3)
    P = np.array([(0.0, 0, 0), (2, 0, 0.5), (0, 1.5, -0.5)])
    bu = rng.uniform(0, 1, 200); bv = rng.uniform(0, 1, 200) * (1 - bu)
    d = rng.normal(size=(200, 3))
    hid = np.full(200, 7)
    # one normal m at all three vertices: +-unit(m) anywhere, against the ray
    m = np.array([0.3, -0.4, 1.2])
    n, ff, u, v = pkg.interpolate_reference({7: P}, attrs_of(pkg, 7, normals=(m, 2 * m, 0.1 * m)), hid, bu, bv, d)
    um = m.astype(np.float32).astype(np.float64); um /= np.linalg.norm(um)
    assert (ff == (d @ um < 0)).all() and np.abs(n - np.where(ff[:, None], um, -um)).max() < 1e-7 and (np.einsum("ij,ij->i", n, d) <= 0).all()
    assert (u == bu).all() and (v == bv).all()                              # no RT_TRI_UVS: the barycentrics
    # identity uv: (bu, bv) as numbers, at f64 and at f32
    for T in (np.float64, np.float32):
        n2, _, u, v = pkg.interpolate_reference({7: P}, attrs_of(pkg, 7, uvs=((0, 0), (1, 0), (0, 1))), hid, bu, bv, d, T)
        assert (u == bu.astype(T)).all() and (v == bv.astype(T)).all() and u.dtype == T
        g = np.cross(P[1] - P[0], P[2] - P[0]); g /= np.linalg.norm(g)
        assert np.abs(np.abs(n2 @ g) - 1.0).max() < 1e-6                    # no RT_TRI_NORMALS: the geometric normal
    # general uv: the convex combination
    uv = np.array(M.BIG_UV)
    _, _, u, v = pkg.interpolate_reference({7: P}, attrs_of(pkg, 7, uvs=uv), hid, bu, bv, d)
    f = uv.astype(np.float32).astype(np.float64)
    assert np.abs(u - ((1 - bu - bv) * f[0, 0] + bu * f[1, 0] + bv * f[2, 0])).max() < 1e-15 and np.abs(v - ((1 - bu - bv) * f[0, 1] + bu * f[1, 1] + bv * f[2, 1])).max() < 1e-15
    # vertex order: swapping n1 and n2 changes the answer
    ns = np.array(M.BIG_NORMALS)
    a, _, _, _ = pkg.interpolate_reference({7: P}, attrs_of(pkg, 7, normals=ns), hid, bu, bv, d)
    s, _, _, _ = pkg.interpolate_reference({7: P}, attrs_of(pkg, 7, normals=ns[[0, 2, 1]]), hid, bu, bv, d)
    assert np.linalg.norm(a - s, axis=1).max() > 0.5
    at1, _, _, _ = pkg.interpolate_reference({7: P}, attrs_of(pkg, 7, normals=ns), [7], [1.0], [0.0], [(0, 0, -1.0)])
    assert np.abs(at1[0] - ns[1] / np.linalg.norm(ns[1])).max() < 1e-7      # bu = 1 is v1
    # normals that cancel: the geometric normal
    c, _, _, _ = pkg.interpolate_reference({7: P}, attrs_of(pkg, 7, normals=((0, 0, 1), (0, 0, -1), (0, 0, 1))), [7], [0.5], [0.0], [(0, 0, -1.0)])
    assert np.abs(np.abs(c[0] @ g) - 1.0) < 1e-12
    assert A.RT_TRI_NORMALS == 1


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_icosphere_normals_interpolate_to_the_radial_direction(pkg, sub):
    """On an icosphere about c with n_i = unit(v_i - c) the interpolated normal is unit(p - c) at the hit point p = sum w_i v_i, to 1e-12 —
    with vertex normals exact in f64 (the f32 rounding of the upload is the ABI's, tests/test_gpu_mesh_attrs.py bounds it)."""
    tris, nrm = pkg.icosphere(sub)
    assert tris.shape == (20 * 4 ** sub, 3, 3) and np.abs(np.linalg.norm(nrm, axis=2) - 1.0).max() < 1e-15
    out = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    assert (np.einsum("ij,ij->i", out, tris.mean(axis=1)) > 0).all()           # counter-clockwise from outside
    edges = {}
    for t in tris:
        for a, b in ((0, 1), (1, 2), (2, 0)):
            key = tuple(sorted([tuple(np.round(t[a], 12)), tuple(np.round(t[b], 12))]))
            edges[key] = edges.get(key, 0) + 1
    assert set(edges.values()) == {2}                                         # closed
    rng = np.random.default_rng(sub)
    k = rng.integers(0, len(tris), 300)
    bu = rng.uniform(0, 1, 300); bv = rng.uniform(0, 1, 300) * (1 - bu)
    p = (1 - bu - bv)[:, None] * tris[k, 0] + bu[:, None] * tris[k, 1] + bv[:, None] * tris[k, 2]

    class Exact:                                                              # an attribute record with f64 normals
        def __init__(self, h, n):
            self.hittable, self.flags, self.n = h, 1, n
    attrs = [Exact(i, nrm[i]) for i in range(len(tris))]
    n, ff, _, _ = pkg.interpolate_reference(tris, attrs, k, bu, bv, -p)
    assert ff.all() and np.abs(n - p / np.linalg.norm(p, axis=1, keepdims=True)).max() < 1e-12


# ---- parse_obj_attrs and JSON -------------------------------------------------------------------------------------------------------------
OBJ = """# a quad, a fan of five, and faces in every form
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0.5 1.5 0
vn 0 0 1
vn 0 1 1
vn 1 0 1
vt 0 0
vt 1 0
vt 1 1
vt 0 1
f 1/1/1 2/2/2 3/3/3
f 1//1 3//3 4//2
f 1/1 2/2 3/3 4/4
f 1 2 3
f -5/-4/-3 -4/-3/-2 -3/-2/-1 -2/-1/-3 -1/-4/-2
f 1/1/1 2/2 3/3/3
"""


def test_parse_obj_attrs(pkg, tmp_path):
    path = tmp_path / "m.obj"
    path.write_text(OBJ)
    tris, vn, vt, has_vn, has_vt = pkg.parse_obj_attrs(str(path))
    assert (tris == pkg.parse_obj(str(path))).all() and len(tris) == 1 + 1 + 2 + 1 + 3 + 1
    assert has_vn.tolist() == [True, True, False, False, False, True, True, True, False] and has_vt.tolist() == [True, False, True, True, False, True, True, True, True]
    N, T = np.array([(0, 0, 1), (0, 1, 1), (1, 0, 1)], float), np.array([(0, 0), (1, 0), (1, 1), (0, 1)], float)
    assert (vn[0] == N[[0, 1, 2]]).all() and (vt[0] == T[[0, 1, 2]]).all()
    assert (vn[1] == N[[0, 2, 1]]).all() and not vt[1].any()                  # v//vn
    assert (vt[2] == T[[0, 1, 2]]).all() and (vt[3] == T[[0, 2, 3]]).all() and not vn[2].any()      # v/vt, a fan of the quad
    assert not vn[4].any() and not vt[4].any()
    # negative indices count back from the end of each table; the fan keeps its first corner
    assert (tris[5] == [[0, 0, 0], [1, 0, 0], [1, 1, 0]]).all() and (vn[5] == N[[0, 1, 2]]).all() and (vt[5] == T[[0, 1, 2]]).all()
    assert (tris[7] == [[0, 0, 0], [0, 1, 0], [0.5, 1.5, 0]]).all() and (vn[7] == N[[0, 0, 1]]).all() and (vt[7] == T[[0, 3, 0]]).all()
    assert not has_vn[8] and has_vt[8]                                         # one corner without vn: the face has none
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//2 3//1\n")
    with pytest.raises(ValueError, match="vn index"):
        pkg.parse_obj_attrs(str(bad))


def test_json_attributes(pkg, tmp_path):
    A = pkg._abi
    (tmp_path / "m.obj").write_text(OBJ)
    doc = {"camera": {"lookfrom": [0, 0, 5], "lookat": [0, 0, 0]},
           "materials": {"grey": {"lambertian": [0.5, 0.5, 0.5]}},
           "objects": {"tri": {"triangle": [[0, 0, 0], [1, 0, 0], [0, 1, 0]], "normals": [[0, 0, 1], [0, 1, 1], [1, 0, 1]], "uvs": [[0, 0], [0.5, 0], [0, 0.5]], "material": "grey"},
                       "flat": {"triangle": [[0, 0, 1], [1, 0, 1], [0, 1, 1]], "material": "grey"},
                       "mesh": {"obj": "m.obj", "material": "grey", "smooth": True, "textured": True, "offset": [3, 0, 0]}},
           "world": {"list": ["tri", "flat", "mesh"]}}
    js = pkg.JsonScene(doc, str(tmp_path))
    at = js.triangle_attrs
    assert len(at) == 1 + 8 and at[0].flags == 3 and [at[0].uv[1][0], at[0].uv[2][1]] == [0.5, 0.5] and list(at[0].n[1]) == [0.0, 1.0, 1.0]
    assert sorted(a.flags for a in at[1:]) == sorted([3, 1, 2, 2, 3, 3, 3, 2])
    info = pkg.compile_info(js.desc, triangle_attrs=at)
    assert info["n_tris"] == 11 and info["n_tri_attrs"] == 9 and info["features"] & A.RT_FEATURE_TRI_ATTR
    doc["objects"]["mesh"].update(smooth=False, textured=False)
    assert len(pkg.JsonScene(doc, str(tmp_path)).triangle_attrs) == 1
    del doc["objects"]["tri"]["normals"], doc["objects"]["tri"]["uvs"]
    doc["world"] = {"list": ["tri", "flat"]}
    assert pkg.JsonScene(doc, str(tmp_path)).triangle_attrs is None
    (tmp_path / "plain.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    doc["objects"]["mesh"] = {"obj": "plain.obj", "material": "grey", "smooth": True}
    doc["world"] = {"list": ["mesh"]}
    with pytest.raises(ValueError, match="smooth"):
        pkg.JsonScene(doc, str(tmp_path))
    doc["objects"]["mesh"] = {"obj": "m.obj", "material": "grey", "smooth": True, "scale": -1.0}
    with pytest.raises(ValueError, match="negative scale"):
        pkg.JsonScene(doc, str(tmp_path))
    doc["objects"]["mesh"].update(smooth=False, textured=True)
    assert len(pkg.JsonScene(doc, str(tmp_path)).triangle_attrs) == 7             # mirrored and textured: the uv do not care
    doc["objects"]["tri"]["uvs"] = [[0, 0], [1, 0]]
    doc["world"] = {"list": ["tri"]}
    with pytest.raises(ValueError, match="uvs"):
        pkg.JsonScene(doc, str(tmp_path))


# ---- the ray sets and the bound for the GPU ray test ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.SCENES)
def test_ray_sets_and_f32_figures(pkg, orc, name):
    """The set is what tests/test_gpu_mesh_attrs.py needs — about 4096 rays, front and back faces, at most 5 % left out as undecidable or
    edge rays — and mesh_attrs.MEASURED_F32[name], which bounds the device (x 2), is what the f32 restatement measures against the f64
    one here, within 1 % (libm builds differ in the last place)."""
    s = M.ray_set(pkg, orc, name)
    n = len(s["rays"])
    hit = s["ref"]["hit"]
    left_out = int((~s["decidable"] | s["edge"]).sum())
    use = s["decidable"] & (s["tri"] >= 0)
    print(f"{name}: {n} rays, {int(hit.sum())} hits, {int((s['tri'] >= 0).sum())} on attribute triangles, {int(s['edge'].sum())} edge, {int((~s['decidable']).sum())} undecidable, "
          f"{int(use.sum())} compared, front faces {int(s['ff'][use].sum())}")
    assert n == 4096 and left_out <= 0.05 * n
    # (under Translate / RotateY the last set_face_normal sees a normal that already opposes the ray: front_face is true but for the rays
    # RotateY's mixed spaces flip — the reference's semantics, which the wrapped set is there to hold)
    assert use.sum() >= 800 and s["ff"][use].sum() >= 200 and (~s["ff"][use]).sum() >= (10 if name == "wrapped" else 200)
    assert (np.einsum("ij,ij->i", s["n"][use], s["rays"]["d"][use].astype(np.float64)) <= 0).all()          # the normal opposes the ray
    if name != "big":         # the interpolated normal is not the facet's: it is (nearly) the sphere's
        flat = s["ref"]["n"][use]
        assert np.linalg.norm(s["n"][use] - flat, axis=1).max() > 0.05
    worst, at, ff_differs, compared = M.f32_figures(pkg, orc, name)
    print(f"{name}: f32 restatement against f64 on {compared} rays: |dn| {worst['n']:.3e} (ray {at['n']})  |d(u,v)| {worst['uv']:.3e} (ray {at['uv']}); front_face differs on {ff_differs}")
    assert ff_differs == 0 and compared >= 0.95 * use.sum()
    for q, v in M.MEASURED_F32[name].items():
        assert abs(worst[q] - v) <= 0.01 * v, (q, worst[q], v)


def test_wrapped_set_replays_the_wrappers(pkg, orc):
    """The wrapper replay of mesh_attrs (Translate, RotateY, FlipFace) is the checker's own: with the GEOMETRIC normal put through it, it
    returns the checker's (normal, front_face) on every hit of the wrapped mesh."""
    s = M.ray_set(pkg, orc, "wrapped")
    k = np.flatnonzero(s["tri"] >= 0)
    mesh, ref = s["mesh"], s["ref"]
    chain = s["chains"][int(s["tri"][k[0]])]
    assert [c[0] for c in chain] == [pkg._abi.RT_HIT_TRANSLATE, pkg._abi.RT_HIT_ROTATE_Y, pkg._abi.RT_HIT_FLIP_FACE]
    dk = M.local_directions(pkg, chain, s["rays"]["d"][k], np.float64)
    P = np.array([mesh.tris[int(h)] for h in s["tri"][k]])
    g = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]); g /= np.linalg.norm(g, axis=1, keepdims=True)
    front = np.einsum("ij,ij->i", dk[-1], g) < 0
    n, ff = M.replay(pkg, chain, dk, np.where(front[:, None], g, -g), front, np.float64)
    assert (ff == ref["ff"][k]).all() and np.abs(n - ref["n"][k]).max() < 1e-12
    assert math.isclose(M.WRAP["degrees"], 30.0)
