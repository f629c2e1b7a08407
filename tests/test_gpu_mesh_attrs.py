"""Triangle attributes on the GPU (include/rt_hip.h "triangle attributes"): ray by ray against the f64 answer of tests/mesh_attrs.py, the
same answer from every device layout, exact plumbing (identity uv and flags-0 records change nothing, in any kernel form), a textured
vertex-normal mesh held to the f64 oracle's render of the rects it tiles, a smooth sphere mesh against the oracle's true Sphere — both in
every kernel form, k_shade among them — and the feature planes of both against ray queries and against the rects' own planes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_attrs as M  # noqa: E402
import rays as R  # noqa: E402

pytestmark = pytest.mark.gpu


def trace(pkg, gpu, scene, rays):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()
    return gpu.trace_rays(scene, t).cpu().numpy().reshape(-1).view(pkg.RAYHIT_DTYPE)


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- 1. ray by ray -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.SCENES)
def test_rays_agree_with_the_f64_answer(pkg, orc, gpu, name):
    """On the decidable non-edge rays that hit a triangle with attributes: front_face is the f64 answer's, n and (u, v) lie within 2 x the
    f32 restatement's own error (mesh_attrs.MEASURED_F32, measured on a CPU). On EVERY ray t, p, hittable, material and hit / miss are
    the bytes of the same upload without attributes, and a hit on anything else is that upload's whole record."""
    from conftest import record_metric
    A = pkg._abi
    s = M.ray_set(pkg, orc, name)
    mesh, rays = s["mesh"], s["rays"]
    feat = pkg.compile_info(mesh.built.desc, triangle_attrs=mesh.attrs)["features"]
    assert feat & A.RT_FEATURE_TRI_ATTR and (name != "wrapped" or feat & 16), feat          # (16: instance transforms, the all-features instance)
    plain, smooth = gpu.upload(mesh.built.desc), gpu.upload(mesh.built.desc, triangle_attrs=mesh.attrs)
    h0, h1 = trace(pkg, gpu, plain, rays), trace(pkg, gpu, smooth, rays)
    plain.close(); smooth.close()
    for f in ("t", "p", "hittable", "material"):
        assert same_bytes(h0[f], h1[f]), f
    assert (((h0["flags"] ^ h1["flags"]) & A.RT_RAYHIT_HIT) == 0).all() and ((h1["flags"] & ~np.uint32(3)) == 0).all()
    other = ~np.isin(h1["hittable"], list(mesh.tris))
    assert same_bytes(h0[other], h1[other])
    g_hit, g_ff = (h1["flags"] & A.RT_RAYHIT_HIT) != 0, (h1["flags"] & A.RT_RAYHIT_FRONT_FACE) != 0
    use = s["decidable"] & ~s["edge"] & (s["tri"] >= 0)
    assert g_hit[use].all(), f"decidable rays {np.flatnonzero(use & ~g_hit)[:8]} miss"
    k = np.flatnonzero(use)
    dn = np.linalg.norm(h1["n"][k].astype(np.float64) - s["n"][k], axis=1)
    duv = np.maximum(np.abs(h1["u"][k].astype(np.float64) - s["u"][k]), np.abs(h1["v"][k].astype(np.float64) - s["v"][k]))
    moved = float(np.linalg.norm(h1["n"][k].astype(np.float64) - h0["n"][k], axis=1).max())
    bound = M.bound_of(name)
    print(f"{name}: {len(rays)} rays, {len(k)} compared; worst |dn| {dn.max():.3e} (ray {k[dn.argmax()]}, allowed {bound['n']:.3e})  |d(u,v)| {duv.max():.3e} "
          f"(ray {k[duv.argmax()]}, allowed {bound['uv']:.3e}); front_face differs on {int((g_ff[k] != s['ff'][k]).sum())}; the normal moves by up to {moved:.3f} against the flat upload")
    record_metric(config="mesh_attrs", scene=name, dn=float(dn.max()), duv=float(duv.max()))
    assert (g_ff[k] == s["ff"][k]).all(), f"front_face differs on decidable rays {k[g_ff[k] != s['ff'][k]][:8]}"
    assert (np.einsum("ij,ij->i", h1["n"][k].astype(np.float64), rays["d"][k].astype(np.float64)) <= 0).all()
    assert dn.max() <= bound["n"], (dn.max(), bound["n"], int(k[dn.argmax()]))
    assert duv.max() <= bound["uv"], (duv.max(), bound["uv"], int(k[duv.argmax()]))
    assert moved > 0.05                                                         # and the attributes are used at all


def test_a_24_byte_options_struct_still_uploads(pkg, orc, gpu):
    """A caller compiled against RtUploadOptions as it was (struct_bytes 24): the upload succeeds, what lies behind the 24 bytes is not
    read, and the scene is the one without attributes."""
    import ctypes as C
    A = pkg._abi
    s = M.ray_set(pkg, orc, "big")
    desc = s["mesh"].built.desc
    old = pkg.upload_options(A.RT_LAYOUT_SCENE_IN_HBM, triangle_attrs=s["mesh"].attrs)
    old.struct_bytes = 24
    old.triangle_attrs = C.cast(C.c_void_p(8), C.POINTER(A.RtTriangleAttrs))      # never dereferenced
    a, b = pkg.Scene(gpu, desc, old), gpu.upload(desc, A.RT_LAYOUT_SCENE_IN_HBM)
    assert same_bytes(trace(pkg, gpu, a, s["rays"]), trace(pkg, gpu, b, s["rays"]))
    a.close(); b.close()


# ---- 2. every layout maps index -> attributes the same way -------------------------------------------------------------------------------
def test_every_layout_gives_the_same_records(pkg, orc, gpu):
    A = pkg._abi
    s = M.ray_set(pkg, orc, "ico2")
    mesh, rays = s["mesh"], s["rays"]
    desc = mesh.built.desc
    cases = [("default", 0, {}, A.RT_BVH_REFERENCE), ("reference_counters", A.RT_LAYOUT_REFERENCE_COUNTERS, {}, A.RT_BVH_REFERENCE),
             ("hbm", A.RT_LAYOUT_SCENE_IN_HBM, {}, A.RT_BVH_REFERENCE), ("hbm_32b", A.RT_LAYOUT_SCENE_IN_HBM | A.RT_LAYOUT_NODES_32B, {}, A.RT_BVH_REFERENCE),
             ("wide", A.RT_LAYOUT_WIDE_NODES, {}, A.RT_BVH_REFERENCE), ("hbm_wide", A.RT_LAYOUT_SCENE_IN_HBM | A.RT_LAYOUT_WIDE_NODES, {}, A.RT_BVH_REFERENCE),
             ("collapse_4", 0, dict(leaf_collapse=4), A.RT_BVH_REFERENCE), ("sah", 0, {}, A.RT_BVH_SAH)]
    keep = ~s["edge"]
    first = None
    for label, flags, more, builder in cases:
        desc.bvh_builder = builder
        try:
            info = pkg.compile_info(desc, flags, triangle_attrs=mesh.attrs, **more)
            scene = gpu.upload(desc, flags, triangle_attrs=mesh.attrs, **more)
        finally:
            desc.bvh_builder = A.RT_BVH_REFERENCE
        h = trace(pkg, gpu, scene, rays)
        scene.close()
        assert info["n_tri_attrs"] == info["n_tris"] == 320, (label, info)
        print(f"{label}: {info['n_nodes']} records, {int(((h['flags'] & 1) != 0).sum())} hits")
        if first is None:
            first = h
            continue
        diff = np.flatnonzero(keep & (h.view(np.uint8).reshape(len(h), -1) != first.view(np.uint8).reshape(len(h), -1)).any(axis=1))
        assert len(diff) == 0, f"{label}: records differ from the default layout's on rays {diff[:8]}"
    k = np.flatnonzero(s["decidable"] & keep & (s["tri"] >= 0))
    assert np.linalg.norm(first["n"][k].astype(np.float64) - s["n"][k], axis=1).max() <= M.bound_of("ico2")["n"]


# ---- 3. plumbing is exact ------------------------------------------------------------------------------------------------------------------
def forms(pkg, gpu, scene, cam, W, H, SPP, **kw):
    """The frame from every kernel form, with what ran: the default render (the wavefront loop, k_extend + k_shade, until at most 2^18 paths
    are alive, then ONE launch of the drain form of k_extend — a frame of fewer paths than that never launches k_shade), RT_FLAG_FUSED (the
    drain form alone) and tail_paths = 1 (k_shade to the end, no drain). Returns {form: (frame, stats)}."""
    A = pkg._abi
    out = {"default": gpu.render(scene, cam, pkg.make_params(W, H, SPP, **kw)),
           "fused": gpu.render(scene, cam, pkg.make_params(W, H, SPP, flags=A.RT_FLAG_FUSED, **kw)),
           "tail_1": gpu.render(scene, cam, pkg.make_params(W, H, SPP, tail_paths=1, **kw))}
    assert out["fused"][1]["shade_launches"] == 0 and out["fused"][1]["drain_paths"] > 0
    assert out["tail_1"][1]["shade_launches"] > 0 and out["tail_1"][1]["drain_paths"] == 0
    return out


def test_identity_uv_and_flags_0_change_nothing(pkg, gpu, earth):
    """Identity uv on every triangle (the attribute instances, the interpolation returning the barycentrics) and flags-0 records (no
    attributes at all) against the upload without: the frame in every kernel form, the four feature planes, the ray hits. The frame is
    192 x 128 x 16 = 393 216 paths, more than the 2^18 at which a render hands over to the drain kernel: the default render runs the wavefront
    loop AND the drain; the two accumulated passes, of half as many paths each, are drain launches."""
    import torch
    A = pkg._abi
    W, H, SPP = 192, 128, 16
    out = {}
    for mode in (None, "identity", "flags0"):
        desc, cam, attrs, keep = M.textured_scene(pkg, earth, mode)
        info = pkg.compile_info(desc, triangle_attrs=attrs)
        assert bool(info["features"] & A.RT_FEATURE_TRI_ATTR) == (mode == "identity") and info["features"] & 32 and info["n_tri_attrs"] == (24 if mode == "identity" else 0)
        scene = gpu.upload(desc, triangle_attrs=attrs)
        f = forms(pkg, gpu, scene, cam, W, H, SPP)
        assert f["default"][1]["shade_launches"] > 0 and f["default"][1]["drain_paths"] > 0, f["default"][1]
        r = {name: img for name, (img, _) in f.items()}
        half = pkg.make_params(W, H, SPP // 2)
        acc, _, _ = gpu.render_pass(scene, cam, half, 0, SPP, False)
        acc, _, _ = gpu.render_pass(scene, cam, half, SPP // 2, SPP, True, rgb_sum=np.ascontiguousarray(acc).reshape(-1))
        r["two_passes"] = acc
        planes = gpu.render_features(scene, cam, pkg.make_params(W, H, SPP))
        torch.cuda.synchronize()
        for name, t in zip(("albedo", "normal", "depth", "hits"), planes):
            r[name] = t.cpu().numpy()
        r["rays"] = trace(pkg, gpu, scene, R.camera_rays(cam, W, H, np.random.default_rng(2)))
        scene.close()
        out[mode] = r
    base = out[None]
    assert np.isfinite(base["default"]).all() and base["default"].max() > 0 and (base["hits"] > 0).sum() > 100
    lit = (base["rays"]["flags"] & 1) != 0
    assert lit.sum() > 100 and (base["rays"]["u"][lit] > 0).any()
    for name in ("fused", "tail_1", "two_passes"):
        assert same_bytes(base[name], base["default"]), name
    for mode in ("identity", "flags0"):
        for name in ("default", "fused", "tail_1", "two_passes", "albedo", "normal", "depth", "hits"):
            assert same_bytes(out[mode][name], base[name]), (mode, name)
        for f in ("t", "hittable", "material", "flags", "p", "n"):
            assert same_bytes(out[mode]["rays"][f], base["rays"][f]), (mode, f)
        assert np.array_equal(out[mode]["rays"]["u"], base["rays"]["u"]) and np.array_equal(out[mode]["rays"]["v"], base["rays"]["v"]), mode


# ---- 4. held to the f64 oracle -------------------------------------------------------------------------------------------------------------
def test_textured_vertex_normal_mesh_against_the_oracles_rects(pkg, orc, gpu, earth):
    """Two triangles that tile an XyRect, with the rect's corner (u, v) and normal at their vertices, are the rect: the oracle's f64 render of
    the rect scene judges the device's render of the mesh, with tests/test_gpu_scenes.py check()'s default tolerances — in every kernel form
    (a 64 x 48 x 16 frame is below the hand-over, so its default render is the drain kernel: tail_paths = 1 is what runs k_shade, here the
    all-features attribute instance), and the forms give one frame. The light's triangles are wound the other way, so a frame lit at all
    is lit through the vertex normals."""
    from conftest import record_metric
    W, H, SPP = 64, 48, 16
    flags = pkg._abi.RT_FLAG_COUNTERS
    prm = pkg.make_params(W, H, SPP, flags=flags)
    rdesc, cam, none, keep_r = M.rect_pair_scene(pkg, earth, False)
    mdesc, _, attrs, keep_m = M.rect_pair_scene(pkg, earth, True)
    assert none is None and len(attrs) == 4
    ref, ost = orc.render(rdesc, cam, prm, precision=64, n_threads=8, count=True)

    def figures(img, st):
        d = np.abs(img.astype(np.float64) - ref) / SPP
        return float(d.mean()), float((d.max(axis=2) > 2e-3).mean()), abs(st["segments"] - ost["segments"]) / ost["segments"]
    scene = gpu.upload(mdesc, triangle_attrs=attrs)
    f = {"default": gpu.render(scene, cam, prm), "fused": gpu.render(scene, cam, pkg.make_params(W, H, SPP, flags=flags | pkg._abi.RT_FLAG_FUSED)),
         "tail_1": gpu.render(scene, cam, pkg.make_params(W, H, SPP, flags=flags, tail_paths=1))}
    assert f["tail_1"][1]["shade_launches"] > 0 and f["tail_1"][1]["drain_paths"] == 0 and f["fused"][1]["shade_launches"] == 0
    rect_img, rect_st = gpu.render(gpu.upload(rdesc), cam, prm)
    flat_img, _ = gpu.render(gpu.upload(mdesc), cam, pkg.make_params(W, H, SPP, flags=flags, tail_paths=1))
    r_mean, r_bad, r_seg = figures(rect_img, rect_st)
    assert np.isfinite(f["default"][0]).all() and ref.mean() / SPP > 0.05
    assert flat_img.mean() < 0.5 * ref.mean()                                   # without the vertex normals the light shows its back
    for form, (img, st) in f.items():
        mean, bad, seg = figures(img, st)
        print(f"mesh with attributes, {form}, against the oracle's rects: mean {mean:.3e}  bad {bad:.4f}  segments {seg:.2e};  the device's own rects: mean {r_mean:.3e}  bad {r_bad:.4f}  "
              f"segments {r_seg:.2e}; oracle mean level {ref.mean() / SPP:.4f}, the mesh without attributes {flat_img.mean() / SPP:.4f}")
        record_metric(config="mesh_attrs", scene="rect_pair", form=form, mean=mean, bad=bad, seg=seg, rect_mean=r_mean, rect_bad=r_bad)
        assert mean <= 1.2e-4 and bad <= 0.015, (form, mean, bad)
        assert abs(st["segments"] - ost["segments"]) <= max(8, 2e-3 * ost["segments"]), (form, st["segments"], ost["segments"])
        assert same_bytes(img, f["default"][0]), form


# ---- 5. it looks like a sphere -------------------------------------------------------------------------------------------------------------
def test_smooth_mesh_looks_like_the_sphere(pkg, orc, gpu):
    """The subdivision-2 icosphere as a mirror under the sky, against the oracle's render of the true Sphere: E_smooth <= E_flat / 4 (a numpy
    ray cast of this setup in f64 gives 5.7e-4 against 1.08e-2) — in every kernel form (tail_paths = 1 is what runs k_shade at this size,
    here the mesh attribute instance), and the forms give one frame."""
    from conftest import record_metric
    W = H = 64
    SPP = 8
    prm = pkg.make_params(W, H, SPP, max_depth=2)
    sdesc, cam, _, keep_s = M.sphere_scene(pkg, "sphere")
    ref, _ = orc.render(sdesc, cam, prm, precision=64, n_threads=8)
    fdesc, _, none, keep_f = M.sphere_scene(pkg, "flat")
    mdesc, _, attrs, keep_m = M.sphere_scene(pkg, "smooth")
    assert none is None and len(attrs) == 320
    flat = forms(pkg, gpu, gpu.upload(fdesc), cam, W, H, SPP, max_depth=2)
    smooth = forms(pkg, gpu, gpu.upload(mdesc, triangle_attrs=attrs), cam, W, H, SPP, max_depth=2)
    for form in smooth:
        e_flat = float(np.abs(flat[form][0].astype(np.float64) - ref).mean() / SPP)
        e_smooth = float(np.abs(smooth[form][0].astype(np.float64) - ref).mean() / SPP)
        print(f"{form}: mean |error| against the true sphere: flat {e_flat:.3e}, smooth {e_smooth:.3e}, ratio {e_smooth / e_flat:.3f}")
        record_metric(config="mesh_attrs", scene="sphere", form=form, e_flat=e_flat, e_smooth=e_smooth)
        assert np.isfinite(smooth[form][0]).all() and e_flat > 1e-3
        assert e_smooth <= e_flat / 4.0, (form, e_smooth, e_flat)
        assert same_bytes(smooth[form][0], smooth["default"][0]) and same_bytes(flat[form][0], flat["default"][0]), form


# ---- 6. the feature planes use the interpolated values --------------------------------------------------------------------------------------
def feature_planes(gpu, scene, cam, prm):
    import torch
    a, n, d, h = gpu.render_features(scene, cam, prm)
    torch.cuda.synchronize()
    return a.cpu().numpy().reshape(-1, 3), n.cpu().numpy().reshape(-1, 3), d.cpu().numpy(), h.cpu().numpy().view(np.uint32)


def test_feature_normals_are_the_interpolated_ones(pkg, orc, gpu):
    """The normal plane of a one-sample feature pass over the smooth subdivision-2 sphere mesh (k_features_export's mesh attribute instance)
    against the n rt_trace_rays reports for the same camera rays, made on the host (tests/features.py camera_rays).
    The bound, from reasoning alone: both are f32 evaluations of the interpolated normal, each within bound_of("ico2") of the f64 answer for
    ITS ray (test 1 holds the ray queries to that), and the two rays differ by the f32 roundings of the device's own camera ray: about
    four operations at magnitude <= 4, each <= half an ulp (2.4e-7), so |dd| <= 1e-6 on |d| = 4; the hit point 4 away moves by
    <= 4 x 2.5e-7 / cos(46 degrees) = 1.5e-6, and so does a unit sphere's normal."""
    import features as F
    A = pkg._abi
    W = H = 32
    SEED = 5
    desc, cam, attrs, keep = M.sphere_scene(pkg, "smooth")
    o, d, tm = F.camera_rays(orc, cam, W, H, SEED, 0)
    rays = R.make_rays(o, d, tm)
    ref = R.ask(orc, desc, rays)
    dec = ~R.undecidable(orc, desc, rays, ref)
    smooth, flat = gpu.upload(desc, triangle_attrs=attrs), gpu.upload(desc)
    assert pkg.compile_info(desc, triangle_attrs=attrs)["features"] == 4 | A.RT_FEATURE_TRI_ATTR
    yard, yard_flat = trace(pkg, gpu, smooth, rays), trace(pkg, gpu, flat, rays)
    albedo, normal, depth, hits = feature_planes(gpu, smooth, cam, pkg.make_params(W, H, 1, seed=SEED))
    _, normal_flat, _, _ = feature_planes(gpu, flat, cam, pkg.make_params(W, H, 1, seed=SEED))
    y_hit = (yard["flags"] & A.RT_RAYHIT_HIT) != 0
    assert not (dec & ((hits != 0) != y_hit)).any() and (dec & y_hit).sum() >= 0.9 * W * H
    k = np.flatnonzero(dec & y_hit)
    dn = np.linalg.norm(normal[k].astype(np.float64) - yard["n"][k], axis=1)
    bound = 2.0 * M.bound_of("ico2")["n"] + 1.5e-6
    moved = np.linalg.norm(normal[k].astype(np.float64) - normal_flat[k], axis=1)
    print(f"feature normals against the ray queries' on {len(k)} pixels: worst |dn| {dn.max():.3e} (allowed {bound:.3e}); against the flat mesh's plane they move by "
          f"{np.median(moved):.3f} (median), as the ray queries' do: {np.median(np.linalg.norm(yard['n'][k].astype(np.float64) - yard_flat['n'][k], axis=1)):.3f}")
    assert dn.max() <= bound, (dn.max(), bound, int(k[dn.argmax()]))
    assert np.median(moved) > 0.01                                              # a facet of this mesh is up to ~0.08 off the sphere's normal


def test_feature_albedo_goes_through_the_interpolated_uv(pkg, gpu, earth):
    """The feature planes of the rect-pair MESH (corner uv on its triangles: k_features_export's all-features attribute instance) against the
    planes of the RECT scene, which the same camera, seed and frame give the same rays bit for bit. Same hits; the normal within 1e-6 (the
    weights' sum and the reciprocal square root: a few f32 ulps of 1); depth within 1e-5 of itself (two f32 formulas for one t); albedo, the
    earth image through (u, v), within 1e-3 on all but 2 % of the hit pixels (the project's allowance for pixels on a texel boundary,
    tests/test_gpu_features.py) — while without attributes each triangle maps the whole image onto itself and most pixels differ."""
    A = pkg._abi
    W, H, SPP = 64, 48, 2
    prm = pkg.make_params(W, H, SPP, seed=3)
    rdesc, cam, _, keep_r = M.rect_pair_scene(pkg, earth, False)
    mdesc, _, attrs, keep_m = M.rect_pair_scene(pkg, earth, True)
    assert pkg.compile_info(mdesc, triangle_attrs=attrs)["features"] & (32 | A.RT_FEATURE_TRI_ATTR) == 32 | A.RT_FEATURE_TRI_ATTR
    ra, rn, rd_, rh = feature_planes(gpu, gpu.upload(rdesc), cam, prm)
    ma, mn, md, mh = feature_planes(gpu, gpu.upload(mdesc, triangle_attrs=attrs), cam, prm)
    fa, _, _, fh = feature_planes(gpu, gpu.upload(mdesc), cam, prm)
    assert (mh == rh).all() and (fh == rh).all() and (rh == SPP).sum() > 0.3 * W * H
    k = np.flatnonzero(rh == SPP)
    off = np.abs(ma[k].astype(np.float64) - ra[k]).max(axis=1) > 1e-3 * SPP
    off_flat = np.abs(fa[k].astype(np.float64) - ra[k]).max(axis=1) > 1e-3 * SPP
    dn = float(np.abs(mn[k].astype(np.float64) - rn[k]).max() / SPP)
    dd = float((np.abs(md[k].astype(np.float64) - rd_[k]) / rd_[k]).max())
    print(f"mesh planes against the rect scene's on {len(k)} pixels: albedo off on {int(off.sum())} ({int(off_flat.sum())} without attributes), worst |dn| {dn:.3e}, |d depth|/depth {dd:.3e}")
    assert off.sum() <= 0.02 * len(k) and off_flat.sum() >= 0.5 * len(k)
    assert dn <= 1e-6 and dd <= 1e-5
