"""Normal maps on the GPU (include/rt_hip.h "normal maps"): ray by ray against the f64 answer of tests/normal_maps.py, the same answer
from every device layout, one frame from every kernel form and from a radiance query, a mapped triangle against its twin with the mapped
normal at its vertices, the feature planes against ray queries, and callers of the older options records."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_attrs as M  # noqa: E402
import normal_maps as NM  # noqa: E402
import rays as R  # noqa: E402

pytestmark = pytest.mark.gpu


def trace(pkg, gpu, scene, rays):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()
    return gpu.trace_rays(scene, t).cpu().numpy().reshape(-1).view(pkg.RAYHIT_DTYPE)


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def mapped_ids(pkg, desc, maps):
    mats = {m.material for m in maps}
    return [i for i in range(desc.n_hittables) if desc.hittables[i].kind == pkg._abi.RT_HIT_TRIANGLE and desc.hittables[i].material in mats]


# ---- 1. ray by ray -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NM.SCENES)
def test_rays_agree_with_the_f64_answer(pkg, orc, gpu, name):
    """On the decidable, non-edge rays away from a texel boundary that hit a mapped attribute triangle: front_face is the f64 answer's and n
    lies within 2 x the f32 statement's own error (normal_maps.MEASURED_F32, measured on a CPU). On EVERY ray t, p, u, v, hittable, material
    and hit / miss are the bytes of the same upload without the map, and a hit on anything unmapped is that upload's whole record. In
    `wrapped` one more triangle of the mapped material carries no attributes: it is mapped too, by its barycentrics."""
    from conftest import record_metric
    A = pkg._abi
    ms = NM.mapped_set(pkg, orc, name)
    s, desc, attrs, maps = ms["base"], ms["desc"], ms["mesh"].attrs, ms["maps"]
    rays = s["rays"]
    feat = pkg.compile_info(desc, triangle_attrs=attrs, normal_maps=maps)["features"]
    assert feat & A.RT_FEATURE_NORMAL_MAP and feat & A.RT_FEATURE_TRI_ATTR and feat & 32, feat
    plain, mapped = gpu.upload(desc, triangle_attrs=attrs), gpu.upload(desc, triangle_attrs=attrs, normal_maps=maps)
    assert plain.fingerprint != mapped.fingerprint
    h0, h1 = trace(pkg, gpu, plain, rays), trace(pkg, gpu, mapped, rays)
    plain.close(); mapped.close()
    for f in ("t", "p", "u", "v", "hittable", "material"):
        assert same_bytes(h0[f], h1[f]), f
    assert (((h0["flags"] ^ h1["flags"]) & A.RT_RAYHIT_HIT) == 0).all() and ((h1["flags"] & ~np.uint32(3)) == 0).all()
    ids = mapped_ids(pkg, desc, maps)
    other = ~np.isin(h1["hittable"], ids)
    assert same_bytes(h0[other], h1[other])
    g_hit, g_ff = (h1["flags"] & A.RT_RAYHIT_HIT) != 0, (h1["flags"] & A.RT_RAYHIT_FRONT_FACE) != 0
    use = ms["use"]
    assert g_hit[use].all(), f"decidable rays {np.flatnonzero(use & ~g_hit)[:8]} miss"
    k = np.flatnonzero(use)
    dn = np.linalg.norm(h1["n"][k].astype(np.float64) - ms["n"][k], axis=1)
    moved = np.linalg.norm(h1["n"][k].astype(np.float64) - h0["n"][k], axis=1)
    bound = NM.bound_of(name)["n"]
    print(f"{name}: {len(rays)} rays, {len(k)} compared; worst |dn| {dn.max():.3e} (ray {k[dn.argmax()]}, allowed {bound:.3e}); front_face differs on "
          f"{int((g_ff[k] != ms['ff'][k]).sum())}; the normal moves by {np.median(moved):.3f} (median) against the unmapped upload")
    record_metric(config="normal_maps", scene=name, dn=float(dn.max()))
    assert (g_ff[k] == ms["ff"][k]).all(), f"front_face differs on decidable rays {k[g_ff[k] != ms['ff'][k]][:8]}"
    assert (np.einsum("ij,ij->i", h1["n"][k].astype(np.float64), rays["d"][k].astype(np.float64)) <= 0).all()
    assert dn.max() <= bound, (dn.max(), bound, int(k[dn.argmax()]))
    assert np.median(moved) > 0.05                                               # with the fields unread nothing moves
    lone = [i for i in ids if i not in ms["mesh"].tris]
    assert len(lone) == (1 if name == "wrapped" else 0)
    if lone:
        # the triangle without attributes (no wrapper above it): uv_k = (0,0), (1,0), (0,1) and (u, v) the barycentrics; its own measured figure
        ls = NM.lone_set(pkg, orc)
        q, bound = ls["k"], NM.bound_of("wrapped_lone")["n"]
        assert ls["hittable"] == lone[0] and (h1["hittable"][q] == lone[0]).all() and len(q) >= 50 and ls["left_out"] <= NM.TEXEL_CAP
        dl = np.linalg.norm(h1["n"][q].astype(np.float64) - ls["n"], axis=1)
        ml = np.linalg.norm(h1["n"][q].astype(np.float64) - h0["n"][q], axis=1)
        print(f"{name}: the triangle without attributes: {len(q)} rays, worst |dn| {dl.max():.3e} (allowed {bound:.3e}), moved by {np.median(ml):.3f} (median)")
        record_metric(config="normal_maps", scene="wrapped_lone", dn=float(dl.max()))
        assert dl.max() <= bound and (g_ff[q] == ls["ff"]).all() and np.median(ml) > 0.05


# ---- 2. every layout ---------------------------------------------------------------------------------------------------------------------------
def test_every_layout_gives_the_same_records(pkg, orc, gpu):
    A = pkg._abi
    ms = NM.mapped_set(pkg, orc, "wrapped")
    s, desc, attrs, maps = ms["base"], ms["desc"], ms["mesh"].attrs, ms["maps"]
    cases = [("default", 0, {}, A.RT_BVH_REFERENCE), ("reference_counters", A.RT_LAYOUT_REFERENCE_COUNTERS, {}, A.RT_BVH_REFERENCE),
             ("hbm", A.RT_LAYOUT_SCENE_IN_HBM, {}, A.RT_BVH_REFERENCE), ("hbm_32b", A.RT_LAYOUT_SCENE_IN_HBM | A.RT_LAYOUT_NODES_32B, {}, A.RT_BVH_REFERENCE),
             ("wide", A.RT_LAYOUT_WIDE_NODES, {}, A.RT_BVH_REFERENCE), ("hbm_wide", A.RT_LAYOUT_SCENE_IN_HBM | A.RT_LAYOUT_WIDE_NODES, {}, A.RT_BVH_REFERENCE),
             ("collapse_4", 0, dict(leaf_collapse=4), A.RT_BVH_REFERENCE), ("sah", 0, {}, A.RT_BVH_SAH),
             ("no_shade_tables", A.RT_LAYOUT_NO_SHADE_TABLES_IN_LDS, {}, A.RT_BVH_REFERENCE)]
    keep = ~s["edge"]
    first = None
    for label, flags, more, builder in cases:
        desc.bvh_builder = builder
        try:
            info = pkg.compile_info(desc, flags, triangle_attrs=attrs, normal_maps=maps, **more)
            scene = gpu.upload(desc, flags, triangle_attrs=attrs, normal_maps=maps, **more)
        finally:
            desc.bvh_builder = A.RT_BVH_REFERENCE
        h = trace(pkg, gpu, scene, s["rays"])
        scene.close()
        assert info["n_tri_attrs"] == 81 and info["n_tris"] == 82 and info["features"] & A.RT_FEATURE_NORMAL_MAP, (label, info)
        print(f"{label}: {info['n_nodes']} records, {int(((h['flags'] & 1) != 0).sum())} hits")
        if first is None:
            first = h
            continue
        diff = np.flatnonzero(keep & (h.view(np.uint8).reshape(len(h), -1) != first.view(np.uint8).reshape(len(h), -1)).any(axis=1))
        assert len(diff) == 0, f"{label}: records differ from the default layout's on rays {diff[:8]}"
    k = np.flatnonzero(ms["use"])
    assert np.linalg.norm(first["n"][k].astype(np.float64) - ms["n"][k], axis=1).max() <= NM.bound_of("wrapped")["n"]


# ---- 3. every kernel form --------------------------------------------------------------------------------------------------------------------
def test_every_kernel_form_gives_one_frame(pkg, orc, gpu):
    """A mapped subdivision-2 sphere mesh under the sky gradient, 48 x 32 x 8: the default render (at this size the drain form of k_extend),
    RT_FLAG_FUSED, tail_paths = 1 (k_shade to the end), two accumulated passes and a pixel-list pass over every pixel give the same bytes;
    and a radiance query along a ray gives the bytes of the render that traces that ray through every pixel (tests/radiance.py)."""
    import torch
    import radiance as RQ
    A = pkg._abi
    W, H, SPP = 48, 32, 8
    mesh = M.build_scene(pkg, "ico2")
    desc, maps = NM.bind(pkg, mesh, NM.random_map())
    cam = mesh.built.cam
    scene, unmapped = gpu.upload(desc, triangle_attrs=mesh.attrs, normal_maps=maps), gpu.upload(desc, triangle_attrs=mesh.attrs)
    prm = pkg.make_params(W, H, SPP)
    out = {"default": gpu.render(scene, cam, prm), "fused": gpu.render(scene, cam, pkg.make_params(W, H, SPP, flags=A.RT_FLAG_FUSED)),
           "tail_1": gpu.render(scene, cam, pkg.make_params(W, H, SPP, tail_paths=1))}
    assert out["fused"][1]["shade_launches"] == 0 and out["fused"][1]["drain_paths"] > 0
    assert out["tail_1"][1]["shade_launches"] > 0 and out["tail_1"][1]["drain_paths"] == 0
    base = out["default"][0]
    flat, _ = gpu.render(unmapped, cam, prm)
    assert np.isfinite(base).all() and np.abs(base - flat).mean() / SPP > 1e-3     # the map is seen
    for form in ("fused", "tail_1"):
        assert same_bytes(out[form][0], base), form
    half = pkg.make_params(W, H, SPP // 2)
    acc, _, _ = gpu.render_pass(scene, cam, half, 0, SPP, False)
    acc, _, _ = gpu.render_pass(scene, cam, half, SPP // 2, SPP, True, rgb_sum=np.ascontiguousarray(acc).reshape(-1))
    assert same_bytes(acc, base)
    for tail in (0, 1):
        lst = torch.arange(W * H, dtype=torch.int32, device="cuda")
        rgb = torch.full((3 * W * H,), 2.5, dtype=torch.float32, device="cuda")
        sq = torch.full((3 * W * H,), 2.5, dtype=torch.float32, device="cuda")
        counts = torch.zeros(W * H, dtype=torch.int32, device="cuda")
        gpu.render_pass_pixels(scene, cam, pkg.make_params(W, H, SPP, tail_paths=tail), 0, SPP, False, lst, lst.numel(), rgb, sq, counts)
        assert same_bytes(rgb.cpu().numpy(), base), tail
        assert (counts.cpu().numpy() == SPP).all()
    # the radiance query: a ray at the mesh from the camera, through a zero-field camera and as path_rays with the draws that camera spent
    origin, direction, seed = (0.3, 0.4, 4.0), (-0.25, -0.2, -4.0), 11
    n0 = RQ.draw_counts(orc, seed)[0]
    zcam = RQ.zero_field_camera(pkg, origin, direction, 0.0)
    for tail in (0, 1):
        zprm = pkg.make_params(RQ.W, RQ.H, 1, seed=seed, tail_paths=tail)
        for sample in range(2):
            img, _, st_r = gpu.render_pass(scene, zcam, zprm, sample, RQ.SAMPLES, False)
            rays = pkg.path_rays(origin, direction, time=0.0, first_draw=n0[:, sample])
            rgb, sq, inv, st_q = gpu.radiance(scene, rays, 1, with_stats=True, seed=seed, first_sample=sample, first_stream=0, tail_paths=tail)
            assert (inv == 0).all() and same_bytes(np.asarray(rgb, np.float32), np.asarray(img, np.float32)), (tail, sample)
            assert st_q["segments"] == st_r["segments"] and st_q["segments"] / st_q["samples"] >= 1.5
            flat_img, _, _ = gpu.render_pass(unmapped, zcam, zprm, sample, RQ.SAMPLES, False)
            assert not same_bytes(flat_img, img)
    scene.close(); unmapped.close()


# ---- 4. the twin -----------------------------------------------------------------------------------------------------------------------------
TWIN_TEXEL = (200, 90, 230)


def twin_scene(pkg, kind):
    """The large triangle of mesh_attrs (facet normal +z) as grey Lambertian under an XzRect light, which is the lights list. kind: "mapped" =
    a one-texel map on its material, "twin" = no map and the f64 mapped normal at all three vertices, "plain" = neither."""
    b = pkg.SceneBuilder(background=(0.02, 0.02, 0.03))
    grey, lamp = b.lambertian((0.7, 0.7, 0.7)), b.diffuse_light((12.0, 12.0, 12.0))
    P = {0: np.array(M.BIG_VERTS)}
    ns = pkg.normal_map_reference(P, None, [0], [0.3], [0.3], np.asarray(TWIN_TEXEL, np.uint8).reshape(1, 1, 3))[0][0]
    t = b.triangle(*M.BIG_VERTS, grey, normals=[ns] * 3 if kind == "twin" else None)
    assert t == 0
    rect = b.xz_rect(-2.0, 2.0, 0.5, 3.0, 4.0, lamp)
    if kind == "mapped":
        b.normal_map(grey, np.asarray(TWIN_TEXEL, np.uint8).reshape(1, 1, 3))
    desc = b.desc(b.hittable_list([t, b.flip_face(rect)]), lights=rect)
    return b, desc, pkg.camera_new((0.5, 0.3, 6.0), (0, 0, 0), (0, 1, 0), 50.0, 1.5, 0.0, 6.0, 0.0, 0.0), ns


def test_mapped_triangle_against_its_twin(pkg, gpu):
    """A constant map is a constant shading normal: the triangle with the map against the same triangle with that normal (the f64 statement's)
    at its vertices. The ray queries' normals agree within the bound measured for `big`; the two 48 x 32 x 8 renders agree within
    tests/test_gpu_scenes.py check()'s default tolerances (mean 1.2e-4, 1.5 % of the pixels beyond 2e-3), and the mapped render is more than
    ten times that away from the unmapped, untwinned one."""
    from conftest import record_metric
    W, H, SPP = 48, 32, 8
    frames, normals = {}, {}
    for kind in ("mapped", "twin", "plain"):
        b, desc, cam, ns = twin_scene(pkg, kind)
        scene = gpu.upload(desc, triangle_attrs=b.triangle_attrs(), normal_maps=b.normal_maps())
        frames[kind] = {form: gpu.render(scene, cam, pkg.make_params(W, H, SPP, **kw))[0].astype(np.float64) for form, kw in (("default", {}), ("tail_1", dict(tail_paths=1)))}
        h = trace(pkg, gpu, scene, R.camera_rays(cam, W, H, np.random.default_rng(2)))
        normals[kind] = h["n"][((h["flags"] & 1) != 0) & (h["hittable"] == 0)].astype(np.float64)
        scene.close()
    assert len(normals["mapped"]) == len(normals["twin"]) > 300
    bound = NM.bound_of("big")["n"]
    d_ref, d_twin = np.linalg.norm(normals["mapped"] - ns, axis=1).max(), np.linalg.norm(normals["mapped"] - normals["twin"], axis=1).max()
    print(f"normals: mapped against the f64 statement {d_ref:.3e}, against the twin {d_twin:.3e} (allowed {bound:.3e}); against the plain triangle {np.linalg.norm(normals['mapped'] - normals['plain'], axis=1).max():.3f}")
    assert d_ref <= bound and d_twin <= bound
    for form in ("default", "tail_1"):
        d = np.abs(frames["mapped"][form] - frames["twin"][form]) / SPP
        far = np.abs(frames["mapped"][form] - frames["plain"][form]) / SPP
        mean, bad = float(d.mean()), float((d.max(axis=2) > 2e-3).mean())
        print(f"{form}: mapped against twin: mean {mean:.3e}  bad {bad:.4f};  against the plain triangle: mean {far.mean():.3e}; level {frames['mapped'][form].mean() / SPP:.4f}")
        record_metric(config="normal_maps", scene="twin", form=form, mean=mean, bad=bad, far=float(far.mean()))
        assert np.isfinite(frames["mapped"][form]).all() and frames["mapped"][form].mean() / SPP > 0.01
        assert mean <= 1.2e-4 and bad <= 0.015, (form, mean, bad)
        assert far.mean() > 10 * 1.2e-4, (form, far.mean())
    assert same_bytes(frames["mapped"]["default"], frames["mapped"]["tail_1"])


# ---- 5. the feature planes ---------------------------------------------------------------------------------------------------------------------
def test_feature_normals_are_the_mapped_ones(pkg, orc, gpu):
    """The normal plane of a feature pass (k_features_export's all-features attribute instance) is the sum of the n rt_trace_rays reports for
    the same camera rays, made on the host (tests/features.py camera_rays), within 1e-6 per sample. The mesh is the FLAT subdivision-2 sphere
    (texture coordinates, no vertex normals), so a mapped normal is constant over a (facet, texel) cell and the f32 roundings of the
    device's own camera ray (about 1e-6 of the hit point, tests/test_gpu_mesh_attrs.py) move it only where they cross into another cell:
    those pixels are left out — a ray query within 4e-6 (M.bound_of uv x 3) of a texel boundary in (u, v), at most 2 % of the pixels that
    hit (the project's allowance for texel boundaries), and an undecidable or an edge ray, at most 5 % (the share the ray sets of
    tests/test_mesh_attrs_host.py allow for the two). Progressive.features() shows the same detail."""
    import torch
    import features as F
    A = pkg._abi
    W = H = 32
    SPP, SEED = 2, 5
    mesh = M.build_scene(pkg, "ico2", smooth=False)
    desc, maps = NM.bind(pkg, mesh, NM.random_map())
    cam = mesh.built.cam
    mapped, unmapped = gpu.upload(desc, triangle_attrs=mesh.attrs, normal_maps=maps), gpu.upload(desc, triangle_attrs=mesh.attrs)
    prm = pkg.make_params(W, H, SPP, seed=SEED)
    want, ok, hit_all, on_texel_edge = np.zeros((W * H, 3)), np.ones(W * H, bool), np.ones(W * H, bool), np.zeros(W * H, bool)
    delta = 3.0 * M.bound_of("ico2")["uv"]
    for sample in range(SPP):
        o, d, tm = F.camera_rays(orc, cam, W, H, SEED, sample)
        rays = R.make_rays(o, d, tm)
        ref = R.ask(orc, desc, rays)
        ids, on = R.objects_at(pkg, desc, ref["p"], np.zeros(len(rays)), mesh.built.extent)
        h = trace(pkg, gpu, mapped, rays)
        hit = (h["flags"] & A.RT_RAYHIT_HIT) != 0
        steady = np.ones(len(rays), bool)
        texel = None
        for su in (0.0, -delta, delta):
            for sv in (0.0, -delta, delta):
                i, j = pkg.texel_of(h["u"].astype(np.float64) + su, h["v"].astype(np.float64) + sv, NM.MAP_W, NM.MAP_H)
                texel = j * NM.MAP_W + i if texel is None else texel
                steady &= (j * NM.MAP_W + i) == texel
        ok &= ~R.undecidable(orc, desc, rays, ref) & (~ref["hit"] | (on.sum(axis=1) == 1)) & (~hit | steady) & (hit == ref["hit"])
        hit_all &= hit
        on_texel_edge |= hit & ~steady
        want += np.where(hit[:, None], h["n"].astype(np.float64), 0.0)
    a, n, dep, hits = gpu.render_features(mapped, cam, prm)
    _, n_flat, _, _ = gpu.render_features(unmapped, cam, prm)
    torch.cuda.synchronize()
    n, n_flat, hits = n.cpu().numpy().reshape(-1, 3), n_flat.cpu().numpy().reshape(-1, 3), hits.cpu().numpy().view(np.uint32)
    k = np.flatnonzero(ok & hit_all)
    assert (hits[k] == SPP).all() and len(k) >= 300                          # (the sphere covers about 0.4 of this frame)
    assert on_texel_edge.sum() <= NM.TEXEL_CAP * hit_all.sum() and len(k) >= (1.0 - NM.TEXEL_CAP - 0.05) * hit_all.sum(), (int(on_texel_edge.sum()), len(k), int(hit_all.sum()))
    dn = np.abs(n[k].astype(np.float64) - want[k]).max(axis=1)
    moved = np.linalg.norm(n[k].astype(np.float64) - n_flat[k], axis=1) / SPP
    print(f"feature normals against the ray queries' sums on {len(k)} of {int(hit_all.sum())} pixels that hit ({int(on_texel_edge.sum())} on a texel boundary): worst |dn| {dn.max():.3e} (allowed {1e-6 * SPP:.1e}); moved by {np.median(moved):.3f} (median)")
    assert dn.max() <= 1e-6 * SPP, (dn.max(), int(k[dn.argmax()]))
    assert np.median(moved) > 0.05
    prog_m = pkg.Progressive(gpu, mapped, cam, pkg.make_params(W, H, 4), 4).features(2)[1]
    prog_u = pkg.Progressive(gpu, unmapped, cam, pkg.make_params(W, H, 4), 4).features(2)[1]
    seen = np.linalg.norm(prog_m.reshape(-1, 3)[k] - prog_u.reshape(-1, 3)[k], axis=1)
    assert prog_m.shape == (H, W, 3) and np.median(seen) > 0.05
    mapped.close(); unmapped.close()


# ---- 6. old callers ----------------------------------------------------------------------------------------------------------------------------
def test_48_byte_options_render_the_unmapped_frame(pkg, gpu):
    """A caller compiled against RtUploadOptionsEnv (struct_bytes 48) with a map list behind its record: the list is not read."""
    A = pkg._abi
    W, H, SPP = 48, 32, 8
    mesh = M.build_scene(pkg, "ico1")
    desc, maps = NM.bind(pkg, mesh, NM.random_map())
    cam = mesh.built.cam
    old = pkg.upload_options(triangle_attrs=mesh.attrs, normal_maps=maps)
    new = pkg.Scene(gpu, desc, pkg.upload_options(triangle_attrs=mesh.attrs, normal_maps=maps))
    old.struct_bytes = 48
    C.cast(C.byref(old), C.POINTER(A.RtUploadOptionsMaps)).contents.normal_maps = C.cast(C.c_void_p(8), C.POINTER(A.RtNormalMap))      # never dereferenced
    a, b = pkg.Scene(gpu, desc, old), gpu.upload(desc, triangle_attrs=mesh.attrs)
    assert a.fingerprint == b.fingerprint != new.fingerprint
    prm = pkg.make_params(W, H, SPP)
    fa, fb, fn = gpu.render(a, cam, prm)[0], gpu.render(b, cam, prm)[0], gpu.render(new, cam, prm)[0]
    assert same_bytes(fa, fb) and not same_bytes(fn, fb) and np.isfinite(fn).all()
    a.close(); b.close(); new.close()
