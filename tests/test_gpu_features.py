"""First-hit features on the GPU (include/rt_hip.h, "first-hit features"): the feature pass's rays are the render's own (bit for bit, in
every device layout), its albedo, normal and depth agree with ray queries of host-made rays and the f64 checker's textures, the sums are
invariant under chunking, sharding and splitting the sample range, and the edges of the contract hold."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import features as F  # noqa: E402
import rays as R  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = ("default", "reference_counters", "hbm", "hbm_32b", "hbm_wide")

# Worst deviation of a one-sample feature pass from the yardstick (ray queries of the host-made f32 rays, colours from the f64 checker at the
# yardstick's (u, v, p)), per scene, on the pixels kept, as measured on an MI355X (DESIGN.md section 12 has the table): |d albedo| (largest
# component), |d normal| (Euclidean), |d depth| / max(1, depth). The test allows 2 x the figure, the margin the project's parity tests use for
# box-to-box ocml rounding. The device builds its ray in f32, the host in f64 rounded to f32: a few ulps of direction, which is what these are.
# (The normals of the mesh are exact: a triangle's normal does not depend on where the ray meets it.)
MEASURED = {
    "book1": dict(albedo=7.720e-08, normal=2.906e-05, depth=8.302e-06),
    "cornell": dict(albedo=2.384e-08, normal=1.307e-04, depth=2.077e-05),
    "mesh": dict(albedo=7.630e-08, normal=0.000e+00, depth=4.575e-07),
    "moving": dict(albedo=7.630e-08, normal=2.621e-04, depth=9.385e-06),
    "rotated_sphere": dict(albedo=7.630e-08, normal=4.237e-06, depth=4.046e-07),
    "earth": dict(albedo=7.467e-08, normal=4.337e-06, depth=1.147e-06),
    "textured": dict(albedo=2.501e-05, normal=2.015e-05, depth=1.399e-06),
}


def layout_flags(A, name):
    return {"default": 0, "reference_counters": A.RT_LAYOUT_REFERENCE_COUNTERS, "hbm": A.RT_LAYOUT_SCENE_IN_HBM,
            "hbm_32b": A.RT_LAYOUT_SCENE_IN_HBM | A.RT_LAYOUT_NODES_32B, "hbm_wide": A.RT_LAYOUT_SCENE_IN_HBM | A.RT_LAYOUT_WIDE_NODES}[name]


def planes(out):
    """(albedo (n, 3), normal (n, 3), depth (n,), hits (n,) u32) of a render_features result, on the host."""
    a, n, d, h = out[:4]
    return a.cpu().numpy().reshape(-1, 3), n.cpu().numpy().reshape(-1, 3), d.cpu().numpy(), h.cpu().numpy().view(np.uint32)


def trace(pkg, gpu, scene, rays):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()
    return gpu.trace_rays(scene, t).cpu().numpy().reshape(-1).view(pkg.RAYHIT_DTYPE)


def lights_scene(pkg, moving):
    """Solid-colour DiffuseLight spheres (some of them moving, or their static twins) over one light rect that faces the camera, under a
    constant background; a camera with a lens and a shutter. Every path ends on its first hit: a render's pixel IS the first-hit albedo."""
    b = pkg.SceneBuilder(background=(0.125, 0.25, 0.5))
    rng = np.random.default_rng(42)
    ids = [b.xz_rect(-2.5, 2.5, -2.5, 2.5, -0.3, b.diffuse_light((0.75, 0.5, 0.25)))]
    for k in range(12):
        c = np.array([rng.uniform(-2.0, 2.0), rng.uniform(0.0, 1.2), rng.uniform(-2.0, 2.0)])
        m = b.diffuse_light(np.round(rng.uniform(0.1, 1.0, 3) * 64) / 64)
        if k % 2 and moving:
            ids.append(b.moving_sphere(c, c + np.array([0.0, 0.4, 0.2]), 0.0, 1.0, 0.3, m))
        else:
            ids.append(b.sphere(c, 0.3, m))
    desc = b.desc(b.bvh(ids, 0.0, 1.0))
    cam = pkg.camera_new((3.0, 2.5, 6.0), (0.0, 0.4, 0.0), (0, 1, 0), 35.0, 40 / 24, 0.3, 7.0, 0.0, 1.0)
    return R.Built(desc, cam, b, 6.0)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_feature_rays_are_the_renders_own(pkg, gpu, layout):
    """albedo_sum of a one-sample feature pass at first_sample = s equals, bit for bit, rgb_sum of rt_render_pass_device over [s, s + 1) in a
    scene of lights: the feature pass and the render made the same ray (jitter, lens offset, time) and rebuilt the same HitRecord."""
    import torch
    A = pkg._abi
    built = lights_scene(pkg, moving=layout != "hbm_wide")          # (the 8-wide walk is for static scenes)
    assert built.cam.lens_radius > 0 and built.cam.time0 < built.cam.time1
    scene = gpu.upload(built.desc, layout_flags(A, layout))
    W, H = 40, 24
    prm = pkg.make_params(W, H, 1, max_depth=4, seed=9, tile_size=16)
    for s in (0, 5):
        rgb = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
        gpu.render_pass(scene, built.cam, prm, s, 8, False, rgb)
        albedo, _, _, hits = planes(gpu.render_features(scene, built.cam, prm, first_sample=s))
        frame = rgb.cpu().numpy().reshape(-1, 3)
        wrong = np.flatnonzero((frame.view(np.uint32) != albedo.view(np.uint32)).any(axis=1))
        assert len(wrong) == 0, f"sample {s}: {len(wrong)} pixels differ, first at {[(int(i) % W, int(i) // W) for i in wrong[:5]]}"
        assert 0.3 * W * H < hits.sum() < 0.95 * W * H and len(np.unique(albedo, axis=0)) >= 8, "the frame should show lights and background"
    scene.close()


@pytest.mark.parametrize("name", F.SCENES)
def test_features_agree_with_the_yardsticks(pkg, orc, gpu, name):
    from conftest import record_metric
    s = F.pixel_set(pkg, orc, name)
    built, rays, ref, und = s["built"], s["rays"], s["ref"], s["undecidable"]
    W, H = F.GRID
    scene = gpu.upload(built.desc)
    yard = trace(pkg, gpu, scene, rays)                              # the yardstick: ray queries of the host-made rays
    albedo, normal, depth, hits = planes(gpu.render_features(scene, built.cam, pkg.make_params(W, H, 1, seed=F.SEED)))
    scene.close()
    A = pkg._abi
    y_hit, y_ff = (yard["flags"] & A.RT_RAYHIT_HIT) != 0, (yard["flags"] & A.RT_RAYHIT_FRONT_FACE) != 0
    # the yardstick against the checker, on this very ray set: hit / miss agree on decidable rays; its own error, measured here, is what the
    # texture-boundary rule moves (u, v, p) by, and stays within 2 x the figures recorded in tests/features.py (which the host test uses)
    assert not (~und & (y_hit != ref["hit"])).any()
    k = np.flatnonzero(~und & y_hit)
    err_p = float(np.abs(yard["p"][k].astype(np.float64) - ref["p"][k]).max())
    du = np.abs(yard["u"][k].astype(np.float64) - ref["u"][k]); du = np.minimum(du, 1.0 - du)
    polar = (ref["v"][k] < 1e-3) | (ref["v"][k] > 1.0 - 1e-3)
    err_uv = float(max(du[~polar].max(), np.abs(yard["v"][k].astype(np.float64) - ref["v"][k])[~polar].max()))
    print(f"{name}: yardstick against the checker |dp| {err_p:.3e} |d(u,v)| {err_uv:.3e} (recorded: {F.YARDSTICK_ERR[name]})")
    assert err_p <= 2 * F.YARDSTICK_ERR[name][0] and err_uv <= 2 * F.YARDSTICK_ERR[name][1]
    want, unstable = F.expected_albedo(pkg, orc, built.desc, y_hit, yard["material"], y_ff, yard["u"], yard["v"], yard["p"], rays["d"], err=(err_p, err_uv))
    # ---- the two caps ----
    print(f"{name}: {W * H} pixels, {int(und.sum())} undecidable, {int((unstable & y_hit).sum())} of {int(y_hit.sum())} hit pixels on a texture boundary (left out)")
    assert und.sum() <= 0.01 * W * H and (unstable & y_hit).sum() <= 0.02 * y_hit.sum()
    keep = ~und & ~unstable
    # ---- hit / miss for every kept pixel; the material shows in the albedo below ----
    wrong = keep & ((hits != 0) != y_hit)
    assert not wrong.any(), f"hit/miss differs on kept pixels {np.flatnonzero(wrong)[:8]}"
    assert (hits <= 1).all() and not normal[hits == 0].any() and not depth[hits == 0].any()
    # ---- measurement, then the bound ----
    dlen = np.linalg.norm(rays["d"].astype(np.float64), axis=1)
    want_depth = np.where(y_hit, yard["t"].astype(np.float64) * dlen, 0.0)
    want_n = np.where(y_hit[:, None], yard["n"].astype(np.float64), 0.0)
    da = float(np.abs(albedo[keep].astype(np.float64) - want[keep]).max())
    dn = float(np.linalg.norm(normal[keep].astype(np.float64) - want_n[keep], axis=1).max())
    dd = float((np.abs(depth[keep].astype(np.float64) - want_depth[keep]) / np.maximum(1.0, want_depth[keep])).max())
    print(f"{name}: worst |d albedo| {da:.3e}  |d normal| {dn:.3e}  |d depth|/max(1,depth) {dd:.3e}")
    record_metric(config="features", scene=name, albedo=da, normal=dn, depth=dd, undecidable=int(und.sum()), boundary=int((unstable & y_hit).sum()))
    assert dd <= 1e-3, "a depth this far off is a wrong ray, not rounding"
    m = MEASURED[name]
    assert da <= 2 * m["albedo"] and dn <= 2 * m["normal"] and dd <= 2 * m["depth"], (da, dn, dd, m)


def frame_bytes(out):
    return b"".join(p.tobytes() for p in planes(out))


@pytest.mark.parametrize("name", ["moving", "textured"])
def test_invariances_bit_for_bit(pkg, gpu, name):
    import torch
    A = pkg._abi
    built = F.build_scene(pkg, name)
    scene = gpu.upload(built.desc)
    W, H, N = 40, 24, 8
    prm = pkg.make_params(W, H, N, seed=3, tile_size=16)
    base = gpu.render_features(scene, built.cam, prm, with_stats=True)
    ref = frame_bytes(base)
    assert base[4]["samples"] == base[4]["segments"] == W * H * N and base[4]["extend_launches"] == 1
    # two calls, the same bytes
    assert frame_bytes(gpu.render_features(scene, built.cam, prm)) == ref
    # [0, 4) then [4, 8) accumulating
    half = pkg.make_params(W, H, N // 2, seed=3, tile_size=16)
    out = gpu.render_features(scene, built.cam, half)
    gpu.render_features(scene, built.cam, half, first_sample=N // 2, accumulate=True, albedo=out[0], normal=out[1], depth=out[2], hits=out[3])
    assert frame_bytes(out) == ref
    # the smallest pool: the pass runs in chunks
    small = gpu.render_features(scene, built.cam, prm, pool_slots=1, with_stats=True)
    assert small[4]["pool_slots"] == 4096 and small[4]["extend_launches"] == -(-W * H // (4096 // N)) > 1
    assert frame_bytes(small) == ref
    # three shards, untiled
    shards = [gpu.render_features(scene, built.cam, pkg.make_params(W, H, N, seed=3, tile_size=16, shard_index=k, shard_count=3)) for k in range(3)]
    full = pkg.make_params(W, H, N, seed=3, tile_size=16, shard_count=3)
    a_ref, n_ref, d_ref, h_ref = planes(base)
    for i, want in ((0, a_ref), (1, n_ref)):
        gathered = torch.cat([s[i] for s in shards])
        frame = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        gpu.untile_device(full, A.RT_OUT_RGB_SUM_F32, gathered.data_ptr(), frame.data_ptr())
        assert frame.cpu().numpy().tobytes() == want.tobytes()
    depth, hits = np.zeros(W * H, np.float32), np.zeros(W * H, np.uint32)
    for k, s in enumerate(shards):
        x, y, ok = pkg.slot_pixels(pkg.make_params(W, H, N, seed=3, tile_size=16, shard_index=k, shard_count=3))
        _, _, d, h = planes(s)
        depth[y[ok] * W + x[ok]], hits[y[ok] * W + x[ok]] = d[ok], h[ok]
        assert not d[~ok].any() and not h[~ok].any() and (~ok).any()              # (the wrapper's zero-filled planes: clipped slots stay 0)
    assert depth.tobytes() == d_ref.tobytes() and hits.tobytes() == h_ref.tobytes()
    scene.close()


def test_edges(pkg, orc, gpu):
    import torch
    A, lib = pkg._abi, pkg.lib()
    W, H, N = 40, 24, 8
    # ---- only the requested planes are written: guard words around every plane, and the clipped slots of a sharded layout ----
    built = lights_scene(pkg, moving=True)
    scene = gpu.upload(built.desc)
    prm = pkg.make_params(W, H, N, seed=9, tile_size=16, shard_index=1, shard_count=3)
    slots = pkg.output_floats(prm) // 3
    _, _, ok = pkg.slot_pixels(prm)
    assert (~ok).any()
    G = 8                                                            # guard words on either side (32 bytes: the planes stay 16-byte aligned)
    raw = [torch.full((3 * slots + 2 * G,), 123.25, dtype=torch.float32, device="cuda"), torch.full((3 * slots + 2 * G,), 123.25, dtype=torch.float32, device="cuda"),
           torch.full((slots + 2 * G,), 123.25, dtype=torch.float32, device="cuda"), torch.full((slots + 2 * G,), 12345, dtype=torch.int32, device="cuda")]
    view = [t[G:-G] for t in raw]
    gpu.render_features(scene, built.cam, prm, albedo=view[0], normal=view[1], depth=view[2], hits=view[3])
    sentinel = (123.25, 123.25, 123.25, 12345)
    for t, v, per in zip(raw, sentinel, (3, 3, 1, 1)):
        h = t.cpu().numpy()
        assert (h[:G] == v).all() and (h[-G:] == v).all()
        body = h[G:-G].reshape(slots, per)
        assert (body[~ok] == v).all() and (body[ok] != v).any(axis=1).all()
    all_four = [t.clone() for t in view]
    # a subset: the same values in the planes given, nothing else exists to write
    only = [torch.full_like(t, v) for t, v in zip(view, sentinel)]
    gpu.render_features(scene, built.cam, prm, albedo=only[0])
    gpu.render_features(scene, built.cam, prm, depth=only[2], hits=only[3])
    assert torch.equal(only[0], all_four[0]) and torch.equal(only[2], all_four[2]) and torch.equal(only[3], all_four[3]) and bool((only[1] == 123.25).all())
    # ---- a pixel that sees only the background: normal and depth sums exactly 0, albedo = the background folded N times ----
    full = pkg.make_params(W, H, N, seed=9, tile_size=16)
    albedo, normal, depth, hits = planes(gpu.render_features(scene, built.cam, full))
    sky = hits == 0
    assert sky.sum() > 20 and (hits == N).sum() > 20
    fold = np.zeros(3, np.float32)
    for _ in range(N):
        fold = fold + np.array(built.desc.background.tuple(), np.float32)
    assert not normal[sky].any() and not depth[sky].any() and (albedo[sky] == fold).all()
    assert (depth[~sky] > 0).all() and normal[~sky].any(axis=1).all()
    # ---- refusals: nothing is written ----
    poison = [torch.full((3 * W * H,), 123.25, dtype=torch.float32, device="cuda") for _ in range(3)] + [torch.full((W * H,), 12345, dtype=torch.int32, device="cuda")]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in poison]
    good_opt, good_buf = pkg.feature_options(), A.RtFeatureBuffers(*ptrs)

    def call(sc=scene, params=full, opt=good_opt, buf=good_buf):
        return lib.rt_render_features_device(gpu._h, sc._h, C.byref(built.cam), C.byref(params), C.byref(opt), C.byref(buf), None)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == v).all()) for t, v in zip(poison, sentinel))
    for kw, word in ((dict(opt=A.RtFeatureOptions(8, 0, 0, 0)), b"struct_bytes"), (dict(opt=A.RtFeatureOptions(16, 6, 0, 0)), b"unknown"),
                     (dict(opt=pkg.feature_options(first_sample=(1 << 32) - N)), b"2^32"), (dict(buf=A.RtFeatureBuffers(None, None, None, None)), b"null"),
                     (dict(buf=A.RtFeatureBuffers(ptrs[0], ptrs[1] + 4, ptrs[2], ptrs[3])), b"aligned"),
                     (dict(buf=A.RtFeatureBuffers(None, None, None, ptrs[3] + 8)), b"aligned"),
                     (dict(params=pkg.make_params(W, H, N, flags=A.RT_FLAG_COUNTERS)), b"RT_FLAG_COUNTERS"), (dict(params=pkg.make_params(W, H, N, flags=A.RT_FLAG_FUSED)), b"RT_FLAG_FUSED")):
        assert call(**kw) == A.RT_ERR_INVALID, word
        assert word in lib.rt_last_error(gpu._h), (word, lib.rt_last_error(gpu._h))
        assert untouched(), word
    fog = R.medium_scene(pkg)
    fog_scene = gpu.upload(fog.desc)
    assert call(sc=fog_scene) == A.RT_ERR_UNSUPPORTED and b"medium" in lib.rt_last_error(gpu._h).lower() and untouched()
    with pytest.raises(pkg.RtError) as e:
        gpu.render_features(fog_scene, fog.cam, full)
    assert e.value.code == A.RT_ERR_UNSUPPORTED
    fog_scene.close()
    # accepted flags: timing fills the stats; sample blocks change nothing
    timed = gpu.render_features(scene, built.cam, pkg.make_params(W, H, N, seed=9, tile_size=16, flags=A.RT_FLAG_TIMING | A.RT_FLAG_SAMPLE_BLOCKS), with_stats=True)
    assert timed[4]["extend_ms"] > 0 and timed[4]["other_ms"] > 0 and timed[4]["render_ms"] > 0
    assert planes(timed)[0].tobytes() == albedo.tobytes() and planes(timed)[3].tobytes() == hits.tobytes()
    scene.close()


def test_hits_count_the_samples_that_hit(pkg, orc, gpu):
    """hits of a two-sample pass = how many of the pixel's two host-made rays the yardstick says hit, on the pixels where both are decidable."""
    s = F.pixel_set(pkg, orc, "textured")
    built = s["built"]
    W, H = F.GRID
    o, d, tm = F.camera_rays(orc, built.cam, W, H, F.SEED, 1)
    rays1 = R.make_rays(o, d, tm)
    ref1 = R.ask(orc, built.desc, rays1)
    dec = ~s["undecidable"] & ~R.undecidable(orc, built.desc, rays1, ref1)
    scene = gpu.upload(built.desc)
    want = sum(((trace(pkg, gpu, scene, r)["flags"] & pkg._abi.RT_RAYHIT_HIT) != 0).astype(np.uint32) for r in (s["rays"], rays1))
    _, _, _, hits = planes(gpu.render_features(scene, built.cam, pkg.make_params(W, H, 2, seed=F.SEED)))
    scene.close()
    assert dec.mean() >= 0.98 and (hits[dec] == want[dec]).all() and set(np.unique(hits)) == {0, 1, 2}


def test_progressive_and_adaptive_features(pkg, gpu):
    """Progressive.features / Adaptive.features: means of a pass of their own, (H, W, 3), (H, W, 3), (H, W) and the hit fraction; a sharded
    instance returns its tiles in place."""
    built = F.build_scene(pkg, "textured")
    scene = gpu.upload(built.desc)
    W, H = 40, 24
    prog = pkg.Progressive(gpu, scene, built.cam, pkg.make_params(W, H, 1, seed=3, tile_size=16), frame_samples=16)
    a, n, d, f = prog.features(4)
    assert a.shape == n.shape == (H, W, 3) and d.shape == f.shape == (H, W) and a.dtype == np.float32
    sums = planes(gpu.render_features(scene, built.cam, pkg.make_params(W, H, 4, seed=3, tile_size=16)))
    assert np.array_equal(a.reshape(-1, 3), sums[0] / np.float32(4)) and np.array_equal(f.reshape(-1), sums[3].astype(np.float32) / np.float32(4))
    hit = f > 0
    assert hit.any() and (~hit).any() and np.median(np.linalg.norm(n[f == 1], axis=1)) > 0.95 and (d[hit] > 1).all() and not d[~hit].any()
    assert prog.samples_done == 0                                   # a feature pass renders no radiance sample
    ada = pkg.Adaptive(gpu, scene, built.cam, pkg.make_params(W, H, 1, seed=3, tile_size=16, shard_index=1, shard_count=3), frame_samples=16)
    a2, n2, d2, f2 = ada.features(4)
    x, y, ok = pkg.slot_pixels(ada.params)
    mine = np.zeros((H, W), bool); mine[y[ok], x[ok]] = True
    assert np.array_equal(a2[mine], a[mine]) and np.array_equal(n2[mine], n[mine]) and np.array_equal(d2[mine], d[mine]) and np.array_equal(f2[mine], f[mine])
    assert not a2[~mine].any() and not d2[~mine].any()
    scene.close()


def test_throughput_script_runs(tmp_path):
    """scripts/gpu_features.py (the figures of DESIGN.md section 12) runs in a process of its own and prints one JSON line."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "scripts", "gpu_features.py"), "--quick"], check=True, timeout=300, cwd=root, capture_output=True, text=True).stdout
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1
    row = json.loads(lines[0])
    assert row["width"] * row["height"] == row["rays_1spp"] and row["features_1spp_ms"] > 0 and row["query_1spp_ms"] > 0 and row["hit_fraction"] > 0
