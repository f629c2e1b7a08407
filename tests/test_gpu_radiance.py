"""Radiance queries on the device (include/rt_hip.h, "radiance queries"): the exact link to the render through a zero-field camera, per-ray
checks at max_depth 1 against trace_rays, the bit-for-bit invariances, a statistical comparison with a render, refusals and the panorama.
tests/radiance.py has the helpers and the reasoning behind the link and the bounds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import features as F  # noqa: E402
import radiance as RQ  # noqa: E402
from conftest import record_metric  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).reshape(-1)


# ---- the link to the render, exact ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "lights_many", "medium", "moving", "book1", "smooth_mesh", "cornell_reference_counters", "cornell_scene_in_hbm",
                                  "book1_wide_nodes", "cornell_never_drain", "cornell_depth_8"])
def test_query_returns_the_renders_samples(pkg, orc, gpu, name):
    """Through a zero-field camera every pixel and sample of a 16 x 12 render traces one ray; 192 copies of that ray, each with the draws the
    camera spent on its stream, must come back from the query with the render's bits: all 192 x 3 floats of each of the 8 samples, and the
    sums and squared sums after the eight accumulating calls."""
    A = pkg._abi
    c = next(x for x in RQ.cases(pkg) if x.name == name)
    n0 = RQ.draw_counts(orc, c.seed)[0]
    scene = RQ.upload(pkg, gpu, c)
    cam = RQ.zero_field_camera(pkg, c.origin, c.direction, c.t)
    prm = pkg.make_params(RQ.W, RQ.H, 1, max_depth=c.max_depth, seed=c.seed, flags=c.flags, tail_paths=c.tail_paths)
    R_sum = np.zeros(3 * RQ.N, np.float32); R_sq = np.zeros(3 * RQ.N, np.float32)
    Q_sum = np.zeros((RQ.N, 3), np.float32); Q_sq = np.zeros((RQ.N, 3), np.float32)
    for s in range(RQ.SAMPLES):
        img, _, st_r = gpu.render_pass(scene, cam, prm, s, RQ.SAMPLES, False)
        gpu.render_pass(scene, cam, prm, s, RQ.SAMPLES, s > 0, rgb_sum=R_sum, sq_sum=R_sq)
        rays = pkg.path_rays(c.origin, c.direction, time=c.t, first_draw=n0[:, s])
        kw = dict(max_depth=c.max_depth, seed=c.seed, first_sample=s, first_stream=0, tail_paths=c.tail_paths)
        rgb, sq, inv, st_q = gpu.radiance(scene, rays, 1, with_stats=True, **kw)
        gpu.radiance(scene, rays, 1, accumulate=s > 0, rgb_sum=Q_sum, sq_sum=Q_sq, **kw)
        assert (inv == 0).all()
        assert (bits(rgb) == bits(img)).all(), (name, s, int((bits(rgb) != bits(img)).sum()))
        assert st_q["samples"] == RQ.N and st_q["segments"] == st_r["segments"]
        if s == 0:      # not a vacuous case: the samples differ from pixel to pixel and the paths bounce
            assert len(np.unique(rgb, axis=0)) >= 96, len(np.unique(rgb, axis=0))
            assert st_q["segments"] / st_q["samples"] >= 2.0
            assert (bits(sq) == bits(rgb * rgb)).all()
    assert (bits(Q_sum) == bits(R_sum)).all() and (bits(Q_sq) == bits(R_sq)).all()
    scene.close()


# ---- varied rays, per ray, at max_depth 1 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["yard", "lit"])
def test_depth_one_agrees_with_trace_rays(pkg, gpu, which):
    """max_depth = 1: a sample is the background of d on a miss, `emitted` on a front-face light hit, 0 otherwise. 4096 rays of mixed origins,
    directions and times; hit or miss and the emitted colour from trace_rays on the same upload, for every ray."""
    A = pkg._abi
    rng = np.random.default_rng(17)
    if which == "yard":
        built = RQ.R.build_scene(pkg, "yard")
        desc = built.desc
        aimed = RQ.R.yard_aimed_rays(pkg, built, rng)[:2048]
        rays = np.concatenate([pkg.path_rays(aimed["o"], aimed["d"], time=aimed["time"]), RQ.varied_rays(pkg, rng, 4096 - len(aimed), (-12, 0.2, -12), (12, 6, 12))])
    else:
        desc = RQ.lit_scene(pkg)
        rays = RQ.varied_rays(pkg, rng, 4096, (-4, -0.4, -2.4), (4, 3.4, 6))
    assert len(rays) == 4096
    scene = gpu.upload(desc)
    hits = gpu.trace_rays(scene, RQ.as_query_rays(pkg, rays))
    rgb, sq, inv = gpu.radiance(scene, rays, 1, max_depth=1, seed=9)
    assert (inv == 0).all() and (hits["flags"] & A.RT_RAYHIT_INVALID_RAY == 0).all()
    hit = (hits["flags"] & A.RT_RAYHIT_HIT) != 0
    assert hit.sum() > 200 and (~hit).sum() > 200, hit.sum()            # both kinds occur in number
    bg = F.background(desc, rays["d"].astype(np.float64))
    want = np.where(hit[:, None], RQ.emitted(pkg, desc, hits), bg)
    # a hit returns a colour copied from the material (exact in f32) or 0; a miss the background within the rounding of the gradient
    assert (rgb[hit] == want[hit].astype(np.float32)).all()
    err = np.abs(rgb[~hit].astype(np.float64) - want[~hit])
    record_metric(test="radiance_depth_one", scene=which, hits=int(hit.sum()), emitters=int((want[hit].sum(axis=1) > 0).sum()), worst_background_error=float(err.max()))
    if desc.background_mode != 0:
        assert err.max() <= RQ.BACKGROUND_BOUND
    else:               # a constant background is the scene's colour as the device holds it, in f32: a copy
        assert (rgb[~hit] == want[~hit].astype(np.float32)).all()
    # miss or hit agrees for every ray: a miss is the background, which no hit returns in these scenes (no emitter has its colour)
    assert bg.min() > 0.1 and (np.abs(rgb[hit].astype(np.float64) - bg[hit]).max(axis=1) > 1e-3).all()
    if which == "lit":
        assert (want[hit].sum(axis=1) > 0).sum() >= 20                  # rays that end on a light's front face
    scene.close()


# ---- invariances, bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lit(pkg, gpu):
    rng = np.random.default_rng(23)
    rays = RQ.varied_rays(pkg, rng, 5000, (-4, -0.4, -2.4), (4, 3.4, 6))
    scene = gpu.upload(RQ.lit_scene(pkg))
    ref = gpu.radiance(scene, rays, 6, max_depth=12, seed=21, first_stream=1000, with_stats=True)
    yield dict(scene=scene, rays=rays, ref=ref, kw=dict(max_depth=12, seed=21))
    scene.close()


def same(a, b):
    return (bits(a[0]) == bits(b[0])).all() and (bits(a[1]) == bits(b[1])).all() and (a[2] == b[2]).all()


def test_invariances(pkg, gpu, lit):
    import torch
    scene, rays, ref, kw = lit["scene"], lit["rays"], lit["ref"], lit["kw"]
    assert np.isfinite(ref[0]).all() and ref[3]["samples"] == 5000 * 6 and ref[3]["segments"] > ref[3]["samples"]
    assert len(np.unique(ref[0], axis=0)) > 1250          # (a ray that leaves the scene at once returns the constant background: the others differ)
    # the same call twice; a pool of 4096 paths (chunks of 4096 rays x 1 sample) against the default (one chunk)
    assert same(gpu.radiance(scene, rays, 6, first_stream=1000, **kw), ref)
    small = gpu.radiance(scene, rays, 6, first_stream=1000, pool_slots=4096, with_stats=True, **kw)
    assert same(small, ref) and small[3]["pool_slots"] == 4096 and ref[3]["pool_slots"] >= 30000 and small[3]["samples"] == 30000
    # never drain
    assert same(gpu.radiance(scene, rays, 6, first_stream=1000, tail_paths=1, **kw), ref)
    # the device variant
    dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    d = gpu.radiance(scene, dev, 6, first_stream=1000, **kw)
    assert same([t.cpu().numpy() for t in d], ref)
    # the list split at 1777, first_stream moved
    a = gpu.radiance(scene, rays[:1777], 6, first_stream=1000, **kw)
    b = gpu.radiance(scene, rays[1777:], 6, first_stream=1000 + 1777, **kw)
    assert same([np.concatenate([x, y]) for x, y in zip(a, b)], ref)
    # the samples split 0..3 and 4..5, accumulating
    rgb, sq, inv = gpu.radiance(scene, rays, 4, first_stream=1000, **kw)
    gpu.radiance(scene, rays, 2, first_sample=4, first_stream=1000, accumulate=True, rgb_sum=rgb, sq_sum=sq, invalid=inv, **kw)
    assert same((rgb, sq, inv), ref)
    # ... on the device, in a pool that holds 4096 paths
    rgb_d, sq_d, inv_d = gpu.radiance(scene, dev, 4, first_stream=1000, pool_slots=4096, **kw)
    gpu.radiance(scene, dev, 2, first_sample=4, first_stream=1000, accumulate=True, rgb_sum=rgb_d, sq_sum=sq_d, invalid=inv_d, pool_slots=4096, **kw)
    assert same((rgb_d.cpu().numpy(), sq_d.cpu().numpy(), inv_d.cpu().numpy()), ref)
    # a different seed, stream or sample range is a different answer
    assert not same(gpu.radiance(scene, rays, 6, first_stream=1001, **kw), ref)
    assert not same(gpu.radiance(scene, rays, 6, first_sample=1, first_stream=1000, **kw), ref)


def test_invalid_rays(pkg, gpu, lit):
    A = pkg._abi
    scene, rays, ref, kw = lit["scene"], lit["rays"], lit["ref"], lit["kw"]
    bad = rays.copy()
    where = np.array([0, 1, 63, 64, 511, 512, 513, 1776, 1777, 2500, 4095, 4096, 4999])
    bad["o"][where[0::3], 0] = np.nan
    bad["d"][where[1::3]] = 0.0
    bad["first_draw"][where[2::3]] = 1 << 16
    bad["time"][where[3]] = np.inf
    ok = np.ones(5000, bool); ok[where] = False
    for pool in (0, 4096):
        rgb, sq, inv, st = gpu.radiance(scene, bad, 6, first_stream=1000, pool_slots=pool, with_stats=True, **kw)
        assert (inv[where] == A.RT_RAYHIT_INVALID_RAY).all() and (inv[ok] == 0).all()
        assert (bits(rgb[where]) == 0).all() and (bits(sq[where]) == 0).all()                 # +0, every bit
        assert (bits(rgb[ok]) == bits(ref[0][ok])).all() and (bits(sq[ok]) == bits(ref[1][ok])).all()     # the neighbours: as with a valid ray in their place
        assert st["samples"] == (5000 - len(where)) * 6
    # accumulating: the sums of an invalid ray are untouched, -0 and NaN included
    rgb = np.full((5000, 3), 7.25, np.float32); sq = np.full((5000, 3), 3.5, np.float32)
    rgb[where[0]] = -0.0; rgb[where[1], 1] = np.nan
    before = (rgb.copy(), sq.copy())
    gpu.radiance(scene, bad, 2, first_stream=1000, accumulate=True, rgb_sum=rgb, sq_sum=sq, **kw)
    assert (bits(rgb[where]) == bits(before[0][where])).all() and (bits(sq[where]) == bits(before[1][where])).all()
    assert (rgb[ok] != before[0][ok]).any(axis=1).mean() > 0.9
    # first_draw = 2^16 - 1 is the last valid count
    last = rays[:4].copy(); last["first_draw"] = (1 << 16) - 1
    assert (gpu.radiance(scene, last, 1, **kw)[2] == 0).all()


# ---- refusals: nothing written --------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_outputs_untouched(pkg, gpu, lit):
    import torch
    A, lib = pkg._abi, pkg.lib()
    scene, rays = lit["scene"], lit["rays"][:256]
    flat = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), rays.view(np.float32)])).cuda()
    dev = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)[:200].copy()).cuda()
    skew = flat[1:1 + 8 * 200].view(200, 8)                                  # 4 bytes off a 16-byte boundary
    assert dev.data_ptr() % 16 == 0 and skew.data_ptr() % 16 == 4 and skew.is_contiguous()
    outs = lambda: (torch.full((200, 3), 5.0, device="cuda"), torch.full((200, 3), 6.0, device="cuda"), torch.full((200,), 9, dtype=torch.uint8, device="cuda"))

    def refused(code, word, r=dev, **kw):
        rgb, sq, inv = outs()
        with pytest.raises(pkg.RtError) as e:
            gpu.radiance(scene, r, kw.pop("samples", 2), rgb_sum=rgb, sq_sum=sq, invalid=inv, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)
        assert (rgb == 5.0).all() and (sq == 6.0).all() and (inv == 9).all()

    refused(A.RT_ERR_INVALID, "samples", samples=0)
    refused(A.RT_ERR_INVALID, "flags", options=pkg.radiance_options(2, flags=4))
    refused(A.RT_ERR_INVALID, "render_flags", options=pkg.radiance_options(2, render_flags=A.RT_FLAG_COUNTERS))
    refused(A.RT_ERR_INVALID, "first_sample", first_sample=(1 << 32) - 2)
    refused(A.RT_ERR_INVALID, "first_stream", first_stream=(1 << 32) - 100)
    refused(A.RT_ERR_INVALID, "max_depth", max_depth=0)
    refused(A.RT_ERR_INVALID, "aligned", r=skew)
    short = pkg.radiance_options(2); short.struct_bytes = 48
    refused(A.RT_ERR_INVALID, "struct_bytes", options=short)
    # NULL rays / rgb_sum with n > 0, NULL options, NULL scene; n == 0 is a no-op that touches nothing
    rgb, sq, inv = outs()
    opt, st = pkg.radiance_options(2), A.RtStats()
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.rt_radiance_rays_device(gpu._h, scene._h, C.byref(opt), None, 200, p(rgb), p(sq), p(inv), C.byref(st)) == A.RT_ERR_INVALID
    assert lib.rt_radiance_rays_device(gpu._h, scene._h, C.byref(opt), p(dev), 200, None, p(sq), p(inv), C.byref(st)) == A.RT_ERR_INVALID
    assert lib.rt_radiance_rays_device(gpu._h, scene._h, None, p(dev), 200, p(rgb), p(sq), p(inv), C.byref(st)) == A.RT_ERR_INVALID
    assert lib.rt_radiance_rays_device(gpu._h, None, C.byref(opt), p(dev), 200, p(rgb), p(sq), p(inv), C.byref(st)) == A.RT_ERR_INVALID
    assert lib.rt_radiance_rays_device(gpu._h, scene._h, C.byref(opt), p(dev), 0, p(rgb), p(sq), p(inv), C.byref(st)) == A.RT_OK
    assert lib.rt_radiance_rays_device(gpu._h, scene._h, C.byref(opt), None, 0, None, None, None, None) == A.RT_OK
    assert (rgb == 5.0).all() and (sq == 6.0).all() and (inv == 9).all()
    # the optional outputs may be NULL: the sums are the ones of a call that asks for all three
    assert lib.rt_radiance_rays_device(gpu._h, scene._h, C.byref(opt), p(dev), 200, p(rgb), None, None, C.byref(st)) == A.RT_OK
    full = gpu.radiance(scene, dev, 2)
    assert (bits(rgb.cpu().numpy()) == bits(full[0].cpu().numpy())).all() and (sq == 6.0).all() and (inv == 9).all() and st.samples == 400
    # the host variant refuses the same things before it copies anything
    h = np.full((256, 3), 5.0, np.float32)
    with pytest.raises(pkg.RtError):
        gpu.radiance(scene, rays, 0, rgb_sum=h, sq_sum=h.copy(), invalid=np.zeros(256, np.uint8))
    assert (h == 5.0).all()
    # timing parts
    # timing parts: 30 000 paths are below the hand-over, so the drain carries them all; with tail_paths = 1 the wavefront loop does
    st = gpu.radiance(scene, lit["rays"], 6, options=pkg.radiance_options(6, max_depth=12, render_flags=A.RT_FLAG_TIMING), with_stats=True)[3]
    assert st["drain_ms"] > 0 and st["other_ms"] > 0 and st["render_ms"] > 0 and st["drain_paths"] >= 30000 and st["extend_ms"] == 0
    st = gpu.radiance(scene, lit["rays"], 6, options=pkg.radiance_options(6, max_depth=12, render_flags=A.RT_FLAG_TIMING, tail_paths=1), with_stats=True)[3]
    assert st["extend_ms"] > 0 and st["shade_ms"] > 0 and st["other_ms"] > 0 and st["drain_paths"] == 0 and st["iterations"] >= 2


# ---- statistical: a real camera on Cornell ------------------------------------------------------------------------------------------------------
def _z_against_render(pkg, orc, gpu, scene, cam, Wc, n, a, b):
    """radiance(n samples, seed b) along the sample-0 camera rays (seed a) of a Wc x Wc frame against render(n spp, seed a), and render(seed b)
    against render(seed a) as the yardstick: ((mean z, N, flat mask) of the query, mean z of the two renders, query sums, render sums)"""
    o, d, tm = F.camera_rays(orc, cam, Wc, Wc, a, 0)
    rays = pkg.path_rays(o, d, time=tm)
    qs, qq, inv = gpu.radiance(scene, rays, n, seed=b)
    assert (inv == 0).all()
    prm_a, prm_b = pkg.make_params(Wc, Wc, n, seed=a), pkg.make_params(Wc, Wc, n, seed=b)
    ra, rqa, _ = gpu.render_pass(scene, cam, prm_a, 0, n, False, sq_sum=np.zeros(3 * Wc * Wc, np.float32))
    rb, rqb, _ = gpu.render_pass(scene, cam, prm_b, 0, n, False, sq_sum=np.zeros(3 * Wc * Wc, np.float32))
    return RQ.mean_z(qs, qq, ra, rqa, n, n), RQ.mean_z(rb, rqb, ra, rqa, n, n)[0], qs, ra


def test_query_estimates_what_the_render_estimates(pkg, orc, gpu):
    """Per pixel and channel z = (mean_q - mean_r) / sqrt(se_q^2 + se_r^2) from both squared sums, in f64; |mean z| <= 4 / sqrt(N) over the N
    values with a variance. The same statistic between two renders (seeds a and b) is recorded beside it as the yardstick of the bound.

    The query traces ONE ray per pixel, the render a jittered footprint, so the two estimate the same number only where the radiance is linear
    over a pixel. The camera that is held to the bound therefore looks, from the box's usual viewpoint, at the part of the back wall above the
    boxes (6 degrees): lit by the lamp and by every other surface, and without a silhouette in view. The book's own 40-degree view is measured
    too, and reported: its first device run gave mean z = -0.262 for the query (bound 0.0745, N = 2883) where two renders gave +0.002 — a pixel
    that straddles an edge is brighter than its point sample half the time and darker the other half, but the darker sample has the smaller
    standard error and so the larger |z|; the exact link above (equal bits on this scene) says the paths themselves are the render's. Its
    values without variance on either side (the lamp seen directly, or nothing) must agree to the rounding of the rays."""
    Wc, n, a, b = 32, 256, 11, 12
    built = RQ.R.build_scene(pkg, "cornell")
    scene = gpu.upload(built.desc)
    wide = built.keep.camera(1.0)
    wall = pkg.camera_new((278.0, 278.0, -800.0), (278.0, 430.0, 555.0), (0, 1, 0), 6.0, 1.0, 0.0, 10.0, 0.0, 0.0)
    (z_q, N, flat), z_r, _, _ = _z_against_render(pkg, orc, gpu, scene, wall, Wc, n, a, b)
    (zw_q, Nw, flat_w), zw_r, qs_w, ra_w = _z_against_render(pkg, orc, gpu, scene, wide, Wc, n, a, b)
    record_metric(test="radiance_vs_render", mean_z_query=z_q, mean_z_two_renders=z_r, n_values=N, bound=4.0 / np.sqrt(N),
                  wide_view_mean_z_query=zw_q, wide_view_mean_z_two_renders=zw_r, wide_view_n_values=Nw, wide_view_flat_values=int(flat_w.sum()))
    print(f"mean z, back wall: query against render {z_q:+.4f}, render against render {z_r:+.4f}, bound {4.0 / np.sqrt(N):.4f}, N = {N}")
    print(f"mean z, whole box: query against render {zw_q:+.4f}, render against render {zw_r:+.4f}, N = {Nw}, flat = {int(flat_w.sum())}")
    assert N > 2000
    assert abs(z_q) <= 4.0 / np.sqrt(N)
    assert flat_w.sum() >= 30
    mq, mr = qs_w.reshape(-1).astype(np.float64)[flat_w] / n, ra_w.reshape(-1).astype(np.float64)[flat_w] / n
    assert np.abs(mq - mr).max() <= 1e-6 * max(1.0, np.abs(mr).max())
    scene.close()


# ---- the panorama ----------------------------------------------------------------------------------------------------------------------------------
def test_panorama_from_inside_a_furnace(pkg, gpu):
    """A 64 x 32 equirectangular panorama from inside a closed box of albedo 0.5 whose floor emits 2: no ray is invalid, every sample is finite
    and lies between 0 and the emitter's radiance, and a ray that looks at the emitter returns exactly its radiance."""
    E, S = 2.0, 16
    desc, keep = RQ.furnace(pkg, radiance=E)
    scene = gpu.upload(desc)
    rays = pkg.equirect_rays((0.25, -0.5, 0.125), 64, 32)
    rgb, sq, inv, st = gpu.radiance(scene, rays, S, max_depth=50, seed=3, with_stats=True)
    assert (inv == 0).all() and np.isfinite(rgb).all() and np.isfinite(sq).all()
    mean = rgb.astype(np.float64) / S
    assert (mean >= 0).all() and (mean <= E).all()
    d, o = rays["d"].astype(np.float64), rays["o"].astype(np.float64)
    t = (-2.0 - o[:, 1]) / np.where(d[:, 1] < 0, d[:, 1], -1e-30)
    p = o + t[:, None] * d
    floor = (d[:, 1] < -0.05) & (np.abs(p[:, 0]) < 1.99) & (np.abs(p[:, 2]) < 1.99)
    assert floor.sum() > 400 and (rgb[floor] == np.float32(E * S)).all()
    walls = d[:, 1] > 0.05                                                   # the upper half sees walls only: reflected light, below the emitter's
    assert (mean[walls] > 0.05).mean() > 0.95 and (mean[walls] < E).all()
    # the furnace's mean: a wall sees the emitter over about a sixth of its hemisphere and walls of the same kind over the rest
    record_metric(test="radiance_panorama", mean_wall=float(mean[walls].mean()), mean_all=float(mean.mean()), segments_per_sample=st["segments"] / st["samples"])
    assert st["samples"] == 64 * 32 * S
    scene.close()


def test_throughput_script_reports_what_it_says(tmp_path):
    """scripts/gpu_radiance.py (the table of DESIGN.md section 16) runs in a process of its own, at a tiny size, and reports what it says."""
    import json
    import subprocess
    root = RQ.R.ROOT
    out = tmp_path / "radiance.json"
    subprocess.run([sys.executable, os.path.join(root, "scripts", "gpu_radiance.py"), "--reps", "2", "--scale", "0.1", "--samples", "8", "--out", str(out)],
                   check=True, timeout=300, cwd=root, capture_output=True)
    doc = json.load(open(out))
    assert doc["frame"] == "60x60" and doc["samples"] == 8 and doc["paths"] == 60 * 60 * 8
    assert doc["query_render_ms"] > 0 and doc["render_render_ms"] > 0 and doc["query_rate_over_render_rate"] > 0
    assert doc["query_segments"] > doc["paths"] and doc["render_segments"] > doc["paths"]
    assert doc["mean_radiance_query"] > 0 and doc["mean_radiance_render"] > 0
