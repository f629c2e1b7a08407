"""Progressive rendering on the GPU (rt_render_pass, include/rt_hip.h): passes that cover [0, N) leave exactly what one rt_render at N
samples per pixel writes, in every layout and with every flag; a lone pass renders the samples it names (against the f64 oracle); the
device's second moments give the fixtures' standard errors; bad passes are refused untouched; a checkpoint resumes bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 40
SPLITS = [(0, 1), (1, 8), (8, 13), (13, 40)]          # uneven, the first of a single sample
SPLITS16 = [(0, 16), (16, 32), (32, 40)]              # RT_FLAG_SAMPLE_BLOCKS: items of 16, the last one ragged


def with_spp(pkg, prm, spp):
    p = pkg._abi.RtParams.from_buffer_copy(prm)
    p.samples_per_pixel = spp
    return p


def run_passes(pkg, gpu, scene, cam, prm, splits, frame, device=False):
    """The passes of `splits` in order (the first overwrites, the rest accumulate): (rgb_sum, sq_sum) as flat float32 arrays."""
    n = pkg.output_floats(prm)
    if device:
        import torch
        rgb = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")      # an overwriting first pass does not read what is there
        sq = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    else:
        rgb, sq = None, np.full(n, 7.0, dtype=np.float32)
    for i, (a, b) in enumerate(splits):
        rgb, sq, st = gpu.render_pass(scene, cam, with_spp(pkg, prm, b - a), a, frame, i > 0, rgb, sq)
        assert st["samples"] % (b - a) == 0 and (prm.shard_count > 1 or st["samples"] == (b - a) * prm.width * prm.height)
    if device:
        return rgb.cpu().numpy(), sq.cpu().numpy()
    return np.asarray(rgb).reshape(-1), np.asarray(sq).reshape(-1)


def assert_passes_equal_one_shot(pkg, gpu, scene, cam, prm, splits=SPLITS, device=False):
    frame = splits[-1][1]
    one, _ = gpu.render(scene, cam, with_spp(pkg, prm, frame))
    rgb, sq = run_passes(pkg, gpu, scene, cam, prm, splits, frame, device)
    assert np.array_equal(rgb, one.reshape(-1)), float(np.abs(rgb - one.reshape(-1)).max())
    # the squared sums of the series are those of one pass over [0, N)
    rgb1, sq1 = run_passes(pkg, gpu, scene, cam, prm, [(0, frame)], frame, device)
    assert np.array_equal(rgb1, rgb) and np.array_equal(sq1, sq)
    assert np.isfinite(sq).all() or prm.nan_policy == pkg._abi.RT_NAN_REFERENCE
    assert (sq[np.isfinite(sq)] >= 0).all()
    return rgb, sq


@pytest.fixture(scope="module")
def book1(pkg, gpu):
    hs = pkg.HostScene("book1", 1)
    return hs, gpu.upload(hs.desc)


@pytest.fixture(scope="module")
def cornell(pkg, gpu):
    hs = pkg.HostScene("cornell", 0)
    return hs, gpu.upload(hs.desc)


def test_passes_book1_lds_host_and_device(pkg, gpu, book1):
    hs, scene = book1
    cam = hs.camera(64 / 40)
    prm = pkg.make_params(64, 40, 1)
    assert gpu.render(scene, cam, with_spp(pkg, prm, 4))[1]["bvh_in_lds"] == 1
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, prm)
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, prm, device=True)


def test_passes_book1_sample_blocks_tail_nan(pkg, gpu, book1):
    A = pkg._abi
    hs, scene = book1
    cam = hs.camera(64 / 40)
    # items of 16 samples (batch means in sq_sum), passes on item boundaries, the last ending at frame_samples
    prm = pkg.make_params(64, 40, 1, flags=A.RT_FLAG_SAMPLE_BLOCKS)
    assert pkg.pass_check(with_spp(pkg, prm, 16), 16, N) == 16
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, prm, SPLITS16)
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, prm, SPLITS16, device=True)
    # the wavefront loop to the end (no hand-over to the fused kernel), the reference's NaN policy, a small pool of long lineages
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, pkg.make_params(64, 40, 1, tail_paths=1))
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, pkg.make_params(64, 40, 1, nan_policy=A.RT_NAN_REFERENCE))
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, pkg.make_params(64, 40, 1, pool_slots=4096), device=True)


def test_passes_book1_sharded(pkg, gpu, book1):
    """tile_size 64, 3 shards of a 130 x 100 frame (clipped edge tiles): every shard's passes give its one-shot shard, tile-compact."""
    hs, scene = book1
    cam = hs.camera(1.3)
    shards = []
    for si in range(3):
        prm = pkg.make_params(130, 100, 1, tile_size=64, shard_index=si, shard_count=3)
        rgb, _ = assert_passes_equal_one_shot(pkg, gpu, scene, cam, prm, device=(si == 1))
        shards.append(rgb)
    per = pkg.output_floats(pkg.make_params(130, 100, 1, tile_size=64, shard_index=0, shard_count=3))
    g = np.zeros(3 * per, dtype=np.float32)
    for si, s in enumerate(shards):
        g[si * per:si * per + s.size] = s
    full, _ = gpu.render(scene, cam, pkg.make_params(130, 100, N))
    assert np.array_equal(pkg.untile(pkg.make_params(130, 100, N, tile_size=64, shard_count=3), g), full)


def test_passes_cornell_lights_instances_fused(pkg, gpu, cornell):
    A = pkg._abi
    hs, scene = cornell
    cam = hs.camera(1.0)
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, pkg.make_params(48, 48, 1), device=True)
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, pkg.make_params(48, 48, 1, flags=A.RT_FLAG_FUSED))


def test_passes_media(pkg, gpu):
    """cornell_smoke_lit: constant media in transformed boxes — the free-path draws are keyed by the absolute sample index."""
    hs = pkg.HostScene("cornell_smoke_lit", 0)
    scene = gpu.upload(hs.desc)
    cam = hs.camera(1.0)
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, pkg.make_params(48, 48, 1))
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, pkg.make_params(48, 48, 1, tail_paths=1), device=True)
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, pkg.make_params(48, 48, 1, flags=pkg._abi.RT_FLAG_SAMPLE_BLOCKS), SPLITS16)


def test_passes_book2_final(pkg, gpu, earth):
    """Moving sphere, image / noise textures, media."""
    hs = pkg.HostScene("final", 1, image=earth)
    scene = gpu.upload(hs.desc)
    assert_passes_equal_one_shot(pkg, gpu, scene, hs.camera(1.0), pkg.make_params(48, 48, 1))


def test_passes_scene_in_hbm(pkg, gpu):
    hs = pkg.HostScene("big_sah", 5, 200000, 256)
    scene = gpu.upload(hs.desc)
    cam = hs.camera(1.0)
    prm = pkg.make_params(40, 40, 1)
    assert gpu.render(scene, cam, with_spp(pkg, prm, 1))[1]["bvh_in_lds"] == 0
    assert_passes_equal_one_shot(pkg, gpu, scene, cam, prm, device=True)


def lone_pass_vs_oracle(pkg, orc, gpu, hs, scene, cam, W, H, mean_tol, bad_tol, sq_tol):
    """A lone pass over samples [5, 8) of an 8-sample frame against the oracle's per-sample radiance of those samples."""
    from conftest import record_metric
    prm = pkg.make_params(W, H, 3)
    n = pkg.output_floats(prm)
    img, sq, st = gpu.render_pass(scene, cam, prm, 5, 8, False, None, np.zeros(n, dtype=np.float32))
    assert st["samples"] == W * H * 3
    _, _, ps = orc.render(hs.desc, cam, pkg.make_params(W, H, 8), precision=64, n_threads=8, per_sample=True)
    ref = ps[:, :, 5:8].sum(axis=2)
    d = np.abs(img.astype(np.float64) - ref) / 3
    bad = float((d.max(axis=2) > 2e-3).mean())
    # the second moment of the same samples: sum of L^2 (one sample per item)
    ref2 = (ps[:, :, 5:8] ** 2).sum(axis=2)
    d2 = np.abs(sq.astype(np.float64) - ref2) / 3
    record_metric(config="progressive", crop=hs.name, mean=float(d.mean()), bad=bad, sq_mean=float(d2.mean()), sq_bad=float((d2.max(axis=2) > 2e-3).mean()))
    assert np.isfinite(img).all()
    assert d.mean() <= mean_tol and bad <= bad_tol, (d.mean(), bad)
    # (a sample whose f32 path leaves the f64 one's differs in L and so in L^2; measured on MI355X: book-1 5.1e-7, Cornell 1.3e-6 —
    # the bounds are about twice that)
    assert d2.mean() <= sq_tol, (d2.mean(), ref2.mean())
    # the other 5 samples are not in it: the full 8-sample frame minus this pass is far from 0
    assert np.abs(ps[:, :, :5].sum(axis=2)).mean() > 10 * d.mean()
    return img


def test_lone_pass_book1_vs_f64_oracle(pkg, orc, gpu, book1):
    hs, scene = book1
    lone_pass_vs_oracle(pkg, orc, gpu, hs, scene, hs.camera(64 / 40), 64, 40, 3e-5, 0.003, 1e-6)


def test_lone_pass_cornell_vs_f64_oracle(pkg, orc, gpu, cornell):
    hs, scene = cornell
    lone_pass_vs_oracle(pkg, orc, gpu, hs, scene, hs.camera(1.0), 40, 40, 1.2e-4, 0.015, 2.5e-6)


def test_device_std_error_matches_the_fixture(pkg, gpu, cornell):
    """C4's light_edge tile at the fixture's 1000 spp, rendered as a one-tile shard with sq_sum: the standard error of every pixel mean
    from the device's second moments against the oracle's (tests/golden/crops_C4.npz, per-sample std / sqrt(spp))."""
    import crops as K
    from conftest import record_metric
    cfg = K.CONFIGS["C4"]
    g = K.load_golden("C4")
    ti, n_tiles = K.tile_index("C4", "light_edge")
    hs, scene = cornell
    cam = hs.camera(cfg["width"] / cfg["height"])
    prm = pkg.make_params(cfg["width"], cfg["height"], cfg["spp"], max_depth=50, seed=cfg["seed"], tile_size=K.TILE, shard_index=ti, shard_count=n_tiles)
    n = pkg.output_floats(prm)
    rgb, sq, _ = gpu.render_pass(scene, cam, prm, 0, cfg["spp"], False, None, np.zeros(n, dtype=np.float32))
    S = rgb[:K.TILE * K.TILE * 3].reshape(K.TILE, K.TILE, 3)
    Q = sq[:K.TILE * K.TILE * 3].reshape(K.TILE, K.TILE, 3)
    se = pkg.std_error(S, Q, cfg["spp"], 1)
    ref = g["light_edge__se"].astype(np.float64)
    mean = S.astype(np.float64) / cfg["spp"]
    # channels whose SE is not rounding-dominated: a spread of at least 1e-3 of the mean and above f32's resolution of Q
    ok = (ref > 1e-3 * np.maximum(mean, 1e-6)) & (ref > 1e-5)
    assert ok.mean() > 0.5
    r = se[ok] / ref[ok]
    med = float(np.median(r))
    spread = float(np.percentile(r, 90) - np.percentile(r, 10))
    record_metric(config="progressive", crop="C4_light_edge_se", median_ratio=med, p10_p90=spread, used=float(ok.mean()))
    # the same seed: the device and the oracle see the same samples, so the two estimates agree to f32 rounding (measured on MI355X:
    # median ratio 1 - 8e-6, 10th-90th percentile spread 1.8e-5; the bounds are twice the spread)
    assert abs(med - 1.0) <= 4e-5, med
    assert spread <= 4e-5, spread


def test_bad_passes_are_refused_untouched(pkg, gpu, book1):
    import torch
    from test_progressive_host import refusals
    A, lib = pkg._abi, pkg.lib()
    hs, scene = book1
    cam = hs.camera(64 / 40)
    for prm, o, word in refusals(pkg):
        if prm.width < 2:
            continue
        n = pkg.output_floats(prm)
        buf, sq = np.full(n, 3.0, dtype=np.float32), np.full(n, 5.0, dtype=np.float32)
        fp = C.POINTER(C.c_float)
        st = A.RtStats()
        assert lib.rt_render_pass(gpu._h, scene._h, C.byref(cam), C.byref(prm), C.byref(o), buf.ctypes.data_as(fp), sq.ctypes.data_as(fp), C.byref(st)) == A.RT_ERR_INVALID
        assert word in lib.rt_last_error(gpu._h), word
        assert (buf == 3.0).all() and (sq == 5.0).all()
        t = torch.full((n,), 3.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert lib.rt_render_pass_device(gpu._h, scene._h, C.byref(cam), C.byref(prm), C.byref(o), C.c_void_p(t.data_ptr()), None, C.byref(st)) == A.RT_ERR_INVALID
        assert word in lib.rt_last_error(gpu._h), word
        assert (t.cpu().numpy() == 3.0).all()
    with pytest.raises(ValueError):
        gpu.render_pass(scene, cam, pkg.make_params(64, 40, 8), 0, 40, True, None, None)      # ACCUMULATE needs sums to add to
    # the context renders on after a refusal
    img, _ = gpu.render(scene, cam, pkg.make_params(64, 40, 2))
    assert np.isfinite(img).all() and img.mean() > 0


def test_progressive_checkpoint_round_trip(pkg, tmp_path):
    hs = pkg.HostScene("book1", 1)
    cam = hs.camera(64 / 40)
    prm = pkg.make_params(64, 40, N, seed=3)
    ctx = pkg.Context(0)
    scene = ctx.upload(hs.desc)
    one, _ = ctx.render(scene, cam, prm)
    _, sq1, _ = ctx.render_pass(scene, cam, prm, 0, N, False, None, np.zeros(pkg.output_floats(prm), dtype=np.float32))
    prog = pkg.Progressive(ctx, scene, cam, prm, N)
    for n in (1, 7, 5):
        prog.step(n)
    assert prog.samples_done == 13 and not prog.done
    path = tmp_path / "frame.npz"
    prog.save(path)
    del prog
    scene.close()
    ctx.close()
    ctx2 = pkg.Context(0)
    scene2 = ctx2.upload(hs.desc)
    other = pkg.make_params(64, 40, N, seed=4)
    with pytest.raises(ValueError, match="seed"):
        pkg.Progressive.load(path, ctx2, scene2, cam, params=other)
    with pytest.raises(ValueError, match="camera"):
        pkg.Progressive.load(path, ctx2, scene2, hs.camera(1.0))
    hs2 = pkg.HostScene("book1", 2)
    with pytest.raises(ValueError, match="scene"):
        pkg.Progressive.load(path, ctx2, ctx2.upload(hs2.desc), cam)
    prog2 = pkg.Progressive.load(path, ctx2, scene2, cam, params=prm)
    assert prog2.samples_done == 13
    seen = []
    assert prog2.run(pass_samples=9, callback=lambda p, st: seen.append(p.samples_done)) == N
    assert seen == [22, 31, 40] and prog2.done and prog2.step(4) is None
    assert np.array_equal(prog2.rgb_sum(), one)
    assert np.array_equal(prog2.sq_sum(), sq1)
    assert np.array_equal(prog2.rgb8(), pkg.tonemap(one, N))
    se = prog2.std_error()
    assert np.isfinite(se).all() and (se >= 0).all() and 0 < prog2.relative_error() < 1
    # stop criteria: a sample target, a noise target
    prog3 = pkg.Progressive(ctx2, scene2, cam, prm, N)
    assert prog3.run(pass_samples=4, until=12) == 12
    assert prog3.run(pass_samples=4, rel_se=1e9) == 16
    scene2.close()
    ctx2.close()
