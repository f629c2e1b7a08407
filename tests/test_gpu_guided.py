"""The guided denoiser on the GPU (rt_denoise_guided_device, include/rt_hip.h "denoising, guided"): the f32 / binary16 kernels against
the numpy restatement (nlm_guided_reference, f64) on progressive and adaptive frames with device-rendered features, the cases whose
answer is exact, the step edge only the guide can see, what the call may and may not write, and the error of guided 16-spp tiles of the
benchmarked frames against their converged fixtures."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crops as K    # noqa: E402
import guided as G   # noqa: E402
from test_denoise_host import DENOISE_SPP, identity_cases, noisy_frame   # noqa: E402
from test_gpu_denoise import progressive_frame, window_range             # noqa: E402
from test_guided_host import CPU_RATIO, GUIDED_CROPS, any_guide, check_step_edge   # noqa: E402

pytestmark = pytest.mark.gpu

N_F = G.FEATURE_SAMPLES
OPTION_SETS = [dict(), dict(window_radius=3, patch_radius=1), dict(window_radius=10, patch_radius=4)]     # the last: the LDS maximum


@pytest.fixture(scope="module")
def book1(pkg, gpu):
    hs = pkg.HostScene("book1", 1)
    return hs, gpu.upload(hs.desc)


@pytest.fixture(scope="module")
def cornell(pkg, gpu):
    hs = pkg.HostScene("cornell", 0)
    return hs, gpu.upload(hs.desc)


def render_guide(pkg, ctx, scene, cam, params, n_f=N_F):
    from importlib import import_module
    return import_module("ray_tracer_archive_amd.denoise").render_guide(ctx, scene, cam, params, n_f)


def host_planes(guide, H, W):
    """The guide's device planes as nlm_guided_reference's keyword arguments."""
    return dict(albedo_sum=guide["albedo"].cpu().numpy().reshape(H, W, 3), normal_sum=guide["normal"].cpu().numpy().reshape(H, W, 3),
                depth_sum=guide["depth"].cpu().numpy().reshape(H, W), hits=guide["hits"].cpu().numpy().view(np.uint32).reshape(H, W))


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).reshape(-1).cuda()


def device_planes(planes):
    return dict(albedo=dev(planes["albedo_sum"]), normal=dev(planes["normal_sum"]), depth=dev(planes["depth_sum"]), hits=dev(planes["hits"]))


def check_against_reference(pkg, out, S, Q, counts_or_n, m, planes, opts, label, n_f=N_F):
    """rt_denoise_device's bound ("Denoising"): |out - ref| <= 2e-3 (max - min of u over the pixel's window) + 1e-6 |ref| per
    channel; invalid pixels exact."""
    from conftest import record_metric
    ref = pkg.nlm_guided_reference(S, Q, counts_or_n, m, n_f, **planes, **opts)
    u, v, valid = pkg.nlm_prepare(S, Q, counts_or_n, m)
    valid = valid & pkg.guide_prepare(n_f, **planes)[1]
    r = opts.get("window_radius", 0) or 10
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert np.array_equal(out[~valid], u[~valid], equal_nan=True)                  # copied through, bit for bit
    rng = window_range(u, valid, r)
    err = np.abs(out.astype(np.float64) - ref)[valid]
    bound = (2e-3 * rng + 1e-6 * np.abs(ref))[valid]
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    record_metric(config="denoise_guided", case=label, options=opts, max_abs_err=float(err.max()), worst_err_over_bound=worst, valid=float(valid.mean()))
    print(f"guided denoise vs reference {label} {opts}: max |err| {float(err.max()):.3g}, worst err/bound {worst:.3g}, valid {valid.mean():.3f}")
    assert (err <= bound).all(), (label, opts, worst)
    return valid


@pytest.mark.parametrize("scene_name,W,H", [("book1", 64, 40), ("book1", 70, 45), ("cornell", 40, 40)])
def test_kernel_matches_the_restatement_on_progressive_frames(pkg, gpu, book1, cornell, scene_name, W, H):
    """70 x 45: 3 x 2 tiles with clipped edges."""
    prog = progressive_frame(pkg, gpu, book1 if scene_name == "book1" else cornell, W, H)
    S, Q = prog.rgb_sum(), prog.sq_sum()
    guide = render_guide(pkg, gpu, prog.scene, prog.cam, prog.params)
    planes = host_planes(guide, H, W)
    assert planes["hits"].max() == N_F
    for opts in OPTION_SETS:
        out = gpu.denoise_guided(prog._rgb, prog._sq, W, H, samples=prog.samples_done, options=pkg.denoise_options(samples_per_item=prog.samples_per_item, **opts),
                                 **guide).cpu().numpy().reshape(H, W, 3)
        check_against_reference(pkg, out, S, Q, prog.samples_done, prog.samples_per_item, planes, opts, f"{scene_name}_{W}x{H}")
        # the Python path: the same feature pass, the same call
        assert np.array_equal(prog.denoised(feature_samples=N_F, **opts), out)
    # feature_samples = 0 is the plain filter, bit for bit
    plain = gpu.denoise(prog._rgb, prog._sq, W, H, samples=prog.samples_done, options=pkg.denoise_options(samples_per_item=prog.samples_per_item))
    assert np.array_equal(prog.denoised(feature_samples=0), plain.cpu().numpy().reshape(H, W, 3)) and np.array_equal(prog.denoised(), prog.denoised(feature_samples=0))
    assert not np.array_equal(prog.denoised(feature_samples=N_F), prog.denoised())


def test_kernel_matches_the_restatement_on_an_adaptive_frame_with_invalid_pixels(pkg, gpu, cornell):
    """Mixed counts from an adaptive run; some pixels hold no sample, some feature pixels are invalid (a non-finite normal sum, more hits
    than feature samples): all of them are copied through and are nobody's neighbour."""
    import torch
    hs, scene = cornell
    W = H = 40
    cam, prm = hs.camera(1.0), pkg.make_params(W, H, 64, max_depth=50, seed=3)
    ada = pkg.Adaptive(gpu, scene, cam, prm, frame_samples=64, min_samples=8, rel_error=0.05)
    ada.run(pass_samples=8)
    whole = ada.denoised(feature_samples=N_F)
    guide = render_guide(pkg, gpu, scene, cam, prm)
    opts0 = pkg.denoise_options(samples_per_item=ada.samples_per_item)
    assert np.array_equal(whole, gpu.denoise_guided(ada._rgb, ada._sq, W, H, counts=ada._counts, options=opts0, **guide).cpu().numpy().reshape(H, W, 3))
    assert np.array_equal(ada.denoised(feature_samples=0), gpu.denoise(ada._rgb, ada._sq, W, H, counts=ada._counts, options=opts0).cpu().numpy().reshape(H, W, 3))
    none = torch.tensor([12 * W + 30, 12 * W + 31, 33 * W + 17], device=ada._rgb.device)
    ada._rgb.view(-1, 3)[none] = 0; ada._sq.view(-1, 3)[none] = 0; ada._counts[none] = 0
    guide["normal"].view(-1, 3)[5 * W + 5, 1] = float("nan"); guide["normal"].view(-1, 3)[20 * W + 21] = float("inf")
    guide["hits"][31 * W + 8] = N_F + 1; guide["hits"][0] = 1 << 30
    torch.cuda.synchronize()
    counts = ada.counts()
    S, Q, planes = ada.rgb_sum(), ada.sq_sum(), host_planes(guide, H, W)
    assert len(np.unique(counts)) >= 3
    for opts in OPTION_SETS:
        out = gpu.denoise_guided(ada._rgb, ada._sq, W, H, counts=ada._counts, options=pkg.denoise_options(samples_per_item=ada.samples_per_item, **opts),
                                 **guide).cpu().numpy().reshape(H, W, 3)
        valid = check_against_reference(pkg, out, S, Q, counts, ada.samples_per_item, planes, opts, "cornell_adaptive_40x40")
        assert (~valid).sum() >= 7 and not valid[5, 5] and not valid[20, 21] and not valid[31, 8] and not valid[0, 0] and not valid[12, 30]


@pytest.mark.parametrize("case", [0, 1])
def test_exact_cases_come_back_bit_for_bit_with_any_guide(pkg, gpu, case):
    name, S, Q, n = identity_cases()[case]
    H, W = S.shape[:2]
    u = pkg.nlm_prepare(S, Q, n, 1)[0]
    g = device_planes(any_guide(H, W))
    for opts in OPTION_SETS:
        out = gpu.denoise_guided(dev(S), dev(Q), W, H, N_F, samples=n, options=pkg.denoise_options(**opts), **g).cpu().numpy().reshape(H, W, 3)
        assert np.array_equal(out, u), (name, opts, float(np.abs(out - u).max()))


def test_constant_guide_and_the_step_edge(pkg, gpu):
    from importlib import import_module
    # a guide that is constant over the frame: g = 0, the plain filter — within the bound of rt_denoise_device's output
    S, Q = noisy_frame()
    H, W = S.shape[:2]
    opts = dict(window_radius=4, patch_radius=2)
    o = pkg.denoise_options(**opts)
    plain = gpu.denoise(dev(S), dev(Q), W, H, samples=16, options=o).cpu().numpy().reshape(H, W, 3)
    const = dict(albedo_sum=np.full((H, W, 3), 1.7, np.float32), normal_sum=np.full((H, W, 3), -0.9, np.float32), depth_sum=np.full((H, W), 31.0, np.float32),
                 hits=np.full((H, W), 3, np.uint32))
    out = gpu.denoise_guided(dev(S), dev(Q), W, H, N_F, samples=16, options=o, **device_planes(const)).cpu().numpy().reshape(H, W, 3)
    u, v, valid = pkg.nlm_prepare(S, Q, 16, 1)
    bound = 2e-3 * window_range(u, valid, 4) + 1e-6 * np.abs(plain)
    print(f"constant guide against rt_denoise_device: bit-equal {np.array_equal(out, plain)}, max |diff| {np.abs(out - plain).max():.3g}")
    assert (np.abs(out.astype(np.float64) - plain) <= bound).all()
    # the step edge (tests/test_guided_host.py): the same assertions on the device
    sigma = import_module("ray_tracer_archive_amd.denoise").GUIDE_DEFAULTS["sigma_albedo"]
    S, Q, n, albedo, n_f = G.step_edge_frame(sigma)
    H, W = S.shape[:2]
    u = pkg.nlm_prepare(S, Q, n, 1)[0]
    plain = gpu.denoise(dev(S), dev(Q), W, H, samples=n).cpu().numpy().reshape(H, W, 3)
    guided = gpu.denoise_guided(dev(S), dev(Q), W, H, n_f, albedo=dev(albedo), samples=n).cpu().numpy().reshape(H, W, 3)
    check_step_edge(plain.astype(np.float64), guided.astype(np.float64), u.astype(np.float64), W)


def test_result_does_not_depend_on_where_tiles_fall_or_on_the_call(pkg, gpu, book1):
    """A frame and the same frame with 13 rows and 5 columns of other pixels in front of it: the same bits, though the pixels sit in other
    workgroups at other positions; and two identical calls give identical bytes."""
    W, H = 70, 40
    prog = progressive_frame(pkg, gpu, book1, W, H)
    S, Q = prog.rgb_sum(), prog.sq_sum()
    planes = host_planes(render_guide(pkg, gpu, prog.scene, prog.cam, prog.params), H, W)
    opts = pkg.denoise_options(window_radius=4, patch_radius=2)
    a = gpu.denoise_guided(dev(S), dev(Q), W, H, N_F, samples=16, options=opts, **device_planes(planes)).cpu().numpy().reshape(H, W, 3)
    again = gpu.denoise_guided(dev(S), dev(Q), W, H, N_F, samples=16, options=opts, **device_planes(planes)).cpu().numpy().reshape(H, W, 3)
    assert a.tobytes() == again.tobytes()
    py, px = 13, 5

    def shifted(p):
        q = np.zeros((H + py, W + px) + p.shape[2:], dtype=p.dtype)
        q[py:, px:] = p
        return q
    cnt = shifted(np.full((H, W), 16, dtype=np.int32))                                    # the padding holds no sample: nobody's neighbour
    b = gpu.denoise_guided(dev(shifted(S)), dev(shifted(Q)), W + px, H + py, N_F, counts=dev(cnt), options=opts,
                           **device_planes({k: shifted(v) for k, v in planes.items()})).cpu().numpy().reshape(H + py, W + px, 3)
    assert np.array_equal(b[py:, px:], a)
    assert (b[:py] == 0).all() and (b[:, :px] == 0).all()


def test_buffers_guards_refusals_and_the_plain_filter_beside_it(pkg, gpu, book1):
    import torch
    A, lib = pkg._abi, pkg.lib()
    W, H = 70, 40
    prog = progressive_frame(pkg, gpu, book1, W, H)
    guide = render_guide(pkg, gpu, prog.scene, prog.cam, prog.params)
    n, PAD = W * H * 3, 64
    plain_before = gpu.denoise(prog._rgb, prog._sq, W, H, samples=16).cpu().numpy()

    def guarded(t, word):
        room = torch.full((t.numel() + 2 * PAD,), word, dtype=t.dtype, device="cuda")
        room[PAD:PAD + t.numel()] = t
        return room, room[PAD:PAD + t.numel()]
    counts = torch.full((W * H,), 16, dtype=torch.int32, device="cuda"); counts[::7] = 8
    inputs = {k: guarded(t, w) for k, t, w in (("rgb", prog._rgb, -7.5), ("sq", prog._sq, -7.5), ("counts", counts, 12345), ("albedo", guide["albedo"], -7.5),
                                               ("normal", guide["normal"], -7.5), ("depth", guide["depth"], -7.5), ("hits", guide["hits"], 12345))}
    before = {k: room.cpu().numpy().copy() for k, (room, _) in inputs.items()}
    out_room = torch.full((n + 2 * PAD,), -123.25, dtype=torch.float32, device="cuda")
    v = {k: view for k, (_, view) in inputs.items()}
    out = gpu.denoise_guided(v["rgb"], v["sq"], W, H, N_F, v["albedo"], v["normal"], v["depth"], v["hits"], counts=v["counts"], out=out_room[PAD:PAD + n])
    host = out_room.cpu().numpy()
    assert out.data_ptr() == out_room[PAD:].data_ptr()
    assert (host[:PAD] == -123.25).all() and (host[PAD + n:] == -123.25).all() and np.isfinite(host[PAD:PAD + n]).all() and not (host[PAD:PAD + n] == -123.25).any()
    for k, (room, _) in inputs.items():
        assert np.array_equal(room.cpu().numpy(), before[k]), k
    uniform = gpu.denoise_guided(v["rgb"], v["sq"], W, H, N_F, v["albedo"], v["normal"], v["depth"], v["hits"], samples=16).cpu().numpy()
    assert not np.array_equal(uniform, host[PAD:PAD + n])                                   # the counts are read
    only_albedo = gpu.denoise_guided(v["rgb"], v["sq"], W, H, N_F, albedo=v["albedo"], samples=16).cpu().numpy()
    assert not np.array_equal(only_albedo, uniform) and not np.array_equal(only_albedo, plain_before)      # every plane is read
    # refused calls leave mean_out as it is
    keep = torch.full((n,), 9.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    vp = C.c_void_p
    ptr = {k: t.data_ptr() for k, t in v.items()}
    good_o, good_g = pkg.denoise_options(), pkg.denoise_guide(N_F, ptr["albedo"], ptr["normal"], ptr["depth"], ptr["hits"])

    def call(o=good_o, g=good_g, rgb=ptr["rgb"], sq=ptr["sq"], samples=16, dst=keep.data_ptr(), w=W):
        return lib.rt_denoise_guided_device(gpu._h, C.byref(o) if o is not None else None, C.byref(g) if g is not None else None, w, H, vp(rgb) if rgb else None,
                                            vp(sq) if sq else None, samples, None, vp(dst) if dst else None)
    short = pkg.denoise_guide(N_F, ptr["albedo"]); short.struct_bytes = 8
    refused = [(dict(o=pkg.denoise_options(window_radius=11)), b"window_radius"), (dict(o=pkg.denoise_options(strength=-1.0)), b"strength"),
               (dict(g=pkg.denoise_guide(N_F, ptr["albedo"], sigma_albedo=-1.0)), b"sigma_albedo"), (dict(g=pkg.denoise_guide(N_F, ptr["albedo"], sigma_normal=float("nan"))), b"sigma_normal"),
               (dict(g=pkg.denoise_guide(N_F, ptr["albedo"], sigma_depth=1e-60)), b"sigma_depth"), (dict(g=short), b"struct_bytes"),
               (dict(g=pkg.denoise_guide(0, ptr["albedo"])), b"feature_samples"), (dict(g=pkg.denoise_guide(N_F, hits=ptr["hits"])), b"rt_denoise_device"),
               (dict(g=pkg.denoise_guide(N_F, depth=ptr["depth"])), b"hits"), (dict(g=None), b"guide"), (dict(rgb=None), b"null"), (dict(sq=None), b"null"),
               (dict(dst=None), b"null"), (dict(samples=0), b"samples"), (dict(w=0), b"size")]
    refused += [(dict(dst=ptr[k]), b"input") for k in ("rgb", "sq", "albedo", "normal", "depth", "hits")]
    for kw, word in refused:
        assert call(**kw) == A.RT_ERR_INVALID, word
        assert word in lib.rt_last_error(gpu._h), (word, lib.rt_last_error(gpu._h))
    assert (keep.cpu().numpy() == 9.5).all()
    for k, (room, _) in inputs.items():
        assert np.array_equal(room.cpu().numpy(), before[k]), k
    # the context filters on after a refusal, and the plain filter beside it returns what it returned before
    assert call() == A.RT_OK and np.array_equal(keep.cpu().numpy(), uniform)
    assert np.array_equal(gpu.denoise(prog._rgb, prog._sq, W, H, samples=16).cpu().numpy(), plain_before)


@pytest.mark.parametrize("name,crop", GUIDED_CROPS)
def test_guided_filter_reduces_error_on_the_device(pkg, gpu, tmp_path, name, crop):
    """The crop's tile as a one-tile shard at 16 spp with sq_sum and a 4-sample feature pass through the same sharding, filtered as a
    64 x 64 frame: MSE against the converged fixture, at most min(1, 2 x the CPU restatement's ratio)."""
    import torch
    from conftest import record_metric
    cfg = K.CONFIGS[name]
    truth = K.load_golden(name)[crop] / cfg["spp"]
    ti, n_tiles = K.tile_index(name, crop)
    hs = K.host_scene(pkg, name, tmp_path)
    scene = gpu.upload(hs.desc)
    cam = hs.camera(cfg["width"] / cfg["height"])
    prm = pkg.make_params(cfg["width"], cfg["height"], DENOISE_SPP, max_depth=50, seed=cfg["seed"], tile_size=K.TILE, shard_index=ti, shard_count=n_tiles)
    rgb, sq, _ = gpu.render_pass(scene, cam, prm, 0, DENOISE_SPP, False, None, np.zeros(pkg.output_floats(prm), dtype=np.float32))
    fprm = pkg.make_params(cfg["width"], cfg["height"], N_F, max_depth=50, seed=cfg["seed"], tile_size=K.TILE, shard_index=ti, shard_count=n_tiles)
    albedo, normal, depth, hits = gpu.render_features(scene, cam, fprm)
    scene.close()
    px = K.TILE * K.TILE
    S, Q = np.ascontiguousarray(rgb[:3 * px]), np.ascontiguousarray(sq[:3 * px])
    out = gpu.denoise_guided(torch.from_numpy(S).cuda(), torch.from_numpy(Q).cuda(), K.TILE, K.TILE, N_F, albedo[:3 * px].clone(), normal[:3 * px].clone(),
                             depth[:px].clone(), hits[:px].clone(), samples=DENOISE_SPP,
                             options=pkg.denoise_options(samples_per_item=pkg.pass_check(prm, 0, DENOISE_SPP))).cpu().numpy().reshape(K.TILE, K.TILE, 3)
    raw = S.reshape(K.TILE, K.TILE, 3).astype(np.float64) / DENOISE_SPP
    mse_raw, mse_out = float(np.mean((raw - truth) ** 2)), float(np.mean((out.astype(np.float64) - truth) ** 2))
    ratio = mse_out / mse_raw
    record_metric(config="denoise_guided", crop=f"{name}_{crop}", mse_raw=mse_raw, mse_filtered=mse_out, ratio=ratio)
    print(f"guided denoise on device {name}/{crop}: raw MSE {mse_raw:.6g}, filtered MSE {mse_out:.6g}, ratio {ratio:.4f}")
    assert ratio <= min(1.0, 2.0 * CPU_RATIO[(name, crop)]), ratio


def test_a_sharded_progressive_frame_untiles_its_feature_planes(pkg, gpu, book1):
    hs, scene = book1
    W, H = 64, 40
    sh = pkg.Progressive(gpu, scene, hs.camera(W / H), pkg.make_params(W, H, 16, max_depth=50, seed=3, tile_size=16, shard_index=1, shard_count=3), frame_samples=16)
    sh.run(pass_samples=16)
    opts = dict(window_radius=3, patch_radius=1)
    d = sh.denoised(feature_samples=N_F, **opts)
    mine = sh.rgb_sum().any(axis=2)
    assert d.shape == (H, W, 3) and (d[~mine] == 0).all() and np.isfinite(d).all() and d[mine].max() > 0
    # the untiled planes are the full frame's own: the same pixels of an unsharded feature pass
    full = host_planes(render_guide(pkg, gpu, scene, sh.cam, pkg.make_params(W, H, 16, max_depth=50, seed=3)), H, W)
    tiled = host_planes(render_guide(pkg, gpu, scene, sh.cam, sh.params), H, W)
    for k in full:
        assert np.array_equal(tiled[k][mine], full[k][mine]), k
    cnt = np.where(mine, 16, 0).astype(np.int32)
    ref = gpu.denoise_guided(dev(sh.rgb_sum()), dev(sh.sq_sum()), W, H, N_F, counts=dev(cnt), options=pkg.denoise_options(samples_per_item=sh.samples_per_item, **opts),
                             **device_planes(tiled)).cpu().numpy().reshape(H, W, 3)
    assert np.array_equal(d, ref)
