"""Adaptive sampling on the GPU (include/rt_hip.h, "adaptive sampling"): a pass over a pixel list leaves, for every listed pixel, the bits
rt_render_pass leaves, in every layout and with every flag; an adaptive frame's pixels hold exactly the sums of a plain render at their
own count; the device's active list is the numpy restatement's; unlisted pixels and refused lists leave every buffer untouched; a
checkpoint resumes bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def with_spp(pkg, prm, spp):
    p = pkg._abi.RtParams.from_buffer_copy(prm)
    p.samples_per_pixel = spp
    return p


def plain_passes(pkg, gpu, scene, cam, prm, splits, frame):
    """rt_render_pass_device over `splits` (the first overwrites): flat (rgb, sq)."""
    import torch
    n = pkg.output_floats(prm)
    rgb, sq = torch.zeros(n, dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.float32, device="cuda")
    for i, (a, b) in enumerate(splits):
        gpu.render_pass(scene, cam, with_spp(pkg, prm, b - a), a, frame, i > 0, rgb, sq)
    return rgb.cpu().numpy(), sq.cpu().numpy()


def buffers(pkg, prm, fill=7.0, count=0):
    import torch
    slots = pkg.output_floats(prm) // 3
    rgb = torch.full((3 * slots,), fill, dtype=torch.float32, device="cuda")
    sq = torch.full((3 * slots,), fill, dtype=torch.float32, device="cuda")
    counts = torch.full((slots,), count, dtype=torch.int32, device="cuda")
    return rgb, sq, counts


def as_list(slots_np):
    import torch
    return torch.from_numpy(np.ascontiguousarray(slots_np, dtype=np.int64).astype(np.int32)).cuda()


@pytest.fixture(scope="module")
def book1(pkg, gpu):
    hs = pkg.HostScene("book1", 1)
    return hs, gpu.upload(hs.desc)


@pytest.fixture(scope="module")
def cornell(pkg, gpu):
    hs = pkg.HostScene("cornell", 0)
    return hs, gpu.upload(hs.desc)


def check_all_pixel_list(pkg, gpu, scene, cam, prm, splits):
    frame = splits[-1][1]
    want_rgb, want_sq = plain_passes(pkg, gpu, scene, cam, prm, splits, frame)
    _, _, ok = pkg.slot_pixels(prm)
    ok3 = np.repeat(ok, 3)
    rgb, sq, counts = buffers(pkg, prm)
    lst = as_list(np.nonzero(ok)[0])
    for i, (a, b) in enumerate(splits):
        st = gpu.render_pass_pixels(scene, cam, with_spp(pkg, prm, b - a), a, frame, i > 0, lst, lst.numel(), rgb, sq, counts)
        assert st["samples"] == lst.numel() * (b - a)
    rgb, sq, c = rgb.cpu().numpy(), sq.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(rgb[ok3], want_rgb[ok3]), float(np.abs(rgb[ok3] - want_rgb[ok3]).max())
    assert np.array_equal(sq[ok3], want_sq[ok3])
    assert (c[ok] == frame).all() and (c[~ok] == 0).all()
    assert (rgb[~ok3] == 7.0).all() and (sq[~ok3] == 7.0).all()          # clipped slots: not written (no shard-wide memset)


def test_all_pixel_list_pass_is_the_plain_pass(pkg, gpu, book1, cornell):
    A = pkg._abi
    hs, scene = book1
    cam = hs.camera(64 / 40)
    check_all_pixel_list(pkg, gpu, scene, cam, pkg.make_params(64, 40, 1), [(0, 3), (3, 20)])
    check_all_pixel_list(pkg, gpu, scene, cam, pkg.make_params(64, 40, 1, flags=A.RT_FLAG_SAMPLE_BLOCKS), [(0, 16), (16, 40)])
    check_all_pixel_list(pkg, gpu, scene, cam, pkg.make_params(64, 40, 1, flags=A.RT_FLAG_FUSED), [(0, 5), (5, 12)])
    check_all_pixel_list(pkg, gpu, scene, cam, pkg.make_params(64, 40, 1, tail_paths=1), [(0, 4), (4, 12)])
    cam70 = hs.camera(70 / 40)
    for si in (0, 1):                                                   # tile-compact shards with clipped edge tiles
        check_all_pixel_list(pkg, gpu, scene, cam70, pkg.make_params(70, 40, 1, tile_size=32, shard_index=si, shard_count=2), [(0, 2), (2, 9)])
    hc, sc = cornell
    camc = hc.camera(1.0)
    check_all_pixel_list(pkg, gpu, sc, camc, pkg.make_params(40, 40, 1), [(0, 8), (8, 24)])
    check_all_pixel_list(pkg, gpu, sc, camc, pkg.make_params(40, 40, 1, tile_size=16, shard_index=1, shard_count=3), [(0, 8), (8, 16)])


def test_adaptive_cornell_holds_plain_renders_at_every_count(pkg, gpu, cornell):
    import torch
    hs, scene = cornell
    W = H = 40
    cam = hs.camera(1.0)
    prm = pkg.make_params(W, H, 1)
    ada = pkg.Adaptive(gpu, scene, cam, prm, frame_samples=256, min_samples=32, rel_error=0.08)
    ada.run(pass_samples=16)
    counts, rgb, sq = ada.counts(), ada.rgb_sum(), ada.sq_sum()
    assert counts.max() == 256 and counts.min() >= 32 and (counts < 256).any(), np.unique(counts)
    assert ada.samples_traced == int(counts.astype(np.int64).sum()) < 256 * W * H
    img = ada.rgb8()
    for n in np.unique(counts):
        sel = counts == n
        want_rgb, want_sq = plain_passes(pkg, gpu, scene, cam, prm, [(0, int(n))], 256)
        want_rgb, want_sq = want_rgb.reshape(H, W, 3), want_sq.reshape(H, W, 3)
        assert np.array_equal(rgb[sel], want_rgb[sel]) and np.array_equal(sq[sel], want_sq[sel]), int(n)
        src = torch.from_numpy(want_rgb.reshape(-1)).cuda()
        out = torch.empty(W * H * 3, dtype=torch.uint8, device="cuda")
        gpu.resolve_device(src.data_ptr(), W, H, int(n), out.data_ptr())
        assert np.array_equal(img[sel], out.cpu().numpy().reshape(H, W, 3)[sel]), int(n)
    se = ada.std_error()
    assert np.isfinite(se).all() and (se >= 0).all()


@pytest.mark.parametrize("nan", [0, 1])
def test_device_list_is_the_reference_list(pkg, gpu, book1, nan):
    import torch
    hs, scene = book1
    for prm, cam in [(pkg.make_params(64, 40, 1, nan_policy=nan), hs.camera(64 / 40)),
                     (pkg.make_params(70, 40, 1, nan_policy=nan, tile_size=32, shard_index=1, shard_count=2), hs.camera(70 / 40))]:
        ada = pkg.Adaptive(gpu, scene, cam, prm, frame_samples=128, min_samples=8, rel_error=0.05, abs_error=1e-3)
        _, _, ok = pkg.slot_pixels(prm)
        for _ in range(4):
            ada.step(8)
            n = ada.select()
            ref = pkg.select_reference(ada._rgb.cpu().numpy(), ada._sq.cpu().numpy(), ada._counts.cpu().numpy().view(np.uint32), ada.samples_done,
                                       128, ada.samples_per_item, ada.options, valid=ok)
            assert np.array_equal(ada.active_list(), ref) and n == ref.size
        assert 0 < n < ok.sum()
        # non-finite sums are never converged: pixels that are still candidates (count == samples_done), converged ones first
        cnt = ada._counts.cpu().numpy().view(np.uint32)
        cand = np.nonzero(ok & (cnt == ada.samples_done))[0]
        conv = np.setdiff1d(cand, ref)
        bad = (conv if conv.size >= 5 else cand)[:5]
        assert bad.size == 5
        rgb = ada._rgb.clone()
        rgb[torch.from_numpy(bad * 3).cuda()] = float("nan")
        rgb[torch.from_numpy(bad * 3 + 1).cuda()] = float("inf")
        out = torch.zeros_like(ada._list)
        n = gpu.adaptive_select(ada.params, ada.options, ada.samples_done, 128, rgb, ada._sq, ada._counts, out)
        ref = pkg.select_reference(rgb.cpu().numpy(), ada._sq.cpu().numpy(), ada._counts.cpu().numpy().view(np.uint32), ada.samples_done, 128, 1,
                                   ada.options, valid=ok)
        assert np.array_equal(out[:n].cpu().numpy().view(np.uint32), ref) and set(bad.tolist()) <= set(ref.tolist())
        # a pixel that stopped earlier does not come back, whatever its sums hold
        stopped = np.nonzero(ok & (cnt < ada.samples_done))[0][:5]
        rgb[torch.from_numpy(stopped * 3).cuda()] = float("nan")
        n = gpu.adaptive_select(ada.params, ada.options, ada.samples_done, 128, rgb, ada._sq, ada._counts, out)
        assert not set(stopped.tolist()) & set(out[:n].cpu().numpy().tolist())


def test_unlisted_pixels_are_untouched(pkg, gpu, book1):
    import torch
    hs, scene = book1
    prm = pkg.make_params(70, 40, 1, tile_size=32, shard_index=1, shard_count=2)
    cam = hs.camera(70 / 40)
    _, _, ok = pkg.slot_pixels(prm)
    rgb, sq, counts = buffers(pkg, prm, fill=-3.25, count=12345)
    listed = np.nonzero(ok)[0][::3]
    counts[torch.from_numpy(listed).cuda()] = 0
    before = (rgb.cpu().numpy(), sq.cpu().numpy(), counts.cpu().numpy())
    lst = as_list(listed)
    gpu.render_pass_pixels(scene, cam, with_spp(pkg, prm, 4), 0, 16, False, lst, lst.numel(), rgb, sq, counts)
    after = (rgb.cpu().numpy(), sq.cpu().numpy(), counts.cpu().numpy())
    other = np.ones(ok.size, bool)
    other[listed] = False
    other3 = np.repeat(other, 3)
    assert other[~ok].all()                                            # the clipped slots are among the untouched
    for b, a, mask in zip(before, after, (other3, other3, other)):
        assert np.array_equal(b[mask].view(np.uint32), a[mask].view(np.uint32))
    assert (after[2][listed] == 4).all() and np.isfinite(after[0][np.repeat(~other, 3)]).all()
    want, _ = plain_passes(pkg, gpu, scene, cam, prm, [(0, 4)], 16)
    assert np.array_equal(after[0][np.repeat(~other, 3)], want[np.repeat(~other, 3)])
    # an empty list is a no-op
    st = gpu.render_pass_pixels(scene, cam, with_spp(pkg, prm, 4), 4, 16, True, lst, 0, rgb, sq, counts)
    assert st["samples"] == 0 and np.array_equal(counts.cpu().numpy(), after[2])
    # per-pixel write_color: a count of 0 is black, the others tone-map with their own count
    full = pkg.make_params(8, 4, 1)
    s = torch.full((8 * 4 * 3,), 2.0, dtype=torch.float32, device="cuda")
    c = torch.tensor([0, 1, 2, 8] * 8, dtype=torch.int32, device="cuda")
    out = torch.empty(8 * 4 * 3, dtype=torch.uint8, device="cuda")
    gpu.resolve_counts_device(s, c, full.width, full.height, out)
    got = out.cpu().numpy().reshape(-1, 3)[:4, 0].tolist()
    assert got[0] == 0 and got == [0] + [int(256 * min(np.float32(np.sqrt(np.float32(1 / k) * 2)), 0.999)) for k in (1, 2, 8)]


def test_refused_lists_leave_every_buffer_unchanged(pkg, gpu, book1):
    A = pkg._abi
    hs, scene = book1
    prm = pkg.make_params(64, 40, 1)
    cam = hs.camera(64 / 40)
    slots = 64 * 40
    rgb, sq, counts = buffers(pkg, prm, fill=1.5, count=0)
    counts[7] = 1
    snap = lambda: [t.cpu().numpy().copy() for t in (rgb, sq, counts)]       # noqa: E731
    before = snap()
    cases = [([5, 3, 9], 8, 16, "ascending"), ([3, 3, 9], 8, 16, "ascending"), ([2, 7, 9], 8, 16, "counts"), ([0, 1, slots], 8, 16, "slots"),
             ([0, 1, 2], 8, 4, "frame_samples")]                                       # bad options: the pass ends beyond frame_samples
    for entries, spp, frame, word in cases:
        lst = as_list(entries)
        with pytest.raises(pkg.RtError) as e:
            gpu.render_pass_pixels(scene, cam, with_spp(pkg, prm, spp), 0, frame, False, lst, lst.numel(), rgb, sq, counts)
        assert e.value.code == A.RT_ERR_INVALID and word in str(e.value), (word, str(e.value))
        for b, a in zip(before, snap()):
            assert np.array_equal(b.view(np.uint8), a.view(np.uint8)), word
    big = as_list(np.arange(slots))
    import ctypes as C
    opt = A.RtPassOptions(C.sizeof(A.RtPassOptions), 0, 0, 16)
    st = A.RtStats()
    lib = pkg.lib()
    rc = lib.rt_render_pass_pixels_device(gpu._h, scene._h, C.byref(cam), C.byref(with_spp(pkg, prm, 8)), C.byref(opt), C.c_void_p(big.data_ptr()), slots + 1,
                                          C.c_void_p(rgb.data_ptr()), C.c_void_p(sq.data_ptr()), C.c_void_p(counts.data_ptr()), C.byref(st))
    assert rc == A.RT_ERR_INVALID and "n_pixels" in lib.rt_last_error(gpu._h).decode()
    opt.flags = 2                                                                       # unknown RT_PASS_* bit
    rc = lib.rt_render_pass_pixels_device(gpu._h, scene._h, C.byref(cam), C.byref(with_spp(pkg, prm, 8)), C.byref(opt), C.c_void_p(big.data_ptr()), 3,
                                          C.c_void_p(rgb.data_ptr()), C.c_void_p(sq.data_ptr()), C.c_void_p(counts.data_ptr()), C.byref(st))
    assert rc == A.RT_ERR_INVALID
    for b, a in zip(before, snap()):
        assert np.array_equal(b.view(np.uint8), a.view(np.uint8))


def test_checkpoint_resumes_bit_for_bit(pkg, gpu, cornell, tmp_path):
    hs, scene = cornell
    cam = hs.camera(1.0)
    prm = pkg.make_params(40, 40, 1, tile_size=16, shard_index=0, shard_count=2)
    kw = dict(frame_samples=128, min_samples=16, rel_error=0.1)
    whole = pkg.Adaptive(gpu, scene, cam, prm, **kw)
    whole.run(pass_samples=16)
    part = pkg.Adaptive(gpu, scene, cam, prm, **kw)
    part.run(pass_samples=16, until=48)
    assert part.samples_done == 48
    part.save(tmp_path / "a.npz")
    with pytest.raises(ValueError):
        pkg.Adaptive.load(tmp_path / "a.npz", gpu, scene, hs.camera(1.2))
    with pytest.raises(ValueError):
        pkg.Progressive.load(tmp_path / "a.npz", gpu, scene, cam)            # not a uniform frame's checkpoint
    back = pkg.Adaptive.load(tmp_path / "a.npz", gpu, scene, cam)
    back.run(pass_samples=16)
    for f in ("counts", "rgb_sum", "sq_sum"):
        a, b = getattr(whole, f)(), getattr(back, f)()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f
    assert np.array_equal(whole.rgb8(), back.rgb8())
