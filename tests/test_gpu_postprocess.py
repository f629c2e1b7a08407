"""The kernels that run after the fold, on synthetic buffers at the sizes where they can go wrong (tests/postprocess.py builds the cases,
tests/test_postprocess_host.py shows the cases are what they claim): k_write_color / k_write_color_counts against write_color in f64,
k_select_* against select_reference from one wave to the scan's run of 15, k_untile against the slot map, k_list_check and the list pass
beyond one workgroup and slot 65535. Every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postprocess as PP  # noqa: E402
from conftest import record_metric  # noqa: E402
from test_gpu_adaptive import as_list, buffers, plain_passes, with_spp  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64            # sentinel elements behind every output buffer


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(n, dtype, fill):
    """A device buffer of n + GUARD elements, all `fill`; the kernels get the first n."""
    import torch
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


# ---- A. write_color -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wc_cases():
    return [(s, spp, PP.write_color_f64(s, spp)) for s, spp in PP.write_color_cases()]


def test_resolve_device_is_write_color_in_f64(gpu, wc_cases):
    """rt_resolve_device on the sums at which a byte changes, their neighbours, the specials and 200 000 random sums, for every spp: the
    bytes of write_color evaluated in f64 (main.rs:141-169), all of them. While the kernel evaluated in f32 it missed 1879 of the 14135
    boundary sums and 1 of the 2.2 million others, each by one."""
    import torch
    n_edge = 257 * 5                                                    # the boundary sums come first in every case
    wrong = wrong_edge = 0
    for sums, spp, want in wc_cases:
        h, w, _ = sums.shape
        src = dev(sums.reshape(-1))
        out = guarded(sums.size, torch.uint8, 0xA5)
        torch.cuda.synchronize()
        gpu.resolve_device(src.data_ptr(), w, h, spp, out.data_ptr())
        got = out.cpu().numpy()
        assert (got[sums.size:] == 0xA5).all(), spp
        assert np.array_equal(src.cpu().numpy().view(np.uint32), sums.reshape(-1).view(np.uint32))
        diff = got[:sums.size].astype(np.int64) - want.reshape(-1)
        print(f"spp {spp}: {int((diff != 0).sum())} of {diff.size} bytes differ, {int((diff[:n_edge] != 0).sum())} of them among the {n_edge} boundary sums, "
              f"max |difference| {int(np.abs(diff).max())}")
        wrong += int((diff != 0).sum())
        wrong_edge += int((diff[:n_edge] != 0).sum())
    record_metric(test="resolve_device_is_write_color_in_f64", bytes_wrong=wrong, boundary_bytes_wrong=wrong_edge)
    assert wrong == 0, (wrong, wrong_edge)


def test_resolve_counts_device_is_write_color_with_each_pixels_count(gpu, wc_cases):
    import torch
    for sums, _, _ in wc_cases:
        h, w, _ = sums.shape
        counts = PP.count_plane(h, w)
        want = PP.write_color_f64(sums, counts)
        out = guarded(sums.size, torch.uint8, 0xA5)
        gpu.resolve_counts_device(dev(sums.reshape(-1)), dev(counts.reshape(-1).view(np.int32)), w, h, out[:sums.size])
        got = out.cpu().numpy()
        assert (got[sums.size:] == 0xA5).all()
        got = got[:sums.size].reshape(sums.shape)
        assert np.array_equal(got, want), int((got != want).sum())
        assert (counts == 0).any() and (got[counts == 0] == 0).all()             # three zero bytes, whatever the sums hold (NaN and inf among them)


# ---- B. adaptive selection ----------------------------------------------------------------------------------------------------------------
def check_select(pkg, ctx, case):
    """One rt_adaptive_select call: the length and the list are the reference's, nothing is written behind the list, the inputs keep
    their bits. Returns the list's length."""
    import torch
    prm = pkg.make_params(**case.params)
    slots = case.counts.size
    ref = PP.reference_list(pkg, case)
    rgb, sq, counts = dev(case.rgb.reshape(-1)), dev(case.sq.reshape(-1)), dev(case.counts.view(np.int32))
    out = torch.full((slots,), -1, dtype=torch.int32, device="cuda")
    n = ctx.adaptive_select(prm, pkg.adaptive_options(*case.options), case.first_sample, case.frame_samples, rgb, sq, counts, out)
    got = out.cpu().numpy().view(np.uint32)
    assert n == ref.size, (case.name, n, ref.size)
    assert np.array_equal(got[:n], ref), case.name
    assert (got[n:] == PP.SENTINEL).all(), case.name
    for t, a in ((rgb, case.rgb), (sq, case.sq), (counts, case.counts)):
        assert np.array_equal(t.cpu().numpy().view(np.uint32).reshape(-1), a.view(np.uint32).reshape(-1)), case.name
    return n


@pytest.mark.parametrize("kw", PP.SELECT_SIZES + PP.SELECT_SHARDS, ids=PP.size_id)
def test_select_is_the_reference_at_every_size_and_pattern(pkg, gpu, kw):
    for case in PP.select_cases([kw]):
        check_select(pkg, gpu, case)


def test_select_on_the_benchmarked_frame(pkg, gpu):
    n = check_select(pkg, gpu, PP.bench_frame_case())                 # 15 000 waves: every thread of the scan owns a run of 15
    assert 0 < n < 960000


def test_select_scratch_is_reused_across_sizes(pkg):
    """One context, a large frame first: the masks and offsets of the later, smaller frames lie in scratch that still holds the larger
    frame's beyond their own n_waves."""
    ctx = pkg.Context(0)
    try:
        check_select(pkg, ctx, PP.bench_frame_case())
        for kw, pattern in [(PP.SELECT_SIZES[0], "everything"), (PP.SELECT_SIZES[9], "bernoulli_0.5"), (PP.SELECT_SIZES[2], "lane63"),
                            (PP.SELECT_SIZES[9], "alternate_waves")]:
            check_select(pkg, ctx, PP.select_case(kw, pattern, (60, PP.PATTERNS.index(pattern))))
    finally:
        ctx.close()
    assert [PP.size_id(PP.SELECT_SIZES[i]) for i in (0, 9, 2)] == ["2x2", "257x257", "8x8"]


def test_select_with_batch_means_of_16(pkg, gpu):
    for case in PP.select_m16_cases(pkg._abi.RT_FLAG_SAMPLE_BLOCKS):
        assert 0 < check_select(pkg, gpu, case) < case.counts.size


def test_select_on_the_knife_edge(pkg, gpu):
    for case in PP.knife_cases(pkg._abi.RT_FLAG_SAMPLE_BLOCKS):
        assert check_select(pkg, gpu, case) == int(case.want.sum()), case.name


def test_select_on_a_shard_without_tiles(pkg, gpu):
    """Shard 5 of 8 of a 16 x 16 frame with tiles of 8 owns none of the 4 tiles: 0 slots. Directly after a select that returned n > 0, the
    empty shard's select returns RT_OK and 0, not the earlier list's length, and touches none of its buffers."""
    import torch
    A = pkg._abi
    assert check_select(pkg, gpu, PP.select_case(PP.SELECT_SIZES[5], "everything", (70, 1))) == 256
    prm = pkg.make_params(16, 16, PP.FRAME, tile_size=8, shard_index=5, shard_count=8)
    assert pkg.output_floats(prm) == 0
    f = torch.full((1,), 3.5, dtype=torch.float32, device="cuda")
    g = torch.full((1,), 4.5, dtype=torch.float32, device="cuda")
    c = torch.full((1,), PP.FIRST, dtype=torch.int32, device="cuda")
    out = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = C.c_uint32(12345)
    opt = pkg.adaptive_options(*PP.OPTIONS)
    rc = pkg.lib().rt_adaptive_select(gpu._h, C.byref(prm), C.byref(opt), PP.FIRST, PP.FRAME, C.c_void_p(f.data_ptr()), C.c_void_p(g.data_ptr()),
                                      C.c_void_p(c.data_ptr()), C.c_void_p(out.data_ptr()), C.byref(n))
    assert rc == A.RT_OK
    assert n.value == 0, n.value
    assert f.item() == 3.5 and g.item() == 4.5 and c.item() == PP.FIRST and out.item() == -1


# ---- C. untile ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,tile,world", PP.UNTILE_SHAPES)
def test_untile_device_is_the_slot_map(pkg, gpu, w, h, tile, world):
    import torch
    A = pkg._abi
    prm0, g32, g8, want32, want8 = PP.untile_case(pkg, w, h, tile, world)
    n = w * h * 3
    for kind, g, want, dtype, fill in ((A.RT_OUT_RGB_SUM_F32, g32, want32, torch.float32, float(PP.FRAME_SENTINEL_F32)),
                                       (A.RT_OUT_RGB8, g8, want8, torch.uint8, int(PP.FRAME_SENTINEL_U8))):
        src = dev(g.reshape(-1))
        frame = guarded(n, dtype, fill)
        torch.cuda.synchronize()
        gpu.untile_device(prm0, kind, src.data_ptr(), frame.data_ptr())
        got = frame.cpu().numpy()
        assert (got[n:] == fill).all()
        assert np.array_equal(got[:n].reshape(h, w, 3), want), kind
        assert np.array_equal(src.cpu().numpy(), g.reshape(-1))
    assert np.array_equal(pkg.untile(prm0, g32.reshape(-1)), want32) and np.array_equal(pkg.untile_rgb8(prm0, g8.reshape(-1)), want8)


# ---- D. pixel lists -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def book1(pkg, gpu):
    hs = pkg.HostScene("book1", 1)
    return hs, gpu.upload(hs.desc)


def test_list_pass_and_refused_lists_beyond_one_workgroup(pkg, gpu, book1):
    """A list of 314 entries over a 66000-slot frame (the last entry is slot 65999): the listed pixels get the plain pass's bits and a
    count of 2, every other slot of the three buffers keeps its bits. Then lists whose fault sits on the boundary between two workgroups
    of k_list_check, or at the very end: refused with the reason, every buffer unchanged."""
    A = pkg._abi
    hs, scene = book1
    W, H = PP.LIST_FRAME
    slots = W * H
    prm = pkg.make_params(W, H, 1)
    cam = hs.camera(W / H)
    want_rgb, want_sq = plain_passes(pkg, gpu, scene, cam, prm, [(0, 2)], 2)
    rgb, sq, counts = buffers(pkg, prm)
    snap = lambda: [t.cpu().numpy().copy() for t in (rgb, sq, counts)]       # noqa: E731
    before = snap()
    listed = PP.list_pass_entries()
    lst = as_list(listed)
    st = gpu.render_pass_pixels(scene, cam, with_spp(pkg, prm, 2), 0, 2, False, lst, lst.numel(), rgb, sq, counts)
    assert st["samples"] == 2 * listed.size
    after = snap()
    on = np.zeros(slots, dtype=bool)
    on[listed] = True
    on3 = np.repeat(on, 3)
    assert np.array_equal(after[0][on3].view(np.uint32), want_rgb[on3].view(np.uint32))
    assert np.array_equal(after[1][on3].view(np.uint32), want_sq[on3].view(np.uint32))
    assert (after[2][on] == 2).all()
    for b, a, mask in zip(before, after, (~on3, ~on3, ~on)):
        assert np.array_equal(b[mask].view(np.uint32), a[mask].view(np.uint32))
    # refused lists on the same buffers: the counts are 0 except at the listed slots
    for entries, word in PP.refused_lists(slots, slots - 1):
        bad = as_list(entries)
        with pytest.raises(pkg.RtError) as e:
            gpu.render_pass_pixels(scene, cam, with_spp(pkg, prm, 2), 0, 2, False, bad, bad.numel(), rgb, sq, counts)
        assert e.value.code == A.RT_ERR_INVALID and word in str(e.value), (word, str(e.value))
        for b, a in zip(after, snap()):
            assert np.array_equal(b.view(np.uint8), a.view(np.uint8)), word
    # a clipped slot in the middle of an otherwise good list of more than 256 entries, on a shard with clipped edge tiles
    prm = pkg.make_params(70, 40, 1, tile_size=32, shard_index=1, shard_count=2)
    cam = hs.camera(70 / 40)
    _, _, ok = pkg.slot_pixels(prm)
    good = np.nonzero(ok)[0][::4]
    clipped = np.nonzero(~ok)[0]
    clipped = clipped[(clipped > good[150]) & (clipped < good[-1])][0]
    entries = np.sort(np.concatenate([good, [clipped]]))
    assert good.size > 256 and 150 < int(np.searchsorted(entries, clipped)) < entries.size - 1
    rgb, sq, counts = buffers(pkg, prm, fill=-3.25)
    before = snap()
    bad = as_list(entries)
    with pytest.raises(pkg.RtError) as e:
        gpu.render_pass_pixels(scene, cam, with_spp(pkg, prm, 2), 0, 2, False, bad, bad.numel(), rgb, sq, counts)
    assert e.value.code == A.RT_ERR_INVALID and "clipped" in str(e.value) and "ascending" not in str(e.value), str(e.value)
    for b, a in zip(before, snap()):
        assert np.array_equal(b.view(np.uint8), a.view(np.uint8))
