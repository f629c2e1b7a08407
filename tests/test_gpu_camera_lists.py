"""Camera lists on the GPU (csrc/camera_lists.h, kernels.h RenderDev::cam_lists): camera rays are answered where they are made — k_generate
and k_shade's regeneration — from the list of their 8 x 8-pixel square instead of by a walk. With and without RT_FLAG_NO_CAMERA_LISTS a
render leaves the same bytes and the same segment and sample counts, in every form of a render: the wavefront kernels to the end
(tail_paths = 1), the hand-over to the per-path kernel, a shard, a progressive pair of passes, a pass over a pixel list — all with a pool
of a quarter of the work items, so that lineages hold 4 items and k_shade regenerates. The lists the device built are the host's, word for
word; a scene the lists do not serve builds none and renders what it rendered."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [("book1", 160, 100, 8), ("book1", 100, 52, 4), ("book1_sah", 96, 64, 4)]


@pytest.fixture(scope="module")
def scenes(pkg, gpu):
    out = {}
    for name in ("book1", "book1_sah"):
        hs = pkg.HostScene(name, 1)
        out[name] = (hs, gpu.upload(hs.desc))
    return out


def with_spp(pkg, prm, spp):
    p = pkg._abi.RtParams.from_buffer_copy(prm)
    p.samples_per_pixel = spp
    return p


def quarter_pool(items):
    """Pool slots for lineages of at least 4 work items: a pool is a multiple of 4096 slots (8 queues filled 512 at a time)."""
    return max(4096, items // 4 // 4096 * 4096)


def params(pkg, w, h, spp, off, **kw):
    """A pool of at most a quarter of the work items, so that k_shade regenerates; off: RT_FLAG_NO_CAMERA_LISTS."""
    return pkg.make_params(w, h, spp, flags=pkg._abi.RT_FLAG_NO_CAMERA_LISTS if off else 0, pool_slots=quarter_pool(w * h * spp // kw.get("shard_count", 1)), **kw)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("name,w,h,spp", SHAPES)
@pytest.mark.parametrize("tail_paths", [1, 0])
def test_render_is_the_same_with_and_without_lists(pkg, gpu, scenes, name, w, h, spp, tail_paths):
    hs, scene = scenes[name]
    cam = hs.camera(w / h)
    img_on, st_on = gpu.render(scene, cam, params(pkg, w, h, spp, False, tail_paths=tail_paths))
    built = gpu.camera_lists_last()
    img_off, st_off = gpu.render(scene, cam, params(pkg, w, h, spp, True, tail_paths=tail_paths))
    assert gpu.camera_lists_last() is None                       # the flag: no lists built
    assert st_on["bvh_in_lds"] == 1 and st_on["pool_slots"] * 4 <= w * h * spp
    if tail_paths == 1:
        assert st_on["drain_paths"] == 0 and st_on["extend_launches"] >= 4
    assert same_bits(img_on, img_off)
    assert st_on["segments"] == st_off["segments"] and st_on["samples"] == st_off["samples"] == w * h * spp
    # the device's lists are the host's
    want = pkg.camera_lists_host(hs.desc, cam, w, h)
    assert built is not None and want is not None and built.shape == want.shape and np.array_equal(built, want)
    # (a square of so small a frame covers much of the scene: some hold more than 16 candidates and are marked "walk", most do not)
    answered = want[:, 0] != pkg._abi.RT_CAMERA_LIST_WALK
    assert answered.mean() > 0.5 and want[answered, 0].max() >= 1


@pytest.mark.parametrize("name,w,h,spp", SHAPES)
def test_shard_is_the_same(pkg, gpu, scenes, name, w, h, spp):
    """Shard 1 of 2, tile-compact output: the lists are keyed by the global pixel."""
    hs, scene = scenes[name]
    cam = hs.camera(w / h)
    kw = dict(tile_size=32, shard_index=1, shard_count=2, tail_paths=1)
    on, st_on = gpu.render(scene, cam, params(pkg, w, h, spp, False, **kw))
    assert gpu.camera_lists_last() is not None
    off, st_off = gpu.render(scene, cam, params(pkg, w, h, spp, True, **kw))
    assert same_bits(on, off) and st_on["segments"] == st_off["segments"] and st_on["samples"] == st_off["samples"]


@pytest.mark.parametrize("name,w,h,spp", SHAPES)
def test_progressive_pair_is_the_same(pkg, gpu, scenes, name, w, h, spp):
    """Two passes, the second with RT_PASS_ACCUMULATE: the lists are rebuilt per pass."""
    hs, scene = scenes[name]
    cam = hs.camera(w / h)
    a = spp // 2
    out = {}
    for off in (False, True):
        prm = params(pkg, w, h, spp, off, tail_paths=1)
        rgb, sq, st0 = gpu.render_pass(scene, cam, with_spp(pkg, prm, a), 0, spp, False, None, np.zeros(pkg.output_floats(prm), np.float32))
        assert (gpu.camera_lists_last() is None) == off
        rgb, sq, st1 = gpu.render_pass(scene, cam, with_spp(pkg, prm, spp - a), a, spp, True, np.ascontiguousarray(rgb).reshape(-1), np.ascontiguousarray(sq).reshape(-1))
        out[off] = (rgb, sq, st0["segments"] + st1["segments"], st0["samples"] + st1["samples"])
    assert same_bits(out[False][0], out[True][0]) and same_bits(out[False][1], out[True][1])
    assert out[False][2:] == out[True][2:]
    one, _ = gpu.render(scene, cam, params(pkg, w, h, spp, False, tail_paths=1))
    assert same_bits(out[False][0], one)


@pytest.mark.parametrize("name,w,h,spp", SHAPES)
def test_pixel_list_pass_is_the_same(pkg, gpu, scenes, name, w, h, spp):
    """One pass over every third pixel (rt_render_pass_pixels_device): a wave of listed pixels spans several squares."""
    import torch
    hs, scene = scenes[name]
    cam = hs.camera(w / h)
    listed = np.arange(0, w * h, 3, dtype=np.int32)
    lst = torch.from_numpy(listed).cuda()
    out = {}
    for off in (False, True):
        prm = pkg.make_params(w, h, spp, flags=pkg._abi.RT_FLAG_NO_CAMERA_LISTS if off else 0, pool_slots=quarter_pool(len(listed) * spp), tail_paths=1)
        rgb = torch.full((3 * w * h,), 2.5, dtype=torch.float32, device="cuda")
        sq = torch.full((3 * w * h,), 2.5, dtype=torch.float32, device="cuda")
        counts = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        st = gpu.render_pass_pixels(scene, cam, prm, 0, spp, False, lst, lst.numel(), rgb, sq, counts)
        assert (gpu.camera_lists_last() is None) == off
        out[off] = (rgb.cpu().numpy(), sq.cpu().numpy(), counts.cpu().numpy(), st["segments"], st["samples"])
    for k in range(3):
        assert same_bits(out[False][k], out[True][k])
    assert out[False][3:] == out[True][3:] and out[False][4] == len(listed) * spp


def test_cornell_builds_no_lists(pkg, gpu):
    """A scene with rects and instances is not eligible: no lists, and the flag changes nothing."""
    hs = pkg.HostScene("cornell", 0)
    scene = gpu.upload(hs.desc)
    cam = hs.camera(1.0)
    on, st_on = gpu.render(scene, cam, pkg.make_params(48, 48, 4))
    assert gpu.camera_lists_last() is None
    off, st_off = gpu.render(scene, cam, pkg.make_params(48, 48, 4, flags=pkg._abi.RT_FLAG_NO_CAMERA_LISTS))
    assert same_bits(on, off) and st_on["segments"] == st_off["segments"]


def test_counters_and_fused_build_no_lists(pkg, gpu, scenes):
    """RT_FLAG_COUNTERS (the counts are the walk's) and RT_FLAG_FUSED render without lists, and render the same frame."""
    A = pkg._abi
    hs, scene = scenes["book1"]
    cam = hs.camera(1.5)
    ref, st = gpu.render(scene, cam, pkg.make_params(96, 64, 4))
    assert gpu.camera_lists_last() is not None
    for flag in (A.RT_FLAG_COUNTERS, A.RT_FLAG_FUSED):
        img, st2 = gpu.render(scene, cam, pkg.make_params(96, 64, 4, flags=flag))
        assert gpu.camera_lists_last() is None
        assert st2["segments"] == st["segments"] and (flag == A.RT_FLAG_COUNTERS or same_bits(img, ref))
    with pytest.raises(pkg.RtError):
        gpu.render(scene, cam, pkg.make_params(96, 64, 4, flags=32))
