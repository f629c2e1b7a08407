"""In-place camera shading on the GPU (kernels.h RenderDev::cam_shade): a camera ray that its square's list answers with a hit is shaded by
the lane that made it — k_generate, k_shade's regeneration — and only the scattered ray is stored. The segment stands in no queue, so it is
counted where its record is read (kernels.h kRayShaded). With and without RT_FLAG_NO_CAMERA_LISTS (which turns the lists and the in-place
shade off) a render leaves the same bytes and the same segment and sample counts: whichever kernel reads k_generate's records first (k_shade,
or the drain with the default tail_paths), with lineages of 1 and of 4 items, at the depth limits 1 (not eligible), 2 (the in-place shade is
the path's last scatter) and 3, in a scene with an emitting sphere (not eligible), with every camera ray hitting and every camera ray
missing, with items of 16 samples, in a shard, a progressive pair and a pixel-list pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def params(pkg, w, h, spp, off, quarter=True, flags=0, items=None, **kw):
    """quarter: a pool of at most a quarter of the work items, so that k_shade regenerates (else one slot per item); off: RT_FLAG_NO_CAMERA_LISTS."""
    items = w * h * spp // kw.get("shard_count", 1) if items is None else items
    return pkg.make_params(w, h, spp, flags=flags | (pkg._abi.RT_FLAG_NO_CAMERA_LISTS if off else 0), pool_slots=quarter_pool(items) if quarter else 0, **kw)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def on_and_off(pkg, gpu, scene, cam, w, h, spp, lists=True, **kw):
    """The render with and without the lists: same bytes, same counts. Returns the frame and the stats of the render with them."""
    on, st_on = gpu.render(scene, cam, params(pkg, w, h, spp, False, **kw))
    assert (gpu.camera_lists_last() is not None) == lists
    off, st_off = gpu.render(scene, cam, params(pkg, w, h, spp, True, **kw))
    assert gpu.camera_lists_last() is None
    print(f"segments {st_on['segments']} / {st_off['segments']}, samples {st_on['samples']} / {st_off['samples']}, drain_paths {st_on['drain_paths']}")
    assert same_bits(on, off)
    assert st_on["segments"] == st_off["segments"]
    assert st_on["samples"] == st_off["samples"]
    if kw.get("tail_paths") == 1:
        assert st_on["drain_paths"] == 0
    return on, st_on


@pytest.mark.parametrize("name,w,h,spp", [("book1", 100, 52, 4), ("book1_sah", 96, 64, 4), ("book1", 96, 64, 4), ("book1_sah", 100, 52, 4)])
@pytest.mark.parametrize("tail_paths", [1, 0])
@pytest.mark.parametrize("quarter", [False, True])
def test_book1_is_the_same(pkg, gpu, scenes, name, w, h, spp, tail_paths, quarter):
    """Depth 50. One slot per item: every record of k_generate is read by the first k_shade (tail_paths 1) or by the drain (0: so few paths go
    to it at once). A quarter pool: lineages of 4, k_shade's regeneration shades in place too. 100 x 52 has partial squares and clipped tiles."""
    hs, scene = scenes[name]
    img, st = on_and_off(pkg, gpu, scene, hs.camera(w / h), w, h, spp, tail_paths=tail_paths, quarter=quarter)
    assert st["bvh_in_lds"] == 1 and st["samples"] == w * h * spp and st["segments"] > st["samples"]
    if quarter:
        assert st["pool_slots"] * 4 <= w * h * spp
    else:
        assert st["pool_slots"] >= w * h * spp
        if tail_paths == 0:
            assert st["extend_launches"] == 0 and st["drain_paths"] > 0       # the drain read k_generate's records


@pytest.mark.parametrize("max_depth", [1, 2, 3])
@pytest.mark.parametrize("tail_paths", [1, 0])
def test_depth_limits(pkg, gpu, scenes, max_depth, tail_paths):
    """max_depth 1: not eligible (the in-place shade would end the path), every sample is one segment. 2: the in-place shade is the last scatter."""
    hs, scene = scenes["book1"]
    w, h, spp = 96, 64, 4
    img, st = on_and_off(pkg, gpu, scene, hs.camera(w / h), w, h, spp, tail_paths=tail_paths, max_depth=max_depth)
    if max_depth == 1:
        assert st["segments"] == st["samples"] == w * h * spp
    else:
        assert st["samples"] < st["segments"] <= max_depth * st["samples"]


def spheres_scene(pkg, gpu, light):
    """A ground sphere, a dozen Lambertian, metal and glass spheres on it and, with `light`, one emitting sphere above them; black background."""
    b = pkg.SceneBuilder(background=(0.0, 0.0, 0.0))
    ids = [b.sphere((0.0, -1000.0, 0.0), 1000.0, b.lambertian((0.5, 0.5, 0.5)))]
    mats = [b.lambertian((0.7, 0.3, 0.2)), b.metal((0.8, 0.8, 0.6), 0.1), b.dielectric(1.5), b.lambertian((0.2, 0.4, 0.8))]
    k = 0
    for z in (-2.0, 0.0, 2.0):
        for x in (-3.0, -1.0, 1.0, 3.0):
            ids.append(b.sphere((x + 0.3 * z, 0.45, z), 0.45, mats[k % len(mats)]))
            k += 1
    if light:
        ids.append(b.sphere((0.0, 2.2, 0.0), 0.6, b.diffuse_light((4.0, 4.0, 4.0))))
    desc = b.desc(b.bvh(ids))
    return b, desc, gpu.upload(desc)


def camera(pkg, lookfrom, lookat, aspect):
    return pkg.camera_new(lookfrom, lookat, (0, 1, 0), 40.0, aspect, 0.0, float(np.linalg.norm(np.subtract(lookfrom, lookat))), 0.0, 0.0)


def test_the_in_place_shade_takes_an_iteration_off(pkg, gpu):
    """That camera rays ARE shaded where they are made: every camera ray hits and every square has a list, one slot per item, max_depth 2, the
    wavefront kernels to the end. Without the lists a path needs two k_shade launches (the camera segment, the segment after it); with them
    the first launch already reads depth-1 records and is the last."""
    keep, desc, scene = spheres_scene(pkg, gpu, False)
    w, h, spp = 64, 40, 4
    cam = camera(pkg, (0.0, 7.0, 4.0), (0.0, 0.0, 0.0), w / h)
    lists = pkg.camera_lists_host(desc, cam, w, h)
    assert lists is not None and (lists[:, 0] != pkg._abi.RT_CAMERA_LIST_WALK).all()
    _, st_on = gpu.render(scene, cam, params(pkg, w, h, spp, False, quarter=False, tail_paths=1, max_depth=2))
    _, st_off = gpu.render(scene, cam, params(pkg, w, h, spp, True, quarter=False, tail_paths=1, max_depth=2))
    print(st_on["iterations"], st_off["iterations"], st_on["segments"], st_off["segments"])
    assert st_off["iterations"] == 2 and st_on["iterations"] == 1
    assert st_on["segments"] == st_off["segments"] == 2 * w * h * spp


@pytest.mark.parametrize("tail_paths", [1, 0])
def test_a_scene_with_an_emitting_sphere_is_not_eligible(pkg, gpu, tail_paths):
    """A camera ray can end on the light: camera rays are answered from the lists, none is shaded in place; the parent's render, bit for bit."""
    keep, desc, scene = spheres_scene(pkg, gpu, True)
    w, h, spp = 64, 40, 8
    img, st = on_and_off(pkg, gpu, scene, camera(pkg, (0.0, 3.0, 9.0), (0.0, 1.0, 0.0), w / h), w, h, spp, tail_paths=tail_paths)
    assert st["segments"] > st["samples"] == w * h * spp and float(np.max(img)) > 0.0      # the light is in view


@pytest.mark.parametrize("tail_paths", [1, 0])
@pytest.mark.parametrize("quarter", [False, True])
def test_every_camera_ray_hits(pkg, gpu, tail_paths, quarter):
    keep, desc, scene = spheres_scene(pkg, gpu, False)
    w, h, spp = 64, 40, 4
    img, st = on_and_off(pkg, gpu, scene, camera(pkg, (0.0, 7.0, 4.0), (0.0, 0.0, 0.0), w / h), w, h, spp, tail_paths=tail_paths, quarter=quarter)
    assert st["segments"] >= 2 * st["samples"] and st["samples"] == w * h * spp            # max_depth 50 >= 2: every path scatters at least once


@pytest.mark.parametrize("tail_paths", [1, 0])
def test_every_camera_ray_misses(pkg, gpu, tail_paths):
    """Looking up past every sphere: every ray is answered with a miss, nothing is shaded in place."""
    keep, desc, scene = spheres_scene(pkg, gpu, False)
    w, h, spp = 64, 40, 4
    img, st = on_and_off(pkg, gpu, scene, camera(pkg, (0.0, 2.5, 6.0), (0.0, 12.0, 0.0), w / h), w, h, spp, tail_paths=tail_paths)
    assert st["segments"] == st["samples"] == w * h * spp


@pytest.mark.parametrize("tail_paths", [1, 0])
def test_sample_blocks(pkg, gpu, scenes, tail_paths):
    """RT_FLAG_SAMPLE_BLOCKS: items of 16 samples, records with s1. Only an item's first camera ray is answered where it is made."""
    hs, scene = scenes["book1"]
    w, h, spp = 96, 64, 32
    img, st = on_and_off(pkg, gpu, scene, hs.camera(w / h), w, h, spp, tail_paths=tail_paths, flags=pkg._abi.RT_FLAG_SAMPLE_BLOCKS, items=w * h * spp // 16)
    assert st["samples"] == w * h * spp and st["pool_slots"] < w * h * spp // 8


def test_shard_is_the_same(pkg, gpu, scenes):
    """Shard 1 of 2, tile-compact output, max_depth 2."""
    hs, scene = scenes["book1"]
    w, h, spp = 100, 52, 4
    on_and_off(pkg, gpu, scene, hs.camera(w / h), w, h, spp, tile_size=32, shard_index=1, shard_count=2, tail_paths=1, max_depth=2)


def test_progressive_pair_is_the_same(pkg, gpu, scenes):
    """Two passes, the second with RT_PASS_ACCUMULATE, max_depth 2: rgb_sum and sq_sum."""
    hs, scene = scenes["book1"]
    w, h, spp = 100, 52, 4
    cam = hs.camera(w / h)
    a = spp // 2
    out = {}
    for off in (False, True):
        prm = params(pkg, w, h, spp, off, tail_paths=1, max_depth=2)
        rgb, sq, st0 = gpu.render_pass(scene, cam, with_spp(pkg, prm, a), 0, spp, False, None, np.zeros(pkg.output_floats(prm), np.float32))
        assert (gpu.camera_lists_last() is None) == off
        rgb, sq, st1 = gpu.render_pass(scene, cam, with_spp(pkg, prm, spp - a), a, spp, True, np.ascontiguousarray(rgb).reshape(-1), np.ascontiguousarray(sq).reshape(-1))
        assert st0["drain_paths"] == 0 and st1["drain_paths"] == 0
        out[off] = (rgb, sq, st0["segments"] + st1["segments"], st0["samples"] + st1["samples"])
    print(out[False][2:], out[True][2:])
    assert same_bits(out[False][0], out[True][0]) and same_bits(out[False][1], out[True][1])
    assert out[False][2] == out[True][2]
    assert out[False][3] == out[True][3] == w * h * spp
    one, _ = gpu.render(scene, cam, params(pkg, w, h, spp, False, tail_paths=1, max_depth=2))
    assert same_bits(out[False][0], one)


def test_pixel_list_pass_is_the_same(pkg, gpu, scenes):
    """One pass over every third pixel (rt_render_pass_pixels_device), max_depth 2."""
    import torch
    hs, scene = scenes["book1"]
    w, h, spp = 100, 52, 4
    cam = hs.camera(w / h)
    listed = np.arange(0, w * h, 3, dtype=np.int32)
    lst = torch.from_numpy(listed).cuda()
    out = {}
    for off in (False, True):
        prm = pkg.make_params(w, h, spp, max_depth=2, flags=pkg._abi.RT_FLAG_NO_CAMERA_LISTS if off else 0, pool_slots=quarter_pool(len(listed) * spp), tail_paths=1)
        rgb = torch.full((3 * w * h,), 2.5, dtype=torch.float32, device="cuda")
        sq = torch.full((3 * w * h,), 2.5, dtype=torch.float32, device="cuda")
        counts = torch.zeros(w * h, dtype=torch.int32, device="cuda")
        st = gpu.render_pass_pixels(scene, cam, prm, 0, spp, False, lst, lst.numel(), rgb, sq, counts)
        assert (gpu.camera_lists_last() is None) == off and st["drain_paths"] == 0
        out[off] = (rgb.cpu().numpy(), sq.cpu().numpy(), counts.cpu().numpy(), st["segments"], st["samples"])
    print(out[False][3:], out[True][3:])
    for k in range(3):
        assert same_bits(out[False][k], out[True][k])
    assert out[False][3] == out[True][3]
    assert out[False][4] == out[True][4] == len(listed) * spp
