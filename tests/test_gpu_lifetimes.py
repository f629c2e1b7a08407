"""Destroying a scene and a context gives their device memory back (rt_scene_destroy, rt_ctx_destroy): five cycles of create, upload, one
call of every family that grows a context buffer, destroy — and the free device memory after every later cycle is the first cycle's.

The bound is a condition, not a measurement. A buffer that is not freed costs its whole size again in every cycle, the families below
hold tens of megabytes between them, and the driver hands memory out in megabytes; so a cycle may move the free memory by at most a quarter
of what one context and scene held, and what they held must be at least 16 MiB or the test says nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays as R  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, SPP, CYCLES = 256, 160, 4, 5


def one_cycle(pkg):
    """-> (free bytes with everything allocated, free bytes after scene and context are closed)"""
    import torch
    A = pkg._abi
    hs = pkg.HostScene("book1", 1)
    ctx = pkg.Context(0)
    scene = ctx.upload(hs.desc)
    cam = hs.camera(W / H)
    # the pools, blocksum, tile_prefix, the counters, out_tmp and a run of events
    rgb, st = ctx.render(scene, cam, pkg.make_params(W, H, SPP, flags=A.RT_FLAG_TIMING))
    assert st["samples"] == W * H * SPP
    # sq_tmp
    prm = pkg.make_params(W, H, SPP)
    rgb, sq, _ = ctx.render_pass(scene, cam, prm, 0, SPP, False, None, np.empty(W * H * 3, dtype=np.float32))
    # rays_tmp and hits_tmp, at both sizes of a result
    rays = np.tile(R.camera_rays(cam, W, H, np.random.default_rng(1)), 4)
    assert len(rays) >= 160000
    hits = ctx.trace_rays(scene, rays)
    occ = ctx.occluded(scene, rays)
    assert np.array_equal(occ != 0, (hits["flags"] & A.RT_RAYHIT_HIT) != 0)
    # feature_rec
    ctx.render_features(scene, cam, prm)
    # denoise_planes
    dev = torch.device("cuda", 0)
    ctx.denoise(torch.from_numpy(rgb.reshape(-1)).to(dev), torch.from_numpy(sq.reshape(-1)).to(dev), W, H, samples=SPP)
    # sel_masks, sel_offsets, adaptive_word, list_map
    ada = pkg.Adaptive(ctx, scene, cam, prm, frame_samples=8, min_samples=2)
    assert ada.step(2)["samples"] == 2 * W * H
    del ada
    torch.cuda.synchronize(dev)
    low = torch.cuda.mem_get_info(dev)[0]
    scene.close()
    ctx.close()
    hs.close()
    return low, torch.cuda.mem_get_info(dev)[0]


def test_destroy_returns_device_memory(pkg):
    low, after = zip(*[one_cycle(pkg) for _ in range(CYCLES)])       # the first cycle warms the runtime and torch's allocator
    held = after[0] - low[0]
    print(f"held by one context and scene: {held / 2**20:.1f} MiB; free after each cycle, against the first: "
          f"{[(a - after[0]) / 2**20 for a in after]} MiB")
    assert held >= 16 * 2**20, held
    for k in range(1, CYCLES):
        assert abs(after[k] - after[0]) <= held / 4, (k, after[k] - after[0], held)
