"""Box records left out of a scene that is walked from LDS (csrc/scene_compile.cpp elide_box_nodes), on the GPU: the default layout against
RT_LAYOUT_ALL_BOX_NODES gives the same frames, segments and hits bit for bit in every kernel form, with fewer box tests."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,W,H,SPP", [("book1", 160, 100, 8), ("final", 96, 96, 4)])
def test_same_frame_fewer_box_tests(pkg, gpu, name, W, H, SPP):
    from conftest import record_metric
    A = pkg._abi
    hs = pkg.HostScene(name, 1)
    cam = hs.camera(W / H)
    prm = pkg.make_params(W, H, SPP, flags=A.RT_FLAG_COUNTERS)
    out = {}
    for key, flags in (("default", 0), ("all", A.RT_LAYOUT_ALL_BOX_NODES)):
        scene = gpu.upload(hs.desc, flags)
        out[key] = gpu.render(scene, cam, prm)
        scene.close()
    (img, st), (img_all, st_all) = out["default"], out["all"]
    assert st["bvh_in_lds"] == st_all["bvh_in_lds"] == 1
    assert st["scene_nodes"] < st_all["scene_nodes"]
    assert np.array_equal(img, img_all)
    assert st["segments"] == st_all["segments"]
    prim, prim_all = np.array(st["prim_tests"], dtype=np.int64), np.array(st_all["prim_tests"], dtype=np.int64)
    excess = float((prim.sum() - prim_all.sum()) / max(1, prim_all.sum()))
    ratio = st["node_tests"] / st_all["node_tests"]
    print(f"{name}: records {st_all['scene_nodes']} -> {st['scene_nodes']}, box tests per segment {st_all['node_tests'] / st_all['segments']:.3f} -> "
          f"{st['node_tests'] / st['segments']:.3f} ({ratio:.4f}), primitive tests {prim_all.tolist()} -> {prim.tolist()} (excess {excess:.3e})")
    record_metric(test="elide", scene=name, node_ratio=ratio, prim_excess=excess)
    assert st["node_tests"] < st_all["node_tests"]
    if name == "book1":
        assert ratio < 0.9
    # a leaf is tested when every box above it was passed: with fewer boxes above it, by no fewer rays
    assert np.all(prim >= prim_all)


def test_drain_form_and_ray_queries(pkg, gpu):
    import torch
    A = pkg._abi
    W, H, SPP = 64, 40, 4
    hs = pkg.HostScene("book1", 1)
    cam = hs.camera(W / H)
    rays = R.camera_rays(cam, W, H, np.random.default_rng(3))
    dev_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()
    out = {}
    for key, flags in (("default", 0), ("all", A.RT_LAYOUT_ALL_BOX_NODES)):
        scene = gpu.upload(hs.desc, flags)
        drain, _ = gpu.render(scene, cam, pkg.make_params(W, H, SPP, seed=7))
        loop, _ = gpu.render(scene, cam, pkg.make_params(W, H, SPP, seed=7, tail_paths=1))
        hits = gpu.trace_rays(scene, dev_rays).cpu().numpy().reshape(-1).view(pkg.RAYHIT_DTYPE)
        scene.close()
        out[key] = (drain, loop, hits)
    for a, b in zip(out["default"], out["all"]):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(out["default"][0], out["default"][1])
    hit = (out["default"][2]["flags"] & A.RT_RAYHIT_HIT) != 0
    assert 0.5 < hit.mean() <= 1.0            # the ground fills the lower half of the frame
