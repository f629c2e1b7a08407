"""Throughput of ray queries (rt_trace_rays_device, include/rt_hip.h): the book-1 primary rays at 1200 x 800 (pixel centres, no lens
offset) through the query, median of `--reps` calls, in Mrays/s; beside it, for scale, extend_ms of the first wavefront iteration of a
1-spp render of the same frame (the same rays plus jitter, through the same traversal kernel). Prints one JSON line.

    python scripts/gpu_rays.py [--reps 5] [--out rays.json]"""
import argparse
import json
import os
import sys

import torch  # noqa: F401  (before the library: one HIP runtime, tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import rta
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = rta.load()
    A = pkg._abi
    W, H = 1200, 800
    hs = pkg.HostScene("book1", 1)
    ctx = pkg.Context(0)
    scene = ctx.upload(hs.desc)
    cam = hs.camera(W / H)
    v3 = lambda v: np.array([v.x, v.y, v.z])
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    u = ((x + 0.5) / (W - 1)).reshape(-1, 1)
    v = ((H - 1 - y + 0.5) / (H - 1)).reshape(-1, 1)
    rays = np.zeros((W * H, 8), dtype=np.float32)
    rays[:, 0:3] = v3(cam.origin)
    rays[:, 4:7] = v3(cam.lower_left_corner) + u * v3(cam.horizontal) + v * v3(cam.vertical) - v3(cam.origin)
    dev = torch.from_numpy(rays).cuda()
    out = torch.empty((W * H, 12), dtype=torch.float32, device="cuda")
    opt = pkg.ray_query_options(flags=A.RT_FLAG_TIMING)
    for _ in range(2):                                          # warm-up
        ctx.trace_rays(scene, dev, options=opt, out=out)
    runs = [ctx.trace_rays(scene, dev, options=opt, out=out, with_stats=True)[1] for _ in range(a.reps)]
    ms = float(np.median([r["render_ms"] for r in runs]))
    ext = float(np.median([r["extend_ms"] for r in runs]))
    hits = int((out.view(torch.int32)[:, 3] & A.RT_RAYHIT_HIT).ne(0).sum().item())
    # for scale: the first iteration of a 1-spp render of the frame (max_depth 1: one wavefront iteration, the camera rays)
    prm = pkg.make_params(W, H, 1, max_depth=1, seed=1, flags=A.RT_FLAG_TIMING, tail_paths=1)
    frame = torch.empty(W * H * 3, dtype=torch.float32, device="cuda")
    for _ in range(2):
        ctx.render_device(scene, cam, prm, frame.data_ptr())
    rr = [ctx.render_device(scene, cam, prm, frame.data_ptr()) for _ in range(a.reps)]
    row = dict(workload=f"book-1 primary rays {W}x{H}", rays=W * H, hits=hits, reps=a.reps, query_ms=round(ms, 4), query_extend_ms=round(ext, 4),
               mrays_per_s=round(W * H / ms / 1e3, 1), mrays_per_s_extend_only=round(W * H / ext / 1e3, 1),
               render_1spp_first_iteration_extend_ms=round(float(np.median([r["extend_ms"] for r in rr])), 4),
               render_1spp_iterations=int(rr[0]["iterations"]), pool_slots=int(runs[0]["pool_slots"]), bvh_in_lds=int(runs[0]["bvh_in_lds"]))
    line = json.dumps(row)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    scene.close()
    ctx.close()


if __name__ == "__main__":
    main()
