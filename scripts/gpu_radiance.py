"""Radiance queries against a render of the same sample count (rt_radiance_rays_device / rt_render_device, include/rt_hip.h).

The Cornell box at 600 x 600 x 64 samples, twice: by the render, and by a radiance query over the frame's camera rays restated on the host
(pixel centres, no lens: the box's camera has none), 64 samples each. Both run `--reps` times after a warm-up, alternating, with
RT_FLAG_TIMING: the library's device events give the traversal, shading, drain and other (generate + resolve / import + fold) parts.
Medians, each side's own spread, the rates in samples per second of the call's wall time, and their ratio. Writes one JSON document.

    python scripts/gpu_radiance.py [--reps 5] [--scale 1.0] [--samples 64] [--out radiance.json]"""
import argparse
import json
import os
import sys

import torch  # noqa: F401  (before the library: one HIP runtime, tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera_rays(np, cam, W, H):
    v3 = lambda v: np.array([v.x, v.y, v.z])
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    u = ((x + 0.5) / (W - 1)).reshape(-1, 1)
    v = ((H - 1 - y + 0.5) / (H - 1)).reshape(-1, 1)
    rays = np.zeros((W * H, 8), dtype=np.float32)
    rays[:, 0:3] = v3(cam.origin)
    rays[:, 4:7] = v3(cam.lower_left_corner) + u * v3(cam.horizontal) + v * v3(cam.vertical) - v3(cam.origin)
    return rays


def main():
    import numpy as np
    import rta
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="frame edge factor (a smoke run uses 0.1)")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = rta.load()
    A = pkg._abi
    ctx = pkg.Context(0)
    W = H = max(16, int(round(600 * a.scale)))
    S = a.samples
    hs = pkg.HostScene("cornell", 0)
    cam = hs.camera(1.0)
    scene = ctx.upload(hs.desc)
    prm = pkg.make_params(W, H, S, max_depth=50, seed=1, flags=A.RT_FLAG_TIMING)
    opt = pkg.radiance_options(S, max_depth=50, seed=1, render_flags=A.RT_FLAG_TIMING)
    frame = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    dev = torch.from_numpy(camera_rays(np, cam, W, H)).cuda()
    rgb = torch.empty((W * H, 3), dtype=torch.float32, device="cuda")
    sq, inv = torch.empty_like(rgb), torch.empty((W * H,), dtype=torch.uint8, device="cuda")
    query = lambda: ctx.radiance(scene, dev, S, options=opt, rgb_sum=rgb, sq_sum=sq, invalid=inv, with_stats=True)[3]
    render = lambda: ctx.render_device(scene, cam, prm, frame.data_ptr())
    for _ in range(2):                                      # warm-up, both entry points
        render(); query()
    sr, sq_ = [], []
    for _ in range(a.reps):                                 # alternating
        sr.append(render()); sq_.append(query())
    assert int(inv.ne(0).sum().item()) == 0 and bool(torch.isfinite(rgb).all().item())
    parts = ("render_ms", "extend_ms", "shade_ms", "drain_ms", "other_ms")
    doc = dict(what="rt_radiance_rays_device over the frame's pixel-centre camera rays against rt_render_device, Cornell box, the same sample count; medians of "
                    "the calls' wall time (render_ms) and of the device parts (RT_FLAG_TIMING)",
               frame=f"{W}x{H}", samples=S, reps=a.reps, paths=W * H * S)
    for side, st in (("render", sr), ("query", sq_)):
        for p in parts:
            doc[f"{side}_{p}"] = round(float(np.median([r[p] for r in st])), 4)
        doc[f"{side}_ms_min_max"] = [round(float(min(r["render_ms"] for r in st)), 4), round(float(max(r["render_ms"] for r in st)), 4)]
        doc[f"{side}_segments"] = int(st[0]["segments"])
        doc[f"{side}_pool_slots"] = int(st[0]["pool_slots"])
        doc[f"{side}_iterations"] = int(st[0]["iterations"])
        doc[f"{side}_msamples_per_s"] = round(W * H * S / doc[f"{side}_render_ms"] / 1e3, 2)
    doc["query_rate_over_render_rate"] = round(doc["query_msamples_per_s"] / doc["render_msamples_per_s"], 4)
    # the means agree as two estimates of one frame do (the query's rays go through the pixel centres, the render's are jittered)
    doc["mean_radiance_render"] = round(float(frame.mean().item()) / S, 5)
    doc["mean_radiance_query"] = round(float(rgb.mean().item()) / S, 5)
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    scene.close()
    ctx.close()


if __name__ == "__main__":
    main()
