"""Throughput of the first-hit feature pass (rt_render_features_device, include/rt_hip.h): the book-1 frame at 1200 x 800, at 1 and at 16
samples per pixel, device-event times (RT_FLAG_TIMING), median of `--reps` calls after warm-up; beside it rt_trace_rays_device on the same
number of rays (the frame's pixel-centre rays, repeated) in the same process, and where the difference goes: the kernels that make the
rays (import), write the per-ray records (export) and fold them. Prints one JSON line.

    python scripts/gpu_features.py [--reps 5] [--quick] [--out features.json]"""
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
    ap.add_argument("--quick", action="store_true", help="a 240 x 160 frame at 1 and 4 samples, 3 calls: a check that the script runs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = rta.load()
    A = pkg._abi
    W, H, many, reps = (240, 160, 4, 3) if a.quick else (1200, 800, 16, a.reps)
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
    med = lambda runs, key: float(np.median([r[key] for r in runs]))
    row = dict(workload=f"book-1 first-hit features {W}x{H}", width=W, height=H, reps=reps)
    opt = pkg.ray_query_options(flags=A.RT_FLAG_TIMING)
    for spp in (1, many):
        prm = pkg.make_params(W, H, spp, seed=1, flags=A.RT_FLAG_TIMING)
        planes = ctx.render_features(scene, cam, prm)
        ctx.render_features(scene, cam, prm, albedo=planes[0], normal=planes[1], depth=planes[2], hits=planes[3])          # warm-up
        fr = [ctx.render_features(scene, cam, prm, albedo=planes[0], normal=planes[1], depth=planes[2], hits=planes[3], with_stats=True)[4] for _ in range(reps)]
        dev = torch.from_numpy(np.tile(rays, (spp, 1))).cuda()
        out = torch.empty((W * H * spp, 12), dtype=torch.float32, device="cuda")
        for _ in range(2):
            ctx.trace_rays(scene, dev, options=opt, out=out)
        qr = [ctx.trace_rays(scene, dev, options=opt, out=out, with_stats=True)[1] for _ in range(reps)]
        tag = "1spp" if spp == 1 else "nspp"
        f_ms, q_ms = med(fr, "extend_ms") + med(fr, "other_ms"), med(qr, "extend_ms") + med(qr, "other_ms")
        row.update({f"rays_{tag}": W * H * spp, f"features_{tag}_ms": round(f_ms, 4), f"features_{tag}_extend_ms": round(med(fr, "extend_ms"), 4),
                    f"features_{tag}_import_ms": round(float(np.median([r["debug"][0] for r in fr])) / 1e3, 4),
                    f"features_{tag}_export_ms": round(float(np.median([r["debug"][1] for r in fr])) / 1e3, 4),
                    f"features_{tag}_fold_ms": round(float(np.median([r["debug"][2] for r in fr])) / 1e3, 4),
                    f"query_{tag}_ms": round(q_ms, 4), f"query_{tag}_extend_ms": round(med(qr, "extend_ms"), 4), f"query_{tag}_other_ms": round(med(qr, "other_ms"), 4),
                    f"features_over_query_{tag}": round(f_ms / q_ms, 3), f"features_{tag}_mrays_per_s": round(W * H * spp / f_ms / 1e3, 1),
                    f"chunks_{tag}": int(fr[0]["extend_launches"])})
        if spp == 1:
            row["hit_fraction"] = round(float(planes[3].sum().item()) / (W * H), 4)
        del dev, out, planes
    row["samples_nspp"] = many
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
