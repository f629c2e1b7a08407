"""Occlusion queries against closest-hit queries on the same rays (rt_occluded_rays_device / rt_trace_rays_device, include/rt_hip.h).

Three scenes — book-1 at 1200 x 800, the Cornell box at 600 x 600, and a triangle height field over a ground rect uploaded with
RT_LAYOUT_SCENE_IN_HBM at 1200 x 800 — and two ray sets each:
  primary  the pixel-centre camera rays of the frame, no limit (mostly occluded: the early exit and nothing else);
  shadow   as many rays from those rays' hit points (misses reuse the hit points in order) to one point above the scene, d spanning the
           two points and t_max = 1 (mostly unoccluded with a finite limit: the interval and nothing else).
Per set the two entry points are called alternately, `--reps` times each after a warm-up, with RT_FLAG_TIMING: the library's own device
events on the context's stream give extend_ms (the traversal kernels) and other_ms (the kernels that read the rays and write the results);
their sum is the device time of a call. Medians, the spread (min .. max) of each side's own repeats, and whether the bytes equal the
closest hit's hit / miss. Writes one JSON document.

    python scripts/gpu_occlusion.py [--reps 5] [--scale 1.0] [--out occlusion.json]"""
import argparse
import json
import os
import sys

import torch  # noqa: F401  (before the library: one HIP runtime, tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mesh_scene(pkg):
    """The height field of the ray-query tests: 12 x 12 x 2 triangles over a ground rect, in a BVH."""
    import numpy as np
    A = pkg._abi
    rng = np.random.default_rng(20240611)
    b = pkg.SceneBuilder(background=(0.5, 0.7, 1.0), background_mode=A.RT_BG_SKY_GRADIENT)
    n, mats = 12, [b.lambertian((0.7, 0.3, 0.3)), b.metal((0.8, 0.8, 0.8), 0.1)]
    h = rng.uniform(0.0, 0.8, (n + 1, n + 1))
    P = lambda i, j: (-2.0 + 4.0 * i / n, float(h[i, j]), -2.0 + 4.0 * j / n)
    ids = []
    for i in range(n):
        for j in range(n):
            ids.append(b.triangle(P(i, j), P(i + 1, j), P(i, j + 1), mats[(i + j) & 1]))
            ids.append(b.triangle(P(i + 1, j), P(i + 1, j + 1), P(i, j + 1), mats[(i + j + 1) & 1]))
    ids.append(b.xz_rect(-6, 6, -6, 6, -0.25, b.lambertian((0.5, 0.5, 0.5))))
    desc = b.desc(b.bvh(ids))
    cam = pkg.camera_new((3.0, 2.0, 6.0), (0.0, 0.5, 0.0), (0, 1, 0), 30.0, 1.5, 0.0, 10.0, 0.0, 0.0)
    return desc, cam, b


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = rta.load()
    A = pkg._abi
    ctx = pkg.Context(0)
    opt = pkg.ray_query_options(flags=A.RT_FLAG_TIMING)
    size = lambda w, h: (max(16, int(round(w * a.scale))), max(16, int(round(h * a.scale))))
    book1, cornell = pkg.HostScene("book1", 1), pkg.HostScene("cornell", 0)
    mdesc, mcam, keep = mesh_scene(pkg)
    W1, H1 = size(1200, 800)
    WC, HC = size(600, 600)
    # (scene, description, camera, frame, layout, the point the shadow rays go to)
    scenes = [("book1", book1.desc, book1.camera(W1 / H1), (W1, H1), 0, (0.0, 30.0, 0.0)),
              ("cornell", cornell.desc, cornell.camera(WC / HC), (WC, HC), 0, (278.0, 540.0, 279.5)),
              ("mesh_hbm", mdesc, mcam, (W1, H1), A.RT_LAYOUT_SCENE_IN_HBM, (1.0, 8.0, 2.0))]
    rows = []
    for name, desc, cam, (W, H), layout, light in scenes:
        scene = ctx.upload(desc, layout)
        prim = camera_rays(np, cam, W, H)
        d_prim = torch.from_numpy(prim).cuda()
        hits = torch.empty((W * H, 12), dtype=torch.float32, device="cuda")
        ctx.trace_rays(scene, d_prim, out=hits)
        rec = hits.cpu().numpy().reshape(-1).view(pkg.RAYHIT_DTYPE)
        k = np.flatnonzero((rec["flags"] & A.RT_RAYHIT_HIT) != 0)
        assert len(k) > 0, name
        src = k[np.arange(W * H) % len(k)] if len(k) < W * H else k       # misses reuse the hit points in order
        shadow = np.zeros((W * H, 8), dtype=np.float32)
        shadow[:, 0:3] = rec["p"][src]
        shadow[:, 4:7] = np.asarray(light, np.float32) - rec["p"][src]
        shadow[:, 7] = 1.0
        for kind, rays in (("primary", prim), ("shadow", shadow)):
            dev = torch.from_numpy(rays).cuda()
            occ = torch.empty((len(rays),), dtype=torch.uint8, device="cuda")
            for _ in range(2):                                  # warm-up, both entry points
                ctx.occluded(scene, dev, options=opt, out=occ)
                ctx.trace_rays(scene, dev, options=opt, out=hits)
            so, stt = [], []
            for _ in range(a.reps):                             # alternating
                so.append(ctx.occluded(scene, dev, options=opt, out=occ, with_stats=True)[1])
                stt.append(ctx.trace_rays(scene, dev, options=opt, out=hits, with_stats=True)[1])
            closest = (hits.view(torch.int32)[:, 3] & A.RT_RAYHIT_HIT).ne(0)
            agree = bool((occ.ne(0) == closest).all().item()) and bool(((occ == 0) | (occ == A.RT_RAYHIT_HIT)).all().item())
            row = dict(scene=name, rays_kind=kind, frame=f"{W}x{H}", layout=int(layout), rays=len(rays), occluded=int(occ.ne(0).sum().item()),
                       agree_with_closest_hit=agree, reps=a.reps, bvh_in_lds=int(so[0]["bvh_in_lds"]), extend_threads=int(so[0]["debug"][6]) if "debug" in so[0] else 0)
            for side, st in (("occluded", so), ("trace", stt)):
                tot = [r["extend_ms"] + r["other_ms"] for r in st]
                row[side + "_ms"] = round(float(np.median(tot)), 4)
                row[side + "_ms_min_max"] = [round(float(min(tot)), 4), round(float(max(tot)), 4)]
                row[side + "_extend_ms"] = round(float(np.median([r["extend_ms"] for r in st])), 4)
                row[side + "_other_ms"] = round(float(np.median([r["other_ms"] for r in st])), 4)
                row[side + "_call_ms"] = round(float(np.median([r["render_ms"] for r in st])), 4)
            row["speedup"] = round(row["trace_ms"] / row["occluded_ms"], 3)
            row["speedup_extend"] = round(row["trace_extend_ms"] / row["occluded_extend_ms"], 3)
            rows.append(row)
            print(json.dumps(row))
        scene.close()
    doc = dict(what="rt_occluded_rays_device against rt_trace_rays_device on the same rays: device time = extend_ms + other_ms (RT_FLAG_TIMING), medians",
               sets=rows)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
