"""Helpers of the guided-denoise tests (tests/test_guided_host.py, tests/test_gpu_guided.py): the first-hit feature sums of one crop of a
benchmarked frame, made on the CPU from the checker's answers — the renderer's camera rays restated for the crop's pixels only (the full
1200 x 800 loop of features.camera_rays is too slow in Python), the checker's world.hit, and the contract's albedo, normal and depth per
sample, folded in f32 in sample order as rt_render_features_device folds them — and the step-edge frame on which the guide must act."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crops as K     # noqa: E402
import features as F  # noqa: E402
import rays as R      # noqa: E402

FEATURE_SAMPLES = 4


def crop_camera_rays(orc, cam, width, height, rect, seed, sample, n_draws=40):
    """features.camera_rays for the pixels of rect = (x0, y0, x1, y1) only, row-major within the rect; the pixel index that keys the
    draws stays y * width + x of the full frame."""
    v3 = lambda v: np.array([v.x, v.y, v.z], dtype=np.float64)
    org, llc, hor, ver, cu, cv = v3(cam.origin), v3(cam.lower_left_corner), v3(cam.horizontal), v3(cam.vertical), v3(cam.u), v3(cam.v)
    x0, y0, x1, y1 = rect
    n = (x1 - x0) * (y1 - y0)
    o, d, tm = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    f32 = np.float32
    j = 0
    for y in range(y0, y1):
        for x in range(x0, x1):
            r = orc.rng_stream(seed, y * width + x, sample, n_draws)[2]
            u, v = (x + float(r[0])) / (width - 1), (height - 1 - y + float(r[1])) / (height - 1)
            k = 2
            while True:
                if k + 3 > n_draws:
                    raise RuntimeError("the disk rejection ran out of draws")
                px, py = f32(-1.0) + f32(2.0) * r[k], f32(-1.0) + f32(2.0) * r[k + 1]
                k += 2
                if f32(f32(px * px) + f32(py * py)) < f32(1.0):
                    break
            off = cu * (cam.lens_radius * float(px)) + cv * (cam.lens_radius * float(py))
            o[j] = org + off
            d[j] = llc + hor * u + ver * v - org - off
            tm[j] = cam.time0 + (cam.time1 - cam.time0) * float(r[k])
            j += 1
    return o, d, tm


def crop_feature_sums(pkg, orc, name, crop, tmp_path, n_f=FEATURE_SAMPLES):
    """(albedo_sum (64, 64, 3) f32, normal_sum (64, 64, 3) f32, depth_sum (64, 64) f32, hits (64, 64) u32) of the crop over samples
    0 .. n_f - 1, as rt_render_features_device states them. The material of a hit is that of the primitive whose surface the checker's hit
    point lies nearest to (the checker reports no material)."""
    cfg = K.CONFIGS[name]
    hs = K.host_scene(pkg, name, tmp_path)
    W, H, rect = cfg["width"], cfg["height"], cfg["crops"][crop]
    cam = hs.camera(W / H)
    desc = hs.desc
    prims = R.primitives(pkg, desc)
    mats = np.array([h.material for _, h, _ in prims])
    n = (rect[2] - rect[0]) * (rect[3] - rect[1])
    albedo, normal = np.zeros((n, 3), dtype=np.float32), np.zeros((n, 3), dtype=np.float32)
    depth, hits = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint32)
    for s in range(n_f):
        o, d, tm = crop_camera_rays(orc, cam, W, H, rect, cfg["seed"], s)
        rays = R.make_rays(o, d, tm)
        ref = R.ask(orc, desc, rays)
        hit = ref["hit"]
        k = np.flatnonzero(hit)
        material = np.full(n, -1)
        if len(k):
            t64 = rays["time"].astype(np.float64)[k]
            dist = np.stack([R.surface_distance(pkg, h, chain, ref["p"][k], t64) for _, h, chain in prims], axis=1)
            material[k] = mats[dist.argmin(axis=1)]
        a = F.expected_albedo(pkg, orc, desc, hit, material, ref["ff"], ref["u"], ref["v"], ref["p"], rays["d"].astype(np.float64))
        albedo += a.astype(np.float32)
        normal += np.where(hit[:, None], ref["n"], 0.0).astype(np.float32)
        length = np.linalg.norm(rays["d"].astype(np.float64), axis=1)
        depth += np.where(hit, ref["t"] * length, 0.0).astype(np.float32)
        hits += hit.astype(np.uint32)
    h, w = rect[3] - rect[1], rect[2] - rect[0]
    return albedo.reshape(h, w, 3), normal.reshape(h, w, 3), depth.reshape(h, w), hits.reshape(h, w)


def step_edge_frame(sigma_albedo, H=40, W=48, n=16, seed=11):
    """(S, Q, n, albedo_sum, n_f): radiance samples in [0, 1] on the left half and in [100, 101] on the right; Q inflated so that the
    variance of the mean is about 50^2 everywhere (the patch distance cannot see the step: plain NLM mixes the halves); albedo planes that
    differ by 10 sigma_albedo in every channel across the edge (g >= 3 x 100 there, the cross weight is below exp(-100))."""
    rng = np.random.default_rng(seed)
    smp = rng.uniform(0.0, 1.0, (H, W, n, 3))
    smp[:, W // 2:] += 100.0
    S = smp.sum(axis=2)
    Q = S * S / n + float(n * (n - 1)) * 50.0 ** 2            # v = (Q - S^2 / n) / (n (n - 1)) = 50^2
    n_f = 4
    albedo = np.full((H, W, 3), 0.25 * n_f, dtype=np.float32)
    albedo[:, W // 2:] += np.float32(10.0 * sigma_albedo * n_f)
    return S.astype(np.float32), Q.astype(np.float32), n, albedo, n_f
