"""Helpers of the feature-moment tests (tests/test_moments_host.py, tests/test_gpu_moments.py): the first-hit feature sums AND squared sums
of one crop of a benchmarked frame, made on the CPU from the checker's answers as tests/guided.py makes the sums — per sample the
contract's albedo, normal and depth, rounded to f32; the sum and the f32 square of that value folded in f32 in sample order, as
rt_render_feature_moments_device folds them — random guides with variances, and the host's fold of squares from one-sample passes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crops as K     # noqa: E402
import features as F  # noqa: E402
import guided as G    # noqa: E402
import rays as R      # noqa: E402

FEATURE_SAMPLES = G.FEATURE_SAMPLES
PLANES = ("albedo_sum", "normal_sum", "depth_sum", "hits", "albedo_sq_sum", "normal_sq_sum", "depth_sq_sum")


def crop_feature_moments(pkg, orc, name, crop, tmp_path, n_f=FEATURE_SAMPLES):
    """guided.crop_feature_sums with the second moments: a dict of albedo_sum, normal_sum (64, 64, 3) f32, depth_sum (64, 64) f32, hits
    (64, 64) u32 — the same additions, so the same bits — and albedo_sq_sum, normal_sq_sum, depth_sq_sum: the f32 fold of fl(x * x)."""
    cfg = K.CONFIGS[name]
    hs = K.host_scene(pkg, name, tmp_path)
    W, H, rect = cfg["width"], cfg["height"], cfg["crops"][crop]
    cam = hs.camera(W / H)
    desc = hs.desc
    prims = R.primitives(pkg, desc)
    mats = np.array([h.material for _, h, _ in prims])
    n = (rect[2] - rect[0]) * (rect[3] - rect[1])
    f32 = np.float32
    albedo, normal, depth, hits = np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros(n, f32), np.zeros(n, np.uint32)
    albedo_sq, normal_sq, depth_sq = np.zeros((n, 3), f32), np.zeros((n, 3), f32), np.zeros(n, f32)
    for s in range(n_f):
        o, d, tm = G.crop_camera_rays(orc, cam, W, H, rect, cfg["seed"], s)
        rays = R.make_rays(o, d, tm)
        ref = R.ask(orc, desc, rays)
        hit = ref["hit"]
        k = np.flatnonzero(hit)
        material = np.full(n, -1)
        if len(k):
            t64 = rays["time"].astype(np.float64)[k]
            dist = np.stack([R.surface_distance(pkg, h, chain, ref["p"][k], t64) for _, h, chain in prims], axis=1)
            material[k] = mats[dist.argmin(axis=1)]
        a = F.expected_albedo(pkg, orc, desc, hit, material, ref["ff"], ref["u"], ref["v"], ref["p"], rays["d"].astype(np.float64)).astype(f32)
        nn = np.where(hit[:, None], ref["n"], 0.0).astype(f32)
        length = np.linalg.norm(rays["d"].astype(np.float64), axis=1)
        dd = np.where(hit, ref["t"] * length, 0.0).astype(f32)
        albedo += a; normal += nn; depth += dd; hits += hit.astype(np.uint32)
        albedo_sq += a * a; normal_sq += nn * nn; depth_sq += dd * dd          # f32 products, f32 additions
    h, w = rect[3] - rect[1], rect[2] - rect[0]
    return dict(albedo_sum=albedo.reshape(h, w, 3), normal_sum=normal.reshape(h, w, 3), depth_sum=depth.reshape(h, w), hits=hits.reshape(h, w),
                albedo_sq_sum=albedo_sq.reshape(h, w, 3), normal_sq_sum=normal_sq.reshape(h, w, 3), depth_sq_sum=depth_sq.reshape(h, w))


def any_moments_guide(H, W, n_f=4, seed=3):
    """Random per-sample features folded to sums and squared sums: a guide with random, consistent variances (hits from 0 to n_f)."""
    rng = np.random.default_rng(seed)
    hit = rng.integers(0, 2, (n_f, H, W)).astype(bool)
    a = rng.uniform(0, 1, (n_f, H, W, 3)).astype(np.float32)
    n = (rng.uniform(-1, 1, (n_f, H, W, 3)) * hit[..., None]).astype(np.float32)
    d = (rng.uniform(1, 30, (n_f, H, W)) * hit).astype(np.float32)
    fold = lambda x: fold_f32(list(x))
    return dict(albedo_sum=fold(a), normal_sum=fold(n), depth_sum=fold(d), hits=hit.sum(axis=0).astype(np.uint32),
                albedo_sq_sum=fold(a * a), normal_sq_sum=fold(n * n), depth_sq_sum=fold(d * d))


def fold_f32(values, start=None):
    """The sequential f32 fold of a list of f32 arrays, from 0 or from `start`."""
    acc = np.zeros_like(values[0], dtype=np.float32) if start is None else np.asarray(start, dtype=np.float32).copy()
    for v in values:
        acc = (acc + np.asarray(v, dtype=np.float32)).astype(np.float32)
    return acc


def variance_step_frame(sigma_albedo, variance_factor):
    """guided.step_edge_frame with squared albedo sums: per pixel VA = variance_factor x the squared albedo step |da|^2 (summed over the
    three channels; 0: the planes of noise-free features, Q = S^2 / n_f). Returns (S, Q, n, albedo_sum, albedo_sq_sum, n_f)."""
    S, Q, n, albedo, n_f = G.step_edge_frame(sigma_albedo)
    a = albedo.astype(np.float64)
    step2 = 3.0 * (10.0 * sigma_albedo) ** 2                  # |a_left - a_right|^2 of the means
    var_c = variance_factor * step2 / 3.0                     # per channel: var(S, Q) = (Q - S^2 / n_f) / (n_f (n_f - 1))
    sq = a * a / n_f + var_c * n_f * (n_f - 1)
    return S, Q, n, albedo, sq.astype(np.float32), n_f
