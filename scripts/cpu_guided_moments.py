"""The variance-guided filter's defaults, measured on the CPU ("Denoising"): python scripts/cpu_guided_moments.py [--out FILE]
For each of the seven crops of tests/test_denoise_host.py: 16-spp sums by the f64 checker, the feature sums and squared sums of samples
0..3 by tests/moments.py, and the numpy restatement nlm_guided_moments_reference (binary16 rounding included) at window radius 8 over the
grid sigmas x variance_strength; beside it the plain filter at r 8 and r 10 and the guided filter with its defaults at r 10. The defaults
of include/rt_hip.h are the grid point with the smallest geometric mean of filtered MSE / raw MSE. Neither the checker nor the
restatement is the code under test."""
import argparse
import json
import multiprocessing
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIGMAS = ((0.01, 0.025, 0.01), (0.02, 0.05, 0.02), (0.02, 0.05, 0.05), (0.05, 0.1, 0.05), (0.2, 0.5, 0.2))
KAPPAS = (4.0, 16.0, 64.0)
RADIUS = 8


def one_crop(job):
    name, crop = job
    import rta
    pkg = rta.load()
    from oracle import binding as orc
    import crops as K
    import moments as M
    from test_denoise_host import DENOISE_SPP, oracle_crop_sums
    tmp = tempfile.mkdtemp()
    truth = K.load_golden(name)[crop] / K.CONFIGS[name]["spp"]
    S, Q = oracle_crop_sums(pkg, orc, name, crop, tmp)
    g = M.crop_feature_moments(pkg, orc, name, crop, tmp)
    sums = {k: g[k] for k in ("albedo_sum", "normal_sum", "depth_sum", "hits")}
    mse = lambda img: float(np.mean((img - truth) ** 2))
    raw = mse(S.astype(np.float64) / DENOISE_SPP)
    row = dict(crop=f"{name}/{crop}", mse_raw=raw, plain_r8=mse(pkg.nlm_reference(S, Q, DENOISE_SPP, 1, window_radius=RADIUS)) / raw,
               plain_r10=mse(pkg.nlm_reference(S, Q, DENOISE_SPP, 1)) / raw,
               guided_r10=mse(pkg.nlm_guided_reference(S, Q, DENOISE_SPP, 1, M.FEATURE_SAMPLES, **sums)) / raw, moments={})
    for sa, sn, sz in SIGMAS:
        for kappa in KAPPAS:
            out = pkg.nlm_guided_moments_reference(S, Q, DENOISE_SPP, 1, M.FEATURE_SAMPLES, **g, sigma_albedo=sa, sigma_normal=sn, sigma_depth=sz,
                                                   variance_strength=kappa, window_radius=RADIUS)
            row["moments"][f"{sa},{sn},{sz},{kappa:g}"] = mse(out) / raw
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--jobs", type=int, default=7)
    a = ap.parse_args()
    from test_denoise_host import DENOISE_CROPS
    with multiprocessing.get_context("spawn").Pool(a.jobs) as pool:
        rows = pool.map(one_crop, DENOISE_CROPS)
    geo_of = lambda f: float(np.exp(np.mean([np.log(f(r)) for r in rows])))
    keys = list(rows[0]["moments"])
    geo = {k: geo_of(lambda r, k=k: r["moments"][k]) for k in keys}
    best = min(keys, key=geo.get)
    res = dict(sigmas=SIGMAS, variance_strengths=KAPPAS, window_radius=RADIUS, crops=rows, geometric_mean=geo, best=best,
               geometric_mean_plain_r8=geo_of(lambda r: r["plain_r8"]), geometric_mean_plain_r10=geo_of(lambda r: r["plain_r10"]),
               geometric_mean_guided_r10=geo_of(lambda r: r["guided_r10"]))
    for r in rows:
        print(f"{r['crop']:28s} raw {r['mse_raw']:.4g}  plain r8 {r['plain_r8']:.4f}  r10 {r['plain_r10']:.4f}  guided r10 {r['guided_r10']:.4f}  moments[{best}] {r['moments'][best]:.4f}")
    for k in keys:
        print(f"{k:24s} {geo[k]:.4f}")
    print("best", best, "geometric mean", geo[best], "plain r8", res["geometric_mean_plain_r8"], "plain r10", res["geometric_mean_plain_r10"], "guided r10",
          res["geometric_mean_guided_r10"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
