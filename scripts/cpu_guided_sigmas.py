"""The guided filter's default sigmas, measured on the CPU ("Denoising"): python scripts/cpu_guided_sigmas.py [--out FILE]
For each of the seven crops of tests/test_denoise_host.py: 16-spp sums by the f64 checker, a 4-sample feature set by tests/guided.py, and
the numpy restatement nlm_guided_reference over the grid sigma_albedo x sigma_normal x sigma_depth; the default is the triple with the
smallest geometric mean of guided MSE / raw MSE. Neither the checker nor the restatement is the code under test."""
import argparse
import itertools
import json
import multiprocessing
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRID = dict(sigma_albedo=(0.05, 0.1, 0.2), sigma_normal=(0.1, 0.25, 0.5), sigma_depth=(0.05, 0.1, 0.2))


def one_crop(job):
    name, crop = job
    import rta
    pkg = rta.load()
    from oracle import binding as orc
    import crops as K
    import guided as G
    from test_denoise_host import DENOISE_SPP, oracle_crop_sums
    tmp = tempfile.mkdtemp()
    truth = K.load_golden(name)[crop] / K.CONFIGS[name]["spp"]
    S, Q = oracle_crop_sums(pkg, orc, name, crop, tmp)
    a, n, d, h = G.crop_feature_sums(pkg, orc, name, crop, tmp)
    mse = lambda img: float(np.mean((img - truth) ** 2))
    raw = mse(S.astype(np.float64) / DENOISE_SPP)
    row = dict(crop=f"{name}/{crop}", mse_raw=raw, plain=mse(pkg.nlm_reference(S, Q, DENOISE_SPP, 1)) / raw, hit_fraction=float(h.mean()) / G.FEATURE_SAMPLES, guided={})
    for sa, sn, sz in itertools.product(*GRID.values()):
        out = pkg.nlm_guided_reference(S, Q, DENOISE_SPP, 1, G.FEATURE_SAMPLES, a, n, d, h, sigma_albedo=sa, sigma_normal=sn, sigma_depth=sz)
        row["guided"][f"{sa},{sn},{sz}"] = mse(out) / raw
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--jobs", type=int, default=7)
    a = ap.parse_args()
    from test_denoise_host import DENOISE_CROPS
    with multiprocessing.get_context("spawn").Pool(a.jobs) as pool:
        rows = pool.map(one_crop, DENOISE_CROPS)
    keys = list(rows[0]["guided"])
    geo = {k: float(np.exp(np.mean([np.log(r["guided"][k]) for r in rows]))) for k in keys}
    best = min(keys, key=geo.get)
    res = dict(grid=GRID, crops=rows, geometric_mean=geo, best=best, geometric_mean_plain=float(np.exp(np.mean([np.log(r["plain"]) for r in rows]))))
    for r in rows:
        print(f"{r['crop']:28s} raw {r['mse_raw']:.4g}  plain {r['plain']:.4f}  guided[{best}] {r['guided'][best]:.4f}")
    print("best", best, "geometric mean", geo[best], "plain", res["geometric_mean_plain"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
