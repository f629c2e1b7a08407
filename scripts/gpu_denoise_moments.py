"""The variance-guided denoiser's measurements ("Denoising"): python scripts/gpu_denoise_moments.py [--out FILE]

  - filter time of rt_denoise_guided_moments_device beside rt_denoise_guided_device and rt_denoise_device at the same window and patch
    radius, in one process, by device events on the context's stream (median after warm-up), at 600 x 600 and 1200 x 800; synthetic noise;
  - the cost of the moments fold: rt_render_feature_moments_device beside rt_render_features_device at 1200 x 800 x 4 (book-1), the whole
    pass and the fold kernel alone (RT_FLAG_TIMING), medians;
  - per scene (book-1 1200 x 800, Cornell 600 x 600), against a reference frame of --ref-spp samples from another seed: the MSE of the raw
    16-spp mean, of the plain filter, of the guided filter and of the variance-guided filter (4 feature samples), each with its defaults.
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # noqa: F401  (first: see tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--feature-samples", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rta
    pkg = rta.load()
    A = pkg._abi
    from ray_tracer_archive_amd.denoise import render_guide
    stream = torch.cuda.Stream()
    ctx = pkg.Context(0, stream=stream.cuda_stream)          # the library's kernels run on this stream: torch events bracket them
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def timed(call, reps):
        for _ in range(3):
            call()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)

    g = torch.Generator(device="cuda"); g.manual_seed(7)
    nf = a.feature_samples
    rnd = lambda n: torch.rand(n, device="cuda", generator=g)   # noqa: E731
    for W, H in ((600, 600), (1200, 800)):
        smp = 0.5 + 0.2 * torch.randn((W * H * 3, 16), device="cuda", generator=g)
        rgb, sq = smp.sum(dim=1).contiguous(), (smp * smp).sum(dim=1).contiguous()
        del smp
        n1, n3 = W * H, W * H * 3
        albedo, normal, depth = nf * rnd(n3), nf * (2 * rnd(n3) - 1), nf * (1 + 9 * rnd(n1))
        sums = dict(albedo=albedo, normal=normal, depth=depth, hits=torch.full((n1,), nf, dtype=torch.int32, device="cuda"))
        squares = dict(albedo_sq=albedo * albedo / nf * (1 + 0.1 * rnd(n3)), normal_sq=normal * normal / nf * (1 + 0.1 * rnd(n3)), depth_sq=depth * depth / nf * (1 + 0.01 * rnd(n1)))
        out = torch.empty(n3, dtype=torch.float32, device="cuda")
        for label, kw in (("r8_f3", dict(window_radius=8)), ("r8_f4", dict(window_radius=8, patch_radius=4)), ("r3_f1", dict(window_radius=3, patch_radius=1))):
            opts = pkg.denoise_options(**kw)
            p = timed(lambda: ctx.denoise(rgb, sq, W, H, samples=16, options=opts, out=out), a.reps)
            q = timed(lambda: ctx.denoise_guided(rgb, sq, W, H, nf, samples=16, options=opts, out=out, **sums), a.reps)
            m = timed(lambda: ctx.denoise_guided_moments(rgb, sq, W, H, nf, samples=16, options=opts, out=out, **sums, **squares), a.reps)
            emit(kind="filter_time", width=W, height=H, options=label, plain_median_ms=round(p[0], 4), guided_median_ms=round(q[0], 4), guided_min_ms=round(q[1], 4),
                 guided_max_ms=round(q[2], 4), moments_median_ms=round(m[0], 4), moments_min_ms=round(m[1], 4), moments_max_ms=round(m[2], 4),
                 moments_over_guided=round(m[0] / q[0], 4), moments_over_plain=round(m[0] / p[0], 4))

    for name, sarg, W, H in (("book1", 1, 1200, 800), ("cornell", 0, 600, 600)):
        hs = pkg.HostScene(name, sarg)
        scene = ctx.upload(hs.desc)
        cam = hs.camera(W / H)
        if name == "book1":
            fprm = pkg.make_params(W, H, nf, max_depth=50, seed=1, flags=A.RT_FLAG_TIMING)
            slots = W * H
            planes = [torch.zeros(c * slots, dtype=torch.int32 if i == 3 else torch.float32, device="cuda") for i, c in enumerate((3, 3, 1, 1, 3, 3, 1))]
            keys = ("albedo", "normal", "depth", "hits", "albedo_sq", "normal_sq", "depth_sq")
            rows = {"features": [], "moments": []}
            for _ in range(3 + a.reps):                          # alternating, so that clocks and caches treat both alike
                rows["features"].append(ctx.render_features(scene, cam, fprm, with_stats=True, **dict(zip(keys[:4], planes[:4])))[4])
                rows["moments"].append(ctx.render_feature_moments(scene, cam, fprm, with_stats=True, **dict(zip(keys, planes)))[7])
            med = lambda which, f: statistics.median(f(st) for st in rows[which][3:])   # noqa: E731
            total = lambda st: st["extend_ms"] + st["other_ms"]                         # noqa: E731  (the kernels of the pass, by device events)
            fold = lambda st: st["debug"][2] / 1000.0                                   # noqa: E731
            emit(kind="fold_cost", scene=name, width=W, height=H, feature_samples=nf, features_kernels_ms=round(med("features", total), 4),
                 moments_kernels_ms=round(med("moments", total), 4), features_fold_ms=round(med("features", fold), 4), moments_fold_ms=round(med("moments", fold), 4),
                 moments_over_features_pass=round(med("moments", total) / med("features", total), 4),
                 moments_over_features_fold=round(med("moments", fold) / max(med("features", fold), 1e-9), 4))
        ref, _ = ctx.render(scene, cam, pkg.make_params(W, H, a.ref_spp, max_depth=50, seed=99))
        ref = ref.astype(np.float64) / a.ref_spp
        n = W * H * 3
        prm = pkg.make_params(W, H, a.spp, max_depth=50, seed=1)
        rgb = torch.zeros(n, dtype=torch.float32, device="cuda"); sq = torch.zeros(n, dtype=torch.float32, device="cuda")
        ctx.render_pass(scene, cam, prm, 0, a.spp, False, rgb, sq)
        m = pkg.pass_check(prm, 0, a.spp)
        guide, guide_m = render_guide(ctx, scene, cam, prm, nf), render_guide(ctx, scene, cam, prm, nf, moments=True)
        raw = rgb.cpu().numpy().reshape(H, W, 3).astype(np.float64) / a.spp
        mse = lambda x: float(np.mean((x.cpu().numpy().reshape(H, W, 3).astype(np.float64) - ref) ** 2))   # noqa: E731
        opts = pkg.denoise_options(samples_per_item=m)
        r8 = pkg.denoise_options(samples_per_item=m, window_radius=8)
        mse_raw = float(np.mean((raw - ref) ** 2))
        t_g = timed(lambda: ctx.denoise_guided(rgb, sq, W, H, samples=a.spp, options=opts, **guide), a.reps)[0]
        t_m = timed(lambda: ctx.denoise_guided_moments(rgb, sq, W, H, samples=a.spp, options=opts, **guide_m), a.reps)[0]
        res = dict(plain_r10=mse(ctx.denoise(rgb, sq, W, H, samples=a.spp, options=opts)), plain_r8=mse(ctx.denoise(rgb, sq, W, H, samples=a.spp, options=r8)),
                   guided_r10=mse(ctx.denoise_guided(rgb, sq, W, H, samples=a.spp, options=opts, **guide)),
                   guided_r8=mse(ctx.denoise_guided(rgb, sq, W, H, samples=a.spp, options=r8, **guide)),
                   moments_r8=mse(ctx.denoise_guided_moments(rgb, sq, W, H, samples=a.spp, options=opts, **guide_m)))
        emit(kind="frame_error", scene=name, width=W, height=H, spp=a.spp, feature_samples=nf, mse_raw=mse_raw, guided_r10_filter_ms=round(t_g, 4),
             moments_r8_filter_ms=round(t_m, 4), **{k + "_over_raw": round(v / mse_raw, 4) for k, v in res.items()})
        scene.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for kw in lines:
                f.write(json.dumps(kw) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
