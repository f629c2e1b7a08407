"""The guided denoiser's measurements ("Denoising"): python scripts/gpu_denoise_guided.py [--out FILE]

  - filter time of rt_denoise_guided_device beside rt_denoise_device in the same process, by device events on the context's stream (median
    after warm-up), at 600 x 600 and 1200 x 800, with the default options and with window_radius 7; synthetic noise of the right size;
  - per scene (book-1 1200 x 800, Cornell 600 x 600), against a reference frame of --ref-spp samples from another seed: the MSE of the raw
    16-spp mean, of the plain and of the guided filter (4 feature samples), and of the raw mean of a frame given the same total time —
    filter plus feature pass — in extra samples (rounded up to a whole sample: in the raw frame's favour).
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
    for W, H in ((600, 600), (1200, 800)):
        smp = 0.5 + 0.2 * torch.randn((W * H * 3, 16), device="cuda", generator=g)
        rgb, sq = smp.sum(dim=1).contiguous(), (smp * smp).sum(dim=1).contiguous()
        del smp
        guide = dict(albedo=nf * torch.rand(W * H * 3, device="cuda", generator=g), normal=nf * (2 * torch.rand(W * H * 3, device="cuda", generator=g) - 1),
                     depth=nf * (1 + 9 * torch.rand(W * H, device="cuda", generator=g)), hits=torch.full((W * H,), nf, dtype=torch.int32, device="cuda"))
        out = torch.empty(W * H * 3, dtype=torch.float32, device="cuda")
        for label, opts in (("defaults", pkg.denoise_options()), ("r7", pkg.denoise_options(window_radius=7))):
            p = timed(lambda: ctx.denoise(rgb, sq, W, H, samples=16, options=opts, out=out), a.reps)
            q = timed(lambda: ctx.denoise_guided(rgb, sq, W, H, nf, samples=16, options=opts, out=out, **guide), a.reps)
            emit(kind="filter_time", width=W, height=H, options=label, plain_median_ms=round(p[0], 4), plain_min_ms=round(p[1], 4), plain_max_ms=round(p[2], 4),
                 guided_median_ms=round(q[0], 4), guided_min_ms=round(q[1], 4), guided_max_ms=round(q[2], 4), guided_over_plain=round(q[0] / p[0], 4))

    for name, sarg, W, H in (("book1", 1, 1200, 800), ("cornell", 0, 600, 600)):
        hs = pkg.HostScene(name, sarg)
        scene = ctx.upload(hs.desc)
        cam = hs.camera(W / H)
        ref, _ = ctx.render(scene, cam, pkg.make_params(W, H, a.ref_spp, max_depth=50, seed=99))
        ref = ref.astype(np.float64) / a.ref_spp
        n = W * H * 3

        def frame(spp):
            prm = pkg.make_params(W, H, spp, max_depth=50, seed=1)
            rgb = torch.zeros(n, dtype=torch.float32, device="cuda"); sq = torch.zeros(n, dtype=torch.float32, device="cuda")
            best = None
            for _ in range(5):                                   # the pass's own device time, best of 5
                _, _, st = ctx.render_pass(scene, cam, prm, 0, spp, False, rgb, sq)
                best = st["render_ms"] if best is None else min(best, st["render_ms"])
            return rgb, sq, best

        rgb, sq, t16 = frame(a.spp)
        prm = pkg.make_params(W, H, a.spp, max_depth=50, seed=1)
        m = pkg.pass_check(prm, 0, a.spp)
        fprm = pkg.make_params(W, H, nf, max_depth=50, seed=1)
        t_feat = min(ctx.render_features(scene, cam, fprm, with_stats=True)[4]["render_ms"] for _ in range(5))
        guide = render_guide(ctx, scene, cam, prm, nf)
        raw = rgb.cpu().numpy().reshape(H, W, 3).astype(np.float64) / a.spp
        mse = lambda x: float(np.mean((x - ref) ** 2))   # noqa: E731
        for label, kw in (("defaults", {}), ("r7", dict(window_radius=7))):
            opts = pkg.denoise_options(samples_per_item=m, **kw)
            t_p = timed(lambda: ctx.denoise(rgb, sq, W, H, samples=a.spp, options=opts), a.reps)[0]
            t_g = timed(lambda: ctx.denoise_guided(rgb, sq, W, H, samples=a.spp, options=opts, **guide), a.reps)[0]
            plain = ctx.denoise(rgb, sq, W, H, samples=a.spp, options=opts).cpu().numpy().reshape(H, W, 3).astype(np.float64)
            out = ctx.denoise_guided(rgb, sq, W, H, samples=a.spp, options=opts, **guide).cpu().numpy().reshape(H, W, 3).astype(np.float64)
            extra = int(np.ceil((t_g + t_feat) / (t16 / a.spp)))
            rgb2, _, t2 = frame(a.spp + extra)
            raw2 = rgb2.cpu().numpy().reshape(H, W, 3).astype(np.float64) / (a.spp + extra)
            emit(kind="equal_time", scene=name, width=W, height=H, options=label, spp=a.spp, feature_samples=nf, render_ms=round(t16, 4),
                 ms_per_spp=round(t16 / a.spp, 4), plain_filter_ms=round(t_p, 4), guided_filter_ms=round(t_g, 4), feature_pass_ms=round(t_feat, 4),
                 guided_in_spp=round((t_g + t_feat) / (t16 / a.spp), 2), equal_time_spp=a.spp + extra, equal_time_render_ms=round(t2, 4), mse_raw=mse(raw),
                 mse_plain=mse(plain), mse_guided=mse(out), mse_equal_time_raw=mse(raw2), guided_over_raw=round(mse(out) / mse(raw), 4),
                 plain_over_raw=round(mse(plain) / mse(raw), 4), guided_over_equal_time=round(mse(out) / mse(raw2), 4),
                 guided_beats_more_samples=bool(mse(out) < mse(raw2)), guided_beats_plain=bool(mse(out) < mse(plain)))
        scene.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for kw in lines:
                f.write(json.dumps(kw) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
