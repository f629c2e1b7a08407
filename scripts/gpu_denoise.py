"""The denoiser's measurements ("Denoising"): python scripts/gpu_denoise.py [--out FILE]

  - filter time by device events on the context's stream (median after warm-up) at 600 x 600, 1200 x 800 and 4096 x 4096, with the default
    options and with window_radius 7; the frames are synthetic noise of the right size (the filter's time does not depend on the data);
  - per scene (book-1 1200 x 800, Cornell 600 x 600), against a reference frame of --ref-spp samples from another seed: the MSE of the raw
    16-spp mean, of its filtered mean, and of the raw mean of a frame given the SAME total time in extra samples
    (16 + filter time / time per sample, rounded up to a whole sample: in the raw frame's favour).
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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rta
    pkg = rta.load()
    stream = torch.cuda.Stream()
    ctx = pkg.Context(0, stream=stream.cuda_stream)          # the library's kernels run on this stream: torch events bracket them
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def filter_ms(rgb, sq, W, H, n, opts, reps):
        out = torch.empty(W * H * 3, dtype=torch.float32, device="cuda")
        for _ in range(3):
            ctx.denoise(rgb, sq, W, H, samples=n, options=opts, out=out)
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.denoise(rgb, sq, W, H, samples=n, options=opts, out=out)
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)

    g = torch.Generator(device="cuda"); g.manual_seed(7)
    for W, H in ((600, 600), (1200, 800), (4096, 4096)):
        smp = 0.5 + 0.2 * torch.randn((W * H * 3, 16), device="cuda", generator=g)
        rgb, sq = smp.sum(dim=1).contiguous(), (smp * smp).sum(dim=1).contiguous()
        del smp
        for label, opts in (("defaults", pkg.denoise_options()), ("r7", pkg.denoise_options(window_radius=7))):
            med, lo, hi = filter_ms(rgb, sq, W, H, 16, opts, a.reps if W < 4096 else max(5, a.reps // 3))
            emit(kind="filter_time", width=W, height=H, options=label, median_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                 ns_per_pixel=round(med * 1e6 / (W * H), 2))

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
        m = pkg.pass_check(pkg.make_params(W, H, a.spp), 0, a.spp)
        raw = rgb.cpu().numpy().reshape(H, W, 3).astype(np.float64) / a.spp
        mse = lambda x: float(np.mean((x - ref) ** 2))   # noqa: E731
        for label, kw in (("defaults", {}), ("r7", dict(window_radius=7))):
            opts = pkg.denoise_options(samples_per_item=m, **kw)
            t_f, _, _ = filter_ms(rgb, sq, W, H, a.spp, opts, a.reps)
            out = ctx.denoise(rgb, sq, W, H, samples=a.spp, options=opts).cpu().numpy().reshape(H, W, 3).astype(np.float64)
            extra = int(np.ceil(t_f / (t16 / a.spp)))
            rgb2, _, t2 = frame(a.spp + extra)
            raw2 = rgb2.cpu().numpy().reshape(H, W, 3).astype(np.float64) / (a.spp + extra)
            emit(kind="equal_time", scene=name, width=W, height=H, options=label, spp=a.spp, render_ms=round(t16, 4), ms_per_spp=round(t16 / a.spp, 4),
                 filter_ms=round(t_f, 4), filter_in_spp=round(t_f / (t16 / a.spp), 2), equal_time_spp=a.spp + extra, equal_time_render_ms=round(t2, 4),
                 mse_raw=mse(raw), mse_filtered=mse(out), mse_equal_time_raw=mse(raw2), filtered_over_raw=round(mse(out) / mse(raw), 4),
                 filtered_over_equal_time=round(mse(out) / mse(raw2), 4), filter_beats_more_samples=bool(mse(out) < mse(raw2)))
        scene.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for kw in lines:
                f.write(json.dumps(kw) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
