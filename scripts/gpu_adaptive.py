"""Adaptive sampling against uniform passes: python scripts/gpu_adaptive.py [--frame 512] [--pass-samples 32] [--rel 0.05]

Per scene (Cornell 600 x 600, book-1 1200 x 800):
  - Adaptive to the target (every pixel's SE <= rel_error * mean + abs_error, or the frame budget): samples traced, wall time;
  - a uniform Progressive with the same passes that stops when its WORST pixel meets the same criterion (rt_adaptive_select on counts that
    all equal the samples done: an empty list), or at the budget: samples traced, wall time;
  - an all-pixels list pass against a plain pass of the same samples (Msamples/s);
  - rt_adaptive_select per call (ms; it blocks until its three kernels are done).
Prints one JSON line per scene."""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (first: see tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", type=int, default=512)
    ap.add_argument("--pass-samples", type=int, default=32)
    ap.add_argument("--min-samples", type=int, default=64)
    ap.add_argument("--rel", type=float, default=0.05)
    ap.add_argument("--abs", type=float, default=1e-3)
    ap.add_argument("--throughput-spp", type=int, default=64)
    ap.add_argument("--scenes", default="cornell,book1")
    a = ap.parse_args()
    import rta
    pkg = rta.load()
    A = pkg._abi
    ctx = pkg.Context(0)
    shapes = {"cornell": ("cornell", 0, 600, 600), "book1": ("book1", 1, 1200, 800)}
    for name in a.scenes.split(","):
        sname, sarg, W, H = shapes[name]
        hs = pkg.HostScene(sname, sarg)
        scene = ctx.upload(hs.desc)
        cam = hs.camera(W / H)
        prm = pkg.make_params(W, H, 1)
        out = dict(scene=name, width=W, height=H, frame=a.frame, pass_samples=a.pass_samples, min_samples=a.min_samples, rel_error=a.rel, abs_error=a.abs)
        # warm-up: kernels loaded, buffers grown
        pkg.Adaptive(ctx, scene, cam, prm, a.frame, min_samples=a.min_samples, rel_error=a.rel, abs_error=a.abs).run(a.pass_samples, until=2 * a.pass_samples)

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ada = pkg.Adaptive(ctx, scene, cam, prm, a.frame, min_samples=a.min_samples, rel_error=a.rel, abs_error=a.abs)
        ada.run(a.pass_samples)
        t_ada = time.perf_counter() - t0
        c = ada.counts()
        out["adaptive"] = dict(samples=int(ada.samples_traced), seconds=round(t_ada, 4), passes=ada.samples_done // a.pass_samples,
                               pixels_at_budget=int((c == a.frame).sum()), mean_spp=round(float(c.mean()), 2), min_spp=int(c.min()))

        # uniform passes, stopped by the worst pixel (same criterion, same device code)
        opts = pkg.adaptive_options(a.min_samples, a.rel, a.abs)
        slots = pkg.output_floats(prm) // 3
        counts = torch.zeros(slots, dtype=torch.int32, device="cuda")
        lst = torch.zeros(slots, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prog = pkg.Progressive(ctx, scene, cam, prm, a.frame)
        n_active = slots
        while not prog.done:
            prog.step(a.pass_samples)
            counts.fill_(prog.samples_done)
            n_active = ctx.adaptive_select(prog.params, opts, prog.samples_done, a.frame, prog._rgb, prog._sq, counts, lst)
            if n_active == 0:
                break
        t_uni = time.perf_counter() - t0
        out["uniform"] = dict(samples=prog.samples_done * W * H, seconds=round(t_uni, 4), spp=prog.samples_done,
                              stopped_by="budget" if n_active != 0 or prog.samples_done >= a.frame else "worst pixel")
        out["samples_ratio"] = round(out["adaptive"]["samples"] / out["uniform"]["samples"], 4)
        out["time_ratio"] = round(t_ada / t_uni, 4)

        # list-mode throughput: an all-pixels list pass against a plain pass
        spp = a.throughput_spp
        p = A.RtParams.from_buffer_copy(prm)
        p.samples_per_pixel = spp
        rgb = torch.zeros(3 * slots, dtype=torch.float32, device="cuda")
        sq = torch.zeros(3 * slots, dtype=torch.float32, device="cuda")
        allp = torch.arange(slots, dtype=torch.int32, device="cuda")
        plain, listed = [], []
        for _ in range(4):
            st = ctx.render_pass(scene, cam, p, 0, spp, False, rgb, sq)[2]
            plain.append(st["render_ms"])
            counts.zero_()
            st = ctx.render_pass_pixels(scene, cam, p, 0, spp, False, allp, slots, rgb, sq, counts)
            listed.append(st["render_ms"])
        ms_p, ms_l = sorted(plain[1:])[1], sorted(listed[1:])[1]
        out["plain_pass"] = dict(ms=round(ms_p, 3), msamples_per_s=round(W * H * spp / ms_p / 1e3, 1))
        out["list_pass_all_pixels"] = dict(ms=round(ms_l, 3), msamples_per_s=round(W * H * spp / ms_l / 1e3, 1))

        # selection cost per pass (three kernels + the length read back)
        counts.fill_(a.min_samples)
        for _ in range(3):
            ctx.adaptive_select(prm, opts, a.min_samples, a.frame, rgb, sq, counts, lst)
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            ctx.adaptive_select(prm, opts, a.min_samples, a.frame, rgb, sq, counts, lst)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        out["select_ms"] = dict(median=round(ts[len(ts) // 2], 3), min=round(ts[0], 3))
        print(json.dumps(out), flush=True)
        scene.close()
    ctx.close()


if __name__ == "__main__":
    main()
