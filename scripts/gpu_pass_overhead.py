"""What rendering a frame in passes costs (rt_render_pass_device, include/rt_hip.h): the bench frame (book-1, 1200 x 800 x 500) as 1, 5
and 25 equal passes, with and without sq_sum, against one rt_render_device; wall time of the whole series, median of `--reps`. Every
series must leave the one-shot frame bit for bit (checked). Prints one JSON line per case.

    python scripts/gpu_pass_overhead.py [--reps 5] [--out pass_overhead.jsonl]"""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (before the library: one HIP runtime, tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import rta
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = rta.load()
    W, H, SPP = 1200, 800, a.spp
    hs = pkg.HostScene("book1", 1)
    ctx = pkg.Context(0)
    scene = ctx.upload(hs.desc)
    cam = hs.camera(W / H)
    prm = pkg.make_params(W, H, SPP)
    n = pkg.output_floats(prm)
    ref = torch.zeros(n, dtype=torch.float32, device="cuda")
    rgb = torch.zeros(n, dtype=torch.float32, device="cuda")
    sq = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):                                          # warm-up
        ctx.render_device(scene, cam, prm, ref.data_ptr())

    def one_shot():
        t = time.perf_counter()
        ctx.render_device(scene, cam, prm, ref.data_ptr())
        return (time.perf_counter() - t) * 1e3

    def series(k, with_sq):
        per = SPP // k
        p = pkg._abi.RtParams.from_buffer_copy(prm)
        p.samples_per_pixel = per
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(k):
            ctx.render_pass(scene, cam, p, i * per, SPP, i > 0, rgb, sq if with_sq else None)
        return (time.perf_counter() - t) * 1e3

    rows = []
    base = float(np.median([one_shot() for _ in range(a.reps)]))
    rows.append(dict(case="rt_render_device", passes=1, sq_sum=False, ms=round(base, 2)))
    for k in (1, 5, 25):
        for with_sq in (False, True):
            ms = float(np.median([series(k, with_sq) for _ in range(a.reps)]))
            same = bool(torch.equal(rgb, ref))
            rows.append(dict(case="rt_render_pass_device", passes=k, sq_sum=with_sq, ms=round(ms, 2), vs_one_shot=round(ms / base - 1, 4),
                             per_extra_pass=round((ms / base - 1) / max(k - 1, 1), 4) if k > 1 else None, bit_identical=same))
            assert same, rows[-1]
    lines = [json.dumps(dict(r, frame=f"{W}x{H}x{SPP}", reps=a.reps)) for r in rows]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    scene.close()
    ctx.close()


if __name__ == "__main__":
    main()
