"""What an environment map costs: the map-lit gallery of tests/environment.py at 600 x 600 under a sampled map, an unsampled map and a constant
background, Msamples/s each (best of --repeat renders after one warm-up; measured numbers, not thresholds).

    python scripts/gpu_environment.py [--spp 32] [--repeat 5] [--map 1024x512] [--out profiles/r18_environment.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--size", type=int, default=600)
    ap.add_argument("--map", default="1024x512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_environment.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (first: the process shares torch's HIP runtime)
    import rta
    import environment as EV
    pkg = rta.load()
    W, H = (int(x) for x in a.map.split("x"))
    rgb = EV.sun_map(W=W, H=H, at=(H // 4, W // 3))
    desc, keep = EV.gallery_scene(pkg)
    cam = EV.gallery_camera(pkg)
    prm = pkg.make_params(a.size, a.size, a.spp, max_depth=50, seed=1)
    ctx = pkg.Context(0)
    out = dict(scene="tests/environment.py gallery_scene", width=a.size, height=a.size, spp=a.spp, max_depth=50, map=a.map, repeat=a.repeat, configs={})
    for name, env in (("sampled_map", pkg.EnvMap(rgb, sampled=True, scale=0.5)), ("unsampled_map", pkg.EnvMap(rgb, sampled=False, scale=0.5)), ("constant_background", None)):
        scene = ctx.upload(desc, env_map=env) if env is not None else ctx.upload(desc)
        try:
            ctx.render(scene, cam, prm)
            runs = []
            for _ in range(a.repeat):
                img, st = ctx.render(scene, cam, prm)
                runs.append(st["render_ms"])
        finally:
            scene.close()
        n = a.size * a.size * a.spp
        out["configs"][name] = dict(render_ms=runs, msamples_per_s=n / (min(runs) * 1e-3) / 1e6, segments_per_sample=st["segments"] / st["samples"],
                                    mean_radiance=float(np.asarray(img, dtype=np.float64).mean() / a.spp))
        print(name, out["configs"][name])
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
