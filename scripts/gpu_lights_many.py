"""What many lights cost with and without RT_SCENE_LIGHTS_MANY (include/rt_hip.h), one JSON line per figure and all of them in --out:
    python scripts/gpu_lights_many.py [--out profiles/r15_lights_many.json]
  cost      examples/cornell_box.json at 600 x 600 x 500 with the LIGHTS LIST's lamp as a grid of 2, 32, 512 and 8192 triangles (the world keeps
            the reference's rect lamp, so the walk is the same in every row and only the light sampler changes); the grid's cells are equal, so both
            picks are uniform over the lamp and the paths are statistically the same. Flag 1
            (RT_SCENE_LIGHTS_ALL_SHAPES: uniform pick, every member's pdf per bounce) and flag 5 (area-weighted pick, light tree). k_shade and
            k_extend ms, median of three renders after a warm-up, RT_FLAG_TIMING. The row (flag 1, 8192) is rendered ONCE at 25 spp and its times
            are multiplied by 20 (`scaled`: true): at full size a single launch of k_shade would run for many seconds.
  variance  the same box, the lights list's lamp as one large triangle (half the rect) and 62 slivers (the other half), 200 x 200 x 64: the median
            per-pixel standard error of the mean (channel 0) under flag 1 and under flag 5 — what the weighted pick buys.
  variance_with_ball  the same with the reference's glass ball in the list too (main.rs:669-684 lists it for its caustic): the ball's area is 7.5 times
            the lamp's and it emits nothing, so a pick by AREA spends 88 % of the light samples on it — the weight is not emitted power."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
args = ap.parse_args()
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np  # noqa: E402
import rta  # noqa: E402

p = rta.load()
A = p._abi
ctx = p.Context(0)
X0, X1, Z0, Z1, Y = 213.0, 343.0, 227.0, 332.0, 554.0


def grid(cells):
    xs, zs = np.linspace(X0, X1, cells[0] + 1), np.linspace(Z0, Z1, cells[1] + 1)
    out = []
    for i in range(cells[0]):
        for j in range(cells[1]):
            x0, x1, z0, z1 = xs[i], xs[i + 1], zs[j], zs[j + 1]
            out += [[(x0, Y, z0), (x1, Y, z1), (x0, Y, z1)], [(x0, Y, z0), (x1, Y, z0), (x1, Y, z1)]]      # front (cross(v1 - v0, v2 - v0)) down
    return out


def slivers():
    """one triangle of half the rect, the other half as a fan of 62 slivers from (X0, Z0)"""
    out = [[(X0, Y, Z0), (X1, Y, Z1), (X0, Y, Z1)]]
    t = np.linspace(0.0, 1.0, 63)
    for a, b in zip(t[:-1], t[1:]):
        out.append([(X0, Y, Z0), (X1, Y, Z0 + (Z1 - Z0) * a), (X1, Y, Z0 + (Z1 - Z0) * b)])
    return out


def scene_desc(tris, many, ball=False):
    js = p.JsonScene(json.load(open(os.path.join(root, "examples", "cornell_box.json"))))
    b = js.b
    lamp = b.diffuse_light((15.0, 15.0, 15.0))
    lights = [b.triangle(*t, lamp) for t in tris] + ([b.sphere((190.0, 90.0, 190.0), 90.0, b.dielectric(1.5))] if ball else [])
    desc = b.desc(js.desc.world, b.hittable_list(lights), lights_all_shapes=True, lights_many=many)
    assert bool(p.compile_info(desc)["features"] & A.RT_FEATURE_LIGHTS_TREE) == many
    return desc, js


rows = []


def emit(row):
    rows.append(row)
    print(json.dumps(row), flush=True)


for cells in ((1, 1), (4, 4), (16, 16), (64, 64)):
    tris = grid(cells)
    for many in (False, True):
        desc, js = scene_desc(tris, many)
        scene = ctx.upload(desc)
        heavy = not many and len(tris) >= 8192
        spp, scale = (25, 20.0) if heavy else (500, 1.0)
        prm = p.make_params(600, 600, spp, flags=A.RT_FLAG_TIMING)
        runs = []
        if not heavy:
            ctx.render(scene, js.camera(1.0), prm)
        for _ in range(1 if heavy else 3):
            img, st = ctx.render(scene, js.camera(1.0), prm)
            runs.append(st)
        st = sorted(runs, key=lambda s: s["render_ms"])[len(runs) // 2]
        emit(dict(tag="cost", triangles=len(tris), lights=len(tris), scene_flags=5 if many else 1, width=600, height=600, spp=500, scaled=heavy,
                  render_ms=round(st["render_ms"] * scale, 2), k_shade_ms=round(st["shade_ms"] * scale, 2), k_extend_ms=round(st["extend_ms"] * scale, 2),
                  drain_ms=round(st["drain_ms"] * scale, 2), segments=int(st["segments"] * scale), finite=bool(np.isfinite(img).all())))
        scene.close()

W, SPP = 200, 64
for ball, many in ((False, False), (False, True), (True, False), (True, True)):
    desc, js = scene_desc(slivers(), many, ball)
    scene = ctx.upload(desc)
    n = W * W * 3
    rgb, sq, st = ctx.render_pass(scene, js.camera(1.0), p.make_params(W, W, SPP, seed=3), 0, SPP, False, rgb_sum=np.zeros(n, np.float32), sq_sum=np.zeros(n, np.float32))
    S, Q = np.asarray(rgb, np.float64).reshape(W, W, 3)[..., 0], np.asarray(sq, np.float64).reshape(W, W, 3)[..., 0]
    se = np.sqrt(np.maximum(Q - S * S / SPP, 0.0) / (SPP * (SPP - 1.0)))
    emit(dict(tag="variance_with_ball" if ball else "variance", lights=64 if ball else 63, scene_flags=5 if many else 1, width=W, height=W, spp=SPP, median_standard_error=float(np.median(se)),
              mean_standard_error=float(se.mean()), mean_radiance=float((S / SPP).mean())))
    scene.close()
ctx.close()
if args.out:
    what = ("scripts/gpu_lights_many.py on an MI355X: the Cornell box at 600 x 600 x 500 with the lights list's lamp as a grid of triangles, scene_flags 1 "
            "(uniform pick, linear pdf) against 5 (area-weighted pick, light tree); and the per-pixel standard error at 200 x 200 x 64 with a lamp of one "
            "large triangle and 62 slivers")
    json.dump(dict(what=what, rows=rows), open(args.out, "w"), indent=1)
