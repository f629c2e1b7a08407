"""What area lights of every shape cost (RT_SCENE_LIGHTS_ALL_SHAPES, include/rt_hip.h), one JSON line per figure:
    python scripts/gpu_lights.py [--root DIR] [--config4-only]
  config4      BASELINE config 4, the Cornell box at 600 x 600 x 500 (the host mirror's scene): Msamples/s and kernel times. With --root the
               library and the package of another checkout are measured (the parent commit's, for a this-against-parent record).
  rect_lamp    examples/cornell_box.json at 600 x 600 x 500, the reference's FlipFace(XzRect) lamp and rect light, flag clear
  tri_lamp     the same box with the lamp as two triangles in the world and in the lights list, flag set: the F_LIGHTS_EXT instances
Each figure is the median of three timed renders after one warm-up, RT_FLAG_TIMING set."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--config4-only", action="store_true")
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path.insert(0, root)
import numpy as np  # noqa: E402
import rta  # noqa: E402

p = rta.load()
ctx = p.Context(0)
W = H = 600
SPP = 500


def measure(tag, desc, cam):
    scene = ctx.upload(desc)
    prm = p.make_params(W, H, SPP, flags=p._abi.RT_FLAG_TIMING)
    ctx.render(scene, cam, prm)
    runs = []
    for _ in range(3):
        img, st = ctx.render(scene, cam, prm)
        runs.append(st)
    st = sorted(runs, key=lambda s: s["render_ms"])[1]
    print(json.dumps(dict(tag=tag, root=os.path.basename(root) or root, width=W, height=H, spp=SPP, render_ms=round(st["render_ms"], 2),
                          msamples_per_s=round(W * H * SPP / st["render_ms"] / 1e3, 1), k_extend_ms=round(st["extend_ms"], 2), k_shade_ms=round(st["shade_ms"], 2),
                          drain_ms=round(st["drain_ms"], 2), segments=st["segments"], finite=bool(np.isfinite(img).all()))), flush=True)
    scene.close()


hs = p.HostScene("cornell", 0)
measure("config4", hs.desc, hs.camera(1.0))
if not args.config4_only:
    doc = json.load(open(os.path.join(root, "examples", "cornell_box.json")))
    js = p.JsonScene(doc)
    measure("rect_lamp", js.desc, js.camera(1.0))
    doc["objects"]["lamp_a"] = {"triangle": [[213, 554, 227], [343, 554, 332], [213, 554, 332]], "material": "light"}
    doc["objects"]["lamp_b"] = {"triangle": [[213, 554, 227], [343, 554, 227], [343, 554, 332]], "material": "light"}
    doc["world"] = {"list": ["left", "right", "lamp_a", "lamp_b", "floor", "ceiling", "back", "block_placed", "ball"]}
    doc["lights"] = ["lamp_a", "lamp_b", "light_ball"]
    doc["lights_all_shapes"] = True
    js = p.JsonScene(doc)
    assert p.compile_info(js.desc)["features"] & p._abi.RT_FEATURE_LIGHTS_EXT
    measure("tri_lamp", js.desc, js.camera(1.0))
ctx.close()
