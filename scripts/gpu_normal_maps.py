"""What normal maps cost on one MI355X, and that they cost nothing where there is none:
    python scripts/gpu_normal_maps.py [--parent-lib /path/to/the/parent's/librt_hip.so] [--out profiles/r20_normal_maps.json]

  map        a subdivision-4 sphere mesh (5120 triangles, sphere normals and the sphere's (u, v), grey Lambertian under the sky gradient) with a
             256 x 128 map made from a height field (mesh.height_to_normal_map) against the same upload without it: 512 x 512 x 64 spp, best of
             three renders each, Msamples/s and the kernel times
  --parent-lib: the same library built from the parent commit. Three runs of each, alternating, of
  bench      bench.py --gpus 1 (the headline), with the frames of the last timed step compared byte for byte
  attrs      scripts/gpu_mesh_attrs.py (the attribute scenes, which carry no map)
Every run is a process of its own under a time limit; the first that fails ends the script."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def run(cmd, lib, limit):
    env = dict(os.environ)
    if lib:
        env["RT_HIP_LIB"] = lib
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def map_cost():
    import rta
    p = rta.load()
    A = p._abi
    W = H = 512
    SPP = 64
    b = p.SceneBuilder(background=(0.5, 0.7, 1.0), background_mode=A.RT_BG_SKY_GRADIENT, bvh_builder=A.RT_BVH_SAH)
    grey = b.lambertian((0.6, 0.6, 0.6))
    tris, nrm = p.icosphere(4)
    uv = p.sphere_uv(nrm)
    ids = [b.triangle(tris[k][0], tris[k][1], tris[k][2], grey, normals=nrm[k], uvs=uv[k]) for k in range(len(tris))]
    y, x = np.mgrid[0:128, 0:256]
    height = 0.5 * np.sin(2 * np.pi * x / 16.0) * np.sin(2 * np.pi * y / 16.0)
    b.normal_map(grey, p.height_to_normal_map(height, 2.0))
    desc = b.desc(b.bvh(ids))
    cam = p.camera_new((0.3, 0.4, 4.0), (0, 0, 0), (0, 1, 0), 32.0, 1.0, 0.0, 4.0, 0.0, 0.0)
    ctx = p.Context(0)
    out = {"mesh": f"icosphere(4): {len(tris)} triangles, sphere normals and uv, Lambertian, SAH; map 256 x 128 from a height field", "width": W, "height": H, "spp": SPP}
    frames = {}
    for tag, maps in (("unmapped", None), ("mapped", b.normal_maps())):
        info = p.compile_info(desc, triangle_attrs=b.triangle_attrs(), normal_maps=maps)
        scene = ctx.upload(desc, triangle_attrs=b.triangle_attrs(), normal_maps=maps)
        ctx.render(scene, cam, p.make_params(W, H, SPP))
        best = None
        for _ in range(3):
            t = time.time(); img, st = ctx.render(scene, cam, p.make_params(W, H, SPP, flags=A.RT_FLAG_TIMING)); dt = time.time() - t
            if best is None or dt < best[0]:
                best = (dt, st)
        dt, st = best
        frames[tag] = img
        out[tag] = dict(features=info["features"], n_tri_attrs=info["n_tri_attrs"], seconds=round(dt, 4), msamples_per_s=round(W * H * SPP / dt / 1e6, 1),
                        extend_ms=round(st["extend_ms"], 2), shade_ms=round(st["shade_ms"], 2), drain_ms=round(st["drain_ms"], 2),
                        segments_per_sample=round(st["segments"] / st["samples"], 3), mean_level=round(float(img.mean()) / SPP, 5))
        print(tag, out[tag], flush=True)
        scene.close()
    out["mean_abs_difference"] = round(float(np.abs(frames["mapped"] - frames["unmapped"]).mean()) / SPP, 5)
    out["mapped_over_unmapped"] = round(out["mapped"]["msamples_per_s"] / out["unmapped"]["msamples_per_s"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-attrs", action="store_true")
    args = ap.parse_args()
    out = {"map": map_cost()}
    if args.parent_lib:
        parent = os.path.abspath(args.parent_lib)
        with tempfile.TemporaryDirectory() as tmp:
            runs = {"this": [], "parent": []}
            for k in range(3):
                for tag, lib in (("parent", parent), ("this", None)):
                    r = run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3", "--dump-outputs", os.path.join(tmp, tag)], lib, 300)
                    runs[tag].append(r["value"])
                    print("bench", tag, r["value"], flush=True)
            same = open(os.path.join(tmp, "this", "rgb_sum.npy"), "rb").read() == open(os.path.join(tmp, "parent", "rgb_sum.npy"), "rb").read()
        out["bench"] = dict(unit="Msamples/s", this=runs["this"], parent=runs["parent"], frames_equal=same,
                            parent_spread=round(max(runs["parent"]) - min(runs["parent"]), 3),
                            median_this_minus_parent=round(float(np.median(runs["this"]) - np.median(runs["parent"])), 3))
        print(out["bench"], flush=True)
        if not args.skip_attrs:
            runs = {"this": [], "parent": []}
            for k in range(3):
                for tag, lib in (("parent", parent), ("this", None)):
                    r = run([sys.executable, "scripts/gpu_mesh_attrs.py"], lib, 400)
                    runs[tag].append({q: r[q]["msamples_per_s"] for q in ("flat", "smooth")})
                    print("attrs", tag, runs[tag][-1], flush=True)
            out["attrs"] = dict(unit="Msamples/s", scene=r["mesh"], this=runs["this"], parent=runs["parent"])
            for q in ("flat", "smooth"):
                pv, tv = [x[q] for x in runs["parent"]], [x[q] for x in runs["this"]]
                out["attrs"][q] = dict(parent_spread=round(max(pv) - min(pv), 2), median_this_minus_parent=round(float(np.median(tv) - np.median(pv)), 2))
            print(out["attrs"], flush=True)
    print(json.dumps(out))
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
