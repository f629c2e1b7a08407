"""A fixed list of small seeded calls through whichever library RT_HIP_LIB selects (api.lib_path), for comparing two builds of the HOST
code: run it once per library, each in a fresh process, and compare the two outputs as text — they must be identical.

One JSON line per call: the crc32 of every output buffer and the RtStats fields that do not depend on host timing — samples, segments,
pool_slots, the scene's constants, n_devices, debug[6..7]; for the chunked paths (ray queries, features) also iterations and
extend_launches, which for a render depend on when the pinned ring's copies land and are never compared.

The calls: book-1 and the Cornell box rendered at 64 x 40 x 8 and 150 x 90 x 3 — unsharded, as shard 1 of 3 with tile 16, with
RT_FLAG_SAMPLE_BLOCKS, RT_FLAG_COUNTERS, tail_paths = 1 and RT_FLAG_FUSED, with pool_slots 4096; a progressive pair of passes with squared
sums and an adaptive list pass; 10 000 rays and occlusion rays on device and host variants with pool_slots 0 and 4096 (three chunks);
features and feature moments at 64 x 40 x 8 with pool_slots 0, 4096 and 4, overwriting and accumulating; book-1 uploaded with
RT_LAYOUT_SCENE_IN_HBM and with RT_LAYOUT_WIDE_NODES beside it; 256 light-sample queries, half of them with a direction given, on the
Cornell box with each kind of lights table (plain, RT_SCENE_LIGHTS_ALL_SHAPES with the lamp as two triangles, RT_SCENE_LIGHTS_MANY on
that); a radiance query of 256 rays x 4 samples on the Cornell box with one invalid ray; the three denoisers on a 64 x 40 x 8 book-1
frame with its features and moments, at patch radii 1 and 3.

--timing PATH adds, in a file of its own (never compared), the median and the range of render_ms over 20 calls after 3 warm ones of a
4096-ray rt_trace_rays_device call and a 64 x 40 x 2 rt_render_device call: a change of host code shows first in small calls.

    RT_HIP_LIB=/path/to/librt_hip.so python scripts/gpu_host_ab.py --out calls.jsonl [--timing timing.json]"""
import argparse
import json
import os
import sys
import zlib

import torch  # noqa: F401  (before the library: one HIP runtime, tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EVERY = ["samples", "segments", "pool_slots", "scene_nodes", "scene_prims", "scene_bytes", "bvh_in_lds", "lds_top_nodes", "n_devices"]
CHUNKED = ["iterations", "extend_launches"]


def camera_rays(np, cam, W, H):
    """pixel-centre rays, float32 (W * H, 8): o, time, d, t_max"""
    v3 = lambda v: np.array([v.x, v.y, v.z])
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    u = ((x + 0.5) / (W - 1)).reshape(-1, 1)
    v = ((H - 1 - y + 0.5) / (H - 1)).reshape(-1, 1)
    rays = np.zeros((W * H, 8), dtype=np.float32)
    rays[:, 0:3] = v3(cam.origin)
    rays[:, 4:7] = v3(cam.lower_left_corner) + u * v3(cam.horizontal) + v * v3(cam.vertical) - v3(cam.origin)
    return rays


def main():
    import numpy as np
    import rta
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--timing", default=None)
    args = ap.parse_args()
    pkg = rta.load()
    A = pkg._abi
    ctx = pkg.Context(0)
    dev = torch.device("cuda", 0)
    lines = []

    def crc(a):
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.ascontiguousarray(a)
        return zlib.crc32(a.tobytes())

    def record(call, outputs, st, chunked=False):
        row = {"call": call, "crc32": [crc(o) for o in outputs]}
        row.update({k: st[k] for k in EVERY + (CHUNKED if chunked else [])})
        row["debug6"], row["debug7"] = st["debug"][6], st["debug"][7]
        lines.append(json.dumps(row))

    def zeroed(kind, n):
        """zero-filled device and host outputs of a ray query"""
        if kind == "trace":
            return torch.zeros((n, 12), dtype=torch.float32, device=dev), np.zeros(n, dtype=pkg.RAYHIT_DTYPE)
        return torch.zeros(n, dtype=torch.uint8, device=dev), np.zeros(n, dtype=np.uint8)

    scenes = {"book1": pkg.HostScene("book1", 1), "cornell": pkg.HostScene("cornell", 0)}
    for name, hs in scenes.items():
        scene = ctx.upload(hs.desc)
        for W, H, spp in [(64, 40, 8), (150, 90, 3)]:
            cam = hs.camera(W / H)
            variants = {"plain": {}, "shard1of3": dict(tile_size=16, shard_index=1, shard_count=3), "blocks": dict(flags=A.RT_FLAG_SAMPLE_BLOCKS),
                        "counters": dict(flags=A.RT_FLAG_COUNTERS), "tail1": dict(tail_paths=1), "fused": dict(flags=A.RT_FLAG_FUSED), "pool4096": dict(pool_slots=4096)}
            for vn, kw in variants.items():
                img, st = ctx.render(scene, cam, pkg.make_params(W, H, spp, seed=7, **kw))
                record(f"render {name} {W}x{H}x{spp} {vn}", [img], st)
        # two passes of a progressive frame with squared sums (host variant), then an adaptive select and list pass
        W, H = 64, 40
        cam = hs.camera(W / H)
        prm = pkg.make_params(W, H, 4, seed=7)
        rgb, sq, st = ctx.render_pass(scene, cam, prm, 0, 8, False, None, np.zeros(W * H * 3, dtype=np.float32))
        rgb, sq, st = ctx.render_pass(scene, cam, prm, 4, 8, True, rgb.reshape(-1), sq.reshape(-1))
        record(f"passes {name} {W}x{H} 4+4", [rgb, sq], st)
        ada = pkg.Adaptive(ctx, scene, cam, prm, frame_samples=16, min_samples=4, rel_error=0.05)
        ada.step(4)
        st = ada.step(4)
        record(f"adaptive {name} {W}x{H} 4+4", [ada._rgb, ada._sq, ada._counts, ada._list[:ada.n_active]], st)
        # ray queries: 10 000 pixel-centre rays, every third one with a limit
        rays = camera_rays(np, hs.camera(125 / 80), 125, 80)
        rays[::3, 7] = 9.0
        d_rays = torch.from_numpy(rays).to(dev)
        for pool in (0, 4096):
            opt = pkg.ray_query_options(pool_slots=pool)
            for kind, fn in (("trace", ctx.trace_rays), ("occluded", ctx.occluded)):      # (zeroed outputs: every byte compared is one the call wrote or left)
                d_out, h_out = zeroed(kind, len(rays))
                out, st = fn(scene, d_rays, opt, out=d_out, with_stats=True)
                record(f"{kind} device {name} pool{pool}", [out], st, chunked=True)
                out, st = fn(scene, rays, opt, out=h_out, with_stats=True)
                record(f"{kind} host {name} pool{pool}", [out], st, chunked=True)
        # features and feature moments (a pool of 4 slots is rounded up to the pool's grain)
        prm = pkg.make_params(64, 40, 8, seed=7)
        for pool in (0, 4096, 4):
            for fn_name, fn in (("features", ctx.render_features), ("moments", ctx.render_feature_moments)):
                *planes, st = fn(scene, cam, prm, pool_slots=pool, with_stats=True)
                record(f"{fn_name} {name} pool{pool}", planes, st, chunked=True)
                *planes, st = fn(scene, cam, prm, 8, True, *planes, pool_slots=pool, with_stats=True)
                record(f"{fn_name} {name} pool{pool} accumulate", planes, st, chunked=True)
        scene.close()
    # layouts that do not fit LDS
    hs = scenes["book1"]
    cam = hs.camera(64 / 40)
    prm = pkg.make_params(64, 40, 8, seed=7)
    d_rays = torch.from_numpy(camera_rays(np, hs.camera(125 / 80), 125, 80)).to(dev)
    for ln, flags in (("hbm", A.RT_LAYOUT_SCENE_IN_HBM), ("hbm_wide", A.RT_LAYOUT_SCENE_IN_HBM | A.RT_LAYOUT_WIDE_NODES)):
        scene = ctx.upload(hs.desc, flags)
        img, st = ctx.render(scene, cam, prm)
        record(f"render book1 64x40x8 {ln}", [img], st)
        for kind, fn in (("trace", ctx.trace_rays), ("occluded", ctx.occluded)):
            out, st = fn(scene, d_rays, out=zeroed(kind, d_rays.shape[0])[0], with_stats=True)
            record(f"{kind} device book1 {ln}", [out], st, chunked=True)
        *planes, st = ctx.render_features(scene, cam, prm, with_stats=True)
        record(f"features book1 {ln}", planes, st, chunked=True)
        scene.close()
    # light-sample queries on the three kinds of lights table
    doc = json.load(open(os.path.join(ROOT, "examples", "cornell_box.json")))
    tri = json.loads(json.dumps(doc))                # the lamp's rectangle as two triangles whose front faces the floor
    tri["objects"]["lamp_a"] = {"triangle": [[213, 554, 227], [343, 554, 332], [213, 554, 332]], "material": "light"}
    tri["objects"]["lamp_b"] = {"triangle": [[213, 554, 227], [343, 554, 227], [343, 554, 332]], "material": "light"}
    tri["world"] = {"list": ["left", "right", "lamp_a", "lamp_b", "floor", "ceiling", "back", "block_placed", "ball"]}
    tri["lights"] = ["lamp_a", "lamp_b", "light_ball"]
    rng = np.random.default_rng(19)
    q = np.zeros(256, dtype=pkg.LIGHTQUERY_DTYPE)
    q["p"] = rng.uniform(20.0, 530.0, (256, 3)).astype(np.float32)
    q["rng_state"] = rng.integers(0, 1 << 63, 256, dtype=np.uint64)
    q["d"][128:] = np.float32([278.0, 554.0, 279.5]) + rng.uniform(-60.0, 60.0, (128, 3)).astype(np.float32) * np.float32([1, 0, 1]) - q["p"][128:]
    q["flags"][128:] = A.RT_LIGHTQ_DIRECTION_GIVEN
    for kind, d in (("plain", doc), ("all_shapes", dict(tri, lights_all_shapes=True)), ("lights_many", dict(tri, lights_all_shapes=True, lights_many=True))):
        js = pkg.JsonScene(d)
        scene = ctx.upload(js.desc)
        out, st = ctx._light_queries(scene, q, True)
        record(f"sample_lights cornell {kind}", [out], st)
        scene.close()
    # a radiance query: 256 pixel-centre rays of the Cornell box, 4 samples each, ray 100 without a direction
    hs = scenes["cornell"]
    scene = ctx.upload(hs.desc)
    rays = camera_rays(np, hs.camera(1.0), 16, 16)
    rays[100, 4:7] = 0.0
    rgb, sq, invalid, st = ctx.radiance(scene, rays, 4, seed=7, with_stats=True)
    record("radiance cornell 256x4", [rgb, sq, invalid], st, chunked=True)
    scene.close()
    # the three denoisers on a book-1 frame with its features and moments
    hs = scenes["book1"]
    W, H = 64, 40
    cam = hs.camera(W / H)
    prm = pkg.make_params(W, H, 8, seed=7)
    scene = ctx.upload(hs.desc)
    rgb, sq, st = ctx.render_pass(scene, cam, prm, 0, 8, False, torch.zeros(W * H * 3, dtype=torch.float32, device=dev), torch.zeros(W * H * 3, dtype=torch.float32, device=dev))
    alb, nrm, dep, hits, alb2, nrm2, dep2 = ctx.render_feature_moments(scene, cam, prm)
    for f in (1, 3):
        opt = pkg.denoise_options(patch_radius=f)
        record(f"denoise book1 {W}x{H}x8 f{f}", [ctx.denoise(rgb, sq, W, H, samples=8, options=opt)], st)
        record(f"denoise_guided book1 {W}x{H}x8 f{f}", [ctx.denoise_guided(rgb, sq, W, H, 8, alb, nrm, dep, hits, samples=8, options=opt)], st)
        record(f"denoise_guided_moments book1 {W}x{H}x8 f{f}", [ctx.denoise_guided_moments(rgb, sq, W, H, 8, alb, nrm, dep, hits, alb2, nrm2, dep2, samples=8, options=opt)], st)
    scene.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(lines)} calls -> {args.out}")

    if args.timing:
        scene = ctx.upload(hs.desc)
        d_rays = d_rays[:4096].contiguous()
        hits = torch.empty((4096, 12), dtype=torch.float32, device=dev)
        frame = torch.empty(64 * 40 * 3, dtype=torch.float32, device=dev)
        prm = pkg.make_params(64, 40, 2, seed=7)
        small = {"trace_rays_device 4096 rays": lambda: ctx.trace_rays(scene, d_rays, out=hits, with_stats=True)[1],
                 "render_device 64x40x2": lambda: ctx.render_device(scene, cam, prm, frame.data_ptr())}
        timing = {"library": pkg.lib_path()}
        for what, call in small.items():
            for _ in range(3):
                call()
            ms = sorted(call()["render_ms"] for _ in range(20))
            timing[what] = {"render_ms_median": 0.5 * (ms[9] + ms[10]), "render_ms_min": ms[0], "render_ms_max": ms[-1], "calls": 20, "warm": 3}
        scene.close()
        with open(args.timing, "w") as f:
            json.dump(timing, f, indent=1)
        print(json.dumps(timing))
    ctx.close()


if __name__ == "__main__":
    main()
