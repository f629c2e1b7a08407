#!/usr/bin/env python3
"""bench.py — Msamples/s (pixels x spp / s) of the path-tracing hot path on the book-1 final scene.

    python bench.py --gpus 1 --steps 3 --warmup 1
    python bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR     # + the last timed step's frame as DIR/rgb_sum.npy
    python bench.py --full                                                # + roofline, variants and the CPU baseline
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One step = one full render of the workload (BASELINE.json configs[1]: book-1 random spheres, 1200x800, 500 spp, depth 50)
through the C ABI, output left in HBM. With N GPUs (one process per GPU) the framebuffer is tile-sharded and gathered on rank 0 by
the LIBRARY (rt_render_gather: grouped ncclSend/ncclRecv, RCCL over xGMI, then the root's untile kernel); torch.distributed (gloo)
only carries the 128-byte RCCL id, the barrier and the max over ranks. Per-GPU work is held fixed (weak scaling: the image grows to
N x 960k pixels at the same aspect and view); `variants.strong_4096` is the SAME 4096x4096 image at every N (strong scaling).
Prints ONE JSON line on rank 0. A plain run sets up, warms up, times the steps and prints the headline; what takes renders of its own
(the strong-scaling leg, the roofline's counting render, the host-resident / SAH / other-config variants, the CPU baseline) runs with --full.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
VALU_PEAK_TLANEOPS = 256 * 4 * 32 * 2.4e9 / 1e12   # 78.64: 256 CUs x 4 SIMD-32 x 2.4 GHz lane-instructions per second (= 157.3 TFLOP/s FP32 FMA / 2)
NODE_BYTES, SPHERE_BYTES, RAY_BYTES, HIT_BYTES = 32, 20, 32, 8   # SURVEY.md §8(d) record sizes
LDS_PEAK_GCYC = 256 * 2.4                          # 614.4: 256 CUs x 2.4 GHz LDS-array cycles per second, in 1e9 (one 256-byte-wide access slot per CU and cycle)
PMC_PROFILE = os.path.join("profiles", "r03_pmc_book1.json")
PMC_PROFILE_C5 = os.path.join("profiles", "r03_pmc_c5.json")
DUMP_MAX_BYTES = 64 << 20        # --dump-outputs: a larger frame (many ranks) is written as a fixed, seeded sample of its pixels


def host_cores():
    """CPU threads this process may really use: affinity mask, capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(math.ceil(int(q) / int(per)))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, int(math.ceil(q / per))))
        except Exception:
            pass
    return max(1, min(n, int(os.environ.get("RT_BENCH_CPU_THREADS", "64"))))


def image_size(n_gpus, base_w=1200, base_h=800):
    """Same 3:2 view, N x the pixels (weak scaling)."""
    if n_gpus == 1:
        return base_w, base_h
    s = math.sqrt(n_gpus)
    # whole 32 x 32 tiles: a shard whose tiles all lie inside the image finds a path's next work item by arithmetic
    return int(round(base_w * s / 32)) * 32, int(round(base_h * s / 32)) * 32


def dump_frame(frame, out_dir):
    """The frame the timed path computed in its last step (float32 per-pixel RGB sums, H x W x 3) as out_dir/rgb_sum.npy. Above
    DUMP_MAX_BYTES, a seeded sample of whole pixels instead: rgb_sum.npy (k x 3) and their row-major indices, rgb_sum_pixel_index.npy."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    a = np.ascontiguousarray(frame.detach().cpu().numpy(), dtype=np.float32)
    if a.nbytes > DUMP_MAX_BYTES:
        n = a.shape[0] * a.shape[1]
        idx = np.sort(np.random.default_rng(1).choice(n, DUMP_MAX_BYTES // 2 // (3 * 4), replace=False))
        np.save(os.path.join(out_dir, "rgb_sum_pixel_index.npy"), idx.astype(np.float64))
        a = a.reshape(n, 3)[idx]
    np.save(os.path.join(out_dir, "rgb_sum.npy"), a)


def other_configs(pkg, ctx, A, B, dev, stream):
    """BASELINE configs 3, 4 and the one-GPU stand-in of config 5 at reduced spp: one warm render, one timed. Config 5 is the scene whose
    BVH lives in HBM: its k_extend gets the HBM view (PMC bytes per segment from profiles/r02_pmc_c5.json, valid for the sources it was
    measured on, x segments / kernel time against 8 TB/s)."""
    import numpy as np
    import torch
    res = {}
    cases = [("C3_book2_final_800x800", "final", 800, 800, 100), ("C4_cornell_600x600", "cornell", 600, 600, 250),
             ("C5_standin_1M_spheres_262K_triangles_2048x2048", "big_sah", 2048, 2048, 16),
             # the scene the C5 PARITY crops are taken from (tests/crops.py): 1 M spheres + the 131 072-triangle torus imported from an OBJ file,
             # reference-shaped tree, 4096x4096 — timed beside the stand-in that is profiled
             ("C5_parity_scene_1M_spheres_obj_mesh_4096x4096", "big_obj", 4096, 4096, 4)]
    for tag, name, W, H, spp in cases:
        if name == "final":
            from PIL import Image
            hs = pkg.HostScene("final", 1, image=np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "earthmap_rgb.png")).convert("RGB")))
        elif name == "big_sah":
            hs = pkg.HostScene("big_sah", 5, 1000000, 512)
        elif name == "big_obj":
            import tempfile
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import crops as K
            obj = os.path.join(tempfile.gettempdir(), "bench_torus_512x128.obj")
            if not os.path.exists(obj):
                K.write_torus_obj(obj, 512, 128)
            hs = pkg.HostScene("big_obj:" + obj, 5, 1000000)
        else:
            hs = pkg.HostScene(name, 0)
        t0 = time.perf_counter()
        scene = ctx.upload(hs.desc)
        up = time.perf_counter() - t0
        cam = hs.camera(W / H)
        prm = pkg.make_params(W, H, spp, max_depth=50, seed=1, flags=A.RT_FLAG_TIMING)
        frame = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        stream.synchronize()
        ctx.render_device(scene, cam, prm, frame.data_ptr())
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        st = ctx.render_device(scene, cam, prm, frame.data_ptr())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t1
        r = {"value": round(W * H * spp / dt / 1e6, 1), "unit": "Msamples/s", "spp": spp, "ms": round(dt * 1e3, 2), "k_extend_ms": round(st["extend_ms"] + st["drain_ms"], 2),
             "k_shade_ms": round(st["shade_ms"], 2), "segments": st["segments"], "bvh_in_lds": st["bvh_in_lds"], "scene_upload_s": round(up, 2)}
        if name == "big_sah":
            try:
                tj = json.load(open(os.path.join(ROOT, PMC_PROFILE_C5)))
                if tj.get("source_hash") == B.source_hash() and st["extend_ms"] > 0:
                    # the profile's bytes and this run's segments both cover the wavefront launches AND the launch that carries the tail
                    bps = tj["kernels"]["k_extend"]["bytes_per_segment"]
                    gbs = bps * st["segments"] / ((st["extend_ms"] + st["drain_ms"]) * 1e-3) / 1e9
                    r["k_extend_hbm"] = {"bound": "hbm", "bytes_per_segment": bps, "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
                                         "l2_hit_rate": tj["kernels"]["k_extend"].get("l2_hit_rate"),
                                         "note": f"PMC FETCH_SIZE x 2 + WRITE_SIZE per segment ({PMC_PROFILE_C5}) x this run's segments / (k_extend + tail launch) time; the walk is "
                                                 "bound by the CU's L1 under divergent 16-byte loads, not by HBM bytes (DESIGN.md section 5)"}
                else:
                    r["k_extend_hbm"] = {"note": f"{PMC_PROFILE_C5} was measured on other sources: not used"}
            except Exception as e:
                r["k_extend_hbm"] = {"error": repr(e)}
        res[tag] = r
        del frame
        scene.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)     # (the first render or two after start-up run ~3 % slow: 84 ms against 81.5 once the part has warmed up)
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="with --full: target CPU-baseline duration (0 = skip)")
    ap.add_argument("--pool-slots", type=int, default=0)
    ap.add_argument("--strong-spp", type=int, default=64, help="with --full: spp of the 4096x4096 strong-scaling leg (0 = skip)")
    ap.add_argument("--no-variants", action="store_true", help="with --full: roofline and CPU baseline only")
    ap.add_argument("--full", action="store_true", help="after the headline: strong-scaling leg, roofline, variants, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's frame as DIR/rgb_sum.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    import torch
    import rta
    pkg = rta.load()
    A = pkg._abi
    from importlib import import_module
    D = import_module("ray_tracer_archive_amd.distributed")
    B = import_module("ray_tracer_archive_amd.build")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("BENCH_REHEARSE_ON_ONE_GPU") == "1":
        local_rank = 0     # rehearsal of the N > 1 control flow on a one-GPU box: every rank on device 0 (RCCL refuses that, so the staged gather runs)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo")          # control plane only: RCCL id, barrier, max over ranks
    n_gpus = max(world, 1)
    if args.gpus != n_gpus and rank == 0:
        print(f"note: --gpus {args.gpus} but WORLD_SIZE={world}; using {n_gpus}", file=sys.stderr)

    # one rank per GPU; on a box with FEWER GPUs than ranks (the one-GPU rehearsal of the N > 1 path) ranks share devices: RCCL then refuses
    # the communicator and the staged gather below takes over, which is the point of the rehearsal
    device_index = local_rank % max(1, torch.cuda.device_count())
    if device_index != local_rank and rank == 0:
        print(f"note: {world} ranks on {torch.cuda.device_count()} GPU(s): ranks share devices (rehearsal; not a scaling measurement)", file=sys.stderr)
    torch.cuda.set_device(device_index)
    dev = torch.device("cuda", device_index)
    # a real (non-null) torch stream, made current: the library launches on it, and HIP events recorded by the library see
    # every kernel of a step
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    assert stream.cuda_stream != 0
    ctx = pkg.Context(device_index, stream.cuda_stream)
    gather_path = "single GPU"
    staged_why = None
    if n_gpus > 1:
        ok, why = D.init_comm_guarded(ctx, rank, n_gpus, dist)   # rt_comm_init_rank + rt_comm_selftest: the data-path collective lives in the library
        if ok:
            gather_path = "rt_render_gather: grouped ncclSend/ncclRecv to rank 0 (RCCL, called from csrc/rt_multi.cpp) + untile kernel"
        else:
            staged_why = why
            gather_path = "FALLBACK: shards staged through host memory over gloo, rt_untile_device on rank 0 (the library's RCCL exchange could not be set up: " + why + ")"
    hs = pkg.HostScene("book1", 1)
    scene = ctx.upload(hs.desc)
    if n_gpus > 1 and staged_why is None:
        # the first exchange between the devices of this node: a small frame, compared on rank 0 with its own render of it
        ok, why = D.trial_gather(ctx, scene, hs.camera(160 / 96), rank, n_gpus, dist, dev)
        if ok:
            gather_path += "; verified on a 160x96 frame against rank 0's own render, bit for bit"
        else:
            staged_why = why
            gather_path = "FALLBACK: shards staged through host memory over gloo, rt_untile_device on rank 0 (the library's RCCL exchange failed its trial: " + why + ")"
    W, H = (args.width, args.height) if args.width and args.height else image_size(n_gpus)
    cam = hs.camera(W / H)
    base = pkg.make_params(W, H, args.spp, max_depth=50, seed=1, flags=A.RT_FLAG_TIMING, pool_slots=args.pool_slots)
    frame1 = torch.empty((H, W, 3), dtype=torch.float32, device=dev) if n_gpus == 1 else None
    stream.synchronize()

    stats_acc = []

    def step():
        if n_gpus == 1:
            stats_acc.append(ctx.render_device(scene, cam, base, frame1.data_ptr()))
            return frame1
        if staged_why is None:
            frame, st = D.render_gathered(ctx, scene, cam, base, rank, A.RT_OUT_RGB_SUM_F32, device=dev)
        else:
            frame, st = D.render_gathered_staged(ctx, scene, cam, base, rank, n_gpus, dist, A.RT_OUT_RGB_SUM_F32, device=dev)
        stats_acc.append(st)
        return frame

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def sum_over_ranks(x):
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64)
        dist.all_reduce(t)
        return float(t.item())

    for _ in range(args.warmup):
        step()
    stats_acc.clear()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0)
    if args.dump_outputs and rank == 0:
        dump_frame(last, args.dump_outputs)     # before any --full leg renders into frame1

    # per-rank device statistics of the timed steps
    seg = sum(s["segments"] for s in stats_acc)
    ext_ms = sum(s["extend_ms"] for s in stats_acc)
    shade_ms = sum(s["shade_ms"] for s in stats_acc)
    other_ms = sum(s["other_ms"] for s in stats_acc)
    gather_ms = sum(s["gather_ms"] for s in stats_acc)
    launches = sum(s["extend_launches"] for s in stats_acc)
    samples_total = sum_over_ranks(float(sum(s["samples"] for s in stats_acc)))

    # ---- strong-scaling leg: the SAME 4096x4096 book-1 image at every N, RGB8 out (write_color on the devices, 3 B/pixel gathered) ----
    strong = None
    if args.full and args.strong_spp > 0 and not args.no_variants:
        try:
            SW = SH = 4096
            scam = hs.camera(SW / SH)
            sprm = pkg.make_params(SW, SH, args.strong_spp, max_depth=50, seed=1, flags=A.RT_FLAG_TIMING)
            if n_gpus == 1:
                f = torch.empty((SH, SW, 3), dtype=torch.float32, device=dev)
                f8 = torch.empty((SH, SW, 3), dtype=torch.uint8, device=dev)
                stream.synchronize()

            def sstep():
                if n_gpus == 1:
                    st = ctx.render_device(scene, scam, sprm, f.data_ptr())
                    ctx.resolve_device(f.data_ptr(), SW, SH, args.strong_spp, f8.data_ptr())
                    return st
                if staged_why is not None:
                    return D.render_gathered_staged(ctx, scene, scam, sprm, rank, n_gpus, dist, A.RT_OUT_RGB8, device=dev)[1]
                return D.render_gathered(ctx, scene, scam, sprm, rank, A.RT_OUT_RGB8, device=dev)[1]
            sstep()
            barrier()
            t1 = time.perf_counter()
            sst = [sstep() for _ in range(2)]
            barrier()
            sdt = max_over_ranks(time.perf_counter() - t1)
            strong = {"value": round(SW * SH * args.strong_spp * 2 / sdt / 1e6, 1), "unit": "Msamples/s", "n_gpus": n_gpus, "width": SW, "height": SH,
                      "spp": args.strong_spp, "steps": 2, "ms_per_step": round(sdt / 2 * 1e3, 2), "output": "RGB8 frame on rank 0 (write_color per shard before the gather)",
                      "gather_ms_rank0": round(sum(s["gather_ms"] for s in sst) / 2, 3), "scaling": "strong",
                      "note": "same image at every N: divide by the N=1 run's figure for the speed-up (north star: >= 6x at 8 GPUs)"}
        except Exception as e:
            strong = {"error": repr(e)}

    if rank != 0:
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    value = samples_total / dt / 1e6
    out = {
        "metric": "Msamples/s (pixels x spp / s), book-1 final scene", "value": round(value, 3), "unit": "Msamples/s",
        "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"book-1 final random-spheres scene (scene_seed 1, 485 spheres: the reference's BVH algorithm over 484 of them, the r = 1000 ground sphere tested before the walk), {W}x{H}, {args.spp} spp, "
                               f"depth 50, seed 1; output rgb_sum left in HBM" + (f"; {n_gpus} ranks, 32x32 tiles round-robin" if n_gpus > 1 else ""),
                   "width": W, "height": H, "spp": args.spp, "max_depth": 50, "pool_slots": stats_acc[0]["pool_slots"] if stats_acc else 0,
                   "bvh_in_lds": stats_acc[0]["bvh_in_lds"] if stats_acc else 0, "gather": gather_path,
                   **({"ranks_share_devices": True} if device_index != int(os.environ.get("LOCAL_RANK", "0")) else {}),
                   "timing": "mean over the timed steps, frame left in HBM (SURVEY 8(d) asks for the host-resident median: +1 copy of 11.5 MB, < 1 ms; DESIGN.md section 5)"},
        "kernel_ms_per_step": {"k_extend": round(ext_ms / args.steps, 3), "k_shade": round(shade_ms / args.steps, 3), "generate+resolve": round(other_ms / args.steps, 3),
                               "gather+untile": round(gather_ms / args.steps, 3), "launches_per_step": launches // max(1, args.steps)},
    }

    def emit():
        print(json.dumps(out))
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()

    if not args.full:
        emit()
        return

    try:
        # ---- roofline of the dominant kernel (k_extend = BVH traversal), rank 0's launches ----
        # The scene (24 KB) is LDS-resident, so the traversal's node/sphere records never reach HBM: the kernel's roof is VALU
        # issue, not HBM. achieved = VALU lane-instructions per launch / average launch duration (HIP events on the launch stream,
        # live); lane-instructions per SEGMENT are a constant of the kernel build, taken from the committed PMC pass of this very
        # workload (SQ_THREAD_CYCLES_VALU / segments) and valid only for the sources it was measured on (source_hash).
        cprm = pkg.make_params(W, H, max(1, args.spp // 10), max_depth=50, seed=1, flags=A.RT_FLAG_COUNTERS,
                               tile_size=32 if n_gpus > 1 else 0, shard_index=0, shard_count=n_gpus)
        tmp = torch.zeros(pkg.output_floats(cprm), dtype=torch.float32, device=dev)
        stream.synchronize()
        cst = ctx.render_device(scene, cam, cprm, tmp.data_ptr())
        vn = cst["node_tests"] / max(1, cst["segments"])
        vp = cst["prim_tests"][0] / max(1, cst["segments"])
        seg_per_sample = cst["segments"] / max(1, cst["samples"])
        b_seg_trav = vn * NODE_BYTES + vp * SPHERE_BYTES
        b_seg = b_seg_trav + RAY_BYTES + HIT_BYTES
        ext_s = ext_ms * 1e-3
        pmc, pmc_note = None, None
        try:
            tj = json.load(open(os.path.join(ROOT, PMC_PROFILE)))
            if tj.get("source_hash") != B.source_hash():
                pmc_note = f"{PMC_PROFILE} was measured on other kernel sources ({tj.get('source_hash')} != {B.source_hash()}): not used"
            else:
                pmc = tj["kernels"]["k_extend"]
        except Exception as e:
            pmc_note = f"{PMC_PROFILE}: {e!r}"
        roof = {"bound": "lds", "kernel": "k_extend",
                "avg_launch_ms": round(ext_ms / max(1, launches), 4), "launches": launches, "segments_per_launch": round(seg / max(1, launches), 1),
                "node_tests_per_segment": round(vn, 2), "sphere_tests_per_segment": round(vp, 2), "segments_per_sample": round(seg_per_sample, 3)}
        if pmc is not None and ext_s > 0:
            # The scene is LDS-resident and every node visit is two 16-byte LDS gathers per lane: of the CU's units the LDS array is the
            # busiest (PMC), so it is the roof this kernel is priced against; VALU lanes are printed beside it. Both are cycles (or
            # lane-instructions) per SEGMENT from the committed PMC pass of this workload x this run's segments / the live launch time.
            lops = pmc["valu_lane_instructions_per_segment"]
            valu = seg * lops / ext_s / 1e12
            lds_cyc = pmc["counters"]["SQ_LDS_IDX_ACTIVE"] / tj["segments"]
            lds = seg * lds_cyc / ext_s / 1e9
            roof.update({"peak": round(LDS_PEAK_GCYC, 1), "unit": "G LDS-array cycles/s",
                         "peak_note": "256 CUs x 2.4 GHz: one LDS-array cycle (a 256-byte-wide access slot) per CU and clock; SQ_LDS_IDX_ACTIVE counts the "
                                      "cycles the array works, bank conflicts included (MI355X_MICROARCH.md, LDS)",
                         "achieved": round(lds, 1), "frac": round(lds / LDS_PEAK_GCYC, 4), "lds_array_cycles_per_segment": round(lds_cyc, 1),
                         "valu": {"bound": "valu", "achieved": round(valu, 2), "peak": round(VALU_PEAK_TLANEOPS, 2), "unit": "Tlaneop/s", "frac": round(valu / VALU_PEAK_TLANEOPS, 4),
                                  "peak_note": "256 CUs x 4 SIMD-32 x 32 lanes x 2.4 GHz VALU lane-instructions/s (FP32 FMA peak 157.3 TFLOP/s = 2 flop per lane-instruction)"},
                         "lane_instructions_per_segment": lops, "lane_instructions_per_launch": round(lops * seg / max(1, launches)),
                         "traffic": round(pmc["bytes_per_segment"] * seg / max(1, launches) / 1e6, 3), "traffic_unit": "MB/launch",
                         "traffic_source": f"{pmc['bytes_per_segment']} B/segment HBM (PMC FETCH_SIZE x 2 + WRITE_SIZE, separate passes) x segments_per_launch",
                         "source": f"{PMC_PROFILE} (source_hash {tj['source_hash']}, git {tj.get('git_commit')})",
                         "pmc": {k: pmc.get(k) for k in ("valu_lane_frac", "valu_issue_frac", "valu_lane_utilisation", "lds_busy", "lds_conflict_share",
                                                         "salu_per_valu", "wait_inst_any_share", "wait_any_share")}})
        else:
            roof.update({"achieved": None, "frac": None, "traffic": None, "note": pmc_note})
        # secondary: the north star's HBM view. Algorithmic bytes (node + sphere records the reference-order traversal touches, + ray
        # read + hit write) against the HBM peak — NOT a fraction of anything the kernel is bound by: these bytes come from LDS.
        alg_gbs = seg * b_seg / ext_s / 1e9 if ext_s > 0 else 0.0
        roof["hbm_view"] = {"algorithmic_bytes_per_segment": round(b_seg, 1), "algorithmic_gbs": round(alg_gbs, 1),
                            "algorithmic_over_hbm_peak": round(alg_gbs / HBM_PEAK_GBS, 3),
                            "measured_hbm_bytes_per_segment": pmc["bytes_per_segment"] if pmc else None,
                            "measured_hbm_gbs": round(seg * pmc["bytes_per_segment"] / ext_s / 1e9, 1) if pmc and ext_s > 0 else None,
                            "measured_over_hbm_peak": round(seg * pmc["bytes_per_segment"] / ext_s / 1e9 / HBM_PEAK_GBS, 4) if pmc and ext_s > 0 else None,
                            "note": f"the 24 KB scene is LDS-resident: HBM sees the ray records only; the HBM roofline applies to config 5 ({PMC_PROFILE_C5})"}
        # the second kernel of a step, k_shade, is the HBM-side one: PMC bytes per segment x this run's segments / its kernel time
        if pmc is not None and shade_ms > 0 and "k_shade" in tj["kernels"]:
            sb = tj["kernels"]["k_shade"]["bytes_per_segment"]
            sg = seg * sb / (shade_ms * 1e-3) / 1e9
            roof["k_shade"] = {"bound": "hbm", "bytes_per_segment": sb, "achieved": round(sg, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(sg / HBM_PEAK_GBS, 4),
                               "share_of_step": round(shade_ms / max(1e-9, ext_ms + shade_ms + other_ms), 3)}
        out["roofline"] = roof
    except Exception as e:   # the contract line must survive a failure in the extras
        out["roofline"] = {"bound": "lds", "error": repr(e)}

    variants = {}
    if strong is not None:
        variants["strong_4096"] = strong
    # ---- the metric as SURVEY 8(d) words it: rt_render (framebuffer resident on the HOST when the call returns), 3 warm + 5 timed, median ----
    if n_gpus == 1 and not args.no_variants:
        try:
            import numpy as np
            hprm = pkg.make_params(W, H, args.spp, max_depth=50, seed=1)
            for _ in range(3):
                ctx.render(scene, cam, hprm)
            ts = []
            for _ in range(5):
                t1 = time.perf_counter(); ctx.render(scene, cam, hprm); ts.append(time.perf_counter() - t1)
            med = float(np.median(ts))
            variants["host_resident_median"] = {"value": round(W * H * args.spp / med / 1e6, 1), "unit": "Msamples/s", "ms": round(med * 1e3, 2), "runs_ms": [round(t * 1e3, 2) for t in ts],
                                                "note": "rt_render: first launch to framebuffer in host memory (one 11.5 MB D2H copy + the numpy buffer the binding allocates), "
                                                        "3 warm + 5 timed, median (SURVEY 8(d)); `value` above is the bench contract's mean with the frame left in HBM"}
        except Exception as e:
            variants["host_resident_median"] = {"error": repr(e)}
    # ---- same workload on the RT_BVH_SAH tree (library option, not the reference's builder): reported beside, never as `value` ----
    if n_gpus == 1 and not args.no_variants:
        try:
            hs2 = pkg.HostScene("book1_sah", 1)
            scene2 = ctx.upload(hs2.desc)
            ctx.render_device(scene2, cam, base, frame1.data_ptr())
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            s2 = ctx.render_device(scene2, cam, base, frame1.data_ptr())
            torch.cuda.synchronize()
            d2 = time.perf_counter() - t1
            variants["bvh_sah"] = {"value": round(s2["samples"] / d2 / 1e6, 1), "unit": "Msamples/s", "extend_ms": round(s2["extend_ms"], 1),
                                   "note": "identical frame (tests/test_gpu_scenes.py::test_sah_builder_gives_the_same_picture), about half the box tests per segment"}
        except Exception as e:   # never let the extra line break the contract line
            variants["bvh_sah"] = {"error": str(e)}
        # ---- the other BASELINE configs at reduced spp (parity-test cases, not bench lines: reported beside for the record) ----
        try:
            variants["other_configs"] = other_configs(pkg, ctx, A, B, dev, stream)
        except Exception as e:
            variants["other_configs"] = {"error": repr(e)}
    if variants:
        out["variants"] = variants

    try:
        # ---- CPU baseline: the oracle (a port of the reference's CPU path), all host cores, bounded samples ----
        if n_gpus == 1 and args.cpu_seconds > 0:
            from oracle import binding as orc
            cores = host_cores()
            bw, bh = 1200, 800
            bcam = hs.camera(bw / bh)
            probe = pkg.make_params(bw, bh, 2, max_depth=50, seed=1)
            _, pst = orc.render(hs.desc, bcam, probe, precision=64, n_threads=cores)
            rate = pst["samples"] / max(pst["seconds"], 1e-6)
            spp_b = int(max(2, min(args.spp, args.cpu_seconds * rate / (bw * bh))))
            bprm = pkg.make_params(bw, bh, spp_b, max_depth=50, seed=1)
            _, bst = orc.render(hs.desc, bcam, bprm, precision=64, n_threads=cores)
            cb = {"value": round(bst["samples"] / bst["seconds"] / 1e6, 3), "unit": "Msamples/s", "cores": cores, "kind": "port",
                  "sample": f"same scene/camera/seed at {bw}x{bh}, {spp_b} spp ({bst['samples']} samples, {bst['seconds']:.1f} s), "
                            f"f64 oracle (oracle/oracle.cpp), std::thread over rows"}
            # BASELINE configs[0] in full (400x225, 100 spp: the reference's own CPU-runnable case), same port
            c1cam = hs.camera(400 / 225)
            c1 = pkg.make_params(400, 225, 100, max_depth=50, seed=1)
            _, c1st = orc.render(hs.desc, c1cam, c1, precision=64, n_threads=cores)
            cb["c1_full"] = {"value": round(c1st["samples"] / c1st["seconds"] / 1e6, 3), "unit": "Msamples/s", "seconds": round(c1st["seconds"], 2),
                             "sample": "BASELINE configs[0] whole: 400x225, 100 spp, depth 50 (9.0 Msamples)"}
            # the reference's own driver shape (main.rs:730-778): one pixel at a time, thread_num threads spawned per pixel
            rows = 8
            y0 = 225 // 2
            _, rst = orc.render_reference_shaped(hs.desc, c1cam, c1, 20, (0, y0, 400, y0 + rows))
            cb["reference_shaped"] = {"value": round(rst["samples"] / rst["seconds"] / 1e6, 4), "unit": "Msamples/s", "threads_per_pixel": 20,
                                      "sample": f"configs[0], rows {y0}..{y0 + rows - 1} ({rst['samples']} samples, {rst['seconds']:.1f} s): one pixel at a time, 20 threads "
                                                f"spawned per pixel x 5 samples each (main.rs:730-778 uses 18, which does not divide 100)"}
            out["cpu_baseline"] = cb
    except Exception as e:
        out["cpu_baseline"] = {"error": repr(e)}
    emit()


if __name__ == "__main__":
    main()
