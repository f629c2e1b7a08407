"""Ray queries on the GPU (include/rt_hip.h, "ray queries"): the production traversal kernels ray by ray against the f64 CPU checker in
every device layout, the bit-for-bit invariances the header promises, the edges, and the export kernel against k_shade's own rebuild of
the HitRecord."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays as R  # noqa: E402

pytestmark = pytest.mark.gpu


def layouts(A):
    return {"default": 0, "reference_counters": A.RT_LAYOUT_REFERENCE_COUNTERS, "hbm": A.RT_LAYOUT_SCENE_IN_HBM,
            "hbm_32b": A.RT_LAYOUT_SCENE_IN_HBM | A.RT_LAYOUT_NODES_32B, "hbm_wide": A.RT_LAYOUT_SCENE_IN_HBM | A.RT_LAYOUT_WIDE_NODES}


CASES = [(s, l) for s in R.SCENES for l in ("default", "reference_counters", "hbm", "hbm_32b", "hbm_wide") if l != "hbm_wide" or s in R.STATIC_SCENES]

# Worst deviation from the f64 checker on agreeing hits, per scene (every layout gave the same figures): relative |dt|, |dp| / scene extent,
# |dn|, |d(u, v)| (u modulo 1, hits within 1e-3 of a sphere's pole left out), as measured on an MI355X (DESIGN.md section 11 has the
# table). The test allows 2 x the figure: box-to-box differences of libm / ocml rounding are of that order, the margin the project's
# parity tests use. The large relative |dt| belong to secondary rays that end a few 1e-3 from where they start: an absolute error of
# 1e-5 in t (RT_SPHERE_TOL, or the f32 rounding of an origin 500 units out) over a t of that size.
MEASURED = {
    "book1": dict(t=9.351e-3, p=3.843e-7, n=1.905e-3, uv=3.837e-4, ta=3.622e-5),
    "cornell": dict(t=2.142e-2, p=1.773e-6, n=1.093e-5, uv=2.656e-6, ta=3.360e-5),
    "mesh": dict(t=8.428e-6, p=2.876e-7, n=1.986e-7, uv=4.262e-6, ta=1.203e-6),
    "moving": dict(t=3.378e-3, p=1.279e-6, n=5.115e-4, uv=6.089e-6, ta=1.260e-5),
    "rotated_sphere": dict(t=2.004e-5, p=2.445e-7, n=2.648e-6, uv=8.235e-7, ta=9.502e-7),
    "earth": dict(t=1.246e-4, p=3.765e-7, n=5.109e-6, uv=4.772e-6, ta=6.607e-6),
}
# `ta`: the worst |dt| / max(1, t), measured the same way. The relative figure is set by the few rays with t ~ 1e-3 and would let a t of
# ordinary size be wrong by a per cent; this one holds every hit's t to the absolute error the device really has.


def trace_device(pkg, gpu, scene, rays, options=None, with_stats=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()
    out = gpu.trace_rays(scene, t, options=options, with_stats=with_stats)
    hits = (out[0] if with_stats else out).cpu().numpy().reshape(-1).view(pkg.RAYHIT_DTYPE)
    return (hits, out[1]) if with_stats else hits


@pytest.mark.parametrize("name,layout", CASES)
def test_rays_agree_with_the_checker(pkg, orc, gpu, name, layout):
    from conftest import record_metric
    A = pkg._abi
    s = R.ray_set(pkg, orc, name)
    built, rays, ref, und = s["built"], s["rays"], s["ref"], s["undecidable"]
    scene = gpu.upload(built.desc, layouts(A)[layout])
    hits, st = trace_device(pkg, gpu, scene, rays, with_stats=True)
    scene.close()
    assert st["segments"] == st["samples"] == len(rays)
    assert layout != "hbm_32b" or st["lds_top_nodes"] == 0      # fewer records than a top holds: M_HBM. The top layout is tests/test_gpu_rays_hbm.py's
    g_hit, g_ff = (hits["flags"] & A.RT_RAYHIT_HIT) != 0, (hits["flags"] & A.RT_RAYHIT_FRONT_FACE) != 0
    assert ((hits["flags"] & ~np.uint32(3)) == 0).all()
    dec = ~und
    print(f"{name}/{layout}: {len(rays)} rays, {int(und.sum())} undecidable (left out), {int((g_hit & dec).sum())} hits compared")
    # ---- condition: on decidable rays hit / miss and front_face agree, for every ray ----
    wrong = dec & (g_hit != ref["hit"])
    assert not wrong.any(), f"hit/miss differs on decidable rays {np.flatnonzero(wrong)[:8]}"
    both = dec & g_hit
    wrong = both & (g_ff != ref["ff"])
    assert not wrong.any(), f"front_face differs on decidable rays {np.flatnonzero(wrong)[:8]}"
    # a miss has the stated form
    miss = ~g_hit
    assert np.isposinf(hits["t"][miss]).all() and (hits["hittable"][miss] == -1).all() and (hits["material"][miss] == -1).all()
    assert (hits["flags"][miss] == 0).all() and not hits["p"][miss].any() and not hits["n"][miss].any() and not hits["u"][miss].any() and not hits["v"][miss].any()
    # ---- the object: `hittable` is a primitive record the checker's hit point lies on, `material` is that record's ----
    ids, on = s["ids"], s["on"]
    col = {int(h): k for k, h in enumerate(ids)}
    for i in np.flatnonzero(both):
        h = int(hits["hittable"][i])
        assert h in col, f"ray {i}: hittable {h} is not a primitive record"
        assert on[i, col[h]], f"ray {i}: the hit point does not lie on hittable {h}"
        assert int(hits["material"][i]) == built.desc.hittables[h].material, f"ray {i}: material"
    # ---- measurement ----
    k = np.flatnonzero(both)
    dt = float(np.max(np.abs(hits["t"][k].astype(np.float64) - ref["t"][k]) / ref["t"][k]))
    dp = float(np.max(np.linalg.norm(hits["p"][k].astype(np.float64) - ref["p"][k], axis=1)) / built.extent)
    dn = float(np.max(np.linalg.norm(hits["n"][k].astype(np.float64) - ref["n"][k], axis=1)))
    kind = np.array([built.desc.hittables[int(h)].kind for h in ids])
    polar = (on[k] & (kind == A.RT_HIT_SPHERE)[None, :]).any(axis=1) & ((ref["v"][k] < 1e-3) | (ref["v"][k] > 1.0 - 1e-3))
    ku = k[~polar]
    du = np.abs(hits["u"][ku].astype(np.float64) - ref["u"][ku]); du = np.minimum(du, 1.0 - du)
    dv = np.abs(hits["v"][ku].astype(np.float64) - ref["v"][ku])
    duv = float(max(du.max(), dv.max()))
    dta = float(np.max(np.abs(hits["t"][k].astype(np.float64) - ref["t"][k]) / np.maximum(1.0, ref["t"][k])))
    print(f"{name}/{layout}: worst |dt|/max(1,t) {dta:.3e}")
    print(f"{name}/{layout}: worst rel|dt| {dt:.3e}  |dp|/extent {dp:.3e}  |dn| {dn:.3e}  |d(u,v)| {duv:.3e}  ({int(polar.sum())} polar hits left out of u, v)")
    record_metric(config="rays", scene=name, layout=layout, dta=dta, dt=dt, dp=dp, dn=dn, duv=duv, undecidable=int(und.sum()), rays=len(rays))
    m = MEASURED[name]
    assert dt <= 2 * m["t"] and dp <= 2 * m["p"] and dn <= 2 * m["n"] and duv <= 2 * m["uv"] and dta <= 2 * m["ta"], (dt, dp, dn, duv, dta, m)


def test_invariances_bit_for_bit(pkg, orc, gpu):
    A = pkg._abi
    s = R.ray_set(pkg, orc, "book1")
    rays = np.concatenate([s["rays"]] * 4)                       # ~10 k rays: longer than a small pool
    scene = gpu.upload(s["built"].desc)
    base = trace_device(pkg, gpu, scene, rays)
    # two calls give equal bytes
    assert base.tobytes() == trace_device(pkg, gpu, scene, rays).tobytes()
    # chunks: a pool of 4096 slots runs the list in three chunks
    small, st = trace_device(pkg, gpu, scene, rays, options=pkg.ray_query_options(pool_slots=4096), with_stats=True)
    assert st["pool_slots"] == 4096 and st["extend_launches"] == -(-len(rays) // 4096)
    assert small.tobytes() == base.tobytes()
    # a permuted list gives the permuted hits
    perm = np.random.default_rng(3).permutation(len(rays))
    assert trace_device(pkg, gpu, scene, rays[perm]).tobytes() == base[perm].tobytes()
    # the host variant equals the device variant
    host = gpu.trace_rays(scene, rays)
    assert host.dtype == pkg.RAYHIT_DTYPE and host.tobytes() == base.tobytes()
    assert gpu.trace_rays(scene, np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)).tobytes() == base.tobytes()
    scene.close()
    # the default layout and LISTS_AS_REFERENCE give equal t bits on book-1 (no equal-t ties in that scene)
    scene = gpu.upload(s["built"].desc, A.RT_LAYOUT_LISTS_AS_REFERENCE)
    other = trace_device(pkg, gpu, scene, rays)
    scene.close()
    assert other["t"].tobytes() == base["t"].tobytes()
    assert (other["hittable"] == base["hittable"]).all()


def test_pool_rule(pkg, orc, gpu):
    """The pool of a query as the library sizes it (RtStats.pool_slots, extend_launches): a multiple of 512 x 8 slots that holds every
    chunk, whatever pool_slots asks for — the rule k_rays_import's bound on a queue's size rests on — and the same hits for every pool."""
    s = R.ray_set(pkg, orc, "mesh")
    scene = gpu.upload(s["built"].desc)
    rays = np.concatenate([s["rays"]] * 5)                       # 12 090 rays
    base = None
    for n in (1, 511, 513, 4096, 4097, len(rays)):
        for pool_slots in (0, 1, 511, 4096, 5000, 8192, 1 << 20):
            hits, st = trace_device(pkg, gpu, scene, rays[:n], options=pkg.ray_query_options(pool_slots=pool_slots), with_stats=True)
            want = -(-min(pool_slots or (1 << 28), n) // 4096) * 4096
            assert st["pool_slots"] == want and st["pool_slots"] % 4096 == 0, (n, pool_slots, st["pool_slots"], want)
            assert st["extend_launches"] == -(-n // want) and st["segments"] == n, (n, pool_slots, st)
            if n == len(rays):
                base = hits if base is None else base
                assert hits.tobytes() == base.tobytes(), (n, pool_slots)
    scene.close()


def test_edges(pkg, orc, gpu):
    import torch
    A = pkg._abi
    s = R.ray_set(pkg, orc, "book1")
    rays = s["rays"]
    scene = gpu.upload(s["built"].desc)
    base = trace_device(pkg, gpu, scene, rays)
    hit = (base["flags"] & A.RT_RAYHIT_HIT) != 0
    assert hit.any() and (~hit).any()
    # t_max below the closest hit turns it into a miss; above it (or "no limit": <= 0, inf, NaN) changes nothing
    lim = rays.copy()
    lim["t_max"] = np.where(hit, base["t"] * np.float32(0.5), np.float32(1.0))
    cut = trace_device(pkg, gpu, scene, lim)
    assert (cut["flags"] == 0).all() and np.isposinf(cut["t"]).all() and (cut["hittable"] == -1).all() and not cut["p"].any()
    for value in (np.where(hit, base["t"] * np.float32(1.5), np.float32(1.0)), -1.0, np.inf, np.nan):
        lim["t_max"] = value
        assert trace_device(pkg, gpu, scene, lim).tobytes() == base.tobytes()
    # invalid rays, mixed into the list, come back flagged; their neighbours' hits are unchanged; the call does not take longer
    bad = rays.copy()
    k = np.arange(5, len(rays), 7)
    third = len(k) // 3
    bad["d"][k[:third]] = 0.0
    bad["o"][k[third:2 * third], 1] = np.nan
    bad["d"][k[2 * third:], 2] = np.inf
    bad["time"][k[::5]] = -np.inf
    trace_device(pkg, gpu, scene, rays)                           # (warm)
    _, st_good = trace_device(pkg, gpu, scene, rays, with_stats=True)
    got, st_bad = trace_device(pkg, gpu, scene, bad, with_stats=True)
    ms_good = float(np.median([trace_device(pkg, gpu, scene, rays, with_stats=True)[1]["render_ms"] for _ in range(7)]))
    ms_bad = float(np.median([trace_device(pkg, gpu, scene, bad, with_stats=True)[1]["render_ms"] for _ in range(7)]))
    ok = np.ones(len(rays), bool); ok[k] = False
    assert got[ok].tobytes() == base[ok].tobytes()
    assert (got["flags"][k] == A.RT_RAYHIT_INVALID_RAY).all() and np.isposinf(got["t"][k]).all()
    assert (got["hittable"][k] == -1).all() and (got["material"][k] == -1).all() and not got["p"][k].any() and not got["n"][k].any()
    assert st_bad["segments"] == st_bad["samples"] == len(rays) - len(k) and st_good["segments"] == len(rays)
    print(f"invalid rays: {len(k)} of {len(rays)}; median of 7 calls {ms_bad:.3f} ms with them, {ms_good:.3f} ms without")
    # the same list with invalid rays in it takes no longer (a call of this size is ~0.06 ms: 0.1 ms of slack for the host's jitter); the
    # single calls above only have to come back at all
    assert ms_bad <= 1.5 * ms_good + 0.1
    assert st_bad["render_ms"] <= 2.0 * st_good["render_ms"] + 20.0
    # a list of invalid rays only
    only = trace_device(pkg, gpu, scene, bad[k])
    assert (only["flags"] == A.RT_RAYHIT_INVALID_RAY).all()
    # n_rays = 0
    assert len(gpu.trace_rays(scene, rays[:0])) == 0
    assert gpu.trace_rays(scene, torch.empty((0, 8), dtype=torch.float32, device="cuda")).numel() == 0
    # timing on request
    _, st = trace_device(pkg, gpu, scene, rays, options=pkg.ray_query_options(flags=A.RT_FLAG_TIMING), with_stats=True)
    assert st["extend_ms"] > 0.0 and st["render_ms"] > 0.0
    # refused options: RT_ERR_INVALID, nothing written
    dev_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    poison = torch.full((len(rays), 12), 123.25, dtype=torch.float32, device="cuda")
    for opt in (A.RtRayQueryOptions(16, 1 << 7, 0, 0), A.RtRayQueryOptions(0, 0, 0, 0)):
        with pytest.raises(pkg.RtError) as e:
            gpu.trace_rays(scene, dev_rays, options=opt, out=poison)
        assert e.value.code == A.RT_ERR_INVALID
        assert bool((poison == 123.25).all())
    scene.close()
    # a scene with a medium: RT_ERR_UNSUPPORTED, the poisoned output untouched (device and host variant)
    fog = R.medium_scene(pkg)
    scene = gpu.upload(fog.desc)
    with pytest.raises(pkg.RtError) as e:
        gpu.trace_rays(scene, dev_rays, out=poison)
    assert e.value.code == A.RT_ERR_UNSUPPORTED and "medium" in str(e.value).lower()
    assert bool((poison == 123.25).all())
    host_out = np.zeros(len(rays), dtype=pkg.RAYHIT_DTYPE); host_out["t"] = 123.25
    with pytest.raises(pkg.RtError):
        gpu.trace_rays(scene, rays, out=host_out)
    assert (host_out["t"] == 123.25).all() and not host_out["flags"].any()
    scene.close()


def test_export_agrees_with_shade(pkg, orc, gpu):
    """k_rays_export restates shade_segment's rebuild of the HitRecord; this keeps the two in step. A Cornell box whose surfaces are all
    DiffuseLights of distinct colours, 1 spp, lens radius 0: a pixel is the emitted colour of the first hit's material, or 0 for a back
    face or a miss. The same camera rays — jitter from the RNG contract (draws 0 and 1 of the pixel's stream) — go
    through the query; emit[material] * front_face must be the frame, pixel for pixel. W - 1 and H - 1 are powers of two, so that the
    renderer's (x + ju) / (W - 1) by hardware reciprocal is the exact quotient and the rays below are the renderer's own, bit for bit."""
    A = pkg._abi
    W, H, SEED = 65, 33, 11
    b = pkg.SceneBuilder(background=(0.0, 0.0, 0.0))
    colours = [(0.25, 0.5, 0.75), (0.75, 0.25, 0.125), (1.0, 1.0, 0.5), (0.5, 0.5, 0.5), (0.125, 0.625, 0.25), (0.375, 0.125, 0.875), (0.875, 0.75, 0.25),
               (0.25, 0.875, 0.875)]
    m = [b.diffuse_light(c) for c in colours]
    box1 = b.translate(b.rotate_y(b.box((0, 0, 0), (165, 330, 165), m[6]), 15.0), (265, 0, 295))
    box2 = b.translate(b.rotate_y(b.box((0, 0, 0), (165, 165, 165), m[7]), -18.0), (130, 0, 65))
    world = b.hittable_list([b.yz_rect(0, 555, 0, 555, 555, m[0]), b.yz_rect(0, 555, 0, 555, 0, m[1]), b.flip_face(b.xz_rect(213, 343, 227, 332, 554, m[2])),
                             b.xz_rect(0, 555, 0, 555, 0, m[3]), b.xz_rect(0, 555, 0, 555, 555, m[4]), b.xy_rect(0, 555, 0, 555, 555, m[5]), box1, box2])
    desc = b.desc(world)
    cam = pkg.camera_new((278, 278, -800), (278, 278, 0), (0, 1, 0), 40.0, W / H, 0.0, 10.0, 0.0, 0.0)
    scene = gpu.upload(desc)
    frame, _ = gpu.render(scene, cam, pkg.make_params(W, H, 1, max_depth=50, seed=SEED))
    f32 = np.float32
    v3 = lambda v: np.array([v.x, v.y, v.z]).astype(f32)
    org, llc, hor, ver = v3(cam.origin), v3(cam.lower_left_corner), v3(cam.horizontal), v3(cam.vertical)
    o = np.zeros((H * W, 3), f32); d = np.zeros((H * W, 3), f32)
    for y in range(H):
        for x in range(W):
            _, _, draws = orc.rng_stream(SEED, y * W + x, 0, 2)
            u = f32(f32(f32(x) + draws[0]) * f32(1.0 / (W - 1)))
            v = f32(f32(f32(H - 1 - y) + draws[1]) * f32(1.0 / (H - 1)))
            o[y * W + x] = org
            d[y * W + x] = ((llc + hor * u) + ver * v) - org          # camera.rs:66-69 in f32, in the order written (lens offset 0)
    hits = gpu.trace_rays(scene, R.make_rays(o, d, np.zeros(H * W, f32)))
    scene.close()
    emit = np.array(colours, f32)
    lit = (hits["flags"] & (A.RT_RAYHIT_HIT | A.RT_RAYHIT_FRONT_FACE)) == (A.RT_RAYHIT_HIT | A.RT_RAYHIT_FRONT_FACE)
    want = np.where(lit[:, None], emit[np.maximum(hits["material"], 0)], f32(0.0)).reshape(H, W, 3)
    n_lit = int(lit.sum())
    # (the camera sees the back of the ceiling, the far wall and one side wall: black; the floor, a side wall, the light and the boxes are lit)
    assert n_lit > H * W // 8 and len(set(hits["material"][lit].tolist())) >= 4, "the frame should show several lit surfaces"
    wrong = np.flatnonzero((frame != want).any(axis=2).reshape(-1))
    assert len(wrong) == 0, f"{len(wrong)} pixels differ, first at {[(int(i) % W, int(i) // W) for i in wrong[:5]]}"


def test_throughput_script_runs(tmp_path):
    """scripts/gpu_rays.py (the figure quoted in DESIGN.md section 11) runs in a process of its own and reports what it says it reports."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "rays.json"
    subprocess.run([sys.executable, os.path.join(root, "scripts", "gpu_rays.py"), "--reps", "3", "--out", str(out)], check=True, timeout=300, cwd=root)
    row = json.loads(out.read_text())
    assert row["rays"] == 1200 * 800 and 0 < row["hits"] <= row["rays"] and row["pool_slots"] >= row["rays"]
    assert row["query_ms"] > 0 and row["query_extend_ms"] > 0 and row["render_1spp_first_iteration_extend_ms"] > 0
    assert abs(row["mrays_per_s"] - row["rays"] / row["query_ms"] / 1e3) <= 0.1 * row["mrays_per_s"]


# ---- axis rays and segments (tests/rays.py axis_set, segment_set) -----------------------------------------------------------------------
# The rays the sets above never hold: directions with +-0, subnormal or 1e-30 components, origins in the planes of box faces, rect edges
# and mesh edges; and point-to-point segments d = q - p with their own t_max near 1. Bounds: 2 x the f32 checker's figure of each set
# (rays.MEASURED_F32_CHECKER); the device's own worst figures are recorded and tabled in DESIGN.md section 11.
FIVE = ("default", "reference_counters", "hbm", "hbm_32b", "hbm_wide")
AXIS_CASES = [(s, l) for s in R.AXIS_SCENES if s not in R.HBM_SCENES for l in FIVE if l != "hbm_wide" or s in R.STATIC_SCENES]    # (field, yard: tests/test_gpu_rays_hbm.py)

# (yard stays in with hbm_wide: it is no static BVH, so that upload keeps the binary walk, and here its answer is looked at)
SEGMENT_CASES = [(s, l) for s in R.SEGMENT_SCENES for l in FIVE if l != "hbm_wide" or s != "moving"]


def hold(pkg, orc, gpu, family, name, layout):
    from conftest import record_metric
    s = R.new_set(pkg, orc, family, name)
    scene = gpu.upload(s["built"].desc, layouts(pkg._abi)[layout])
    try:
        hits, st = trace_device(pkg, gpu, scene, s["rays"], with_stats=True)
    finally:
        scene.close()
    assert st["segments"] == st["samples"] == len(s["rays"])
    worst, _ = R.hold_to_checker(pkg, s, hits, f"{family}/{name}", f"{family}/{name}/{layout}")
    record_metric(config="rays_" + family, scene=name, layout=layout, dta=worst["ta"], dt=worst["t"], dp=worst["p"], dn=worst["n"], duv=worst["uv"],
                  dtabs=worst["tabs"], undecidable=int(s["undecidable"].sum()), rays=len(s["rays"]))
    return s, hits


@pytest.mark.parametrize("name,layout", AXIS_CASES)
def test_axis_rays_agree_with_the_checker(pkg, orc, gpu, name, layout):
    s, hits = hold(pkg, orc, gpu, "axis", name, layout)
    hit = (hits["flags"] & pkg._abi.RT_RAYHIT_HIT) != 0
    assert hit[s["rim"]].all() and hit[s["edge"]].all()


@pytest.mark.parametrize("name,layout", SEGMENT_CASES)
def test_segments_agree_with_the_checker(pkg, orc, gpu, name, layout):
    """Each segment carries its own t_max (0.98 or 1.5): the closest hit under a caller's limit, against the checker asked with that limit."""
    s, hits = hold(pkg, orc, gpu, "segments", name, layout)
    hit = (hits["flags"] & pkg._abi.RT_RAYHIT_HIT) != 0
    assert (hits["t"][hit] <= s["rays"]["t_max"][hit]).all() and (hits["t"][hit] >= np.float32(0.001)).all()


@pytest.mark.parametrize("name,flags", [("book1", ()), ("field", ()), ("field", ("RT_LAYOUT_NODES_32B",)), ("field", ("RT_LAYOUT_WIDE_NODES",)),
                                        ("yard", ()), ("yard", ("RT_LAYOUT_NODES_32B",))])
def test_axis_rays_do_not_stall_a_walk(pkg, orc, gpu, name, flags):
    """What the cap of |1/d| in the three slab tests (csrc/kernels.hip set_slab_ray, set_grid_ray, the 8-wide refill) exists for: a ray
    with a zero component must not pass every box. The axis set against its twin — each zero-class component replaced by 1e-3 x the
    largest, an ordinary ray through nearly the same boxes — in the LDS walk (book1), the three HBM walks of `field` and the two of
    `yard` (where set_grid_ray / set_slab_ray run again after every LT_XFORM record, on a ray the transform made): the median of
    7 calls after a warm one, with the allowance test_edges uses for the host's jitter. A ray that passes every one of ~3,700 records
    costs some 50 x an ordinary one."""
    A = pkg._abi
    s = R.axis_set(pkg, orc, name)
    rays, other = s["rays"], R.twin(s["rays"])
    assert not R.zero_class(other["d"]).any() and R.zero_class(rays["d"]).any(axis=1).all()
    f = 0
    for word in flags:
        f |= getattr(A, word)
    scene = gpu.upload(s["built"].desc, f)
    try:
        ms = {}
        for label, r in (("axis", rays), ("twin", other)):
            trace_device(pkg, gpu, scene, r)                           # (warm)
            ms[label] = float(np.median([trace_device(pkg, gpu, scene, r, with_stats=True)[1]["render_ms"] for _ in range(7)]))
    finally:
        scene.close()
    print(f"{name} {'|'.join(flags) or 'default'}: median of 7 calls {ms['axis']:.3f} ms for the axis set, {ms['twin']:.3f} ms for its twin")
    assert ms["axis"] <= 1.5 * ms["twin"] + 0.1
