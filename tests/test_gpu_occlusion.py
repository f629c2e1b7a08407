"""Occlusion queries on the GPU (include/rt_hip.h, "occlusion queries"): the any-hit walk ray by ray against the f64 CPU checker in every
device layout; against the device's own closest hit, exactly, for every placement of t_max around it; the bit-for-bit invariances the
header promises; the edges; and the measurement script."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays as R  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = ("default", "reference_counters", "hbm", "hbm_32b", "hbm_wide")
CASES = [(s, l) for s in R.SCENES for l in LAYOUTS if l != "hbm_wide" or s in R.STATIC_SCENES]     # tests/test_gpu_rays.py::CASES


def layouts(A):
    return {"default": 0, "reference_counters": A.RT_LAYOUT_REFERENCE_COUNTERS, "hbm": A.RT_LAYOUT_SCENE_IN_HBM,
            "hbm_32b": A.RT_LAYOUT_SCENE_IN_HBM | A.RT_LAYOUT_NODES_32B, "hbm_wide": A.RT_LAYOUT_SCENE_IN_HBM | A.RT_LAYOUT_WIDE_NODES}


def to_device(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()


def occluded_device(gpu, scene, rays, options=None, with_stats=False):
    out = gpu.occluded(scene, to_device(rays), options=options, with_stats=with_stats)
    occ = (out[0] if with_stats else out).cpu().numpy()
    assert occ.dtype == np.uint8 and occ.shape == (len(rays),)
    return (occ, out[1]) if with_stats else occ


def trace_device(pkg, gpu, scene, rays):
    return gpu.trace_rays(scene, to_device(rays)).cpu().numpy().reshape(-1).view(pkg.RAYHIT_DTYPE)


@pytest.mark.parametrize("name,layout", CASES)
def test_occlusion_agrees_with_the_checker_and_the_closest_hit(pkg, orc, gpu, name, layout):
    """(1) t_max = no limit: the byte is the f64 checker's hit / miss on every decidable ray (rays.undecidable: R = 64 ulps, at most 1 % of
    a set). (2) against rt_trace_rays on the same scene and layout, with no exception: the any-hit walk compares the root the closest-hit
    walk computed with the limit the closest-hit export compares it with."""
    A = pkg._abi
    s = R.ray_set(pkg, orc, name)
    rays, ref, und = s["rays"], s["ref"], s["undecidable"]
    assert und.mean() <= 0.01
    scene = gpu.upload(s["built"].desc, layouts(A)[layout])
    try:
        occ, st = occluded_device(gpu, scene, rays, with_stats=True)
        assert st["segments"] == st["samples"] == len(rays)
        assert layout != "hbm_32b" or st["lds_top_nodes"] == 0      # M_HBM, not the top layout (tests/test_gpu_rays_hbm.py)
        assert np.isin(occ, (0, A.RT_RAYHIT_HIT)).all()
        dec = ~und
        wrong = dec & ((occ == A.RT_RAYHIT_HIT) != ref["hit"])
        print(f"{name}/{layout}: {len(rays)} rays, {int(und.sum())} undecidable (left out), {int((occ != 0).sum())} occluded")
        assert not wrong.any(), f"occluded differs from the checker on decidable rays {np.flatnonzero(wrong)[:8]}"
        # ---- the device's own closest hit ----
        base = trace_device(pkg, gpu, scene, rays)
        hit = (base["flags"] & A.RT_RAYHIT_HIT) != 0
        assert hit.any() and (~hit).any() and np.isfinite(base["t"][hit]).all() and (base["t"][hit] >= np.float32(0.001)).all()
        want = np.where(hit, A.RT_RAYHIT_HIT, 0).astype(np.uint8)
        assert (occ == want).all(), f"no limit: differs from rt_trace_rays at {np.flatnonzero(occ != want)[:8]}"
        f32 = np.float32

        def with_limit(on_hits, on_misses):
            q = rays.copy()
            q["t_max"] = np.where(hit, on_hits, f32(on_misses)).astype(f32)
            return occluded_device(gpu, scene, q)
        t = np.where(hit, base["t"], f32(1.0)).astype(f32)
        for label, limit, expect in (("0.5 t", t * f32(0.5), np.zeros(len(rays), np.uint8)), ("1.5 t", t * f32(1.5), want), ("t bit for bit", t, want),
                                     ("nextafter(t, 0)", np.nextafter(t, f32(0.0)), np.zeros(len(rays), np.uint8))):
            for finite in (1.0, 1e-2, 1e6):                  # misses, with any finite limit: 0
                got = with_limit(limit, finite)
                assert (got == expect).all(), f"t_max = {label} (misses {finite}): differs at {np.flatnonzero(got != expect)[:8]}"
        for none in (0.0, -1.0, np.inf, np.nan):             # "no limit", every spelling
            q = rays.copy(); q["t_max"] = f32(none)
            assert (occluded_device(gpu, scene, q) == want).all(), none
    finally:
        scene.close()


FIVE_SCENES = [(s, l) for s in R.SEGMENT_SCENES for l in LAYOUTS if l != "hbm_wide" or s != "moving"]


@pytest.mark.parametrize("name,layout", FIVE_SCENES)
def test_segments_blocked_or_not(pkg, orc, gpu, name, layout):
    """Shadow rays as INTEGRATION.md section 12 tells callers to write them — d = q - p, t_max near 1 (rays.segment_set: 0.98 onto a
    surface, 1.5 past a free point): the byte is the f64 checker's blocked / unblocked on every decidable segment, and rt_trace_rays'
    hit / miss under the same t_max on EVERY segment."""
    A = pkg._abi
    s = R.segment_set(pkg, orc, name)
    rays, ref, dec = s["rays"], s["ref"], s["decidable"]
    scene = gpu.upload(s["built"].desc, layouts(A)[layout])
    try:
        occ, st = occluded_device(gpu, scene, rays, with_stats=True)
        base = trace_device(pkg, gpu, scene, rays)
    finally:
        scene.close()
    assert st["segments"] == st["samples"] == len(rays) and np.isin(occ, (0, A.RT_RAYHIT_HIT)).all()
    blocked = occ == A.RT_RAYHIT_HIT
    print(f"segments/{name}/{layout}: {len(rays)} segments, {int((~dec).sum())} undecidable (left out), {int(blocked.sum())} blocked")
    wrong = np.flatnonzero(dec & (blocked != ref["hit"]))
    assert len(wrong) == 0, f"blocked / unblocked differs from the checker on decidable segments {wrong[:8]}"
    hit = (base["flags"] & A.RT_RAYHIT_HIT) != 0
    assert (blocked == hit).all(), f"differs from rt_trace_rays under the same t_max at {np.flatnonzero(blocked != hit)[:8]}"
    assert blocked.mean() > 0.25 and (~blocked).mean() > 0.2


@pytest.mark.parametrize("name,layout", [(s, l) for s in R.AXIS_SCENES for l in LAYOUTS if l != "hbm_wide" or s != "moving"])
def test_axis_rays_any_hit_equals_the_closest_hit(pkg, orc, gpu, name, layout):
    """The axis sets (rays.axis_set), no limit: the byte is rt_trace_rays' hit / miss on every ray, and the checker's on the decidable ones."""
    A = pkg._abi
    s = R.axis_set(pkg, orc, name)
    scene = gpu.upload(s["built"].desc, layouts(A)[layout])
    try:
        occ = occluded_device(gpu, scene, s["rays"])
        base = trace_device(pkg, gpu, scene, s["rays"])
    finally:
        scene.close()
    hit = (base["flags"] & A.RT_RAYHIT_HIT) != 0
    want = np.where(hit, A.RT_RAYHIT_HIT, 0).astype(np.uint8)
    assert (occ == want).all(), f"no limit: differs from rt_trace_rays at {np.flatnonzero(occ != want)[:8]}"
    wrong = np.flatnonzero(s["decidable"] & ((occ != 0) != s["ref"]["hit"]))
    assert len(wrong) == 0, f"occluded differs from the checker on decidable axis rays {wrong[:8]}"


def test_the_sets_cover_what_the_header_names(pkg, orc, gpu):
    """Cornell: hits inside RotateY / Translate instances and on Box sides; moving: ray times that matter; mesh: triangles."""
    A = pkg._abi
    for name, kinds in (("cornell", {A.RT_HIT_BOX}), ("moving", {A.RT_HIT_MOVING_SPHERE}), ("mesh", {A.RT_HIT_TRIANGLE})):
        s = R.ray_set(pkg, orc, name)
        scene = gpu.upload(s["built"].desc)
        base = trace_device(pkg, gpu, scene, s["rays"])
        scene.close()
        hit = (base["flags"] & A.RT_RAYHIT_HIT) != 0
        seen = {s["built"].desc.hittables[int(h)].kind for h in base["hittable"][hit]}
        assert kinds <= seen, (name, seen)
    assert np.ptp(R.ray_set(pkg, orc, "moving")["rays"]["time"]) > 0.5


def test_invariances_bit_for_bit(pkg, orc, gpu):
    s = R.ray_set(pkg, orc, "book1")
    rays = np.concatenate([s["rays"]] * 4)                       # ~10 k rays: longer than a small pool
    # a finite limit on every other ray, so that both kinds of interval are in the list
    rays["t_max"][1::2] = 6.0
    scene = gpu.upload(s["built"].desc)
    base = occluded_device(gpu, scene, rays)
    assert 0 < int((base != 0).sum()) < len(rays)
    # two calls give equal bytes
    assert base.tobytes() == occluded_device(gpu, scene, rays).tobytes()
    # chunks: a pool of 4096 slots runs the list in three chunks
    small, st = occluded_device(gpu, scene, rays, options=pkg.ray_query_options(pool_slots=4096), with_stats=True)
    assert st["pool_slots"] == 4096 and st["extend_launches"] == -(-len(rays) // 4096) == 3
    assert small.tobytes() == base.tobytes()
    # a permuted list gives the permuted bytes
    perm = np.random.default_rng(3).permutation(len(rays))
    assert occluded_device(gpu, scene, rays[perm]).tobytes() == base[perm].tobytes()
    # the host variant equals the device variant; the (n, 8) float form equals the structured form
    host = gpu.occluded(scene, rays)
    assert isinstance(host, np.ndarray) and host.dtype == np.uint8 and host.tobytes() == base.tobytes()
    assert gpu.occluded(scene, np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)).tobytes() == base.tobytes()
    scene.close()


def test_pool_rule(pkg, orc, gpu):
    """The pool of an occlusion query is the ray query's (tests/test_gpu_rays.py::test_pool_rule): a multiple of 512 x 8 slots that holds
    every chunk, whatever pool_slots asks for, and the same bytes for every pool."""
    s = R.ray_set(pkg, orc, "mesh")
    scene = gpu.upload(s["built"].desc)
    rays = np.concatenate([s["rays"]] * 5)
    base = None
    for n in (1, 511, 513, 4097, len(rays)):
        for pool_slots in (0, 1, 4096, 5000, 1 << 20):
            occ, st = occluded_device(gpu, scene, rays[:n], options=pkg.ray_query_options(pool_slots=pool_slots), with_stats=True)
            want = -(-min(pool_slots or (1 << 28), n) // 4096) * 4096
            assert st["pool_slots"] == want, (n, pool_slots, st["pool_slots"], want)
            assert st["extend_launches"] == -(-n // want) and st["segments"] == n, (n, pool_slots, st)
            if n == len(rays):
                base = occ if base is None else base
                assert occ.tobytes() == base.tobytes(), (n, pool_slots)
    scene.close()


def test_edges(pkg, orc, gpu):
    import torch
    A = pkg._abi
    s = R.ray_set(pkg, orc, "book1")
    rays = s["rays"]
    scene = gpu.upload(s["built"].desc)
    base = occluded_device(gpu, scene, rays)
    # invalid rays, mixed into the list, come back as 4; their neighbours' bytes are unchanged; samples = segments = the valid rays
    bad = rays.copy()
    k = np.arange(5, len(rays), 7)
    third = len(k) // 3
    bad["d"][k[:third]] = 0.0
    bad["o"][k[third:2 * third], 1] = np.nan
    bad["d"][k[2 * third:], 2] = np.inf
    bad["time"][k[::5]] = -np.inf
    got, st = occluded_device(gpu, scene, bad, with_stats=True)
    ok = np.ones(len(rays), bool); ok[k] = False
    assert (got[ok] == base[ok]).all() and (got[k] == A.RT_RAYHIT_INVALID_RAY).all()
    assert st["segments"] == st["samples"] == len(rays) - len(k)
    # a list of invalid rays only: flagged throughout (host and device variant)
    only, st = occluded_device(gpu, scene, bad[k], with_stats=True)
    assert (only == A.RT_RAYHIT_INVALID_RAY).all() and st["segments"] == 0
    assert (gpu.occluded(scene, bad[k]) == A.RT_RAYHIT_INVALID_RAY).all()
    # n_rays = 0 is a no-op
    assert len(gpu.occluded(scene, rays[:0])) == 0
    assert gpu.occluded(scene, torch.empty((0, 8), dtype=torch.float32, device="cuda")).numel() == 0
    # timing on request
    _, st = occluded_device(gpu, scene, rays, options=pkg.ray_query_options(flags=A.RT_FLAG_TIMING), with_stats=True)
    assert st["extend_ms"] > 0.0 and st["other_ms"] > 0.0 and st["render_ms"] > 0.0
    # n bytes are written and no more: a canary behind them stays (an odd offset too: the bytes need no alignment)
    dev_rays = to_device(rays)
    n = len(rays)
    for off in (0, 1, 3):
        buf = torch.full((off + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        gpu.occluded(scene, dev_rays, out=buf[off:off + n])
        got = buf.cpu().numpy()
        assert (got[:off] == 0xA5).all() and (got[off + n:] == 0xA5).all() and (got[off:off + n] == base).all(), off
    # refused options: RT_ERR_INVALID, nothing written; the context goes on answering
    poison = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    for opt in (A.RtRayQueryOptions(16, 1 << 7, 0, 0), A.RtRayQueryOptions(0, 0, 0, 0), A.RtRayQueryOptions(16, A.RT_FLAG_COUNTERS, 0, 0)):
        with pytest.raises(pkg.RtError) as e:
            gpu.occluded(scene, dev_rays, options=opt, out=poison)
        assert e.value.code == A.RT_ERR_INVALID
        assert bool((poison == 0x5A).all())
    lib = pkg.lib()
    import ctypes as C
    assert lib.rt_occluded_rays_device(gpu._h, scene._h, None, None, n, C.c_void_p(poison.data_ptr()), None) == A.RT_ERR_INVALID      # NULL rays
    assert lib.rt_occluded_rays_device(gpu._h, scene._h, None, C.c_void_p(dev_rays.data_ptr()), n, None, None) == A.RT_ERR_INVALID    # NULL output
    assert lib.rt_occluded_rays_device(gpu._h, scene._h, None, C.c_void_p(dev_rays.data_ptr()), 1 << 32, C.c_void_p(poison.data_ptr()), None) == A.RT_ERR_INVALID
    # a device ray list that is not 16-byte aligned is refused (the bytes may lie anywhere: the canary runs above)
    skew = torch.zeros((n * 8 + 1,), dtype=torch.float32, device="cuda")[1:]
    assert skew.data_ptr() % 16 != 0
    assert lib.rt_occluded_rays_device(gpu._h, scene._h, None, C.c_void_p(skew.data_ptr()), n, C.c_void_p(poison.data_ptr()), None) == A.RT_ERR_INVALID
    assert b"aligned" in lib.rt_last_error(gpu._h)
    assert bool((poison == 0x5A).all())
    assert (occluded_device(gpu, scene, rays) == base).all()
    scene.close()
    # a scene with a medium: RT_ERR_UNSUPPORTED, the poisoned output untouched (device and host variant)
    fog = R.medium_scene(pkg)
    scene = gpu.upload(fog.desc)
    with pytest.raises(pkg.RtError) as e:
        gpu.occluded(scene, dev_rays, out=poison)
    assert e.value.code == A.RT_ERR_UNSUPPORTED and "medium" in str(e.value).lower()
    assert bool((poison == 0x5A).all())
    host_out = np.full(n, 0x5A, np.uint8)
    with pytest.raises(pkg.RtError) as e:
        gpu.occluded(scene, rays, out=host_out)
    assert e.value.code == A.RT_ERR_UNSUPPORTED and (host_out == 0x5A).all()
    scene.close()
    # ... and the context answers the next scene
    scene = gpu.upload(s["built"].desc)
    assert (occluded_device(gpu, scene, rays) == base).all()
    scene.close()


def test_measurement_script_runs(tmp_path):
    """scripts/gpu_occlusion.py (the table of DESIGN.md section 11) runs in a process of its own, at a tiny size, and reports what it says."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "occlusion.json"
    subprocess.run([sys.executable, os.path.join(root, "scripts", "gpu_occlusion.py"), "--reps", "2", "--scale", "0.1", "--out", str(out)], check=True,
                   timeout=300, cwd=root)
    rows = json.loads(out.read_text())["sets"]
    assert {(r["scene"], r["rays_kind"]) for r in rows} == {(sc, k) for sc in ("book1", "cornell", "mesh_hbm") for k in ("primary", "shadow")}
    for r in rows:
        assert r["rays"] > 0 and 0 <= r["occluded"] <= r["rays"] and r["agree_with_closest_hit"] is True
        for side in ("occluded", "trace"):
            assert r[side + "_ms"] > 0 and r[side + "_extend_ms"] > 0 and r[side + "_other_ms"] > 0
        assert abs(r["speedup"] - r["trace_ms"] / r["occluded_ms"]) <= 0.01 * r["speedup"] + 1e-3
