"""The walks of a scene that does NOT fit LDS, ray by ray (tests/rays.py, scene `field`: ~3,700 records, more than the default LDS top of
1024 and at most the 4096 a top can hold): every upload of rays.field_matrix — compressed records per direction octant (every choice
of octant axes), 32-byte records with a top of 1 .. 1024 records in LDS (k_extend's M_TOP) or none (M_HBM), member boxes, the
reference's lists, a park cost, the 8-wide tree, collapsed leaves — against the f64 CPU checker, against the device's own closest hit
through the any-hit walk, and bit for bit against each other; the same for the scene's axis set (rays.axis_set: axis-parallel rays, rim
rays on the ground rect's edges, edge rays on the height field's border); and one small render through the top layouts and the three carriers.

And the same for `yard` (rays.yard_scene: ~3,800 records): a BVH over a time range with moving spheres, 80 Boxes under a transform each,
rects of every axis (half of them under FlipFace) and four kinds of instance — a rotated and translated BVH of spheres, a chain of three
wrappers over a mesh, an instance whose own frame lies 400 units from where it stands (moving spheres inside), and two groups under
RotateY(90) and RotateY(180). What `field` cannot reach: LT_XFORM records in M_C16 (a lane stays on the record array of its world
octant while its local direction lies in another), in M_TOP (enter and exit in LDS, the instance's records in HBM) and M_HBM; the
compressed grid stretched over instance-local boxes; LT_MOVING; and WIDE_NODES on a scene that is no static BVH, which keeps the
binary walk and must give the default upload's bytes.

The scene's surfaces are disjoint, so no ray finds two primitives at one t: the one way layouts may differ (include/rt_hip.h, the layout
section) is absent, and what the header promises is equality of the records, not closeness. (The axis set holds four exceptions, which
test_the_matrix_bit_for_bit_on_axis_rays names: rays straight down onto a corner vertex of the height field that two triangles share.)

Tolerance of t, p, n, u, v: 2 x rays.MEASURED_F32_CHECKER[scene], the CPU checker's f32 instance against its f64 answers on this set —
the factor and the rule of tests/test_gpu_paths.py. Nothing in it comes from the device, whose own worst figures are recorded
(record_metric) and tabled in DESIGN.md section 11."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays as R  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = ("field", "yard")
TOP_SIZES = {"field": (1, 2, 3, 7, 100, 1024, 4096), "yard": (1, 2, 3, 7, 100, 1024, 4096, R.YARD_TOP)}
TOPS = {scene: [f"top_{k}" for k in TOP_SIZES[scene]] for scene in SCENES}
CASES = {scene: ["c16", "c16_one_order"] + [f"c16_axes_{k}" for k in range(1, 8)] + TOPS[scene] +
         ["top_one_order", "member_boxes", "lists_as_reference", "lists_as_reference_top_7", "park_cost", "wide", "collapse_4", "collapse_4_hbm",
          "c16_sah", "top_1024_sah", "wide_sah"] for scene in SCENES}
BASE = {"field": "c16_one_order", "yard": "c16_one_order"}
# the uploads of `yard` that ask for the 8-wide tree and get the binary walk (no static BVH), and the upload each must equal byte for byte
WIDE_KEEPS_BINARY = {"wide": "c16", "wide_sah": "c16_sah"}

_results = {}
_uploads = {}          # (scene, case) -> uploads made for it: 1, asserted by the matrix tests


def to_device(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()


def run_case(pkg, orc, gpu, scene, case):
    """One upload per scene and case: the closest hits with their stats, and the any-hit bytes for the three limits of (c), for the
    scene's ray set and for its axis set. Kept per process."""
    if (scene, case) in _results:
        return _results[scene, case]
    A = pkg._abi
    name, flags, more = R.field_matrix(A, scene)[case]
    s = R.ray_set(pkg, orc, name)
    rays = s["rays"]
    f32 = np.float32
    _uploads[scene, case] = _uploads.get((scene, case), 0) + 1
    up = gpu.upload(s["built"].desc, flags, **more)
    try:
        out, st = gpu.trace_rays(up, to_device(rays), with_stats=True)
        hits = out.cpu().numpy().reshape(-1).view(pkg.RAYHIT_DTYPE)

        def any_hit(rays, hits):
            hit = (hits["flags"] & A.RT_RAYHIT_HIT) != 0
            occ = {}
            for label, limit in (("none", np.zeros(len(rays), f32)), ("t", np.where(hit, hits["t"], f32(1.0)).astype(f32)),
                                 ("below", np.where(hit, np.nextafter(hits["t"], f32(0.0)), f32(1.0)).astype(f32))):
                q = rays.copy()
                q["t_max"] = limit
                o, ost = gpu.occluded(up, to_device(q), with_stats=True)
                occ[label] = o.cpu().numpy()
                assert ost["bvh_in_lds"] == st["bvh_in_lds"] and ost["lds_top_nodes"] == st["lds_top_nodes"] and ost["segments"] == len(rays)
            return occ
        occ = any_hit(rays, hits)
        # the axis set (rays.axis_set) through the same upload
        axis = R.axis_set(pkg, orc, name)
        out, ast = gpu.trace_rays(up, to_device(axis["rays"]), with_stats=True)
        axis_hits = out.cpu().numpy().reshape(-1).view(pkg.RAYHIT_DTYPE)
        assert ast["segments"] == ast["samples"] == len(axis["rays"]) and ast["lds_top_nodes"] == st["lds_top_nodes"] and ast["bvh_in_lds"] == st["bvh_in_lds"]
        axis_occ = any_hit(axis["rays"], axis_hits)
    finally:
        up.close()
    _results[scene, case] = dict(set=s, flags=flags, more=more, hits=hits, stats=st, occ=occ, axis=axis, axis_hits=axis_hits, axis_occ=axis_occ)
    return _results[scene, case]


def test_the_matrix_is_the_one_of_rays_py(pkg):
    for scene in SCENES:
        assert sorted(CASES[scene]) == sorted(R.field_matrix(pkg._abi, scene))
    assert len(CASES["yard"]) == len(CASES["field"]) + 1


def hold_rays(pkg, orc, gpu, scene, case):
    from conftest import record_metric
    A = pkg._abi
    r = run_case(pkg, orc, gpu, scene, case)
    s, hits, st, flags, more = r["set"], r["hits"], r["stats"], r["flags"], r["more"]
    built, rays, ref, und = s["built"], s["rays"], s["ref"], s["undecidable"]
    assert st["segments"] == st["samples"] == len(rays)
    # ---- (a) which kernel ran ----
    want_top = 0
    if flags & A.RT_LAYOUT_NODES_32B:
        skip = pkg.compile_dump(built.desc, flags, **more)[0]["skip"]
        want_top = R.top_rule(skip, min(more.get("lds_top_records", 0) or 1024, 4096))
    print(f"{case}: bvh_in_lds {st['bvh_in_lds']}, lds_top_nodes {st['lds_top_nodes']} (the depth-cut rule gives {want_top}), {st['scene_nodes']} records")
    record_metric(config="rays_hbm_kernel", scene=scene, case=case, bvh_in_lds=int(st["bvh_in_lds"]), lds_top_nodes=int(st["lds_top_nodes"]), top_rule=int(want_top),
                  scene_nodes=int(st["scene_nodes"]))
    assert st["bvh_in_lds"] == (1 if case in R.FITS_LDS else 0)
    assert st["lds_top_nodes"] == want_top
    if case in ("top_7", "top_100", "top_1024", "top_1024_sah", "top_one_order", "lists_as_reference_top_7", f"top_{R.YARD_TOP}"):
        assert st["lds_top_nodes"] > 0, "this case is meant to run M_TOP"
    if case == "top_4096":
        assert st["lds_top_nodes"] == 0, "the whole tree fits a top of 4096 records: M_HBM"
    if scene == "yard" and case in WIDE_KEEPS_BINARY:
        # RtStats does not name the walk: what it shows is that the upload holds the default layout's records, and nothing of an 8-wide tree
        other = run_case(pkg, orc, gpu, scene, WIDE_KEEPS_BINARY[case])
        assert all(st[k] == other["stats"][k] for k in ("scene_nodes", "scene_prims", "scene_bytes", "bvh_in_lds", "lds_top_nodes")), (st, other["stats"])
        assert hits.tobytes() == other["hits"].tobytes() and r["axis_hits"].tobytes() == other["axis_hits"].tobytes(), "WIDE_NODES on a scene that keeps the binary walk"
        assert all((r[o][k] == other[o][k]).all() for o in ("occ", "axis_occ") for k in ("none", "t", "below"))
    # ---- (b) against the checker, on decidable rays ----
    g_hit, g_ff = (hits["flags"] & A.RT_RAYHIT_HIT) != 0, (hits["flags"] & A.RT_RAYHIT_FRONT_FACE) != 0
    assert ((hits["flags"] & ~np.uint32(3)) == 0).all()
    dec = ~und
    print(f"{case}: {len(rays)} rays, {int(und.sum())} undecidable (left out), {int((g_hit & dec).sum())} hits compared")
    left = s["by_origin"]             # (reported: what the device makes of the rays that only the rule on the origin leaves out)
    other = left & ((g_hit != ref["hit"]) | (g_hit & ref["hit"] & (np.abs(hits["t"] - ref["t"]) > 1e-3 * np.maximum(1.0, ref["t"]))))
    print(f"{case}: of {int(left.sum())} rays left out by the rule on the origin alone the device answers {int(other.sum())} as the checker does not: {np.flatnonzero(other).tolist()}")
    wrong = dec & (g_hit != ref["hit"])
    assert not wrong.any(), f"hit/miss differs on decidable rays {np.flatnonzero(wrong)[:8]}"
    both = dec & g_hit
    wrong = both & (g_ff != ref["ff"])
    assert not wrong.any(), f"front_face differs on decidable rays {np.flatnonzero(wrong)[:8]}"
    miss = ~g_hit
    assert np.isposinf(hits["t"][miss]).all() and (hits["hittable"][miss] == -1).all() and (hits["material"][miss] == -1).all()
    assert (hits["flags"][miss] == 0).all() and not hits["p"][miss].any() and not hits["n"][miss].any() and not hits["u"][miss].any() and not hits["v"][miss].any()
    ids, on = s["ids"], s["on"]
    col = np.full(built.desc.n_hittables, -1)
    col[ids] = np.arange(len(ids))
    k = np.flatnonzero(both)
    h = hits["hittable"][k]
    assert ((h >= 0) & (h < len(col))).all() and (col[h] >= 0).all(), "a hittable that is not a primitive record"
    off = k[~on[k, col[h]]]
    assert len(off) == 0, f"rays {off[:8]}: the checker's hit point does not lie on the reported hittable {hits['hittable'][off[:8]]}"
    mat = np.array([built.desc.hittables[int(i)].material for i in h])
    assert (hits["material"][k] == mat).all(), f"material differs on rays {k[hits['material'][k] != mat][:8]}"
    worst, at = R.deviations(pkg, s, k, hits["t"], hits["p"], hits["n"], hits["u"], hits["v"])
    bound = {q: 2.0 * v for q, v in R.MEASURED_F32_CHECKER[scene].items()}
    print(f"{case}: worst rel|dt| {worst['t']:.3e}  |dp|/extent {worst['p']:.3e}  |dn| {worst['n']:.3e}  |d(u,v)| {worst['uv']:.3e}  |dt|/max(1,t) {worst['ta']:.3e}"
          f"  at rays {at}")
    record_metric(config="rays_hbm", scene=scene, case=case, dta=worst["ta"], dt=worst["t"], dp=worst["p"], dn=worst["n"], duv=worst["uv"], undecidable=int(und.sum()),
                  rays=len(rays))
    for q in bound:
        assert worst[q] <= bound[q], (q, worst[q], bound[q], at[q])
    # ---- (c) the any-hit walk on the same upload against the closest hit, exactly ----
    want = np.where(g_hit, A.RT_RAYHIT_HIT, 0).astype(np.uint8)
    occ = r["occ"]
    assert (occ["none"] == want).all(), f"no limit: differs from the closest hit at {np.flatnonzero(occ['none'] != want)[:8]}"
    assert (occ["t"] == want).all(), f"t_max = t bit for bit: differs at {np.flatnonzero(occ['t'] != want)[:8]}"
    assert not occ["below"].any(), f"t_max = nextafter(t, 0) (misses: 1.0): occluded at {np.flatnonzero(occ['below'])[:8]}"


@pytest.mark.parametrize("case", CASES["field"])
def test_field_rays(pkg, orc, gpu, case):
    hold_rays(pkg, orc, gpu, "field", case)


@pytest.mark.parametrize("case", CASES["yard"])
def test_yard_rays(pkg, orc, gpu, case):
    """test_field_rays for `yard`. u, v of a moving sphere are 0 by the header, in the checker as on the device: compared as such."""
    hold_rays(pkg, orc, gpu, "yard", case)


def describe(pkg, s, a, b, i):
    d = s["built"].desc
    on = s["ids"][s["on"][i]]
    return (f"ray {i}: t {a['t'][i]!r} / {b['t'][i]!r}, hittable {a['hittable'][i]} / {b['hittable'][i]} "
            f"(kinds {d.hittables[max(int(a['hittable'][i]), 0)].kind} / {d.hittables[max(int(b['hittable'][i]), 0)].kind}), flags {a['flags'][i]} / {b['flags'][i]}, "
            f"checker t {s['ref']['t'][i]!r} on hittables {on.tolist()}")


def matrix_bit_for_bit(pkg, orc, gpu, scene):
    """(d) On decidable rays every binary walk — and the 8-wide walk, which calls the same primitive functions — returns the RtRayHit bytes
    of c16_one_order, whatever the records, their order, their memory or the BVH builder; the top_k cases (same records, same order, another
    memory) equal each other on ALL rays; collapsed leaves give the same hittable and the same t bits."""
    from conftest import record_metric
    base_case, cases, tops = BASE[scene], CASES[scene], TOPS[scene]
    base = run_case(pkg, orc, gpu, scene, base_case)
    s = base["set"]
    dec = ~s["undecidable"]
    differing = {}
    for case in cases:
        got = run_case(pkg, orc, gpu, scene, case)["hits"]
        if case in ("collapse_4", "collapse_4_hbm"):
            bad = dec & ((got["hittable"] != base["hits"]["hittable"]) | (got["t"].view(np.uint32) != base["hits"]["t"].view(np.uint32)))
        else:
            bad = dec & (got.view(np.uint8).reshape(len(got), -1) != base["hits"].view(np.uint8).reshape(len(got), -1)).any(axis=1)
        differing[case] = np.flatnonzero(bad)
        if bad.any():
            print(f"{case} against {base_case}: " + "; ".join(describe(pkg, s, got, base["hits"], int(i)) for i in differing[case][:4]))
    total = int(sum(len(v) for v in differing.values()))
    print(f"decidable rays that differ from {base_case}, over {len(cases)} uploads: {total}  {({c: len(v) for c, v in differing.items() if len(v)})}")
    record_metric(config="rays_hbm_matrix", scene=scene, uploads=len(cases), decidable_rays_differing=total)
    made = {k: v for k, v in _uploads.items() if k[0] == scene}
    print(f"uploads made for {scene}: {sum(made.values())} for {len(made)} cases")
    assert set(made) == {(scene, c) for c in cases} and set(made.values()) == {1}, "run_case keeps one upload per scene and case"
    first = run_case(pkg, orc, gpu, scene, tops[0])["hits"]
    for case in tops[1:]:
        got = run_case(pkg, orc, gpu, scene, case)["hits"]
        assert got.tobytes() == first.tobytes(), f"{case} differs from {tops[0]} on rays {np.flatnonzero((got.view(np.uint8).reshape(len(got), -1) != first.view(np.uint8).reshape(len(got), -1)).any(axis=1))[:8]}"
    assert total == 0, {c: v[:8].tolist() for c, v in differing.items() if len(v)}


def test_the_matrix_bit_for_bit(pkg, orc, gpu):
    matrix_bit_for_bit(pkg, orc, gpu, "field")


def test_yard_matrix_bit_for_bit(pkg, orc, gpu):
    """matrix_bit_for_bit for `yard`: 28 uploads, every one a binary walk (the two WIDE_NODES uploads fell back to it)."""
    matrix_bit_for_bit(pkg, orc, gpu, "yard")


def hold_axis_rays(pkg, orc, gpu, scene, case):
    """The axis set of `field` (rays.axis_set: zero-class direction components, origins on the 1/4 lattice, rim rays on the ground rect's
    edges — the rect a walk tests when it begins — and edge rays on the height field's border) through every upload of the matrix: (b)
    against the f64 checker, within 2 x the f32 checker's figures of that set; (c) the any-hit walk against the closest hit, exactly."""
    from conftest import record_metric
    A = pkg._abi
    r = run_case(pkg, orc, gpu, scene, case)
    s, hits = r["axis"], r["axis_hits"]
    worst, _ = R.hold_to_checker(pkg, s, hits, "axis/" + scene, f"axis/{scene}/{case}")
    record_metric(config="rays_hbm_axis", scene=scene, case=case, dta=worst["ta"], dt=worst["t"], dp=worst["p"], dn=worst["n"], duv=worst["uv"], dtabs=worst["tabs"],
                  undecidable=int(s["undecidable"].sum()), rays=len(s["rays"]))
    g_hit = (hits["flags"] & A.RT_RAYHIT_HIT) != 0
    assert g_hit[s["rim"]].all() and g_hit[s["edge"]].all()
    want = np.where(g_hit, A.RT_RAYHIT_HIT, 0).astype(np.uint8)
    occ = r["axis_occ"]
    assert (occ["none"] == want).all(), f"no limit: differs from the closest hit at {np.flatnonzero(occ['none'] != want)[:8]}"
    assert (occ["t"] == want).all(), f"t_max = t bit for bit: differs at {np.flatnonzero(occ['t'] != want)[:8]}"
    assert not occ["below"].any(), f"t_max = nextafter(t, 0) (misses: 1.0): occluded at {np.flatnonzero(occ['below'])[:8]}"


@pytest.mark.parametrize("case", CASES["field"])
def test_field_axis_rays(pkg, orc, gpu, case):
    hold_axis_rays(pkg, orc, gpu, "field", case)


@pytest.mark.parametrize("case", CASES["yard"])
def test_yard_axis_rays(pkg, orc, gpu, case):
    """test_field_axis_rays for `yard`: the seeded origins inside the footprints of A, B and D, where xform_ray turns a world axis ray
    into a local ray with components the transform made (6e-17 under RotateY(90) and RotateY(180)) before set_slab_ray / set_grid_ray
    see it; rim rays on the ground rect, which lies beside the BVH in a list here."""
    hold_axis_rays(pkg, orc, gpu, "yard", case)


def matrix_bit_for_bit_on_axis_rays(pkg, orc, gpu, scene):
    """(d) for the axis set: on its decidable rays — rim and edge rays among them — every walk returns the RtRayHit bytes of c16_one_order
    (collapsed leaves: the same hittable and the same t bits), and the top_k cases equal each other on ALL rays. The one way layouts may
    differ (include/rt_hip.h, the layout section) is present here on a handful of rays: an edge ray straight down onto a corner vertex
    of the height field that two triangles share finds both at one t, and which of them reports the hit is the walk's choice. On the
    rays whose checker point lies on two primitives the t and p bits must agree (the hittable is held to the checker's point by
    test_field_axis_rays); everywhere else, every byte."""
    from conftest import record_metric
    base_case, cases, tops = BASE[scene], CASES[scene], TOPS[scene]
    base = run_case(pkg, orc, gpu, scene, base_case)
    s = base["axis"]
    dec = s["decidable"]
    assert dec[s["rim"]].all() and dec[s["edge"]].all()
    tie = s["ref"]["hit"] & (s["on"].sum(axis=1) >= 2)
    print(f"axis rays whose hit point lies on two primitives: {np.flatnonzero(tie).tolist()}")
    # (field: the corner vertices its edge rays aim at; yard: whatever shared edges of B's mesh the seeded rays find by themselves)
    assert (0 if scene == "yard" else 1) <= tie.sum() <= 8 and s["edge"][tie].all()
    tp = lambda h: np.concatenate([h["t"].view(np.uint32)[:, None], h["p"].view(np.uint32)], axis=1)
    differing = {}
    for case in cases:
        got = run_case(pkg, orc, gpu, scene, case)["axis_hits"]
        if case in ("collapse_4", "collapse_4_hbm"):
            bad = dec & ~tie & ((got["hittable"] != base["axis_hits"]["hittable"]) | (got["t"].view(np.uint32) != base["axis_hits"]["t"].view(np.uint32)))
        else:
            bad = dec & ~tie & (got.view(np.uint8).reshape(len(got), -1) != base["axis_hits"].view(np.uint8).reshape(len(got), -1)).any(axis=1)
        bad |= tie & (tp(got) != tp(base["axis_hits"])).any(axis=1)
        differing[case] = np.flatnonzero(bad)
        if bad.any():
            print(f"{case} against {base_case}: " + "; ".join(describe(pkg, s, got, base["axis_hits"], int(i)) for i in differing[case][:4]))
    total = int(sum(len(v) for v in differing.values()))
    print(f"decidable axis rays that differ from {base_case}, over {len(cases)} uploads: {total}  {({c: len(v) for c, v in differing.items() if len(v)})}")
    record_metric(config="rays_hbm_axis_matrix", scene=scene, uploads=len(cases), decidable_rays_differing=total)
    assert all(v == 1 for k, v in _uploads.items() if k[0] == scene), "run_case keeps one upload per scene and case"
    first = run_case(pkg, orc, gpu, scene, tops[0])["axis_hits"]
    for case in tops[1:]:
        assert run_case(pkg, orc, gpu, scene, case)["axis_hits"].tobytes() == first.tobytes(), case
    assert total == 0, {c: v[:8].tolist() for c, v in differing.items() if len(v)}


def test_the_matrix_bit_for_bit_on_axis_rays(pkg, orc, gpu):
    matrix_bit_for_bit_on_axis_rays(pkg, orc, gpu, "field")


def test_yard_matrix_bit_for_bit_on_axis_rays(pkg, orc, gpu):
    matrix_bit_for_bit_on_axis_rays(pkg, orc, gpu, "yard")


def render_through_the_top_layouts(pkg, orc, gpu, name):
    """A render of the same scene (32 x 24, 4 spp, depth 8): the frame and the segment count are the same bytes whether the top in LDS holds
    7, 63, 1023 records or none (M_TOP against M_HBM); with a top of 7 the wavefront loop run to the end (tail_paths = 1), the drain
    hand-over (the default: M_TOP with DRAIN) and the fused kernel give one frame; and against the default compressed layout fewer than
    2e-3 of the pixels differ, the share tests/test_gpu_scenes.py allows between layouts."""
    A = pkg._abi
    built = R.ray_set(pkg, orc, name)["built"]
    W, H, SPP = 32, 24, 4
    prm = lambda **kw: pkg.make_params(W, H, SPP, max_depth=8, seed=20240917, **kw)
    frames = {}
    for top in (7, 100, 0, 4096):
        scene = gpu.upload(built.desc, A.RT_LAYOUT_NODES_32B, lds_top_records=top)
        try:
            img, st = gpu.render(scene, built.cam, prm())
            assert st["bvh_in_lds"] == 0 and (st["lds_top_nodes"] > 0) == (top != 4096), (top, st["lds_top_nodes"])
            assert st["samples"] == W * H * SPP and np.isfinite(img).all()
            frames[top] = (img, st["segments"])
            if top == 7:
                assert st["drain_paths"] > 0                         # the default: the drain kernel carried the paths, in M_TOP
                loop, sl = gpu.render(scene, built.cam, prm(tail_paths=1))
                assert sl["drain_paths"] == 0 and sl["lds_top_nodes"] == st["lds_top_nodes"]
                fused, sf = gpu.render(scene, built.cam, prm(flags=A.RT_FLAG_FUSED, tail_paths=1))
                assert sf["drain_paths"] > 0
                assert loop.tobytes() == img.tobytes() == fused.tobytes() and sl["segments"] == st["segments"] == sf["segments"]
        finally:
            scene.close()
    for top in (100, 0, 4096):
        assert frames[top][0].tobytes() == frames[7][0].tobytes() and frames[top][1] == frames[7][1], top
    scene = gpu.upload(built.desc)
    try:
        c16, st = gpu.render(scene, built.cam, prm())
        assert st["bvh_in_lds"] == 0 and st["lds_top_nodes"] == 0
    finally:
        scene.close()
    share = float((np.abs(c16 - frames[7][0]).max(axis=2) > 0).mean())
    print(f"pixels that differ between top_7 and the default compressed layout: {share:.4f}; segments {frames[7][1]} / {st['segments']}")
    assert share < 2e-3


def test_field_render_through_the_top_layouts(pkg, orc, gpu):
    render_through_the_top_layouts(pkg, orc, gpu, "field")


def test_yard_render_through_the_top_layouts(pkg, orc, gpu):
    """render_through_the_top_layouts for `yard`, shutter 0 .. 1 (its camera's): paths through instances and moving spheres in M_TOP,
    handed from the wavefront loop to the drain kernel."""
    render_through_the_top_layouts(pkg, orc, gpu, "yard")
