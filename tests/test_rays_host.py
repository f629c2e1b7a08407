"""Ray queries without a GPU (include/rt_hip.h, "ray queries"): the struct mirrors against a compiled probe of the header,
rt_ray_query_check's refusals, the source-id tables of the scene compiler as far as the host can see them, and — with the CPU checker
alone — that the ray sets the GPU test compares are decidable enough."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays as R  # noqa: E402


def test_ray_structs_match_the_header(pkg, tmp_path):
    A = pkg._abi
    body = ""
    for name in ("RtRay", "RtRayHit", "RtRayQueryOptions"):
        body += f'printf("{name} %zu\\n", sizeof({name}));'
        body += "".join(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in getattr(A, name)._fields_)
    body += 'printf("flags %u %u %u\\n", (unsigned)RT_RAYHIT_HIT, (unsigned)RT_RAYHIT_FRONT_FACE, (unsigned)RT_RAYHIT_INVALID_RAY);'
    src = tmp_path / "rq.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){' + body + "return 0;}")
    exe = tmp_path / "rq"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split(None, 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, size, dt in (("RtRay", 32, pkg.RAY_DTYPE), ("RtRayHit", 48, pkg.RAYHIT_DTYPE), ("RtRayQueryOptions", 16, None)):
        T = getattr(A, name)
        assert int(got[name]) == C.sizeof(T) == size, name
        for f, _ in T._fields_:
            assert int(got[f"{name}.{f}"]) == getattr(T, f).offset, (name, f)
            if dt is not None:
                assert dt.fields[f][1] == getattr(T, f).offset, (name, f)
        if dt is not None:
            assert dt.itemsize == size
    assert got["flags"].split() == [str(A.RT_RAYHIT_HIT), str(A.RT_RAYHIT_FRONT_FACE), str(A.RT_RAYHIT_INVALID_RAY)] == ["1", "2", "4"]
    assert A.RT_ABI_VERSION == 3 == pkg.lib().rt_abi_version()


def test_ray_query_check(pkg):
    A, lib = pkg._abi, pkg.lib()
    assert lib.rt_ray_query_check(None, 0) == A.RT_OK
    assert lib.rt_ray_query_check(None, (1 << 32) - 1) == A.RT_OK
    good = pkg.ray_query_options(flags=A.RT_FLAG_TIMING, pool_slots=4096)
    assert lib.rt_ray_query_check(C.byref(good), 1000) == A.RT_OK
    pkg.ray_query_check(good, 5)

    def opt(size=16, flags=0):
        return A.RtRayQueryOptions(size, flags, 0, 0)
    for o, n, word in ((opt(size=0), 1, b"struct_bytes"), (opt(size=8), 1, b"struct_bytes"), (opt(flags=1 << 9), 1, b"unknown"),
                       (opt(flags=A.RT_FLAG_COUNTERS), 1, b"unknown"), (opt(), 1 << 32, b"2^32"), (None, 1 << 40, b"2^32")):
        assert lib.rt_ray_query_check(C.byref(o) if o is not None else None, n) == A.RT_ERR_INVALID, word
        assert word in lib.rt_last_error(None), (word, lib.rt_last_error(None))
    with pytest.raises(pkg.RtError) as e:
        pkg.ray_query_check(opt(flags=64), 1)
    assert e.value.code == A.RT_ERR_INVALID
    # without a context nothing is traced, and nothing is touched
    assert lib.rt_trace_rays(None, None, None, None, 0, None, None) == A.RT_ERR_INVALID
    assert lib.rt_trace_rays_device(None, None, None, None, 0, None, None) == A.RT_ERR_INVALID


def test_scenes_cover_the_primitive_kinds(pkg):
    """What the GPU test relies on: the six scenes hold, between them, every primitive kind and wrapper, stay small enough for a checker
    that rebuilds its scene per ray, and none of them holds a medium (the refused scene does)."""
    A = pkg._abi
    kinds = set()
    for name in R.SCENES:
        b = R.build_scene(pkg, name)
        info = pkg.compile_info(b.desc)
        n = info["n_spheres"] + info["n_moving"] + info["n_rects"] + info["n_tris"]
        assert 0 < n <= 520 and info["n_media"] == 0, (name, info)
        kinds |= {b.desc.hittables[i].kind for i in range(b.desc.n_hittables)}
    assert {A.RT_HIT_SPHERE, A.RT_HIT_MOVING_SPHERE, A.RT_HIT_XY_RECT, A.RT_HIT_XZ_RECT, A.RT_HIT_YZ_RECT, A.RT_HIT_TRIANGLE, A.RT_HIT_BOX,
            A.RT_HIT_TRANSLATE, A.RT_HIT_ROTATE_Y, A.RT_HIT_FLIP_FACE, A.RT_HIT_BVH, A.RT_HIT_LIST} <= kinds
    assert pkg.compile_info(R.medium_scene(pkg).desc)["n_media"] == 1


@pytest.mark.parametrize("name", R.SCENES)
def test_ray_sets_are_decidable(pkg, orc, name):
    """At most 1 % of each set changes its answer under +-R ulps of its direction (rays.R_ULPS); every hit point lies on an object of the
    description; the sets hold a few thousand f32 rays, camera and secondary, hits and misses."""
    s = R.ray_set(pkg, orc, name)
    rays, ref, und = s["rays"], s["ref"], s["undecidable"]
    n = len(rays)
    n_cam = R.GRID[0] * R.GRID[1]
    print(f"{name}: {n} rays ({n_cam} camera), {int(ref['hit'].sum())} hits, {int(und.sum())} undecidable at R = {R.R_ULPS} ulps")
    assert 1500 <= n <= 6000 and n > n_cam
    assert rays.dtype == pkg.RAY_DTYPE and rays["o"].dtype == np.float32
    assert ref["hit"].sum() > n // 4 and (~ref["hit"]).sum() > 0
    assert und.mean() <= 0.01, f"{name}: {und.mean():.4f} of the rays are undecidable"
    hit = ref["hit"] & ~und
    assert s["on"][hit].any(axis=1).all(), f"{name}: a hit point lies on no object of the description"
    # spheres: hits within 1e-3 of a pole (u is ill-conditioned there) stay below 1 % of the set
    A = pkg._abi
    kind = np.array([s["built"].desc.hittables[int(i)].kind for i in s["ids"]])
    on_sphere = (s["on"] & (kind == A.RT_HIT_SPHERE)[None, :]).any(axis=1) & ref["hit"]
    polar = on_sphere & ((ref["v"] < 1e-3) | (ref["v"] > 1.0 - 1e-3))
    assert polar.mean() < 0.01
    if name == "moving":
        assert np.ptp(rays["time"]) > 0.5
    if name == "earth":
        assert np.ptp(ref["u"][on_sphere]) > 0.3 and np.ptp(ref["v"][on_sphere]) > 0.3


def test_import_logic_keeps_malformed_rays_and_overfull_queues_out(pkg):
    """A paper check of a COPY: k_rays_import's rules (csrc/kernels.hip) restated in numpy, made before any ray reached a persistent walk
    kernel. It does not run the library (tests/test_gpu_rays.py does: test_edges for the validity rule, test_pool_rule for the pool), so
    it shows that the rules as stated are sound, not that the kernel follows them: (a) its validity rule drops
    every ray with a non-finite component, the zero direction and directions whose |d|^2 leaves the normal f32 range; (b) with the pool
    rule of rt_trace_rays (P a multiple of 512 x 8, chunks of at most P rays, workgroup b of 512 rays feeding queue b mod 8) no queue can
    be handed more rays than queue_cap, whatever the list length or pool_slots."""
    f32 = np.float32

    def valid(o, time, d):
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            o, d, time = np.asarray(o, f32), np.asarray(d, f32), f32(time)
            a = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))
            fin = np.all(np.abs(o) < f32(np.inf)) and abs(time) < f32(np.inf) and np.all(np.abs(d) < f32(np.inf))
            return bool(fin and a >= f32(1.17549435e-38) and a < f32(np.inf))
    assert valid((0, 0, 0), 0.0, (0, 0, 1)) and valid((1e6, -3, 2), 0.5, (1e-3, 0, 0)) and valid((0, 0, 0), 0, (1e15, 1e15, 1e15))
    for o, t, d in (((np.nan, 0, 0), 0, (0, 0, 1)), ((0, np.inf, 0), 0, (0, 0, 1)), ((0, 0, 0), np.nan, (0, 0, 1)), ((0, 0, 0), -np.inf, (0, 0, 1)),
                    ((0, 0, 0), 0, (0, 0, 0)), ((0, 0, 0), 0, (-0.0, 0.0, -0.0)), ((0, 0, 0), 0, (np.nan, 1, 0)), ((0, 0, 0), 0, (1, -np.inf, 0)),
                    ((0, 0, 0), 0, (1e-30, 0, 0)), ((0, 0, 0), 0, (1e-40, 1e-40, 0)), ((0, 0, 0), 0, (3e19, 3e19, 0)), ((0, 0, 0), 0, (3.4e38, 0, 0))):
        assert not valid(o, t, d), (o, t, d)
    Q, GRAIN = 8, 512 * 8
    for n_rays in (1, 63, 512, 513, 4096, 4097, 10752, 960000, (1 << 28) + 5, (1 << 32) - 1):
        for pool_slots in (0, 1, 511, 4096, 5000, 1 << 20):
            P = min(pool_slots if pool_slots else 1 << 28, n_rays)
            P = max(GRAIN, min(-(-P // GRAIN) * GRAIN, 0xFFFFF000))
            cap = P // Q
            assert cap % 512 == 0 and P % GRAIN == 0
            for n in {min(P, n_rays), n_rays % P or min(P, n_rays)}:              # a full chunk and the last one
                blocks = -(-n // 512)
                per_queue = [len(range(q, blocks, Q)) * 512 for q in range(Q)]    # every workgroup stores at most 512 rays
                assert max(per_queue) <= cap, (n_rays, pool_slots, n, per_queue, cap)


# ---- the batch entry of the checker, and the ray set of a scene that does not fit LDS (tests/test_gpu_rays_hbm.py) ----------------------
@pytest.mark.parametrize("name", ["mesh", "moving"])
def test_batch_world_hit_equals_the_per_ray_entry(pkg, orc, name):
    """orc_world_hit_many at precision 64 is orc_world_hit's code path with the scene built once: the same bits for every ray, hits and
    misses, with the limit as a scalar and per ray; and a limit below the hit turns it into a miss in both."""
    s = R.ray_set(pkg, orc, name)
    rays, desc = s["rays"], s["built"].desc
    batch, single = R.ask(orc, desc, rays), R.ask_per_ray(orc, desc, rays)
    assert batch["hit"].any() and (~batch["hit"]).any()
    for k in single:
        assert batch[k].dtype == single[k].dtype and batch[k].tobytes() == single[k].tobytes(), k
    o, d, tm = rays["o"].astype(np.float64), rays["d"].astype(np.float64), rays["time"].astype(np.float64)
    limit = np.where(batch["hit"], batch["t"] * np.where(np.arange(len(rays)) & 1, 0.5, 1.5), 1.0)
    hit, rec = orc.world_hit_many(desc, o, d, tm, 0.001, limit)
    for i in range(0, len(rays), 7):
        one = orc.world_hit(desc, o[i], d[i], tm[i], 0.001, limit[i])
        assert (one is not None) == bool(hit[i]), i
        if one is not None:
            assert (one["t"],) + one["p"] + one["normal"] + (one["u"], one["v"], float(one["front_face"])) == tuple(rec[i]), i
    assert (hit[batch["hit"]] == ((np.arange(len(rays)) & 1) == 0)[batch["hit"]]).all()
    # precision 32 is the checker's f32 instance: every number it reports is an f32, and it is not the f64 answer rounded
    h32, r32 = orc.world_hit_many(desc, o, d, tm, precision=32)
    both = h32 & batch["hit"]
    assert both.sum() > len(rays) // 4 and (r32 == r32.astype(np.float32)).all()
    assert (r32[both, 0] != batch["t"][both].astype(np.float32)).any()
    with pytest.raises(RuntimeError):
        orc.world_hit_many(desc, o, d, tm, precision=16)


def field_configs(pkg, scene="field"):
    A = pkg._abi
    return [(case, name, flags, more) for case, (name, flags, more) in R.field_matrix(A, scene).items()]


def test_field_does_not_fit_lds(pkg):
    """What tests/test_gpu_rays_hbm.py relies on, for both builders and every upload of its matrix: the scene does not fit LDS, and it
    compiles to more records than the default LDS top holds (1024: the top is partial, M_TOP) and at most the 4096 a top can hold
    (lds_top_records = 4096 keeps no top: M_HBM). The one exception is named: leaf_collapse = 4 folds the tree below the LDS budget."""
    A = pkg._abi
    built = {name: R.build_scene(pkg, name) for name in R.HBM_OF["field"]}
    for case, scene, flags, more in field_configs(pkg):
        info = pkg.compile_info(built[scene].desc, flags & ~A.RT_LAYOUT_SCENE_IN_HBM, **more)
        print(f"{case}: {info['n_nodes']} records, fits_lds = {info['fits_lds']}, n_first = {info['n_first']}")
        if case in R.FITS_LDS or case == "collapse_4_hbm":
            assert info["fits_lds"] == 1 and info["n_nodes"] > 1024, (case, info)
            continue
        assert info["fits_lds"] == 0 and 1024 < info["n_nodes"] <= 4096, (case, info)
        assert info["n_media"] == 0 and info["n_moving"] == 0 and info["n_spheres"] == R.FIELD_SPHERES and info["n_tris"] == 2 * R.FIELD_GRID ** 2
        # the ground rect is tested when a walk begins (the first_leaf twin) unless the lists are the reference's or the walk is 8-wide
        assert info["n_first"] == (0 if flags & (A.RT_LAYOUT_LISTS_AS_REFERENCE | A.RT_LAYOUT_WIDE_NODES) else 1), (case, info)
    # members without boxes make a smaller tree, which fits: that layout is the existing ray tests' (tests/test_gpu_rays.py)
    for scene in R.HBM_OF["field"]:
        assert pkg.compile_info(built[scene].desc, A.RT_LAYOUT_REFERENCE_COUNTERS)["fits_lds"] == 1
        assert pkg.wide_layout_check(built[scene].desc)["depth"] >= 3


def test_field_top_layouts(pkg):
    """The top layouts the GPU test uploads, built and verified on the host (rt_scene_top_layout_check: one address space over both
    memories, every skip link landing where the plain array's does): the number of top records is the depth-cut rule restated in
    rays.top_rule, > 0 for tops of 7, 100 and 1024 records and 0 for 4096 (the whole tree fits: M_HBM)."""
    L = pkg.lib()
    for name in R.HBM_OF["field"]:
        desc = R.build_scene(pkg, name).desc
        skip = pkg.compile_dump(desc, pkg._abi.RT_LAYOUT_NODES_32B)[0]["skip"]
        for max_top in (1, 2, 3, 7, 100, 1024, 4096):
            n = C.c_uint64(0)
            assert L.rt_scene_top_layout_check(C.byref(desc), max_top, C.byref(n)) == pkg._abi.RT_OK, L.rt_last_error(None)
            assert n.value == R.top_rule(skip, max_top) <= max_top, (name, max_top, n.value)
            assert (n.value > 0) == (max_top in (7, 100, 1024)) or max_top in (1, 2, 3), (name, max_top, n.value)
            print(f"{name}: top of at most {max_top} records holds {n.value}")


def test_field_ray_set(pkg, orc):
    """The field set is decidable enough (rays.py's cap of 1 %), spread over every direction octant — the compressed layout keeps one
    record array per octant — and over every primitive kind of the scene; every hit lies on exactly one primitive (no two surfaces
    meet), and field_sah shares the rays and the answers."""
    A = pkg._abi
    s = R.ray_set(pkg, orc, "field")
    rays, ref, und = s["rays"], s["ref"], s["undecidable"]
    print(f"field: {len(rays)} rays, {int(ref['hit'].sum())} hits, {int(und.sum())} undecidable at R = {R.R_ULPS} ulps")
    assert 2000 <= len(rays) <= 4000 and rays.dtype == pkg.RAY_DTYPE
    assert und.mean() <= 0.01, f"{und.mean():.4f} of the rays are undecidable"
    dec = ~und
    d = rays["d"]
    octant = (d[:, 0] < 0) * 1 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 4
    per_octant = np.bincount(octant[dec], minlength=8)
    print("decidable rays per direction octant:", per_octant.tolist())
    assert per_octant.min() >= 50
    hit = ref["hit"] & dec
    assert (s["on"][hit].sum(axis=1) == 1).all(), "a hit point lies on no primitive, or on two"
    kind = np.array([s["built"].desc.hittables[int(i)].kind for i in s["ids"]])
    for k in (A.RT_HIT_SPHERE, A.RT_HIT_TRIANGLE, A.RT_HIT_BOX, A.RT_HIT_XZ_RECT):
        n = int((s["on"][:, kind == k].any(axis=1) & hit).sum())
        print(f"hits on primitives of kind {k}: {n}")
        assert n >= 20, k
    assert (~ref["hit"] & dec).sum() >= 100
    t = R.ray_set(pkg, orc, "field_sah")
    assert t["rays"] is rays and t["ref"] is ref and t["built"].desc.bvh_builder == A.RT_BVH_SAH and s["built"].desc.bvh_builder == A.RT_BVH_REFERENCE


def test_field_f32_checker_figures(pkg, orc):
    """rays.MEASURED_F32_CHECKER["field"], which bounds the device (x 2), is what the checker's f32 instance measures against its f64
    answers here — within 1 % (libm builds differ in the last place) — and the two instances agree on hit / miss and front_face for every
    decidable ray."""
    worst, at, a = R.f32_checker_figures(pkg, orc, "field")
    s = R.ray_set(pkg, orc, "field")
    dec = ~s["undecidable"]
    print("f32 checker against f64 checker:", {k: f"{v:.3e} (ray {at[k]})" for k, v in worst.items()})
    assert not (dec & (a["hit"] != s["ref"]["hit"])).any() and not (dec & a["hit"] & (a["ff"] != s["ref"]["ff"])).any()
    for k, v in R.MEASURED_F32_CHECKER["field"].items():
        assert abs(worst[k] - v) <= 0.01 * v, (k, worst[k], v)


# ---- `yard`: the second scene that does not fit LDS — a BVH over a time range with instances and moving spheres -------------------------
YARD_TOPS = (1, 2, 3, 7, 100, 1024, 4096, R.YARD_TOP)


def test_yard_does_not_fit_lds(pkg):
    """test_field_does_not_fit_lds for `yard`, both builders and every upload of its matrix: it does not fit LDS and compiles to more
    records than the default top holds and at most 4096 (leaf_collapse = 4 is the named exception); it holds at least 500 moving spheres
    and 84 transforms (80 wrapped Boxes with an angle each, A, the three-wrapper chain of B as one, C; D adds two) and no medium;
    and the 8-wide layout refuses it, so a WIDE_NODES upload keeps the binary walk."""
    A = pkg._abi
    built = {name: R.build_scene(pkg, name) for name in R.HBM_OF["yard"]}
    for case, scene, flags, more in field_configs(pkg, "yard"):
        info = pkg.compile_info(built[scene].desc, flags & ~A.RT_LAYOUT_SCENE_IN_HBM, **more)
        print(f"{case}: {info['n_nodes']} records, fits_lds = {info['fits_lds']}, {info['n_moving']} moving spheres, {info['n_xforms']} transforms")
        assert info["n_moving"] >= 500 and info["n_xforms"] >= 84 and info["n_media"] == 0, (case, info)
        if case in R.FITS_LDS or case == "collapse_4_hbm":
            assert info["fits_lds"] == 1 and info["n_nodes"] > 1024, (case, info)
            continue
        assert info["fits_lds"] == 0 and 1024 < info["n_nodes"] <= 4096, (case, info)
    for scene in R.HBM_OF["yard"]:
        with pytest.raises(pkg.RtError) as e:
            pkg.wide_layout_check(built[scene].desc)
        assert "not a static BVH" in str(e.value), str(e.value)
    # 80 distinct transforms on the Boxes: no two share an angle
    d = built["yard"].desc
    angles = [d.hittables[i].p[0] for i in range(d.n_hittables) if d.hittables[i].kind == A.RT_HIT_ROTATE_Y]
    assert len(set(angles)) >= R.YARD_BOXES + 4


def test_yard_top_layouts(pkg):
    """test_field_top_layouts for `yard`, with one more top (rays.YARD_TOP). The two LT_XFORM records of a wrapper are siblings in the
    threaded array — enter, the wrapped subtree, exit, under the same enclosing records — so the depth cut never parts them (asserted
    for every top); what a top does part is the pair from records of the subtree between them: the walk reads `enter` from LDS, changes the ray's
    space, walks the instance's lower records in HBM and comes back to LDS for `exit`. That holds for A, B and C with YARD_TOP under the
    reference's builder (its balanced tree keeps them below every smaller top) and with the default top under SAH."""
    L, A = pkg.lib(), pkg._abi
    across = {}
    for name in R.HBM_OF["yard"]:
        desc = R.build_scene(pkg, name).desc
        nodes = pkg.compile_dump(desc, A.RT_LAYOUT_NODES_32B)[0]
        pairs = R.xform_pairs(nodes["leaf"])
        assert len(pairs) >= 84
        for max_top in YARD_TOPS:
            n = C.c_uint64(0)
            assert L.rt_scene_top_layout_check(C.byref(desc), max_top, C.byref(n)) == A.RT_OK, L.rt_last_error(None)
            top = R.top_mask(nodes["skip"], max_top)
            assert n.value == R.top_rule(nodes["skip"], max_top) == top.sum() <= max_top, (name, max_top, n.value)
            assert (n.value > 0) == (max_top not in (1, 4096)), (name, max_top, n.value)
            assert all(top[a] == top[e] for a, e in pairs), "an enter record and its exit on two sides of the cut"
            across[name, max_top] = [(a, e) for a, e in pairs if top[a] and e - a > 100 and not top[a + 1:e].all()]
            print(f"{name}: top of at most {max_top} records holds {n.value}; instances entered in LDS and walked in HBM: {across[name, max_top]}")
    assert len(across["yard", R.YARD_TOP]) == 3 and len(across["yard_sah", 1024]) == 3


def yard_conditions(pkg, s, label, tie=None):
    """The conditions of a set of `yard`, whichever family: at most 1 % undecidable, at least 50 decidable rays in every direction
    octant (by the sign bits), every decidable hit on exactly one primitive (but the rays `tie`), at least 100 decidable misses, times
    spread over the shutter. Returns the decidable hits per class of rays.yard_hit_classes."""
    rays, ref, und = s["rays"], s["ref"], s["undecidable"]
    dec = ~und
    print(f"{label}: {len(rays)} rays, {int(ref['hit'].sum())} hits, {int(und.sum())} undecidable (R = {R.R_ULPS} ulps on d, O = {R.O_ULPS} on o)")
    assert rays.dtype == pkg.RAY_DTYPE and und.mean() <= 0.01, f"{und.mean():.4f} of the rays are undecidable"
    sign = np.signbit(rays["d"])
    per_octant = np.bincount((sign[:, 0] * 1 + sign[:, 1] * 2 + sign[:, 2] * 4)[dec], minlength=8)
    print(f"{label}: decidable rays per direction octant: {per_octant.tolist()}")
    assert per_octant.min() >= 50
    hit = ref["hit"] & dec
    single = hit if tie is None else hit & ~tie
    assert (s["on"][single].sum(axis=1) == 1).all(), "a hit point lies on no primitive, or on two"
    assert (~ref["hit"] & dec).sum() >= 100 and np.ptp(rays["time"]) > 0.5
    count = {name: int((m & hit).sum()) for name, m in R.yard_hit_classes(pkg, s).items()}
    print(f"{label}: decidable hits per class: {count}")
    return count


def test_yard_ray_set(pkg, orc):
    """test_field_ray_set for `yard`: the conditions of yard_conditions, and at least 20 decidable hits on every class the scene was
    built for — bare spheres, bare moving spheres, wrapped Boxes, xy and yz rects, rects under FlipFace, spheres in A, triangles in B,
    spheres and moving spheres in C, primitives in D; yard_sah shares the rays and the answers."""
    A = pkg._abi
    s = R.ray_set(pkg, orc, "yard")
    assert 2000 <= len(s["rays"]) <= 4000
    count = yard_conditions(pkg, s, "yard")
    assert len(count) == 11 and min(count.values()) >= 20, count
    t = R.ray_set(pkg, orc, "yard_sah")
    assert t["rays"] is s["rays"] and t["ref"] is s["ref"] and t["built"].desc.bvh_builder == A.RT_BVH_SAH and s["built"].desc.bvh_builder == A.RT_BVH_REFERENCE


@pytest.mark.parametrize("family", ["axis", "segments"])
def test_yard_new_sets(pkg, orc, family):
    """yard_conditions for the axis set and the segment set of `yard` (test_axis_sets and test_segment_sets hold them to what every such
    set is held to). Axis: at least 200 of the seeded origins lie inside the footprints of A, B and D, where a world axis ray becomes
    a local ray with components the transform made; a hit point on two primitives is a shared edge of B's mesh, a named edge ray. Hits per class: the 20 of
    test_yard_ray_set hold here for the classes that fill a volume; the thin ones (rects of one axis, the 12 + 12 objects of D, the
    50 moving spheres of C) are held to presence only — the ray set reaches them with aimed rays, which neither family can have: an
    axis ray's direction is drawn from the axes (and misses every rect it runs parallel to), and a segment's source is drawn from the
    ray set's hits in their proportion."""
    s = R.new_set(pkg, orc, family, "yard")
    count = yard_conditions(pkg, s, f"{family}/yard", tie=s.get("edge"))
    assert sum(v > 0 for v in count.values()) == 11
    assert min(count[k] for k in ("bare spheres", "bare moving spheres", "wrapped Boxes", "spheres in A", "triangles in B", "spheres in C")) >= 20, count
    if family == "axis":
        o = s["rays"]["o"][:R.AXIS_RAYS]
        inside = np.zeros(len(o), bool)
        for x0, x1, z0, z1 in (R.YARD_BLOCKS[k] for k in "ABD"):
            inside |= (o[:, 0] > x0) & (o[:, 0] < x1) & (o[:, 2] > z0) & (o[:, 2] < z1)
        print(f"axis/yard: {int(inside.sum())} seeded origins inside the footprints of A, B and D; {int(s['edge'].sum())} edge rays")
        assert inside.sum() >= 200 and s["rim"].sum() == 48 and s["edge"].sum() <= 8


def test_yard_f32_checker_figures(pkg, orc):
    """test_field_f32_checker_figures for `yard`."""
    worst, at, a = R.f32_checker_figures(pkg, orc, "yard")
    s = R.ray_set(pkg, orc, "yard")
    dec = ~s["undecidable"]
    print("f32 checker against f64 checker:", {k: f"{v:.3e} (ray {at[k]})" for k, v in worst.items()})
    assert not (dec & (a["hit"] != s["ref"]["hit"])).any() and not (dec & a["hit"] & (a["ff"] != s["ref"]["ff"])).any()
    for k, v in R.MEASURED_F32_CHECKER["yard"].items():
        assert abs(worst[k] - v) <= 0.01 * v, (k, worst[k], v)


@pytest.mark.parametrize("family", ["rays", "axis", "segments"])
def test_the_origin_rule(pkg, orc, family):
    """rays.origin_undecidable moves the origin by +-O ulps of the coarsest instance frame and counts a changed answer on that frame's
    primitives. Every set made before it keeps the bits of its mask (no frame of theirs is coarse enough to change an answer: the
    Cornell box's reach 4 x the world's ulp); on `yard` it finds rays of every family but the axis set's — most of them leave a surface of
    instance C, 400 units out in its own frame, within a few degrees of the tangent — among them the one ray of the ray set, decidable
    by the rule on d, on which the checker's f32 instance finds the sphere it stands on again; with both rules the f32 instance gives
    the f64 instance's answer on every decidable ray."""
    make = {"rays": R.ray_set, "axis": R.axis_set, "segments": R.segment_set}[family]
    names = {"rays": R.SCENES + ["field"], "axis": R.AXIS_SCENES[:-1], "segments": R.SEGMENT_SCENES[:-1]}[family]
    rule = R.segment_undecidable if family == "segments" else R.undecidable
    for name in names + ["yard"]:
        s = make(pkg, orc, name)
        desc = s["built"].desc
        none = np.zeros(len(s["rays"]), bool)
        old = rule(orc, desc, s["rays"], s["ref"]) & ~(s.get("rim", none) | s.get("edge", none))
        more = int((s["undecidable"] & ~old).sum())
        print(f"{family}/{name}: {int(old.sum())} undecidable by the rule on d, {more} more by the rule on o")
        assert not (old & ~s["undecidable"]).any()
        if name != "yard":
            assert old.tobytes() == s["undecidable"].tobytes(), name
            continue
        assert more > 0 or family == "axis"
        if family == "rays":
            a = R.ask(orc, desc, s["rays"], precision=32)
            assert (R.changed(a, s["ref"]) & ~old & s["ref"]["hit"] & a["hit"]).sum() >= 1 and not (R.changed(a, s["ref"]) & ~s["undecidable"]).any()


# ---- axis rays and segments (rays.axis_set, rays.segment_set): what tests/test_gpu_rays.py, _hbm.py and _occlusion.py rely on ------------
@pytest.mark.parametrize("name", R.SCENES + ["field"])
def test_the_extended_rule_keeps_the_existing_masks(pkg, orc, name):
    """rays.undecidable moves a direction component below 1e-20 by R ulps of the ray's largest component. Each existing set's mask is
    the same bits with and without the extension (a few camera rays hold such a component: those of a camera that looks along an axis)."""
    s = R.ray_set(pkg, orc, name)
    print(f"{name}: {int(R.zero_class(s['rays']['d']).any(axis=1).sum())} rays with a zero-class direction component")
    old = R.undecidable(orc, s["built"].desc, s["rays"], s["ref"], small=0.0)
    assert old.dtype == s["undecidable"].dtype and old.tobytes() == s["undecidable"].tobytes()


@pytest.mark.parametrize("name", R.AXIS_SCENES)
def test_axis_sets(pkg, orc, name):
    """About 2000 seeded rays per scene, half with two zero-class direction components and half with one, every zero-class value and
    every axis among them, about half of the origins on the 1/4 lattice; at most 1 % undecidable under the extended rule; no ray whose
    checker t is NaN (an origin in a rect's plane with d parallel to it: the reference's own 0 / 0); and the two named subsets: rim rays
    hit a rect, edge rays hit a triangle, in the f64 checker and in its f32 instance alike."""
    A = pkg._abi
    s = R.axis_set(pkg, orc, name)
    rays, ref, und, rim, edge = s["rays"], s["ref"], s["undecidable"], s["rim"], s["edge"]
    d = rays["d"]
    zc = R.zero_class(d)
    n_zero = zc.sum(axis=1)
    print(f"axis/{name}: {len(rays)} rays, {int(ref['hit'].sum())} hits, {int(und.sum())} undecidable at R = {R.R_ULPS} ulps (extended rule), "
          f"{int(rim.sum())} rim, {int(edge.sum())} edge, {int(s['snapped'].sum())} origins on the 1/4 lattice")
    assert R.AXIS_RAYS <= len(rays) <= R.AXIS_RAYS + 200 and rays.dtype == pkg.RAY_DTYPE
    assert und.mean() <= 0.01, f"{name}: {und.mean():.4f} of the axis rays are undecidable"
    assert not (und & (rim | edge)).any() and (s["decidable"] == ~und).all()
    assert not np.isnan(ref["t"]).any() and not np.isnan(ref["p"]).any()
    assert ref["hit"].sum() > len(rays) // 8 and (~ref["hit"]).sum() > len(rays) // 8
    assert set(np.unique(n_zero)) == {1, 2} and 0.4 < (n_zero == 2).mean() < 0.6
    bits = d.view(np.uint32)[zc]
    assert set(np.unique(bits)) == set(R.ZERO_CLASS.view(np.uint32).tolist()), "every zero-class value occurs: +-0, +-1e-40, +-1e-30"
    for axis in range(3):
        pure = (n_zero == 2) & ~zc[:, axis]
        assert (pure & (d[:, axis] > 0)).sum() >= 50 and (pure & (d[:, axis] < 0)).sum() >= 50, axis
    mag = np.abs(d[~zc & (n_zero == 2)[:, None]])
    assert mag.min() == 0.125 and mag.max() == 8.0
    assert 0.4 < s["snapped"][:R.AXIS_RAYS].mean() < 0.6
    assert (rays["o"][s["snapped"]] * 4 == np.round(rays["o"][s["snapped"]] * 4)).all()
    if name in R.TIMED_SCENES:
        assert np.ptp(rays["time"]) > 0.5
    hit = ref["hit"] & ~und
    assert s["on"][hit].any(axis=1).all(), f"{name}: a hit point lies on no object of the description"
    kind = np.array([s["built"].desc.hittables[int(i)].kind for i in s["ids"]])
    f32 = R.ask(orc, s["built"].desc, rays, precision=32)
    assert rim.any() == (name in R.RIM_SCENES) and rim.sum() <= 64 and edge[R.AXIS_RAYS:].any() == (name in R.EDGE_SCENES)
    if rim.any():
        rect = np.isin(kind, (A.RT_HIT_XY_RECT, A.RT_HIT_XZ_RECT, A.RT_HIT_YZ_RECT))
        assert (n_zero[rim] == 2).all() and (d[rim][zc[rim]] == 0.0).all()
        assert ref["hit"][rim].all() and f32["hit"][rim].all() and s["on"][rim][:, rect].any(axis=1).all()
    if edge.any():
        tri = kind == A.RT_HIT_TRIANGLE
        assert ref["hit"][edge].all() and s["on"][edge][:, tri].any(axis=1).all(), "an edge ray that does not hit a triangle"
        assert f32["hit"][edge].all() and (np.abs(f32["t"][edge] - ref["t"][edge]) <= 1e-3).all(), "the f32 instance leaks through an edge"
        assert name != "mesh" or (s["on"][edge][:, tri].sum(axis=1) >= 2).sum() >= 20      # (field: the border, which one triangle owns)
    if name == "mesh":
        i = R.AXIS_RAYS + int(rim.sum())
        assert edge[i] and tuple(rays["o"][i]) == R.EDGE_RAY[0] and tuple(rays["d"][i]) == tuple(np.float32(R.EDGE_RAY[1]))
        assert abs(ref["t"][i] - 0.2451517) < 1e-6


@pytest.mark.parametrize("name", R.SEGMENT_SCENES)
def test_segment_sets(pkg, orc, name):
    """About 2000 segments d = q - p per scene with |d| >= 0.5, half of them ending on a surface (t_max = 0.98) and half at a free point
    (1.5); at most 5 % undecidable (R ulps on d, t_min halved and doubled, t_max -+ 1e-3); blocked and unblocked each more than a quarter."""
    s = R.segment_set(pkg, orc, name)
    rays, ref, und = s["rays"], s["ref"], s["undecidable"]
    length = np.linalg.norm(rays["d"].astype(np.float64), axis=1)
    print(f"segments/{name}: {len(rays)} segments, |d| {length.min():.2f} .. {length.max():.1f}, {int(ref['hit'].sum())} blocked, "
          f"{int(und.sum())} undecidable ({und.mean():.4f})")
    assert 0.9 * R.SEGMENTS <= len(rays) <= R.SEGMENTS and rays.dtype == pkg.RAY_DTYPE and length.min() >= R.SEGMENT_MIN
    assert und.mean() <= R.SEGMENT_CAPS.get(name, R.SEGMENT_CAP), f"{name}: {und.mean():.4f} of the segments are undecidable"
    assert set(np.unique(rays["t_max"])) == {np.float32(R.T_SURFACE), np.float32(R.T_FREE)}
    assert (rays["t_max"] == np.float32(R.T_SURFACE)).tolist() == s["on_surface"].tolist() and 0.45 < s["on_surface"].mean() < 0.55
    assert ref["hit"].mean() > 0.25 and (~ref["hit"]).mean() > 0.25
    assert (ref["t"][ref["hit"]] <= R.T_FREE).all() and not np.isnan(ref["t"]).any()
    hit = ref["hit"] & ~und
    assert s["on"][hit].any(axis=1).all(), f"{name}: a hit point lies on no object of the description"
    if name in R.SEGMENT_REACH:
        o = rays["o"].astype(np.float64)
        assert np.linalg.norm(o, axis=1).max() <= R.SEGMENT_REACH[name] + 1e-3
        assert np.linalg.norm((o + rays["d"])[s["on_surface"]], axis=1).max() <= R.SEGMENT_REACH[name] + 1e-3
    if name in R.SEGMENT_NEAR:               # surface targets lie near, but every SEGMENT_LONG-th, which lies where the seed put it
        far = int((length[s["on_surface"]] > R.SEGMENT_NEAR[name] + 1e-3).sum())
        print(f"segments/{name}: {far} segments longer than {R.SEGMENT_NEAR[name]} end on a surface, the longest {length[s['on_surface']].max():.1f}")
        assert 50 <= far <= R.SEGMENTS // (2 * R.SEGMENT_LONG) and length[s["on_surface"]].max() > 3 * R.SEGMENT_NEAR[name]
    if name in R.TIMED_SCENES:
        assert np.ptp(rays["time"]) > 0.5


def test_segment_lengths_span_two_decades(pkg, orc):
    length = np.concatenate([np.linalg.norm(R.segment_set(pkg, orc, n)["rays"]["d"].astype(np.float64), axis=1) for n in R.SEGMENT_SCENES])
    print(f"|d| over the segment sets: {length.min():.2f} .. {length.max():.1f}")
    assert length.max() >= 100.0 * length.min()


@pytest.mark.parametrize("key", [f"axis/{n}" for n in R.AXIS_SCENES] + [f"segments/{n}" for n in R.SEGMENT_SCENES])
def test_new_sets_f32_checker_figures(pkg, orc, key):
    """rays.MEASURED_F32_CHECKER[key], which bounds the device (x 2), is what the checker's f32 instance measures against its f64 answers
    here, within 1 % (libm builds differ in the last place). Reported, not asserted — the judge of the device is the f64 checker alone —
    is on how many decidable rays the f32 instance gives another answer; but they are few, so that the figures speak for the set."""
    family, name = key.split("/")
    worst, at, a, differs, other = R.f32_figures(pkg, orc, family, name)
    s = R.new_set(pkg, orc, family, name)
    print(f"{key}: f32 checker against f64 checker:", {k: f"{v:.3e} (ray {at[k]})" for k, v in worst.items()})
    print(f"{key}: on {len(differs)} decidable rays the f32 checker's hit / miss is not the f64 checker's; on {len(other)} both hit, elsewhere")
    assert len(differs) + len(other) <= 0.02 * len(s["rays"])
    assert set(R.MEASURED_F32_CHECKER[key]) == set(worst)
    for k, v in R.MEASURED_F32_CHECKER[key].items():
        assert abs(worst[k] - v) <= 0.01 * v, (k, worst[k], v)
