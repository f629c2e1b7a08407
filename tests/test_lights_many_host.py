"""RT_SCENE_LIGHTS_MANY without a GPU (include/rt_hip.h): the flag's rules, the light tree's invariants from rt_scene_light_tree_dump, the weight
rule restated in numpy, and light_reference in f64 with the flag set (the estimator stays unbiased, the pick follows the areas)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lights_cases as LC  # noqa: E402
import lights_many_cases as LM  # noqa: E402


# ---- the flag ---------------------------------------------------------------------------------------------------------------------------------------
def test_flag_rules(pkg):
    A = pkg._abi
    assert A.RT_SCENE_LIGHTS_MANY == 4 and A.RT_FEATURE_LIGHTS_TREE == 512 and A.RT_LIGHTQ_LINEAR == 2
    desc, keep, _ = LM.query_case(pkg, "two")
    assert desc.scene_flags == 5
    info = pkg.compile_info(desc)
    assert info["n_lights"] == 2 and info["features"] & 512 and info["features"] & A.RT_FEATURE_LIGHTS_EXT and info["features"] & 64
    desc.scene_flags = 4                                               # the flag alone
    with pytest.raises(pkg.RtError) as e:
        pkg.compile_info(desc)
    assert e.value.code == A.RT_ERR_INVALID and "needs RT_SCENE_LIGHTS_ALL_SHAPES" in str(e.value)
    for bad in (2, 3, 6, 7):
        desc.scene_flags = bad
        with pytest.raises(pkg.RtError) as e:
            pkg.compile_info(desc)
        assert e.value.code == A.RT_ERR_INVALID and "scene_flags" in str(e.value) and "unknown bit" in str(e.value), bad
    for flags in (0, 1):
        desc.scene_flags = flags
        assert pkg.compile_info(desc)["features"] & 512 == 0
        with pytest.raises(pkg.RtError) as e:                          # no tree to dump
            pkg.light_tree(desc)
        assert e.value.code == A.RT_ERR_INVALID
    import ctypes as C
    assert C.sizeof(A.RtSceneDesc) == 152


def test_a_list_of_the_references_own_kinds_takes_the_extended_records_too(pkg):
    b = pkg.SceneBuilder()
    lamp, grey = b.diffuse_light((4, 4, 4)), b.lambertian((0.7, 0.7, 0.7))
    lights = [b.xz_rect(-1, 1, -1, 1, 3, lamp), b.sphere((0, 2, 0), 0.5, lamp)]
    world = b.hittable_list([b.xz_rect(-5, 5, -5, 5, 0, grey)] + lights)
    on = b.desc(world, b.hittable_list(lights), lights_all_shapes=True, lights_many=True)
    assert pkg.compile_info(on)["features"] & (256 | 512) == 256 | 512
    off = b.desc(world, b.hittable_list(lights), lights_all_shapes=True)
    assert pkg.compile_info(off)["features"] & (256 | 512) == 0


def test_refusals_of_all_shapes_apply_unchanged(pkg):
    A = pkg._abi
    b = pkg.SceneBuilder()
    lamp, grey = b.diffuse_light((4, 4, 4)), b.lambertian((0.7, 0.7, 0.7))
    floor = b.hittable_list([b.xz_rect(-5, 5, -5, 5, 0, grey)])
    for member, word in ((b.triangle((0, 3, 0), (1, 3, 0), (2, 3, 0), lamp), "zero area"), (b.moving_sphere((0, 3, 0), (0, 3.5, 0), 0.0, 1.0, 0.5, lamp), "moving sphere"),
                         (b.hittable_list([b.sphere((0, 3, 0), 0.5, lamp)]), "nested list")):
        good = b.triangle((0, 3, 0), (1, 3, 0), (0, 3, 1), lamp)
        desc = b.desc(floor, b.hittable_list([good, member]), lights_all_shapes=True, lights_many=True)
        with pytest.raises(pkg.RtError) as e:
            pkg.compile_info(desc)
        assert e.value.code == A.RT_ERR_INVALID and word in str(e.value) and "member 1" in str(e.value)


def test_json_key(pkg):
    import json
    doc = LC.cornell_doc(True)
    doc["lights_many"] = True
    js = pkg.JsonScene(doc)
    assert js.desc.scene_flags == 5 and pkg.compile_info(js.desc)["features"] & 512
    assert pkg.JsonScene(LC.cornell_doc(True)).desc.scene_flags == 1
    with pytest.raises(ValueError):
        pkg.JsonScene(dict(doc, lights_many=1))
    json.dumps(doc)


# ---- the tree ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LM.CASES)
def test_tree_invariants(pkg, name):
    desc, keep, _ = LM.query_case(pkg, name)
    t = pkg.light_tree(desc)
    nodes, slot_member = t["nodes"], t["slot_member"]
    n = len(slot_member)
    assert n == pkg.compile_info(desc)["n_lights"] and len(nodes) == 2 * n - 1
    mn, mx = LM.node_boxes(nodes)
    assert (mn <= mx).all() and np.isfinite(mn).all() and np.isfinite(mx).all()
    # skip links in range; every member in exactly one leaf, the leaves' slots counting up from the left
    idx = np.arange(len(nodes))
    assert (nodes["skip"] > idx).all() and (nodes["skip"] <= len(nodes)).all()
    leaves = nodes["leaf"][nodes["leaf"] != 0]
    assert np.array_equal(leaves, np.arange(1, n + 1)) and sorted(slot_member.tolist()) == list(range(n))
    assert (nodes["skip"][nodes["leaf"] != 0] == idx[nodes["leaf"] != 0] + 1).all()
    # pre-order: an inner record's children are the next record and the record at that one's skip link, and together they end where it ends;
    # the subtrees nest (a walk that passes every box visits every record once, in order)
    seen = 0

    def walk(i):
        nonlocal seen
        assert i == seen
        seen += 1
        if nodes["leaf"][i] != 0:
            return 1
        a, b = i + 1, int(nodes["skip"][i + 1])
        assert b < nodes["skip"][i] and nodes["skip"][b] == nodes["skip"][i]
        for c in (a, b):                                              # a parent's box holds its children's
            assert (mn[i] <= mn[c]).all() and (mx[i] >= mx[c]).all(), (i, c)
        la, lb = walk(a), walk(b)
        assert la - lb in (0, 1)                                       # the median split
        return la + lb
    assert walk(0) == n and seen == len(nodes)
    # a leaf's box holds its member's world-space vertices (triangles; every member of the first five cases)
    verts = LM.world_vertices(pkg, desc)
    leaf_of = {int(slot_member[int(nodes["leaf"][i]) - 1]): i for i in idx if nodes["leaf"][i] != 0}
    n_checked = 0
    for k, v in enumerate(verts):
        if v is None:
            continue
        i = leaf_of[k]
        assert (v >= mn[i]).all() and (v <= mx[i]).all(), (k, v, mn[i], mx[i])
        n_checked += 1
    assert n_checked == (n if name != "mixed" else 11)


def test_mixed_boxes_hold_the_other_shapes(pkg):
    desc, keep, _ = LM.query_case(pkg, "mixed")
    t = pkg.light_tree(desc)
    mn, mx = LM.node_boxes(t["nodes"])
    leaf_of = {int(t["slot_member"][int(l) - 1]): i for i, l in enumerate(t["nodes"]["leaf"]) if l != 0}
    expect = {0: ((-1.0, 2.0, 3.0), (1.0, 3.0, 3.0)), 1: ((2.9, 2.0, -0.5), (2.9, 3.2, 0.5)), 2: ((1.5, 2.0, -1.5), (2.5, 2.8, -0.5)),
              3: ((-2.2, 2.8, -0.2), (-1.8, 3.2, 0.2)), 4: ((-2.4, 2.6, -0.4), (-1.6, 3.4, 0.4)), 5: ((-2.6, 2.4, -0.6), (-1.4, 3.6, 0.6))}
    for k, (lo, hi) in expect.items():
        i = leaf_of[k]
        assert (mn[i] <= np.array(lo)).all() and (mx[i] >= np.array(hi)).all(), k
        assert (mn[i] >= np.array(lo) - 0.01).all() and (mx[i] <= np.array(hi) + 0.01).all(), k     # and not much more


def test_tree_is_deterministic(pkg):
    a = pkg.light_tree(LM.query_case(pkg, "ico2")[0])
    b = pkg.light_tree(LM.query_case(pkg, "ico2")[0])
    for key in a:
        assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key


# ---- the weights ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LM.CASES)
def test_weights_are_the_rule(pkg, name):
    desc, keep, _ = LM.query_case(pkg, name)
    t = pkg.light_tree(desc)
    p, cdf = pkg.light_weights(desc)
    assert np.array_equal(t["p"].view(np.uint32), p.view(np.uint32)) and np.array_equal(t["cdf"].view(np.uint32), cdf.view(np.uint32))
    assert (np.diff(cdf.astype(np.float64)) >= 0).all() and cdf[-1] == np.float32(1.0) and (p >= 0).all()
    assert abs(float(p.astype(np.float64).sum()) - 1.0) < 1e-5
    if name == "graded_lamp":
        assert p.max() / p.min() >= 100.0
        # the areas themselves: cell (i, j) has edges e_i e_j, each of its two triangles half of it, the quad's area is 4
        e = np.diff(LM.graded_edges(8))
        want = np.repeat((e[:, None] * e[None, :]).reshape(-1) / 2.0, 2) / 4.0
        assert np.allclose(p, want, rtol=1e-6)
    if name == "mixed":
        assert p.max() / p.min() >= 1e3
        assert math.isclose(p[3] / p[0], 4.0 * math.pi * 0.04 / 2.0, rel_tol=1e-6)     # sphere r = 0.2 against the 2 x 1 rect
        assert math.isclose(p[2] / p[0], 2.0 * (0.8 + 0.8 + 1.0) / 2.0, rel_tol=1e-6)   # the 1 x 0.8 x 1 box


# ---- light_reference in f64 with the flag ---------------------------------------------------------------------------------------------------------
def _icosphere0(pkg, lights_many):
    b = pkg.SceneBuilder()
    lamp, grey = b.diffuse_light((4, 4, 4)), b.lambertian((0.7, 0.7, 0.7))
    tris, _ = pkg.icosphere(0)
    lights = [b.triangle(*(0.8 * t + np.array([0.0, 3.0, 0.0])), lamp) for t in tris]
    desc = b.desc(b.hittable_list([b.xz_rect(-50, 50, -50, 50, -2, grey)] + lights), b.hittable_list(lights), lights_all_shapes=True, lights_many=lights_many)
    return desc, b


def test_congruent_members_the_flag_changes_no_pdf(pkg):
    """the 20 congruent triangles of icosphere(0): p_k = 1 / 20 up to rounding, so the weighted sum is the mean"""
    on, k1 = _icosphere0(pkg, True)
    off, k2 = _icosphere0(pkg, False)
    pts, states = LC.query_points("icosphere", ((-2.0, -1.0, -2.0), (2.0, 1.0, 2.0)))
    drawn = pkg.light_reference(on, pts, states)
    a = pkg.light_reference(on, pts, dirs=drawn["d"].astype(np.float32))["pdf"]
    b = pkg.light_reference(off, pts, dirs=drawn["d"].astype(np.float32))["pdf"]
    assert (a > 0).all() and np.abs(a / b - 1.0).max() <= 1e-12
    p, cdf = pkg.light_weights(on)
    assert len(set(p.tolist())) == 1 and p[0] == np.float32(0.05)


@pytest.mark.parametrize("name", ("three", "graded_lamp", "mixed"))
def test_pick_frequencies_follow_the_areas(pkg, name):
    desc, keep, box = LM.query_case(pkg, name)
    n = 1 << 16
    rng = np.random.default_rng(5)
    states = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    pts = np.zeros((n, 3), np.float32)
    ref = pkg.light_reference(desc, pts, states)
    p, _ = pkg.light_weights(desc)
    counts = np.bincount(ref["light"], minlength=len(p)).astype(np.float64)
    sigma = np.sqrt(n * p.astype(np.float64) * (1.0 - p.astype(np.float64)))
    assert (np.abs(counts - n * p.astype(np.float64)) <= 5.0 * sigma + 1e-9).all()
    assert (ref["n_draws"] == 3).all() or name == "mixed"              # one draw for the pick, two for a triangle


def test_the_estimator_is_unbiased_on_the_graded_lamp(pkg):
    """mean of 1 / pdf over directions drawn from the list = the solid angle of what the list covers: the quad, as two triangles"""
    desc, keep, box = LM.query_case(pkg, "graded_lamp")
    n = 1 << 16
    rng = np.random.default_rng(9)
    states = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    for point in ((0.3, 0.0, -0.2), (1.5, 1.0, 0.7)):
        pts = np.tile(np.array(point, np.float32), (n, 1))
        ref = pkg.light_reference(desc, pts, states)
        assert (ref["pdf"] > 0).all()
        w = 1.0 / ref["pdf"]
        q = LM.LAMP_FACE
        omega = pkg.solid_angle_triangle(np.array(point, float), q[0], q[1], q[2]) + pkg.solid_angle_triangle(np.array(point, float), q[0], q[2], q[3])
        se = w.std(ddof=1) / math.sqrt(n)
        print(f"{point}: mean 1/pdf {w.mean():.6f}, solid angle {omega:.6f}, SE {se:.2e}, z {(w.mean() - omega) / se:+.2f}")
        assert abs(w.mean() - omega) <= 5.0 * se


@pytest.mark.parametrize("name", LM.CASES)
def test_the_query_points_keep_the_undecidable_share_small(pkg, name):
    desc, keep, box = LM.query_case(pkg, name)
    pts, states = LC.query_points("many_" + name, box)
    r64 = pkg.light_reference(desc, pts, states, dtype=np.float64)
    ok = LM.decidable(r64)
    print(f"{name}: undecidable {1.0 - ok.mean():.4f}")
    assert 1.0 - ok.mean() <= LC.SKIP_SHARE
