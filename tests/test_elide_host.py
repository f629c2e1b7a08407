"""Box records left out of a scene that is walked from LDS (csrc/scene_compile.cpp elide_box_nodes), on the CPU: the default dump against
the dump with RT_LAYOUT_ALL_BOX_NODES — which records went, that the links still lead where they led, that the Python walk of
tests/test_compile.py finds the same hits with fewer box tests, and that the kept set is the cheapest of ALL sets under the compiler's model."""
import itertools

import numpy as np
import pytest

import elide as E
from test_compile import traverse

# (spheres, bvh_seed, seed of the positions): the seeds of the two small scenes are picked so that the pass leaves out at least one record
SCENES = {9: (3, 1), 12: (7, 2), 137: (99, 4)}


def seeded(pkg, n):
    bvh_seed, seed = SCENES[n]
    rng = np.random.default_rng(seed)
    b = pkg.SceneBuilder(bvh_seed=bvh_seed)
    m = b.lambertian((0.5, 0.5, 0.5))
    ids = [b.sphere(rng.uniform(-8, 8, 3), rng.uniform(0.1, 1.0), m) for _ in range(n)]
    return b, b.desc(b.bvh(ids))


@pytest.fixture(scope="module")
def dumps(pkg):
    out = {}
    for n in SCENES:
        b, desc = seeded(pkg, n)
        full = pkg.compile_dump(desc, pkg._abi.RT_LAYOUT_ALL_BOX_NODES)
        dflt = pkg.compile_dump(desc, 0)
        out[n] = dict(keep=b, desc=desc, full=full, dflt=dflt, kept=E.kept_mask(full[0], dflt[0]))
    return out


@pytest.mark.parametrize("n", list(SCENES))
def test_elided_array_is_the_full_array_minus_inner_boxes(pkg, dumps, n):
    d = dumps[n]
    (full, sph_f, meta_f), (dflt, sph_d, meta_d), kept = d["full"], d["dflt"], d["kept"]
    assert np.array_equal(sph_f, sph_d) and np.array_equal(meta_f, meta_d)
    gone = full[~kept]
    assert len(gone) >= 1 and len(gone) == len(full) - len(dflt)
    assert np.all(gone["leaf"] == 0) and np.all(E.boxed(gone))
    assert set(np.flatnonzero(~kept)) <= set(E.inner_records(full))
    assert np.array_equal(full["leaf"][full["leaf"] != 0], dflt["leaf"][dflt["leaf"] != 0])          # the leaves, in their order
    E.check_links(full, dflt, kept)
    A = pkg._abi
    i_full, i_dflt = pkg.compile_info(d["desc"], A.RT_LAYOUT_ALL_BOX_NODES), pkg.compile_info(d["desc"], 0)
    assert i_dflt["n_nodes"] == len(dflt) and i_full["n_nodes"] == len(full)
    assert i_full["n_box_nodes"] - i_dflt["n_box_nodes"] == len(gone) and i_dflt["n_box_nodes"] <= len(dflt)
    assert i_full["fits_lds"] == i_dflt["fits_lds"] == 1


@pytest.mark.parametrize("n", list(SCENES))
def test_walk_finds_the_same_hits(pkg, dumps, n):
    d = dumps[n]
    (full, spheres, _), (dflt, _, _) = d["full"], d["dflt"]
    rng = np.random.default_rng(100 + n)
    v_full = v_dflt = n_hit = 0
    for _ in range(300):
        o = rng.uniform(-14, 14, 3)
        c = spheres[rng.integers(len(spheres))].astype(float)
        aim = c[:3] + rng.normal(size=3) * c[3]                     # near a sphere: about half of the rays hit something
        t0, k0, v0 = traverse(full, spheres, o, aim - o)
        t1, k1, v1 = traverse(dflt, spheres, o, aim - o)
        assert (t0, k0) == (t1, k1)
        n_hit += k0 >= 0
        v_full, v_dflt = v_full + v0, v_dflt + v1
    print(f"{n} spheres: {n_hit} of 300 rays hit, box tests {v_full} -> {v_dflt}")
    assert n_hit > 30
    if n == 137:
        assert v_dflt <= v_full


@pytest.mark.parametrize("n", [9, 12])
def test_kept_set_is_the_cheapest_of_all(pkg, dumps, n):
    """Every subset of the inner records, priced by the model restated in elide.model_cost: none is cheaper than the library's, and the
    library's is not the full array (a tie would have kept the record)."""
    d = dumps[n]
    full, kept = d["full"][0], d["kept"]
    inner = E.inner_records(full, every_child_boxed=False)       # the rule as the model states it, without the library's addition
    assert 1 <= len(inner) <= 11 and np.all(E.boxed(full))
    mine = E.model_cost(full, kept)
    costs = {}
    for r in range(len(inner) + 1):
        for out in itertools.combinations(inner, r):
            k = np.ones(len(full), bool)
            k[list(out)] = False
            costs[out] = E.model_cost(full, k)
    best = min(costs.values())
    print(f"{n} spheres: {len(inner)} inner records, {int((~kept).sum())} left out, model cost {costs[()]:.4f} -> {mine:.4f}, cheapest of {len(costs)} sets {best:.4f}")
    assert mine <= best + 1e-12 * max(1.0, best)
    assert (~kept).sum() >= 1 and mine < costs[()]


def test_book1_camera_rays_visit_fewer_boxes(pkg):
    hs = pkg.HostScene("book1", 1)
    A = pkg._abi
    full, spheres, _ = pkg.compile_dump(hs.desc, A.RT_LAYOUT_ALL_BOX_NODES)
    dflt, _, _ = pkg.compile_dump(hs.desc, 0)
    first = E.first_spheres(pkg.compile_info(hs.desc, 0))
    assert first == E.first_spheres(pkg.compile_info(hs.desc, A.RT_LAYOUT_ALL_BOX_NODES)) and len(first) == 1
    E.check_links(full, dflt, E.kept_mask(full, dflt))
    cam = hs.camera(1.5)
    o = np.array(cam.origin.tuple())
    llc, hor, ver = (np.array(v.tuple()) for v in (cam.lower_left_corner, cam.horizontal, cam.vertical))
    rng = np.random.default_rng(5)
    v_full = v_dflt = 0
    for _ in range(200):
        s, t = rng.uniform(0, 1, 2)
        dirn = llc + s * hor + t * ver - o
        t0, k0, v0 = traverse(full, spheres, o, dirn, first=first)
        t1, k1, v1 = traverse(dflt, spheres, o, dirn, first=first)
        assert (t0, k0) == (t1, k1)
        v_full, v_dflt = v_full + v0, v_dflt + v1
    print(f"book-1, 200 camera rays: box tests {v_full} -> {v_dflt} ({v_dflt / v_full:.3f})")
    assert v_dflt < 0.9 * v_full


def mixed_scene(pkg):
    """A BVH over spheres, two media, two moving spheres and two instanced boxes: leaves of every kind that comes without a box."""
    rng = np.random.default_rng(17)
    b = pkg.SceneBuilder(bvh_seed=11)
    m = b.lambertian((0.5, 0.5, 0.5))
    ids = [b.sphere(rng.uniform(-8, 8, 3), rng.uniform(0.2, 1.0), m) for _ in range(40)]
    for k in range(2):
        c = rng.uniform(-8, 8, 3)
        ids.append(b.constant_medium(b.sphere(c, 1.2, b.dielectric(1.5)), 0.5, (0.9, 0.9, 0.9)))
        c = rng.uniform(-8, 8, 3)
        ids.append(b.moving_sphere(c, c + [0, 0.5, 0], 0.0, 1.0, 0.4, m))
        ids.append(b.translate(b.rotate_y(b.box((-0.5, -0.5, -0.5), (0.5, 0.8, 0.5), m), 20.0 + 30 * k), rng.uniform(-8, 8, 3)))
    order = rng.permutation(len(ids))
    return b, b.desc(b.bvh([ids[k] for k in order], 0.0, 1.0))


@pytest.mark.parametrize("name", ["mixed", "final"])          # (scenes that hold such records)
def test_a_box_stays_above_a_record_without_one(pkg, name):
    """A medium, a moving sphere, the records that enter and leave an instance have no box of their own: the box above them is their only
    cull and stays, whatever the model says of it; everything that went had boxed children only."""
    A = pkg._abi
    keep, desc = mixed_scene(pkg) if name == "mixed" else (pkg.HostScene(name, 1), None)
    desc = desc if desc is not None else keep.desc
    full, dflt = pkg.compile_dump(desc, A.RT_LAYOUT_ALL_BOX_NODES)[0], pkg.compile_dump(desc, 0)[0]
    kept = E.kept_mask(full, dflt)
    E.check_links(full, dflt, kept)
    assert np.array_equal(full["leaf"][full["leaf"] != 0], dflt["leaf"][dflt["leaf"] != 0])
    strict, loose = set(E.inner_records(full)), set(E.inner_records(full, every_child_boxed=False))
    guards = loose - strict
    print(f"{name}: {len(full)} records, {int((~kept).sum())} left out of {len(strict)} that may go, {len(guards)} boxes kept for a child without one")
    assert (~kept).sum() >= 1 and set(np.flatnonzero(~kept)) <= strict
    assert len(guards) >= 1 and all(kept[g] for g in guards)
    bx, par = E.boxed(full), E.parents(full)
    assert all(kept[par[i]] for i in np.flatnonzero(~bx) if par[i] >= 0)


@pytest.mark.parametrize("bad", [float("nan"), 1e39, -1e39])
def test_box_that_is_not_finite(pkg, bad):
    """A sphere with a NaN or an overflowing coordinate gives every box above it a corner that is not finite. Such a record is no box
    test (the device passes that axis always): it stays, what lies below it is treated as trees of their own, and the compiler returns."""
    A = pkg._abi
    rng = np.random.default_rng(2)
    b = pkg.SceneBuilder(bvh_seed=7)
    m = b.lambertian((0.5, 0.5, 0.5))
    ids = [b.sphere(rng.uniform(-8, 8, 3), rng.uniform(0.1, 1.0), m) for _ in range(12)]
    ids[5] = b.sphere((1.0, bad, 2.0), 0.5, m)
    desc = b.desc(b.bvh(ids))
    full, dflt = pkg.compile_dump(desc, A.RT_LAYOUT_ALL_BOX_NODES)[0], pkg.compile_dump(desc, 0)[0]
    bx = E.boxed(full)
    assert (~bx).sum() >= 1
    kept = E.kept_mask(full, dflt)
    E.check_links(full, dflt, kept)
    assert np.all(kept[~bx]) and np.all(full["leaf"][~kept] == 0)
    assert pkg.compile_info(desc, 0)["n_nodes"] == len(dflt)
    inner = E.inner_records(full)
    if len(inner) <= 11:
        mine = E.model_cost(full, kept)
        best = mine
        for r in range(len(inner) + 1):
            for out in itertools.combinations(inner, r):
                k = np.ones(len(full), bool)
                k[list(out)] = False
                best = min(best, E.model_cost(full, k))
        assert mine <= best + 1e-12 * max(1.0, best)


@pytest.mark.parametrize("switch", ["RT_LAYOUT_LISTS_AS_REFERENCE", "RT_LAYOUT_NO_MEMBER_BOXES", "RT_LAYOUT_REFERENCE_COUNTERS", "RT_LAYOUT_SCENE_IN_HBM"])
def test_switches_that_keep_every_box(pkg, dumps, switch):
    A = pkg._abi
    f = getattr(A, switch)
    hs = pkg.HostScene("book1", 1)
    for desc in (hs.desc, dumps[137]["desc"]):
        a, b = pkg.compile_dump(desc, f), pkg.compile_dump(desc, f | A.RT_LAYOUT_ALL_BOX_NODES)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        assert pkg.compile_info(desc, f) == pkg.compile_info(desc, f | A.RT_LAYOUT_ALL_BOX_NODES)


def test_scene_that_does_not_fit_lds_keeps_every_box(pkg):
    hs = pkg.HostScene("big", 5, 20000, 32)
    A = pkg._abi
    assert pkg.compile_info(hs.desc, 0)["fits_lds"] == 0
    assert pkg.compile_info(hs.desc, 0) == pkg.compile_info(hs.desc, A.RT_LAYOUT_ALL_BOX_NODES)
