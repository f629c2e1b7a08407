"""Camera lists on the CPU (csrc/camera_lists.h through rt_camera_lists_host): per 8 x 8-pixel square, the spheres of the tree a camera ray of
that square can meet. The lists are held to brute force: random camera rays made by the camera's own formulas (kernels.hip new_camera_ray, in
f32 as the device makes them, and in f64), every sphere whose LINE such a ray meets at t > 0 — the quadratic in f64 — must be in its square's
list, none may be missing; a square marked "walk" counts as covered. book-1 must not need the escape at K = 16, and a list names its spheres in
the order the node records reach their leaves.

book-1 at 1200 x 800 (scene seed 1, the bench's): mean list length 1.427, longest 9, 31.4 % of the squares empty, no square marked "walk"."""
import numpy as np
import pytest

N_RAYS = 200_000
WALK = 0xFFFFFFFF


def leaf_order(nodes):
    """Sphere indices in the order the node records reach their leaves (kind 1 = sphere: leaf = kind << 28 | count << 24 | first)."""
    out = []
    for leaf in nodes["leaf"]:
        leaf = int(leaf)
        if leaf and (leaf >> 28) == 1:
            out.extend(range(leaf & 0xFFFFFF, (leaf & 0xFFFFFF) + ((leaf >> 24) & 15)))
    return np.array(out, dtype=np.int64)


def camera_rays(cam, width, height, n, rng, dtype):
    """n rays of random pixels as new_camera_ray makes them (jitter, lens disk), evaluated in `dtype`; extra: corner cases of the jitter."""
    f = dtype
    v3 = lambda v: np.array([v.x, v.y, v.z], dtype=np.float32).astype(f)      # the device reads the camera as f32
    x, y = rng.integers(0, width, n), rng.integers(0, height, n)
    ju, jv = rng.random(n), rng.random(n)
    k = n // 16                                                               # a share of the rays on the edges of their pixel
    ju[:k] = rng.choice([0.0, 1.0 - 2.0 ** -24], k); jv[:k] = rng.choice([0.0, 1.0 - 2.0 ** -24], k)
    p = rng.uniform(-1, 1, (4 * n, 2))
    p = p[(p * p).sum(1) < 1.0][:n]
    p[:k] /= np.linalg.norm(p[:k], axis=1, keepdims=True) * (1 + 1e-7)        # ... and on the rim of the lens
    u = ((x.astype(f) + ju.astype(f)) / f(width - 1))[:, None]
    v = (((height - 1 - y).astype(f) + jv.astype(f)) / f(height - 1))[:, None]
    lens = f(np.float32(cam.lens_radius))
    off = v3(cam.u) * (lens * p[:, :1].astype(f)) + v3(cam.v) * (lens * p[:, 1:].astype(f))
    o = v3(cam.origin) + off
    d = v3(cam.lower_left_corner) + v3(cam.horizontal) * u + v3(cam.vertical) * v - v3(cam.origin) - off
    return x, y, o.astype(np.float64), d.astype(np.float64)


def missing(lists, width, x, y, o, d, spheres, members):
    """(rays x spheres met) pairs, and how many of them are in no list: brute force in f64 over `members` (sphere indices)."""
    sqx = (width + 7) // 8
    sq = (y >> 3) * sqx + (x >> 3)
    cnt = lists[sq, 0]
    n_met = n_missing = 0
    a = (d * d).sum(1)
    for s in members:
        c, r = spheres[s, :3].astype(np.float64), abs(float(spheres[s, 3]))
        oc = o - c
        hb = (oc * d).sum(1)
        disc = hb * hb - a * ((oc * oc).sum(1) - r * r)
        met = np.zeros(len(o), bool)
        ok = disc >= 0
        met[ok] = (-hb[ok] + np.sqrt(disc[ok])) / a[ok] > 0                   # the far root: some point of the ray at t > 0 is inside
        if not met.any():
            continue
        rows = lists[sq[met]]
        listed = (rows[:, 1:] == s) & (np.arange(16)[None, :] < np.minimum(rows[:, :1], 16))
        covered = listed.any(1) | (cnt[met] == WALK)
        n_met += int(met.sum()); n_missing += int((~covered).sum())
    return n_met, n_missing


def check(pkg, desc, cam, width, height, seed, n=N_RAYS):
    lists = pkg.camera_lists_host(desc, cam, width, height)
    assert lists is not None and lists.shape == (((width + 7) // 8) * ((height + 7) // 8), 17)
    nodes, spheres, _ = pkg.compile_dump(desc)
    order = leaf_order(nodes)
    rng = np.random.default_rng(seed)
    met = 0
    for dtype in (np.float32, np.float64):
        x, y, o, d = camera_rays(cam, width, height, n // 2, rng, dtype)
        m, miss = missing(lists, width, x, y, o, d, spheres, order)
        assert miss == 0, (dtype, miss, m)
        met += m
    # the order of a list is the leaf order
    rank = np.full(len(spheres), -1, dtype=np.int64); rank[order] = np.arange(len(order))
    for row in lists:
        k = int(row[0])
        if k == WALK:
            continue
        assert k <= 16 and (row[1 + k:] == 0).all()
        r = rank[row[1:1 + k]]
        assert (r >= 0).all() and (np.diff(r) > 0).all()
    return lists, met


def book1_camera(pkg, aspect, aperture):
    return pkg.camera_new((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0, 1, 0), 20.0, aspect, aperture, 10.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def book1(pkg):
    return pkg.HostScene("book1", 1)


def test_book1_bench_frame_needs_no_escape(pkg, book1):
    """The bench's frame and camera: conservative, no square marked "walk" at K = 16, and the lists are short (a useless predicate would hide here)."""
    cam = book1.camera(1200 / 800)
    lists, met = check(pkg, book1.desc, cam, 1200, 800, 1)
    cnt = lists[:, 0]
    assert (cnt != WALK).all()
    print(f"book-1 1200x800: mean list {cnt.mean():.3f}, longest {cnt.max()}, empty {float((cnt == 0).mean()):.3f}, spheres met by {N_RAYS} rays: {met}")
    assert met > N_RAYS // 2                     # the rays do meet spheres: the check above is not vacuous
    assert cnt.max() <= 12 and cnt.mean() < 2.5  # the issue's look-alike: 9 and 1.38
    # the ground is tested before the tree and is in no list
    first = pkg.compile_info(book1.desc)["first"]
    assert len(first) == 1 and first[0] >> 28 == 1
    ground = first[0] & 0xFFFFFF
    for row in lists:
        assert ground not in row[1:1 + int(row[0])]


@pytest.mark.parametrize("width,height,aperture", [(100, 52, 0.1), (1200, 800, 0.0), (1200, 800, 1.0), (100, 52, 0.0), (100, 52, 1.0), (64, 40, 0.1)])
def test_book1_frames_and_lenses(pkg, book1, width, height, aperture):
    """Frames that are no multiple of 8, lens radius 0, 0.05 (the book's) and 0.5."""
    check(pkg, book1.desc, book1_camera(pkg, width / height, aperture), width, height, 2)


def test_lens_vectors_that_are_not_orthonormal(pkg, book1):
    """An RtCamera filled by hand: new_camera_ray offsets the origin by R (u px + v py) whatever u and v are, so the lens the lists must
    cover is that ellipse, here 1.7 times longer than R along a skewed axis."""
    cam = book1_camera(pkg, 100 / 52, 1.0)
    u = np.array([cam.u.x, cam.u.y, cam.u.z]); v = np.array([cam.v.x, cam.v.y, cam.v.z])
    u, v = 1.7 * u, v + 0.5 * u
    cam.u.x, cam.u.y, cam.u.z = u
    cam.v.x, cam.v.y, cam.v.z = v
    plain, _ = check(pkg, book1.desc, book1_camera(pkg, 100 / 52, 1.0), 100, 52, 6)
    wide, _ = check(pkg, book1.desc, cam, 100, 52, 6)
    assert (np.minimum(wide[:, 0], 17) >= np.minimum(plain[:, 0], 17)).all() and not np.array_equal(wide, plain)


def small_scene(pkg, extra):
    rng = np.random.default_rng(5)
    b = pkg.SceneBuilder(bvh_seed=3)
    m, g = b.lambertian((0.5, 0.5, 0.5)), b.dielectric(1.5)
    ids = [b.sphere(rng.uniform(-6, 6, 3), float(rng.uniform(0.2, 1.0)), m) for _ in range(40)]
    ids += [b.sphere(c, r, g) for c, r in extra]
    return b, b.desc(b.bvh(ids)), len(ids) - len(extra)


def sphere_index(pkg, desc, centre):
    _, spheres, _ = pkg.compile_dump(desc)
    return int(np.argmin(np.abs(spheres[:, :3] - np.asarray(centre, np.float32)).sum(1)))


@pytest.mark.parametrize("aperture", [0.0, 0.1, 1.0])
def test_camera_inside_a_glass_sphere(pkg, aperture):
    """The lens lies inside a sphere: every ray leaves through it, every list names it."""
    keep, desc, _ = small_scene(pkg, [((9.0, 1.0, 9.0), 2.0)])
    cam = pkg.camera_new((9.0, 1.0, 9.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0, 1.5, aperture, 8.0, 0.0, 0.0)
    lists, _ = check(pkg, desc, cam, 96, 64, 3)
    s = sphere_index(pkg, desc, (9.0, 1.0, 9.0))
    for row in lists:
        assert row[0] == WALK or s in row[1:1 + int(row[0])]


def test_sphere_behind_the_camera(pkg):
    """A sphere wholly behind the lens is met by no ray at t > 0 — and is in no list, although every line of the frame's middle passes through it."""
    keep, desc, _ = small_scene(pkg, [((13.5, 1.5, 13.5), 1.0)])
    cam = pkg.camera_new((9.0, 1.0, 9.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0, 1.5, 0.2, 8.0, 0.0, 0.0)
    lists, _ = check(pkg, desc, cam, 96, 64, 4)
    s = sphere_index(pkg, desc, (13.5, 1.5, 13.5))
    for row in lists:
        assert row[0] != WALK and s not in row[1:1 + int(row[0])]


def test_sphere_at_the_corner_of_a_square(pkg):
    """A sphere that the rays of a square reach only at the square's corner: tangent, from outside, to the ray through the pixel corner
    (jitter 0, pinhole). The rays at that corner meet it; the four squares around the corner name it."""
    W, H = 96, 64
    cam = pkg.camera_new((9.0, 1.0, 9.0), (0.0, 0.0, 0.0), (0, 1, 0), 40.0, 1.5, 0.0, 8.0, 0.0, 0.0)
    v3 = lambda v: np.array([v.x, v.y, v.z])
    u, v = 40 / (W - 1), (H - 1 - 23) / (H - 1)            # the corner shared by squares (4, 2), (5, 2), (4, 3) ... : pixel (40, 23)'s lower left
    d = v3(cam.lower_left_corner) + u * v3(cam.horizontal) + v * v3(cam.vertical) - v3(cam.origin)
    d /= np.linalg.norm(d)
    n = v3(cam.horizontal) / np.linalg.norm(v3(cam.horizontal)) + v3(cam.vertical) / np.linalg.norm(v3(cam.vertical))
    n -= d * (n @ d); n /= np.linalg.norm(n)
    r = 0.3
    centre = v3(cam.origin) + 6.0 * d + n * r * (1 - 1e-4)
    keep, desc, _ = small_scene(pkg, [(tuple(centre), r)])
    lists, _ = check(pkg, desc, cam, W, H, 5)
    s = sphere_index(pkg, desc, centre)
    _, spheres, _ = pkg.compile_dump(desc)
    # the corner ray itself, from each of the four pixels that share the corner (jitter 0 or just below 1)
    e = 1.0 - 2.0 ** -24
    x = np.array([40, 39, 40, 39]); y = np.array([23, 23, 24, 24])
    ju = np.array([0.0, e, 0.0, e]); jv = np.array([0.0, 0.0, e, e])
    uu = ((x + ju) / (W - 1))[:, None]; vv = ((H - 1 - y + jv) / (H - 1))[:, None]
    dd = v3(cam.lower_left_corner) + uu * v3(cam.horizontal) + vv * v3(cam.vertical) - v3(cam.origin)
    oo = np.broadcast_to(v3(cam.origin), dd.shape)
    met, miss = missing(lists, W, x, y, oo, dd, spheres, [s])
    assert met >= 1 and miss == 0
    sqx = (W + 7) // 8
    for sx, sy in ((4, 2), (5, 2), (4, 3), (5, 3)):
        row = lists[sy * sqx + sx]
        assert row[0] == WALK or s in row[1:1 + int(row[0])]


def test_scenes_the_lists_do_not_serve(pkg):
    """A scene with a primitive that is no static sphere has no lists; the flag is part of the ABI."""
    hs = pkg.HostScene("cornell", 0)
    assert pkg.camera_lists_host(hs.desc, hs.camera(1.0), 64, 64) is None
    assert pkg._abi.RT_FLAG_NO_CAMERA_LISTS == 16
