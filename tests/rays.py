"""Ray sets for the ray-query tests (tests/test_rays_host.py, tests/test_gpu_rays.py, tests/test_gpu_occlusion.py): six small scenes that
fit LDS, and per scene a fixed list of f32 rays — pixel-centre camera rays plus one generation of secondary rays from the CPU checker's
hit points in seeded random directions — with the checker's f64 answer for every ray, which rays are DECIDABLE, and which object every
hit lies on. And two scenes that do not fit LDS (tests/test_gpu_rays_hbm.py) — `field`, a static BVH, and `yard`, a BVH over a time
range with instances and moving spheres, each with a `_sah` twin — their sets made the same way, the uploads they are walked through
(field_matrix) and the checker's own f32 figures that bound the device there (MEASURED_F32_CHECKER).
And two families of rays those sets never hold (further down): axis_set — directions with zero, signed-zero, subnormal or 1e-30
components from origins on the 1/4 lattice, with the rim and edge subsets — and segment_set — point-to-point rays d = q - p with a
t_max of their own near 1.

A ray is undecidable when the checker's answer changes under a perturbation of its direction by +-R f32 ulps per component (8 fixed sign
patterns): hit <-> miss, t moving by more than 1e-3 * max(1, t), or front_face flipping. Such a ray grazes a silhouette or an edge; an f32
traversal may land on either side of it, and the tests leave it out (and say how many there were). Where an instance frame lies far
from the world's (`yard`, instance C) the origin is perturbed too: O_ULPS, origin_undecidable."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# R: 64 ulps, from the device's own error. The case that decides it is a ray of book-1 that passes 1e-5 inside the silhouette of an
# r = 0.2 sphere 8.4 units away (16 ulps do not reach it, and the device reports the ground behind the sphere). The device's f64 refinement of a sphere root forms the
# discriminant hb^2 - a * c with a = |d|^2 as the f32 traversal carries it (relative error ~eps = 6e-8), so the discriminant is good to
# eps * a * |oc|^2, which moves a silhouette by eps * |oc|^2 / (2 r) — 1e-5 units here. A perturbation of R ulps moves the ray sideways by
# about R * 1.2e-7 * |oc| at the sphere: covering the device's error needs R >= |oc| / (4 r), i.e. 10 for that ray and 31 for the farthest
# small spheres of the scene (|oc| = 25); R = 64 keeps a factor of two. The 1 % cap holds with room (2 of 2688 rays of book-1, none elsewhere).
R_ULPS = 64
SMALL = 1e-20           # a direction component below this is "zero-class": see undecidable()
SIGNS = [(1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1), (-1, 1, 1), (-1, 1, -1), (-1, -1, 1), (-1, -1, -1)]
SCENES = ["book1", "cornell", "mesh", "moving", "rotated_sphere", "earth"]
STATIC_SCENES = ["book1", "cornell", "mesh", "rotated_sphere", "earth"]
# the ray set of scenes that do not fit LDS (tests/test_gpu_rays_hbm.py): one geometry, the reference's BVH builder and the SAH one
HBM_SCENES = ["field", "field_sah", "yard", "yard_sah"]
HBM_OF = {"field": ["field", "field_sah"], "yard": ["yard", "yard_sah"]}
HBM_GEOMETRY = {"field": "field", "field_sah": "field", "yard": "yard", "yard_sah": "yard"}   # the sets depend on the geometry alone
FIELD_SPHERES, FIELD_GRID, FIELD_SEED, FIELD_BOX_RAYS = 1250, 23, 20250317, 64
# `yard` (yard_scene): what stands alone in a cell of the unit lattice, the frame instance C is built in, and the xz footprints
# (x0, x1, z0, z1) the lattice keeps free for the instances A, B, C, D
YARD_SEED, YARD_FAR = 20261020, 400.0
YARD_SPHERES, YARD_MOVING, YARD_BOXES, YARD_RECTS = 450, 450, 80, 60
YARD_BLOCKS = {"A": (-7.5, -0.5, -7.5, -0.5), "B": (0.4, 7.6, 0.4, 7.6), "C": (-10.6, -5.4, -0.6, 4.6), "D": (2.4, 9.6, -9.6, -2.4)}
YARD_D = ((90.0, (4.2, -6.0)), (180.0, (7.8, -6.0)))      # D's two groups: the angle of the RotateY above each, and where it stands in the world (x, z)
GRID = (48, 32)         # camera rays per scene: pixel centres of a 48 x 32 frame (+ as many secondary rays as they have hits)


def earth_image():
    from PIL import Image
    return np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "earthmap_rgb.png")).convert("RGB"))


class Built:
    """A scene description, its camera and whatever keeps their memory alive."""
    def __init__(self, desc, cam, keep, extent):
        self.desc, self.cam, self.keep, self.extent = desc, cam, keep, extent


def field_scene(pkg, builder):
    """A static BVH that does not fit LDS (a few thousand records, more than the default LDS top of 1024 and at most the 4096 a top can hold):
    FIELD_SPHERES spheres over a height field of FIELD_GRID^2 x 2 triangles, one Box, one ground rect. No two surfaces meet — spheres
    are placed by rejection, 0.05 apart and outside the box's footprint; the height field lies between the rect and everything else —
    so no ray finds two primitives at one t, the one way layouts may differ (include/rt_hip.h, the layout section)."""
    rng = np.random.default_rng(FIELD_SEED)
    b = pkg.SceneBuilder(background=(0.5, 0.7, 1.0), background_mode=pkg._abi.RT_BG_SKY_GRADIENT, bvh_builder=builder)
    mats = [b.lambertian((0.7, 0.3, 0.3)), b.metal((0.8, 0.8, 0.8), 0.1), b.dielectric(1.5)]
    centres, radii = np.zeros((FIELD_SPHERES, 3)), np.zeros(FIELD_SPHERES)
    k = 0
    while k < FIELD_SPHERES:
        c = np.array([rng.uniform(-12.0, 12.0), rng.uniform(0.5, 3.5), rng.uniform(-12.0, 12.0)])
        r = rng.uniform(0.2, 0.4)
        if abs(c[0]) < 1.6 and abs(c[2]) < 1.6:
            continue
        if k and (np.linalg.norm(centres[:k] - c, axis=1) < radii[:k] + r + 0.05).any():
            continue
        centres[k], radii[k] = c, r
        k += 1
    ids = [b.sphere(centres[i], float(radii[i]), mats[i % 3]) for i in range(FIELD_SPHERES)]
    n = FIELD_GRID
    h = rng.uniform(-1.0, -0.2, (n + 1, n + 1))
    P = lambda i, j: (-12.0 + 24.0 * i / n, float(h[i, j]), -12.0 + 24.0 * j / n)
    tri_mats = [b.lambertian((0.3, 0.6, 0.3)), b.metal((0.7, 0.7, 0.9), 0.2)]
    for i in range(n):
        for j in range(n):
            ids.append(b.triangle(P(i, j), P(i + 1, j), P(i, j + 1), tri_mats[(i + j) & 1]))
            ids.append(b.triangle(P(i + 1, j), P(i + 1, j + 1), P(i, j + 1), tri_mats[(i + j + 1) & 1]))
    ids.append(b.box((-1.0, 0.0, -1.0), (1.0, 2.0, 1.0), b.lambertian((0.8, 0.7, 0.2))))
    ids.append(b.xz_rect(-14, 14, -14, 14, -1.25, b.lambertian((0.5, 0.5, 0.5))))
    desc = b.desc(b.bvh(ids))
    cam = pkg.camera_new((14.0, 5.0, 16.0), (0.0, 0.5, 0.0), (0, 1, 0), 40.0, 1.5, 0.0, 10.0, 0.0, 0.0)
    return Built(desc, cam, b, 14.0)


# a top of `yard` that holds the LT_XFORM records of the instances A, B and C and not their subtrees (the reference's builder makes a
# balanced tree over 1,043 members: the instances sit 11 levels down, below every smaller top): tests/test_rays_host.py::test_yard_top_layouts
YARD_TOP = 3000


def field_matrix(A, scene="field"):
    """The uploads of tests/test_gpu_rays_hbm.py for `field` or `yard`: case -> (scene, layout flags, the other RtUploadOptions fields).
    None of them fits LDS (tests/test_rays_host.py::test_field_does_not_fit_lds), but `collapse_4`: leaf_collapse = 4 folds the tree to
    ~1,600 records (yard: ~1,900), which do; `collapse_4_hbm` is the same upload kept out of LDS by flag. On `yard`, which is no static
    BVH, the `wide` cases keep the binary walk."""
    m = {"c16": (0, {}), "c16_one_order": (A.RT_LAYOUT_CHILD_ORDER_AS_REFERENCE, {})}
    for k in range(1, 8):
        m[f"c16_axes_{k}"] = (0, dict(octant_axes=k))
    for k in (1, 2, 3, 7, 100, 0, 4096) + ((YARD_TOP,) if scene == "yard" else ()):
        m[f"top_{k or 1024}"] = (A.RT_LAYOUT_NODES_32B, dict(lds_top_records=k))
    m["top_one_order"] = (A.RT_LAYOUT_NODES_32B | A.RT_LAYOUT_CHILD_ORDER_AS_REFERENCE, dict(lds_top_records=7))
    m["member_boxes"] = (A.RT_LAYOUT_MEMBER_BOXES, {})
    m["lists_as_reference"] = (A.RT_LAYOUT_LISTS_AS_REFERENCE, {})
    m["lists_as_reference_top_7"] = (A.RT_LAYOUT_LISTS_AS_REFERENCE | A.RT_LAYOUT_NODES_32B, dict(lds_top_records=7))
    m["park_cost"] = (0, dict(list_park_cost=2.0))
    m["wide"] = (A.RT_LAYOUT_WIDE_NODES, {})
    m["collapse_4"] = (0, dict(leaf_collapse=4))
    m["collapse_4_hbm"] = (A.RT_LAYOUT_SCENE_IN_HBM, dict(leaf_collapse=4))
    out = {k: (scene,) + v for k, v in m.items()}
    for k in ("c16", "top_1024", "wide"):
        out[k + "_sah"] = (scene + "_sah",) + m[k]
    return out


FITS_LDS = ("collapse_4",)          # the cases of field_matrix whose flags make the scene fit LDS


def top_rule(skip, max_top):
    """Records of the top of the tree a NODES_32B upload keeps in LDS (RtStats.lds_top_nodes), restated from the skip links of the
    compiled records: depth = the number of enclosing subtrees [i, skip_i); the top is every record above the deepest cut that holds at
    most max_top records — or nothing, when the first level alone exceeds max_top or the whole tree fits."""
    return int(top_mask(skip, max_top).sum())


def top_mask(skip, max_top):
    """top_rule's records themselves: a mask over the compiled records."""
    n, ends, depth = len(skip), [], np.zeros(len(skip), np.int64)
    for i in range(n):
        while ends and ends[-1] <= i:
            ends.pop()
        depth[i] = len(ends)
        if skip[i] > i + 1:
            ends.append(int(skip[i]))
    per_depth = np.bincount(depth)
    total = cut = 0
    for count in per_depth:
        if total + count > max_top:
            break
        total += count
        cut += 1
    return depth < cut if 0 < total < n else np.zeros(n, bool)


def xform_pairs(leaf):
    """[(enter, exit)] record indices of every LT_XFORM pair of a compiled record array (csrc/device_types.h: leaf type 6, bit 23 set on
    the record that closes a wrapper), innermost pairs first as they close."""
    kind, is_exit = np.asarray(leaf) >> 28, (np.asarray(leaf) & (1 << 23)) != 0
    open_, pairs = [], []
    for i in np.flatnonzero(kind == 6):
        if is_exit[i]:
            pairs.append((open_.pop(), int(i)))
        else:
            open_.append(int(i))
    assert not open_
    return pairs


def field_box_rays(rng):
    """FIELD_BOX_RAYS primary rays at the Box of field_scene, from seeded points above the spheres towards seeded points inside the box.
    The camera's own rays reach the box on a handful of pixels (it stands behind 14 units of spheres: 1 to 10 hits over 40 scene seeds);
    these make it a kind the set covers. They get their secondary rays like every other primary ray."""
    o = np.stack([rng.uniform(-4.0, 4.0, FIELD_BOX_RAYS), rng.uniform(4.5, 7.0, FIELD_BOX_RAYS), rng.uniform(-4.0, 4.0, FIELD_BOX_RAYS)], axis=1)
    to = np.stack([rng.uniform(-0.9, 0.9, FIELD_BOX_RAYS), rng.uniform(0.1, 1.9, FIELD_BOX_RAYS), rng.uniform(-0.9, 0.9, FIELD_BOX_RAYS)], axis=1)
    return make_rays(o, to - o, np.zeros(FIELD_BOX_RAYS))


def rot_y(deg, x, z, inverse=False):
    """RotateY's map of a point (hittable.rs:152-157: child -> parent), or its inverse (parent -> child)."""
    th = np.radians(deg); c, s = np.cos(th), np.sin(th)
    return (c * x - s * z, s * x + c * z) if inverse else (c * x + s * z, -s * x + c * z)


def yard_scene(pkg, builder):
    """A BVH over a time range that does not fit LDS, with instances and moving spheres (tests/test_gpu_rays_hbm.py): spheres, moving
    spheres, Translate(RotateY(Box)) with an angle each, and rects of all three axes (every second one under FlipFace), each alone
    in a cell of the unit lattice over [-12, 12) x [0, 4) x [-12, 12); and in the footprints the lattice keeps free (YARD_BLOCKS):
    A  Translate(RotateY(BVH(500 spheres on a 0.5 lattice), 30), (-4, 0, -4)), the shape of main.rs:640-646;
    B  RotateY(Translate(RotateY(BVH(12 x 12 x 2 triangles), 20), T), 25) with T such that it stands at (4, 0, 4): a chain of three;
    C  Translate(BVH(50 spheres + 50 moving spheres around (far, 0, far), 0, 1), (-8 - far, 0, 2 - far)), far = YARD_FAR: an instance
       whose own coordinates lie hundreds of units from where it stands (they stretch the compressed records' grid over the whole
       scene), with moving spheres inside;
    D  two groups of spheres, moving spheres, rects and a Box, under RotateY(90) and RotateY(180): the f32 sine / cosine of those is
       ~6e-17, not 0, so a world axis ray becomes a local ray with a component of that size made by the library itself.
    The ground rect lies beside the BVH in a HittableList. No two surfaces meet: every object keeps 0.05 from its cell's faces, and the
    instances from each other's footprints. Built.parts maps "A", "B", "C", "D" to the hittable ids of their primitives."""
    rng = np.random.default_rng(YARD_SEED)
    b = pkg.SceneBuilder(background=(0.5, 0.7, 1.0), background_mode=pkg._abi.RT_BG_SKY_GRADIENT, bvh_builder=builder)
    mats = [b.lambertian((0.7, 0.3, 0.3)), b.metal((0.8, 0.8, 0.8), 0.1), b.dielectric(1.5), b.lambertian((0.3, 0.4, 0.8)), b.metal((0.9, 0.6, 0.2), 0.3)]
    mat = lambda: mats[int(rng.integers(0, len(mats)))]
    u = rng.uniform

    def moving(cc, r):                                        # centres moving at most 0.2 per axis over times 0 .. 1, about cc
        delta = u(-0.2, 0.2, 3)
        return b.moving_sphere(cc - delta / 2, cc + delta / 2, 0.0, 1.0, r, mat())

    def rect(axis, cc, half, flip):
        lo, hi = cc - half, cc + half
        h = (b.xy_rect(lo[0], hi[0], lo[1], hi[1], cc[2], mat()) if axis == 0 else
             b.yz_rect(lo[1], hi[1], lo[2], hi[2], cc[0], mat()) if axis == 1 else b.xz_rect(lo[0], hi[0], lo[2], hi[2], cc[1], mat()))
        return b.flip_face(h) if flip else h

    free = lambda i, k: not any(i + 1 > x0 and i < x1 and k + 1 > z0 and k < z1 for x0, x1, z0, z1 in YARD_BLOCKS.values())
    cells = np.array([(i, j, k) for i in range(-12, 12) for k in range(-12, 12) if free(i, k) for j in range(4)], np.float64)
    cells = cells[rng.permutation(len(cells))][:YARD_SPHERES + YARD_MOVING + YARD_BOXES + YARD_RECTS] + 0.5
    ids = []
    for n, cc in enumerate(cells):
        if n < YARD_SPHERES:
            r = u(0.2, 0.3)
            ids.append(b.sphere(cc + u(-0.15, 0.15, 3), r, mat()))
        elif n < YARD_SPHERES + YARD_MOVING:
            ids.append(moving(cc + u(-0.05, 0.05, 3), u(0.15, 0.25)))
        elif n < YARD_SPHERES + YARD_MOVING + YARD_BOXES:
            h = u(0.15, 0.25, 3)
            ids.append(b.translate(b.rotate_y(b.box(-h, h, mat()), u(-180.0, 180.0)), cc + u(-0.05, 0.05, 3)))
        else:
            k = n - (YARD_SPHERES + YARD_MOVING + YARD_BOXES)
            ids.append(rect(k % 3, cc + u(-0.05, 0.05, 3), 0.35, (k // 3) & 1 == 1))        # the three axes take turns, plain and flipped
    parts, first = {}, 0

    def part(name):
        nonlocal first
        parts[name] = np.array([i for i in range(first, len(b.hittables)) if b.hittables[i].material >= 0])
        first = len(b.hittables)
    part("bare")
    # A
    sub = [b.sphere((-2.25 + 0.5 * i + u(-0.03, 0.03), 0.25 + 0.5 * j + u(-0.03, 0.03), -2.25 + 0.5 * k + u(-0.03, 0.03)), u(0.1, 0.2), mat())
           for i in range(10) for j in range(5) for k in range(10)]
    ids.append(b.translate(b.rotate_y(b.bvh(sub), 30.0), (-4.0, 0.0, -4.0)))
    part("A")
    # B
    n = 12
    h = rng.uniform(0.3, 1.2, (n + 1, n + 1))
    P = lambda i, j: (-2.5 + 5.0 * i / n, float(h[i, j]), -2.5 + 5.0 * j / n)
    sub = []
    for i in range(n):
        for j in range(n):
            sub.append(b.triangle(P(i, j), P(i + 1, j), P(i, j + 1), mats[(i + j) & 1]))
            sub.append(b.triangle(P(i + 1, j), P(i + 1, j + 1), P(i, j + 1), mats[3 + ((i + j) & 1)]))
    tx, tz = rot_y(25.0, 4.0, 4.0, inverse=True)
    ids.append(b.rotate_y(b.translate(b.rotate_y(b.bvh(sub), 20.0), (tx, 0.0, tz)), 25.0))
    part("B")
    # C
    far, sub = YARD_FAR, []
    for i in range(5):
        for j in range(4):
            for k in range(5):
                cc = np.array([far - 2.0 + i, 0.5 + j, far - 2.0 + k]) + u(-0.1, 0.1, 3)
                sub.append(moving(cc, u(0.15, 0.25)) if (i + j + k) & 1 else b.sphere(cc, u(0.2, 0.3), mat()))
    ids.append(b.translate(b.bvh(sub, 0.0, 1.0), (-8.0 - far, 0.0, 2.0 - far)))
    part("C")
    # D: twelve objects per group at world offsets (x, z) in {-1, 0, 1} x {-2.5 .. 2.5} about where the group stands, built in the group's own frame
    for deg, (wx, wz) in YARD_D:
        spots = [(ox, oy, oz) for ox in (-1.0, 0.0, 1.0) for oz in (-2.5, -1.5, -0.5, 0.5, 1.5, 2.5) for oy in (0.5, 1.5, 2.5)]
        sub = []
        for n, s in enumerate([spots[i] for i in rng.permutation(len(spots))[:12]]):
            lx, lz = rot_y(round(deg), wx + s[0], wz + s[2], inverse=True)
            cc = np.array([np.round(lx, 6), s[1], np.round(lz, 6)]) + u(-0.05, 0.05, 3)
            if n < 6:
                sub.append(b.sphere(cc, u(0.2, 0.3), mat()))
            elif n < 8:
                sub.append(moving(cc, u(0.15, 0.25)))
            elif n < 11:
                sub.append(rect(n % 3, cc, 0.35, n == 9))
            else:
                e = u(0.15, 0.3, 3)
                sub.append(b.box(cc - e, cc + e, mat()))
        ids.append(b.rotate_y(b.bvh(sub, 0.0, 1.0), deg))
    part("D")
    ground = b.xz_rect(-14, 14, -14, 14, -0.25, b.lambertian((0.5, 0.5, 0.5)))
    desc = b.desc(b.hittable_list([b.bvh(ids, 0.0, 1.0), ground]))
    cam = pkg.camera_new((14.0, 6.0, 16.0), (0.0, 1.0, 0.0), (0, 1, 0), 40.0, 1.5, 0.0, 10.0, 0.0, 1.0)
    built = Built(desc, cam, b, 14.0)
    built.parts = parts
    return built


def moving_centre(h, tm):
    a = list(h.p)
    return np.array(a[0:3]) + (tm - a[6]) / (a[7] - a[6]) * (np.array(a[3:6]) - np.array(a[0:3]))


def yard_aimed_rays(pkg, built, rng):
    """Primary rays at what the camera of yard_scene sees too little of, in the manner of field_box_rays: two at every xy and yz rect of
    the lattice, plain and flipped, one from each side out of the rect's own cell; 48 each at A, B and D and 96 at C from seeded points above the
    instance towards one of its objects; and 64 at bare moving spheres out of the sphere's own
    cell, at times within 0.02 of 0 and of 1. They get their secondary rays like every other primary ray."""
    A = pkg._abi
    H, u = built.desc.hittables, rng.uniform
    chains = {i: (h, chain) for i, h, chain in primitives(pkg, built.desc)}
    o, to, tm = [], [], []

    def add(a, b_, t):
        o.append(a); to.append(b_); tm.append(t)

    def to_world(chain, q):                                   # child -> parent, innermost wrapper first
        q = np.array(q, np.float64)
        for kind, prm in reversed(chain):
            if kind == A.RT_HIT_ROTATE_Y:
                q[0], q[2] = rot_y(prm[0], q[0], q[2])
            elif kind == A.RT_HIT_TRANSLATE:
                q = q + np.array(prm[:3])
        return q

    def centre(i, t):
        h, chain = chains[int(i)]
        a = list(h.p)
        if h.kind == A.RT_HIT_SPHERE:
            c = np.array(a[:3])
        elif h.kind == A.RT_HIT_MOVING_SPHERE:
            c = moving_centre(h, t)
        elif h.kind == A.RT_HIT_BOX:
            c = (np.array(a[0:3]) + np.array(a[3:6])) / 2
        elif h.kind == A.RT_HIT_TRIANGLE:
            c = (np.array(a[0:3]) + np.array(a[3:6]) + np.array(a[6:9])) / 3
        else:
            axes = {A.RT_HIT_XY_RECT: (0, 1, 2), A.RT_HIT_XZ_RECT: (0, 2, 1), A.RT_HIT_YZ_RECT: (1, 2, 0)}[h.kind]
            c = np.zeros(3)
            c[axes[0]], c[axes[1]], c[axes[2]] = (a[0] + a[1]) / 2, (a[2] + a[3]) / 2, a[4]
        return to_world(chain, c)
    for i in built.parts["bare"]:
        k = H[int(i)].kind
        if k in (A.RT_HIT_XY_RECT, A.RT_HIT_YZ_RECT):
            normal = 2 if k == A.RT_HIT_XY_RECT else 0
            for side in (-1.0, 1.0):
                c = centre(i, 0.0)
                a, t = c + u(-0.2, 0.2, 3), c + u(-0.25, 0.25, 3)
                a[normal], t[normal] = c[normal] + side * u(0.3, 0.4), c[normal]
                add(a, t, u(0.0, 1.0))
    for name, count in (("A", 48), ("B", 48), ("C", 96), ("D", 48)):
        ids = built.parts[name]
        for n in range(count):
            t = u(0.0, 1.0)
            c = centre(ids[rng.integers(0, len(ids))], t)
            add(np.array([c[0] + u(-3.0, 3.0), u(4.5, 7.0), c[2] + u(-3.0, 3.0)]), c + u(-0.1, 0.1, 3), t)
    bare_moving = [i for i in built.parts["bare"] if H[int(i)].kind == A.RT_HIT_MOVING_SPHERE]
    for n, i in enumerate(rng.choice(bare_moving, 64, replace=False)):
        t = u(0.0, 0.02) if n & 1 else u(0.98, 1.0)
        c = centre(i, t)
        d = rng.normal(size=3); d *= 0.42 / np.linalg.norm(d)
        add(np.floor(c) + 0.5 + d, c + u(-0.05, 0.05, 3), t)
    o, to = np.array(o), np.array(to)
    return make_rays(o, to - o, np.array(tm))


def build_scene(pkg, name):
    A = pkg._abi
    if name in HBM_SCENES:
        builder = A.RT_BVH_SAH if name.endswith("_sah") else A.RT_BVH_REFERENCE
        return yard_scene(pkg, builder) if HBM_GEOMETRY[name] == "yard" else field_scene(pkg, builder)
    if name == "book1":
        hs = pkg.HostScene("book1", 1)
        # (the book's camera looks at the origin, which is the north pole of the r = 1000 ground sphere: u is ill-conditioned within 3 units
        # of it. This one looks past it, so that polar hits stay rare.)
        return Built(hs.desc, pkg.camera_new((13.0, 2.0, 3.0), (6.0, 0.5, -4.0), (0, 1, 0), 20.0, 1.5, 0.0, 10.0, 0.0, 0.0), hs, 1000.0)
    if name == "cornell":
        hs = pkg.HostScene("cornell", 0)
        return Built(hs.desc, hs.camera(1.5), hs, 555.0)
    rng = np.random.default_rng(20240611)
    b = pkg.SceneBuilder(background=(0.5, 0.7, 1.0), background_mode=A.RT_BG_SKY_GRADIENT)
    t0 = t1 = 0.0
    lookfrom, lookat, vfov = (3.0, 2.0, 6.0), (0.0, 0.5, 0.0), 30.0
    if name == "mesh":
        # a bumpy height field of 12 x 12 x 2 = 288 triangles over a ground rect
        n, mats = 12, [b.lambertian((0.7, 0.3, 0.3)), b.metal((0.8, 0.8, 0.8), 0.1)]
        h = rng.uniform(0.0, 0.8, (n + 1, n + 1))
        P = lambda i, j: (-2.0 + 4.0 * i / n, float(h[i, j]), -2.0 + 4.0 * j / n)
        ids = []
        for i in range(n):
            for j in range(n):
                ids.append(b.triangle(P(i, j), P(i + 1, j), P(i, j + 1), mats[(i + j) & 1]))
                ids.append(b.triangle(P(i + 1, j), P(i + 1, j + 1), P(i, j + 1), mats[(i + j + 1) & 1]))
        ids.append(b.xz_rect(-6, 6, -6, 6, -0.25, b.lambertian((0.5, 0.5, 0.5))))
        world = b.bvh(ids)
    elif name == "moving":
        t1 = 1.0
        ids = [b.sphere((0, -100.5, 0), 100.0, b.lambertian((0.5, 0.5, 0.5)))]
        for k in range(40):
            c = np.array([rng.uniform(-2.5, 2.5), rng.uniform(0.0, 1.2), rng.uniform(-2.5, 2.5)])
            m = b.lambertian(rng.uniform(0, 1, 3)) if k & 1 else b.metal(rng.uniform(0.5, 1, 3), 0.0)
            if k % 3 == 0:
                ids.append(b.sphere(c, 0.25, m))
            else:
                ids.append(b.moving_sphere(c, c + np.array([0.0, rng.uniform(0.1, 0.5), rng.uniform(-0.3, 0.3)]), 0.0, 1.0, 0.25, m))
        world = b.bvh(ids, 0.0, 1.0)
    elif name == "rotated_sphere":
        # a sphere under a lone RotateY: hittable.rs:173 calls set_face_normal with the CHILD-space ray against the rotated-back normal
        s = b.rotate_y(b.sphere((1.0, 0.6, 0.3), 0.6, b.lambertian((0.8, 0.3, 0.3))), 65.0)
        g = b.rotate_y(b.sphere((-1.2, 0.5, -0.4), 0.5, b.dielectric(1.5)), -130.0)
        world = b.hittable_list([s, g, b.xz_rect(-5, 5, -5, 5, 0.0, b.lambertian((0.5, 0.5, 0.5)))])
    elif name == "earth":
        tex = b.image(earth_image())
        world = b.hittable_list([b.sphere((0, 0.9, 0), 0.9, b.lambertian(texture=tex)), b.sphere((0, -100, 0), 100.0, b.lambertian((0.5, 0.5, 0.5)))])
    else:
        raise KeyError(name)
    desc = b.desc(world)
    cam = pkg.camera_new(lookfrom, lookat, (0, 1, 0), vfov, 1.5, 0.0, 10.0, t0, t1)
    return Built(desc, cam, b, 100.0 if name in ("moving", "earth") else 6.0)


def medium_scene(pkg):
    """A scene with a ConstantMedium: ray queries refuse it."""
    b = pkg.SceneBuilder(background=(0.5, 0.7, 1.0))
    fog = b.constant_medium(b.sphere((0, 0, 0), 1.0, b.dielectric(1.5)), 0.2, (1, 1, 1))
    world = b.hittable_list([fog, b.sphere((0, -101, 0), 100.0, b.lambertian((0.5, 0.5, 0.5)))])
    return Built(b.desc(world), pkg.camera_new((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, 1.5, 0.0, 5.0, 0.0, 0.0), b, 100.0)


def make_rays(o, d, tm, t_max=0.0):
    from ray_tracer_archive_amd import RAY_DTYPE
    n = len(o)
    r = np.zeros(n, dtype=RAY_DTYPE)
    r["o"], r["d"], r["time"], r["t_max"] = np.asarray(o, np.float32), np.asarray(d, np.float32), np.asarray(tm, np.float32), t_max
    return r


def camera_rays(cam, width, height, rng):
    """Pixel-centre rays of Camera::get_ray (camera.rs:60-70) without lens offset, rounded to f32; times seeded in [time0, time1]."""
    v3 = lambda v: np.array([v.x, v.y, v.z])
    x, y = np.meshgrid(np.arange(width), np.arange(height))
    u = ((x + 0.5) / (width - 1)).reshape(-1, 1)
    v = ((height - 1 - y + 0.5) / (height - 1)).reshape(-1, 1)
    org = v3(cam.origin)
    d = v3(cam.lower_left_corner) + u * v3(cam.horizontal) + v * v3(cam.vertical) - org
    tm = rng.uniform(cam.time0, cam.time1, len(d)) if cam.time1 > cam.time0 else np.full(len(d), cam.time0)
    return make_rays(np.broadcast_to(org, d.shape), d, tm)


def limits(rays):
    """The interval's end the library reads from RtRay.t_max (include/rt_hip.h): <= 0, +inf or NaN mean no limit."""
    t = rays["t_max"].astype(np.float64)
    return np.where(t > 0.0, t, np.inf)


def ask(orc, desc, rays, precision=64, t_min=0.001, limit=None):
    """The checker's world.hit for every ray, as arrays: hit (bool), t, p, n, u, v, ff. One batch call: the scene is built once. The
    interval ends at `limit` (a scalar or one per ray), or, by default, where each ray's own t_max says."""
    lim = limits(rays) if limit is None else limit
    if np.ndim(lim) and np.isposinf(lim).all():
        lim = float("inf")
    hit, rec = orc.world_hit_many(desc, rays["o"], rays["d"], rays["time"], t_min, lim, precision)
    miss = ~hit
    out = dict(hit=hit, t=rec[:, 0].copy(), p=rec[:, 1:4].copy(), n=rec[:, 4:7].copy(), u=rec[:, 7].copy(), v=rec[:, 8].copy(), ff=rec[:, 9] != 0.0)
    out["t"][miss] = np.inf
    return out


def ask_per_ray(orc, desc, rays):
    """ask() through the per-ray entry orc_world_hit, which builds the scene for every ray: what the batch entry is held to, bit for bit."""
    n = len(rays)
    out = dict(hit=np.zeros(n, bool), t=np.full(n, np.inf), p=np.zeros((n, 3)), n=np.zeros((n, 3)), u=np.zeros(n), v=np.zeros(n), ff=np.zeros(n, bool))
    L = orc.lib()
    buf = (C.c_double * 10)()
    o3, d3 = (C.c_double * 3)(), (C.c_double * 3)()
    O, D, T = rays["o"].astype(np.float64), rays["d"].astype(np.float64), rays["time"].astype(np.float64)
    for i in range(n):
        o3[0], o3[1], o3[2] = O[i]
        d3[0], d3[1], d3[2] = D[i]
        k = L.orc_world_hit(C.byref(desc), o3, d3, T[i], 0.001, float("inf"), buf)
        if k < 0:
            raise RuntimeError("checker: " + L.orc_last_error().decode())
        if k > 0:
            out["hit"][i], out["t"][i], out["p"][i], out["n"][i] = True, buf[0], buf[1:4], buf[4:7]
            out["u"][i], out["v"][i], out["ff"][i] = buf[7], buf[8], buf[9] != 0.0
    return out


def changed(a, ref):
    """Rays on which the answer a is not the answer ref: hit <-> miss, t moved by more than 1e-3 * max(1, t), front_face flipped."""
    both = a["hit"] & ref["hit"]
    moved = np.zeros(len(both), bool)
    moved[both] = np.abs(a["t"][both] - ref["t"][both]) > 1e-3 * np.maximum(1.0, ref["t"][both])
    return (a["hit"] != ref["hit"]) | (both & (moved | (a["ff"] != ref["ff"])))


def undecidable(orc, desc, rays, ref, r_ulps=R_ULPS, small=SMALL):
    """The rule of the module's docstring. A component below `small` in magnitude (zero, a subnormal, 1e-30: its own ulp is no
    perturbation at all) is moved by R ulps of the ray's LARGEST component instead; small = 0 is the rule without that extension. No set
    made before the extension holds such a component, so their masks are the same bits under both
    (tests/test_rays_host.py::test_the_extended_rule_keeps_the_existing_masks)."""
    bad = np.zeros(len(rays), bool)
    d = rays["d"]
    ulp = np.spacing(np.abs(d))
    if small > 0.0:
        ulp = np.where(np.abs(d) < np.float32(small), np.spacing(np.abs(d).max(axis=1, keepdims=True)), ulp)
    step = np.float32(r_ulps) * ulp.astype(np.float32)
    for s in SIGNS:
        q = rays.copy()
        q["d"] = d + np.asarray(s, np.float32) * step
        bad |= changed(ask(orc, desc, q), ref)
    return bad


def to_local(pkg, chain, q):
    """The world points q (n, 3) in the frame below the wrappers `chain` (outermost first), in f64."""
    A = pkg._abi
    for kind, prm in chain:
        if kind == A.RT_HIT_TRANSLATE:
            q = q - np.array(prm[:3])
        elif kind == A.RT_HIT_ROTATE_Y:
            th = np.radians(prm[0]); c, s = np.cos(th), np.sin(th)
            q = np.stack([c * q[:, 0] - s * q[:, 2], q[:, 1], s * q[:, 0] + c * q[:, 2]], axis=1)
    return q


# O: 3 ulps of the coarsest frame, from the device's own arithmetic as R is. Below a Translate / RotateY the device tests a primitive
# against o_l = fl(o - offset) (csrc/kernels.hip xform_ray) and a centre it keeps in f32 (a moving sphere's: interpolated in f32): three
# roundings of half an ulp of the FRAME's coordinates in o_l - c, per axis. Where the frame's coordinates are no larger than the
# world's that is the rounding the ray's origin took when the set was made, and nothing new; in instance C of `yard`, 400 units out,
# it is 4.6e-5 units on a ray whose origin has an ulp of 5e-7 — a secondary ray that leaves a sphere of C at 89 degrees from the
# normal starts up to that far inside it and finds the sphere again at t = 4.6e-5 / cos = 2.6e-3 > t_min, which no perturbation of d
# produces (the f32 checker does, and so does the device: 1 decidable ray of the set by the rule on d alone). O = 3 is a factor of
# two, as R keeps.
O_ULPS = 3


def origin_undecidable(pkg, orc, desc, rays, ref, o_ulps=O_ULPS):
    """The rule of the module's docstring for the ORIGIN, where an instance frame makes it coarser: per ray, the frames (wrapper chains
    with a Translate or a RotateY) in which the origin's largest coordinate has a larger f32 ulp than in the world; the origin is moved
    by +-O of the largest such ulp per component (the 8 sign patterns), and a changed answer counts where the primitive hit, before or
    after, lies in one of those frames — the error enters in the tests of that frame's primitives and nowhere else. A scene without
    such a frame keeps its mask."""
    A = pkg._abi
    prims = primitives(pkg, desc)
    key = lambda chain: tuple((k, tuple(p[:3])) for k, p in chain if k != A.RT_HIT_FLIP_FACE)
    frames = {}
    for col, (_, _, chain) in enumerate(prims):
        if key(chain):
            frames.setdefault(key(chain), (chain, []))[1].append(col)
    bad = np.zeros(len(rays), bool)
    if not frames:
        return bad
    o = rays["o"].astype(np.float64)
    own = np.spacing(np.abs(rays["o"]).max(axis=1))
    step, coarse = np.zeros(len(rays), np.float32), np.zeros((len(rays), len(prims)), bool)      # coarse[i, k]: primitive k lies in a coarser frame of ray i
    for chain, cols in frames.values():
        ulp = np.spacing(np.abs(to_local(pkg, chain, o)).max(axis=1).astype(np.float32))
        coarse[:, cols] = (ulp > own)[:, None]
        step = np.where(ulp > own, np.maximum(step, ulp), step)
    touched = np.flatnonzero(step > 0)
    if not len(touched):
        return bad
    sub = rays[touched]
    sub_ref = {k: v[touched] for k, v in ref.items()}
    tm = sub["time"].astype(np.float64)
    on_ref = objects_at(pkg, desc, sub_ref["p"], tm, 0.0)[1] & sub_ref["hit"][:, None]
    for s in SIGNS:
        q = sub.copy()
        q["o"] = sub["o"] + np.asarray(s, np.float32) * (np.float32(o_ulps) * step[touched])[:, None]
        a = ask(orc, desc, q)
        k = np.flatnonzero(changed(a, sub_ref))
        if len(k):
            on_new = objects_at(pkg, desc, a["p"][k], tm[k], 0.0)[1] & a["hit"][k][:, None]
            bad[touched[k]] |= ((on_ref[k] | on_new) & coarse[touched[k]]).any(axis=1)
    return bad


# ---- which object a hit point lies on: a walk of the description in f64 -----------------------------------------------------------------
def primitives(pkg, desc):
    """[(hittable id, record, wrapper chain outermost first)] of every primitive reachable from desc.world."""
    A = pkg._abi
    out = []

    def walk(i, chain):
        h = desc.hittables[i]
        if h.kind in (A.RT_HIT_LIST, A.RT_HIT_BVH):
            for c in range(h.n_children):
                walk(desc.children[h.first_child + c], chain)
        elif h.kind in (A.RT_HIT_TRANSLATE, A.RT_HIT_ROTATE_Y, A.RT_HIT_FLIP_FACE):
            walk(h.first_child, chain + [(h.kind, list(h.p))])
        elif h.kind != A.RT_HIT_CONSTANT_MEDIUM:
            out.append((i, h, chain))
    walk(desc.world, [])
    return out


def surface_distance(pkg, h, chain, p, tm):
    """Distance of the world points p (n, 3) from the surface of primitive h under its wrappers, at the times tm."""
    A = pkg._abi
    q = to_local(pkg, chain, p)                               # world -> local, outermost wrapper first
    a = list(h.p)
    if h.kind == A.RT_HIT_SPHERE:
        return np.abs(np.linalg.norm(q - np.array(a[:3]), axis=1) - abs(a[3]))
    if h.kind == A.RT_HIT_MOVING_SPHERE:
        c0, c1 = np.array(a[0:3]), np.array(a[3:6])
        c = c0 + ((tm - a[6]) / (a[7] - a[6]))[:, None] * (c1 - c0)
        return np.abs(np.linalg.norm(q - c, axis=1) - abs(a[8]))

    def rect(ia, ib, ik, a0, a1, b0, b1, k):
        out_ = np.maximum.reduce([a0 - q[:, ia], q[:, ia] - a1, b0 - q[:, ib], q[:, ib] - b1, np.zeros(len(q))])
        return np.maximum(np.abs(q[:, ik] - k), out_)
    if h.kind == A.RT_HIT_XY_RECT:
        return rect(0, 1, 2, *a[:5])
    if h.kind == A.RT_HIT_XZ_RECT:
        return rect(0, 2, 1, *a[:5])
    if h.kind == A.RT_HIT_YZ_RECT:
        return rect(1, 2, 0, *a[:5])
    if h.kind == A.RT_HIT_BOX:
        lo, hi = np.array(a[0:3]), np.array(a[3:6])
        outside = np.maximum.reduce([lo - q, q - hi, np.zeros_like(q)]).max(axis=1)
        face = np.minimum(np.abs(q - lo), np.abs(q - hi)).min(axis=1)
        return np.maximum(outside, face)
    if h.kind == A.RT_HIT_TRIANGLE:
        v0, v1, v2 = np.array(a[0:3]), np.array(a[3:6]), np.array(a[6:9])
        nrm = np.cross(v1 - v0, v2 - v0); area2 = np.linalg.norm(nrm); nrm = nrm / area2
        plane = np.abs((q - v0) @ nrm)
        b1 = np.cross(q - v0, v2 - v0) @ nrm / area2
        b2 = np.cross(v1 - v0, q - v0) @ nrm / area2
        outside = np.maximum.reduce([-b1, -b2, b1 + b2 - 1.0, np.zeros(len(q))])
        return np.maximum(plane, outside * np.sqrt(area2))
    raise ValueError(h.kind)


def objects_at(pkg, desc, p, tm, extent):
    """(ids, on): ids[k] = hittable id of primitive k; on[i, k] = point i lies on primitive k (within 1e-7 of the scene's extent)."""
    prims = primitives(pkg, desc)
    dist = np.stack([surface_distance(pkg, h, chain, p, tm) for _, h, chain in prims], axis=1)
    return np.array([i for i, _, _ in prims]), dist <= 1e-7 * max(1.0, extent)


def yard_hit_classes(pkg, s):
    """{class: mask over the rays of a set of `yard`}: the checker's hit point lies on a primitive of that class — by kind, by the
    instance that holds it (Built.parts), and `flipped`: a rect of the lattice under FlipFace."""
    A = pkg._abi
    built, ids, on = s["built"], s["ids"], s["on"]
    kind = np.array([built.desc.hittables[int(i)].kind for i in ids])
    flipped = np.array([any(k == A.RT_HIT_FLIP_FACE for k, _ in chain) for _, _, chain in primitives(pkg, built.desc)])
    part = {name: np.isin(ids, members) for name, members in built.parts.items()}
    cols = {"bare spheres": part["bare"] & (kind == A.RT_HIT_SPHERE), "bare moving spheres": part["bare"] & (kind == A.RT_HIT_MOVING_SPHERE),
            "wrapped Boxes": part["bare"] & (kind == A.RT_HIT_BOX), "xy rects": part["bare"] & (kind == A.RT_HIT_XY_RECT),
            "yz rects": part["bare"] & (kind == A.RT_HIT_YZ_RECT), "flipped rects": part["bare"] & flipped,
            "spheres in A": part["A"] & (kind == A.RT_HIT_SPHERE), "triangles in B": part["B"] & (kind == A.RT_HIT_TRIANGLE),
            "spheres in C": part["C"] & (kind == A.RT_HIT_SPHERE), "moving spheres in C": part["C"] & (kind == A.RT_HIT_MOVING_SPHERE),
            "primitives in D": part["D"]}
    return {name: s["ref"]["hit"] & on[:, c].any(axis=1) for name, c in cols.items()}


def deviations(pkg, s, k, t, p, n, u, v):
    """Worst deviation from the set's f64 answers on the rays k, in the definitions of tests/test_gpu_rays.py: dict(t = relative |dt|,
    p = |dp| / extent, n = |dn|, uv = |d(u, v)| with u modulo 1 and sphere hits within 1e-3 of a pole left out, ta = |dt| / max(1, t), tabs = |dt|)
    and the rays that set each figure. t, p, n, u, v: the answers under test for the whole set."""
    A = pkg._abi
    built, ref, ids, on = s["built"], s["ref"], s["ids"], s["on"]
    f = lambda a: np.asarray(a)[k].astype(np.float64)
    dt = np.abs(f(t) - ref["t"][k])
    kind = np.array([built.desc.hittables[int(h)].kind for h in ids])
    polar = (on[k] & (kind == A.RT_HIT_SPHERE)[None, :]).any(axis=1) & ((ref["v"][k] < 1e-3) | (ref["v"][k] > 1.0 - 1e-3))
    du = np.abs(f(u) - ref["u"][k]); du = np.minimum(du, 1.0 - du)
    dv = np.abs(f(v) - ref["v"][k])
    each = dict(t=dt / ref["t"][k], p=np.linalg.norm(f(p) - ref["p"][k], axis=1) / built.extent, n=np.linalg.norm(f(n) - ref["n"][k], axis=1),
                uv=np.where(polar, 0.0, np.maximum(du, dv)), ta=dt / np.maximum(1.0, ref["t"][k]), tabs=dt)
    return {q: float(e.max()) for q, e in each.items()}, {q: int(k[int(e.argmax())]) for q, e in each.items()}


# The checker against itself: its f32 instance (Scene<float>) against its f64 answers on the decidable rays both hit, in deviations()'s
# definitions, measured on a CPU (tests/test_rays_host.py::test_field_f32_checker_figures measures them again and holds them to this
# table). What plain f32 arithmetic costs on this set; the device is allowed 2 x each figure (tests/test_gpu_rays_hbm.py), the factor of
# tests/test_gpu_paths.py. Nothing here comes from a GPU.
MEASURED_F32_CHECKER = {
    "field": dict(t=1.451e-2, p=2.312e-4, n=8.155e-3, uv=4.650e-3, ta=1.595e-4),
    "yard": dict(t=2.042e-3, p=2.076e-4, n=1.561e-2, uv=1.589e-3, ta=1.056e-4),
    # the axis sets and the segment sets (f32_figures; tabs = |dt| itself: a segment's t lies in [0, 1.5])
    "axis/book1": dict(t=2.055e-03, p=4.401e-07, n=2.297e-04, uv=8.022e-05, ta=1.815e-04, tabs=3.059e-04),
    "axis/cornell": dict(t=3.684e-06, p=3.697e-07, n=7.452e-07, uv=6.125e-07, ta=2.048e-06, tabs=3.302e-04),
    "axis/mesh": dict(t=3.176e-06, p=1.172e-07, n=1.835e-07, uv=1.478e-06, ta=3.700e-07, tabs=4.484e-06),
    "axis/moving": dict(t=2.263e-05, p=6.368e-07, n=5.229e-05, uv=6.683e-06, ta=1.189e-05, tabs=5.003e-05),
    "axis/rotated_sphere": dict(t=2.224e-06, p=7.986e-07, n=8.008e-06, uv=3.712e-06, ta=2.215e-06, tabs=1.260e-05),
    "axis/earth": dict(t=8.187e-05, p=4.391e-07, n=5.618e-06, uv=7.993e-06, ta=3.000e-05, tabs=4.451e-05),
    "axis/field": dict(t=2.407e-04, p=9.187e-06, n=3.806e-04, uv=1.074e-04, ta=1.154e-05, tabs=1.370e-04),
    "axis/yard": dict(t=1.229e-04, p=2.070e-05, n=1.243e-03, uv=2.235e-04, ta=1.768e-05, tabs=2.448e-04),
    "segments/book1": dict(t=4.815e-04, p=5.186e-06, n=3.406e-04, uv=1.564e-04, ta=1.958e-04, tabs=1.958e-04),
    "segments/cornell": dict(t=4.599e-06, p=4.664e-06, n=2.878e-05, uv=1.407e-05, ta=4.463e-06, tabs=4.463e-06),
    "segments/mesh": dict(t=2.977e-05, p=2.824e-07, n=1.922e-07, uv=5.427e-06, ta=7.834e-07, tabs=7.834e-07),
    "segments/moving": dict(t=1.879e-03, p=1.113e-05, n=7.259e-04, uv=3.158e-05, ta=9.867e-05, tabs=9.867e-05),
    "segments/field": dict(t=3.449e-03, p=1.498e-05, n=9.245e-04, uv=1.278e-04, ta=1.614e-05, tabs=1.614e-05),
    "segments/yard": dict(t=8.289e-03, p=1.461e-05, n=9.159e-04, uv=8.093e-05, ta=6.173e-05, tabs=6.173e-05),
}


def f32_checker_figures(pkg, orc, name):
    s = ray_set(pkg, orc, name)
    a = ask(orc, s["built"].desc, s["rays"], precision=32)
    k = np.flatnonzero(~s["undecidable"] & s["ref"]["hit"] & a["hit"])
    worst, at = deviations(pkg, s, k, a["t"], a["p"], a["n"], a["u"], a["v"])
    return worst, at, a


_cache = {}


def ray_set(pkg, orc, name):
    """dict(built, rays, ref, undecidable, by_origin, ids, on) for one scene, computed once per process. undecidable: by the rule on d
    or by the rule on o (origin_undecidable); by_origin: by the latter alone."""
    if name in _cache:
        return _cache[name]
    built = build_scene(pkg, name)
    if HBM_GEOMETRY.get(name, name) != name:                  # the geometry of "field" / "yard": the checker's answers do not depend on the device's builder
        _cache[name] = dict(ray_set(pkg, orc, HBM_GEOMETRY[name]), built=built)
        return _cache[name]
    rng = np.random.default_rng(7 + (SCENES + HBM_SCENES).index(name))
    prim = camera_rays(built.cam, GRID[0], GRID[1], rng)
    if name == "field":
        prim = np.concatenate([prim, field_box_rays(rng)])
    if name == "yard":
        prim = np.concatenate([prim, yard_aimed_rays(pkg, built, rng)])
    first = ask(orc, built.desc, prim)
    k = np.flatnonzero(first["hit"])
    dirs = rng.normal(size=(len(k), 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    sec = make_rays(first["p"][k], dirs, prim["time"][k])
    rays = np.concatenate([prim, sec])
    ref = ask(orc, built.desc, rays)
    by_d = undecidable(orc, built.desc, rays, ref)
    und = by_d | origin_undecidable(pkg, orc, built.desc, rays, ref)
    ids, on = objects_at(pkg, built.desc, ref["p"], rays["time"].astype(np.float64), built.extent)
    _cache[name] = dict(built=built, rays=rays, ref=ref, undecidable=und, by_origin=und & ~by_d, ids=ids, on=on)
    return _cache[name]


# ---- axis rays: directions with zero-class components, origins on the 1/4 lattice -------------------------------------------------------
# The slab tests cap |1/d| (csrc/kernels.hip set_slab_ray and its two copies), go_root picks the octant from the sign bit, and the
# primitive tests reject inf and NaN roots: none of which a camera ray or a random secondary ray reaches. These sets do.
AXIS_SCENES = ["book1", "cornell", "mesh", "moving", "rotated_sphere", "earth", "field", "yard"]
TIMED_SCENES = ("moving", "yard")                                                   # scenes with a time range: ray times are seeded over [0, 1]
AXIS_RAYS, AXIS_SEED = 2000, 99
ZERO_CLASS = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-30, -1e-30], np.float32)        # +-0, a subnormal, a tiny normal
# origins: uniform in this box around the scene's content (the Cornell box without its walls' planes; above book-1's ground)
AXIS_BOX = {"book1": ((-11, 0.05, -11), (11, 3, 11)), "cornell": ((5, 5, 5), (550, 550, 550)), "mesh": ((-5, -0.2, -5), (5, 2, 5)),
            "moving": ((-3, 0, -3), (3, 2.5, 3)), "rotated_sphere": ((-4, 0.05, -4), (4, 2.5, 4)), "earth": ((-3, 0.05, -3), (3, 2.5, 3)),
            "field": ((-13, -1.2, -13), (13, 6, 13)), "yard": ((-13, -0.2, -13), (13, 5, 13))}
RIM_SCENES, EDGE_SCENES = ("field", "mesh", "cornell", "yard"), ("mesh", "field")
EDGE_RAY = ((2.75, 0.5, 1.0), (-4.0, -0.24134248, -1e-30))      # in the plane z = 1 of `mesh`, through an edge two triangles share


def zero_class(d):
    return np.abs(d) < np.float32(SMALL)


def axis_dirs(rng, n):
    """About half pure axis directions (two zero-class components), half with one; the axis component is +-2^-3 .. 2^3."""
    d = np.zeros((n, 3), np.float32)
    kind = rng.integers(0, 2, n)
    for i in range(n):
        ax = rng.permutation(3)
        d[i, ax[0]] = np.float32(2.0 ** rng.integers(-3, 4)) * rng.choice([-1, 1])
        if kind[i]:
            d[i, ax[1]] = np.float32(rng.uniform(0.2, 2.0)) * rng.choice([-1, 1])
        for a in ax[1 + kind[i]:]:
            d[i, a] = rng.choice(ZERO_CLASS)
    return d


def rim_rays(name, rng):
    """Pure axis rays (true zeros, both signs) at an axis-aligned rect with an in-plane coordinate ON the rect's edge, or both on its
    corner: every coordinate is dyadic, the in-plane coordinate stays o + t * 0 = o, the interval is inclusive: a hit, exactly."""
    zero = lambda: rng.choice(ZERO_CLASS[:2])
    q = lambda lo, hi: np.round(rng.uniform(lo, hi) * 4) / 4
    o, d = [], []
    if name in ("field", "mesh", "yard"):            # the ground rect, from above, outside the height field and the spheres (yard: the lattice)
        e, top = (6.0, 2.0) if name == "mesh" else (14.0, 6.0)
        for k in range(48):
            a, b = rng.choice([-e, e]), (rng.choice([-e, e]) if k % 4 == 0 else q(-e, e))
            o.append((a, q(0.0, top), b) if k & 1 else (b, q(0.0, top), a))
            d.append((zero(), -(2.0 ** rng.integers(-3, 4)), zero()))
    if name == "cornell":                            # the far wall z = 555 along x = 0 / 555 and y = 555; the side walls along z = 555 and y = 555
        for k in range(48):
            e, s = rng.choice([0.0, 555.0]), q(360.0, 550.0)          # (above the tall box)
            m = 2.0 ** rng.integers(-3, 4)
            if k % 3 == 0:
                o.append((e, s, q(50.0, 500.0))); d.append((zero(), zero(), m))
            elif k % 3 == 1:
                o.append((q(50.0, 500.0), 555.0, q(50.0, 500.0))); d.append((zero(), zero(), m))
            else:
                o.append((q(50.0, 500.0), s, 555.0)); d.append((m * rng.choice([-1, 1]), zero(), zero()))
    return np.array(o, np.float64).reshape(-1, 3), np.array(d, np.float32).reshape(-1, 3)


def edge_rays(name, rng):
    """Rays that lie in a vertical plane which holds mesh edges, or go straight down onto mesh vertices and edges. Only the planes whose
    coordinate is dyadic qualify — the vertices are f64 in the description and f32 on the device: -1, 0, 1 (shared edges) and +-2 (the
    border) of `mesh`, +-12 (the border) of `field`. On a border the zero-class component is a true zero: a ray that drifts outwards by
    t * 1e-30 does leave the mesh."""
    border = 2.0 if name == "mesh" else 12.0
    zc = lambda at: rng.choice(ZERO_CLASS[:2] if abs(at) == border else ZERO_CLASS)
    q = lambda lo, hi: np.round(rng.uniform(lo, hi) * 4) / 4
    o, d = [], []

    def add(x, y, z, dx, dy, dz):
        o.append((x, y, z)); d.append((dx, dy, dz))
    if name == "mesh":
        add(*EDGE_RAY[0], *EDGE_RAY[1])
        for k in range(30):                          # in a plane x = c or z = c, from above the mesh (its heights end at 0.8) down onto it
            c, far, side = rng.choice([-2.0, -1.0, 0.0, 1.0, 2.0]), q(1.0, 1.75), rng.choice([-1, 1])
            run = -side * 2.0 ** rng.integers(0, 3)
            fall, y = -rng.uniform(0.5, 1.0) * abs(run), q(1.0, 1.25)
            add(c, y, side * far, zc(c), fall, run) if k & 1 else add(side * far, y, c, run, fall, zc(c))
        for k in range(30):                          # straight down onto an edge (one coordinate on a plane) or a vertex (both)
            c, b = rng.choice([-2.0, -1.0, 0.0, 1.0, 2.0]), (rng.choice([-1.0, 0.0, 1.0]) if k % 3 == 0 else q(-2.0, 2.0))
            m = -(2.0 ** rng.integers(-3, 4))
            add(c, q(1.0, 2.0), b, zc(c), m, zc(b)) if k & 1 else add(b, q(1.0, 2.0), c, zc(b), m, zc(c))
    if name == "field":                              # below the spheres (their lowest point is y = 0.1), above the height field (y <= -0.2)
        for k in range(30):
            c, b = rng.choice([-12.0, 12.0]), (rng.choice([-12.0, 12.0]) if k % 5 == 0 else q(-12.0, 12.0))
            m = -(2.0 ** rng.integers(-3, 4))
            add(c, 0.0, b, zc(c), m, zc(b)) if k & 1 else add(b, 0.0, c, zc(b), m, zc(c))
        for k in range(16):                          # along the border, in its plane
            c, run, b = rng.choice([-12.0, 12.0]), rng.choice([-1, 1]) * 2.0 ** rng.integers(0, 3), q(-6.0, 6.0)
            fall = -rng.uniform(0.1, 0.3) * abs(run)
            add(c, 0.0, b, zc(c), fall, run) if k & 1 else add(b, 0.0, c, run, fall, zc(c))
    return np.array(o, np.float64).reshape(-1, 3), np.array(d, np.float32).reshape(-1, 3)


def twin(rays):
    """The same rays with every zero-class component replaced by 1e-3 x the ray's largest component (the sign bit kept): an ordinary
    ray through nearly the same boxes, which no cap of |1/d| touches."""
    out = rays.copy()
    d = rays["d"]
    big = np.abs(d).max(axis=1, keepdims=True)
    out["d"] = np.where(zero_class(d), np.copysign(np.float32(1e-3) * big, d), d)
    return out


def finish_set(pkg, orc, built, rays, und):
    """und(ref): the set's rule on d; the rule on o (origin_undecidable) is added here, and `by_origin` are the rays it alone leaves out."""
    ref = ask(orc, built.desc, rays)
    ids, on = objects_at(pkg, built.desc, ref["p"], rays["time"].astype(np.float64), built.extent)
    by_d = und(ref)
    both = by_d | origin_undecidable(pkg, orc, built.desc, rays, ref)
    return dict(built=built, rays=rays, ref=ref, ids=ids, on=on, undecidable=both, by_origin=both & ~by_d)


def axis_set(pkg, orc, name):
    """dict(built, rays, ref, undecidable, decidable, ids, on, snapped, rim, edge) for one scene of AXIS_SCENES, computed once per
    process: AXIS_RAYS seeded rays, then the rim rays, then the edge rays. rim and edge (masks) are exempt from the perturbation rule —
    their answer is exact — so `undecidable` is never set on them, and decidable = ~undecidable is what the device is held to."""
    key = ("axis", name)
    if key in _cache:
        return _cache[key]
    built = build_scene(pkg, name)
    if HBM_GEOMETRY.get(name, name) != name:                  # the geometry of "field" / "yard" (as ray_set)
        _cache[key] = dict(axis_set(pkg, orc, HBM_GEOMETRY[name]), built=built)
        return _cache[key]
    rng = np.random.default_rng(AXIS_SEED + AXIS_SCENES.index(name))
    n = AXIS_RAYS
    lo, hi = np.array(AXIS_BOX[name][0], np.float64), np.array(AXIS_BOX[name][1], np.float64)
    o = rng.uniform(lo, hi, (n, 3))
    snapped = rng.integers(0, 2, n).astype(bool)
    o[snapped] = np.round(o[snapped] * 4) / 4
    d = axis_dirs(rng, n)
    tm = rng.uniform(0.0, 1.0, n) if name in TIMED_SCENES else np.zeros(n)
    ro, rd = rim_rays(name, rng) if name in RIM_SCENES else (np.zeros((0, 3)), np.zeros((0, 3), np.float32))
    eo, ed = edge_rays(name, rng) if name in EDGE_SCENES else (np.zeros((0, 3)), np.zeros((0, 3), np.float32))
    rays = make_rays(np.concatenate([o, ro, eo]), np.concatenate([d, rd, ed]), np.concatenate([tm, np.zeros(len(ro) + len(eo))]))
    rim, edge = np.zeros(len(rays), bool), np.zeros(len(rays), bool)
    rim[n:n + len(ro)] = True
    edge[n + len(ro):] = True
    s = finish_set(pkg, orc, built, rays, lambda ref: undecidable(orc, built.desc, rays, ref))
    # ... and the seeded rays that found an edge by themselves: the hit point lies on two triangles or more
    tri = np.array([built.desc.hittables[int(h)].kind == pkg._abi.RT_HIT_TRIANGLE for h in s["ids"]])
    edge |= s["ref"]["hit"] & (s["on"][:, tri].sum(axis=1) >= 2)
    s["undecidable"] &= ~(rim | edge)
    s["by_origin"] &= ~(rim | edge)
    s.update(snapped=np.concatenate([snapped, np.ones(len(ro) + len(eo), bool)]), rim=rim, edge=edge, decidable=~s["undecidable"])
    _cache[key] = s
    return s


# ---- segments: point-to-point rays, d = q - p, the interval ending near t = 1 -------------------------------------------------------------
SEGMENT_SCENES = ["book1", "cornell", "mesh", "moving", "field", "yard"]
SEGMENTS, SEGMENT_SEED, SEGMENT_MIN, SEGMENT_CAP = 2000, 5, 0.5, 0.05
T_SURFACE, T_FREE = 0.98, 1.5           # t_max of a segment whose target lies on a surface / is a free point
# both ends within this distance of the origin: segments that start or end hundreds of units out on a ground sphere say nothing about
# shadow rays (and the f32 checker, which sets the tolerances, loses the small spheres from there)
SEGMENT_REACH = {"book1": 15.0, "moving": 15.0}
# free targets within this distance of the source, per axis: `field` is dense (1250 spheres), and a segment across it is blocked nine
# times in ten
SEGMENT_LOCAL = {"field": 2.0, "yard": 2.0}
# surface targets within this distance of the source: a long segment is undecidable more often (t_min and t_max -+ 1e-3 are in units of
# |d|: 0.04 units at |d| = 20), and `yard` is held to a cap of 1 %. Every SEGMENT_LONG-th surface target stays where the seed put it,
# anywhere in the scene, so that long segments that end on a surface remain in the set
SEGMENT_NEAR = {"yard": 6.0}
SEGMENT_LONG = 8
SEGMENT_CAPS = {"yard": 0.01}           # (the others: SEGMENT_CAP)


def segment_undecidable(orc, desc, rays, ref):
    """The R-ulp rule on d (with the limit each segment carries), and in addition: the answer must not change with t_min halved or
    doubled — the origin surface's own root lies below 1e-4 in t for |d| >= 0.5 — nor with t_max -+ 1e-3, rays.py's own threshold for
    "t moved" and 100 x RT_SPHERE_TOL."""
    bad = undecidable(orc, desc, rays, ref)
    lim = limits(rays)
    for t_min, dl in ((0.0005, 0.0), (0.002, 0.0), (0.001, -1e-3), (0.001, 1e-3)):
        bad |= changed(ask(orc, desc, rays, t_min=t_min, limit=lim + dl), ref)
    return bad


def segment_set(pkg, orc, name):
    """dict(built, rays, ref, undecidable, ids, on, on_surface) for one scene of SEGMENT_SCENES: segments from decidable hit points p of
    ray_set (rounded to f32) to targets q — for half of them another hit point of that set (t_max = T_SURFACE: the segment stops short
    of the target's own surface), for the rest a seeded free point in AXIS_BOX (t_max = T_FREE) — with d = q - p in f32, |d| >= 0.5, and
    both ends within SEGMENT_REACH. ref is the checker's answer under each segment's own t_max."""
    key = ("segments", name)
    if key in _cache:
        return _cache[key]
    s = ray_set(pkg, orc, name)
    built, ref0 = s["built"], s["ref"]
    rng = np.random.default_rng(SEGMENT_SEED + SEGMENT_SCENES.index(name))
    k = np.flatnonzero(ref0["hit"] & ~s["undecidable"])
    if name in SEGMENT_REACH:
        k = k[np.linalg.norm(ref0["p"][k], axis=1) <= SEGMENT_REACH[name]]
    src = k[rng.integers(0, len(k), SEGMENTS)]
    p = ref0["p"][src].astype(np.float32)
    on_surface = np.arange(SEGMENTS) % 2 == 0
    lo, hi = np.array(AXIS_BOX[name][0], np.float64), np.array(AXIS_BOX[name][1], np.float64)
    if name in SEGMENT_LOCAL:
        lo, hi = np.maximum(lo, p - SEGMENT_LOCAL[name]), np.minimum(hi, p + SEGMENT_LOCAL[name])
    other = k[rng.integers(0, len(k), SEGMENTS)]
    if name in SEGMENT_NEAR:                                  # the first of a seeded order of the hit points that lies near enough
        for i in np.flatnonzero((np.linalg.norm(ref0["p"][other] - p, axis=1) > SEGMENT_NEAR[name]) & (np.arange(SEGMENTS) // 2 % SEGMENT_LONG != 0)):
            near = k[np.linalg.norm(ref0["p"][k] - p[i], axis=1) <= SEGMENT_NEAR[name]]
            other[i] = near[rng.integers(0, len(near))]
    q = np.where(on_surface[:, None], ref0["p"][other], rng.uniform(lo, hi, (SEGMENTS, 3))).astype(np.float32)
    d = q - p
    keep = np.linalg.norm(d.astype(np.float64), axis=1) >= SEGMENT_MIN
    rays = make_rays(p[keep], d[keep], s["rays"]["time"][src][keep], np.where(on_surface[keep], np.float32(T_SURFACE), np.float32(T_FREE)))
    out = finish_set(pkg, orc, built, rays, lambda ref: segment_undecidable(orc, built.desc, rays, ref))
    out["on_surface"] = on_surface[keep]
    out["decidable"] = ~out["undecidable"]
    _cache[key] = out
    return out


def new_set(pkg, orc, family, name):
    return axis_set(pkg, orc, name) if family == "axis" else segment_set(pkg, orc, name)


def f32_figures(pkg, orc, family, name):
    """The checker's f32 instance on a new set: its worst figures on the decidable rays on which it gives the f64 instance's answer
    (both hit, and changed() sees no difference: the figures are to say what f32 arithmetic costs on a hit, not how far apart two
    different surfaces lie; edge rays left out: which of the triangles that share the edge reports the hit, and with it n, u, v, is
    either instance's to choose), the rays that set them, its answers, and the decidable rays left out because its answer is another one:
    (hit / miss differs, both hit but t moved or front_face flipped). On book-1's segments those are the rays that leave the r = 1000
    ground sphere: |oc|^2 - r^2 in f32 is good to 0.06 there, and the f32 instance finds the sphere it stands on again at t ~ 0.01 —
    which the device, with its f64 roots, must not."""
    s = new_set(pkg, orc, family, name)
    a = ask(orc, s["built"].desc, s["rays"], precision=32, limit=limits(s["rays"]))
    other = changed(a, s["ref"])
    k = np.flatnonzero(s["decidable"] & ~s.get("edge", False) & s["ref"]["hit"] & a["hit"] & ~other)
    worst, at = deviations(pkg, s, k, a["t"], a["p"], a["n"], a["u"], a["v"])
    return worst, at, a, np.flatnonzero(s["decidable"] & (a["hit"] != s["ref"]["hit"])), np.flatnonzero(s["decidable"] & other & a["hit"] & s["ref"]["hit"])


def bound_of(key):
    """What the device is allowed on a new set: 2 x the f32 checker's own figure (the project's factor; nothing comes from a GPU)."""
    return {q: 2.0 * v for q, v in MEASURED_F32_CHECKER[key].items()}


def hold_to_checker(pkg, s, hits, key, label):
    """The assertions of tests/test_gpu_rays.py::test_rays_agree_with_the_checker for a new set (axis_set, segment_set) and the RtRayHit
    records `hits` of one upload: hit / miss on every decidable ray — rim and edge rays among them — and front_face on every decidable
    hit; the form of a miss; `hittable` a primitive the checker's point lies on, and its material; the deviations of t, p, n, u, v
    within bound_of(key). On an edge ray either triangle that shares the edge may report the hit, so front_face, n, u, v are not
    compared there: it must hit, on a primitive the checker's point lies on, at the checker's t within the same bound.
    Returns (worst figures, the rays that set them)."""
    A = pkg._abi
    built, ref, dec = s["built"], s["ref"], s["decidable"]
    none = np.zeros(len(dec), bool)
    rim, edge = s.get("rim", none), s.get("edge", none)
    g_hit, g_ff = (hits["flags"] & A.RT_RAYHIT_HIT) != 0, (hits["flags"] & A.RT_RAYHIT_FRONT_FACE) != 0
    assert ((hits["flags"] & ~np.uint32(3)) == 0).all()
    print(f"{label}: {len(dec)} rays, {int((~dec).sum())} undecidable (left out), {int(rim.sum())} rim, {int(edge.sum())} edge, {int((g_hit & dec).sum())} hits compared")
    wrong = np.flatnonzero(dec & (g_hit != ref["hit"]))
    what = [f"{i}{' (rim)' if rim[i] else ' (edge)' if edge[i] else ''}: o {s['rays']['o'][i].tolist()} d {s['rays']['d'][i].tolist()} checker t {ref['t'][i]!r} device t {hits['t'][i]!r}"
            for i in wrong[:8]]
    assert len(wrong) == 0, f"{label}: hit/miss differs on {len(wrong)} decidable rays: " + "; ".join(what)
    both = dec & g_hit
    wrong = both & ~edge & (g_ff != ref["ff"])
    assert not wrong.any(), f"{label}: front_face differs on decidable rays {np.flatnonzero(wrong)[:8]}"
    miss = ~g_hit
    assert np.isposinf(hits["t"][miss]).all() and (hits["hittable"][miss] == -1).all() and (hits["material"][miss] == -1).all()
    assert (hits["flags"][miss] == 0).all() and not hits["p"][miss].any() and not hits["n"][miss].any() and not hits["u"][miss].any() and not hits["v"][miss].any()
    ids, on = s["ids"], s["on"]
    col = np.full(built.desc.n_hittables, -1)
    col[ids] = np.arange(len(ids))
    k = np.flatnonzero(both)
    h = hits["hittable"][k]
    assert ((h >= 0) & (h < len(col))).all() and (col[h] >= 0).all(), f"{label}: a hittable that is not a primitive record"
    off = k[~on[k, col[h]]]
    assert len(off) == 0, f"{label}: rays {off[:8]}: the checker's hit point does not lie on the reported hittable {hits['hittable'][off[:8]]}"
    mat = np.array([built.desc.hittables[int(i)].material for i in h])
    assert (hits["material"][k] == mat).all(), f"{label}: material differs on rays {k[hits['material'][k] != mat][:8]}"
    worst, at = deviations(pkg, s, np.flatnonzero(both & ~edge), hits["t"], hits["p"], hits["n"], hits["u"], hits["v"])
    bound = bound_of(key)
    print(f"{label}: worst rel|dt| {worst['t']:.3e}  |dp|/extent {worst['p']:.3e}  |dn| {worst['n']:.3e}  |d(u,v)| {worst['uv']:.3e}  |dt|/max(1,t) {worst['ta']:.3e}"
          f"  |dt| {worst['tabs']:.3e}  at rays {at};  allowed {({q: f'{v:.3e}' for q, v in bound.items()})}")
    if (both & edge).any():
        e_worst, e_at = deviations(pkg, s, np.flatnonzero(both & edge), hits["t"], hits["p"], hits["n"], hits["u"], hits["v"])
        print(f"{label}: edge rays: worst rel|dt| {e_worst['t']:.3e}  |dp|/extent {e_worst['p']:.3e}  |dt|/max(1,t) {e_worst['ta']:.3e}  |dt| {e_worst['tabs']:.3e}")
        for q in ("t", "p", "ta", "tabs"):
            assert e_worst[q] <= bound[q], (label, "edge", q, e_worst[q], bound[q], e_at[q])
    for q in bound:
        assert worst[q] <= bound[q], (label, q, worst[q], bound[q], at[q])
    return worst, at
