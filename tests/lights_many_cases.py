"""Scenes shared by the tests of RT_SCENE_LIGHTS_MANY (test_lights_many_host.py, test_gpu_lights_many.py): lights lists with the flag pair set
(scene_flags = 5), a few units above the cloud of query points lights_cases uses.

    one, two, three   lists of 1, 2 and 3 triangles: a root that is a leaf, and an odd split
    graded_lamp       the XZ quad [-1, 1]^2 at y = 3 as 8 x 8 cells with geometrically graded edges (largest edge 12 x the smallest): 128 coplanar
                      triangles, flat boxes, areas spanning 144
    ico2              icosphere(2), 320 triangles of radius 0.5, each under Translate(RotateY(..))
    mixed             17 members: an XY and a YZ rect, a box, three concentric spheres (one ray meets several members), 11 triangles from 0.05 to
                      1.5 units across, four of them wrapped; areas span more than 10^3"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lights_cases as LC  # noqa: E402

CASES = ("one", "two", "three", "graded_lamp", "ico2", "mixed")
PICK_GAP = 2.0 ** -24          # a pick whose draw lies this close to a cdf edge is not held to the yardstick
LAMP_Y, GRADE = 3.0, 12.0
ICO_AT, ICO_R, ICO_DEG = (0.0, 2.6, 0.9), 0.5, 25.0
TRIS3 = (LC.TRI, ((1.5, 2.4, -1.2), (2.4, 2.9, -0.2), (1.2, 3.1, 0.4)), ((-2.2, 2.2, 0.8), (-1.1, 2.3, 1.9), (-2.0, 3.0, 1.6)))


def graded_edges(cells, lo=-1.0, hi=1.0, grade=GRADE):
    """cells + 1 coordinates from lo to hi whose steps grow geometrically, the last `grade` times the first"""
    r = grade ** (1.0 / (cells - 1))
    steps = r ** np.arange(cells)
    x = lo + (hi - lo) * np.concatenate([[0.0], np.cumsum(steps)]) / steps.sum()
    x[-1] = hi
    return x


def graded_lamp_triangles(cells=8, y=LAMP_Y):
    """(2 cells^2, 3, 3): every cell as two triangles whose front (the side cross(v1 - v0, v2 - v0) points to) faces down"""
    xs = zs = graded_edges(cells)
    out = []
    for i in range(cells):
        for j in range(cells):
            x0, x1, z0, z1 = xs[i], xs[i + 1], zs[j], zs[j + 1]
            out.append([(x0, y, z0), (x1, y, z1), (x0, y, z1)])
            out.append([(x0, y, z0), (x1, y, z0), (x1, y, z1)])
    return np.array(out)


LAMP_FACE = np.array([(-1.0, LAMP_Y, -1.0), (1.0, LAMP_Y, -1.0), (1.0, LAMP_Y, 1.0), (-1.0, LAMP_Y, 1.0)])      # the untessellated quad, front down


def ico2_world_triangles(pkg):
    tris, _ = pkg.icosphere(2)
    return LC._roty(ICO_R * tris, ICO_DEG) + np.array(ICO_AT)


def members(pkg, b, name, lamp):
    """the lights list's members, in list order"""
    if name in ("one", "two", "three"):
        return [b.triangle(*t, lamp) for t in TRIS3[:CASES.index(name) + 1]]
    if name == "graded_lamp":
        return [b.triangle(*t, lamp) for t in graded_lamp_triangles()]
    if name == "ico2":
        tris, _ = pkg.icosphere(2)
        return [b.translate(b.rotate_y(b.triangle(*(ICO_R * t), lamp), ICO_DEG), ICO_AT) for t in tris]
    if name == "mixed":
        out = [b.xy_rect(-1.0, 1.0, 2.0, 3.0, 3.0, lamp), b.yz_rect(2.0, 3.2, -0.5, 0.5, 2.9, lamp), b.box((1.5, 2.0, -1.5), (2.5, 2.8, -0.5), lamp)]
        out += [b.sphere((-2.0, 3.0, 0.0), r, lamp) for r in (0.2, 0.4, 0.6)]
        rng = np.random.default_rng(41)
        for k in range(11):
            size = (0.05, 0.05, 0.1, 0.2, 0.3, 0.4, 0.6, 0.8, 1.0, 1.2, 1.5)[k]
            c = np.array([rng.uniform(-2.0, 2.0), rng.uniform(2.2, 3.2), rng.uniform(-2.0, 2.0)])
            v = [c + size * rng.uniform(-0.5, 0.5, 3) for _ in range(3)]
            v[1][1] = v[0][1] + 0.3 * size                      # never edge-on to the points below: the triangle stays near a horizontal plane
            v[2][1] = v[0][1] - 0.2 * size
            t = b.triangle(*v, lamp)
            if k % 3 == 1:
                t = b.translate(b.rotate_y(t, 35.0 * k), (0.1 * k, 0.05 * k, -0.1 * k)) if k != 4 else b.flip_face(b.rotate_y(t, -50.0))
            out.append(t)
        return out
    raise KeyError(name)


def query_case(pkg, name, lights_many=True):
    """(desc, builder, (lo, hi) of the points' box): the lights are in the world too; flags 5, or 1 with lights_many=False"""
    b = pkg.SceneBuilder()
    lamp, grey = b.diffuse_light((4.0, 4.0, 4.0)), b.lambertian((0.7, 0.7, 0.7))
    lights = members(pkg, b, name, lamp)
    floor = b.xz_rect(-50.0, 50.0, -50.0, 50.0, -2.0, grey)
    desc = b.desc(b.hittable_list([floor] + lights), b.hittable_list(lights), lights_all_shapes=True, lights_many=lights_many)
    return desc, b, ((-2.0, -1.0, -2.0), (2.0, 1.0, 2.0))


def decidable(ref64):
    return LC.decidable(ref64) & (ref64["pick_gap"] > PICK_GAP)


def deviations(pkg, desc, pts, states):
    """lights_cases.deviations with the pick's own undecidable queries left out"""
    r64 = pkg.light_reference(desc, pts, states, dtype=np.float64)
    r32 = pkg.light_reference(desc, pts, states, dtype=np.float32)
    keep = decidable(r64)
    assert (r32["light"] == r64["light"])[keep].all() and (r32["n_draws"] == r64["n_draws"])[keep].all()
    dd = np.linalg.norm(r32["d"].astype(np.float64) - r64["d"], axis=1) / np.linalg.norm(r64["d"], axis=1)
    dp = np.abs(r32["pdf"].astype(np.float64) - r64["pdf"]) / r64["pdf"]
    return r64, keep, float(dd[keep].max()), float(dp[keep].max())


def emitter_case(pkg, name, lights_many=True):
    """(desc, builder, faces): lights_cases' floor under `graded_lamp` or `ico2` as the emitter; faces as lights_cases.form_factor reads them.
    ico2: the LIGHTS LIST holds the members under Translate(RotateY(..)); the WORLD holds the same triangles bare, at their world-space
    vertices. What emits is decided in the world, and there the reference's wrappers do not leave a DiffuseLight one-sided: RotateY::hit calls
    set_face_normal with the ray of its child space on the normal it has turned back (hittable.rs:173), so near the silhouette of a turned body
    Translate finds front_face false and the face is dark from outside — 0.9 % of this sphere's light at 25 degrees, growing as sqrt(spp) in z
    (measured on the device with scene_flags 1 and 5 alike). The closed form knows one-sided faces; bare triangles are exactly that."""
    b = pkg.SceneBuilder()
    lamp, grey = b.diffuse_light((LC.LE, LC.LE, LC.LE)), b.lambertian((LC.ALBEDO, LC.ALBEDO, LC.ALBEDO))
    lights = members(pkg, b, name, lamp)
    faces = [LAMP_FACE] if name == "graded_lamp" else list(ico2_world_triangles(pkg))
    in_world = lights if name == "graded_lamp" else [b.triangle(*t, lamp) for t in faces]
    floor = b.xz_rect(-60.0, 60.0, -60.0, 60.0, 0.0, grey)
    desc = b.desc(b.hittable_list([floor] + in_world), b.hittable_list(lights), lights_all_shapes=True, lights_many=lights_many)
    return desc, b, faces


def world_vertices(pkg, desc):
    """per member of a lights list of triangles (bare, or under wrappers): its (3, 3) world-space vertices, numpy f64 from the desc"""
    A = pkg._abi
    H, L = desc.hittables, desc.hittables[desc.lights]
    out = []
    for c in range(L.n_children):
        h, maps = H[desc.children[L.first_child + c]], []
        while h.kind in (A.RT_HIT_TRANSLATE, A.RT_HIT_ROTATE_Y, A.RT_HIT_FLIP_FACE):
            maps.append((h.kind, [h.p[i] for i in range(3)]))
            h = H[h.first_child]
        if h.kind != A.RT_HIT_TRIANGLE:
            out.append(None)
            continue
        v = np.array([h.p[i] for i in range(9)], dtype=np.float64).reshape(3, 3)
        for kind, p in reversed(maps):                            # innermost wrapper first
            if kind == A.RT_HIT_TRANSLATE:
                v = v + np.array(p)
            elif kind == A.RT_HIT_ROTATE_Y:
                v = LC._roty(v, p[0])
        out.append(v)
    return out


def node_boxes(nodes):
    """(mn, mx) (n, 3) f64 of the dumped records: centre -+ half extent, as the device reads them"""
    c = np.stack([nodes["cx"], nodes["cy"], nodes["cz"]], axis=1).astype(np.float64)
    h = np.stack([nodes["hx"], nodes["hy"], nodes["hz"]], axis=1).astype(np.float64)
    return c - h, c + h
