"""What the box-record elision of the scene compiler is worth in box tests, on the CPU: python scripts/cpu_elide_counts.py [--paths N] [--out FILE]
For book-1 under both builders (the reference's tree, RT_BVH_SAH): the dumped records with every box (RT_LAYOUT_ALL_BOX_NODES) and as an
upload lays them out (default), the compiler's choice checked against the model restated in tests/elide.py, and the Python walk of both
arrays over the segments of N camera paths — lens, diffuse (cosine), metal and glass bounces, depth 50; colours are not needed. Writes,
per builder: inner records, records left out, segments per path, box tests and sphere tests per segment before and after. Host only: no GPU,
and neither the checker nor the device's kernels take part."""
import argparse
import json
import math
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

META_MAT_MASK = (1 << 22) - 1      # csrc/device_types.h


def unit(v):
    n = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (v[0] / n, v[1] / n, v[2] / n)


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def in_unit_sphere(rnd):
    while True:
        p = (rnd.uniform(-1, 1), rnd.uniform(-1, 1), rnd.uniform(-1, 1))
        if dot(p, p) < 1:
            return p


def cosine_about(n, rnd):
    r1, r2 = rnd.random(), rnd.random()
    phi, s = 2 * math.pi * r1, math.sqrt(r2)
    x, y, z = math.cos(phi) * s, math.sin(phi) * s, math.sqrt(1 - r2)
    a = (0.0, 1.0, 0.0) if abs(n[0]) > 0.9 else (1.0, 0.0, 0.0)
    v = unit((n[1] * a[2] - n[2] * a[1], n[2] * a[0] - n[0] * a[2], n[0] * a[1] - n[1] * a[0]))
    u = (n[1] * v[2] - n[2] * v[1], n[2] * v[0] - n[0] * v[2], n[0] * v[1] - n[1] * v[0])
    return tuple(x * u[k] + y * v[k] + z * n[k] for k in range(3))


def scatter(mat, A, d, n_out, rnd):
    """The next direction of a path that hit a sphere with outward normal n_out, or None (absorbed)."""
    front = dot(d, n_out) < 0
    n = n_out if front else tuple(-c for c in n_out)
    if mat.kind == A.RT_MAT_LAMBERTIAN:
        return cosine_about(n, rnd)
    ud = unit(d)
    if mat.kind == A.RT_MAT_METAL:
        k = 2 * dot(ud, n)
        f = in_unit_sphere(rnd)
        out = tuple(ud[i] - k * n[i] + mat.fuzz * f[i] for i in range(3))
        return out if dot(out, n) > 0 else None
    if mat.kind == A.RT_MAT_DIELECTRIC:
        ratio = 1.0 / mat.ir if front else mat.ir
        cos_t = min(-dot(ud, n), 1.0)
        sin_t = math.sqrt(max(0.0, 1.0 - cos_t * cos_t))
        r0 = ((1 - ratio) / (1 + ratio)) ** 2
        if ratio * sin_t > 1.0 or r0 + (1 - r0) * (1 - cos_t) ** 5 > rnd.random():
            k = 2 * dot(ud, n)
            return tuple(ud[i] - k * n[i] for i in range(3))
        perp = tuple(ratio * (ud[i] + cos_t * n[i]) for i in range(3))
        par = -math.sqrt(abs(1.0 - dot(perp, perp)))
        return tuple(perp[i] + par * n[i] for i in range(3))
    return None


def count(pkg, builder, n_paths, seed):
    import elide as E
    A = pkg._abi
    hs = pkg.HostScene("book1", 1)
    desc = hs.desc
    desc.bvh_builder = builder
    full, spheres, meta = pkg.compile_dump(desc, A.RT_LAYOUT_ALL_BOX_NODES)
    dflt, _, _ = pkg.compile_dump(desc, 0)
    kept = E.kept_mask(full, dflt)
    E.check_links(full, dflt, kept)
    first = E.first_spheres(pkg.compile_info(desc, 0))
    mats = [desc.materials[int(m) & META_MAT_MASK] for m in meta]
    walks = (E.Walk(full, spheres, first), E.Walk(dflt, spheres, first))
    cam = hs.camera(1.5)
    v3 = lambda v: (v.x, v.y, v.z)
    org, llc, hor, ver, cu, cv = (v3(x) for x in (cam.origin, cam.lower_left_corner, cam.horizontal, cam.vertical, cam.u, cam.v))
    rnd = random.Random(seed)
    segments, visits, tests = 0, [0, 0], [0, 0]
    for _ in range(n_paths):
        while True:
            lx, ly = rnd.uniform(-1, 1), rnd.uniform(-1, 1)
            if lx * lx + ly * ly < 1:
                break
        off = tuple(cam.lens_radius * (lx * cu[k] + ly * cv[k]) for k in range(3))
        s, t = rnd.random(), rnd.random()
        o = tuple(org[k] + off[k] for k in range(3))
        d = tuple(llc[k] + s * hor[k] + t * ver[k] - org[k] - off[k] for k in range(3))
        for _depth in range(50):
            segments += 1
            got = [w(o, d) for w in walks]
            assert got[0][:2] == got[1][:2], "the two arrays disagree on a hit"
            for k in range(2):
                visits[k] += got[k][2]
                tests[k] += got[k][3]
            tt, hit = got[0][:2]
            if hit < 0:
                break
            p = tuple(o[k] + tt * d[k] for k in range(3))
            c = walks[0].sph[hit]
            n_out = tuple((p[k] - c[k]) / c[3] for k in range(3))
            d = scatter(mats[hit], A, d, n_out, rnd)
            if d is None:
                break
            o = p
    inner = E.inner_records(full)
    return dict(builder="sah" if builder == A.RT_BVH_SAH else "reference", records=int(len(full)), inner_records=int(len(inner)), records_elided=int((~kept).sum()),
                model_cost_all_boxes=round(E.model_cost(full, np.ones(len(full), bool)), 4), model_cost_default=round(E.model_cost(full, kept), 4),
                paths=n_paths, segments_per_path=round(segments / n_paths, 3),
                box_tests_per_segment_all_boxes=round(visits[0] / segments, 3), box_tests_per_segment_default=round(visits[1] / segments, 3),
                box_tests_ratio=round(visits[1] / visits[0], 4),
                sphere_tests_per_segment_all_boxes=round(tests[0] / segments, 3), sphere_tests_per_segment_default=round(tests[1] / segments, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import rta
    pkg = rta.load()
    A = pkg._abi
    rows = [count(pkg, b, args.paths, args.seed) for b in (A.RT_BVH_REFERENCE, A.RT_BVH_SAH)]
    rows[1]["box_tests_sah_over_reference_default"] = round(rows[1]["box_tests_per_segment_default"] / rows[0]["box_tests_per_segment_default"], 4)
    text = "\n".join(json.dumps(r) for r in rows)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
