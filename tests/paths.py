"""Probe scenes for the per-sample shading tests (tests/test_paths_host.py, tests/test_gpu_paths.py): small open scenes, one per family
of shade_segment's branches, each in two forms, rendered at 32 x 24 x 8 samples and max_depth 1, 2, 4 and 8 — and for every sample the
f64 checker's radiance and path record (oracle/binding.py render_paths: segment count, terminal code, event mask, margins), which
samples are DECIDABLE, and the f32 checker's answer.

A sample is decidable when, across the unperturbed f64 run and 8 runs in which every ray the path traces has its direction rounded to
f32 and moved by +-R f32 ulps per component (the 8 sign patterns of tests/rays.py),
  * the segment count, the terminal code and the event mask are the same,
  * the radiances spread by no more than 1e-3 * max(1, |L|) per channel (rays.py's rule on t, on L), and
  * every random-number threshold of the path — |p|^2 < 1 of the rejection samplers, reflectance > draw, the free path against the
    distance inside a medium (relative) — was decided by at least DRAW_MARGIN, and
  * every root a primitive test of the path compared with t_min lies at least TMIN_MARGIN from it, measured as the distance the ray's
    origin would have to move along the surface normal to carry the root across: |root - t_min| * |d . n|.
Everything in the rule comes from the checker at precision 64; neither the device nor the f32 checker takes part in it. An undecidable
sample grazes a silhouette, an edge, a texture boundary or a threshold; an f32 path may leave the f64 one there, and the tests leave it
out, under a cap of 5 % per case (CAP).

DRAW_MARGIN = 1e-5: the f32 uniform is the top 24 bits of the draw the f64 uniform takes 53 of, so the two differ by less than 2^-24 =
6e-8. That moves a reflectance comparison by 6e-8 and |2u - 1|^2 summed over three components by at most 3 * 2 * 2 * 6e-8 = 7e-7, to
which f32 rounding of the sum adds 2e-7; 1e-5 keeps a factor of ten over the larger, and makes 1e-5 of the rejection tests undecidable.
`draw < 0.5` of the mixture needs no margin: the two uniforms share their top bit.

TMIN_MARGIN = 6e-5, from a failure of the rule without it: the f32 checker left the f64 path on 9 decidable samples, all of one kind — a
ray sampled towards a light leaves a sphere pointing slightly INTO it, and the sphere's own far root -2 hb / a (1.4 t_min in the case
traced) is accepted in f64 and lost in f32. The perturbation of the direction moves that root by R * eps = 8e-6 of itself; but the f32 hit
point the ray starts from is off the surface by delta ~ eps * |oc|^2 / r (the error of hb^2 - a * c at the previous hit: 5.6e-6 in that
case; 3e-5 for |oc| = 10 and r = 0.2, the limits of these scenes), which moves the root by delta / |d^ . n|, without bound at a grazing
exit. The margin is that displacement; 6e-5 is twice the largest delta. (The device's sphere_fast and start-primitive rules, DESIGN.md
section 2, remove this error; the f32 checker, which stands in for the device on the CPU, has it.)

RtSceneDesc.scene_flags and triangle attributes (include/rt_hip.h) add three margins, each recorded by the checker at precision 64:
  * LIGHT_EDGE_MARGIN = 1e-4 and LIGHT_COS_MARGIN = 1e-2, the thresholds tests/lights_cases.py uses for single queries. MixturePdf::value is
    called with the direction that was drawn, not with the perturbed one the next segment traces, so the +-R-ulp runs do not see the list's
    pdf jump where that direction passes the edge of a light it does not reach (an occluded one, or one behind the light it was drawn
    from). Every evaluation of the list's pdf against a member of a kind the reference has not (XY and YZ rects, triangles, boxes, anything
    under a wrapper chain) records how far its crossing with the member's plane lies from the member's edge (rects: scene units; triangles:
    barycentrics; near misses count) and |cos| at a member it meets: pdf = t^2 |v|^2 / (|cos| area) loses 1 / |cos| of its digits. A
    crossing between a triangle's edge and that edge moved out by the f32 closed-edge bound (oracle.cpp tri_close_edges with the device's
    unit roundoff) records 0: there the rule answers by precision, a hit in f32 and a miss in f64. The reference's own bare XZ rect and
    sphere lights keep the rule they had.
  * the weighted pick of RT_SCENE_LIGHTS_MANY records min_k |u - cdf_k| into the same margin as the other draws (DRAW_MARGIN).
  * NORMAL_MARGIN = 1e-8: an interpolated normal records | |s|^2 - FLT_MIN | / max_i |w_i n_i|^2 for s = w0 n0 + bu n1 + bv n2. Each
    component of s carries 3 roundings of terms no larger than the largest: |ds| <= 3 * 2^-24 max|w_i n_i| in f32, so the DIRECTION of
    unit(s) is off by 1.8e-7 / (|s| / max|w_i n_i|); at a ratio of 1e-4 (1e-8 squared) that is 1.8e-3 rad, beyond SPREAD, and the +-R-ulp
    runs, which move (bu, bv) and not the rounding of the sum, need not show it. Below it, and on the line itself, which side of FLT_MIN
    the squared length falls is an accident of the arithmetic.

R: rays.py derives 64 ulps from the device's sphere discriminant for |oc| / (4 r) up to 31. The probe scenes keep everything within about
10 units of the origin and radii >= 0.2, so |oc| / (4 r) <= 12.5 < 31: the same R covers them with more room."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays as RAYS  # noqa: E402

R_ULPS = RAYS.R_ULPS
SIGNS = RAYS.SIGNS
DRAW_MARGIN = 1e-5
TMIN_MARGIN = 6e-5
LIGHT_EDGE_MARGIN, LIGHT_COS_MARGIN = 1e-4, 1e-2      # tests/lights_cases.py EDGE_MIN, COS_MIN
NORMAL_MARGIN = 1e-8
SPREAD = 1e-3
CAP = 0.05
COVERAGE = 50                 # decidable samples that must carry each required event bit (at max_depth 8)
W, H, SPP, SEED = 32, 24, 8, 20240917      # W - 1 = 31 is no power of two: the camera's hardware reciprocal is part of what is tested
DEPTHS = (1, 2, 4, 8)
FORMS = ("own", "all")

# ---- which kernel instance a scene runs on -----------------------------------------------------------------------------------------
# The library reports a scene's feature bits (rt_scene_compile_info: RtCompileInfo.features, the F_* of csrc/kernels.h); pick_variant
# (csrc/kernels.hip) runs it on the smallest of four compiled sets that covers them. The rule is restated here; the scenes' expected
# variants are in SCENES below and test_paths_host.py checks them against what the library reports.
F_MOVING, F_RECT, F_TRI, F_MEDIUM, F_XFORM, F_TEX, F_LIGHTS, F_ALL = 1, 2, 4, 8, 16, 32, 64, 127
VARIANT_SETS = (("0", 0), ("mesh", F_RECT | F_TRI), ("box", F_RECT | F_XFORM | F_LIGHTS), ("all", F_ALL))
# ... and the kernels that rebuild a HitRecord and shade have six more instances (with_record_variant, with_shade_variant): triangle attributes
# (128) on the mesh set or the full one; extended light records (256: RT_SCENE_LIGHTS_ALL_SHAPES with a member of a new kind, or
# RT_SCENE_LIGHTS_MANY) and the light tree (512: RT_SCENE_LIGHTS_MANY) always on the full one, each without and with attributes.
F_TRI_ATTR, F_LIGHTS_EXT, F_LIGHTS_TREE = 128, 256, 512
NEW_INSTANCES = ("mesh+attr", "all+attr", "all+lx", "all+attr+lx", "all+lt", "all+attr+lt")


def features_of(pkg, built):
    return pkg.compile_info(built.desc, **(dict(triangle_attrs=built.attrs) if built.attrs is not None else {}))["features"]


def variant_of(pkg, built):
    need = features_of(pkg, built)
    assert need & ~(F_ALL | F_TRI_ATTR | F_LIGHTS_EXT | F_LIGHTS_TREE) == 0 and (not need & F_LIGHTS_TREE or need & F_LIGHTS_EXT), need
    name = "all" if need & F_LIGHTS_EXT else next(n for n, have in VARIANT_SETS if need & F_ALL & ~have == 0)
    if need & F_TRI_ATTR:
        name = ("all" if name != "mesh" else "mesh") + "+attr"
    return name + ("+lt" if need & F_LIGHTS_TREE else "+lx" if need & F_LIGHTS_EXT else "")


class Built:
    def __init__(self, desc, cam, keep, attrs=None):
        self.desc, self.cam, self.keep, self.attrs = desc, cam, keep, attrs      # attrs: the RtTriangleAttrs array that travels beside the desc, or None


def _ico(pkg, b, centre, radius, mat, subdivisions=1):
    """mesh.icosphere about `centre` with sphere normals and the sphere's own (u, v) at its vertices; returns the triangles' ids"""
    tris, nrm = pkg.icosphere(subdivisions)
    uv = pkg.sphere_uv(nrm)
    return [b.triangle(*(radius * tris[k] + np.asarray(centre, float)), mat, normals=nrm[k], uvs=uv[k]) for k in range(len(tris))]


def _lamp_members(pkg, b, lamp):
    """The lights list of `lights_many`: a quad of 2 x 2 at y = 3.2 as 4 x 4 graded cells (32 triangles, areas 0.005 to 0.68), a small sphere
    (2.0), a large box (15.5) and a YZ rect under Translate(RotateY(..)): p_k from 2e-4 to 0.7.
    The sphere's radius is 0.4, the bulbs' of the older scenes, and no less: sphere.rs:75-84 forms pdf = 1 / (2 pi (1 - cos_max)) with
    cos_max = sqrt(1 - r^2 / d^2), and 1 - cos_max = r^2 / (2 d^2) keeps an absolute error of an ulp of 1 (two roundings at 1, 2^-24 each) —
    a relative one of 2^-23 * 2 d^2 / r^2 in f32: 5e-5 at d = 6 for r = 0.4, which the older scenes' figures show, and 2e-4 for r = 0.2.
    (The first device run of this scene had r = 0.2: one decidable sample of smooth_lit, (y, x, s) = (14, 4, 4) at depth 8, whose direction
    met that sphere 3.5 units away, stood 9.8e-5 of its radiance from the f64 checker where the f32 checker stands 2.6e-5 from it — neither
    wrong, both within that bound — and the scene's 101 sphere samples had not shown the f32 checker's own tail.)"""
    import lights_many_cases as LM
    out = [b.triangle(*t, lamp) for t in LM.graded_lamp_triangles(cells=4, y=3.2)]
    out.append(b.sphere((2.8, 1.9, 1.4), 0.4, lamp))
    out.append(b.box((1.8, -0.2, -2.3), (3.6, 1.3, -0.9), lamp))
    out.append(b.translate(b.rotate_y(b.yz_rect(0.0, 1.2, -0.6, 0.6, 0.0, lamp), 25.0), (-3.4, 0.0, -1.2)))
    return out


def _camera(pkg, lookfrom, lookat, vfov=40.0, aperture=0.0, t0=0.0, t1=0.0):
    focus = float(np.linalg.norm(np.array(lookfrom, float) - np.array(lookat, float)))
    return pkg.camera_new(lookfrom, lookat, (0, 1, 0), vfov, W / H, aperture, focus, t0, t1)


def _image():
    return RAYS.earth_image()[::16, ::16]


def _cluster(pkg, b, at, k):
    """"One of everything else": a triangle, a wrapped textured box, a medium and a light for the lights list, within 0.8 k units of
    `at`. Returns (world ids, light ids). It puts a scene on F_ALL whatever else it holds; it may be hit like anything else."""
    x, y, z = at
    grey = b.lambertian((0.6, 0.6, 0.6))
    tri = b.triangle((x - 0.9 * k, y - 0.3 * k, z - 0.5 * k), (x + 0.9 * k, y - 0.3 * k, z - 0.5 * k), (x, y + 1.4 * k, z - 0.5 * k), grey)   # a backdrop
    chk = b.lambertian(texture=b.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))
    box = b.translate(b.rotate_y(b.box((-0.25 * k, -0.25 * k, -0.25 * k), (0.25 * k, 0.25 * k, 0.25 * k), chk), 25.0), (x + 0.3 * k, y - 0.05 * k, z))
    fog = b.constant_medium(b.sphere((x - 0.15 * k, y + 0.85 * k, z), 0.35 * k, b.dielectric(1.5)), 4.0, (0.8, 0.8, 0.9))
    lamp = b.sphere((x + 0.5 * k, y + 0.6 * k, z), 0.2 * k, b.diffuse_light((4.0, 4.0, 3.0)))
    return [tri, box, fog, lamp], [lamp]


def _wrappers(pkg, b, wrap):
    """The five chains of test_gpu_scenes.test_instance_wrappers, over a ground rect of 8 units."""
    g, w, glass = b.lambertian((0.8, 0.3, 0.3)), b.lambertian((0.73,) * 3), b.dielectric(1.5)
    inner = b.hittable_list([b.box((-1, -1, -1), (1, 1.5, 1), w), b.sphere((2.5, 0, 0), 1.0, glass), b.sphere((-2.5, 0, 0.5), 0.9, g)])
    obj = {"translate": lambda: b.translate(inner, (1, 0.5, -2)),
           "rotate": lambda: b.rotate_y(inner, 30),
           "both": lambda: b.translate(b.rotate_y(inner, 30), (1, 0.5, -2)),
           "flip_both": lambda: b.flip_face(b.translate(b.rotate_y(inner, -40), (0, 0.5, -1))),
           "double_rotate": lambda: b.rotate_y(b.translate(b.rotate_y(inner, 20), (1, 0, 0)), 25)}[wrap]()
    return [obj, b.xz_rect(-8, 8, -8, 8, -1.5, g)]


def build_scene(pkg, name, form):
    """(Built, expected variant of the "own" form). The "all" form adds _cluster and runs on F_ALL."""
    A = pkg._abi
    sky = dict(background=(0.5, 0.7, 1.0), background_mode=A.RT_BG_SKY_GRADIENT)
    rng = np.random.default_rng(11)
    lights, cam, at = [], None, (2.6, 1.2, 0.5)
    if name in ("glass", "glass_inside"):
        # spheres only: solid, hollow (negative inner radius) and one with ir < 1 (cannot refract from OUTSIDE); the second view has the
        # camera inside the solid one
        b = pkg.SceneBuilder(**sky)
        gl = b.dielectric(1.5)
        ids = [b.sphere((0, -8.5, 0), 8.0, b.lambertian((0.5, 0.5, 0.5))), b.sphere((-1.8, 0.3, 0), 0.8, gl),
               b.sphere((0, 0.3, 0), 0.8, gl), b.sphere((0, 0.3, 0), -0.7, gl), b.sphere((1.8, 0.3, 0), 0.8, b.dielectric(0.7)),
               b.sphere((0.9, 0.0, -1.8), 0.5, b.lambertian((0.7, 0.3, 0.3))), b.sphere((-0.9, 0.0, 1.6), 0.5, b.lambertian((0.2, 0.4, 0.8)))]
        cam = _camera(pkg, (0, 1.5, 7), (0, 0.2, 0), 40.0) if name == "glass" else _camera(pkg, (-1.8, 0.4, 0.3), (1.0, 0.2, -0.5), 70.0)
        at = (2.2, 1.6, 1.0) if name == "glass" else (0.6, 0.9, -0.8)
        own = "0"
    elif name == "glass_mesh":
        b = pkg.SceneBuilder(**sky)
        gl = b.dielectric(1.5)
        ids = [b.xz_rect(-8, 8, -8, 8, -0.5, b.lambertian((0.5, 0.5, 0.5))), b.box((-2.4, -0.5, -0.6), (-1.0, 0.9, 0.6), gl),
               b.triangle((-0.6, -0.4, 0.4), (1.0, -0.4, 0.0), (0.2, 1.4, 0.2), gl), b.sphere((2.0, 0.3, 0), 0.8, gl),
               b.sphere((0.3, 0.0, -1.6), 0.5, b.lambertian((0.7, 0.3, 0.3)))]
        cam = _camera(pkg, (0.5, 1.8, 7), (0, 0.2, 0), 40.0)
        at = (2.4, 1.7, 1.0)
        own = "mesh"
    elif name == "metal":
        # fuzz 0, 0.3 and 1 on spheres and rects; a MOVING metal sphere beside a moving diffuse one (Metal::scatter resets the ray's time to 0)
        b = pkg.SceneBuilder(**sky)
        ids = [b.xz_rect(-8, 8, -8, 8, -0.5, b.metal((0.8, 0.8, 0.8), 0.3)),
               b.sphere((-2.0, 0.2, 0), 0.7, b.metal((0.9, 0.6, 0.3), 0.0)), b.sphere((-0.5, 0.2, 0), 0.7, b.metal((0.7, 0.8, 0.9), 0.3)),
               b.sphere((1.0, 0.2, 0), 0.7, b.metal((0.8, 0.8, 0.8), 1.0)), b.xy_rect(-3, 3, -0.5, 2.5, -2.0, b.metal((0.9, 0.9, 0.9), 0.0)),
               b.yz_rect(-0.5, 2.0, -2.0, 1.5, -3.2, b.metal((0.6, 0.9, 0.6), 1.0)),
               b.moving_sphere((2.4, 0.0, 0.6), (2.4, 0.5, 0.6), 0.0, 1.0, 0.5, b.metal((0.9, 0.9, 0.5), 0.1)),
               b.moving_sphere((1.6, -0.1, 1.6), (1.9, 0.2, 1.6), 0.0, 1.0, 0.4, b.lambertian((0.7, 0.2, 0.2)))]
        cam = _camera(pkg, (1.0, 2.0, 7), (0, 0.3, 0), 40.0, t0=0.0, t1=1.0)
        at = (-2.4, 1.0, 1.6)
        own = "all"
    elif name in ("lights_both", "lights_rect", "lights_sphere", "lights_none", "lights_default"):
        if name == "lights_none":
            # Lambertian spheres and no lights list: CosinePdf alone
            b = pkg.SceneBuilder(**sky)
            ids = [b.sphere((0, -8.5, 0), 8.0, b.lambertian((0.5, 0.5, 0.5)))]
            ids += [b.sphere((-1.6 + 1.6 * k, 0.2, 0.3 * k), 0.7, b.lambertian(c)) for k, c in enumerate([(0.8, 0.3, 0.3), (0.3, 0.8, 0.3), (0.3, 0.3, 0.8)])]
            own = "0"
        else:
            b = pkg.SceneBuilder(background=(0.3, 0.4, 0.5))
            if name == "lights_default":      # (no flat Lambertian here: (1, 0, 0) from a point of an axis-aligned rect runs in the rect's plane)
                ids = [b.sphere((0, -8.5, 0), 8.0, b.metal((0.6, 0.6, 0.6), 0.2))]     # (nor a large Lambertian: (1, 0, 0) grazes a wide band of it)
            else:
                ids = [b.xz_rect(-8, 8, -8, 8, -0.5, b.lambertian((0.6, 0.6, 0.6))), b.xy_rect(-4, 4, -0.5, 3.5, -2.5, b.lambertian((0.7, 0.5, 0.3)))]
            ids += [b.sphere((-1.6 + 1.6 * k, 0.2, 0.3 * k), 0.7, b.lambertian(c)) for k, c in enumerate([(0.8, 0.3, 0.3), (0.3, 0.8, 0.3), (0.3, 0.3, 0.8)])]
            if name == "lights_default":
                # an xy-rect in the lights list has the trait defaults (pdf_value 0, random (1, 0, 0), hittable.rs:54-59): where the light
                # half is chosen and (1, 0, 0) points below the surface, both pdfs are 0 and the sample is 0 * L / 0 = NaN
                wall = b.xy_rect(-1.0, 1.0, 0.5, 2.5, -2.0, b.diffuse_light((6.0, 6.0, 6.0)))
                ids.append(wall); lights.append(wall)
            elif name != "lights_sphere":
                panel = b.xz_rect(-1.0, 1.0, -0.5, 1.5, 3.0, b.diffuse_light((6.0, 6.0, 6.0)))
                ids.append(b.flip_face(panel)); lights.append(panel)
            if name not in ("lights_rect", "lights_default"):
                bulb = b.sphere((2.6, 1.6, 1.0), 0.4, b.diffuse_light((5.0, 4.0, 3.0)))
                ids.append(bulb); lights.append(bulb)
            own = "box"
        cam = _camera(pkg, (0.5, 2.0, 7.5), (0, 0.6, 0), 40.0)
        at = (-2.6, 1.7, 1.0)
    elif name in ("textures", "textures_wrapped"):
        # checker, nested checker, noise, image and the empty image, as Lambertian albedos and as a DiffuseLight's colour, on a sphere, a
        # rect, a triangle and a moving sphere; `textures_wrapped` holds the same things under translate(rotate_y(...))
        b = pkg.SceneBuilder(background=(0.8, 0.8, 0.8))
        chk = b.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))
        noise, img, empty = b.noise(4.0, rng), b.image(_image()), b.image(None)
        nested = b.checker_textures(b.checker_textures(noise, b.solid_color((0.9, 0.1, 0.1))), img)
        inner = [b.sphere((-2.0, 0.3, 0), 0.8, b.lambertian(texture=noise)), b.sphere((0.0, 0.3, 0), 0.8, b.lambertian(texture=img)),
                 b.sphere((2.0, 0.3, 0), 0.8, b.lambertian(texture=chk)), b.sphere((-1.0, 0.0, 1.6), 0.5, b.lambertian(texture=empty)),
                 b.xy_rect(-3, 3, -0.5, 2.5, -1.5, b.lambertian(texture=nested)),
                 b.triangle((0.6, -0.4, 1.8), (2.2, -0.4, 1.4), (1.4, 0.8, 1.6), b.lambertian(texture=noise)),
                 b.moving_sphere((1.0, 1.6, 0.0), (1.0, 1.9, 0.0), 0.0, 1.0, 0.45, b.lambertian(texture=img)),
                 b.sphere((-1.2, 1.7, 0.0), 0.45, b._mat(A.RT_MAT_DIFFUSE_LIGHT, chk)),
                 b.xz_rect(-4, 4, -3, 3, -0.5, b.lambertian(texture=chk))]
        if name == "textures":
            ids = inner
        else:
            ids = [b.translate(b.rotate_y(b.hittable_list(inner), 20.0), (0.3, 0.2, -0.4))]
        cam = _camera(pkg, (0.4, 1.6, 6), (0, 0.6, 0), 52.0, t0=0.0, t1=1.0)
        at = (-3.0, 1.9, 0.8)
        own = "all"
    elif name in ("media", "media_inside"):
        # Isotropic media: a dense one (2) bounded by a sphere, a thin one (0.05) by a rotated, translated box, and one inside a glass sphere
        b = pkg.SceneBuilder(**sky)
        ids = [b.xz_rect(-8, 8, -8, 8, -0.5, b.lambertian((0.5, 0.5, 0.5))),
               b.constant_medium(b.sphere((-1.8, 0.5, 0), 1.0, b.dielectric(1.5)), 2.0, (0.9, 0.9, 0.9)),
               b.constant_medium(b.translate(b.rotate_y(b.box((-0.9, -0.5, -0.9), (0.9, 1.3, 0.9), b.dielectric(1.5)), 30.0), (0.6, 0.0, -0.3)), 0.05, (0.2, 0.4, 0.9)),
               b.sphere((2.6, 0.4, 0.4), 0.9, b.dielectric(1.5)),
               b.constant_medium(b.sphere((2.6, 0.4, 0.4), 0.75, b.dielectric(1.5)), 1.5, (0.9, 0.3, 0.3))]
        cam = _camera(pkg, (0.5, 1.8, 7.5), (0.3, 0.3, 0), 40.0) if name == "media" else _camera(pkg, (-1.8, 0.6, 0.2), (1.5, 0.3, 0.0), 70.0)
        at = (0.4, 2.3, 0.6) if name == "media" else (0.4, 1.9, 0.9)
        own = "all"
    elif name.startswith("wrap_"):
        b = pkg.SceneBuilder(background=(0.7, 0.8, 1.0))
        ids = _wrappers(pkg, b, name[5:])
        cam = _camera(pkg, (0, 3, 10), (0, 0, -1), 45.0)
        at = (-3.0, 2.6, 1.5)
        own = "box"
    elif name == "rotated_sphere":
        # rays.py's: a sphere under a lone RotateY (hittable.rs:173 tests the CHILD-space ray against the rotated-back normal)
        b = pkg.SceneBuilder(**sky)
        ids = [b.rotate_y(b.sphere((1.0, 0.6, 0.3), 0.6, b.lambertian((0.8, 0.3, 0.3))), 65.0),
               b.rotate_y(b.sphere((-1.2, 0.5, -0.4), 0.5, b.dielectric(1.5)), -130.0), b.xz_rect(-5, 5, -5, 5, 0.0, b.lambertian((0.5, 0.5, 0.5)))]
        cam = _camera(pkg, (3.0, 2.0, 6.0), (0.0, 0.5, 0.0), 30.0)
        at = (-1.0, 0.9, 1.2)
        own = "box"
    elif name == "camera":
        # aperture > 0 and time0 < time1 over moving spheres
        b = pkg.SceneBuilder(**sky)
        ids = [b.sphere((0, -8.5, 0), 8.0, b.lambertian((0.5, 0.5, 0.5)))]
        for k in range(5):
            c = np.array([-2.4 + 1.2 * k, 0.1 + 0.1 * k, -1.0 + 0.5 * k])
            ids.append(b.moving_sphere(c, c + np.array([0.0, 0.4, 0.1 * k]), 0.0, 1.0, 0.5, b.lambertian(rng.uniform(0.2, 0.9, 3)) if k & 1 else b.metal((0.8, 0.8, 0.8), 0.1)))
        ids.append(b.sphere((0.0, 0.3, 1.8), 0.6, b.dielectric(1.5)))
        cam = _camera(pkg, (0, 1.5, 7), (0, 0.2, 0), 40.0, aperture=0.3, t0=0.0, t1=1.0)
        at = (2.4, 1.7, 1.0)
        own = "all"
    elif name in ("lights_shapes", "lights_shapes_wrapped", "lights_many", "lights_many_padded", "lights_many_one", "lights_many_two", "smooth_lit", "smooth_lit_many"):
        # RtSceneDesc.scene_flags: Lambertian receivers (a floor, a back wall, three spheres) under a lights list of the new kinds; every
        # member is emissive and is in the world too (but the 1e-6 member of lights_many_two, which nothing could see)
        b = pkg.SceneBuilder(background=(0.3, 0.4, 0.5))
        lamp = b.diffuse_light((5.0, 5.0, 4.0))
        ids = [b.xz_rect(-8, 8, -8, 8, -0.5, b.lambertian((0.6, 0.6, 0.6))), b.xy_rect(-4, 4, -0.5, 3.5, -2.5, b.lambertian((0.7, 0.5, 0.3)))]
        if name.startswith("smooth_lit"):
            ids.append(b.bvh(_ico(pkg, b, (0.0, 0.5, 0.2), 1.0, b.lambertian((0.8, 0.4, 0.3)))))
        else:
            ids += [b.sphere((-1.6 + 1.6 * k, 0.2, 0.3 * k), 0.7, b.lambertian(c)) for k, c in enumerate([(0.8, 0.3, 0.3), (0.3, 0.8, 0.3), (0.3, 0.3, 0.8)])]
        in_world = None
        if name == "lights_shapes":          # unequal sizes: 1.5, 2.25, 2.9, 7.6 and 2.0 square units
            lights = [b.xy_rect(-3.2, -1.7, 1.4, 2.4, -1.2, lamp), b.yz_rect(0.4, 1.9, -1.0, 0.5, 3.3, lamp),
                      b.triangle((-0.8, 3.0, -0.6), (1.0, 3.3, 0.2), (0.0, 2.8, 1.5), lamp), b.box((1.4, 1.6, -2.0), (2.7, 2.5, -0.8), lamp),
                      b.sphere((2.8, 1.3, 1.2), 0.4, lamp)]
        elif name == "lights_shapes_wrapped":
            lights = [b.translate(b.rotate_y(b.xy_rect(-0.8, 0.7, -0.5, 0.5, 0.0, lamp), 35.0), (-0.9, 2.4, -1.7)),
                      b.flip_face(b.translate(b.triangle((-0.8, 0.0, -0.6), (1.0, 0.3, 0.2), (0.0, -0.2, 1.5), lamp), (0.2, 3.0, 0.0))),
                      b.rotate_y(b.box((1.7, 1.9, -1.5), (2.4, 2.4, -0.8), lamp), 20.0),
                      b.rotate_y(b.translate(b.rotate_y(b.sphere((0.5, 0.0, 0.0), 0.4, lamp), 40.0), (-3.0, 1.6, 0.4)), -25.0),
                      b.xz_rect(2.2, 3.4, 0.2, 1.4, 2.9, lamp)]
        elif name == "lights_many_one":
            lights = [b.triangle((-0.8, 3.0, -0.6), (1.0, 3.3, 0.2), (0.0, 2.8, 1.5), lamp)]
        elif name == "lights_many_two":      # areas 4 and 4e-6: p = (1 - 1e-6, 1e-6) and cdf = (1 - 1e-6, 1) as floats
            lights = [b.xz_rect(-1.0, 1.0, -1.0, 1.0, 3.2, lamp), b.triangle((2.0, 3.0, 0.0), (2.0 + 8.0 ** 0.5 * 1e-3, 3.0, 0.0), (2.0, 3.0, 8.0 ** 0.5 * 1e-3), lamp)]
            in_world = lights[:1]
        else:
            lights = _lamp_members(pkg, b, lamp)
        ids += lights if in_world is None else in_world
        if name == "lights_many_padded":     # lights_many with PADDING Lambertian spheres behind the camera, which no camera ray sees (test_gpu_paths.py)
            grey = b.lambertian((0.5, 0.5, 0.5))
            ids += [b.sphere((x, y, z), 0.2, grey) for x, y, z in np.random.default_rng(3).uniform((-6.0, 0.0, 8.5), (6.0, 6.0, 10.5), (PADDING, 3))]
        cam = _camera(pkg, (0.5, 2.0, 7.5), (0, 0.6, 0), 40.0)
        at = (-2.6, 1.7, 1.0)
        flags = dict(lights_all_shapes=True, lights_many=name.startswith("lights_many") or name == "smooth_lit_many")
        own = {"lights_shapes": "all+lx", "lights_shapes_wrapped": "all+lx", "smooth_lit": "all+attr+lx", "smooth_lit_many": "all+attr+lt"}.get(name, "all+lt")
    elif name == "smooth_mesh":
        # triangle attributes on every material that reads the normal: the subdivision-1 icosphere three times, each with sphere normals and
        # the sphere's (u, v) — Lambertian under the image texture, glass under Translate(RotateY(..)), metal under FlipFace — beside a plain
        # triangle and one whose record has flags 0
        b = pkg.SceneBuilder(**sky)
        grey = b.lambertian((0.5, 0.5, 0.5))
        plain = b.triangle((-3.4, -0.4, -1.6), (-1.6, -0.4, -2.2), (-2.6, 1.6, -1.9), b.lambertian((0.7, 0.3, 0.3)))
        inert = b.triangle((1.4, -0.4, -2.2), (3.4, -0.4, -1.6), (2.4, 1.6, -1.9), b.lambertian((0.3, 0.7, 0.3)))
        b.tri_attrs.append(A.RtTriangleAttrs(inert, 0))
        ids = [b.xz_rect(-8, 8, -8, 8, -0.5, grey), plain, inert,
               b.bvh(_ico(pkg, b, (-2.0, 0.4, 0.0), 0.9, b.lambertian(texture=b.image(_image())))),
               b.translate(b.rotate_y(b.bvh(_ico(pkg, b, (0.0, 0.0, 0.0), 0.9, b.dielectric(1.5))), 25.0), (0.1, 0.4, 0.3)),
               b.flip_face(b.bvh(_ico(pkg, b, (2.1, 0.4, 0.0), 0.9, b.metal((0.8, 0.8, 0.9), 0.0))))]
        cam = _camera(pkg, (0.4, 1.6, 7), (0, 0.3, 0), 40.0)
        at = (0.2, 2.4, 1.2)
        own = "all+attr"
    elif name == "smooth_cancel":
        # vertex normals a, -a, a: the sum (w0 - bu + bv) a cancels on the line bu = 1 / 2, which runs through the middle of the frame; beside
        # it the normal is +-a. A second triangle carries normals of lengths 3, 0.2 and 40.
        b = pkg.SceneBuilder(**sky)
        a = (0.2, 0.3, 1.0)
        ids = [b.xz_rect(-8, 8, -8, 8, -0.5, b.lambertian((0.5, 0.5, 0.5))),
               b.triangle((-2.6, -0.4, 0.0), (2.6, -0.4, 0.0), (0.0, 2.6, -0.6), b.lambertian((0.8, 0.6, 0.3)), normals=(a, tuple(-x for x in a), a)),
               b.triangle((-3.2, -0.4, 1.6), (-1.2, -0.4, 2.0), (-2.4, 0.9, 1.4), b.lambertian((0.3, 0.5, 0.8)),
                          normals=((0.6, 0.0, 2.94), (-0.04, 0.08, 0.18), (0.0, 16.0, 36.7)), uvs=((0.1, 0.2), (0.9, 0.3), (0.4, 0.8)))]
        cam = _camera(pkg, (0.0, 1.4, 7), (0, 0.8, 0), 40.0)
        at = (2.4, 1.6, 1.2)
        own = "mesh+attr"
    else:
        raise KeyError(name)
    if not name.startswith(("lights_shapes", "lights_many", "smooth_lit")):
        flags = {}
    if form == "all":
        more, lamp = _cluster(pkg, b, at, 3.0 if name.startswith("wrap_") else 2.0)
        ids, lights = ids + more, lights + lamp
    elif form != "own":
        raise KeyError(form)
    world = b.hittable_list(ids) if name in ("lights_both", "wrap_translate", "media_inside") else b.bvh(ids, 0.0, 1.0)
    desc = b.desc(world, b.hittable_list(lights) if lights else -1, **flags)
    return Built(desc, cam, b, b.triangle_attrs()), own


# ---- scene -> the event bits it is meant to exercise: each on at least COVERAGE decidable samples at max_depth 8, in both forms ----------
# (lambertian_cosine_only is asked of the "own" form only: the cluster's lamp gives the "all" form a lights list, and with one every
# Lambertian bounce samples the mixture.)
_GLASS = ["dielectric_refract", "dielectric_reflect_schlick", "dielectric_reflect_cannot_refract", "dielectric_back_face"]
_WRAP = ["hit_box_side", "hit_sphere", "hit_rect", "dielectric_refract", "lambertian_cosine_only"]
REQUIRED = {
    "glass": _GLASS + ["hit_sphere", "lambertian_cosine_only", "tex_solid"],
    "glass_inside": _GLASS + ["hit_sphere"],
    "glass_mesh": _GLASS + ["hit_box_side", "hit_triangle", "hit_rect", "hit_sphere"],
    "metal": ["metal", "hit_sphere", "hit_rect", "hit_moving_sphere", "time", "lambertian_cosine_only"],
    "lights_both": ["lambertian_light_xz_rect", "lambertian_light_sphere", "lambertian_mixture_cosine", "under_flip_face", "hit_rect", "hit_sphere"],
    "lights_rect": ["lambertian_light_xz_rect", "lambertian_mixture_cosine", "under_flip_face"],
    "lights_sphere": ["lambertian_light_sphere", "lambertian_mixture_cosine"],
    "lights_none": ["lambertian_cosine_only", "hit_sphere"],
    "lights_default": ["lambertian_mixture_cosine", "hit_rect"],
    "textures": ["tex_solid", "tex_checker", "tex_noise", "tex_image", "tex_empty_image", "hit_sphere", "hit_rect", "hit_triangle", "hit_moving_sphere", "time"],
    "textures_wrapped": ["tex_solid", "tex_checker", "tex_noise", "tex_image", "tex_empty_image", "hit_sphere", "hit_rect", "hit_triangle", "hit_moving_sphere",
                         "under_translate", "under_rotate_y"],
    "media": ["isotropic", "medium_scattered", "medium_passed", "dielectric_refract", "dielectric_back_face"],
    "media_inside": ["isotropic", "medium_scattered", "medium_passed"],
    "wrap_translate": _WRAP + ["under_translate"],
    "wrap_rotate": _WRAP + ["under_rotate_y"],
    "wrap_both": _WRAP + ["under_translate", "under_rotate_y"],
    "wrap_flip_both": _WRAP + ["under_translate", "under_rotate_y", "under_flip_face"],
    "wrap_double_rotate": _WRAP + ["under_translate", "under_rotate_y"],
    "rotated_sphere": ["under_rotate_y", "hit_sphere", "dielectric_refract", "lambertian_cosine_only"],
    "camera": ["lens_offset", "time", "hit_moving_sphere", "metal", "lambertian_cosine_only"],
    # RtSceneDesc.scene_flags and triangle attributes
    "lights_shapes": ["lambertian_light_xy_yz_rect", "lambertian_light_triangle", "lambertian_light_box", "lambertian_light_sphere", "lambertian_mixture_cosine"],
    "lights_shapes_wrapped": ["lambertian_light_wrapped", "lambertian_light_xy_yz_rect", "lambertian_light_triangle", "lambertian_light_box",
                              "lambertian_light_sphere", "lambertian_light_xz_rect", "under_flip_face", "under_rotate_y", "under_translate"],
    "lights_many": ["lambertian_light_cdf_pick", "lambertian_light_triangle", "lambertian_light_box", "lambertian_light_sphere", "lambertian_light_wrapped",
                    "lambertian_mixture_cosine"],
    "lights_many_one": ["lambertian_light_cdf_pick", "lambertian_light_triangle"],
    "lights_many_two": ["lambertian_light_cdf_pick", "lambertian_light_xz_rect"],
    "smooth_mesh": ["normal_interpolated", "uv_interpolated", "tex_image", "dielectric_refract", "metal", "hit_triangle",
                    "under_translate", "under_rotate_y", "under_flip_face"],
    "smooth_cancel": ["normal_interpolated", "uv_interpolated", "hit_triangle"],
    "smooth_lit": ["normal_interpolated", "lambertian_light_triangle", "lambertian_light_box"],
    "smooth_lit_many": ["normal_interpolated", "lambertian_light_cdf_pick", "lambertian_light_triangle", "lambertian_light_box"],
}
# normal_fallback (the vertex normals cancel: |sum|^2 below FLT_MIN) is taken on a set of measure zero — the sum of three unit vectors with
# weights of a point INSIDE a triangle vanishes on a line at most, and a ray meets a line only by an accident of rounding — so no render can
# be asked for COVERAGE samples of it. smooth_cancel is there for the samples BESIDE the line (NORMAL_MARGIN); the branch itself is held by
# known answers on rays aimed at points where the sum is exactly 0 (tests/test_oracle_kat.py, tests/test_mesh_attrs_host.py).
MEASURE_ZERO = ["normal_fallback"]
SCENES = list(REQUIRED)
# what the cluster adds to every "all" form
REQUIRED_ALL_FORM = ["hit_triangle", "under_translate", "under_rotate_y", "tex_checker", "medium_scattered", "lambertian_light_sphere"]
PADDING = 512
CASES = [(s, f, d) for s in SCENES for f in FORMS for d in DEPTHS]

# ---- the f32 checker against the f64 checker on decidable samples: worst |L32 - L64| / max(1, |L64|) over the four depths, per scene and
# form, as measured on the CPU (test_paths_host.py prints them; DESIGN.md section 2 has the table). The GPU test allows 2 x the figure.
MEASURED_F32_ORACLE = {
    ("glass", "own"): 5.89e-05,
    ("glass", "all"): 6.29e-05,
    ("glass_inside", "own"): 6.02e-06,
    ("glass_inside", "all"): 3.69e-06,
    ("glass_mesh", "own"): 7.63e-06,
    ("glass_mesh", "all"): 7.63e-06,
    ("metal", "own"): 2.56e-04,
    ("metal", "all"): 2.56e-04,
    ("lights_both", "own"): 4.57e-05,
    ("lights_both", "all"): 5.76e-05,
    ("lights_rect", "own"): 3.06e-05,
    ("lights_rect", "all"): 4.57e-05,
    ("lights_sphere", "own"): 9.48e-06,
    ("lights_sphere", "all"): 1.49e-05,
    ("lights_none", "own"): 1.38e-05,
    ("lights_none", "all"): 2.25e-05,
    ("lights_default", "own"): 8.99e-06,
    ("lights_default", "all"): 1.20e-05,
    ("textures", "own"): 5.64e-05,
    ("textures", "all"): 4.65e-05,
    ("textures_wrapped", "own"): 1.04e-04,
    ("textures_wrapped", "all"): 7.84e-05,
    ("media", "own"): 6.90e-06,
    ("media", "all"): 6.90e-06,
    ("media_inside", "own"): 2.47e-06,
    ("media_inside", "all"): 4.10e-06,
    ("wrap_translate", "own"): 1.21e-05,
    ("wrap_translate", "all"): 1.59e-05,
    ("wrap_rotate", "own"): 6.62e-06,
    ("wrap_rotate", "all"): 8.84e-06,
    ("wrap_both", "own"): 8.76e-06,
    ("wrap_both", "all"): 1.60e-05,
    ("wrap_flip_both", "own"): 1.32e-05,
    ("wrap_flip_both", "all"): 1.91e-05,
    ("wrap_double_rotate", "own"): 9.42e-06,
    ("wrap_double_rotate", "all"): 1.72e-05,
    ("rotated_sphere", "own"): 3.97e-05,
    ("rotated_sphere", "all"): 7.24e-05,
    ("camera", "own"): 5.78e-05,
    ("camera", "all"): 7.84e-05,
    ("lights_shapes", "own"): 7.37e-05,
    ("lights_shapes", "all"): 5.56e-05,
    ("lights_shapes_wrapped", "own"): 2.48e-05,
    ("lights_shapes_wrapped", "all"): 4.83e-05,
    ("lights_many", "own"): 5.85e-05,
    ("lights_many", "all"): 6.37e-05,
    ("lights_many_one", "own"): 1.52e-05,
    ("lights_many_one", "all"): 3.11e-05,
    ("lights_many_two", "own"): 7.09e-05,
    ("lights_many_two", "all"): 1.05e-04,
    ("smooth_mesh", "own"): 3.67e-06,
    ("smooth_mesh", "all"): 7.83e-06,
    ("smooth_cancel", "own"): 4.56e-06,
    ("smooth_cancel", "all"): 8.93e-07,
    ("smooth_lit", "own"): 8.72e-06,
    ("smooth_lit", "all"): 1.44e-05,
    ("smooth_lit_many", "own"): 1.70e-05,
    ("smooth_lit_many", "all"): 7.13e-06,
}

_cache = {}
_scenes = {}


def scene(pkg, name, form):
    if (name, form) not in _scenes:
        _scenes[(name, form)] = build_scene(pkg, name, form)
    return _scenes[(name, form)]


def params(pkg, depth, spp=SPP, **kw):
    return pkg.make_params(W, H, spp, max_depth=depth, seed=SEED, **kw)


def deviation(L, L64):
    """|L - L64| / max(1, |L64|) per sample (the largest channel)."""
    return np.abs(L - L64).max(axis=-1) / np.maximum(1.0, np.abs(L64).max(axis=-1))


def decide(pkg, orc, name, form, depth, threads=8):
    """dict(built, base, decidable, f32) for one case, computed once per process: `base` is the unperturbed f64 run (render_paths' dict),
    `decidable` a bool array (H, W, SPP), `f32` the precision-32 run."""
    key = (name, form, depth)
    if key in _cache:
        return _cache[key]
    built, _ = scene(pkg, name, form)
    prm = params(pkg, depth)
    base = orc.render_paths(built.desc, built.cam, prm, precision=64, n_threads=threads, count=True, attrs=built.attrs)
    same = np.ones(base["segments"].shape, bool)
    lo, hi, margin, tmin = base["radiance"].copy(), base["radiance"].copy(), base["margin"].copy(), base["tmin_margin"].copy()
    more = {k: base[k].copy() for k in ("light_edge", "light_cos", "normal_margin")}
    for s in SIGNS:
        q = orc.render_paths(built.desc, built.cam, prm, precision=64, n_threads=threads, r_ulps=R_ULPS, signs=s, attrs=built.attrs)
        more = {k: np.minimum(v, q[k]) for k, v in more.items()}
        same &= (q["segments"] == base["segments"]) & (q["terminal"] == base["terminal"]) & (q["events"] == base["events"])
        lo, hi, margin = np.minimum(lo, q["radiance"]), np.maximum(hi, q["radiance"]), np.minimum(margin, q["margin"])
        tmin = np.minimum(tmin, q["tmin_margin"])
    size = np.maximum(1.0, np.abs(base["radiance"]).max(axis=-1))
    decidable = same & ((hi - lo).max(axis=-1) <= SPREAD * size) & (margin >= DRAW_MARGIN) & (tmin >= TMIN_MARGIN)
    decidable &= (more["light_edge"] >= LIGHT_EDGE_MARGIN) & (more["light_cos"] >= LIGHT_COS_MARGIN) & (more["normal_margin"] >= NORMAL_MARGIN)
    f32 = orc.render_paths(built.desc, built.cam, prm, precision=32, n_threads=threads, attrs=built.attrs)
    _cache[key] = dict(built=built, base=base, decidable=decidable, f32=f32)
    return _cache[key]


def all_form_variant(own):
    """the instance the "all" form of a scene runs on: the full set, with what the scene's own instance carries beyond the seven old bits"""
    return "all" + (own[own.index("+"):] if "+" in own else "")


# the feature bits 128 / 256 / 512 (RtCompileInfo.features) each new scene is meant to report, in either form
NEW_FEATURES = {"lights_shapes": F_LIGHTS_EXT, "lights_shapes_wrapped": F_LIGHTS_EXT, "lights_many": F_LIGHTS_EXT | F_LIGHTS_TREE,
                "lights_many_one": F_LIGHTS_EXT | F_LIGHTS_TREE, "lights_many_two": F_LIGHTS_EXT | F_LIGHTS_TREE, "smooth_mesh": F_TRI_ATTR,
                "smooth_cancel": F_TRI_ATTR, "smooth_lit": F_TRI_ATTR | F_LIGHTS_EXT, "smooth_lit_many": F_TRI_ATTR | F_LIGHTS_EXT | F_LIGHTS_TREE}


def bit(orc, name):
    return orc.EVENTS[name]


def describe(orc, mask):
    return "+".join(n for n in orc.EVENT_NAMES if mask & orc.EVENTS[n]) or "-"
