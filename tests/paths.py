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


def variant_of(pkg, desc):
    need = pkg.compile_info(desc)["features"]
    for name, have in VARIANT_SETS:
        if need & ~have == 0:
            return name
    raise AssertionError(need)


class Built:
    def __init__(self, desc, cam, keep):
        self.desc, self.cam, self.keep = desc, cam, keep


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
    else:
        raise KeyError(name)
    if form == "all":
        more, lamp = _cluster(pkg, b, at, 3.0 if name.startswith("wrap_") else 2.0)
        ids, lights = ids + more, lights + lamp
    elif form != "own":
        raise KeyError(form)
    world = b.hittable_list(ids) if name in ("lights_both", "wrap_translate", "media_inside") else b.bvh(ids, 0.0, 1.0)
    desc = b.desc(world, b.hittable_list(lights) if lights else -1)
    return Built(desc, cam, b), own


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
}
SCENES = list(REQUIRED)
# what the cluster adds to every "all" form
REQUIRED_ALL_FORM = ["hit_triangle", "under_translate", "under_rotate_y", "tex_checker", "medium_scattered", "lambertian_light_sphere"]
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
    base = orc.render_paths(built.desc, built.cam, prm, precision=64, n_threads=threads, count=True)
    same = np.ones(base["segments"].shape, bool)
    lo, hi, margin, tmin = base["radiance"].copy(), base["radiance"].copy(), base["margin"].copy(), base["tmin_margin"].copy()
    for s in SIGNS:
        q = orc.render_paths(built.desc, built.cam, prm, precision=64, n_threads=threads, r_ulps=R_ULPS, signs=s)
        same &= (q["segments"] == base["segments"]) & (q["terminal"] == base["terminal"]) & (q["events"] == base["events"])
        lo, hi, margin = np.minimum(lo, q["radiance"]), np.maximum(hi, q["radiance"]), np.minimum(margin, q["margin"])
        tmin = np.minimum(tmin, q["tmin_margin"])
    size = np.maximum(1.0, np.abs(base["radiance"]).max(axis=-1))
    decidable = same & ((hi - lo).max(axis=-1) <= SPREAD * size) & (margin >= DRAW_MARGIN) & (tmin >= TMIN_MARGIN)
    f32 = orc.render_paths(built.desc, built.cam, prm, precision=32, n_threads=threads)
    _cache[key] = dict(built=built, base=base, decidable=decidable, f32=f32)
    return _cache[key]


def bit(orc, name):
    return orc.EVENTS[name]


def describe(orc, mask):
    return "+".join(n for n in orc.EVENT_NAMES if mask & orc.EVENTS[n]) or "-"
