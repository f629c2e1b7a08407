"""Shading on the GPU, sample by sample (tests/paths.py): every DECIDABLE sample of the probe scenes — each scene in its own kernel
variant and on F_ALL, at max_depth 1, 2, 4 and 8 — against the f64 checker, with no share allowed; the segment counter; the NaN
policies; and the carriers (wavefront, drain kernel, fused kernel) and device layouts bit for bit against each other.

The tolerance of a scene is 2 x the worst figure of the f32 CHECKER on its decidable samples (paths.MEASURED_F32_ORACLE, measured on the
CPU): the factor the parity tests here use for ocml against libm, FMA contraction and the hardware reciprocal in fdiv. Nothing in it
comes from the device, whose own worst figure is recorded (record_metric) and tabled in DESIGN.md section 2."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paths as P  # noqa: E402

pytestmark = pytest.mark.gpu

_uploaded = {}


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for scene in _uploaded.values():
        scene.close()
    _uploaded.clear()


def uploaded(pkg, gpu, name, form, layout=0):
    key = (name, form, layout)
    if key not in _uploaded:
        built, _ = P.scene(pkg, name, form)
        _uploaded[key] = gpu.upload(built.desc, layout, **(dict(triangle_attrs=built.attrs) if built.attrs is not None else {}))
    return _uploaded[key]


def device_samples(pkg, gpu, scene, cam, depth, **kw):
    """(radiance float32 (H, W, SPP, 3), segments per pass): sample s of the frame is the lone pass [s, s + 1) of SPP."""
    out = np.zeros((P.H, P.W, P.SPP, 3), np.float32)
    segs = []
    prm = P.params(pkg, depth, spp=1, **kw)
    for s in range(P.SPP):
        img, _, st = gpu.render_pass(scene, cam, prm, s, P.SPP, False)
        assert st["samples"] == P.W * P.H
        out[:, :, s] = img
        segs.append(int(st["segments"]))
    return out, segs


@pytest.mark.parametrize("name,form,depth", P.CASES)
def test_every_decidable_sample_agrees_with_the_checker(pkg, orc, gpu, name, form, depth):
    from conftest import record_metric
    c = P.decide(pkg, orc, name, form, depth)
    dec, base = c["decidable"], c["base"]
    L, segs = device_samples(pkg, gpu, uploaded(pkg, gpu, name, form), c["built"].cam, depth)
    # ---- default NaN policy: a sample the checker calls non-finite is 0, everything is finite ----
    assert np.isfinite(L).all()
    nonfinite = dec & (base["terminal"] == orc.TERM_NONFINITE)
    assert not L[nonfinite].any(), f"{int((L[nonfinite] != 0).any(axis=-1).sum())} scrubbed samples are not 0"
    # ---- radiance, every decidable sample ----
    dev = P.deviation(L.astype(np.float64), base["radiance"])
    worst = float(dev[dec].max())
    i = tuple(int(v) for v in np.unravel_index(np.argmax(np.where(dec, dev, -1.0)), dev.shape))
    print(f"{name}/{form}/depth {depth}: {dec.size} samples, {int((~dec).sum())} undecidable, {int(dec.sum())} compared, worst figure {worst:.3e} "
          f"(f32 checker {P.MEASURED_F32_ORACLE[(name, form)]:.2e})")
    record_metric(config="paths", scene=name, form=form, depth=depth, worst=worst, undecidable=int((~dec).sum()), samples=int(dec.size))
    tol = 2.0 * P.MEASURED_F32_ORACLE[(name, form)]
    wrong = np.argwhere(dec & (dev > tol))
    assert len(wrong) == 0, (f"{len(wrong)} decidable samples outside {tol:.2e}; worst {worst:.3e} at (y, x, s) = {i}: device {L[i]}, checker {base['radiance'][i]}, "
                             f"{int(base['segments'][i])} segments, terminal {int(base['terminal'][i])}, {P.describe(orc, int(base['events'][i]))}")
    # ---- the segment counter of every lone pass: both count world.hit calls; only an undecidable sample's path may differ ----
    for s in range(P.SPP):
        want = int(base["segments"][:, :, s].sum())
        slack = depth * int((~dec[:, :, s]).sum())
        assert abs(segs[s] - want) <= slack, (s, segs[s], want, slack)


@pytest.mark.parametrize("name,form", [(s, f) for s in P.SCENES for f in P.FORMS])
def test_nan_policy_reference(pkg, orc, gpu, name, form):
    """RT_NAN_REFERENCE sums samples as they are: a decidable sample is non-finite on the device exactly where the checker's terminal code
    says so, and elsewhere it is the default policy's sample, bit for bit."""
    A = pkg._abi
    c = P.decide(pkg, orc, name, form, 8)
    dec, base = c["decidable"], c["base"]
    scene = uploaded(pkg, gpu, name, form)
    raw, _ = device_samples(pkg, gpu, scene, c["built"].cam, 8, nan_policy=A.RT_NAN_REFERENCE)
    scrubbed, _ = device_samples(pkg, gpu, scene, c["built"].cam, 8)
    bad = ~np.isfinite(raw).all(axis=-1)
    want = base["terminal"] == orc.TERM_NONFINITE
    wrong = np.argwhere(dec & (bad != want))
    print(f"{name}/{form}: {int((dec & want).sum())} decidable non-finite samples, {int((bad & ~dec).sum())} more on undecidable ones")
    if name == "lights_default":
        assert int((dec & want).sum()) >= P.COVERAGE          # (the scene that is there to produce them)
    assert len(wrong) == 0, [tuple(int(v) for v in i) for i in wrong[:8]]
    assert raw[~bad].tobytes() == scrubbed[~bad].tobytes() and not scrubbed[bad].any()


@pytest.mark.parametrize("name,form", [(s, f) for s in P.SCENES for f in P.FORMS])
def test_carriers_bit_for_bit(pkg, gpu, name, form):
    """shade_segment is run by k_shade (the wavefront loop to the end: tail_paths = 1), by the drain kernel (the default) and by the
    fused kernel (RT_FLAG_FUSED): the same frame, samples and segments from all three."""
    A = pkg._abi
    built, _ = P.scene(pkg, name, form)
    scene = uploaded(pkg, gpu, name, form)
    a, sa = gpu.render(scene, built.cam, P.params(pkg, 8, tail_paths=1))
    assert sa["drain_paths"] == 0
    for kw in (dict(), dict(flags=A.RT_FLAG_FUSED, tail_paths=1)):
        b, sb = gpu.render(scene, built.cam, P.params(pkg, 8, **kw))
        assert sb["drain_paths"] > 0, kw
        assert a.tobytes() == b.tobytes(), kw
        assert sa["samples"] == sb["samples"] == P.W * P.H * P.SPP and sa["segments"] == sb["segments"], kw


@pytest.mark.parametrize("name,form", [("glass", "own"), ("lights_none", "own"), ("glass_mesh", "own"), ("wrap_flip_both", "own"), ("textures_wrapped", "all"),
                                       ("lights_many", "own"), ("smooth_lit", "own")])
def test_layouts_bit_for_bit(pkg, gpu, name, form):
    """Scenes of every kernel variant (0 twice: glass with its hollow ball, Lambertian spheres; mesh, box, all; the light tree; attributes
    under extended lights): shading does not depend on where the walk found its records."""
    A = pkg._abi
    built, _ = P.scene(pkg, name, form)
    prm = P.params(pkg, 8)
    a, sa = gpu.render(uploaded(pkg, gpu, name, form), built.cam, prm)
    for layout in (A.RT_LAYOUT_SCENE_IN_HBM, A.RT_LAYOUT_REFERENCE_COUNTERS):
        b, sb = gpu.render(uploaded(pkg, gpu, name, form, layout), built.cam, prm)
        assert a.tobytes() == b.tobytes(), layout
        assert sa["segments"] == sb["segments"], layout
    assert sa["bvh_in_lds"] == 1 and gpu.render(uploaded(pkg, gpu, name, form, A.RT_LAYOUT_SCENE_IN_HBM), built.cam, prm)[1]["bvh_in_lds"] == 0


def test_lights_table_reads_the_same_from_lds_and_hbm(pkg, orc, gpu):
    """k_shade finds the lights table of RT_SCENE_LIGHTS_MANY (LightX records, tree records, cdf, slots) in its LDS blob where the shade
    tables fit 8 KB (rt_api.cpp) and in HBM otherwise. `lights_many` fits; `lights_many_padded` is the same scene with paths.PADDING
    Lambertian spheres behind the camera, whose sphere records alone exceed 8 KB. Every sample whose path the checker finds decidable in
    both scenes, and the same in both (segments, terminal, events and radiance, bit for bit: it never meets the padding — a padding sphere
    that is tested and missed changes nothing), must be bit-identical on the device.
    The library reports nowhere whether the blob was built, so the two sizes are bounded here from the compiled tables' counts
    (rt_scene_compile_info) and the record sizes of csrc/device_types.h, as rt_api.cpp sums them: 12 tables, each padded to 16 bytes."""
    a, b = P.decide(pkg, orc, "lights_many", "own", 8), P.decide(pkg, orc, "lights_many_padded", "own", 8)

    def blob_bounds(built):
        i = pkg.compile_info(built.desc)
        n = i["n_lights"]
        lights = 96 * n + 32 * (2 * n - 1) + 8 * n                      # LightX records, tree records, cdf and slots
        low = 20 * i["n_spheres"] + 36 * i["n_rects"] + lights
        # a moving sphere 48 + 4 B; a material 20 B; an Xform 32 B; a Wrap 112 B, one per composite transform and wrap 0 (the scene has no
        # chain of FlipFace alone); a Texture 32 B, at most one per texture of the builder
        high = low + 52 * i["n_moving"] + 20 * i["n_materials"] + 32 * i["n_xforms"] + 112 * (i["n_xforms"] + 1) + 32 * len(built.keep.textures) + 12 * 15
        return low, high
    assert blob_bounds(a["built"])[1] <= 8 * 1024 < blob_bounds(b["built"])[0], (blob_bounds(a["built"]), blob_bounds(b["built"]))
    same = a["decidable"] & b["decidable"]
    for k in ("segments", "terminal", "events", "radiance"):
        eq = a["base"][k] == b["base"][k]
        same &= eq.all(axis=-1) if eq.ndim == 4 else eq
    assert same.mean() > 0.9, same.mean()
    assert int((same & ((a["base"]["events"] & np.uint64(orc.EVENTS["lambertian_light_cdf_pick"])) != 0)).sum()) >= P.COVERAGE
    La, _ = device_samples(pkg, gpu, uploaded(pkg, gpu, "lights_many", "own"), a["built"].cam, 8)
    Lb, _ = device_samples(pkg, gpu, uploaded(pkg, gpu, "lights_many_padded", "own"), b["built"].cam, 8)
    differ = np.argwhere(same & (La.view(np.uint32) != Lb.view(np.uint32)).any(axis=-1))
    print(f"lights table in LDS against HBM: {int(same.sum())} of {same.size} samples compared, {len(differ)} differ")
    assert len(differ) == 0, [tuple(int(v) for v in i) for i in differ[:8]]
