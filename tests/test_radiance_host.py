"""Radiance queries (include/rt_hip.h, "radiance queries"), the part that needs no device: the argument checks of rt_radiance_check, the ray
helpers of radiance.py, and the conditions the exact link of tests/test_gpu_radiance.py rests on (tests/radiance.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radiance as RQ  # noqa: E402


def test_records_match_the_header(pkg, tmp_path):
    import subprocess
    A = pkg._abi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(RtPathRay), '
                   'sizeof(RtRadianceOptions), offsetof(RtPathRay, first_draw), offsetof(RtRadianceOptions, seed), offsetof(RtRadianceOptions, tail_paths));return 0;}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(RQ.R.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [32, 56, 28, 32, 48]
    assert [C.sizeof(A.RtPathRay), C.sizeof(A.RtRadianceOptions), A.RtPathRay.first_draw.offset, A.RtRadianceOptions.seed.offset,
            A.RtRadianceOptions.tail_paths.offset] == got
    assert pkg.PATHRAY_DTYPE.itemsize == 32 and pkg.PATHRAY_DTYPE.fields["first_draw"][1] == 28


def test_check_refuses_with_a_reason(pkg):
    A, lib = pkg._abi, pkg.lib()
    good = pkg.radiance_options(samples=4)
    pkg.radiance_check(good, 0)
    pkg.radiance_check(good, 1 << 28)                                   # at least 2^28 rays per call
    pkg.radiance_check(good, (1 << 32) - 1)                             # the exact limit: first_stream + n_rays <= 2^32 - 1
    pkg.radiance_check(pkg.radiance_options(samples=4, first_stream=(1 << 32) - 1 - 100), 100)
    pkg.radiance_check(pkg.radiance_options(samples=(1 << 32) - 1), 1)
    pkg.radiance_check(pkg.radiance_options(samples=1, first_sample=(1 << 32) - 2, render_flags=A.RT_FLAG_TIMING), 5)

    def refused(opt, n, word):
        with pytest.raises(pkg.RtError) as e:
            pkg.radiance_check(opt, n)
        assert e.value.code == A.RT_ERR_INVALID and word in str(e.value), str(e.value)

    refused(None, 1, "null")
    short = pkg.radiance_options(samples=4); short.struct_bytes = C.sizeof(A.RtRadianceOptions) - 8
    refused(short, 1, "struct_bytes")
    refused(pkg.radiance_options(samples=4, flags=2), 1, "flags")
    refused(pkg.radiance_options(samples=4, render_flags=A.RT_FLAG_COUNTERS), 1, "render_flags")
    refused(pkg.radiance_options(samples=4, render_flags=A.RT_FLAG_TIMING | 64), 1, "render_flags")
    refused(pkg.radiance_options(samples=0), 1, "samples")
    refused(pkg.radiance_options(samples=2, first_sample=(1 << 32) - 2), 1, "first_sample")
    refused(pkg.radiance_options(samples=1, first_sample=(1 << 32) - 1), 1, "first_sample")
    refused(pkg.radiance_options(samples=4, max_depth=0), 1, "max_depth")
    refused(pkg.radiance_options(samples=4, max_depth=256), 1, "max_depth")
    refused(pkg.radiance_options(samples=4, nan_policy=2), 1, "nan_policy")
    refused(good, 1 << 32, "first_stream + n_rays")
    refused(pkg.radiance_options(samples=4, first_stream=(1 << 32) - 100), 100, "first_stream + n_rays")
    refused(pkg.radiance_options(samples=4, first_stream=1 << 40), 1, "first_stream + n_rays")
    refused(pkg.radiance_options(samples=4, first_stream=(1 << 64) - 1), 2, "first_stream + n_rays")     # (no wrap-around)
    # without a context every entry point that would compute says so before it reads anything
    assert lib.rt_radiance_rays(None, None, C.byref(good), None, 0, None, None, None, None) == A.RT_ERR_INVALID
    assert lib.rt_radiance_rays_device(None, None, C.byref(good), None, 0, None, None, None, None) == A.RT_ERR_INVALID


def test_path_rays(pkg):
    r = pkg.path_rays((1, 2, 3), [(0, 0, -1), (0, 1, 0)], time=0.25, first_draw=[0, 5])
    assert r.dtype == pkg.PATHRAY_DTYPE and r.shape == (2,)
    assert (r["o"] == np.float32([1, 2, 3])).all() and (r["d"][1] == np.float32([0, 1, 0])).all()
    assert (r["time"] == np.float32(0.25)).all() and list(r["first_draw"]) == [0, 5]
    flat = r.view(np.float32).reshape(2, 8)
    assert flat[1, 7].view(np.uint32) == 5 and flat[0, 3] == np.float32(0.25)


def test_equirect_rays(pkg):
    Wp, Hp = 64, 32
    r = pkg.equirect_rays((0.5, 1.0, -2.0), Wp, Hp, time=0.5)
    assert r.shape == (Wp * Hp,) and (r["o"] == np.float32([0.5, 1.0, -2.0])).all() and (r["time"] == np.float32(0.5)).all() and (r["first_draw"] == 0).all()
    d = r["d"].reshape(Hp, Wp, 3)
    # unit length to one ulp of 1: a unit f64 vector rounded once, component by component
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=2) - 1.0).max() <= 2.0 ** -23
    # mirrored columns mirror x, mirrored rows mirror y, exactly
    assert (d[:, ::-1, 0] == -d[:, :, 0]).all() and (d[:, ::-1, 1] == d[:, :, 1]).all() and (d[:, ::-1, 2] == d[:, :, 2]).all()
    assert (d[::-1, :, 1] == -d[:, :, 1]).all() and (d[::-1, :, 0] == d[:, :, 0]).all() and (d[::-1, :, 2] == d[:, :, 2]).all()
    # row 0 is the top and points up; y falls from row to row; the centre looks along -z and x grows to the right
    assert (d[0, :, 1] > 0.99).all() and (d[-1, :, 1] < -0.99).all() and (np.diff(d[:, 0, 1]) < 0).all()
    assert d[Hp // 2, Wp // 2, 2] < -0.99 and d[Hp // 2, Wp // 2, 0] > 0 and d[Hp // 2, Wp // 2 - 1, 0] < 0
    assert d[Hp // 2, 3 * Wp // 4, 0] > 0.99 and d[Hp // 2, 0, 2] > 0.99


def test_standard_error(pkg):
    x = np.random.default_rng(2).uniform(0, 3, (5, 64, 3))
    se = pkg.standard_error(x.sum(axis=1), (x * x).sum(axis=1), 64)
    assert np.allclose(se, x.std(axis=1, ddof=1) / 8.0, rtol=1e-9)
    with pytest.raises(ValueError):
        pkg.standard_error(x.sum(axis=1), (x * x).sum(axis=1), 1)


def test_draw_counts_of_the_camera(pkg, orc):
    """n0 = 2 + 2 k + 1 with k >= 1 trials; no trial of the seeds used lies within 4 ulp of the disk's edge (where the device's f32 test could
    differ from this restatement); at least three values of k occur; and the count agrees with the draws tests/features.py::camera_rays
    consumes (its time is the draw after the accepted pair)."""
    ks = set()
    for seed in sorted(set(c.seed for c in RQ.cases(pkg))):
        n0, k, gap = RQ.draw_counts(orc, seed)
        assert gap > 4.0, (seed, gap)
        assert (k >= 1).all() and (n0 == 2 + 2 * k + 1).all()
        ks |= set(int(x) for x in np.unique(k))
    assert len(ks) >= 3, ks
    # against camera_rays: a camera whose time range is [0, 1] reports the draw it took as the time
    cam = pkg.camera_new((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, RQ.W / RQ.H, 0.0, 5.0, 0.0, 1.0)
    seed = RQ.cases(pkg)[0].seed
    import features as F
    _, _, tm = F.camera_rays(orc, cam, RQ.W, RQ.H, seed, 3)
    n0 = RQ.draw_counts(orc, seed)[0]
    for i in range(RQ.N):
        assert tm[i] == float(orc.rng_stream(seed, i, 3, 64)[2][n0[i, 3] - 1])


@pytest.mark.parametrize("case", ["cornell", "lights_many", "medium", "moving", "book1", "smooth_mesh"])
def test_the_aim_is_not_vacuous(pkg, orc, case):
    """The checker's render through the zero-field camera: sample 0 of the 192 pixels takes at least 96 distinct values and a path has at
    least 2 segments on average — the ray meets a surface that scatters and sees light. (The GPU test asserts the same of the device.)"""
    c = next(x for x in RQ.cases(pkg) if x.name == case)
    desc, attrs, _ = RQ.build(pkg, c.scene)
    cam = RQ.zero_field_camera(pkg, c.origin, c.direction, c.t)
    prm = pkg.make_params(RQ.W, RQ.H, 1, max_depth=c.max_depth, seed=c.seed)
    out = orc.render_paths(desc, cam, prm, precision=32, n_threads=4, attrs=attrs)
    rad, seg = out["radiance"].reshape(RQ.N, 3), out["segments"].reshape(RQ.N)
    assert len(np.unique(rad.astype(np.float32), axis=0)) >= 96
    assert seg.mean() >= 2.0
    # and the ray is what the camera makes: exact in f32
    o, d, tm = __import__("features").camera_rays(orc, cam, RQ.W, RQ.H, c.seed, 0)
    assert (o == np.asarray(c.origin, float)).all() and (d == np.asarray(c.direction, float)).all() and (tm == c.t).all()
    assert (np.float32(o) == o).all() and (np.float32(d) == d).all()
