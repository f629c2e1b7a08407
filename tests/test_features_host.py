"""First-hit features without a GPU (include/rt_hip.h, "first-hit features"): the struct mirrors against a compiled probe of the header,
rt_features_check's refusals, the numpy restatement of the renderer's camera ray against the camera's geometry, and — with the CPU
checker alone — that the pixel sets the GPU test compares stay inside its two caps."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import features as F  # noqa: E402
import rays as R  # noqa: E402


def test_feature_symbols_and_structs_match_the_header(pkg, tmp_path):
    A, lib = pkg._abi, pkg.lib()
    for name in ("rt_features_check", "rt_render_features_device"):
        assert name in A.RT_HIP_SYMBOLS and hasattr(lib, name), name
    body = ""
    for name in ("RtFeatureOptions", "RtFeatureBuffers"):
        body += f'printf("{name} %zu\\n", sizeof({name}));'
        body += "".join(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in getattr(A, name)._fields_)
    body += 'printf("flag %u\\n", (unsigned)RT_FEATURES_ACCUMULATE); printf("abi %u\\n", (unsigned)RT_ABI_VERSION);'
    src = tmp_path / "ft.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_hip.h"\nint main(void){' + body + "return 0;}")
    exe = tmp_path / "ft"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split(None, 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, size in (("RtFeatureOptions", 16), ("RtFeatureBuffers", 4 * C.sizeof(C.c_void_p))):
        T = getattr(A, name)
        assert int(got[name]) == C.sizeof(T) == size, name
        for f, _ in T._fields_:
            assert int(got[f"{name}.{f}"]) == getattr(T, f).offset, (name, f)
    assert int(got["flag"]) == A.RT_FEATURES_ACCUMULATE == 1
    assert int(got["abi"]) == A.RT_ABI_VERSION == 3 == lib.rt_abi_version()


def test_features_check(pkg):
    A, lib = pkg._abi, pkg.lib()
    prm = pkg.make_params(40, 24, 8, tile_size=16)
    pkg.features_check(prm, pkg.feature_options())
    pkg.features_check(prm, pkg.feature_options(first_sample=5, accumulate=True, pool_slots=4096))
    pkg.features_check(pkg.make_params(40, 24, 8, tile_size=16, shard_index=2, shard_count=3), pkg.feature_options())
    for flags in (A.RT_FLAG_TIMING, A.RT_FLAG_SAMPLE_BLOCKS, A.RT_FLAG_TIMING | A.RT_FLAG_SAMPLE_BLOCKS):
        pkg.features_check(pkg.make_params(40, 24, 8, flags=flags), pkg.feature_options())
    pkg.features_check(pkg.make_params(40, 24, 8), pkg.feature_options(first_sample=(1 << 32) - 1 - 8))
    big = A.RtFeatureOptions(64, 0, 0, 0)                          # a caller compiled against a longer struct
    assert lib.rt_features_check(C.byref(prm), C.byref(big)) == A.RT_OK

    def refused(params, opt, word):
        assert lib.rt_features_check(C.byref(params) if params is not None else None, C.byref(opt) if opt is not None else None) == A.RT_ERR_INVALID, word
        assert word in lib.rt_last_error(None), (word, lib.rt_last_error(None))
    refused(prm, A.RtFeatureOptions(0, 0, 0, 0), b"struct_bytes")
    refused(prm, A.RtFeatureOptions(12, 0, 0, 0), b"struct_bytes")
    refused(prm, A.RtFeatureOptions(16, 2, 0, 0), b"unknown")
    refused(prm, A.RtFeatureOptions(16, 1 << 31, 0, 0), b"unknown")
    refused(prm, pkg.feature_options(first_sample=(1 << 32) - 8), b"2^32")
    refused(prm, pkg.feature_options(first_sample=(1 << 32) - 1), b"2^32")
    refused(prm, None, b"null")
    refused(None, pkg.feature_options(), b"null")
    refused(pkg.make_params(40, 24, 8, flags=A.RT_FLAG_COUNTERS), pkg.feature_options(), b"RT_FLAG_COUNTERS")
    refused(pkg.make_params(40, 24, 8, flags=A.RT_FLAG_FUSED | A.RT_FLAG_TIMING), pkg.feature_options(), b"RT_FLAG_FUSED")
    refused(pkg.make_params(40, 24, 0), pkg.feature_options(), b"samples_per_pixel")
    refused(pkg.make_params(40, 24, 8, tile_size=12), pkg.feature_options(), b"tile_size")
    with pytest.raises(pkg.RtError) as e:
        pkg.features_check(prm, pkg.feature_options(flags=4))
    assert e.value.code == A.RT_ERR_INVALID
    # without a context nothing runs, and nothing is touched
    assert lib.rt_render_features_device(None, None, None, None, None, None, None) == A.RT_ERR_INVALID


def test_camera_ray_restatement_against_the_camera(pkg, orc):
    """tests/features.py camera_rays — the draws of new_camera_ray in their order — against the geometry of the checker's Camera::new: with
    the jitter forced to 0.5 and no lens, the pixel-centre rays of rays.camera_rays; with a lens, origins on the lens disk and every ray
    through its pixel's point of the focus plane; times inside the shutter interval, from the draw after the accepted disk pair."""
    A = pkg._abi
    W, H = 24, 16
    cam = A.RtCamera()
    d3 = lambda v: (C.c_double * len(v))(*v)
    orc.lib().orc_camera_new(d3((3.0, 2.0, 6.0)), d3((0.0, 0.5, 0.0)), d3((0.0, 1.0, 0.0)), d3((30.0, 1.5, 0.0, 10.0)), 0.0, 0.0, C.byref(cam))
    o, d, tm = F.camera_rays(orc, cam, W, H, F.SEED, 0, jitter=0.5)
    centre = R.camera_rays(cam, W, H, np.random.default_rng(0))
    assert np.array_equal(o.astype(np.float32), centre["o"]) and np.array_equal(d.astype(np.float32), centre["d"]) and not tm.any()
    # a lens and a shutter: the same pixels, jittered
    orc.lib().orc_camera_new(d3((3.0, 2.0, 6.0)), d3((0.0, 0.5, 0.0)), d3((0.0, 1.0, 0.0)), d3((30.0, 1.5, 0.4, 7.0)), 0.25, 0.75, C.byref(cam))
    assert cam.lens_radius == 0.2
    o, d, tm = F.camera_rays(orc, cam, W, H, F.SEED, 3)
    v3 = lambda v: np.array([v.x, v.y, v.z])
    off = o - v3(cam.origin)
    r = np.linalg.norm(off, axis=1)
    assert (r < cam.lens_radius * (1 + 1e-12)).all() and r.max() > 0.8 * cam.lens_radius and np.abs(off @ v3(cam.w)).max() < 1e-12
    target = o + d - v3(cam.lower_left_corner)                     # = u * horizontal + v * vertical
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    u = (target @ v3(cam.horizontal)) / (v3(cam.horizontal) @ v3(cam.horizontal)) * (W - 1) - x.reshape(-1)
    v = (target @ v3(cam.vertical)) / (v3(cam.vertical) @ v3(cam.vertical)) * (H - 1) - (H - 1 - y.reshape(-1))
    assert (u > -1e-9).all() and (u < 1 + 1e-9).all() and (v > -1e-9).all() and (v < 1 + 1e-9).all() and np.ptp(u) > 0.9 and np.ptp(v) > 0.9
    assert (tm >= 0.25).all() and (tm < 0.75).all() and np.ptp(tm) > 0.4
    # the jitter is draws 0 and 1, the time the draw behind the accepted disk pair
    i = 5 * W + 7
    draws = orc.rng_stream(F.SEED, i, 3, 40)[2].astype(np.float64)
    assert abs(u[i] - draws[0]) < 1e-9 and abs(v[i] - draws[1]) < 1e-9
    k = 2
    while (2 * draws[k] - 1) ** 2 + (2 * draws[k + 1] - 1) ** 2 >= 1.0:
        k += 2
    assert tm[i] == 0.25 + 0.5 * draws[k + 2]


@pytest.mark.parametrize("name", F.SCENES)
def test_pixel_sets_stay_inside_the_caps(pkg, orc, name):
    """The two caps of tests/test_gpu_features.py, with the checker's own hits: at most 1 % of a scene's sample-0 rays are undecidable, and
    at most 2 % of its hit pixels lie on a texture boundary (the colour moves by more than 1e-3 under the ray queries' measured error)."""
    s = F.pixel_set(pkg, orc, name)
    built, rays, ref, und = s["built"], s["rays"], s["ref"], s["undecidable"]
    hit = ref["hit"]
    ids, on = R.objects_at(pkg, built.desc, ref["p"], rays["time"].astype(np.float64), built.extent)
    assert on[hit & ~und].any(axis=1).all()
    material = np.where(on.any(axis=1), np.array([built.desc.hittables[int(i)].material for i in ids])[on.argmax(axis=1)], -1)
    albedo, unstable = F.expected_albedo(pkg, orc, built.desc, hit & on.any(axis=1), material, ref["ff"], ref["u"], ref["v"], ref["p"], rays["d"], err=F.YARDSTICK_ERR[name])
    print(f"{name}: {len(rays)} pixels, {int(hit.sum())} hits, {int(und.sum())} undecidable, {int((unstable & hit).sum())} on a texture boundary")
    assert hit.sum() > len(rays) // 5 and (name == "cornell" or (~hit).sum() > 0)
    assert und.mean() <= 0.01, f"{name}: {und.mean():.4f} of the pixels are undecidable"
    assert (unstable & hit).sum() <= 0.02 * hit.sum(), f"{name}: {(unstable & hit).sum()} of {hit.sum()} hit pixels on a texture boundary"
    assert np.isfinite(albedo).all() and (albedo >= 0).all()
    if name == "textured":
        assert len(np.unique(np.round(albedo[hit], 3), axis=0)) > 50           # the Perlin sphere and both checker colours are in view
