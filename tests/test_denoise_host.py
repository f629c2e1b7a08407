"""CPU: the denoiser's host side (include/rt_hip.h, "denoising"): rt_denoise_check's refusals, the numpy restatement nlm_reference on
cases whose answer is known, and the proof that the specified filter (not a kernel) lowers the error of 16-spp crops of the benchmarked
frames against their converged fixtures (tests/golden/crops_C2.npz, crops_C4.npz), rendered here by the f64 oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crops as K   # noqa: E402

# The crops of the error-reduction tests (here and in tests/test_gpu_denoise.py), chosen on the CPU with this file: every crop of C2 and C4
# whose 16-spp frame has variance. C2's sky_horizon is left out: all but a sliver of it sees only the sky, its variance is rounding.
DENOISE_CROPS = [("C2", "glass_sphere"), ("C2", "metal_sphere_rim"), ("C2", "ground_small_spheres"),
                 ("C4", "light_edge"), ("C4", "box_and_green_wall"), ("C4", "glass_sphere"), ("C4", "caustic_floor")]
DENOISE_SPP = 16


def identity_cases():
    """(name, S, Q, n): frames the filter must return unchanged. constant: every pixel the same, zero variance (every weight is 1 and the
    mean of equal values is that value); distinct: pairwise distinct pixels at least 1/64 apart with Q = S^2 / k, so v = 0 and every
    foreign patch distance is at least (1/64)^2 / (49 eps) > 1e4: its weight underflows to 0 in f32 and in f64."""
    n, H, W = 16, 40, 48
    const = np.empty((H, W, 3), dtype=np.float32)
    const[:] = np.array([410, 2867, 5325], dtype=np.float32) / 4096 * n           # 12-bit values: S^2 / n is exact in f32, so v = 0
    u = (np.arange(H * W, dtype=np.float64).reshape(H, W) / 64.0 + 0.25)
    S = np.stack([u * n, (u + 0.5) * n, (u * 2.0) * n], axis=2).astype(np.float32)      # exactly representable: multiples of 1/4 below 2^11
    Sd = S.astype(np.float64)
    Q = (Sd * Sd / n).astype(np.float32)
    assert np.array_equal(Q.astype(np.float64) * n, Sd * Sd)                              # Q - S^2/k is exactly 0
    return [("constant", const, (const.astype(np.float64) ** 2 / n).astype(np.float32), n), ("distinct", S, Q, n)]


def test_denoise_check_validates(pkg):
    A, lib = pkg._abi, pkg.lib()
    assert lib.rt_denoise_check(1200, 800, None) == A.RT_OK
    assert lib.rt_denoise_check(1200, 800, C.byref(pkg.denoise_options())) == A.RT_OK
    assert lib.rt_denoise_check(64, 64, C.byref(pkg.denoise_options(A.RT_DENOISE_MAX_WINDOW_RADIUS, A.RT_DENOISE_MAX_PATCH_RADIUS, 4, 0.7, 0.5, 1e-6))) == A.RT_OK
    assert C.sizeof(A.RtDenoiseOptions) == 40
    bad = [(dict(window_radius=17), b"window_radius"), (dict(patch_radius=5), b"patch_radius"),
           (dict(strength=-0.45), b"strength"), (dict(strength=float("nan")), b"strength"), (dict(strength=float("inf")), b"strength"),
           (dict(strength=-0.0), b"strength"), (dict(alpha=-1.0), b"alpha"), (dict(alpha=float("nan")), b"alpha"),
           (dict(eps=-1e-10), b"eps"), (dict(eps=float("inf")), b"eps"), (dict(eps=1e-60), b"eps")]
    for kw, word in bad:
        assert lib.rt_denoise_check(64, 64, C.byref(pkg.denoise_options(**kw))) == A.RT_ERR_INVALID, kw
        assert word in lib.rt_last_error(None), (kw, lib.rt_last_error(None))
        with pytest.raises(pkg.RtError):
            pkg.denoise_check(64, 64, pkg.denoise_options(**kw))
    short = pkg.denoise_options(); short.struct_bytes = C.sizeof(A.RtDenoiseOptions) - 8
    assert lib.rt_denoise_check(64, 64, C.byref(short)) == A.RT_ERR_INVALID and b"struct_bytes" in lib.rt_last_error(None)
    unset = pkg.denoise_options(); unset.struct_bytes = 0
    assert lib.rt_denoise_check(64, 64, C.byref(unset)) == A.RT_ERR_INVALID
    for w, h in ((0, 64), (64, 0), (0, 0), (65536, 65536)):
        assert lib.rt_denoise_check(w, h, None) == A.RT_ERR_INVALID and b"size" in lib.rt_last_error(None)
    # no device is needed to refuse a call without a context
    assert lib.rt_denoise_device(None, None, 64, 64, None, None, 16, None, None) == A.RT_ERR_INVALID


@pytest.mark.parametrize("case", [0, 1])
def test_reference_identity_cases(pkg, case):
    name, S, Q, n = identity_cases()[case]
    u, v, valid = pkg.nlm_prepare(S, Q, n, 1)
    assert valid.all() and (v == 0).all()
    for opts in (dict(), dict(window_radius=3, patch_radius=1)):
        out = pkg.nlm_reference(S, Q, n, 1, **opts)
        assert np.array_equal(out, u.astype(np.float64)), name


def noisy_frame(H=24, W=28, n=16, seed=5):
    rng = np.random.default_rng(seed)
    base = 0.5 + 0.4 * np.sin(np.arange(W) / 5.0)[None, :, None] * np.cos(np.arange(H) / 7.0)[:, None, None] + np.array([0.0, 0.1, 0.2])
    smp = base[:, :, None, :] + 0.2 * rng.standard_normal((H, W, n, 3))
    return smp.sum(axis=2).astype(np.float32), (smp ** 2).sum(axis=2).astype(np.float32)


def test_reference_invalid_pixels_pass_through_and_influence_nobody(pkg):
    S, Q = noisy_frame()
    H, W = S.shape[:2]
    counts = np.full((H, W), 16, dtype=np.uint32)
    counts[5, 6] = 1            # one item: no variance
    counts[10, 11] = 0          # no sample
    S[10, 11] = 0.0; Q[10, 11] = 0.0
    S[15, 3, 1] = np.inf        # a non-finite sum
    opts = dict(window_radius=4, patch_radius=2)
    out = pkg.nlm_reference(S, Q, counts, 1, **opts)
    u, v, valid = pkg.nlm_prepare(S, Q, counts, 1)
    assert not valid[5, 6] and not valid[10, 11] and not valid[15, 3] and valid.sum() == H * W - 3
    assert np.array_equal(out[5, 6], S[5, 6].astype(np.float64)) and np.array_equal(out[10, 11], np.zeros(3))
    assert np.array_equal(out[15, 3], u[15, 3].astype(np.float64)) and np.isinf(out[15, 3, 1])
    assert np.isfinite(out[valid]).all()
    assert np.abs(out[valid] - u[valid]).max() > 1e-3            # the filter does filter
    S2, Q2 = S.copy(), Q.copy()
    S2[5, 6] += 100.0; S2[15, 3, 0] = -7.0; Q2[15, 3, 2] = 1e9
    out2 = pkg.nlm_reference(S2, Q2, counts, 1, **opts)
    other = np.ones((H, W), dtype=bool); other[5, 6] = other[15, 3] = False
    assert np.array_equal(out2[other], out[other])
    # m = 4 samples per item: 16 samples are 4 items, 4 samples are one item and therefore invalid
    c4 = np.full((H, W), 16, dtype=np.uint32); c4[2, 2] = 4
    assert pkg.nlm_prepare(S, Q, c4, 4)[2].sum() == H * W - 2     # (15, 3) is still non-finite
    # and the uniform form agrees with a constant counts buffer
    Sf, Qf = noisy_frame()
    assert np.array_equal(pkg.nlm_reference(Sf, Qf, 16, 1, **opts), pkg.nlm_reference(Sf, Qf, np.full((H, W), 16), 1, **opts))


def test_reference_depends_on_the_pixels_own_count(pkg):
    S, Q = noisy_frame()
    H, W = S.shape[:2]
    opts = dict(window_radius=4, patch_radius=2)
    a = pkg.nlm_reference(S, Q, 16, 1, **opts)
    counts = np.full((H, W), 16, dtype=np.uint32)
    counts[12, 14] = 8           # the same sums read as 8 samples: another mean, another variance
    b = pkg.nlm_reference(S, Q, counts, 1, **opts)
    assert np.abs(b[12, 14] - a[12, 14]).max() > 0.1
    far = np.ones((H, W), dtype=bool); far[12 - 6:12 + 7, 14 - 6:14 + 7] = False     # beyond window + patch nothing changes
    assert np.array_equal(a[far], b[far]) and not np.array_equal(a[~far], b[~far])


def oracle_crop_sums(pkg, orc, name, crop, tmp_path, spp=DENOISE_SPP):
    """(S, Q) of the crop at `spp` samples per pixel by the f64 oracle, rounded to f32 as the device's buffers are (m = 1)."""
    cfg = K.CONFIGS[name]
    hs = K.host_scene(pkg, name, tmp_path)
    cam = hs.camera(cfg["width"] / cfg["height"])
    prm = pkg.make_params(cfg["width"], cfg["height"], spp, max_depth=50, seed=cfg["seed"])
    _, _, ps = orc.render(hs.desc, cam, prm, precision=64, n_threads=8, rect=cfg["crops"][crop], per_sample=True)
    return ps.sum(axis=2).astype(np.float32), (ps * ps).sum(axis=2).astype(np.float32)


def test_crop_choice_covers_both_frames():
    assert len(DENOISE_CROPS) >= 4 and {n for n, _ in DENOISE_CROPS} == {"C2", "C4"}
    for name, crop in DENOISE_CROPS:
        assert crop in K.CONFIGS[name]["crops"]


@pytest.mark.parametrize("name,crop", DENOISE_CROPS)
def test_filter_reduces_error_against_the_converged_crop(pkg, orc, tmp_path, name, crop):
    """The specified filter with its defaults on a 16-spp oracle render of the crop: MSE against the converged fixture below the raw
    mean's. (Figures of this test on the CPU: DESIGN.md, "Denoising".)"""
    cfg = K.CONFIGS[name]
    truth = K.load_golden(name)[crop] / cfg["spp"]
    S, Q = oracle_crop_sums(pkg, orc, name, crop, tmp_path)
    assert np.isfinite(S).all() and np.isfinite(Q).all()
    raw = S.astype(np.float64) / DENOISE_SPP
    out = pkg.nlm_reference(S, Q, DENOISE_SPP, 1)
    mse_raw, mse_out = float(np.mean((raw - truth) ** 2)), float(np.mean((out - truth) ** 2))
    print(f"denoise {name}/{crop}: raw MSE {mse_raw:.6g}, filtered MSE {mse_out:.6g}, ratio {mse_out / mse_raw:.4f}")
    assert mse_out < mse_raw, (mse_raw, mse_out)
