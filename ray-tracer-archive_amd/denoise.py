"""Denoising of low-sample frames: non-local means over the sample variance (include/rt_hip.h, "denoising").

nlm_reference restates the filter in numpy — the prepare step in f64 rounded to f32, the filter step in f64 from those f32 planes — and is
what the device kernels (csrc/denoise.hip, f32) are tested against. nlm_guided_reference is the same filter with its weights joined with
first-hit features ("denoising, guided"): guide_prepare makes the binary16 guide components, the filter step is nlm_reference's own.
nlm_guided_moments_reference is the guided filter with its feature distance variance-cancelled and variance-normalised ("denoising, guided
with feature variances"): guide_moments_prepare makes the ten binary16 components, three standard errors among them.
denoise_frame is the device path behind Progressive.denoised() and Adaptive.denoised(); render_guide makes the feature pass they join in.
"""
import numpy as np

from . import _abi as A
from .api import denoise_options
from .layout import in_place, on_device

DEFAULTS = dict(window_radius=10, patch_radius=3, strength=0.45, alpha=1.0, eps=1e-10)
MOMENTS_MAX_WINDOW_RADIUS = 8                                                     # RT_DENOISE_GUIDED_MOMENTS_MAX_WINDOW_RADIUS, and what 0 means there
GUIDE_MOMENTS_DEFAULTS = dict(sigma_albedo=0.01, sigma_normal=0.025, sigma_depth=0.01, variance_strength=64.0)   # the library's (include/rt_hip.h; measured: DESIGN.md, "Denoising")
GUIDE_DEFAULTS = dict(sigma_albedo=0.2, sigma_normal=0.5, sigma_depth=0.2)      # the library's (include/rt_hip.h; measured: DESIGN.md, "Denoising")


def _options(opts):
    o = dict(DEFAULTS)
    for k, v in opts.items():
        if k not in o:
            raise TypeError(f"unknown denoise option '{k}'")
        if v:                                   # a field left 0 takes its default, as in RtDenoiseOptions
            o[k] = v
    return int(o["window_radius"]), int(o["patch_radius"]), float(o["strength"]), float(o["alpha"]), float(o["eps"])


def nlm_prepare(rgb_sum, sq_sum, counts_or_n, m):
    """The prepare step: per pixel the mean u and the variance of the mean v, f32 (H, W, 3), and which pixels are valid (H, W).
    counts_or_n: one sample count for every pixel, or an (H, W) array of counts; m: samples per work item."""
    S32 = np.asarray(rgb_sum, dtype=np.float32)
    if S32.ndim != 3 or S32.shape[2] != 3:
        raise ValueError("rgb_sum must be (H, W, 3)")
    S = S32.astype(np.float64)
    Q = np.asarray(sq_sum, dtype=np.float32).reshape(S.shape).astype(np.float64)
    H, W = S.shape[:2]
    n = np.broadcast_to(np.asarray(counts_or_n), (H, W)).astype(np.int64) if np.ndim(counts_or_n) else np.full((H, W), int(counts_or_n), dtype=np.int64)
    m = int(m)
    items = -(-n // m)
    valid = (n > 0) & (items >= 2) & np.isfinite(S).all(axis=2) & np.isfinite(Q).all(axis=2)
    k, nn = items.astype(np.float64)[..., None], n.astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        u = np.where(nn > 0, S / nn, 0.0).astype(np.float32)
        d = Q - S * S / k
        d = np.where(d > 0.0, d, 0.0)
        v = (d / (k * (k - 1.0)) / (float(m) * float(m))).astype(np.float32)
    v[~valid] = 0.0
    return u, v, valid


def _filter(u32, v32, valid, opts, guide=None, kappa=None):
    """The filter step in f64 from the prepared f32 planes; guide: (H, W, 7) binary16 components whose squared distance joins the patch
    distance, or None; with kappa given, guide is (H, W, 10) — the seven and the standard errors sA, sN, sZ — and g takes the variance form.
    Every sum is taken directly, term by term; the output is u[p] + sum w (u[q] - u[p]) / sum w."""
    r, f, kk, alpha, eps = _options(opts)
    H, W = valid.shape
    pad = r + f
    u = np.zeros((H + 2 * pad, W + 2 * pad, 3)); v = np.zeros_like(u); ok = np.zeros((H + 2 * pad, W + 2 * pad), dtype=bool)
    u[pad:pad + H, pad:pad + W] = u32; v[pad:pad + H, pad:pad + W] = v32; ok[pad:pad + H, pad:pad + W] = valid
    u = np.where(ok[..., None], u, 0.0)          # an invalid pixel's u may be non-finite: it takes part in nothing
    Ha, Wa = H + 2 * f, W + 2 * f                  # the pixels p + o
    if guide is not None:
        G = np.zeros((H + 2 * pad, W + 2 * pad, guide.shape[2]))
        G[pad:pad + H, pad:pad + W] = np.where(valid[..., None], guide.astype(np.float64), 0.0)

    def shifted(a, dy, dx, h, w, margin):
        return a[margin + dy:margin + dy + h, margin + dx:margin + dx + w]

    ua, va, oka = shifted(u, 0, 0, Ha, Wa, r), shifted(v, 0, 0, Ha, Wa, r), shifted(ok, 0, 0, Ha, Wa, r)
    up, okp = u[pad:pad + H, pad:pad + W], valid
    sw = np.zeros((H, W)); swu = np.zeros((H, W, 3))
    k2 = kk * kk
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ub, vb, okb = shifted(u, dy, dx, Ha, Wa, r), shifted(v, dy, dx, Ha, Wa, r), shifted(ok, dy, dx, Ha, Wa, r)
                part = oka & okb
                t = ((ua - ub) ** 2 - alpha * (va + np.minimum(va, vb))) / (eps + k2 * (va + vb))
                t = np.where(part, t.sum(axis=2), 0.0)
                D = np.zeros((H, W)); cnt = np.zeros((H, W))
                for oy in range(2 * f + 1):
                    for ox in range(2 * f + 1):
                        D += t[oy:oy + H, ox:ox + W]
                        cnt += part[oy:oy + H, ox:ox + W]
                uq, okq = shifted(u, dy, dx, H, W, pad), shifted(ok, dy, dx, H, W, pad)
                pair = okp & okq
                d = D / np.maximum(3.0 * cnt, 1.0)
                if guide is None:
                    w = np.where(pair, np.exp(-np.maximum(d, 0.0)), 0.0)
                elif kappa is not None:
                    Fp, Fq = shifted(G, 0, 0, H, W, pad), shifted(G, dy, dx, H, W, pad)
                    g = np.zeros((H, W))
                    for lo, hi, s in ((0, 3, 7), (3, 6, 8), (6, 7, 9)):
                        d2 = ((Fp[..., lo:hi] - Fq[..., lo:hi]) ** 2).sum(axis=2)
                        Vp, Vq = Fp[..., s] ** 2, Fq[..., s] ** 2
                        g += np.maximum(d2 - (Vp + np.minimum(Vp, Vq)), 0.0) / (1.0 + kappa * (Vp + Vq))
                    w = np.where(pair, np.exp(-(np.maximum(d, 0.0) + g)), 0.0)
                else:
                    g = ((shifted(G, 0, 0, H, W, pad) - shifted(G, dy, dx, H, W, pad)) ** 2).sum(axis=2)
                    w = np.where(pair, np.exp(-(np.maximum(d, 0.0) + g)), 0.0)
                sw += w
                swu += w[..., None] * (uq - up)
        out = up + swu / np.where(sw > 0, sw, 1.0)[..., None]          # summed as differences from u[p], as the kernels do: a constant frame is exact
    return np.where(valid[..., None], out, u32.astype(np.float64))


def nlm_reference(rgb_sum, sq_sum, counts_or_n, m, **opts):
    """The filter of include/rt_hip.h restated: the filtered mean radiance, f64 (H, W, 3). opts: window_radius, patch_radius, strength,
    alpha, eps (0 or absent: the default). Every sum is taken directly, term by term, in f64."""
    u32, v32, valid = nlm_prepare(rgb_sum, sq_sum, counts_or_n, m)
    return _filter(u32, v32, valid, opts)


def guide_prepare(feature_samples, albedo_sum=None, normal_sum=None, depth_sum=None, hits=None, sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0):
    """The guide of include/rt_hip.h ("denoising, guided"): (F, valid) — F (H, W, 7) binary16, the components A0 A1 A2 N0 N1 N2 Z computed
    in f64, rounded to f32, then to binary16 (round to nearest even) and clamped to +-65504; a plane that is None gives 0. valid (H, W):
    every given feature sum is finite and hits <= feature_samples. albedo_sum / normal_sum: (H, W, 3), depth_sum / hits: (H, W)."""
    n_f = int(feature_samples)
    if n_f < 1:
        raise ValueError("feature_samples must be >= 1")
    if albedo_sum is None and normal_sum is None and depth_sum is None:
        raise ValueError("a guide needs one of albedo_sum, normal_sum, depth_sum (the filter without a guide is nlm_reference)")
    if depth_sum is not None and hits is None:
        raise ValueError("depth_sum needs hits")
    sig = [float(s) if s else GUIDE_DEFAULTS[k] for k, s in (("sigma_albedo", sigma_albedo), ("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth))]
    first = next(p for p in (albedo_sum, normal_sum, depth_sum) if p is not None)
    H, W = np.shape(first)[:2]
    F = np.zeros((H, W, 7))
    valid = np.ones((H, W), dtype=bool)
    with np.errstate(all="ignore"):
        for plane, at, sigma in ((albedo_sum, 0, sig[0]), (normal_sum, 3, sig[1])):
            if plane is not None:
                s = np.asarray(plane, dtype=np.float32).reshape(H, W, 3).astype(np.float64)
                valid &= np.isfinite(s).all(axis=2)
                F[..., at:at + 3] = s / float(n_f) / sigma
        h = np.asarray(hits).reshape(H, W).astype(np.int64) if hits is not None else np.zeros((H, W), dtype=np.int64)
        valid &= h <= n_f
        if depth_sum is not None:
            s = np.asarray(depth_sum, dtype=np.float32).reshape(H, W).astype(np.float64)
            valid &= np.isfinite(s)
            F[..., 6] = np.where(h > 0, np.log(np.maximum(s / np.maximum(h, 1), 1e-30)) / sig[2], 0.0)
        F16 = np.clip(F.astype(np.float32).astype(np.float16), np.float16(-65504), np.float16(65504))
    F16[~valid] = 0
    return F16, valid


def nlm_guided_reference(rgb_sum, sq_sum, counts_or_n, m, feature_samples, albedo_sum=None, normal_sum=None, depth_sum=None, hits=None,
                         sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0, **opts):
    """The guided filter of include/rt_hip.h restated: nlm_reference with g(p,q), the squared distance of the binary16 guide components,
    added to max(d, 0) in the weight; f64 (H, W, 3). A pixel the guide makes invalid is invalid for the colour part too."""
    u32, v32, valid = nlm_prepare(rgb_sum, sq_sum, counts_or_n, m)
    F, ok = guide_prepare(feature_samples, albedo_sum, normal_sum, depth_sum, hits, sigma_albedo, sigma_normal, sigma_depth)
    if ok.shape != valid.shape:
        raise ValueError("the feature planes have another size than the frame")
    valid = valid & ok
    v32 = v32.copy(); v32[~valid] = 0.0
    return _filter(u32, v32, valid, opts, guide=F)


def guide_moments_prepare(feature_samples, albedo_sum=None, normal_sum=None, depth_sum=None, hits=None, albedo_sq_sum=None, normal_sq_sum=None,
                          depth_sq_sum=None, sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0):
    """The guide of include/rt_hip.h ("denoising, guided with feature variances"): (F, valid) — F (H, W, 10) binary16: A0 A1 A2 N0 N1 N2 Z
    as guide_prepare makes them (with this filter's default sigmas), then the standard errors sA, sN, sZ of the three groups over their
    sigmas, from var(S, Q) = max(Q - S^2 / n_f, 0) / (n_f (n_f - 1)); all in f64, rounded to f32, then to binary16, clamped to +-65504. A
    sum plane that is None zeroes its group, a squared plane that is None its variance. valid (H, W): every given sum and squared sum is
    finite and hits <= feature_samples."""
    n_f = int(feature_samples)
    if n_f < 2:
        raise ValueError("feature_samples must be >= 2 (a variance needs two samples)")
    if albedo_sum is None and normal_sum is None and depth_sum is None:
        raise ValueError("a guide needs one of albedo_sum, normal_sum, depth_sum (the filter without a guide is nlm_reference)")
    if depth_sum is not None and hits is None:
        raise ValueError("depth_sum needs hits")
    sig = [float(s) if s else GUIDE_MOMENTS_DEFAULTS[k] for k, s in (("sigma_albedo", sigma_albedo), ("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth))]
    first = next(p for p in (albedo_sum, normal_sum, depth_sum) if p is not None)
    H, W = np.shape(first)[:2]
    F = np.zeros((H, W, 10))
    valid = np.ones((H, W), dtype=bool)
    nf = float(n_f)

    def var(S, Q):
        d = Q - S * S / nf
        return np.where(d > 0.0, d, 0.0) / (nf * (nf - 1.0))
    with np.errstate(all="ignore"):
        for plane, sq, at, se, sigma in ((albedo_sum, albedo_sq_sum, 0, 7, sig[0]), (normal_sum, normal_sq_sum, 3, 8, sig[1])):
            q = None
            if sq is not None:
                q = np.asarray(sq, dtype=np.float32).reshape(H, W, 3).astype(np.float64)
                valid &= np.isfinite(q).all(axis=2)
            if plane is not None:
                s = np.asarray(plane, dtype=np.float32).reshape(H, W, 3).astype(np.float64)
                valid &= np.isfinite(s).all(axis=2)
                F[..., at:at + 3] = s / nf / sigma
                if q is not None:
                    V = var(s[..., 0], q[..., 0]) + var(s[..., 1], q[..., 1]) + var(s[..., 2], q[..., 2])
                    F[..., se] = np.sqrt(V) / sigma
        h = np.asarray(hits).reshape(H, W).astype(np.int64) if hits is not None else np.zeros((H, W), dtype=np.int64)
        valid &= h <= n_f
        qz = None
        if depth_sq_sum is not None:
            qz = np.asarray(depth_sq_sum, dtype=np.float32).reshape(H, W).astype(np.float64)
            valid &= np.isfinite(qz)
        if depth_sum is not None:
            s = np.asarray(depth_sum, dtype=np.float32).reshape(H, W).astype(np.float64)
            valid &= np.isfinite(s)
            hh = np.maximum(h, 1).astype(np.float64)
            mean = np.maximum(s / hh, 1e-30)
            F[..., 6] = np.where(h > 0, np.log(mean) / sig[2], 0.0)
            if qz is not None:
                k = nf / hh
                VZ = np.where(h > 0, var(s, qz) * (k * k) / (mean * mean), 0.0)
                F[..., 9] = np.sqrt(VZ) / sig[2]
        F16 = np.clip(F.astype(np.float32).astype(np.float16), np.float16(-65504), np.float16(65504))
    F16[~valid] = 0
    return F16, valid


def nlm_guided_moments_reference(rgb_sum, sq_sum, counts_or_n, m, feature_samples, albedo_sum=None, normal_sum=None, depth_sum=None, hits=None,
                                 albedo_sq_sum=None, normal_sq_sum=None, depth_sq_sum=None, sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0,
                                 variance_strength=0.0, **opts):
    """The variance-guided filter of include/rt_hip.h restated: nlm_reference with
    g(p,q) = sum_j max(|F_j,p - F_j,q|^2 - (V_j,p + min(V_j,p, V_j,q)), 0) / (1 + kappa (V_j,p + V_j,q)) over the groups albedo, normal,
    depth (V = the squared binary16 standard error) added to max(d, 0) in the weight; f64 (H, W, 3). window_radius 0 or absent means 8,
    and 8 is the most. A pixel the guide makes invalid is invalid for the colour part too."""
    opts = dict(opts)
    if not opts.get("window_radius"):
        opts["window_radius"] = MOMENTS_MAX_WINDOW_RADIUS
    if int(opts["window_radius"]) > MOMENTS_MAX_WINDOW_RADIUS:
        raise ValueError("window_radius is above RT_DENOISE_GUIDED_MOMENTS_MAX_WINDOW_RADIUS (8)")
    kappa = float(variance_strength) if variance_strength else GUIDE_MOMENTS_DEFAULTS["variance_strength"]
    kappa = float(np.float32(kappa))                                                    # the kernel's argument is f32
    u32, v32, valid = nlm_prepare(rgb_sum, sq_sum, counts_or_n, m)
    F, ok = guide_moments_prepare(feature_samples, albedo_sum, normal_sum, depth_sum, hits, albedo_sq_sum, normal_sq_sum, depth_sq_sum, sigma_albedo, sigma_normal,
                                  sigma_depth)
    if ok.shape != valid.shape:
        raise ValueError("the feature planes have another size than the frame")
    valid = valid & ok
    v32 = v32.copy(); v32[~valid] = 0.0
    return _filter(u32, v32, valid, opts, guide=F, kappa=kappa)


def render_guide(ctx, scene, cam, params, feature_samples, sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0, moments=False, variance_strength=0.0):
    """A feature pass of `feature_samples` samples per pixel over the frame's camera rays (Context.render_features, device tensors) as
    the `guide` of denoise_frame: full-frame planes; a sharded frame's planes are untiled as its sums are, the other shards' pixels 0.
    moments: the pass is Context.render_feature_moments and the guide carries the squared sums and variance_strength too — what
    denoise_frame hands to rt_denoise_guided_moments_device."""
    prm = A.RtParams.from_buffer_copy(params)
    prm.samples_per_pixel = int(feature_samples)
    prm.flags &= A.RT_FLAG_TIMING | A.RT_FLAG_SAMPLE_BLOCKS      # (a feature pass refuses the counter and the fused-kernel diagnostics)
    planes = ctx.render_feature_moments(scene, cam, prm) if moments else ctx.render_features(scene, cam, prm)
    if prm.shard_count > 1:
        planes = tuple(on_device(in_place(prm, t.cpu().numpy(), ch), t.device) for t, ch in zip(planes, (3, 3, 1, 1, 3, 3, 1)))
    guide = dict(feature_samples=int(feature_samples), albedo=planes[0], normal=planes[1], depth=planes[2], hits=planes[3],
                 sigma_albedo=sigma_albedo, sigma_normal=sigma_normal, sigma_depth=sigma_depth)
    if moments:
        guide.update(albedo_sq=planes[4], normal_sq=planes[5], depth_sq=planes[6], variance_strength=variance_strength)
    return guide


def denoise_frame(ctx, rgb_sum, sq_sum, width, height, samples_per_item, samples=0, counts=None, rgb8=False, guide=None, **opts):
    """rt_denoise_device on full-frame device tensors — with `guide` (Context.denoise_guided's feature arguments, as render_guide
    returns them) rt_denoise_guided_device, or rt_denoise_guided_moments_device when the guide carries squared sums; the f32 mean (H, W, 3) on the host, or with rgb8 its write_color bytes (rt_resolve_device
    with one sample per pixel: the library's only tone map)."""
    import torch
    o = denoise_options(samples_per_item=samples_per_item, **opts)
    if guide is None:
        out = ctx.denoise(rgb_sum, sq_sum, width, height, samples=samples, counts=counts, options=o)
    elif "albedo_sq" in guide:
        out = ctx.denoise_guided_moments(rgb_sum, sq_sum, width, height, samples=samples, counts=counts, options=o, **guide)
    else:
        out = ctx.denoise_guided(rgb_sum, sq_sum, width, height, samples=samples, counts=counts, options=o, **guide)
    if not rgb8:
        return out.cpu().numpy().reshape(height, width, 3)
    b = torch.empty(height * width * 3, dtype=torch.uint8, device=out.device)
    ctx.resolve_device(out.data_ptr(), width, height, 1, b.data_ptr())
    return b.cpu().numpy().reshape(height, width, 3)
