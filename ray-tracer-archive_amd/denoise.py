"""Denoising of low-sample frames: non-local means over the sample variance (include/rt_hip.h, "denoising").

nlm_reference restates the filter in numpy — the prepare step in f64 rounded to f32, the filter step in f64 from those f32 planes — and is
what the device kernels (csrc/denoise.hip, f32) are tested against. denoise_frame is the device path behind Progressive.denoised() and
Adaptive.denoised().
"""
import numpy as np

DEFAULTS = dict(window_radius=10, patch_radius=3, strength=0.45, alpha=1.0, eps=1e-10)


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


def nlm_reference(rgb_sum, sq_sum, counts_or_n, m, **opts):
    """The filter of include/rt_hip.h restated: the filtered mean radiance, f64 (H, W, 3). opts: window_radius, patch_radius, strength,
    alpha, eps (0 or absent: the default). Every sum is taken directly, term by term, in f64."""
    r, f, kk, alpha, eps = _options(opts)
    u32, v32, valid = nlm_prepare(rgb_sum, sq_sum, counts_or_n, m)
    H, W = valid.shape
    pad = r + f
    u = np.zeros((H + 2 * pad, W + 2 * pad, 3)); v = np.zeros_like(u); ok = np.zeros((H + 2 * pad, W + 2 * pad), dtype=bool)
    u[pad:pad + H, pad:pad + W] = u32; v[pad:pad + H, pad:pad + W] = v32; ok[pad:pad + H, pad:pad + W] = valid
    u = np.where(ok[..., None], u, 0.0)          # an invalid pixel's u may be non-finite: it takes part in nothing
    Ha, Wa = H + 2 * f, W + 2 * f                  # the pixels p + o

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
                w = np.where(pair, np.exp(-np.maximum(d, 0.0)), 0.0)
                sw += w
                swu += w[..., None] * uq
        out = swu / np.where(sw > 0, sw, 1.0)[..., None]
    return np.where(valid[..., None], out, u32.astype(np.float64))


def denoise_frame(ctx, rgb_sum, sq_sum, width, height, samples_per_item, samples=0, counts=None, rgb8=False, **opts):
    """rt_denoise_device on full-frame device tensors; the f32 mean (H, W, 3) on the host, or with rgb8 its write_color bytes
    (rt_resolve_device with one sample per pixel: the library's only tone map)."""
    import torch
    from .api import denoise_options
    o = denoise_options(samples_per_item=samples_per_item, **opts)
    out = ctx.denoise(rgb_sum, sq_sum, width, height, samples=samples, counts=counts, options=o)
    if not rgb8:
        return out.cpu().numpy().reshape(height, width, 3)
    b = torch.empty(height * width * 3, dtype=torch.uint8, device=out.device)
    ctx.resolve_device(out.data_ptr(), width, height, 1, b.data_ptr())
    return b.cpu().numpy().reshape(height, width, 3)
