"""Adaptive sampling over rt_adaptive_select and rt_render_pass_pixels_device (include/rt_hip.h, "adaptive sampling").

After every pass only the pixels whose standard error is still above the tolerance get more samples. Every pixel keeps its own sample
count; a pixel with n samples holds exactly the sums one rt_render_pass over [0, n) writes for it, so the frame is reproducible bit for
bit, can be saved to an .npz checkpoint and finished later in another process.

    ada = Adaptive(ctx, scene, cam, params, frame_samples=1024, min_samples=32, rel_error=0.01)
    ada.run(pass_samples=32)
    img = ada.rgb8()
"""
import time

import numpy as np

from . import _abi as A
from .api import adaptive_check, adaptive_options, output_floats, pass_check
from .progressive import CHECKPOINT_VERSION, camera_array, check_checkpoint, denoise_front, on_device, params_array, params_from_array

KIND = "adaptive"
ADAPTIVE_VERSION = 1


def slot_pixels(params):
    """Pixel (x, y) of every output slot of the rgb_sum layout (full frame, or this shard's tiles back to back) and whether it lies in
    the image (clipped slots of edge tiles do not)."""
    W, H = int(params.width), int(params.height)
    slots = output_floats(params) // 3
    s = np.arange(slots, dtype=np.int64)
    if params.shard_count <= 1:
        return s % W, s // W, np.ones(slots, dtype=bool)
    ts = int(params.tile_size) or 32
    tiles_x = -(-W // ts)
    lt, r = s // (ts * ts), s % (ts * ts)
    tile = int(params.shard_index) + lt * int(params.shard_count)
    x, y = (tile % tiles_x) * ts + r % ts, (tile // tiles_x) * ts + r // ts
    return x, y, (x < W) & (y < H)


def select_reference(rgb_sum, sq_sum, counts, first_sample, frame_samples, m, opts, valid=None):
    """The active list of rt_adaptive_select restated in numpy, op for op (f64): ascending slots p with counts[p] == first_sample <
    frame_samples that are below opts.min_samples or not converged. rgb_sum / sq_sum: 3 floats per slot; counts: one per slot; valid:
    which slots are image pixels (None: all)."""
    S3 = np.asarray(rgb_sum, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    Q3 = np.asarray(sq_sum, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    c = np.asarray(counts).reshape(-1).astype(np.int64)
    m = int(m)
    cand = c == int(first_sample)
    if int(first_sample) >= int(frame_samples):
        cand[:] = False
    if valid is not None:
        cand &= np.asarray(valid, dtype=bool).reshape(-1)
    items = -(-c // m)
    k = items.astype(np.float64)[:, None]
    n = c.astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        d = Q3 - S3 * S3 / k
        d = np.where(d > 0.0, d, 0.0)
        var = d / (k * (k - 1.0))
        tol = float(opts.abs_error) + float(opts.rel_error) * np.abs(S3 / n)
        conv = (var / (float(m) * float(m))) <= tol * tol
    conv &= np.isfinite(S3) & np.isfinite(Q3)
    converged = conv.all(axis=1) & (items >= 2)
    active = cand & ((c < int(opts.min_samples)) | ~converged)
    return np.nonzero(active)[0].astype(np.uint32)


def check_counts(counts, slots, frame_samples, samples_done=None):
    """The per-pixel sample counts of a checkpoint: one non-negative integer per output slot, none above frame_samples (nor above
    samples_done, the pass the frame has reached). Pure host code: raises ValueError, returns the counts as uint32."""
    c = np.asarray(counts)
    if c.shape != (int(slots),):
        raise ValueError(f"counts have shape {c.shape}, expected ({int(slots)},)")
    if c.dtype.kind not in "iu":
        raise ValueError(f"counts are {c.dtype}, not integers")
    c64 = c.astype(np.int64)
    if c64.size and c64.min() < 0:
        raise ValueError("a count is negative")
    top = int(frame_samples) if samples_done is None else min(int(frame_samples), int(samples_done))
    if c64.size and c64.max() > top:
        raise ValueError(f"a count ({int(c64.max())}) is above {top} samples")
    return c64.astype(np.uint32)


def check_adaptive_checkpoint(meta, params=None, frame_samples=None, cam=None, fingerprint=None):
    """An adaptive checkpoint's metadata and counts against what the caller resumes it with (None: not compared). Raises ValueError."""
    if str(np.asarray(meta.get("kind", ""))) != KIND:
        raise ValueError("not an adaptive-sampling checkpoint (kind)")
    if "adaptive_version" not in meta or int(np.asarray(meta["adaptive_version"])) != ADAPTIVE_VERSION:
        raise ValueError(f"adaptive checkpoint version differs from {ADAPTIVE_VERSION}")
    common = dict(meta)
    common["version"] = np.int64(CHECKPOINT_VERSION)          # the fields both checkpoint kinds share: progressive.check_checkpoint
    check_checkpoint(common, params=params, frame_samples=frame_samples, cam=cam, fingerprint=fingerprint)
    for k in ("params", "min_samples", "rel_error", "abs_error", "rgb_sum", "sq_sum", "counts"):
        if k not in meta:
            raise ValueError(f"checkpoint has no '{k}'")
    prm = params_from_array(np.asarray(meta["params"]), int(np.asarray(meta["frame_samples"])))
    slots = output_floats(prm) // 3
    for k in ("rgb_sum", "sq_sum"):
        if np.asarray(meta[k]).shape != (3 * slots,):
            raise ValueError(f"checkpoint {k} has another size than the frame")
    check_counts(meta["counts"], slots, int(np.asarray(meta["frame_samples"])), int(np.asarray(meta["samples_done"])))


class Adaptive:
    """A frame rendered in passes over the pixels that are still noisy, into device buffers owned by this object (torch tensors)."""

    def __init__(self, ctx, scene, cam, params, frame_samples, min_samples=None, rel_error=0.01, abs_error=0.0):
        import torch
        self.ctx, self.scene, self.cam = ctx, scene, cam
        self.params = A.RtParams.from_buffer_copy(params)
        self.frame_samples = int(frame_samples)
        self.params.samples_per_pixel = self.frame_samples
        self.samples_per_item = pass_check(self.params, 0, self.frame_samples)
        m = self.samples_per_item
        self.options = adaptive_options(2 * m if min_samples is None else min_samples, rel_error, abs_error)
        adaptive_check(self.params, self.options, 0, self.frame_samples)
        self.fingerprint = scene.fingerprint
        self.slots = output_floats(self.params) // 3
        dev = torch.device("cuda", ctx.device_id)
        self._rgb = torch.zeros(3 * self.slots, dtype=torch.float32, device=dev)
        self._sq = torch.zeros(3 * self.slots, dtype=torch.float32, device=dev)
        self._counts = torch.zeros(self.slots, dtype=torch.int32, device=dev)
        self._list = torch.zeros(self.slots, dtype=torch.int32, device=dev)
        self.samples_done = 0            # first_sample of the next pass: the count every active pixel holds
        self.n_active = None             # length of the last selected list (None: not selected yet)
        self.samples_traced = 0          # over all passes of this object (a loaded checkpoint starts from its counts' sum)
        self.last_stats = None

    @property
    def min_samples(self):
        return int(self.options.min_samples)

    def select(self):
        """rt_adaptive_select for the next pass; returns the list's length (the list itself stays on the device)."""
        self.n_active = self.ctx.adaptive_select(self.params, self.options, self.samples_done, self.frame_samples, self._rgb, self._sq, self._counts, self._list)
        return self.n_active

    def active_list(self):
        """The last selected list, as ascending uint32 slots (host copy)."""
        return self._list[:self.n_active or 0].cpu().numpy().view(np.uint32).copy()

    @property
    def done(self):
        return self.n_active == 0 or self.samples_done >= self.frame_samples

    def step(self, n):
        """Selects, then renders the next `n` samples (fewer at the end of the frame) of the selected pixels. Returns the pass's stats, or
        None once no pixel is active."""
        n = min(int(n), self.frame_samples - self.samples_done)
        if n <= 0 or self.select() == 0:
            return None
        prm = A.RtParams.from_buffer_copy(self.params)
        prm.samples_per_pixel = n
        st = self.ctx.render_pass_pixels(self.scene, self.cam, prm, self.samples_done, self.frame_samples, self.samples_done > 0, self._list, self.n_active,
                                         self._rgb, self._sq, self._counts)
        self.samples_done += n
        self.samples_traced += st["samples"]
        self.last_stats = st
        return st

    def run(self, pass_samples, until=None, seconds=None, callback=None):
        """Passes of `pass_samples` until no pixel is active, or the active pixels hold `until` samples, or `seconds` of wall time.
        callback(self, stats) after every pass; returning False from it stops the loop. Returns samples_done."""
        target = self.frame_samples if until is None else min(int(until), self.frame_samples)
        t0 = time.monotonic()
        while self.samples_done < target:
            st = self.step(min(int(pass_samples), target - self.samples_done))
            if st is None:
                break
            if callback is not None and callback(self, st) is False:
                break
            if seconds is not None and time.monotonic() - t0 >= seconds:
                break
        return self.samples_done

    # ---- the frame ----
    def _flat_counts(self):
        return self._counts.cpu().numpy().view(np.uint32)

    def _in_place(self, flat, channels):
        """slot-ordered values -> (H, W[, channels]); a sharded frame: this shard's tiles in place, other pixels 0."""
        p = self.params
        if p.shard_count <= 1:
            return flat.reshape((p.height, p.width, channels) if channels > 1 else (p.height, p.width))
        x, y, ok = slot_pixels(p)
        out = np.zeros((p.height, p.width, channels) if channels > 1 else (p.height, p.width), dtype=flat.dtype)
        out[y[ok], x[ok]] = flat.reshape(-1, channels)[ok] if channels > 1 else flat[ok]
        return out

    def counts(self):
        """Samples per pixel, uint32 (H, W)."""
        return self._in_place(self._flat_counts(), 1)

    def rgb_sum(self):
        return self._in_place(self._rgb.cpu().numpy(), 3)

    def sq_sum(self):
        return self._in_place(self._sq.cpu().numpy(), 3)

    def mean(self):
        """Per-pixel mean radiance, f64 (H, W, 3); 0 where a pixel holds no sample."""
        c = self.counts().astype(np.float64)[..., None]
        with np.errstate(all="ignore"):
            return np.where(c > 0, self.rgb_sum().astype(np.float64) / c, 0.0)

    def std_error(self):
        """Standard error of every pixel mean, f64 (H, W, 3), with the pixel's own k = counts / m items; inf below two items."""
        m = self.samples_per_item
        k = (-(-self.counts().astype(np.int64) // m)).astype(np.float64)[..., None]
        S, Q = self.rgb_sum().astype(np.float64), self.sq_sum().astype(np.float64)
        with np.errstate(all="ignore"):
            var = np.maximum(Q - S * S / k, 0.0) / (k * (k - 1.0))
            se = np.sqrt(var) / m
        return np.where(k >= 2, se, np.inf)

    def rgb8(self):
        """write_color with every pixel's own count (rt_resolve_counts_device): uint8 (H, W, 3)."""
        import torch
        p = self.params
        dev = self._rgb.device
        if p.shard_count <= 1:
            rgb, cnt = self._rgb, self._counts
        else:
            rgb, cnt = on_device(self.rgb_sum(), dev), on_device(self.counts().view(np.int32), dev)
        out = torch.empty(p.height * p.width * 3, dtype=torch.uint8, device=dev)
        self.ctx.resolve_counts_device(rgb, cnt, p.width, p.height, out)
        return out.cpu().numpy().reshape(p.height, p.width, 3)

    def denoised(self, rgb8=False, feature_samples=0, sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0, feature_variance=False, variance_strength=0.0, **opts):
        """The frame filtered by rt_denoise_device with every pixel's own count (opts: denoise_options fields): the mean radiance, f32
        (H, W, 3), or its write_color bytes with rgb8=True. A pixel below two work items is copied through; a sharded frame is untiled first.
        feature_samples = N > 0: a feature pass of N samples per pixel is rendered (Context.render_features) and the weights are joined
        with it (rt_denoise_guided_device; the sigmas: RtDenoiseGuide, 0 = the default). 0: the plain filter.
        feature_variance=True with feature_samples = N >= 2: the pass keeps the features' second moments (Context.render_feature_moments)
        and the filter is rt_denoise_guided_moments_device (sigmas and variance_strength: RtDenoiseGuideMoments, 0 = the default;
        window_radius 0 = 8, at most 8)."""
        from .denoise import denoise_frame
        p = self.params
        rgb, sq, sharded = denoise_front(self, opts, feature_samples, sigma_albedo, sigma_normal, sigma_depth, feature_variance, variance_strength)
        cnt = on_device(self.counts().view(np.int32), rgb.device) if sharded else self._counts
        return denoise_frame(self.ctx, rgb, sq, p.width, p.height, self.samples_per_item, counts=cnt, rgb8=rgb8, **opts)

    def features(self, samples):
        """First-hit features of this frame's camera rays (rt_render_features_device), from a pass of its own of `samples` samples per pixel
        — uniform, independent of the radiance samples held: (albedo (H, W, 3), normal (H, W, 3), depth (H, W), hit fraction (H, W)), f32
        means; normal and depth over the samples that hit. A sharded frame is untiled first."""
        from .features import feature_means
        return feature_means(self.ctx, self.scene, self.cam, self.params, samples)

    # ---- checkpoints ----
    def save(self, path):
        """An .npz checkpoint: sums, counts, samples_done, frame_samples, the options, the RtParams fields, the camera and the scene."""
        np.savez(path, kind=np.array(KIND), adaptive_version=np.int64(ADAPTIVE_VERSION), samples_done=np.int64(self.samples_done),
                 frame_samples=np.int64(self.frame_samples), min_samples=np.int64(self.min_samples), rel_error=np.float64(self.options.rel_error),
                 abs_error=np.float64(self.options.abs_error), params=params_array(self.params), camera=camera_array(self.cam),
                 fingerprint=np.array(self.fingerprint), rgb_sum=self._rgb.cpu().numpy(), sq_sum=self._sq.cpu().numpy(), counts=self._flat_counts())

    @classmethod
    def load(cls, path, ctx, scene, cam, params=None):
        """Resumes a checkpoint on `ctx` with `scene` and `cam` (and, if given, `params`). ValueError when anything does not match."""
        import torch
        with np.load(path) as f:
            z = {k: f[k] for k in f.files}
        check_adaptive_checkpoint(z, params=params, cam=cam, fingerprint=scene.fingerprint)
        prm = params_from_array(z["params"], int(z["frame_samples"]))
        ada = cls(ctx, scene, cam, prm, int(z["frame_samples"]), min_samples=int(z["min_samples"]), rel_error=float(z["rel_error"]),
                  abs_error=float(z["abs_error"]))
        ada._rgb.copy_(torch.from_numpy(z["rgb_sum"]))
        ada._sq.copy_(torch.from_numpy(z["sq_sum"]))
        ada._counts.copy_(torch.from_numpy(z["counts"].astype(np.uint32).view(np.int32)))
        torch.cuda.synchronize(ada._rgb.device)
        ada.samples_done = int(z["samples_done"])
        ada.samples_traced = int(z["counts"].astype(np.int64).sum())
        return ada
