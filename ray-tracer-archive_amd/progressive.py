"""Progressive, resumable rendering over rt_render_pass_device (include/rt_hip.h, "progressive rendering").

A frame of `frame_samples` samples per pixel is rendered as a series of sample passes into device accumulators (torch tensors): the
per-pixel RGB sums and, optionally, the sums of the squared work-item sums, from which the standard error of every pixel follows.
Passes that cover [0, N) leave exactly what one rt_render at N samples per pixel writes, so a frame can be previewed, stopped once it is
good enough, saved to an .npz checkpoint and finished later in another process, bit for bit as if rendered at once.

    prog = Progressive(ctx, scene, cam, params, frame_samples=1024)
    prog.run(pass_samples=64, seconds=30, rel_se=0.01)
    prog.save("frame.npz")
    ...
    prog = Progressive.load("frame.npz", ctx, scene, cam)
    prog.run(pass_samples=64)
"""
import time

import numpy as np

from . import _abi as A
from .api import output_floats, pass_check, untile

CHECKPOINT_VERSION = 1
# every RtParams field but samples_per_pixel (a pass sets its own) and the padding
PARAM_FIELDS = ("width", "height", "max_depth", "seed", "nan_policy", "flags", "tile_size", "shard_index", "shard_count", "pool_slots", "tail_paths")


def params_array(params):
    return np.array([int(getattr(params, f)) for f in PARAM_FIELDS], dtype=np.uint64)


def camera_array(cam):
    v = []
    for f in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w"):
        v.extend(getattr(cam, f).tuple())
    v.extend([cam.lens_radius, cam.time0, cam.time1])
    return np.array(v, dtype=np.float64)


def params_from_array(a, samples_per_pixel=1):
    p = A.RtParams()
    for f, x in zip(PARAM_FIELDS, a):
        setattr(p, f, int(x))
    p.samples_per_pixel = samples_per_pixel
    return p


def check_checkpoint(meta, params=None, frame_samples=None, cam=None, fingerprint=None):
    """Checks a checkpoint's metadata (a mapping such as np.load's result) against what the caller is about to resume it with; every
    argument left None is not compared. Pure host code: raises ValueError naming what differs, returns None when it all matches."""
    def get(k):
        if k not in meta:
            raise ValueError(f"checkpoint has no '{k}'")
        return np.asarray(meta[k])

    if int(get("version")) != CHECKPOINT_VERSION:
        raise ValueError(f"checkpoint version {int(get('version'))}, expected {CHECKPOINT_VERSION}")
    done, frame = int(get("samples_done")), int(get("frame_samples"))
    if not 0 <= done <= frame:
        raise ValueError(f"checkpoint holds {done} samples of a {frame}-sample frame")
    if frame_samples is not None and frame != int(frame_samples):
        raise ValueError(f"checkpoint frame_samples {frame} differs from {int(frame_samples)}")
    if params is not None:
        mine, theirs = get("params"), params_array(params)
        if mine.shape != theirs.shape:
            raise ValueError("checkpoint params have another shape")
        for f, a, b in zip(PARAM_FIELDS, mine, theirs):
            if a != b:
                raise ValueError(f"checkpoint params.{f} = {int(a)} differs from {int(b)}")
    if cam is not None and not np.array_equal(get("camera"), camera_array(cam)):
        raise ValueError("checkpoint camera differs")
    if fingerprint is not None and str(get("fingerprint")) != str(fingerprint):
        raise ValueError("checkpoint scene differs (scene description fingerprint)")


def std_error(rgb_sum, sq_sum, samples, samples_per_item):
    """Standard error of every pixel mean, f64 (include/rt_hip.h): SE = sqrt((Q - S^2/k) / (k (k - 1))) / m with k items of m
    samples; the variance is clamped at 0 (f32 cancellation in near-constant pixels). inf where fewer than two items are folded."""
    m = int(samples_per_item)
    k = -(-int(samples) // m)
    S = np.asarray(rgb_sum, dtype=np.float64)
    if k < 2:
        return np.full(S.shape, np.inf)
    Q = np.asarray(sq_sum, dtype=np.float64)
    var = np.maximum(Q - S * S / k, 0.0) / (k * (k - 1.0))
    return np.sqrt(var) / m


def on_device(a, dev):
    """A host array (an untiled plane of sums or counts) as a flat tensor on `dev`."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev)


def denoise_front(frame, opts, feature_samples, sigma_albedo, sigma_normal, sigma_depth, feature_variance, variance_strength):
    """The front of Progressive.denoised and Adaptive.denoised: the argument check, the guide of a feature pass of the frame's camera rays
    (into opts["guide"]), and the frame's sums as full-frame device tensors — its own, or for a sharded frame its untiled ones. Returns
    (rgb_sum, sq_sum, sharded)."""
    from .denoise import render_guide
    if feature_variance and int(feature_samples) < 2:
        raise ValueError("feature_variance needs feature_samples >= 2")
    p, dev = frame.params, frame._rgb.device
    if feature_samples:
        opts["guide"] = render_guide(frame.ctx, frame.scene, frame.cam, p, feature_samples, sigma_albedo, sigma_normal, sigma_depth, moments=bool(feature_variance),
                                     variance_strength=variance_strength)
    if p.shard_count <= 1:
        return frame._rgb, frame._sq, False
    return on_device(frame.rgb_sum(), dev), on_device(frame.sq_sum(), dev), True


class Progressive:
    """A frame rendered in passes into device accumulators owned by this object (torch tensors on the context's GPU)."""

    def __init__(self, ctx, scene, cam, params, frame_samples, sq_sum=True):
        import torch
        self.ctx, self.scene, self.cam = ctx, scene, cam
        self.params = A.RtParams.from_buffer_copy(params)
        self.frame_samples = int(frame_samples)
        self.params.samples_per_pixel = self.frame_samples
        self.samples_per_item = pass_check(self.params, 0, self.frame_samples)     # validates the frame; m of every pass
        self.fingerprint = scene.fingerprint
        n = output_floats(self.params)
        dev = torch.device("cuda", ctx.device_id)
        self._rgb = torch.zeros(n, dtype=torch.float32, device=dev)
        self._sq = torch.zeros(n, dtype=torch.float32, device=dev) if sq_sum else None
        self.samples_done = 0
        self.last_stats = None

    @property
    def done(self):
        return self.samples_done >= self.frame_samples

    def step(self, n):
        """Renders the next `n` samples per pixel (fewer at the end of the frame). Returns the pass's stats (None: the frame is done)."""
        n = min(int(n), self.frame_samples - self.samples_done)
        if n <= 0:
            return None
        prm = A.RtParams.from_buffer_copy(self.params)
        prm.samples_per_pixel = n
        _, _, st = self.ctx.render_pass(self.scene, self.cam, prm, self.samples_done, self.frame_samples, self.samples_done > 0, self._rgb, self._sq)
        self.samples_done += n
        self.last_stats = st
        return st

    def run(self, pass_samples, until=None, seconds=None, rel_se=None, callback=None):
        """Passes of `pass_samples` until `until` samples per pixel (default: the whole frame), or `seconds` of wall time, or a relative
        error (relative_error()) of at most `rel_se`, whichever comes first. callback(self, stats) is called after every pass; returning
        False from it stops the loop. Returns samples_done."""
        target = self.frame_samples if until is None else min(int(until), self.frame_samples)
        t0 = time.monotonic()
        while self.samples_done < target:
            st = self.step(min(int(pass_samples), target - self.samples_done))
            if callback is not None and callback(self, st) is False:
                break
            if seconds is not None and time.monotonic() - t0 >= seconds:
                break
            if rel_se is not None and self.relative_error() <= rel_se:
                break
        return self.samples_done

    def _untiled(self, flat):
        p = self.params
        if p.shard_count <= 1:
            return flat.reshape(p.height, p.width, 3)
        # this shard's tiles in place, the other shards' pixels 0
        q = A.RtParams.from_buffer_copy(p)
        q.shard_index = 0
        per = output_floats(q)
        g = np.zeros(per * p.shard_count, dtype=np.float32)
        g[p.shard_index * per:p.shard_index * per + flat.size] = flat
        return untile(p, g)

    def rgb_sum(self):
        """Per-pixel RGB sums over samples_done samples, f32 (H, W, 3) (a sharded frame: this shard's tiles in place, 0 elsewhere)."""
        return self._untiled(self._rgb.cpu().numpy())

    def sq_sum(self):
        if self._sq is None:
            raise ValueError("this frame keeps no squared sums (sq_sum=False)")
        return self._untiled(self._sq.cpu().numpy())

    def std_error(self):
        """Standard error of every pixel's mean radiance, f64 (H, W, 3)."""
        return std_error(self.rgb_sum(), self.sq_sum(), self.samples_done, self.samples_per_item)

    def relative_error(self):
        """RMS of the per-pixel standard error over the frame's pixels, relative to the frame's mean radiance (inf before two items)."""
        se = self.std_error()
        if not np.isfinite(se).all():
            return float("inf")
        mean = float(np.mean(self.rgb_sum(), dtype=np.float64)) / max(self.samples_done, 1)
        return float(np.sqrt(np.mean(se * se))) / mean if mean > 0 else float("inf")

    def rgb8(self):
        """write_color of the frame so far (rt_resolve_device with samples_done samples): uint8 (H, W, 3)."""
        import torch
        if self.samples_done == 0:
            raise ValueError("no samples rendered yet")
        p = self.params
        dev = self._rgb.device
        src = self._rgb if p.shard_count <= 1 else on_device(self.rgb_sum(), dev)
        out = torch.empty(p.height * p.width * 3, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        self.ctx.resolve_device(src.data_ptr(), p.width, p.height, self.samples_done, out.data_ptr())
        return out.cpu().numpy().reshape(p.height, p.width, 3)

    def denoised(self, rgb8=False, feature_samples=0, sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0, feature_variance=False, variance_strength=0.0, **opts):
        """The frame so far filtered by rt_denoise_device (non-local means over the sample variance; opts: denoise_options fields, the
        frame's samples per work item is filled in): the mean radiance, f32 (H, W, 3), or its write_color bytes with rgb8=True. A
        sharded frame is untiled first: the other shards' pixels hold no sums and come out as they are, 0.
        feature_samples = N > 0: a feature pass of N samples per pixel is rendered (Context.render_features) and the weights are joined
        with it (rt_denoise_guided_device; the sigmas: RtDenoiseGuide, 0 = the default). 0: the plain filter.
        feature_variance=True with feature_samples = N >= 2: the pass keeps the features' second moments (Context.render_feature_moments)
        and the filter is rt_denoise_guided_moments_device (sigmas and variance_strength: RtDenoiseGuideMoments, 0 = the default;
        window_radius 0 = 8, at most 8)."""
        from .denoise import denoise_frame
        if self.samples_done == 0:
            raise ValueError("no samples rendered yet")
        if self._sq is None:
            raise ValueError("this frame keeps no squared sums (sq_sum=False)")
        p = self.params
        rgb, sq, sharded = denoise_front(self, opts, feature_samples, sigma_albedo, sigma_normal, sigma_depth, feature_variance, variance_strength)
        if not sharded:
            return denoise_frame(self.ctx, rgb, sq, p.width, p.height, self.samples_per_item, samples=self.samples_done, rgb8=rgb8, **opts)
        from .adaptive import slot_pixels
        x, y, ok = slot_pixels(p)
        cnt = np.zeros((p.height, p.width), dtype=np.int32)          # the other shards' pixels hold no sample: nobody's neighbours
        cnt[y[ok], x[ok]] = self.samples_done
        return denoise_frame(self.ctx, rgb, sq, p.width, p.height, self.samples_per_item, counts=on_device(cnt, rgb.device), rgb8=rgb8, **opts)

    def features(self, samples):
        """First-hit features of this frame's camera rays (rt_render_features_device), from a pass of its own of `samples` samples per pixel
        — uniform, independent of the radiance samples held: (albedo (H, W, 3), normal (H, W, 3), depth (H, W), hit fraction (H, W)), f32
        means; normal and depth over the samples that hit. A sharded frame is untiled first."""
        from .features import feature_means
        return feature_means(self.ctx, self.scene, self.cam, self.params, samples)

    def save(self, path):
        """An .npz checkpoint: the sums, samples_done, frame_samples, the RtParams fields, the camera and the scene fingerprint."""
        z = dict(version=np.int64(CHECKPOINT_VERSION), samples_done=np.int64(self.samples_done), frame_samples=np.int64(self.frame_samples),
                 params=params_array(self.params), camera=camera_array(self.cam), fingerprint=np.array(self.fingerprint),
                 rgb_sum=self._rgb.cpu().numpy())
        if self._sq is not None:
            z["sq_sum"] = self._sq.cpu().numpy()
        np.savez(path, **z)

    @classmethod
    def load(cls, path, ctx, scene, cam, params=None):
        """Resumes a checkpoint on `ctx` with `scene` and `cam` (and, if given, `params`). ValueError when the camera, the scene
        description, the params or the buffers do not match the checkpoint's."""
        import torch
        with np.load(path) as f:
            z = {k: f[k] for k in f.files}
        check_checkpoint(z, params=params, cam=cam, fingerprint=scene.fingerprint)
        prm = params_from_array(z["params"], int(z["frame_samples"]))
        prog = cls(ctx, scene, cam, prm, int(z["frame_samples"]), sq_sum="sq_sum" in z)
        if z["rgb_sum"].shape != tuple(prog._rgb.shape):
            raise ValueError("checkpoint sums have another size than the frame")
        prog._rgb.copy_(torch.from_numpy(z["rgb_sum"]))
        if prog._sq is not None:
            prog._sq.copy_(torch.from_numpy(z["sq_sum"]))
        torch.cuda.synchronize(prog._rgb.device)
        prog.samples_done = int(z["samples_done"])
        return prog
