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
from .api import output_floats, pass_check
from .denoise import denoise_frame, render_guide
from .features import feature_means
from .layout import in_place, on_device

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


def read_checkpoint(path):
    """The arrays of an .npz checkpoint as a dict."""
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def std_error(rgb_sum, sq_sum, samples, samples_per_item):
    """Standard error of every pixel mean, f64 (include/rt_hip.h): SE = sqrt((Q - S^2/k) / (k (k - 1))) / m with k items of m
    samples; the variance is clamped at 0 (f32 cancellation in near-constant pixels). samples: the frame's one count, or an (H, W) plane
    of every pixel's own. inf where fewer than two items are folded."""
    m = int(samples_per_item)
    k = (-(-np.asarray(samples, dtype=np.int64) // m)).astype(np.float64)
    if k.ndim:
        k = k[..., None]
    S, Q = np.asarray(rgb_sum, dtype=np.float64), np.asarray(sq_sum, dtype=np.float64)
    with np.errstate(all="ignore"):
        var = np.maximum(Q - S * S / k, 0.0) / (k * (k - 1.0))
        se = np.sqrt(var) / m
    return np.where(k >= 2, se, np.inf)


class Frame:
    """What Progressive and Adaptive share: the frame's description, its device accumulators (torch tensors on the context's GPU, owned
    by this object) and what follows from the sums alone. A subclass renders the passes (step) and knows the samples every pixel holds."""

    def __init__(self, ctx, scene, cam, params, frame_samples, sq_sum=True):
        import torch
        self.ctx, self.scene, self.cam = ctx, scene, cam
        self.params = A.RtParams.from_buffer_copy(params)
        self.frame_samples = int(frame_samples)
        self.params.samples_per_pixel = self.frame_samples
        self.samples_per_item = pass_check(self.params, 0, self.frame_samples)     # validates the frame; m of every pass
        self.fingerprint = scene.fingerprint
        self.slots = output_floats(self.params) // 3
        dev = torch.device("cuda", ctx.device_id)
        self._rgb = torch.zeros(3 * self.slots, dtype=torch.float32, device=dev)
        self._sq = torch.zeros(3 * self.slots, dtype=torch.float32, device=dev) if sq_sum else None
        self.samples_done = 0            # first_sample of the next pass
        self.last_stats = None

    def _passes(self, pass_samples, until, seconds, callback, good_enough=None):
        """The loop of run: passes of `pass_samples` up to `until` samples (None: the whole frame). After every pass, in this order: a step
        that rendered nothing, a callback(self, stats) that returns False, `seconds` of wall time and good_enough() end it."""
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
            if good_enough is not None and good_enough():
                break
        return self.samples_done

    def rgb_sum(self):
        """Per-pixel RGB sums over the samples rendered, f32 (H, W, 3) (a sharded frame: this shard's tiles in place, 0 elsewhere)."""
        return in_place(self.params, self._rgb.cpu().numpy(), 3)

    def sq_sum(self):
        """Per-pixel sums of the squared work-item sums, f32 (H, W, 3), laid out as rgb_sum."""
        if self._sq is None:
            raise ValueError("this frame keeps no squared sums (sq_sum=False)")
        return in_place(self.params, self._sq.cpu().numpy(), 3)

    def denoised(self, rgb8=False, feature_samples=0, sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0, feature_variance=False, variance_strength=0.0, **opts):
        """The frame so far filtered by rt_denoise_device (non-local means over the sample variance, with the samples every pixel holds;
        opts: denoise_options fields, the frame's samples per work item is filled in): the mean radiance, f32 (H, W, 3), or its
        write_color bytes with rgb8=True. A pixel below two work items is copied through. A sharded frame is untiled first: the other
        shards' pixels hold no sums and come out as they are, 0.
        feature_samples = N > 0: a feature pass of N samples per pixel is rendered (Context.render_features) and the weights are joined
        with it (rt_denoise_guided_device; the sigmas: RtDenoiseGuide, 0 = the default). 0: the plain filter.
        feature_variance=True with feature_samples = N >= 2: the pass keeps the features' second moments (Context.render_feature_moments)
        and the filter is rt_denoise_guided_moments_device (sigmas and variance_strength: RtDenoiseGuideMoments, 0 = the default;
        window_radius 0 = 8, at most 8)."""
        samples, counts = self._denoise_counts()
        if self._sq is None:
            raise ValueError("this frame keeps no squared sums (sq_sum=False)")
        if feature_variance and int(feature_samples) < 2:
            raise ValueError("feature_variance needs feature_samples >= 2")
        p, dev = self.params, self._rgb.device
        if feature_samples:
            opts["guide"] = render_guide(self.ctx, self.scene, self.cam, p, feature_samples, sigma_albedo, sigma_normal, sigma_depth, moments=bool(feature_variance),
                                         variance_strength=variance_strength)
        rgb, sq = (self._rgb, self._sq) if p.shard_count <= 1 else (on_device(self.rgb_sum(), dev), on_device(self.sq_sum(), dev))
        return denoise_frame(self.ctx, rgb, sq, p.width, p.height, self.samples_per_item, samples=samples, counts=counts, rgb8=rgb8, **opts)

    def features(self, samples):
        """First-hit features of this frame's camera rays (rt_render_features_device), from a pass of its own of `samples` samples per pixel
        — uniform, independent of the radiance samples held: (albedo (H, W, 3), normal (H, W, 3), depth (H, W), hit fraction (H, W)), f32
        means; normal and depth over the samples that hit. A sharded frame is untiled first."""
        return feature_means(self.ctx, self.scene, self.cam, self.params, samples)

    def _checkpoint(self):
        """What both kinds of checkpoint hold: samples_done, frame_samples, the RtParams fields, the camera, the scene fingerprint, the sums."""
        z = dict(samples_done=np.int64(self.samples_done), frame_samples=np.int64(self.frame_samples), params=params_array(self.params),
                 camera=camera_array(self.cam), fingerprint=np.array(self.fingerprint), rgb_sum=self._rgb.cpu().numpy())
        if self._sq is not None:
            z["sq_sum"] = self._sq.cpu().numpy()
        return z

    def _restore(self, z):
        """The sums and samples_done of a checked checkpoint into this frame; the caller waits for the copies."""
        import torch
        self._rgb.copy_(torch.from_numpy(z["rgb_sum"]))
        if self._sq is not None:
            self._sq.copy_(torch.from_numpy(z["sq_sum"]))
        self.samples_done = int(z["samples_done"])


class Progressive(Frame):
    """A frame rendered in passes into device accumulators owned by this object (torch tensors on the context's GPU); sq_sum=False keeps
    no squared sums, and with them no standard error and no denoised()."""

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
        return self._passes(pass_samples, until, seconds, callback, None if rel_se is None else lambda: self.relative_error() <= rel_se)

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

    def _denoise_counts(self):
        """(samples, counts) of denoise_frame: samples_done for every pixel; a sharded frame: a plane with it at this shard's pixels, as
        the other shards' pixels hold no sample and are nobody's neighbours."""
        if self.samples_done == 0:
            raise ValueError("no samples rendered yet")
        if self.params.shard_count <= 1:
            return self.samples_done, None
        return 0, on_device(in_place(self.params, np.full(self.slots, self.samples_done, dtype=np.int32), 1), self._rgb.device)

    def save(self, path):
        """An .npz checkpoint: the sums, samples_done, frame_samples, the RtParams fields, the camera and the scene fingerprint."""
        np.savez(path, version=np.int64(CHECKPOINT_VERSION), **self._checkpoint())

    @classmethod
    def load(cls, path, ctx, scene, cam, params=None):
        """Resumes a checkpoint on `ctx` with `scene` and `cam` (and, if given, `params`). ValueError when the camera, the scene
        description, the params or the buffers do not match the checkpoint's."""
        import torch
        z = read_checkpoint(path)
        check_checkpoint(z, params=params, cam=cam, fingerprint=scene.fingerprint)
        prm = params_from_array(z["params"], int(z["frame_samples"]))
        prog = cls(ctx, scene, cam, prm, int(z["frame_samples"]), sq_sum="sq_sum" in z)
        if z["rgb_sum"].shape != tuple(prog._rgb.shape):
            raise ValueError("checkpoint sums have another size than the frame")
        prog._restore(z)
        torch.cuda.synchronize(prog._rgb.device)
        return prog


