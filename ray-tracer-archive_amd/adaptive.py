"""Adaptive sampling over rt_adaptive_select and rt_render_pass_pixels_device (include/rt_hip.h, "adaptive sampling").

After every pass only the pixels whose standard error is still above the tolerance get more samples. Every pixel keeps its own sample
count; a pixel with n samples holds exactly the sums one rt_render_pass over [0, n) writes for it, so the frame is reproducible bit for
bit, can be saved to an .npz checkpoint and finished later in another process.

    ada = Adaptive(ctx, scene, cam, params, frame_samples=1024, min_samples=32, rel_error=0.01)
    ada.run(pass_samples=32)
    img = ada.rgb8()
"""
import numpy as np

from . import _abi as A
from .api import adaptive_check, adaptive_options, output_floats
from .layout import in_place, on_device
from .progressive import CHECKPOINT_VERSION, Frame, check_checkpoint, params_from_array, read_checkpoint, std_error

KIND = "adaptive"
ADAPTIVE_VERSION = 1


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


class Adaptive(Frame):
    """A frame rendered in passes over the pixels that are still noisy, into device buffers owned by this object (torch tensors)."""

    def __init__(self, ctx, scene, cam, params, frame_samples, min_samples=None, rel_error=0.01, abs_error=0.0):
        import torch
        super().__init__(ctx, scene, cam, params, frame_samples)
        self.options = adaptive_options(2 * self.samples_per_item if min_samples is None else min_samples, rel_error, abs_error)
        adaptive_check(self.params, self.options, 0, self.frame_samples)
        self._counts = torch.zeros(self.slots, dtype=torch.int32, device=self._rgb.device)
        self._list = torch.zeros(self.slots, dtype=torch.int32, device=self._rgb.device)
        self.n_active = None             # length of the last selected list (None: not selected yet)
        self.samples_traced = 0          # over all passes of this object (a loaded checkpoint starts from its counts' sum)

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
        self.samples_done += n           # the count every active pixel holds
        self.samples_traced += st["samples"]
        self.last_stats = st
        return st

    def run(self, pass_samples, until=None, seconds=None, callback=None):
        """Passes of `pass_samples` until no pixel is active, or the active pixels hold `until` samples, or `seconds` of wall time.
        callback(self, stats) after every pass; returning False from it stops the loop. Returns samples_done."""
        return self._passes(pass_samples, until, seconds, callback)

    # ---- the frame ----
    def _flat_counts(self):
        return self._counts.cpu().numpy().view(np.uint32)

    def counts(self):
        """Samples per pixel, uint32 (H, W)."""
        return in_place(self.params, self._flat_counts(), 1)

    def mean(self):
        """Per-pixel mean radiance, f64 (H, W, 3); 0 where a pixel holds no sample."""
        c = self.counts().astype(np.float64)[..., None]
        with np.errstate(all="ignore"):
            return np.where(c > 0, self.rgb_sum().astype(np.float64) / c, 0.0)

    def std_error(self):
        """Standard error of every pixel mean, f64 (H, W, 3), with the pixel's own k = counts / m items; inf below two items."""
        return std_error(self.rgb_sum(), self.sq_sum(), self.counts(), self.samples_per_item)

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

    def _denoise_counts(self):
        """(samples, counts) of denoise_frame: every pixel's own count, as a full-frame device plane."""
        if self.params.shard_count <= 1:
            return 0, self._counts
        return 0, on_device(self.counts().view(np.int32), self._rgb.device)

    # ---- checkpoints ----
    def save(self, path):
        """An .npz checkpoint: sums, counts, samples_done, frame_samples, the options, the RtParams fields, the camera and the scene."""
        np.savez(path, kind=np.array(KIND), adaptive_version=np.int64(ADAPTIVE_VERSION), min_samples=np.int64(self.min_samples),
                 rel_error=np.float64(self.options.rel_error), abs_error=np.float64(self.options.abs_error), counts=self._flat_counts(), **self._checkpoint())

    @classmethod
    def load(cls, path, ctx, scene, cam, params=None):
        """Resumes a checkpoint on `ctx` with `scene` and `cam` (and, if given, `params`). ValueError when anything does not match."""
        import torch
        z = read_checkpoint(path)
        check_adaptive_checkpoint(z, params=params, cam=cam, fingerprint=scene.fingerprint)
        prm = params_from_array(z["params"], int(z["frame_samples"]))
        ada = cls(ctx, scene, cam, prm, int(z["frame_samples"]), min_samples=int(z["min_samples"]), rel_error=float(z["rel_error"]),
                  abs_error=float(z["abs_error"]))
        ada._restore(z)
        ada._counts.copy_(torch.from_numpy(z["counts"].astype(np.uint32).view(np.int32)))
        torch.cuda.synchronize(ada._rgb.device)
        ada.samples_traced = int(z["counts"].astype(np.int64).sum())
        return ada


