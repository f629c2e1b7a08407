"""First-hit feature frames over rt_render_features_device (include/rt_hip.h, "first-hit features"): the per-pixel means a feature-guided
filter or an external denoiser starts from, for the camera rays of the frame a Progressive or an Adaptive object renders."""
import numpy as np

from . import _abi as A
from .layout import in_place


def feature_means(ctx, scene, cam, params, samples, first_sample=0, pool_slots=0):
    """One feature pass of `samples` samples per pixel (uniform, whatever the radiance counts are) with the frame's RtParams; returns
    (albedo (H, W, 3), normal (H, W, 3), depth (H, W), hit_fraction (H, W)), f32 means: the albedo over the samples, the normal and the
    depth over the samples that hit (0 where none did), the fraction of the samples that hit. A sharded frame is untiled first: this
    shard's tiles in place, the other shards' pixels 0."""
    samples = int(samples)
    if samples < 1:
        raise ValueError("a feature pass needs at least one sample per pixel")
    prm = A.RtParams.from_buffer_copy(params)
    prm.samples_per_pixel = samples
    prm.flags &= A.RT_FLAG_TIMING | A.RT_FLAG_SAMPLE_BLOCKS      # (a feature pass refuses the counter and the fused-kernel diagnostics)
    albedo, normal, depth, hits = ctx.render_features(scene, cam, prm, first_sample=first_sample, pool_slots=pool_slots)
    a, n = albedo.cpu().numpy().reshape(-1, 3), normal.cpu().numpy().reshape(-1, 3)
    d, h = depth.cpu().numpy(), hits.cpu().numpy().view(np.uint32).astype(np.float32)
    over_hits = np.where(h > 0, h, np.float32(1))
    planes = (a / np.float32(samples), n / over_hits[:, None], d / over_hits, h / np.float32(samples))
    return tuple(in_place(prm, p, 3 if p.ndim == 2 else 1) for p in planes)
