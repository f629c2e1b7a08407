"""Rays for Context.radiance (include/rt_hip.h, "radiance queries"): RtPathRay records from origins and directions, the rays of an
equirectangular panorama — the worked example of a camera model the built-in thin lens cannot express — and the standard error of the
per-ray means."""
import numpy as np

from .api import PATHRAY_DTYPE


def path_rays(o, d, time=0, first_draw=0):
    """A PATHRAY_DTYPE array from origins and directions (each (n, 3), or one (3,) vector for all), times and first_draw counts (scalars or
    (n,)). Values are rounded to f32 once, here."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    n = max([a.shape[0] for a in (o, d) if a.ndim == 2] + [np.size(time) if np.ndim(time) else 1, np.size(first_draw) if np.ndim(first_draw) else 1])
    rays = np.zeros(n, dtype=PATHRAY_DTYPE)
    rays["o"] = np.broadcast_to(o, (n, 3)).astype(np.float32)
    rays["d"] = np.broadcast_to(d, (n, 3)).astype(np.float32)
    rays["time"] = np.broadcast_to(np.asarray(time, dtype=np.float64), (n,)).astype(np.float32)
    rays["first_draw"] = np.broadcast_to(np.asarray(first_draw), (n,)).astype(np.uint32)
    return rays


def equirect_rays(origin, width, height, time=0.0):
    """The width * height rays of an equirectangular panorama seen from `origin`, row-major, through the pixel centres. Row 0 is the top and y
    is up; the centre of the image looks along -z and x grows to the right. Pixel (x, y) has the elevation el = pi (height / 2 - (y + 0.5)) /
    height and the azimuth az = 2 pi ((x + 0.5) - width / 2) / width, and looks along d = (cos el sin az, sin el, -cos el cos az). Mirrored
    rows and columns have exactly negated angles, so their directions mirror exactly. Unit directions are formed in f64 and rounded to f32
    once."""
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError("a panorama needs at least one pixel")
    el = np.pi * ((height / 2.0 - (np.arange(height, dtype=np.float64) + 0.5)) / height)
    az = 2.0 * np.pi * (((np.arange(width, dtype=np.float64) + 0.5) - width / 2.0) / width)
    ce, se = np.cos(el)[:, None], np.sin(el)[:, None]
    d = np.stack([ce * np.sin(az)[None, :], np.broadcast_to(se, (height, width)), -ce * np.cos(az)[None, :]], axis=-1)
    return path_rays(np.asarray(origin, dtype=np.float64).reshape(3), d.reshape(-1, 3), time=time)


def standard_error(rgb_sum, sq_sum, samples):
    """The standard error of the per-ray mean rgb_sum / samples, from the sums of a radiance query over `samples` samples (rt_render_pass's
    formula with m = 1): sqrt(max(Q - S^2 / k, 0) / (k (k - 1))), in f64. Needs samples >= 2."""
    k = float(samples)
    if k < 2:
        raise ValueError("a standard error needs at least two samples")
    s, q = np.asarray(rgb_sum, dtype=np.float64), np.asarray(sq_sum, dtype=np.float64)
    return np.sqrt(np.maximum(q - s * s / k, 0.0) / (k * (k - 1.0)))
