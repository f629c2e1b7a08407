"""Environment maps (include/rt_hip.h RtEnvMap): an HDR equirectangular image as background and, sampled, as one more light.

EnvMap           the record an upload takes: upload_options(env_map=EnvMap(rgb)), Context.upload(desc, env_map=...)
env_reference    the numpy statement of the header's four rules — lookup, tables, draw, pdf — in float32 (the device's arithmetic, operation
                 for operation) or float64 (the yardstick), on the streams of lights._Rng
env_tables       rt_env_tables: the two cdf tables as the upload builds them
load_hdr         a Radiance .hdr (RGBE) reader, flat and run-length encoded scanlines, pure numpy

The header is the authority; this module restates it. Row 0 of a map is up (+y); column 0 begins at -x and the columns turn towards +z."""
import ctypes as C
import math

import numpy as np

from . import _abi as A
from .lights import _Ops, _Rng

LUMA = (0.2126, 0.7152, 0.0722)


class EnvMap:
    """rgb: (H, W, 3) linear radiance, finite and >= 0 (kept as a float32 copy the record points into); sampled: RT_ENV_SAMPLED; scale multiplies
    every texel. Nothing is checked here: the upload (or rt_env_tables) refuses what the header refuses."""

    def __init__(self, rgb, sampled=True, scale=1.0, flags=None):
        self.rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if self.rgb.ndim != 3 or self.rgb.shape[2] != 3:
            raise ValueError("rgb must have the shape (height, width, 3)")
        self.record = A.RtEnvMap(C.sizeof(A.RtEnvMap), (A.RT_ENV_SAMPLED if sampled else 0) if flags is None else flags, self.rgb.shape[1], self.rgb.shape[0],
                                 self.rgb.ctypes.data_as(C.POINTER(C.c_float)), scale, 0)

    width = property(lambda self: int(self.record.width))
    height = property(lambda self: int(self.record.height))
    scale = property(lambda self: float(self.record.scale))
    sampled = property(lambda self: bool(self.record.flags & A.RT_ENV_SAMPLED))


def env_tables(env):
    """rt_env_tables: (marg (H,), cond (H, W)) float32, as the upload builds them. Host only. Raises RtError for a map an upload refuses."""
    from .api import _check, lib
    marg, cond = np.zeros(env.height, np.float32), np.zeros((env.height, env.width), np.float32)
    fp = C.POINTER(C.c_float)
    _check(lib().rt_env_tables(C.byref(env.record), marg.ctypes.data_as(fp), cond.ctypes.data_as(fp)))
    return marg, cond


def tables_reference(rgb):
    """The header's TABLES rule: (marg, cond, total). f64, every sum sequential (np.cumsum accumulates in order), one rounding to f32 at the end."""
    rgb = np.asarray(rgb, dtype=np.float32).astype(np.float64)
    H, W = rgb.shape[:2]
    st = np.sin(math.pi * (np.arange(H) + 0.5) / H)
    f = ((LUMA[0] * rgb[..., 0] + LUMA[1] * rgb[..., 1]) + LUMA[2] * rgb[..., 2]) * st[:, None]
    run = np.cumsum(f, axis=1)
    rows = run[:, -1]
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(rows[:, None] > 0.0, run / rows[:, None], (np.arange(W) + 1.0)[None, :] / W).astype(np.float32)
    cond[:, -1] = 1.0
    mrun = np.cumsum(rows)
    total = float(mrun[-1])
    marg = (mrun / total if total > 0.0 else (np.arange(H) + 1.0) / H).astype(np.float32)
    marg[-1] = 1.0
    return marg, cond, total


def _texel(M, W, H, d):
    """LOOKUP: (i, j, border) of directions d (three arrays in M.T, any length). border: the distance, in texels and in this dtype, to the nearest
    border between two texels (the seam and the poles are no borders: the clamps decide there)."""
    T = M.T
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ud = M.unit(d)
        theta = np.arccos(-ud[1]).astype(T)
        phi = (np.arctan2(-ud[2], ud[0]).astype(T) + T(math.pi)).astype(T)
        u = phi * T(T(0.5) * T(1.0 / math.pi))
        v = theta * T(1.0 / math.pi)
        u = np.minimum(np.maximum(np.nan_to_num(u, nan=0.0), T(0.0)), T(1.0))
        v = T(1.0) - np.minimum(np.maximum(np.nan_to_num(v, nan=0.0), T(0.0)), T(1.0))
        fi, fj = u * T(W), v * T(H)
    i = np.minimum(fi.astype(np.int64), W - 1)
    j = np.minimum(fj.astype(np.int64), H - 1)

    def gap(f, n):
        k = np.rint(f.astype(np.float64))
        return np.where((k >= 1) & (k <= n - 1), np.abs(f.astype(np.float64) - k), np.inf)
    return i, j, np.minimum(gap(fi, W), gap(fj, H)), ud


def _pdf(M, W, H, marg, cond, d):
    T = M.T
    i, j, border, ud = _texel(M, W, H, d)
    m, c = marg.astype(T), cond.astype(T)
    m_lo = np.where(j > 0, m[np.maximum(j - 1, 0)], T(0.0))
    c_lo = np.where(i > 0, c[j, np.maximum(i - 1, 0)], T(0.0))
    mass = (m[j] - m_lo) * (c[j, i] - c_lo)
    with np.errstate(invalid="ignore", divide="ignore"):
        sin_theta = np.sqrt(T(1.0) - ud[1] * ud[1])
        pdf = ((mass * T(W)) * T(H)) / (T(2.0 * math.pi * math.pi) * sin_theta)
    return np.where(sin_theta > 0, pdf, T(0.0)).astype(T), i, j, border, sin_theta


def _draw(M, W, H, marg, cond, g, live):
    """DRAW: two rnd() of the streams in `live`; (d, i, j)."""
    T = M.T
    u1, u2 = g.rnd(live), g.rnd(live)
    m, c = marg.astype(T), cond.astype(T)
    j = np.minimum((m[None, :] <= u1[:, None]).sum(axis=1), H - 1)          # the first index whose entry exceeds the draw
    row = c[j]
    i = np.minimum((row <= u2[:, None]).sum(axis=1), W - 1)
    m_lo = np.where(j > 0, m[np.maximum(j - 1, 0)], T(0.0))
    c_lo = np.where(i > 0, row[np.arange(len(i)), np.maximum(i - 1, 0)], T(0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        fy = (u1 - m_lo) / (m[j] - m_lo)
        fx = (u2 - c_lo) / (row[np.arange(len(i)), i] - c_lo)
        a = (i.astype(T) + fx) / T(W)
        b = (j.astype(T) + fy) / T(H)
        phi, th = T(2.0 * math.pi) * a, T(math.pi) * b
        sb, cb = np.sin(th).astype(T), np.cos(th).astype(T)
        d = [-(sb * np.cos(phi).astype(T)), cb, sb * np.sin(phi).astype(T)]
    return d, i, j


def env_reference(env, dirs=None, states=None, dtype=np.float64):
    """The header's rules for one map, in `dtype` (np.float32: the device's arithmetic; np.float64: the yardstick; the tables are the f32 ones in
    both, as the header's pdf takes f32 cdf differences).
    dirs (n, 3), read as f32:  dict(i, j, radiance (n, 3) = scale * texel, pdf, border (texels to the nearest border between texels), sin_theta)
    states (n uint64):         the DRAW on lights._Rng streams: dict(d (n, 3), i, j (the drawn texel), n_draws) and, for the drawn directions in
                               this dtype, the entries above."""
    T = np.dtype(dtype).type
    M = _Ops(T)
    W, H = env.width, env.height
    marg, cond, total = tables_reference(env.rgb)
    out = dict(marg=marg, cond=cond, total=total)
    if states is not None:
        g = _Rng(np.asarray(states, dtype=np.uint64).reshape(-1), T)
        d, i, j = _draw(M, W, H, marg, cond, g, np.ones(g.s.shape, dtype=bool))
        out.update(d=np.stack(d, axis=1), drawn_i=i, drawn_j=j, n_draws=g.n.copy())
    else:
        dd = np.asarray(dirs, dtype=np.float32).reshape(-1, 3)
        d = [dd[:, k].astype(T) for k in range(3)]
    pdf, i, j, border, sin_theta = _pdf(M, W, H, marg, cond, d)
    rad = (np.float32(env.scale) * env.rgb[j, i]).astype(np.float32) if T is np.float32 else float(np.float32(env.scale)) * env.rgb[j, i].astype(np.float64)
    out.update(i=i, j=j, radiance=rad, pdf=pdf, border=border, sin_theta=sin_theta)
    return out


def texel_solid_angle(W, H, j):
    """Solid angle of a texel of row j: (2 pi / W) (cos(pi j / H) - cos(pi (j + 1) / H)), f64."""
    return 2.0 * math.pi / W * (math.cos(math.pi * j / H) - math.cos(math.pi * (j + 1) / H))


# ---- Radiance .hdr (RGBE) -------------------------------------------------------------------------------------------------------------------------------
def _rgbe_to_float(px):
    """(n, 4) uint8 -> (n, 3) float32: mantissa * 2^(e - 136), 0 where e = 0."""
    e = px[:, 3].astype(np.int32)
    scale = np.where(e > 0, np.ldexp(1.0, e - 136), 0.0)
    return (px[:, :3].astype(np.float64) * scale[:, None]).astype(np.float32)


def load_hdr(data):
    """A Radiance picture as an (H, W, 3) float32 array of linear radiance, row 0 = top. data: bytes, or a path. Reads FORMAT=32-bit_rle_rgbe with
    the resolution line "-Y H +X W" (the orientation every writer emits), flat scanlines and the run-length encoding of 8 <= W < 32768 (each
    scanline: 2 2 W_hi W_lo, then the four channels one after another as runs). EXPOSURE lines are not applied; the old per-pixel run-length
    form (1 1 1 n) and XYZE are refused."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        with open(data, "rb") as fh:
            data = fh.read()
    data = bytes(data)
    if not (data.startswith(b"#?RADIANCE") or data.startswith(b"#?RGBE")):
        raise ValueError("not a Radiance picture (no #? signature)")
    pos, fmt = 0, None
    while True:
        end = data.find(b"\n", pos)
        if end < 0:
            raise ValueError("truncated header")
        line, pos = data[pos:end].strip(), end + 1
        if line.startswith(b"FORMAT="):
            fmt = line[7:]
        if not line:
            break
    if fmt is not None and fmt != b"32-bit_rle_rgbe":
        raise ValueError("unsupported FORMAT " + fmt.decode(errors="replace"))
    end = data.find(b"\n", pos)
    res = data[pos:end].split()
    if end < 0 or len(res) != 4 or res[0] != b"-Y" or res[2] != b"+X":
        raise ValueError("unsupported resolution line (expected -Y H +X W)")
    H, W = int(res[1]), int(res[3])
    if H <= 0 or W <= 0:
        raise ValueError("bad resolution")
    pos = end + 1
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.empty((H, W, 4), dtype=np.uint8)
    for y in range(H):
        if pos + 4 > len(buf):
            raise ValueError("truncated picture")
        rle = 8 <= W < 32768 and buf[pos] == 2 and buf[pos + 1] == 2 and (int(buf[pos + 2]) << 8 | int(buf[pos + 3])) == W
        if not rle:
            if pos + 4 * W > len(buf):
                raise ValueError("truncated picture")
            line = buf[pos:pos + 4 * W].reshape(W, 4)
            if W > 1 and ((line[1:, 0] == 1) & (line[1:, 1] == 1) & (line[1:, 2] == 1)).any():
                raise ValueError("old run-length form (1 1 1 n) is not supported")
            out[y] = line
            pos += 4 * W
            continue
        pos += 4
        for ch in range(4):
            x = 0
            while x < W:
                if pos >= len(buf):
                    raise ValueError("truncated picture")
                n = int(buf[pos]); pos += 1
                if n > 128:
                    n -= 128
                    if n == 0 or x + n > W or pos >= len(buf):
                        raise ValueError("bad run")
                    out[y, x:x + n, ch] = buf[pos]; pos += 1
                else:
                    if n == 0 or x + n > W or pos + n > len(buf):
                        raise ValueError("bad run")
                    out[y, x:x + n, ch] = buf[pos:pos + n]; pos += n
                x += n
    return _rgbe_to_float(out.reshape(-1, 4)).reshape(H, W, 3)
