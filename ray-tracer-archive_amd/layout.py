"""The layout of a frame's buffers: which pixel every slot of an rgb_sum-ordered buffer holds (include/rt_hip.h, rt_output_floats), and the
one scatter from slot order to an image that Progressive, Adaptive, the feature pass and the denoiser's guide go through. Reassembling
many shards' gathered buffers is another problem: rt_untile (api.untile, distributed.assemble, Context.untile_device)."""
import numpy as np

from .api import output_floats


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


def in_place(params, flat, channels):
    """Slot-ordered values, `channels` per slot, as an image in their dtype: (H, W), or (H, W, channels) for more than one channel. An
    unsharded frame is a reshape; a sharded frame has this shard's in-image slots in place and every other pixel 0."""
    shape = (int(params.height), int(params.width)) + ((channels,) if channels > 1 else ())
    if params.shard_count <= 1:
        return flat.reshape(shape)
    x, y, ok = slot_pixels(params)
    out = np.zeros(shape, dtype=flat.dtype)
    out[y[ok], x[ok]] = flat.reshape((-1,) + shape[2:])[ok]
    return out


def on_device(a, dev):
    """A host array (an untiled plane of sums or counts) as a flat tensor on `dev`."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev)
