"""Case builders for the kernels that run after the fold (tests/test_postprocess_host.py, tests/test_gpu_postprocess.py): write_color,
the adaptive selection, untile and the pixel-list check. Every case is a synthetic buffer with an exact expected value; nothing here has
a tolerance. Functions that need the package take it as `pkg` (the fixture of conftest.py)."""
from collections import namedtuple

import numpy as np

F32 = np.float32
FLT_MIN = F32(1.17549435e-38)
FLT_MAX = np.finfo(F32).max
DENORM_MIN = F32(1e-45)                          # the smallest subnormal, 2^-149
SENTINEL = 0xFFFFFFFF

# ---- A. write_color ---------------------------------------------------------------------------------------------------------------------
SPPS = (1, 2, 3, 5, 7, 10, 16, 30, 100, 500, 1000)
COUNT_CYCLE = SPPS + (0, 2 ** 32 - 1)            # the per-pixel count plane of the counts kernel cycles through these
WC_WIDTH = 251                                   # 3 * 251 is odd: H * W * 3 is a multiple of 256 only if H is
WC_RANDOM = 200_000


def ulps(x, k):
    """The f32 values k representable steps away from x (k < 0: towards -inf)."""
    x = np.asarray(x, dtype=F32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf), dtype=F32)
    return x


def write_color_boundary(spp):
    """The f32 sums at which a byte changes, spp * (b / 256)^2 for b = 0 .. 256, each with its neighbours at -2 .. +2 ulps."""
    b = np.arange(257, dtype=np.float64)
    v = (spp * (b / 256.0) ** 2).astype(F32)
    return np.concatenate([ulps(v, k) for k in (-2, -1, 0, 1, 2)])


def write_color_specials(spp):
    top = F32(0.999 * 0.999 * spp)
    return np.concatenate([
        np.array([0.0, -0.0, DENORM_MIN, FLT_MIN, spp, 2 * spp, 1e30, FLT_MAX, np.inf, -np.inf, np.nan, -1.0, -DENORM_MIN], dtype=F32),
        np.array([ulps(top, k) for k in (-2, -1, 0, 1, 2)], dtype=F32)])


def write_color_cases():
    """(sums float32 (H, W, 3), spp) for every spp of SPPS: the boundary sums, the specials, WC_RANDOM uniform sums in [0, 2 spp), padded
    with uniform sums to whole rows. The element count is no multiple of 256, so the last workgroup is part-filled."""
    cases = []
    for i, spp in enumerate(SPPS):
        rng = np.random.default_rng([41, i])
        v = np.concatenate([write_color_boundary(spp), write_color_specials(spp), (rng.random(WC_RANDOM) * 2 * spp).astype(F32)])
        row = 3 * WC_WIDTH
        pad = -v.size % row
        v = np.concatenate([v, (rng.random(pad) * 2 * spp).astype(F32)])
        assert v.size % 256 != 0 and v.size % row == 0
        cases.append((v.reshape(-1, WC_WIDTH, 3), spp))
    return cases


def count_plane(h, w):
    """Per-pixel counts cycling through COUNT_CYCLE (13 values; 13 and 3 are coprime, so every count meets every channel and every row offset)."""
    return np.resize(np.array(COUNT_CYCLE, dtype=np.uint32), h * w).reshape(h, w)


def write_color_f64(sums, spp_or_counts):
    """main.rs:141-169 in numpy f64: NaN on the sum -> 0, 1.0 / spp, multiply, sqrt, clamp to [0, 0.999], 256 *, saturating cast with
    NaN -> 0. spp_or_counts: one spp, or one count per pixel (shape sums.shape[:-1]); a count of 0 gives 0."""
    c = np.asarray(sums, dtype=F32).astype(np.float64)
    n = np.asarray(spp_or_counts, dtype=np.uint32).astype(np.float64)
    per_pixel = n.ndim > 0
    if per_pixel:
        n = n[..., None]
    with np.errstate(all="ignore"):
        c = np.where(np.isnan(c), 0.0, c)
        scale = 1.0 / n
        c = np.sqrt(scale * c)
        c = np.where(c < 0.0, 0.0, np.where(c > 0.999, 0.999, c))
        q = 256.0 * c
        out = np.where(np.isnan(q), 0.0, np.clip(q, 0.0, 255.0)).astype(np.uint8)      # the cast truncates, as `as u8` does
    if per_pixel:
        out = np.where(n == 0.0, np.uint8(0), out)
    return out


# ---- B. adaptive selection --------------------------------------------------------------------------------------------------------------
SelectCase = namedtuple("SelectCase", "params first_sample frame_samples options rgb sq counts name want")
"""params: make_params kwargs; options: (min_samples, rel_error, abs_error); rgb / sq: (slots, 3) float32; counts: (slots,) uint32;
want: the slots the case is built to select (bool per slot; None: whatever the reference says)."""

SELECT_SIZES = [dict(width=w, height=h) for w, h in
                [(2, 2), (3, 21), (8, 8), (5, 13), (3, 85), (16, 16), (7, 37), (255, 257), (256, 256), (257, 257), (25, 5243)]]
SELECT_SHARDS = [dict(width=400, height=350, tile_size=32, shard_index=0, shard_count=2),
                 dict(width=400, height=350, tile_size=32, shard_index=1, shard_count=2),
                 dict(width=300, height=260, tile_size=256, shard_index=1, shard_count=2),
                 dict(width=70, height=40, tile_size=8, shard_index=2, shard_count=3)]
BENCH_FRAME = dict(width=1200, height=800)
PATTERNS = ("nothing", "everything", "slot0", "last", "lane63", "lane0", "alternate_waves", "bernoulli_0.5", "bernoulli_0.01", "bernoulli_0.99",
            "nonfinite")
FIRST, FRAME, OPTIONS = 8, 64, (4, 0.05, 0.0)      # m = 1; 8 >= min_samples, so every candidate reaches the variance test


def size_id(kw):
    s = f"{kw['width']}x{kw['height']}"
    return s + (f"-t{kw['tile_size']}-s{kw['shard_index']}of{kw['shard_count']}" if kw.get("shard_count", 1) > 1 else "")


def layout(kw):
    """slot_pixels of make_params(**kw) without the library: (slots, in-image mask)."""
    x, _, ok = layout_pixels(kw)
    return x.size, ok


def layout_pixels(kw):
    """slot_pixels of make_params(**kw) without the library: (x, y, in-image mask) of every slot."""
    W, H, sc = kw["width"], kw["height"], kw.get("shard_count", 1)
    if sc <= 1:
        s = np.arange(W * H, dtype=np.int64)
        return s % W, s // W, np.ones(W * H, dtype=bool)
    ts, si = kw["tile_size"], kw["shard_index"]
    tiles_x, tiles_y = -(-W // ts), -(-H // ts)
    n_tiles = tiles_x * tiles_y
    n_local = (n_tiles - si + sc - 1) // sc if n_tiles > si else 0
    s = np.arange(n_local * ts * ts, dtype=np.int64)
    lt, r = s // (ts * ts), s % (ts * ts)
    tile = si + lt * sc
    x, y = (tile % tiles_x) * ts + r % ts, (tile // tiles_x) * ts + r // ts
    return x, y, (x < W) & (y < H)


def pattern_mask(pattern, valid, rng):
    slots = valid.size
    s = np.arange(slots)
    if pattern == "nothing":
        want = np.zeros(slots, dtype=bool)
    elif pattern == "everything":
        want = np.ones(slots, dtype=bool)
    elif pattern == "slot0":
        want = s == 0
    elif pattern == "last":
        want = s == np.nonzero(valid)[0][-1]
    elif pattern == "lane63":
        want = s % 64 == 63
    elif pattern == "lane0":
        want = s % 64 == 0
    elif pattern == "alternate_waves":
        want = (s // 64) % 2 == 0
    else:                                                     # Bernoulli: at least one slot each way, so no frame degenerates to all or none
        p = 0.5 if pattern == "nonfinite" else float(pattern.split("_")[1])
        want = rng.random(slots) < p
        ok = np.nonzero(valid)[0]
        if not want[ok].any():
            want[rng.choice(ok)] = True
        if want[ok].all():
            want[rng.choice(ok)] = False
    return want & valid


def select_buffers(want, valid, first_sample, frame_samples, rng, k_items=None):
    """Sums and counts that make exactly `want` the active list, by two mechanisms at once. A wanted slot is a candidate (count ==
    first_sample) whose sums are noisy in one channel. Of the others, every second one is a candidate with converged sums, and the rest
    carry noisy sums and a count other than first_sample (they stopped earlier). Clipped slots carry noisy sums and count == first_sample:
    only their place outside the image keeps them out. k_items: the work items behind the count (count / m; None: the count, m = 1)."""
    slots = want.size
    k = first_sample if k_items is None else k_items
    S = ((0.1 + 0.9 * rng.random((slots, 3))) * first_sample).astype(F32)
    base = S.astype(np.float64) ** 2 / k
    quiet = (base * (1 + 1e-4)).astype(F32)                   # variance ~ 1e-4 S^2 / k^2: a hundred times inside rel_error 0.05
    loud = (base * 1.5).astype(F32)                           # variance ~ S^2 / (2 k^2): far outside
    ch = rng.integers(0, 3, slots)
    Q = quiet.copy()
    rows = np.nonzero(want)[0]
    Q[rows, ch[rows]] = loud[rows, ch[rows]]
    others = np.nonzero(~want & valid)[0]
    by_count = others[1::2]                                   # the first of the others is always a converged candidate
    Q[by_count] = loud[by_count]
    Q[~valid] = loud[~valid]
    counts = np.full(slots, first_sample, dtype=np.uint32)
    counts[by_count] = rng.choice(np.array([0, first_sample // 2, first_sample - 1, first_sample + 1, frame_samples], dtype=np.uint32), by_count.size)
    return S, Q, counts


def select_case(kw, pattern, seed):
    rng = np.random.default_rng([17] + list(seed))
    slots, valid = layout(kw)
    want = pattern_mask(pattern, valid, rng)
    S, Q, counts = select_buffers(want, valid, FIRST, FRAME, rng)
    if pattern == "nonfinite":                                # 1 % of the slots: NaN or +-inf in one channel of rgb or sq
        bad = rng.random(slots) < 0.01
        if not (bad & valid & (counts == FIRST)).any():
            bad[np.nonzero(valid & (counts == FIRST))[0][0]] = True
        rows = np.nonzero(bad)[0]
        val = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=F32), rows.size)
        in_sq = rng.random(rows.size) < 0.5
        chn = rng.integers(0, 3, rows.size)
        S[rows[~in_sq], chn[~in_sq]] = val[~in_sq]
        Q[rows[in_sq], chn[in_sq]] = val[in_sq]
        want = want | (bad & valid & (counts == FIRST))       # a candidate with a non-finite sum is never converged; a stopped pixel stays out
    return SelectCase(dict(kw, spp=FRAME), FIRST, FRAME, OPTIONS, S, Q, counts, f"{size_id(kw)}/{pattern}", want)


def select_cases(sizes=None):
    """Every pattern at every size of `sizes` (default: SELECT_SIZES and SELECT_SHARDS), then the benchmarked frame once."""
    every = SELECT_SIZES + SELECT_SHARDS
    for kw in (every if sizes is None else sizes):
        for pi, pattern in enumerate(PATTERNS):
            yield select_case(kw, pattern, (every.index(kw) if kw in every else 99, pi))
    if sizes is None:
        yield bench_frame_case()


def bench_frame_case(pattern="bernoulli_0.5"):
    return select_case(BENCH_FRAME, pattern, (50, PATTERNS.index(pattern)))


def select_m16_cases(flag_sample_blocks):
    """m = 16 (RT_FLAG_SAMPLE_BLOCKS, frame_samples 256): batch means of 16 samples, sums drawn as test_adaptive_host.py's
    test_select_reference_is_the_header_formula_with_batch_means draws them (there k = 4 only). want is None: the reference decides."""
    m, frame = 16, 256
    for i, (w, h) in enumerate([(257, 257), (5, 13)]):
        for j, first in enumerate((32, 64)):
            rng = np.random.default_rng([23, i, j])
            slots = w * h
            S = (rng.random((slots, 3)) * first).astype(F32)
            k = first // m                                    # converged iff the excess r of Q over S^2 / k is <= rel^2 (k - 1): r's range
            r = rng.random((slots, 3)) * 0.5 * (k - 1) / 3    # follows k, so that at k = 2 as at k = 4 about half the channels converge
            Q = (S.astype(np.float64) ** 2 / k * (1 + r)).astype(F32)
            counts = np.full(slots, first, dtype=np.uint32)
            counts[rng.random(slots) < 0.1] = first - 16      # stopped a pass earlier
            yield SelectCase(dict(width=w, height=h, spp=frame, flags=flag_sample_blocks), first, frame, (32, 0.3, 1e-3), S, Q, counts,
                             f"{w}x{h}/m16/first{first}", None)


# the knife edge: one 4 x 2 frame; per channel S and Q of the pixels below, the same in all three channels unless said otherwise
KNIFE_PIXELS = ("on the edge: converged", "one ulp up: selected", "Q < S^2/k: converged", "S = 0, Q = 0: converged", "count below first_sample: out",
                "count above first_sample: out", "one ulp up in one channel: selected", "far outside: selected")


def knife_cases(flag_sample_blocks):
    """var / m^2 == tol^2 exactly (converged: the criterion is <=) and Q one f32 ulp above it (selected), in exact arithmetic.
    m = 1: count 4, S = 8, rel_error 0.5, abs_error 0: k = 4, d = Q - 64/4, var = d / 12, tol = 0.5 * 8/4 = 1, so var <= 1 iff Q <= 28.
    m = 16: count 64, S = 128: k = 4, d = Q - 16384/4, var / 256 = d / 3072, tol = 0.5 * 128/64 = 1, so converged iff Q <= 7168.
    Every quantity is a small integer or an integer plus one f32 ulp: no operation rounds on either side of the comparison."""
    for m, count, s_val, q_edge, flags in ((1, 4, 8.0, 28.0, 0), (16, 64, 128.0, 7168.0, flag_sample_blocks)):
        frame = 64 if m == 1 else 256
        up = float(ulps(F32(q_edge), 1))
        S = np.full((8, 3), s_val, dtype=F32)
        Q = np.full((8, 3), q_edge, dtype=F32)
        Q[1] = up
        Q[2] = s_val * s_val / 4 - 1.0                         # below S^2 / k: d is clamped to 0
        S[3], Q[3] = 0.0, 0.0                                  # tolerance 0 and variance 0: 0 <= 0
        Q[4], Q[5] = 4 * q_edge, 4 * q_edge                    # noisy, but not candidates
        Q[6, 1] = up
        Q[7] = 4 * q_edge
        counts = np.full(8, count, dtype=np.uint32)
        counts[4], counts[5] = count - m, count + m
        kw = dict(width=4, height=2, spp=frame, flags=flags)
        cand = np.array([1, 1, 1, 1, 0, 0, 1, 1], dtype=bool)
        yield SelectCase(kw, count, frame, (2 * m, 0.5, 0.0), S, Q, counts, f"knife/m{m}", np.array([0, 1, 0, 0, 0, 0, 1, 1], dtype=bool))
        yield SelectCase(kw, count, frame, (2 * count, 0.5, 0.0), S, Q, counts, f"knife/m{m}/below_min_samples", cand)      # every candidate, whatever its noise
        yield SelectCase(dict(kw, spp=count), count, count, (2 * m, 0.5, 0.0), S, Q, counts, f"knife/m{m}/frame_end", np.zeros(8, dtype=bool))


def reference_list(pkg, case):
    """select_reference of a case, as tests/test_gpu_adaptive.py calls it: m from pass_check, valid from slot_pixels."""
    prm = pkg.make_params(**case.params)
    m = pkg.pass_check(prm, 0, case.frame_samples)
    return pkg.select_reference(case.rgb, case.sq, case.counts, case.first_sample, case.frame_samples, m, pkg.adaptive_options(*case.options),
                                valid=pkg.slot_pixels(prm)[2])


# ---- C. untile ----------------------------------------------------------------------------------------------------------------------------
UNTILE_SHAPES = [(2, 2, 8, 1), (2, 2, 8, 3), (63, 5, 8, 2), (64, 4, 8, 5), (65, 3, 16, 2), (129, 67, 8, 7), (129, 67, 32, 3), (129, 67, 64, 8),
                 (300, 260, 256, 2), (257, 9, 16, 4)]
FRAME_SENTINEL_F32, FRAME_SENTINEL_U8 = F32(-1.0), np.uint8(0xA5)


def shard_params(pkg, w, h, tile, world, rank):
    return pkg.make_params(w, h, 1, tile_size=tile, shard_index=rank, shard_count=world)


def gathered_slot_pixels(pkg, prm):
    """slot_pixels of a shard's buffer as the untile entry points read it. With one shard the gathered buffer is still tile after tile
    (shard 0 of 1), whereas slot_pixels describes the row-major frame an unsharded render writes: the same formula with world = 1 then."""
    if prm.shard_count > 1:
        return pkg.slot_pixels(prm)
    ts, W, H = int(prm.tile_size), int(prm.width), int(prm.height)
    tiles_x, tiles_y = -(-W // ts), -(-H // ts)
    s = np.arange(tiles_x * tiles_y * ts * ts, dtype=np.int64)
    tile, r = s // (ts * ts), s % (ts * ts)
    x, y = (tile % tiles_x) * ts + r % ts, (tile // tiles_x) * ts + r // ts
    return x, y, (x < W) & (y < H)


def untile_case(pkg, w, h, tile, world):
    """(params of shard 0, gathered f32 (world, per_shard), gathered u8, expected f32 frame, expected u8 frame). Each gathered element
    holds its own global index (f32: as a float, below 2^24; u8: a multiplicative hash of it); the expected frames start as sentinels
    and every element of them is written exactly once."""
    prm0 = shard_params(pkg, w, h, tile, world, 0)
    x0, _, _ = gathered_slot_pixels(pkg, prm0)
    per_shard = 3 * x0.size                                   # every shard buffer has the size of shard 0's, the largest
    idx = np.arange(world * per_shard, dtype=np.uint64).reshape(world, per_shard)
    assert idx.size < 2 ** 24
    g32 = idx.astype(F32)
    g8 = ((idx * np.uint64(2654435761) >> np.uint64(24)) & np.uint64(0xFF)).astype(np.uint8)
    want32 = np.full((h, w, 3), FRAME_SENTINEL_F32, dtype=F32)
    want8 = np.full((h, w, 3), FRAME_SENTINEL_U8, dtype=np.uint8)
    written = np.zeros((h, w), dtype=np.int64)
    for r in range(world):
        x, y, ok = gathered_slot_pixels(pkg, shard_params(pkg, w, h, tile, world, r))
        assert 3 * x.size <= per_shard
        want32[y[ok], x[ok]] = g32[r, :3 * x.size].reshape(-1, 3)[ok]
        want8[y[ok], x[ok]] = g8[r, :3 * x.size].reshape(-1, 3)[ok]
        np.add.at(written, (y[ok], x[ok]), 1)
    assert (written == 1).all() and (want32 >= 0).all()
    return prm0, g32, g8, want32, want8


# ---- D. pixel lists -----------------------------------------------------------------------------------------------------------------------
LIST_FRAME = (264, 250)                                       # 66000 slots: beyond slot 65535


def list_pass_entries():
    """Every 211th slot and the last one: 314 entries, a workgroup of k_list_check and a part-filled second."""
    slots = LIST_FRAME[0] * LIST_FRAME[1]
    lst = np.concatenate([np.arange(0, slots, 211), [slots - 1]]).astype(np.int64)
    assert lst.size == 314 and lst.size % 256 != 0
    return lst


def refused_lists(slots, done_slot):
    """(entries, word of the message) for lists over slots whose count is 0, except done_slot, whose count is not. Each fault sits where
    one workgroup of k_list_check ends and the next begins (entries 255 / 256), or at the very end of a list of 300."""
    good = np.arange(300, dtype=np.int64) * 211 + 1
    assert good[-1] < slots and done_slot not in good and done_slot > good[-2]
    a = good.copy(); a[[255, 256]] = a[[256, 255]]            # noqa: E702   entry 256 is below entry 255: only thread 0 of the second workgroup sees it
    b = good.copy(); b[257] = b[256]                          # noqa: E702
    c = good.copy(); c[-1] = done_slot                        # noqa: E702
    d = good.copy(); d[-1] = slots                            # noqa: E702
    return [(a, "ascending"), (b, "ascending"), (c, "counts"), (d, "slots")]
