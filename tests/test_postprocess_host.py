"""The case builders of tests/postprocess.py without a GPU: the numpy restatements are pinned to the host mirror, and every case is shown
to be what it claims, so that the GPU tests (tests/test_gpu_postprocess.py) cannot pass vacuously."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postprocess as PP  # noqa: E402
from conftest import record_metric  # noqa: E402


# ---- A. write_color -----------------------------------------------------------------------------------------------------------------------
def write_color_f32(sums, spp):
    """The same operations as PP.write_color_f64, each rounded to f32: what the device kernels computed before they went to f64."""
    f = np.float32
    c = np.asarray(sums, dtype=f).copy()
    with np.errstate(all="ignore"):
        c[np.isnan(c)] = f(0)
        scale = f(1) / f(spp)
        c = np.sqrt(scale * c, dtype=f)
        c = np.where(c < f(0), f(0), np.where(c > f(0.999), f(0.999), c)).astype(f)
        q = f(256) * c
        return np.where(np.isnan(q), f(0), np.clip(q, f(0), f(255))).astype(np.uint8)


def test_write_color_f64_is_the_host_mirror(pkg):
    for sums, spp in PP.write_color_cases():
        assert sums.dtype == np.float32 and sums.ndim == 3 and sums.shape[2] == 3 and sums.size % 256 != 0
        assert np.array_equal(PP.write_color_f64(sums, spp), pkg.tonemap(sums, spp)), spp
    # per-pixel counts: every count's pixels are that spp's frame, and a count of 0 is black whatever the sum holds
    sums, _ = PP.write_color_cases()[3]
    counts = PP.count_plane(*sums.shape[:2])
    got = PP.write_color_f64(sums, counts)
    for n in PP.COUNT_CYCLE:
        sel = counts == n
        assert sel.any()
        assert np.array_equal(got[sel], pkg.tonemap(sums, n)[sel] if n else np.zeros((int(sel.sum()), 3), np.uint8)), n
    # single pixels through rt_host_write_color, the function main.rs's loop calls
    for v, spp, want in [(0.25, 1, 128), (2.0, 2, 255), (np.nan, 1, 0), (-1.0, 1, 0), (np.inf, 7, 255), (1.0, 2 ** 32 - 1, 0)]:
        assert pkg.write_color([v, v, v], spp) == (want,) * 3 == tuple(PP.write_color_f64(np.full((1, 1, 3), v, np.float32), spp)[0, 0])


def test_f32_write_color_misses_the_boundary_inputs():
    """The condition that keeps the GPU comparison from being vacuous: evaluated in f32, write_color gives another byte than in f64 on at
    least 1000 of the boundary inputs (measured: see the printed figure), always the neighbouring byte."""
    differ = total = 0
    for spp in PP.SPPS:
        v = PP.write_color_boundary(spp).reshape(1, -1, 1).repeat(3, axis=2)
        a, b = PP.write_color_f64(v, spp).astype(np.int64), write_color_f32(v, spp).astype(np.int64)
        assert np.abs(a - b).max() <= 1
        differ += int((a != b)[..., 0].sum())
        total += v.shape[1]
    print(f"f32 and f64 write_color differ on {differ} of {total} boundary inputs")
    record_metric(test="f32_write_color_misses_the_boundary_inputs", differ=differ, total=total)
    assert total == len(PP.SPPS) * 257 * 5
    assert differ >= 1000, (differ, total)


# ---- B. adaptive selection ----------------------------------------------------------------------------------------------------------------
def check_pattern(case, ref, valid):
    slots = valid.size
    pattern = case.name.split("/")[1]
    sharded = case.params.get("shard_count", 1) > 1
    cand = valid & (case.counts == case.first_sample)
    n_waves = -(-slots // 64)
    if pattern == "nothing":
        assert ref.size == 0 and cand.any()                               # not for want of candidates
    elif pattern == "everything":
        assert np.array_equal(ref, np.nonzero(valid)[0])
    elif pattern == "slot0":
        assert ref.tolist() == [0]
    elif pattern == "last":
        assert ref.tolist() == [int(np.nonzero(valid)[0][-1])] and (sharded or ref[0] == slots - 1)
    elif pattern == "lane63":
        assert (ref % 64 == 63).all() and ref.size == (int((valid[63::64]).sum()) if sharded else slots // 64)
    elif pattern == "lane0":
        assert (ref % 64 == 0).all() and ref.size == (int((valid[0::64]).sum()) if sharded else n_waves)
    elif pattern == "alternate_waves":
        assert ((ref // 64) % 2 == 0).all()
        assert ref.size == sum(int(valid[64 * w:64 * w + 64].sum()) for w in range(0, n_waves, 2))
    elif pattern.startswith("bernoulli"):
        assert 0.001 * cand.sum() <= ref.size <= 0.999 * cand.sum(), (case.name, ref.size, int(cand.sum()))
    elif pattern == "nonfinite":
        bad = ~(np.isfinite(case.rgb).all(axis=1) & np.isfinite(case.sq).all(axis=1))
        assert (bad & cand).any() and set(np.nonzero(bad & cand)[0].tolist()) <= set(ref.tolist())
        assert not set(np.nonzero(bad & ~cand)[0].tolist()) & set(ref.tolist())
    else:
        raise AssertionError(pattern)


def test_select_cases_are_what_they_name(pkg):
    seen = set()
    n_cases = 0
    for case in PP.select_cases():
        prm = pkg.make_params(**case.params)
        valid = pkg.slot_pixels(prm)[2]
        slots, valid_np = PP.layout(case.params)
        assert slots == valid.size == case.counts.size and np.array_equal(valid, valid_np), case.name
        assert case.rgb.shape == case.sq.shape == (slots, 3) and case.rgb.dtype == case.sq.dtype == np.float32
        ref = PP.reference_list(pkg, case)
        assert ref.dtype == np.uint32
        assert (np.diff(ref.astype(np.int64)) > 0).all() and (ref.size == 0 or ref[-1] < slots) and valid[ref].all(), case.name
        assert np.array_equal(ref, np.nonzero(case.want)[0]), case.name
        check_pattern(case, ref, valid)
        # both mechanisms at once: among the in-image slots left out, some are converged candidates and (room permitting) some stopped earlier
        out = valid & ~case.want
        if out.sum() >= 2:
            assert (out & (case.counts == case.first_sample)).any() and (out & (case.counts != case.first_sample)).any(), case.name
        seen.add(case.name.split("/")[1])
        n_cases += 1
    assert seen == set(PP.PATTERNS) and n_cases == len(PP.PATTERNS) * (len(PP.SELECT_SIZES) + len(PP.SELECT_SHARDS)) + 1
    # the sizes are the ones at which the scan's run changes: waves per frame, and the runs of a 1024-thread scan
    runs = {PP.size_id(kw): -(-(-(-PP.layout(kw)[0] // 64)) // 1024) for kw in PP.SELECT_SIZES + PP.SELECT_SHARDS + [PP.BENCH_FRAME]}
    assert runs["255x257"] == runs["256x256"] == 1 and runs["257x257"] == 2 and runs["25x5243"] == 3 and runs["1200x800"] == 15
    assert runs["400x350-t32-s0of2"] == runs["400x350-t32-s1of2"] == runs["300x260-t256-s1of2"] == 2
    assert PP.layout(PP.SELECT_SHARDS[0])[0] == 72 * 1024 and PP.layout(PP.SELECT_SHARDS[1])[0] == 71 * 1024


def test_select_m16_cases_select_some_and_not_all(pkg):
    A = pkg._abi
    for case in PP.select_m16_cases(A.RT_FLAG_SAMPLE_BLOCKS):
        prm = pkg.make_params(**case.params)
        assert pkg.pass_check(prm, 0, case.frame_samples) == 16
        pkg.adaptive_check(prm, pkg.adaptive_options(*case.options), case.first_sample, case.frame_samples)
        ref = PP.reference_list(pkg, case)
        cand = case.counts == case.first_sample
        assert 0 < ref.size < cand.sum() < cand.size and cand[ref].all(), case.name
        assert (np.diff(ref.astype(np.int64)) > 0).all()


def test_select_reference_decides_the_knife_edge(pkg):
    A = pkg._abi
    names = []
    for case in PP.knife_cases(A.RT_FLAG_SAMPLE_BLOCKS):
        prm = pkg.make_params(**case.params)
        m = pkg.pass_check(prm, 0, case.frame_samples)
        assert m == (16 if "m16" in case.name else 1)
        pkg.adaptive_check(prm, pkg.adaptive_options(*case.options), case.first_sample, case.frame_samples)
        assert len(PP.KNIFE_PIXELS) == case.counts.size == 8
        ref = PP.reference_list(pkg, case)
        assert ref.tolist() == np.nonzero(case.want)[0].tolist(), (case.name, ref.tolist())
        names.append(case.name)
        if case.name.count("/") == 1:
            # the edge by hand, in integers: d / (k (k - 1)) / m^2 against tol^2 = 1
            k, q_edge, s = 4, float(case.sq[0, 0]), float(case.rgb[0, 0])
            assert (q_edge - s * s / k) / (k * (k - 1)) / (m * m) == 1.0 == (0.5 * s / case.first_sample) ** 2
            assert float(case.sq[1, 0]) > q_edge and np.nextafter(np.float32(q_edge), np.float32(np.inf)) == case.sq[1, 0]
            assert ref.tolist() == [1, 6, 7]
    assert len(names) == 6


# ---- C. untile ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,tile,world", PP.UNTILE_SHAPES)
def test_host_untile_is_the_slot_map(pkg, w, h, tile, world):
    prm0, g32, g8, want32, want8 = PP.untile_case(pkg, w, h, tile, world)
    assert world == 1 or g32.shape[1] == pkg.output_floats(prm0)      # (one shard: the gathered buffer is tiled, the render's output is not)
    assert np.array_equal(pkg.untile(prm0, g32.reshape(-1)), want32)
    assert np.array_equal(pkg.untile_rgb8(prm0, g8.reshape(-1)), want8)
    if (w, h, tile, world) == (2, 2, 8, 3):
        assert pkg.output_floats(PP.shard_params(pkg, w, h, tile, world, 1)) == pkg.output_floats(PP.shard_params(pkg, w, h, tile, world, 2)) == 0


@pytest.mark.parametrize("w,h,tile,world", [(70, 40, 32, 2), (40, 40, 16, 3), (130, 100, 64, 3), (17, 9, 8, 4), (16, 16, 16, 3)])
def test_in_place_is_the_untile_of_one_shard(pkg, w, h, tile, world):
    """layout.in_place against the path it replaced — the shard's buffer at its offset in a zeroed gathered buffer, then rt_untile — bit
    for bit, and its one-channel form against this directory's own restatement of the layout. Every slot holds a non-zero value, the
    clipped slots of edge tiles too, so a scatter that does not drop them shows."""
    from ray_tracer_archive_amd.layout import in_place
    rng = np.random.default_rng(1000 * w + h)
    per_shard = pkg.output_floats(PP.shard_params(pkg, w, h, tile, world, 0))
    sizes = []
    for r in range(world):
        prm = PP.shard_params(pkg, w, h, tile, world, r)
        x, y, ok = PP.layout_pixels(dict(width=w, height=h, tile_size=tile, shard_index=r, shard_count=world))
        sizes.append(x.size)
        assert pkg.output_floats(prm) == 3 * x.size <= per_shard
        flat = rng.uniform(0.5, 2.0, 3 * x.size).astype(np.float32)
        gathered = np.zeros(world * per_shard, dtype=np.float32)
        gathered[r * per_shard:r * per_shard + flat.size] = flat
        got = in_place(prm, flat, 3)
        assert got.dtype == np.float32 and got.shape == (h, w, 3)
        assert np.array_equal(got.view(np.uint32), pkg.untile(prm, gathered).view(np.uint32)), r
        assert int((got != 0).all(axis=2).sum()) == int(ok.sum())
        counts = rng.integers(1, 2 ** 32, x.size, dtype=np.uint32)
        want = np.zeros((h, w), dtype=np.uint32)
        want[y[ok], x[ok]] = counts[ok]
        got = in_place(prm, counts, 1)
        assert got.dtype == np.uint32 and np.array_equal(got, want), r
    assert (w, h, tile, world) != (16, 16, 16, 3) or sizes == [256, 0, 0]
    assert (w, h, tile, world) != (17, 9, 8, 4) or sizes == [128, 128, 64, 64]          # 3 x 2 tiles, the right column and the bottom row clipped
    whole = pkg.make_params(w, h, 1)                          # an unsharded frame: a reshape
    flat = np.arange(3 * w * h, dtype=np.float32)
    assert np.array_equal(in_place(whole, flat, 3), flat.reshape(h, w, 3)) and np.array_equal(in_place(whole, flat[:w * h], 1), flat[:w * h].reshape(h, w))


# ---- D. pixel lists -------------------------------------------------------------------------------------------------------------------------
def test_list_cases_put_their_faults_on_the_workgroup_boundary():
    slots = PP.LIST_FRAME[0] * PP.LIST_FRAME[1]
    lst = PP.list_pass_entries()
    assert slots == 66000 and (np.diff(lst) > 0).all() and lst[-1] == slots - 1 > 65535
    (a, _), (b, _), (c, _), (d, _) = PP.refused_lists(slots, slots - 1)
    bad_order = lambda x: np.nonzero(np.diff(x) <= 0)[0] + 1          # noqa: E731   the entries a thread of k_list_check finds out of order
    assert bad_order(a).tolist() == [256] and bad_order(b).tolist() == [257]
    assert bad_order(c).size == 0 and c[-1] == slots - 1 and not set(c[:-1].tolist()) & set(lst.tolist())
    assert bad_order(d).size == 0 and d[-1] == slots and (d[:-1] < slots).all()
