"""The ray-list and output-buffer validators of the binding (api.py _host_rays, _check_out), which Context.trace_rays, occluded and
radiance share: plain functions of arrays, so their host forms are tested without a device. The ValueError texts are the ones the three
methods have always raised."""
import numpy as np
import pytest


def _api(pkg):
    import sys
    return sys.modules[pkg.__name__ + ".api"]


@pytest.mark.parametrize("dtype_name", ["RAY_DTYPE", "PATHRAY_DTYPE"])
def test_host_rays(pkg, dtype_name):
    api = _api(pkg)
    dtype = getattr(pkg, dtype_name)
    f = np.arange(5 * 8, dtype=np.float32).reshape(5, 8)
    got = api._host_rays(f, dtype, dtype_name)                       # (n, 8) float32: the same bytes, viewed as records
    assert got.dtype == dtype and got.shape == (5,) and got.flags.c_contiguous and got.tobytes() == f.tobytes()
    got = api._host_rays(f[::2], dtype, dtype_name)                  # ... also when the rows are not contiguous
    assert got.shape == (3,) and got.tobytes() == np.ascontiguousarray(f[::2]).tobytes()
    rec = np.zeros((2, 3), dtype=dtype)
    rec["o"] = 1.5
    got = api._host_rays(rec, dtype, dtype_name)                     # a record array of any shape: flattened
    assert got.dtype == dtype and got.shape == (6,) and got.tobytes() == rec.tobytes()
    for empty in (np.zeros((0, 8), dtype=np.float32), np.zeros(0, dtype=dtype)):
        got = api._host_rays(empty, dtype, dtype_name)               # n = 0
        assert got.dtype == dtype and got.shape == (0,)
    message = f"host rays must be a numpy array of {dtype_name}, or float32 of shape (n, 8)"
    for bad in (np.zeros((5, 7), dtype=np.float32), np.zeros(8, dtype=np.float32), np.zeros((2, 2, 8), dtype=np.float32), np.zeros((5, 8), dtype=np.float64),
                np.zeros((5, 8), dtype=np.int32), [[0.0] * 8]):
        with pytest.raises(ValueError) as e:
            api._host_rays(bad, dtype, dtype_name)
        assert str(e.value) == message
    other = pkg.PATHRAY_DTYPE if dtype_name == "RAY_DTYPE" else pkg.RAY_DTYPE
    with pytest.raises(ValueError) as e:                             # the other query's records are not reinterpreted
        api._host_rays(np.zeros(3, dtype=other), dtype, dtype_name)
    assert str(e.value) == message


def test_check_out_host(pkg):
    api = _api(pkg)
    n = 5
    hits_message = "out must be a C-contiguous numpy array of n RAYHIT_DTYPE records"
    api._check_out(np.empty(n, dtype=pkg.RAYHIT_DTYPE), False, pkg.RAYHIT_DTYPE, n, hits_message)
    api._check_out(np.empty(n, dtype=np.uint8), False, np.dtype(np.uint8), n, "m")
    api._check_out(np.empty(0, dtype=np.uint8), False, np.uint8, 0, "m")
    api._check_out(np.empty((n, 3), dtype=np.float32), False, np.float32, 3 * n, "m")
    for bad in (np.empty(n + 1, dtype=pkg.RAYHIT_DTYPE), np.empty(n, dtype=np.uint8), np.empty((n, 12), dtype=np.float32), np.empty(2 * n, dtype=pkg.RAYHIT_DTYPE)[::2],
                [0] * n, None):
        with pytest.raises(ValueError) as e:
            api._check_out(bad, False, pkg.RAYHIT_DTYPE, n, hits_message)
        assert str(e.value) == hits_message
    with pytest.raises(ValueError) as e:                             # a host array where a device tensor is due
        api._check_out(np.empty(n, dtype=np.uint8), True, np.uint8, n, "out must be a contiguous uint8 CUDA tensor of n elements")
    assert str(e.value) == "out must be a contiguous uint8 CUDA tensor of n elements"


def test_the_methods_raise_todays_texts(pkg):
    """trace_rays, occluded and radiance validate a host call before they touch the context: on a Context that was never created, a wrong ray
    list or output raises the ValueError it always has."""
    Ctx, rays = pkg.Context, np.zeros((5, 8), dtype=np.float32)
    ctx = Ctx.__new__(Ctx)
    ctx._h = None
    for call, message in ((lambda: Ctx.trace_rays(ctx, None, rays[:, :7]), "host rays must be a numpy array of RAY_DTYPE, or float32 of shape (n, 8)"),
                          (lambda: Ctx.occluded(ctx, None, rays.astype(np.float64)), "host rays must be a numpy array of RAY_DTYPE, or float32 of shape (n, 8)"),
                          (lambda: Ctx.radiance(ctx, None, rays[:, :7], 1), "host rays must be a numpy array of PATHRAY_DTYPE, or float32 of shape (n, 8)"),
                          (lambda: Ctx.trace_rays(ctx, None, rays, out=np.empty(4, dtype=pkg.RAYHIT_DTYPE)), "out must be a C-contiguous numpy array of n RAYHIT_DTYPE records"),
                          (lambda: Ctx.trace_rays(ctx, None, rays, out=np.empty((5, 12), dtype=np.float32)), "out must be a C-contiguous numpy array of n RAYHIT_DTYPE records"),
                          (lambda: Ctx.occluded(ctx, None, rays, out=np.empty(5, dtype=np.int8)), "out must be a C-contiguous numpy array of n uint8"),
                          (lambda: Ctx.occluded(ctx, None, np.zeros((0, 8), dtype=np.float32), out=np.empty(1, dtype=np.uint8)), "out must be a C-contiguous numpy array of n uint8"),
                          (lambda: Ctx.radiance(ctx, None, rays, 1, rgb_sum=np.empty((5, 4), dtype=np.float32)), "rgb_sum must be a C-contiguous numpy array of 15 float32"),
                          (lambda: Ctx.radiance(ctx, None, rays, 1, sq_sum=np.empty(15, dtype=np.float64)), "sq_sum must be a C-contiguous numpy array of 15 float32"),
                          (lambda: Ctx.radiance(ctx, None, rays, 1, invalid=np.empty(5, dtype=np.float32)), "invalid must be a C-contiguous numpy array of 5 uint8"),
                          (lambda: Ctx.radiance(ctx, None, rays, 1, accumulate=True), "accumulate needs the rgb_sum and sq_sum of the samples so far")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == message
