"""Occlusion queries without a GPU (include/rt_hip.h, "occlusion queries"): the two symbols are declared, exported and bound; they refuse
a call without a context; the Python wrapper accepts the three ray forms as far as a host without a device can tell; and the kernels the
feature adds — the any-hit instances of k_extend, k_rays_import<true>, k_occluded_export — are in the gfx950 code object the build made,
one k_extend instance per (mode, variant), with no scratch and (the walks) no static LDS."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rays as R  # noqa: E402

SYMBOLS = ("rt_occluded_rays", "rt_occluded_rays_device")


def test_symbols_are_declared_exported_and_bound(pkg):
    A = pkg._abi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_hip.h")).read(), flags=re.S)
    raw = C.CDLL(pkg.lib_path())
    for name in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name + " is not declared in include/rt_hip.h"
        assert name in A.RT_HIP_SYMBOLS and hasattr(raw, name), name
        f = getattr(pkg.lib(), name)
        assert f.restype is C.c_int32 and len(f.argtypes) == 7, name
    assert A.RT_ABI_VERSION == 3 == pkg.lib().rt_abi_version()
    # the header no longer says the mode is missing, and says what a wide scene gets
    text = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert "there is no any-hit mode" not in text and "rt_occluded_rays" in text and "RT_LAYOUT_WIDE_NODES" in text
    assert callable(pkg.Context.occluded)


def test_null_context_and_option_refusals(pkg):
    A, lib = pkg._abi, pkg.lib()
    rays = (A.RtRay * 2)()
    out = (C.c_uint8 * 3)(7, 7, 7)
    assert lib.rt_occluded_rays(None, None, None, C.cast(rays, C.c_void_p), 2, C.cast(out, C.c_void_p), None) == A.RT_ERR_INVALID
    assert b"ctx" in lib.rt_last_error(None)
    assert lib.rt_occluded_rays_device(None, None, None, None, 0, None, None) == A.RT_ERR_INVALID
    assert list(out) == [7, 7, 7]
    # the options of an occlusion query are the ray query's, and rt_ray_query_check is their check
    assert lib.rt_ray_query_check(C.byref(pkg.ray_query_options(flags=A.RT_FLAG_TIMING, pool_slots=4096)), 1000) == A.RT_OK
    for o, n, word in ((A.RtRayQueryOptions(8, 0, 0, 0), 1, b"struct_bytes"), (A.RtRayQueryOptions(16, 1 << 7, 0, 0), 1, b"unknown"),
                       (A.RtRayQueryOptions(16, A.RT_FLAG_COUNTERS, 0, 0), 1, b"unknown"), (None, 1 << 32, b"2^32")):
        assert lib.rt_ray_query_check(C.byref(o) if o is not None else None, n) == A.RT_ERR_INVALID
        assert word in lib.rt_last_error(None)


class _NoDevice:
    """Stands in for a context on a host without one: the wrapper's own argument checks run before the library is asked."""
    _h = None
    device_id = 0


def test_wrapper_takes_the_three_ray_forms(pkg):
    A = pkg._abi
    occluded = pkg.Context.occluded
    scene = _NoDevice()
    rays = R.make_rays(np.zeros((5, 3)), np.tile([0.0, 0.0, 1.0], (5, 1)), np.zeros(5), t_max=1.0)
    flat = np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)
    assert flat.shape == (5, 8) and (flat[:, 7] == 1.0).all()
    # structured and (n, 8) float32 host forms reach the library, which refuses the missing context and writes nothing
    for form in (rays, flat):
        out = np.full(5, 9, np.uint8)
        with pytest.raises(pkg.RtError) as e:
            occluded(_NoDevice(), scene, form, out=out)
        assert e.value.code == A.RT_ERR_INVALID and (out == 9).all()
    # what the wrapper itself refuses
    for bad in (np.zeros((5, 7), np.float32), np.zeros((5, 8), np.float64), np.zeros(40, np.float32)):
        with pytest.raises(ValueError):
            occluded(_NoDevice(), scene, bad)
    for bad_out in (np.zeros(4, np.uint8), np.zeros(5, np.int32), np.zeros((5, 2), np.uint8)[:, 0]):
        with pytest.raises(ValueError):
            occluded(_NoDevice(), scene, rays, out=bad_out)
    # the tensor form: a CPU tensor is not the device variant's input
    import torch
    with pytest.raises(ValueError):
        occluded(_NoDevice(), scene, torch.zeros((5, 8), dtype=torch.float32))


def _kernel_metadata(lib_path, tmp_path):
    """{demangled kernel name: (vgpr, sgpr, scratch bytes, static LDS bytes)} of the gfx950 code object inside the built library."""
    import shutil
    hipcc = os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")          # the compiler the build used; its LLVM tools lie beside it
    rocm = os.path.dirname(os.path.dirname(hipcc))
    dirs = [os.path.join(rocm, "llvm", "bin"), os.path.join(rocm, "lib", "llvm", "bin"), "/opt/rocm/llvm/bin"]
    tool = lambda n: next((os.path.join(d, n) for d in dirs if os.path.exists(os.path.join(d, n))), n)
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib_path, str(tmp_path / "unused.so")])
    subprocess.check_call([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
    notes = subprocess.check_output([tool("llvm-readelf"), "--notes", co], text=True)
    out = {}
    for b in notes.split("  - .agpr_count")[1:]:
        get = lambda k: re.search(r"\.%s:\s+(\S+)" % k, b).group(1)
        name = subprocess.check_output(["c++filt", get("name")], text=True).strip()
        out[re.sub(r"\(.*", "", name)] = (int(get("vgpr_count")), int(get("sgpr_count")), int(get("private_segment_fixed_size")), int(get("group_segment_fixed_size")))
    return out


def test_new_kernels_are_built_for_gfx950_without_scratch(pkg, tmp_path):
    meta = _kernel_metadata(pkg.lib_path(), tmp_path)
    anyhit = {k: v for k, v in meta.items() if "k_extend<" in k and k.rstrip(">").endswith("true") and k.count(",") == 6}
    for name, (vgpr, sgpr, scratch, lds) in sorted(anyhit.items()):
        print(f"vgpr {vgpr:>3} sgpr {sgpr:>3} scratch {scratch:>4} lds {lds:>5}  {name}")
    # one instance per (mode, variant): four modes x {spheres, mesh, box, everything but media}; no counters, no drain, no list
    want = {(mode, feat) for mode in (0, 1, 2, 3) for feat in (0, 6, 82, 119)}
    got = set()
    for name in anyhit:
        m = re.search(r"k_extend<(\d+), (\d+)u, (\w+), (\d+)u, (\w+), (\w+), true>", name)
        assert m, name
        assert (m.group(3), m.group(5), m.group(6)) == ("false", "false", "false"), name
        assert (int(m.group(1)), int(m.group(2))) not in got, "two group sizes of " + name
        got.add((int(m.group(1)), int(m.group(2))))
    assert got == want, (sorted(got), sorted(want))
    for name, (vgpr, sgpr, scratch, lds) in anyhit.items():
        # no scratch; no static LDS (the staged scene starts at LDS address 0); within the 128 registers a 1024-thread group leaves a lane
        assert scratch == 0 and lds == 0 and vgpr <= 128, (name, vgpr, sgpr, scratch, lds)
    for k in ("void rtk::k_rays_import<true>", "rtk::k_occluded_export"):
        assert k in meta, k + " is not in the code object"
        assert meta[k][2] == 0, (k, meta[k])
    assert meta["rtk::k_occluded_export"][3] == 0
    # the closest-hit kernels of a query are still there beside them
    assert "void rtk::k_rays_import<false>" in meta and any(k.startswith("void rtk::k_rays_export<") for k in meta)
