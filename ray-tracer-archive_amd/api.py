"""Thin object wrappers over librt_hip.so. Names follow the C ABI (include/rt_hip.h, include/rt_host.h)."""
import ctypes as C
import os

import numpy as np

from . import _abi as A
from .build import LIB_PATH

_lib = None


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rt error {code}: {msg}")
        self.code = code


def lib_path():
    # RT_HIP_LIB selects a tuning build (scripts/ only); the default is the in-tree lib/librt_hip.so
    return os.environ.get("RT_HIP_LIB", LIB_PATH)


def lib():
    """Load librt_hip.so. Raises if it has not been built (python __graft_entry__.py / build.py)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RtError(A.RT_ERR_NO_DEVICE, f"{path} is missing: build it first (ray-tracer-archive_amd/build.py); "
                          "the product path has no fallback")
        _lib = A.declare(C.CDLL(path))
        if _lib.rt_abi_version() != A.RT_ABI_VERSION:
            raise RtError(A.RT_ERR_INVALID, "librt_hip.so ABI version mismatch")
    return _lib


def _check(code, ctx=None):
    if code != A.RT_OK:
        msg = lib().rt_last_error(ctx).decode() if ctx is not None else lib().rt_last_error(None).decode()
        raise RtError(code, msg)


def make_params(width, height, spp, max_depth=50, seed=1, nan_policy=A.RT_NAN_PER_SAMPLE, flags=0, tile_size=0, shard_index=0,
                shard_count=1, pool_slots=0, tail_paths=0):
    return A.RtParams(width, height, spp, max_depth, seed, nan_policy, flags, tile_size, shard_index, shard_count, pool_slots, tail_paths, 0)


def pass_check(params, first_sample, frame_samples, accumulate=False):
    """rt_pass_check (host only): the samples per work item m of the frame; raises RtError (RT_ERR_INVALID, with the reason) for a pass
    that does not satisfy the contract of include/rt_hip.h."""
    opt = A.RtPassOptions(C.sizeof(A.RtPassOptions), A.RT_PASS_ACCUMULATE if accumulate else 0, first_sample, frame_samples)
    m = C.c_uint32(0)
    _check(lib().rt_pass_check(C.byref(params), C.byref(opt), C.byref(m)))
    return m.value


def adaptive_options(min_samples, rel_error=0.0, abs_error=0.0):
    return A.RtAdaptiveOptions(C.sizeof(A.RtAdaptiveOptions), int(min_samples), float(rel_error), float(abs_error))


def adaptive_check(params, options, first_sample, frame_samples):
    """rt_adaptive_check (host only): raises RtError (RT_ERR_INVALID, with the reason) for options the contract refuses."""
    _check(lib().rt_adaptive_check(C.byref(params), C.byref(options), first_sample, frame_samples))


def denoise_options(window_radius=0, patch_radius=0, samples_per_item=0, strength=0.0, alpha=0.0, eps=0.0):
    """RtDenoiseOptions; a field left 0 takes its default (window 10, patch 3, m 1, strength 0.45, alpha 1, eps 1e-10)."""
    return A.RtDenoiseOptions(C.sizeof(A.RtDenoiseOptions), int(window_radius), int(patch_radius), int(samples_per_item), float(strength), float(alpha), float(eps))


def denoise_check(width, height, options=None):
    """rt_denoise_check (host only): raises RtError (RT_ERR_INVALID, with the reason) for a size or options the filter refuses."""
    _check(lib().rt_denoise_check(width, height, C.byref(options) if options is not None else None))


def denoise_guide(feature_samples, albedo=None, normal=None, depth=None, hits=None, sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0):
    """RtDenoiseGuide (include/rt_hip.h, "denoising, guided"): the feature planes of rt_render_features_device — CUDA tensors, raw device
    addresses, or None for a plane not used — folded over feature_samples samples per pixel; a sigma left 0 takes its default."""
    ptr = lambda t: None if t is None else int(t) if isinstance(t, int) else t.data_ptr()
    return A.RtDenoiseGuide(C.sizeof(A.RtDenoiseGuide), int(feature_samples), ptr(albedo), ptr(normal), ptr(depth), ptr(hits),
                            float(sigma_albedo), float(sigma_normal), float(sigma_depth))


def denoise_guided_check(width, height, options, guide):
    """rt_denoise_guided_check (host only): raises RtError (RT_ERR_INVALID, with the reason) for what the guided filter refuses."""
    _check(lib().rt_denoise_guided_check(width, height, C.byref(options) if options is not None else None, C.byref(guide) if guide is not None else None))


def denoise_guide_moments(feature_samples, albedo=None, normal=None, depth=None, hits=None, albedo_sq=None, normal_sq=None, depth_sq=None,
                          sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0, variance_strength=0.0):
    """RtDenoiseGuideMoments (include/rt_hip.h, "denoising, guided with feature variances"): the planes of rt_render_feature_moments_device
    — CUDA tensors, raw device addresses, or None — folded over feature_samples >= 2 samples per pixel; a sigma or the variance strength
    left 0 takes its default."""
    ptr = lambda t: None if t is None else int(t) if isinstance(t, int) else t.data_ptr()
    return A.RtDenoiseGuideMoments(C.sizeof(A.RtDenoiseGuideMoments), int(feature_samples), ptr(albedo), ptr(normal), ptr(depth), ptr(hits), ptr(albedo_sq),
                                   ptr(normal_sq), ptr(depth_sq), float(sigma_albedo), float(sigma_normal), float(sigma_depth), float(variance_strength))


def denoise_guided_moments_check(width, height, options, guide):
    """rt_denoise_guided_moments_check (host only): raises RtError (RT_ERR_INVALID, with the reason) for what the variance-guided filter refuses."""
    _check(lib().rt_denoise_guided_moments_check(width, height, C.byref(options) if options is not None else None, C.byref(guide) if guide is not None else None))


# numpy views of RtRay / RtRayHit (include/rt_hip.h, "ray queries"): 32 and 48 bytes, field for field
RAY_DTYPE = np.dtype([("o", np.float32, 3), ("time", np.float32), ("d", np.float32, 3), ("t_max", np.float32)])
RAYHIT_DTYPE = np.dtype([("t", np.float32), ("hittable", np.int32), ("material", np.int32), ("flags", np.uint32),
                         ("p", np.float32, 3), ("u", np.float32), ("n", np.float32, 3), ("v", np.float32)])
# ... and of RtLightQuery / RtLightSample ("light-sample queries"): 40 and 24 bytes
LIGHTQUERY_DTYPE = np.dtype([("p", np.float32, 3), ("flags", np.uint32), ("rng_state", np.uint64), ("d", np.float32, 3), ("_pad", np.float32)])
LIGHTSAMPLE_DTYPE = np.dtype([("d", np.float32, 3), ("pdf", np.float32), ("light", np.int32), ("n_draws", np.uint32)])


def ray_query_options(flags=0, pool_slots=0):
    return A.RtRayQueryOptions(C.sizeof(A.RtRayQueryOptions), flags, pool_slots, 0)


def ray_query_check(options=None, n_rays=0):
    """rt_ray_query_check (host only): raises RtError (RT_ERR_INVALID, with the reason) for options or a ray count a query refuses."""
    _check(lib().rt_ray_query_check(C.byref(options) if options is not None else None, n_rays))


# ... and of RtPathRay ("radiance queries"): 32 bytes, RAY_DTYPE with first_draw in the place of t_max
PATHRAY_DTYPE = np.dtype([("o", np.float32, 3), ("time", np.float32), ("d", np.float32, 3), ("first_draw", np.uint32)])


def radiance_options(samples, max_depth=50, seed=1, first_sample=0, first_stream=0, accumulate=False, nan_policy=A.RT_NAN_PER_SAMPLE, pool_slots=0,
                     tail_paths=0, render_flags=0, flags=None):
    """RtRadianceOptions (include/rt_hip.h, "radiance queries"); flags overrides the accumulate bit when given."""
    f = (A.RT_RADIANCE_ACCUMULATE if accumulate else 0) if flags is None else int(flags)
    return A.RtRadianceOptions(C.sizeof(A.RtRadianceOptions), f, int(render_flags), int(nan_policy), int(samples), int(first_sample), int(max_depth),
                               int(pool_slots), int(seed), int(first_stream), int(tail_paths), 0)


def radiance_check(options, n_rays=0):
    """rt_radiance_check (host only): raises RtError (RT_ERR_INVALID, with the reason) for options or a ray count a radiance query refuses."""
    _check(lib().rt_radiance_check(C.byref(options) if options is not None else None, n_rays))


def feature_options(first_sample=0, accumulate=False, pool_slots=0, flags=None):
    """RtFeatureOptions (include/rt_hip.h, "first-hit features"); flags overrides the accumulate bit when given."""
    f = (A.RT_FEATURES_ACCUMULATE if accumulate else 0) if flags is None else int(flags)
    return A.RtFeatureOptions(C.sizeof(A.RtFeatureOptions), f, int(first_sample), int(pool_slots))


def features_check(params, options):
    """rt_features_check (host only): raises RtError (RT_ERR_INVALID, with the reason) for a feature pass the contract refuses."""
    _check(lib().rt_features_check(C.byref(params), C.byref(options) if options is not None else None))


def feature_moment_buffers(albedo=None, normal=None, depth=None, hits=None, albedo_sq=None, normal_sq=None, depth_sq=None):
    """RtFeatureMomentBuffers (include/rt_hip.h, "first-hit features, second moments"): CUDA tensors, raw device addresses, or None."""
    ptr = lambda t: None if t is None else int(t) if isinstance(t, int) else t.data_ptr()
    return A.RtFeatureMomentBuffers(C.sizeof(A.RtFeatureMomentBuffers), 0, ptr(albedo), ptr(normal), ptr(depth), ptr(hits), ptr(albedo_sq), ptr(normal_sq), ptr(depth_sq))


def feature_moments_check(params, options, buffers):
    """rt_feature_moments_check (host only): raises RtError (RT_ERR_INVALID, with the reason) for a pass with second moments the contract refuses."""
    _check(lib().rt_feature_moments_check(C.byref(params), C.byref(options) if options is not None else None, C.byref(buffers) if buffers is not None else None))


def _feature_buffers(albedo=None, normal=None, depth=None, hits=None):
    """RtFeatureBuffers (include/rt_hip.h, "first-hit features"): CUDA tensors, or None for a plane not wanted."""
    return A.RtFeatureBuffers(*[t.data_ptr() if t is not None else None for t in (albedo, normal, depth, hits)])


# the two feature passes (Context._feature_pass)
_FEATURE_PLANES = ("rt_render_features_device", _feature_buffers, (3, 3, 1, 1), ((0, 1, "albedo / normal"), (2, None, "depth"), (3, None, "hits")))
_MOMENT_PLANES = ("rt_render_feature_moments_device", feature_moment_buffers, (3, 3, 1, 1, 3, 3, 1),
                  ((0, 1, "albedo / normal"), (4, 5, "albedo_sq / normal_sq"), (2, 6, "depth / depth_sq"), (3, None, "hits")))


def _check_device(a, b, n, what, float_):
    """a (and b, unless None) are contiguous CUDA tensors of n elements (n None: any), float32 or a 32-bit integer type."""
    import torch
    ok = (torch.float32,) if float_ else (torch.int32, torch.uint32) if hasattr(torch, "uint32") else (torch.int32,)
    for t in (a, b):
        if t is not None and (not t.is_cuda or t.dtype not in ok or not t.is_contiguous() or (n is not None and t.numel() != n)):
            raise ValueError(f"{what}: contiguous CUDA tensors of {'float32' if float_ else '32-bit integers'}" + (f", {n} elements" if n is not None else ""))


def _host_rays(rays, dtype, dtype_name):
    """A host ray list as a flat C-contiguous array of `dtype` records (RAY_DTYPE, PATHRAY_DTYPE): given as such, or as float32 of shape
    (n, floats per record)."""
    k = dtype.itemsize // 4
    rays = np.asarray(rays)
    if rays.dtype != dtype:
        if rays.dtype != np.float32 or rays.ndim != 2 or rays.shape[1] != k:
            raise ValueError(f"host rays must be a numpy array of {dtype_name}, or float32 of shape (n, {k})")
        rays = np.ascontiguousarray(rays).view(dtype).reshape(-1)
    return np.ascontiguousarray(rays).reshape(-1)


def _device_rays(rays, dtype):
    """A device ray list: a contiguous float32 CUDA tensor of shape (n, floats per `dtype` record). Returns n."""
    import torch
    k = dtype.itemsize // 4
    if not rays.is_cuda or rays.dtype != torch.float32 or not rays.is_contiguous() or rays.dim() != 2 or rays.shape[1] != k:
        raise ValueError(f"device rays must be a contiguous float32 CUDA tensor of shape (n, {k})")
    return rays.shape[0]


def _check_out(out, device, dtype, size, message):
    """An output buffer of `size` elements of `dtype`: a contiguous CUDA tensor (device; a torch dtype) or a C-contiguous numpy array."""
    if device:
        ok = getattr(out, "is_cuda", False) and out.dtype == dtype and out.is_contiguous() and out.numel() == size
    else:
        ok = isinstance(out, np.ndarray) and out.dtype == dtype and out.flags.c_contiguous and out.size == size
    if not ok:
        raise ValueError(message)


# the two kinds of ray query (Context._ray_query): an RtRayHit record per ray, or one byte
_CLOSEST_HIT = ("rt_trace_rays", RAYHIT_DTYPE, "n RAYHIT_DTYPE records", "float32", 12)
_OCCLUSION = ("rt_occluded_rays", np.dtype(np.uint8), "n uint8", "uint8", 1)


def output_floats(params):
    n = C.c_uint64(0)
    _check(lib().rt_output_floats(C.byref(params), C.byref(n)))
    return n.value


def _vec(v):
    return (C.c_double * len(v))(*[float(x) for x in v])


def camera_new(lookfrom, lookat, vup, vfov, aspect_ratio, aperture, focus_dist, time0, time1):
    """Camera::new (camera.rs:21-59)."""
    cam = A.RtCamera()
    lib().rt_host_camera_new(_vec(lookfrom), _vec(lookat), _vec(vup), _vec([vfov, aspect_ratio, aperture, focus_dist]), time0, time1, C.byref(cam))
    return cam


def write_color(pixel_color, spp):
    """write_color (main.rs:141-169) for one pixel sum."""
    out = (C.c_uint8 * 3)()
    lib().rt_host_write_color(_vec(pixel_color), spp, out)
    return tuple(out)


def tonemap(rgb_sum, spp):
    rgb_sum = np.ascontiguousarray(rgb_sum, dtype=np.float32)
    h, w, _ = rgb_sum.shape
    out = np.empty((h, w, 3), dtype=np.uint8)
    _check(lib().rt_host_tonemap(rgb_sum.ctypes.data_as(C.POINTER(C.c_float)), w, h, spp, out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


def write_png(path, rgb8):
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w, _ = rgb8.shape
    return lib().rt_host_write_png(str(path).encode(), rgb8.ctypes.data_as(C.POINTER(C.c_uint8)), w, h)


def write_image(path, rgb8, quality=100):
    """rt_host_write_image: creates the parent directories and encodes by extension (.jpg at `quality` — the reference's
    output/book3/image12.jpg, main.rs:653-656,791-796 — or .png)."""
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w, _ = rgb8.shape
    return lib().rt_host_write_image(str(path).encode(), rgb8.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, quality)


def untile(params, gathered):
    gathered = np.ascontiguousarray(gathered, dtype=np.float32)
    out = np.zeros((params.height, params.width, 3), dtype=np.float32)
    _check(lib().rt_untile(C.byref(params), gathered.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def untile_rgb8(params, gathered):
    gathered = np.ascontiguousarray(gathered, dtype=np.uint8)
    out = np.zeros((params.height, params.width, 3), dtype=np.uint8)
    _check(lib().rt_untile_rgb8(C.byref(params), gathered.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


def comm_unique_id():
    """rt_comm_unique_id: the 128 bytes rank 0 hands to every other rank (over the launcher's own channel)."""
    buf = (C.c_uint8 * A.RT_COMM_ID_BYTES)()
    _check(lib().rt_comm_unique_id(buf))
    return bytes(buf)


def compile_info(desc, layout_flags=0, **more):
    """rt_scene_compile_info[_ex]: what the scene compiler makes of a graph (host only); `more` as for upload_options."""
    info = A.RtCompileInfo()
    opt = upload_options(layout_flags, **more)
    _check(lib().rt_scene_compile_info_ex(C.byref(desc), C.byref(opt), C.byref(info)))
    out = {n: getattr(info, n) for n, _ in info._fields_ if n != "first"}
    out["first"] = [int(info.first[k]) for k in range(info.n_first)]
    return out


def wide_layout_check(desc):
    """rt_scene_wide_layout_check: builds and verifies the 8-wide tree of a static BVH on the host; returns its statistics."""
    info = A.RtWideInfo()
    _check(lib().rt_scene_wide_layout_check(C.byref(desc), C.byref(info)))
    return {n: getattr(info, n) for n, _ in info._fields_ if not n.startswith("_")}


def compile_dump(desc, layout_flags=0, **more):
    """rt_scene_compile_dump[_ex]: (nodes structured array, spheres (n,4) f32, sphere_meta u32); `more` as for upload_options."""
    info = compile_info(desc, layout_flags, **more)
    opt = upload_options(layout_flags, **more)
    node_t = np.dtype([("mn", np.float32, 3), ("skip", np.uint32), ("mx", np.float32, 3), ("leaf", np.uint32)])
    nodes = np.zeros(info["n_nodes"], dtype=node_t)
    n_s = max(1, info["n_spheres"] + info["n_media"])   # media boundaries add private spheres
    spheres = np.zeros((n_s, 4), dtype=np.float32)
    meta = np.zeros(n_s, dtype=np.uint32)
    _check(lib().rt_scene_compile_dump_ex(C.byref(desc), C.byref(opt), nodes.ctypes.data_as(C.c_void_p), len(nodes), spheres.ctypes.data_as(C.POINTER(C.c_float)),
                                          meta.ctypes.data_as(C.POINTER(C.c_uint32)), n_s))
    return nodes, spheres[:info["n_spheres"]], meta[:info["n_spheres"]]


def camera_lists_host(desc, cam, width, height):
    """rt_camera_lists_host: the camera lists of a width x height frame as a (squares, 17) uint32 array — row-major over
    ceil(width / 8) x ceil(height / 8) squares; column 0 the count (A.RT_CAMERA_LIST_WALK: more than 16), then sphere indices in leaf
    order. None: the lists do not serve this scene or camera."""
    n = C.c_uint64(0)
    _check(lib().rt_camera_lists_host(C.byref(desc), C.byref(cam), width, height, None, 0, C.byref(n)))
    if n.value == 0:
        return None
    out = np.zeros((n.value, A.RT_CAMERA_LIST_WORDS), dtype=np.uint32)
    _check(lib().rt_camera_lists_host(C.byref(desc), C.byref(cam), width, height, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(n)))
    return out


class HostScene:
    """A scene function of main.rs, built by the C++ host mirror (host/rt_host.hpp)."""

    def __init__(self, name, scene_seed=1, arg0=0, arg1=0, image=None):
        self._h = C.c_void_p()
        self._image = None
        ip, iw, ih = None, 0, 0
        if image is not None:
            self._image = np.ascontiguousarray(image, dtype=np.uint8)
            ih, iw, _ = self._image.shape
            ip = self._image.ctypes.data_as(C.POINTER(C.c_uint8))
        _check(lib().rt_host_scene_create(name.encode(), scene_seed, arg0, arg1, ip, iw, ih, C.byref(self._h)))
        self.name = name

    @property
    def desc(self):
        return lib().rt_host_scene_desc(self._h).contents

    def camera(self, aspect_ratio):
        cam = A.RtCamera()
        _check(lib().rt_host_scene_camera(self._h, float(aspect_ratio), C.byref(cam)))
        return cam

    def close(self):
        if self._h:
            lib().rt_host_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def upload_options(layout_flags=0, lds_top_records=0, octant_axes=0, leaf_collapse=0, list_park_cost=0.0, triangle_attrs=None, env_map=None, normal_maps=None):
    """RtUploadOptions (include/rt_hip.h): how the scene is laid out on the device, never what it looks like — and the per-vertex normals /
    texture coordinates of its triangles: triangle_attrs = a ctypes array or a sequence of RtTriangleAttrs (SceneBuilder.triangle_attrs()) —
    and its environment map: env_map = an environment.EnvMap; the record returned is then the first 40 bytes of an RtUploadOptionsEnv, with
    struct_bytes = its 48 — and the normal maps of its materials: normal_maps = a ctypes array or a sequence of RtNormalMap
    (SceneBuilder.normal_maps(); an empty sequence is a list of none); the record is then the first 40 bytes of an RtUploadOptionsMaps, with
    struct_bytes = its 64."""
    if normal_maps is not None:                             # the record grown twice: its first 40 bytes are the options, and those are what is handed on
        big = A.RtUploadOptionsMaps()
        opt = big.base.base                                 # (a view into big, which it keeps alive)
        opt.struct_bytes = C.sizeof(A.RtUploadOptionsMaps)
        if len(normal_maps):
            maps = normal_maps if isinstance(normal_maps, C.Array) else (A.RtNormalMap * len(normal_maps))(*normal_maps)
            big.normal_maps, big.n_normal_maps = maps, len(maps)
            opt._keep_maps = maps                           # the record points into it
        if env_map is not None:
            big.base.env_map = C.pointer(env_map.record)
            opt._keep_env = env_map                         # the record points into its texels
    elif env_map is not None:                               # the grown record, likewise
        ext = A.RtUploadOptionsEnv()
        ext.env_map = C.pointer(env_map.record)
        opt = ext.base
        opt.struct_bytes = C.sizeof(A.RtUploadOptionsEnv)
        opt._keep_env = env_map
    else:
        opt = A.RtUploadOptions(C.sizeof(A.RtUploadOptions))
    opt.layout_flags, opt.lds_top_records, opt.octant_axes, opt.leaf_collapse, opt.list_park_cost = layout_flags, lds_top_records, octant_axes, leaf_collapse, list_park_cost
    if triangle_attrs is not None and len(triangle_attrs):
        arr = triangle_attrs if isinstance(triangle_attrs, C.Array) else (A.RtTriangleAttrs * len(triangle_attrs))(*triangle_attrs)
        opt.triangle_attrs, opt.n_triangle_attrs = arr, len(arr)
        opt._keep = arr                                     # the options point into it
    return opt


def runtime_libraries():
    """rt_runtime_libraries: (paths of the mapped libamdhip64 / libhsa-runtime64 / librccl objects, ok) — ok is False when one is mapped twice."""
    buf = C.create_string_buffer(8192)
    code = lib().rt_runtime_libraries(buf, len(buf))
    return [p for p in buf.value.decode().split("\n") if p], code == A.RT_OK


def scene_fingerprint(desc, triangle_attrs=None, env_map=None, normal_maps=None):
    """sha256 (hex) over the arrays and scalars of an RtSceneDesc — and over the RtTriangleAttrs records that travel beside it, if any sets a
    flag, over the environment map (an environment.EnvMap), if there is one, and over the RtNormalMap records, if there are any (their
    images are the desc's, so covered already): what a progressive checkpoint records of the scene it was rendered from. A scene without
    attributes and without maps has the print it always had; of a record only what its flags make the library read counts, in the order of
    the hittable ids (normal maps: of the material ids)."""
    import hashlib
    h = hashlib.sha256()

    def arr(ptr, n, ctype):
        h.update(int(n).to_bytes(8, "little"))
        if n and ptr:
            h.update(C.string_at(C.cast(ptr, C.c_void_p).value, int(n) * C.sizeof(ctype)))

    arr(desc.hittables, desc.n_hittables, A.RtHittable)
    arr(desc.children, desc.n_children, C.c_int32)
    arr(desc.materials, desc.n_materials, A.RtMaterial)
    arr(desc.textures, desc.n_textures, A.RtTexture)
    arr(desc.perlins, desc.n_perlins, A.RtPerlin)
    h.update(int(desc.n_images).to_bytes(8, "little"))
    for k in range(desc.n_images if desc.images else 0):
        im = desc.images[k]
        h.update(np.array([im.width, im.height], dtype=np.uint32).tobytes())
        if im.data:
            h.update(C.string_at(C.cast(im.data, C.c_void_p).value, im.width * im.height * 3))
    h.update(np.array([desc.world, desc.lights, desc.background_mode, desc.bvh_builder], dtype=np.int32).tobytes())
    h.update(np.array(desc.background.tuple(), dtype=np.float64).tobytes() + int(desc.bvh_seed).to_bytes(8, "little"))
    if desc.scene_flags:                                     # (a scene without flags has the print it always had)
        h.update(b"scene_flags" + int(desc.scene_flags).to_bytes(4, "little"))
    live = sorted((a for a in (triangle_attrs if triangle_attrs is not None else ()) if a.flags), key=lambda a: a.hittable)
    if live:
        h.update(b"triangle_attrs" + len(live).to_bytes(8, "little"))
        for a in live:
            h.update(np.array([a.hittable, a.flags], dtype=np.int64).tobytes())
            if a.flags & A.RT_TRI_NORMALS:
                h.update(bytes(a.n))
            if a.flags & A.RT_TRI_UVS:
                h.update(bytes(a.uv))
    if env_map is not None:
        r = env_map.record
        h.update(b"env_map" + np.array([r.flags, r.width, r.height], dtype=np.uint32).tobytes() + np.float32(r.scale).tobytes() + env_map.rgb.tobytes())
    maps = sorted(normal_maps if normal_maps is not None else (), key=lambda m: m.material)
    if maps:
        h.update(b"normal_maps" + len(maps).to_bytes(8, "little"))
        for m in maps:
            h.update(np.array([m.material, m.image, m.flags], dtype=np.int64).tobytes() + np.float32(m.strength).tobytes())
    return h.hexdigest()


class Scene:
    def __init__(self, ctx, desc, options=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        _check(lib().rt_scene_upload_ex(ctx._h, C.byref(desc), C.byref(options) if options is not None else None, C.byref(self._h)), ctx._h)
        attrs = getattr(options, "_keep", None) if options is not None and options.struct_bytes >= C.sizeof(A.RtUploadOptions) else None
        env = getattr(options, "_keep_env", None) if options is not None and options.struct_bytes >= C.sizeof(A.RtUploadOptionsEnv) else None
        if env is not None and not getattr(options, "_b_base_").env_map:
            env = None                                       # (the field was cleared after upload_options set it)
        maps = getattr(options, "_keep_maps", None) if options is not None and options.struct_bytes >= C.sizeof(A.RtUploadOptionsMaps) else None
        self.fingerprint = scene_fingerprint(desc, attrs, env, maps)   # (progressive checkpoints: the scene a frame's sums belong to)

    def close(self):
        if self._h and self.ctx._h:
            lib().rt_scene_destroy(self.ctx._h, self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """rt_ctx_create: one per (process, device, stream)."""

    def __init__(self, device_id=0, stream=None):
        self._h = C.c_void_p()
        self.device_id = device_id
        _check(lib().rt_ctx_create(device_id, C.c_void_p(stream) if stream else None, C.byref(self._h)))

    def upload(self, desc, layout_flags=0, **more):
        """rt_scene_upload_ex; layout_flags = RT_LAYOUT_* (A.RT_LAYOUT_REFERENCE_COUNTERS: the layout whose test counts are the reference's);
        triangle_attrs= (in `more`): RtTriangleAttrs records, env_map= an environment.EnvMap, normal_maps= RtNormalMap records, see upload_options."""
        return Scene(self, desc, upload_options(layout_flags, **more) if (layout_flags or more) else None)

    def fail_next_renders(self, n):
        """rt_test_fail_next_renders: fault injection for the failure-path tests."""
        _check(lib().rt_test_fail_next_renders(self._h, n), self._h)

    def render(self, scene, cam, params):
        """rt_render: returns (rgb_sum float32 array, stats dict). Full frame -> (H, W, 3); sharded -> flat."""
        n = output_floats(params)
        out = np.empty(n, dtype=np.float32)
        st = A.RtStats()
        _check(lib().rt_render(self._h, scene._h, C.byref(cam), C.byref(params), out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)), self._h)
        if params.shard_count <= 1:
            out = out.reshape(params.height, params.width, 3)
        return out, st.as_dict()

    def camera_lists_last(self):
        """rt_camera_lists_last: the camera lists the last render or pass built on the device, as camera_lists_host returns them; None: it built none."""
        n = C.c_uint64(0)
        _check(lib().rt_camera_lists_last(self._h, None, 0, C.byref(n)), self._h)
        if n.value == 0:
            return None
        out = np.zeros((n.value, A.RT_CAMERA_LIST_WORDS), dtype=np.uint32)
        _check(lib().rt_camera_lists_last(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(n)), self._h)
        return out

    def render_device(self, scene, cam, params, device_ptr):
        """rt_render_device: result stays in caller-owned device memory (e.g. a torch tensor's data_ptr())."""
        st = A.RtStats()
        _check(lib().rt_render_device(self._h, scene._h, C.byref(cam), C.byref(params), C.c_void_p(device_ptr), C.byref(st)), self._h)
        return st.as_dict()

    def render_pass(self, scene, cam, params, first_sample, frame_samples, accumulate, rgb_sum=None, sq_sum=None):
        """rt_render_pass / rt_render_pass_device: samples first_sample .. first_sample + params.samples_per_pixel - 1 of a frame of
        frame_samples samples per pixel, overwriting (accumulate False) or adding into (True) rgb_sum and, if given, sq_sum.

        Host variant: rgb_sum / sq_sum are numpy float32 arrays of output_floats(params) elements (None: a new one; accumulating needs
        the caller's). Device variant: torch tensors on this context's GPU (both of them, or rgb_sum alone). Returns
        (rgb_sum, sq_sum, stats); a full-frame host result is shaped (H, W, 3)."""
        opt = A.RtPassOptions(C.sizeof(A.RtPassOptions), A.RT_PASS_ACCUMULATE if accumulate else 0, first_sample, frame_samples)
        st = A.RtStats()
        n = output_floats(params)
        if rgb_sum is not None and hasattr(rgb_sum, "data_ptr"):
            import torch
            for t in (rgb_sum, sq_sum):
                if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n):
                    raise ValueError(f"device buffers must be contiguous float32 CUDA tensors of {n} elements")
            torch.cuda.synchronize(rgb_sum.device)        # the library's stream is not torch's
            _check(lib().rt_render_pass_device(self._h, scene._h, C.byref(cam), C.byref(params), C.byref(opt), C.c_void_p(rgb_sum.data_ptr()),
                                               C.c_void_p(sq_sum.data_ptr()) if sq_sum is not None else None, C.byref(st)), self._h)
            return rgb_sum, sq_sum, st.as_dict()
        if rgb_sum is None:
            if accumulate:
                raise ValueError("an accumulating host pass needs the sums to add into (rgb_sum)")
            rgb_sum = np.empty(n, dtype=np.float32)
        for a in (rgb_sum, sq_sum):
            if a is not None and (not isinstance(a, np.ndarray) or a.dtype != np.float32 or not a.flags.c_contiguous or a.size != n):
                raise ValueError(f"host buffers must be C-contiguous float32 numpy arrays of {n} elements")
        fp = C.POINTER(C.c_float)
        _check(lib().rt_render_pass(self._h, scene._h, C.byref(cam), C.byref(params), C.byref(opt), rgb_sum.ctypes.data_as(fp),
                                    sq_sum.ctypes.data_as(fp) if sq_sum is not None else None, C.byref(st)), self._h)
        if params.shard_count <= 1:
            rgb_sum = rgb_sum.reshape(params.height, params.width, 3)
            sq_sum = sq_sum.reshape(params.height, params.width, 3) if sq_sum is not None else None
        return rgb_sum, sq_sum, st.as_dict()

    # ---- adaptive sampling (include/rt_hip.h, "adaptive sampling"): device tensors only ----
    def adaptive_select(self, params, options, first_sample, frame_samples, rgb_sum, sq_sum, counts, pixels_out):
        """rt_adaptive_select: writes the active list (ascending output slots, int32/uint32 tensor of at least output_floats / 3 entries)
        into pixels_out and returns its length."""
        slots = output_floats(params) // 3
        _check_device(rgb_sum, sq_sum, n=3 * slots, what="rgb_sum / sq_sum", float_=True)
        _check_device(counts, pixels_out, n=slots, what="counts / pixels_out", float_=False)
        n = C.c_uint32(0)
        import torch
        torch.cuda.synchronize(rgb_sum.device)
        _check(lib().rt_adaptive_select(self._h, C.byref(params), C.byref(options), first_sample, frame_samples, C.c_void_p(rgb_sum.data_ptr()),
                                        C.c_void_p(sq_sum.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(pixels_out.data_ptr()), C.byref(n)), self._h)
        return n.value

    def render_pass_pixels(self, scene, cam, params, first_sample, frame_samples, accumulate, pixels, n_pixels, rgb_sum, sq_sum, counts):
        """rt_render_pass_pixels_device: samples first_sample .. first_sample + params.samples_per_pixel - 1 of the first n_pixels slots
        of `pixels` only; counts of those slots become the pass's end. sq_sum may be None. Returns the stats."""
        slots = output_floats(params) // 3
        _check_device(rgb_sum, sq_sum, n=3 * slots, what="rgb_sum / sq_sum", float_=True)
        _check_device(counts, None, n=slots, what="counts", float_=False)
        _check_device(pixels, None, n=None, what="pixels", float_=False)
        if n_pixels > pixels.numel():
            raise ValueError("n_pixels is larger than the pixel list")
        opt = A.RtPassOptions(C.sizeof(A.RtPassOptions), A.RT_PASS_ACCUMULATE if accumulate else 0, first_sample, frame_samples)
        st = A.RtStats()
        import torch
        torch.cuda.synchronize(rgb_sum.device)
        _check(lib().rt_render_pass_pixels_device(self._h, scene._h, C.byref(cam), C.byref(params), C.byref(opt), C.c_void_p(pixels.data_ptr()), n_pixels,
                                                  C.c_void_p(rgb_sum.data_ptr()), C.c_void_p(sq_sum.data_ptr()) if sq_sum is not None else None,
                                                  C.c_void_p(counts.data_ptr()), C.byref(st)), self._h)
        return st.as_dict()

    def resolve_counts_device(self, rgb_sum, counts, width, height, rgb8_out):
        """rt_resolve_counts_device: write_color of a full frame with every pixel's own sample count, into a uint8 tensor."""
        _check_device(rgb_sum, None, n=3 * width * height, what="rgb_sum", float_=True)
        _check_device(counts, None, n=width * height, what="counts", float_=False)
        import torch
        if not rgb8_out.is_cuda or rgb8_out.dtype != torch.uint8 or not rgb8_out.is_contiguous() or rgb8_out.numel() != 3 * width * height:
            raise ValueError("rgb8_out must be a contiguous uint8 CUDA tensor of width * height * 3 elements")
        torch.cuda.synchronize(rgb_sum.device)
        _check(lib().rt_resolve_counts_device(self._h, C.c_void_p(rgb_sum.data_ptr()), C.c_void_p(counts.data_ptr()), width, height,
                                              C.c_void_p(rgb8_out.data_ptr())), self._h)

    # ---- ray queries (include/rt_hip.h, "ray queries") ----
    def _ray_query(self, kind, scene, rays, options, out, with_stats):
        """trace_rays and occluded: kind = (host entry point — its device variant is that + "_device", a result's numpy dtype, what the
        host message calls n of them, the torch dtype's name and the elements per ray of a device result). The two call it through the
        class: a host test hands them a stand-in for a context, which the argument checks below never touch."""
        name, np_dtype, n_of_them, torch_name, per_ray = kind
        st = A.RtStats()
        opt = C.byref(options) if options is not None else None
        if hasattr(rays, "data_ptr"):
            import torch
            n = _device_rays(rays, RAY_DTYPE)
            if out is None:
                out = torch.empty((n, per_ray) if per_ray > 1 else (n,), dtype=getattr(torch, torch_name), device=rays.device)
            _check_out(out, True, getattr(torch, torch_name), per_ray * n,
                       f"out must be a contiguous {torch_name} CUDA tensor of {'n * %d' % per_ray if per_ray > 1 else 'n'} elements")
            if rays.device.index != self.device_id or out.device != rays.device:      # another GPU's pointer means nothing to this context's kernels
                raise ValueError(f"rays and out must live on this context's device (cuda:{self.device_id})")
            torch.cuda.synchronize(rays.device)           # the library's stream is not torch's
            fn, p_rays, p_out = getattr(lib(), name + "_device"), rays.data_ptr(), out.data_ptr()
        else:
            rays = _host_rays(rays, RAY_DTYPE, "RAY_DTYPE")
            n = rays.shape[0]
            if out is None:
                out = np.empty(n, dtype=np_dtype)
            _check_out(out, False, np_dtype, n, f"out must be a C-contiguous numpy array of {n_of_them}")
            fn, p_rays, p_out = getattr(lib(), name), rays.ctypes.data, out.ctypes.data
        _check(fn(self._h, scene._h, opt, C.c_void_p(p_rays if n else None), n, C.c_void_p(p_out if n else None), C.byref(st)), self._h)
        return (out, st.as_dict()) if with_stats else out

    def trace_rays(self, scene, rays, options=None, out=None, with_stats=False):
        """rt_trace_rays / rt_trace_rays_device: the closest hit of every ray.

        Host variant: `rays` is a numpy array of RAY_DTYPE (or float32 of shape (n, 8): o, time, d, t_max); returns a RAYHIT_DTYPE array.
        Device variant: `rays` is a contiguous float32 CUDA tensor of shape (n, 8); returns a float32 CUDA tensor of shape (n, 12) holding
        the RtRayHit records (view the integer fields with .view(torch.int32), or RAYHIT_DTYPE after .cpu().numpy()). `out` receives the
        hits when given (same kind and size); a refused call raises RtError and leaves it untouched. with_stats: also return the stats."""
        return Context._ray_query(self, _CLOSEST_HIT, scene, rays, options, out, with_stats)

    def occluded(self, scene, rays, options=None, out=None, with_stats=False):
        """rt_occluded_rays / rt_occluded_rays_device: one byte per ray — RT_RAYHIT_HIT (1) when anything is hit in [0.001, t_max], else 0;
        RT_RAYHIT_INVALID_RAY (4) for a ray that is never traced. Exactly the hit / miss of trace_rays, for less work.

        `rays` as for trace_rays: a numpy array of RAY_DTYPE or float32 of shape (n, 8) (host variant, returns a uint8 numpy array of length
        n), or a contiguous float32 CUDA tensor of shape (n, 8) (device variant, returns a uint8 CUDA tensor of length n). `out` receives
        the bytes when given (same kind, n elements); a refused call raises RtError and leaves it untouched. with_stats: also the stats."""
        return Context._ray_query(self, _OCCLUSION, scene, rays, options, out, with_stats)

    # ---- light-sample queries (include/rt_hip.h, "light-sample queries") ----
    def _light_queries(self, scene, q, with_stats):
        st = A.RtStats()
        n = q.shape[0]
        out = np.empty(n, dtype=LIGHTSAMPLE_DTYPE)
        _check(lib().rt_sample_lights(self._h, scene._h, None, C.c_void_p(q.ctypes.data if n else None), n, C.c_void_p(out.ctypes.data if n else None),
                                      C.byref(st)), self._h)
        return (out, st.as_dict()) if with_stats else out

    def sample_lights(self, scene, points, states, with_stats=False):
        """rt_sample_lights: for every point (float32, shape (n, 3)) and generator state (uint64, n) one pick of the scene's lights list, the
        picked member's draw and the list's pdf of the drawn direction — what a Lambertian bounce of a render does for its light half, by the
        same device functions. Returns a LIGHTSAMPLE_DTYPE array: d (not normalised), pdf, light (the member's index), n_draws."""
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        states = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1)
        if states.shape[0] != points.shape[0]:
            raise ValueError("one generator state per point")
        q = np.zeros(points.shape[0], dtype=LIGHTQUERY_DTYPE)
        q["p"], q["rng_state"] = points, states
        return self._light_queries(scene, q, with_stats)

    def light_pdf(self, scene, points, dirs, with_stats=False, linear=False):
        """rt_sample_lights with RT_LIGHTQ_DIRECTION_GIVEN: the lights list's pdf_value at (point, direction), nothing drawn. Returns the pdfs
        (float32, n). linear: RT_LIGHTQ_LINEAR — a scene with a light tree (RT_SCENE_LIGHTS_MANY) evaluates the sum by the plain loop over its
        table instead of through the tree; any other scene ignores it."""
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        if dirs.shape[0] != points.shape[0]:
            raise ValueError("one direction per point")
        q = np.zeros(points.shape[0], dtype=LIGHTQUERY_DTYPE)
        q["p"], q["d"], q["flags"] = points, dirs, A.RT_LIGHTQ_DIRECTION_GIVEN | (A.RT_LIGHTQ_LINEAR if linear else 0)
        r = self._light_queries(scene, q, with_stats)
        return (r[0]["pdf"].copy(), r[1]) if with_stats else r["pdf"].copy()

    # ---- radiance queries (include/rt_hip.h, "radiance queries") ----
    def radiance(self, scene, rays, samples, max_depth=50, seed=1, first_sample=0, first_stream=0, accumulate=False, rgb_sum=None, sq_sum=None,
                 invalid=None, nan_policy=A.RT_NAN_PER_SAMPLE, pool_slots=0, tail_paths=0, with_stats=False, options=None):
        """rt_radiance_rays / rt_radiance_rays_device: the path tracer on the caller's rays. Ray i is traced `samples` times on the streams
        (seed, first_stream + i, first_sample .. first_sample + samples - 1); returns (rgb_sum, sq_sum, invalid): per ray the RGB sum of the
        samples, the sum of their squares (both float32, shape (n, 3)) and a flag byte (RT_RAYHIT_INVALID_RAY for a ray that is never traced).

        Host variant: `rays` is a numpy array of PATHRAY_DTYPE (or float32 of shape (n, 8): o, time, d, and first_draw's bits); numpy results.
        Device variant: `rays` is a contiguous float32 CUDA tensor of shape (n, 8); CUDA tensors. rgb_sum / sq_sum / invalid receive the
        results when given (same kind, 3 n / 3 n / n elements); accumulate=True folds on from the sums they hold. A refused call raises RtError
        and leaves them untouched. options: an RtRadianceOptions to pass as it is (radiance_options). with_stats: also return the stats."""
        st = A.RtStats()
        if options is None:
            options = radiance_options(samples, max_depth, seed, first_sample, first_stream, accumulate, nan_policy, pool_slots, tail_paths)
        acc = bool(options.flags & A.RT_RADIANCE_ACCUMULATE)
        if acc and (rgb_sum is None or sq_sum is None):
            raise ValueError("accumulate needs the rgb_sum and sq_sum of the samples so far")
        if hasattr(rays, "data_ptr"):
            import torch
            n = _device_rays(rays, PATHRAY_DTYPE)
            if rgb_sum is None:
                rgb_sum = torch.empty((n, 3), dtype=torch.float32, device=rays.device)
            if sq_sum is None:
                sq_sum = torch.empty((n, 3), dtype=torch.float32, device=rays.device)
            if invalid is None:
                invalid = torch.empty((n,), dtype=torch.uint8, device=rays.device)
            _check_device(rgb_sum, sq_sum, 3 * n, "rgb_sum / sq_sum", True)
            _check_out(invalid, True, torch.uint8, n, "invalid must be a contiguous uint8 CUDA tensor of n elements")
            if rays.device.index != self.device_id or any(t.device != rays.device for t in (rgb_sum, sq_sum, invalid)):
                raise ValueError(f"rays and outputs must live on this context's device (cuda:{self.device_id})")
            torch.cuda.synchronize(rays.device)           # the library's stream is not torch's
            ptr = lambda t: C.c_void_p(t.data_ptr() if n else None)
            _check(lib().rt_radiance_rays_device(self._h, scene._h, C.byref(options), ptr(rays), n, ptr(rgb_sum), ptr(sq_sum), ptr(invalid), C.byref(st)), self._h)
        else:
            rays = _host_rays(rays, PATHRAY_DTYPE, "PATHRAY_DTYPE")
            n = rays.shape[0]
            if rgb_sum is None:
                rgb_sum = np.empty((n, 3), dtype=np.float32)
            if sq_sum is None:
                sq_sum = np.empty((n, 3), dtype=np.float32)
            if invalid is None:
                invalid = np.empty(n, dtype=np.uint8)
            for a, dt, k, what in ((rgb_sum, np.float32, 3 * n, "rgb_sum"), (sq_sum, np.float32, 3 * n, "sq_sum"), (invalid, np.uint8, n, "invalid")):
                _check_out(a, False, dt, k, f"{what} must be a C-contiguous numpy array of {k} {np.dtype(dt).name}")
            ptr = lambda a: C.c_void_p(a.ctypes.data if n else None)
            _check(lib().rt_radiance_rays(self._h, scene._h, C.byref(options), ptr(rays), n, ptr(rgb_sum), ptr(sq_sum), ptr(invalid), C.byref(st)), self._h)
        return (rgb_sum, sq_sum, invalid, st.as_dict()) if with_stats else (rgb_sum, sq_sum, invalid)

    # ---- first-hit features (include/rt_hip.h, "first-hit features"): device tensors only ----
    def _feature_pass(self, table, scene, cam, params, first_sample, accumulate, planes, pool_slots, with_stats):
        """render_features and render_feature_moments: table = (entry point, what makes its buffers record of the planes, elements per slot
        of every plane — plane 3, hits, holds integers —, the planes checked together as (plane, plane or None, what the message calls them))."""
        import torch
        name, make_buffers, per_slot, checked = table
        slots = output_floats(params) // 3
        if all(t is None for t in planes):
            if accumulate:
                raise ValueError("an accumulating feature pass needs the planes to add into")
            dev = torch.device("cuda", self.device_id)
            planes = tuple(torch.zeros(k * slots, dtype=torch.int32 if i == 3 else torch.float32, device=dev) for i, k in enumerate(per_slot))
        for i, j, what in checked:
            _check_device(planes[i], planes[j] if j is not None else None, n=per_slot[i] * slots, what=what, float_=i != 3)
        if any(t is not None and t.device.index != self.device_id for t in planes):      # another GPU's pointer means nothing to this context's kernels
            raise ValueError(f"feature planes must live on this context's device (cuda:{self.device_id})")
        opt = feature_options(first_sample, accumulate, pool_slots)
        buf = make_buffers(*planes)
        st = A.RtStats()
        torch.cuda.synchronize(torch.device("cuda", self.device_id))        # the library's stream is not torch's
        _check(getattr(lib(), name)(self._h, scene._h, C.byref(cam), C.byref(params), C.byref(opt), C.byref(buf), C.byref(st)), self._h)
        return planes + (st.as_dict(),) if with_stats else planes

    def render_features(self, scene, cam, params, first_sample=0, accumulate=False, albedo=None, normal=None, depth=None, hits=None, pool_slots=0,
                        with_stats=False):
        """rt_render_features_device: per-slot sums of the first hit's albedo, normal and depth, and the number of hits, over samples
        first_sample .. first_sample + params.samples_per_pixel - 1 of the render's own camera rays.

        albedo / normal: float32 CUDA tensors of 3 * slots elements (slots = output_floats(params) // 3), depth: float32 of slots, hits: a
        32-bit integer tensor of slots. Only the planes given are written; with none given all four are made (zero-filled, so clipped slots
        of a sharded layout read 0). accumulate: the fold starts from the planes' values. Returns (albedo, normal, depth, hits), None for a
        plane not wanted, and the stats too with with_stats. A refused call raises RtError and leaves the planes untouched."""
        return self._feature_pass(_FEATURE_PLANES, scene, cam, params, first_sample, accumulate, (albedo, normal, depth, hits), pool_slots, with_stats)

    def render_feature_moments(self, scene, cam, params, first_sample=0, accumulate=False, albedo=None, normal=None, depth=None, hits=None, albedo_sq=None,
                               normal_sq=None, depth_sq=None, pool_slots=0, with_stats=False):
        """rt_render_feature_moments_device: render_features with the per-slot sums of squares beside the sums — albedo_sq / normal_sq
        float32 of 3 * slots elements, depth_sq float32 of slots. Only the planes given are written; with none given all seven are made
        (zero-filled). Returns (albedo, normal, depth, hits, albedo_sq, normal_sq, depth_sq), None for a plane not wanted, and the stats
        too with with_stats. A refused call raises RtError and leaves the planes untouched."""
        return self._feature_pass(_MOMENT_PLANES, scene, cam, params, first_sample, accumulate, (albedo, normal, depth, hits, albedo_sq, normal_sq, depth_sq), pool_slots,
                                  with_stats)

    # ---- denoising (include/rt_hip.h, "denoising"): device tensors only ----
    def _denoise(self, name, guide, planes, rgb_sum, sq_sum, width, height, samples, counts, options, out):
        """The three denoise methods: name = the entry point, guide = its guide record (None: the plain filter, which takes none), planes
        = the guide's tensors as _check_device takes them: (a, b or None, elements per pixel, what the message calls them, float_)."""
        import torch
        n = 3 * width * height
        _check_device(rgb_sum, sq_sum, n=n, what="rgb_sum / sq_sum", float_=True)
        if counts is not None:
            _check_device(counts, None, n=width * height, what="counts", float_=False)
        for a, b, per_pixel, what, float_ in planes:
            _check_device(a, b, n=per_pixel * width * height, what=what, float_=float_)
        if any(t is not None and t.device != rgb_sum.device for a, b, *_ in planes for t in (a, b, counts, sq_sum)):
            raise ValueError("the sums, the counts and the feature planes must live on one device")
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=rgb_sum.device)
        _check_device(out, None, n=n, what="out", float_=True)
        torch.cuda.synchronize(rgb_sum.device)        # the library's stream is not torch's
        records = (C.byref(options) if options is not None else None,) + ((C.byref(guide),) if guide is not None else ())
        _check(getattr(lib(), name)(self._h, *records, width, height, C.c_void_p(rgb_sum.data_ptr()), C.c_void_p(sq_sum.data_ptr()), int(samples),
                                    C.c_void_p(counts.data_ptr()) if counts is not None else None, C.c_void_p(out.data_ptr())), self._h)
        return out

    def denoise(self, rgb_sum, sq_sum, width, height, samples=0, counts=None, options=None, out=None):
        """rt_denoise_device: the filtered MEAN radiance of a full frame from its sums (float32 CUDA tensors of width * height * 3
        elements) and either the uniform sample count `samples` or per-pixel `counts` (32-bit integer tensor of width * height). Returns
        `out` (a new float32 tensor of width * height * 3 elements when None); a refused call raises RtError and leaves `out` untouched."""
        return self._denoise("rt_denoise_device", None, (), rgb_sum, sq_sum, width, height, samples, counts, options, out)

    def denoise_guided(self, rgb_sum, sq_sum, width, height, feature_samples, albedo=None, normal=None, depth=None, hits=None, samples=0, counts=None,
                       options=None, sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0, out=None):
        """rt_denoise_guided_device: Context.denoise with the weights joined with full-frame feature planes (render_features with
        shard_count <= 1: albedo / normal float32 of width * height * 3, depth float32 and hits 32-bit integers of width * height; None =
        not used) folded over feature_samples samples. Returns `out`; a refused call raises RtError and leaves `out` untouched."""
        guide = denoise_guide(feature_samples, albedo, normal, depth, hits, sigma_albedo, sigma_normal, sigma_depth)
        planes = ((albedo, normal, 3, "albedo / normal", True), (depth, None, 1, "depth", True), (hits, None, 1, "hits", False))
        return self._denoise("rt_denoise_guided_device", guide, planes, rgb_sum, sq_sum, width, height, samples, counts, options, out)

    def denoise_guided_moments(self, rgb_sum, sq_sum, width, height, feature_samples, albedo=None, normal=None, depth=None, hits=None, albedo_sq=None,
                               normal_sq=None, depth_sq=None, samples=0, counts=None, options=None, sigma_albedo=0.0, sigma_normal=0.0, sigma_depth=0.0,
                               variance_strength=0.0, out=None):
        """rt_denoise_guided_moments_device: Context.denoise_guided with the feature distance variance-cancelled and variance-normalised
        from the squared sums of render_feature_moments (albedo_sq / normal_sq float32 of width * height * 3, depth_sq float32 of
        width * height; None = that group's variance is 0), feature_samples >= 2. window_radius 0 means 8 here, at most 8. Returns `out`;
        a refused call raises RtError and leaves `out` untouched."""
        guide = denoise_guide_moments(feature_samples, albedo, normal, depth, hits, albedo_sq, normal_sq, depth_sq, sigma_albedo, sigma_normal, sigma_depth,
                                      variance_strength)
        planes = ((albedo, normal, 3, "albedo / normal", True), (albedo_sq, normal_sq, 3, "albedo_sq / normal_sq", True), (depth, depth_sq, 1, "depth / depth_sq", True),
                  (hits, None, 1, "hits", False))
        return self._denoise("rt_denoise_guided_moments_device", guide, planes, rgb_sum, sq_sum, width, height, samples, counts, options, out)

    # ---- one process per GPU: RCCL communicator on this context (rt_multi.cpp) ----
    def comm_init_rank(self, unique_id, rank, world):
        buf = (C.c_uint8 * A.RT_COMM_ID_BYTES)(*unique_id)
        _check(lib().rt_comm_init_rank(self._h, buf, rank, world), self._h)

    def comm_selftest(self):
        _check(lib().rt_comm_selftest(self._h), self._h)

    def render_gather(self, scene, cam, params, output_kind=A.RT_OUT_RGB_SUM_F32, frame_ptr=None):
        """rt_render_gather (collective): this rank's shard is rendered and sent to rank 0, which leaves the full frame at frame_ptr."""
        st = A.RtStats()
        _check(lib().rt_render_gather(self._h, scene._h, C.byref(cam), C.byref(params), output_kind, C.c_void_p(frame_ptr) if frame_ptr else None, C.byref(st)),
               self._h)
        return st.as_dict()

    def untile_device(self, params, output_kind, gathered_ptr, frame_ptr):
        _check(lib().rt_untile_device(self._h, C.byref(params), output_kind, C.c_void_p(gathered_ptr), C.c_void_p(frame_ptr)), self._h)

    def resolve_device(self, rgb_sum_ptr, width, height, spp, rgb8_ptr):
        _check(lib().rt_resolve_device(self._h, C.c_void_p(rgb_sum_ptr), width, height, spp, C.c_void_p(rgb8_ptr)), self._h)

    def close(self):
        if self._h:
            lib().rt_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiScene:
    def __init__(self, mctx, desc, options=None):
        self.mctx = mctx
        self._h = C.c_void_p()
        code = lib().rt_scene_upload_multi_ex(mctx._h, C.byref(desc), C.byref(options) if options is not None else None, C.byref(self._h))
        if code != A.RT_OK:
            raise RtError(code, lib().rt_last_error_multi(mctx._h).decode())

    def close(self):
        if self._h and self.mctx._h:
            lib().rt_scene_destroy_multi(self.mctx._h, self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiContext:
    """rt_ctx_create_multi: ONE process driving n GPUs (what the reference's single-process host binds). The framebuffer is
    tile-sharded over the devices and gathered on the first one with RCCL inside rt_render_multi."""

    def __init__(self, device_ids):
        self._h = C.c_void_p()
        ids = (C.c_int * len(device_ids))(*device_ids)
        _check(lib().rt_ctx_create_multi(ids, len(device_ids), C.byref(self._h)))
        self.n = len(device_ids)

    def upload(self, desc, layout_flags=0, **more):
        return MultiScene(self, desc, upload_options(layout_flags, **more) if (layout_flags or more) else None)

    def _render(self, fn, scene, cam, params, out, ptr_t):
        st = A.RtStats()
        code = fn(self._h, scene._h, C.byref(cam), C.byref(params), out.ctypes.data_as(C.POINTER(ptr_t)), C.byref(st))
        if code != A.RT_OK:
            raise RtError(code, lib().rt_last_error_multi(self._h).decode())
        return out, st.as_dict()

    def render(self, scene, cam, params):
        """rt_render_multi: full frame of f32 RGB sums on the host."""
        return self._render(lib().rt_render_multi, scene, cam, params, np.empty((params.height, params.width, 3), dtype=np.float32), C.c_float)

    def render_rgb8(self, scene, cam, params):
        """rt_render_multi_rgb8: write_color applied per shard on the devices, RGB8 gathered (3 B/pixel over xGMI)."""
        return self._render(lib().rt_render_multi_rgb8, scene, cam, params, np.empty((params.height, params.width, 3), dtype=np.uint8), C.c_uint8)

    def close(self):
        if self._h:
            lib().rt_ctx_destroy_multi(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
