"""MI355X-native path-tracing hot path — Python host bindings over the C ABI (include/rt_hip.h).

The directory name has a hyphen, so import it through ``rta.load()`` at the repo root (it registers
this package as ``ray_tracer_archive_amd``).  Importing the package never touches the GPU; creating
a ``Context`` does, and fails loudly when the HIP library or a device is missing — there is no CPU
fallback in the product path.
"""
from . import _abi  # noqa: F401
from .api import (Context, Scene, HostScene, RtError, camera_new, lib, lib_path, tonemap, write_color, write_png, write_image, untile,
                  output_floats, make_params, compile_info, compile_dump, MultiContext, MultiScene, comm_unique_id, untile_rgb8, wide_layout_check, runtime_libraries, upload_options,
                  pass_check, scene_fingerprint, adaptive_check, adaptive_options, denoise_check, denoise_options, denoise_guide, denoise_guided_check,
                  RAY_DTYPE, RAYHIT_DTYPE, LIGHTQUERY_DTYPE, LIGHTSAMPLE_DTYPE, ray_query_check, ray_query_options, feature_options, features_check,
                  denoise_guide_moments, denoise_guided_moments_check, feature_moment_buffers, feature_moments_check, camera_lists_host,
                  PATHRAY_DTYPE, radiance_options, radiance_check)  # noqa: F401
from .layout import slot_pixels  # noqa: F401
from .features import feature_means  # noqa: F401
from .radiance import path_rays, equirect_rays, standard_error  # noqa: F401
from .adaptive import Adaptive, select_reference, check_counts, check_adaptive_checkpoint  # noqa: F401
from .denoise import nlm_reference, nlm_prepare, nlm_guided_reference, guide_prepare, nlm_guided_moments_reference, guide_moments_prepare  # noqa: F401
from .progressive import Progressive, check_checkpoint, std_error  # noqa: F401
from .scene import SceneBuilder  # noqa: F401
from .scene_json import JsonScene, load_scene, parse_obj, parse_obj_attrs  # noqa: F401
from .mesh import icosphere, interpolate_reference, sphere_uv, normal_map_reference, height_to_normal_map, texel_of  # noqa: F401
from .environment import EnvMap, env_reference, env_tables, load_hdr  # noqa: F401
from .lights import light_reference, light_tree, light_weights, solid_angle_triangle  # noqa: F401
