//! gpu_ffi.rs — `extern "C"` bindings of include/rt_hip.h (ABI version 3) for the reference crate.
//!
//! Where it goes: `raytracer/src/gpu_ffi.rs`, with `mod gpu_ffi;` added to the module list of `main.rs:7-24`.
//! It replaces nothing by itself: docs/main_rs.patch swaps the pixel loops `main.rs:730-784` for one call.
//!
//! UNVERIFIED TEXT: this image has no Rust toolchain, so this file has never been compiled. What IS
//! checked (tests/test_abi.py::test_rust_shim_covers_the_header) is that every function the header declares is bound
//! here under the same name and that every `#[repr(C)]` struct lists the header's fields in the header's order.
//! Edition 2018 / rustc 1.60 (the reference's pin, rust-toolchain:1): no `c"..."` literals, no `unsafe extern`.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int, c_void};

pub const RT_ABI_VERSION: u32 = 3;

// RtStatus
pub const RT_OK: c_int = 0;
pub const RT_ERR_INVALID: c_int = -1;
pub const RT_ERR_UNSUPPORTED: c_int = -2;
pub const RT_ERR_DEVICE: c_int = -3;
pub const RT_ERR_NO_DEVICE: c_int = -4;
pub const RT_ERR_OOM: c_int = -5;
pub const RT_ERR_PEER: c_int = -6;        // a collective render was called off because another rank failed; the message names it

/// vec3.rs:5-8
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtVec3 { pub x: f64, pub y: f64, pub z: f64 }

/// camera.rs:6-18, field for field
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtCamera {
    pub origin: RtVec3, pub lower_left_corner: RtVec3, pub horizontal: RtVec3, pub vertical: RtVec3,
    pub u: RtVec3, pub v: RtVec3, pub w: RtVec3, pub lens_radius: f64, pub time0: f64, pub time1: f64,
}

// RtTextureKind (texture.rs)
pub const RT_TEX_SOLID: i32 = 0;
pub const RT_TEX_CHECKER: i32 = 1;
pub const RT_TEX_NOISE: i32 = 2;
pub const RT_TEX_IMAGE: i32 = 3;
#[repr(C)] #[derive(Clone, Copy)]
pub struct RtTexture { pub kind: i32, pub a: i32, pub b: i32, pub _pad: i32, pub color: RtVec3, pub scale: f64 }
/// perlin.rs:7-12
#[repr(C)]
pub struct RtPerlin { pub ranvec: [[f64; 3]; 256], pub perm_x: [u32; 256], pub perm_y: [u32; 256], pub perm_z: [u32; 256] }
/// texture.rs:99-104: RGB8, row-major
#[repr(C)] #[derive(Clone, Copy)]
pub struct RtImage { pub data: *const u8, pub width: u32, pub height: u32 }

// RtMaterialKind (material.rs)
pub const RT_MAT_LAMBERTIAN: i32 = 0;
pub const RT_MAT_METAL: i32 = 1;
pub const RT_MAT_DIELECTRIC: i32 = 2;
pub const RT_MAT_DIFFUSE_LIGHT: i32 = 3;
pub const RT_MAT_ISOTROPIC: i32 = 4;
#[repr(C)] #[derive(Clone, Copy)]
pub struct RtMaterial { pub kind: i32, pub texture: i32, pub albedo: RtVec3, pub fuzz: f64, pub ir: f64 }

// RtHittableKind: one record per Arc<dyn Hittable>
pub const RT_HIT_SPHERE: i32 = 0;
pub const RT_HIT_MOVING_SPHERE: i32 = 1;
pub const RT_HIT_XY_RECT: i32 = 2;
pub const RT_HIT_XZ_RECT: i32 = 3;
pub const RT_HIT_YZ_RECT: i32 = 4;
pub const RT_HIT_TRIANGLE: i32 = 5;
pub const RT_HIT_BOX: i32 = 6;
pub const RT_HIT_LIST: i32 = 7;
pub const RT_HIT_BVH: i32 = 8;
pub const RT_HIT_TRANSLATE: i32 = 9;
pub const RT_HIT_ROTATE_Y: i32 = 10;
pub const RT_HIT_FLIP_FACE: i32 = 11;
pub const RT_HIT_CONSTANT_MEDIUM: i32 = 12;
#[repr(C)] #[derive(Clone, Copy)]
pub struct RtHittable { pub kind: i32, pub material: i32, pub first_child: i32, pub n_children: i32, pub p: [f64; 10] }

pub const RT_BG_CONSTANT: i32 = 0;       // main.rs:692 `background`
pub const RT_BG_SKY_GRADIENT: i32 = 1;   // book-1 sky (not in the reference)
pub const RT_BVH_REFERENCE: i32 = 0;     // BVHNode::construct as intended (bvh.rs:77-130)
pub const RT_BVH_SAH: i32 = 1;           // binned SAH: same picture, fewer node visits

pub const RT_SCENE_LIGHTS_ALL_SHAPES: u32 = 1;   // RtSceneDesc.scene_flags: rects of any orientation, triangles, boxes and wrapped members are sampled as lights
pub const RT_SCENE_LIGHTS_MANY: u32 = 4;         // RtSceneDesc.scene_flags, with RT_SCENE_LIGHTS_ALL_SHAPES: area-weighted pick, the list's pdf through a light tree
#[repr(C)]
pub struct RtSceneDesc {
    pub abi_version: u32, pub scene_flags: u32,
    pub hittables: *const RtHittable, pub n_hittables: u64,
    pub children: *const i32, pub n_children: u64,
    pub materials: *const RtMaterial, pub n_materials: u64,
    pub textures: *const RtTexture, pub n_textures: u64,
    pub perlins: *const RtPerlin, pub n_perlins: u64,
    pub images: *const RtImage, pub n_images: u64,
    pub world: i32, pub lights: i32, pub background_mode: i32, pub bvh_builder: i32,
    pub background: RtVec3, pub bvh_seed: u64,
}

pub const RT_NAN_PER_SAMPLE: u32 = 0;
pub const RT_NAN_REFERENCE: u32 = 1;     // main.rs:146-155: the pixel SUM is scrubbed
pub const RT_FLAG_COUNTERS: u32 = 1;
pub const RT_FLAG_TIMING: u32 = 2;
pub const RT_FLAG_SAMPLE_BLOCKS: u32 = 4;
pub const RT_FLAG_FUSED: u32 = 8;         // diagnostic: the whole render by the fused per-path (tail) kernel
pub const RT_FLAG_NO_CAMERA_LISTS: u32 = 16;   // A/B: camera rays are walked like every other ray (same frame); an unknown bit is RT_ERR_INVALID
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtParams {
    pub width: u32, pub height: u32, pub samples_per_pixel: u32, pub max_depth: u32, pub seed: u64,
    pub nan_policy: u32, pub flags: u32, pub tile_size: u32, pub shard_index: u32, pub shard_count: u32, pub pool_slots: u32,
    pub tail_paths: u32, pub _pad: u32,
}

// RtUploadOptions.layout_flags: how a scene is laid out on the device (never what it looks like); 0 = the library's defaults
pub const RT_LAYOUT_LISTS_AS_REFERENCE: u32 = 1;
pub const RT_LAYOUT_LISTS_CULLED: u32 = 2;
pub const RT_LAYOUT_NO_MEMBER_BOXES: u32 = 4;
pub const RT_LAYOUT_MEMBER_BOXES: u32 = 8;
pub const RT_LAYOUT_CHILD_ORDER_AS_REFERENCE: u32 = 16;
pub const RT_LAYOUT_SCENE_IN_HBM: u32 = 32;
pub const RT_LAYOUT_NODES_32B: u32 = 64;
pub const RT_LAYOUT_NO_SHADE_TABLES_IN_LDS: u32 = 128;
pub const RT_LAYOUT_NO_EXTEND_TABLES_IN_LDS: u32 = 256;
pub const RT_LAYOUT_WIDE_NODES: u32 = 512;
pub const RT_LAYOUT_ALL_BOX_NODES: u32 = 1024;
pub const RT_LAYOUT_REFERENCE_COUNTERS: u32 = 1 | 4 | 16;   // RtStats test counts = the reference's own
// per-vertex normals / texture coordinates of RT_HIT_TRIANGLE records (RtTriangleAttrs.flags), handed over in RtUploadOptions
pub const RT_TRI_NORMALS: u32 = 1;
pub const RT_TRI_UVS: u32 = 2;
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtTriangleAttrs {
    pub hittable: i32, pub flags: u32, pub n: [[f32; 3]; 3], pub uv: [[f32; 2]; 3],
}
// an environment map: an HDR equirectangular image as background and, with RT_ENV_SAMPLED, as one more light (RtEnvMap.flags)
pub const RT_ENV_SAMPLED: u32 = 1;
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct RtEnvMap {
    pub struct_bytes: u32, pub flags: u32, pub width: u32, pub height: u32, pub rgb: *const f32, pub scale: f32, pub _pad: u32,
}
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct RtUploadOptions {
    pub struct_bytes: u32, pub layout_flags: u32, pub lds_top_records: u32, pub octant_axes: u32, pub leaf_collapse: u32, pub list_park_cost: f32,
    pub triangle_attrs: *const RtTriangleAttrs, pub n_triangle_attrs: u64,
}
// the options record grown at its end: hand `&x.base` (base.struct_bytes = size_of::<RtUploadOptionsEnv>()) to every entry point that takes options
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct RtUploadOptionsEnv {
    pub base: RtUploadOptions, pub env_map: *const RtEnvMap,
}
impl RtUploadOptionsEnv {
    pub fn new(env_map: *const RtEnvMap) -> Self {
        RtUploadOptionsEnv { base: RtUploadOptions { struct_bytes: std::mem::size_of::<RtUploadOptionsEnv>() as u32, ..Default::default() }, env_map }
    }
}
// a normal map: tangent-space shading normals on the triangles of one material (RtNormalMap.flags); the texels are an RtImage of the desc
pub const RT_NMAP_FLIP_GREEN: u32 = 1;
pub const RT_FEATURE_NORMAL_MAP: u32 = 2048;   // RtCompileInfo.features: a device triangle carries a map
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtNormalMap {
    pub material: i32, pub image: i32, pub strength: f32, pub flags: u32,
}
// ... grown once more: hand `&x.base.base` (struct_bytes = size_of::<RtUploadOptionsMaps>() = 64); `maps` must outlive the upload
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct RtUploadOptionsMaps {
    pub base: RtUploadOptionsEnv, pub normal_maps: *const RtNormalMap, pub n_normal_maps: u64,
}
impl RtUploadOptionsMaps {
    pub fn new(env_map: *const RtEnvMap, maps: &[RtNormalMap]) -> Self {
        let mut base = RtUploadOptionsEnv::new(env_map);
        base.base.struct_bytes = std::mem::size_of::<RtUploadOptionsMaps>() as u32;
        RtUploadOptionsMaps { base, normal_maps: if maps.is_empty() { std::ptr::null() } else { maps.as_ptr() }, n_normal_maps: maps.len() as u64 }
    }
}
impl Default for RtUploadOptions {
    fn default() -> Self {
        RtUploadOptions { struct_bytes: std::mem::size_of::<RtUploadOptions>() as u32, layout_flags: 0, lds_top_records: 0, octant_axes: 0, leaf_collapse: 0,
                          list_park_cost: 0.0, triangle_attrs: std::ptr::null(), n_triangle_attrs: 0 }
    }
}

// progressive rendering: a frame in resumable sample passes (rt_render_pass); RtPassOptions.flags
pub const RT_PASS_ACCUMULATE: u32 = 1;    // add into the output buffer(s), folding on from the value already there
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtPassOptions {
    pub struct_bytes: u32, pub flags: u32, pub first_sample: u32, pub frame_samples: u32,
}
// adaptive sampling: passes over the pixels whose standard error is still above the tolerance (rt_adaptive_select)
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtAdaptiveOptions {
    pub struct_bytes: u32, pub min_samples: u32, pub rel_error: f64, pub abs_error: f64,
}
// denoising: non-local means over the sample variance (rt_denoise_device); a field left 0 takes its default
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtDenoiseOptions {
    pub struct_bytes: u32, pub window_radius: u32, pub patch_radius: u32, pub samples_per_item: u32,
    pub strength: f64, pub alpha: f64, pub eps: f64,
}
// guided denoising (rt_denoise_guided_device): full-frame feature planes of rt_render_features_device; a sigma left 0 takes its default
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct RtDenoiseGuide {
    pub struct_bytes: u32, pub feature_samples: u32,
    pub albedo_sum: *const c_void, pub normal_sum: *const c_void, pub depth_sum: *const c_void, pub hits: *const c_void,
    pub sigma_albedo: f64, pub sigma_normal: f64, pub sigma_depth: f64,
}
pub const RT_DENOISE_GUIDED_MAX_WINDOW_RADIUS: u32 = 10;
// guided denoising with feature variances (rt_denoise_guided_moments_device): the planes of rt_render_feature_moments_device; 0 = default
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct RtDenoiseGuideMoments {
    pub struct_bytes: u32, pub feature_samples: u32,
    pub albedo_sum: *const c_void, pub normal_sum: *const c_void, pub depth_sum: *const c_void, pub hits: *const c_void,
    pub albedo_sq_sum: *const c_void, pub normal_sq_sum: *const c_void, pub depth_sq_sum: *const c_void,
    pub sigma_albedo: f64, pub sigma_normal: f64, pub sigma_depth: f64, pub variance_strength: f64,
}
pub const RT_DENOISE_GUIDED_MOMENTS_MAX_WINDOW_RADIUS: u32 = 8;
// ray queries: the closest hit of caller-supplied rays (rt_trace_rays); t_max <= 0 or +inf = no limit
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtRay { pub o: [f32; 3], pub time: f32, pub d: [f32; 3], pub t_max: f32 }
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtRayHit {
    pub t: f32, pub hittable: i32, pub material: i32, pub flags: u32,
    pub p: [f32; 3], pub u: f32, pub n: [f32; 3], pub v: f32,
}
pub const RT_RAYHIT_HIT: u32 = 1; pub const RT_RAYHIT_FRONT_FACE: u32 = 2; pub const RT_RAYHIT_INVALID_RAY: u32 = 4;
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtRayQueryOptions { pub struct_bytes: u32, pub flags: u32, pub pool_slots: u32, pub _pad: u32 }
// first-hit features (rt_render_features_device): per-slot sums of albedo, normal, depth and the hit count of the render's own camera rays
pub const RT_FEATURES_ACCUMULATE: u32 = 1;
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtFeatureOptions { pub struct_bytes: u32, pub flags: u32, pub first_sample: u32, pub pool_slots: u32 }
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct RtFeatureBuffers { pub albedo_sum: *mut c_void, pub normal_sum: *mut c_void, pub depth_sum: *mut c_void, pub hits: *mut c_void }
// the same pass with the per-slot sums of squares beside the sums (rt_render_feature_moments_device)
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct RtFeatureMomentBuffers {
    pub struct_bytes: u32, pub _pad: u32,
    pub albedo_sum: *mut c_void, pub normal_sum: *mut c_void, pub depth_sum: *mut c_void, pub hits: *mut c_void,
    pub albedo_sq_sum: *mut c_void, pub normal_sq_sum: *mut c_void, pub depth_sq_sum: *mut c_void,
}
pub const RT_DENOISE_MAX_WINDOW_RADIUS: u32 = 16;
pub const RT_DENOISE_MAX_PATCH_RADIUS: u32 = 4;

pub const RT_N_PRIM_TYPES: usize = 6;
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtStats {
    pub render_ms: f64, pub extend_ms: f64, pub shade_ms: f64, pub other_ms: f64,
    pub samples: u64, pub segments: u64, pub node_tests: u64, pub prim_tests: [u64; RT_N_PRIM_TYPES],
    pub iterations: u32, pub extend_launches: u32, pub shade_launches: u32, pub pool_slots: u32,
    pub scene_nodes: u64, pub scene_prims: u64, pub scene_bytes: u64, pub bvh_in_lds: u32, pub _pad: u32, pub debug: [u64; 8],
    pub gather_ms: f64, pub n_devices: u32, pub lds_top_nodes: u32, pub drain_ms: f64, pub drain_paths: u32, pub _pad2: u32,
}

#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtWideInfo {
    pub n_nodes: u64, pub n_leaf_entries: u64, pub n_inner_entries: u64, pub n_prims: u64, pub depth: u32, pub _pad: u32,
    pub mean_children: f64, pub mean_leaf_members: f64,
}

#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtCompileInfo {
    pub n_nodes: u64, pub n_box_nodes: u64, pub n_spheres: u64, pub n_moving: u64, pub n_rects: u64, pub n_tris: u64,
    pub n_media: u64, pub n_xforms: u64, pub n_lights: u64, pub n_materials: u64, pub features: u32, pub fits_lds: u32,
    pub n_first: u32, pub first: [u32; 4], pub n_tri_attrs: u32,
}

pub const RT_LIGHTQ_DIRECTION_GIVEN: u32 = 1;    // RtLightQuery.flags: evaluate the pdf of the caller's d, draw nothing
pub const RT_LIGHTQ_LINEAR: u32 = 2;             // RtLightQuery.flags: a scene with a light tree evaluates the pdf by the plain loop over its table
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtLightQuery { pub p: [f32; 3], pub flags: u32, pub rng_state: u64, pub d: [f32; 3], pub _pad: f32 }       // 40 B
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtLightSample { pub d: [f32; 3], pub pdf: f32, pub light: i32, pub n_draws: u32 }                           // 24 B
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtLightQueryOptions { pub struct_bytes: u32, pub flags: u32 }
// radiance queries (rt_radiance_rays): the path tracer on caller-supplied rays, per-ray sums over a sample range
pub const RT_RADIANCE_ACCUMULATE: u32 = 1;
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtPathRay { pub o: [f32; 3], pub time: f32, pub d: [f32; 3], pub first_draw: u32 }                           // 32 B
#[repr(C)] #[derive(Clone, Copy, Default, Debug)]
pub struct RtRadianceOptions {
    pub struct_bytes: u32, pub flags: u32, pub render_flags: u32, pub nan_policy: u32,
    pub samples: u32, pub first_sample: u32, pub max_depth: u32, pub pool_slots: u32,
    pub seed: u64, pub first_stream: u64, pub tail_paths: u32, pub _pad: u32,
}

pub const RT_OUT_RGB_SUM_F32: u32 = 0;
pub const RT_OUT_RGB8: u32 = 1;
pub const RT_COMM_ID_BYTES: usize = 128;

#[repr(C)] pub struct RtCtx { _p: [u8; 0] }
#[repr(C)] pub struct RtScene { _p: [u8; 0] }
#[repr(C)] pub struct RtMultiCtx { _p: [u8; 0] }
#[repr(C)] pub struct RtMultiScene { _p: [u8; 0] }

#[link(name = "rt_hip")]
extern "C" {
    pub fn rt_abi_version() -> u32;
    pub fn rt_last_error(ctx: *const RtCtx) -> *const c_char;

    // ---- one GPU ----
    pub fn rt_ctx_create(device_id: c_int, stream: *mut c_void, out_ctx: *mut *mut RtCtx) -> c_int;
    pub fn rt_ctx_destroy(ctx: *mut RtCtx) -> c_int;
    pub fn rt_scene_upload(ctx: *mut RtCtx, desc: *const RtSceneDesc, out_scene: *mut *mut RtScene) -> c_int;
    /// the same with the device layout chosen per upload (NULL options = defaults); a threaded host cannot use process environment for that
    pub fn rt_scene_upload_ex(ctx: *mut RtCtx, desc: *const RtSceneDesc, options: *const RtUploadOptions, out_scene: *mut *mut RtScene) -> c_int;
    pub fn rt_scene_destroy(ctx: *mut RtCtx, scene: *mut RtScene) -> c_int;
    pub fn rt_output_floats(params: *const RtParams, out_n: *mut u64) -> c_int;
    /// replaces the body of the pixel loops main.rs:731-784 (without write_color)
    pub fn rt_render(ctx: *mut RtCtx, scene: *const RtScene, cam: *const RtCamera, params: *const RtParams,
                     rgb_sum_host: *mut f32, stats: *mut RtStats) -> c_int;
    pub fn rt_render_device(ctx: *mut RtCtx, scene: *const RtScene, cam: *const RtCamera, params: *const RtParams,
                            rgb_sum_device: *mut c_void, stats: *mut RtStats) -> c_int;
    /// host only: validates a pass and reports the samples per work item of the frame
    pub fn rt_pass_check(params: *const RtParams, options: *const RtPassOptions, out_samples_per_item: *mut u32) -> c_int;
    /// samples first_sample .. first_sample + spp - 1; sq_sum_host may be null
    pub fn rt_render_pass(ctx: *mut RtCtx, scene: *const RtScene, cam: *const RtCamera, params: *const RtParams, options: *const RtPassOptions,
                          rgb_sum_host: *mut f32, sq_sum_host: *mut f32, stats: *mut RtStats) -> c_int;
    pub fn rt_render_pass_device(ctx: *mut RtCtx, scene: *const RtScene, cam: *const RtCamera, params: *const RtParams, options: *const RtPassOptions,
                                 rgb_sum_device: *mut c_void, sq_sum_device: *mut c_void, stats: *mut RtStats) -> c_int;
    /// host only: validates adaptive options for a frame (min_samples >= 2 work items, tolerances finite and >= 0, first_sample on an item boundary)
    pub fn rt_adaptive_check(params: *const RtParams, options: *const RtAdaptiveOptions, first_sample: u32, frame_samples: u32) -> c_int;
    /// the active list: ascending output slots with counts == first_sample that are below min_samples or not converged; *n_out entries
    pub fn rt_adaptive_select(ctx: *mut RtCtx, params: *const RtParams, options: *const RtAdaptiveOptions, first_sample: u32, frame_samples: u32,
                              rgb_sum_device: *const c_void, sq_sum_device: *const c_void, counts_device: *const c_void, pixels_device_out: *mut c_void,
                              n_out: *mut u32) -> c_int;
    /// samples first_sample .. first_sample + spp - 1 of the listed slots only; counts[slot] = first_sample + spp; sq_sum_device may be null
    pub fn rt_render_pass_pixels_device(ctx: *mut RtCtx, scene: *const RtScene, cam: *const RtCamera, params: *const RtParams, options: *const RtPassOptions,
                                        pixels_device: *const c_void, n_pixels: u32, rgb_sum_device: *mut c_void, sq_sum_device: *mut c_void,
                                        counts_device: *mut c_void, stats: *mut RtStats) -> c_int;
    /// write_color with each pixel's own count (full frame); a count of 0 gives black
    pub fn rt_resolve_counts_device(ctx: *mut RtCtx, rgb_sum_device: *const c_void, counts_device: *const c_void, width: u32, height: u32,
                                    rgb8_device: *mut c_void) -> c_int;
    /// host only: validates a frame size and denoise options (null = defaults)
    pub fn rt_denoise_check(width: u32, height: u32, options: *const RtDenoiseOptions) -> c_int;
    /// filtered MEAN radiance (width * height * 3 f32) from rgb_sum, sq_sum and the sample count; counts_device null = uniform `samples`
    pub fn rt_denoise_device(ctx: *mut RtCtx, options: *const RtDenoiseOptions, width: u32, height: u32, rgb_sum_device: *const c_void,
                             sq_sum_device: *const c_void, samples: u32, counts_device: *const c_void, mean_out_device: *mut c_void) -> c_int;
    /// host only: validates a frame size, denoise options (null = defaults; window_radius <= 10 here) and a guide
    pub fn rt_denoise_guided_check(width: u32, height: u32, options: *const RtDenoiseOptions, guide: *const RtDenoiseGuide) -> c_int;
    /// rt_denoise_device with the weights joined with albedo, normal and log depth of the first hit (binary16 guide records)
    pub fn rt_denoise_guided_device(ctx: *mut RtCtx, options: *const RtDenoiseOptions, guide: *const RtDenoiseGuide, width: u32, height: u32,
                                    rgb_sum_device: *const c_void, sq_sum_device: *const c_void, samples: u32, counts_device: *const c_void,
                                    mean_out_device: *mut c_void) -> c_int;
    /// host only: validates the options and the guide of the variance-guided filter (window_radius 0 = 8, at most 8; feature_samples >= 2)
    pub fn rt_denoise_guided_moments_check(width: u32, height: u32, options: *const RtDenoiseOptions, guide: *const RtDenoiseGuideMoments) -> c_int;
    /// rt_denoise_guided_device with the feature distance variance-cancelled and variance-normalised from the features' second moments
    pub fn rt_denoise_guided_moments_device(ctx: *mut RtCtx, options: *const RtDenoiseOptions, guide: *const RtDenoiseGuideMoments, width: u32, height: u32,
                                            rgb_sum_device: *const c_void, sq_sum_device: *const c_void, samples: u32, counts_device: *const c_void,
                                            mean_out_device: *mut c_void) -> c_int;
    /// host only: validates ray-query options (null = defaults) and a ray count
    pub fn rt_ray_query_check(options: *const RtRayQueryOptions, n_rays: u64) -> c_int;
    /// closest hits of n_rays RtRay records in device memory, one RtRayHit each (device memory, 16-byte aligned)
    pub fn rt_trace_rays_device(ctx: *mut RtCtx, scene: *const RtScene, options: *const RtRayQueryOptions, rays_device: *const c_void, n_rays: u64,
                                hits_device: *mut c_void, stats: *mut RtStats) -> c_int;
    pub fn rt_trace_rays(ctx: *mut RtCtx, scene: *const RtScene, options: *const RtRayQueryOptions, rays_host: *const RtRay, n_rays: u64,
                         hits_host: *mut RtRayHit, stats: *mut RtStats) -> c_int;
    /// occlusion: one byte per ray (RT_RAYHIT_HIT when anything is hit in [0.001, t_max], RT_RAYHIT_INVALID_RAY for a ray never traced)
    pub fn rt_occluded_rays_device(ctx: *mut RtCtx, scene: *const RtScene, options: *const RtRayQueryOptions, rays_device: *const c_void, n_rays: u64,
                                   occluded_device: *mut c_void, stats: *mut RtStats) -> c_int;
    pub fn rt_occluded_rays(ctx: *mut RtCtx, scene: *const RtScene, options: *const RtRayQueryOptions, rays_host: *const RtRay, n_rays: u64,
                            occluded_host: *mut u8, stats: *mut RtStats) -> c_int;
    /// the scene's own light sampler: one RtLightSample per RtLightQuery (device memory, 8-byte aligned); lights = -1 is RT_ERR_UNSUPPORTED
    pub fn rt_sample_lights_device(ctx: *mut RtCtx, scene: *const RtScene, options: *const RtLightQueryOptions, queries_device: *const c_void, n: u64,
                                   results_device: *mut c_void, stats: *mut RtStats) -> c_int;
    pub fn rt_sample_lights(ctx: *mut RtCtx, scene: *const RtScene, options: *const RtLightQueryOptions, queries_host: *const RtLightQuery, n: u64,
                            results_host: *mut RtLightSample, stats: *mut RtStats) -> c_int;
    /// host only: validates (options, n_rays) of a radiance query
    pub fn rt_radiance_check(options: *const RtRadianceOptions, n_rays: u64) -> c_int;
    /// radiance along n_rays RtPathRay records: per-ray RGB sums over the samples (3 f32 each), optional sums of squares and flag bytes
    pub fn rt_radiance_rays_device(ctx: *mut RtCtx, scene: *const RtScene, options: *const RtRadianceOptions, rays_device: *const c_void, n_rays: u64,
                                   rgb_sum_device: *mut c_void, sq_sum_device: *mut c_void, invalid_device: *mut c_void, stats: *mut RtStats) -> c_int;
    pub fn rt_radiance_rays(ctx: *mut RtCtx, scene: *const RtScene, options: *const RtRadianceOptions, rays_host: *const RtPathRay, n_rays: u64,
                            rgb_sum_host: *mut f32, sq_sum_host: *mut f32, invalid_host: *mut u8, stats: *mut RtStats) -> c_int;
    /// host only: validates a feature pass (params, options)
    pub fn rt_features_check(params: *const RtParams, options: *const RtFeatureOptions) -> c_int;
    /// first-hit feature sums of samples [first_sample, first_sample + samples_per_pixel) into the caller's device planes (null = not wanted)
    pub fn rt_render_features_device(ctx: *mut RtCtx, scene: *const RtScene, cam: *const RtCamera, params: *const RtParams,
                                     options: *const RtFeatureOptions, buffers: *const RtFeatureBuffers, stats: *mut RtStats) -> c_int;
    /// host only: validates a feature pass with second moments (params, options, the buffers' struct_bytes)
    pub fn rt_feature_moments_check(params: *const RtParams, options: *const RtFeatureOptions, buffers: *const RtFeatureMomentBuffers) -> c_int;
    /// rt_render_features_device plus the per-slot sums of squares of albedo, normal and depth
    pub fn rt_render_feature_moments_device(ctx: *mut RtCtx, scene: *const RtScene, cam: *const RtCamera, params: *const RtParams,
                                            options: *const RtFeatureOptions, buffers: *const RtFeatureMomentBuffers, stats: *mut RtStats) -> c_int;
    pub fn rt_untile(params: *const RtParams, gathered: *const f32, rgb_sum: *mut f32) -> c_int;
    /// write_color (main.rs:141-169) on the device
    pub fn rt_resolve_device(ctx: *mut RtCtx, rgb_sum_device: *const c_void, width: u32, height: u32,
                             samples_per_pixel: u32, rgb8_device: *mut c_void) -> c_int;

    // ---- all GPUs of the node from this one process: what main.rs binds (docs/main_rs.patch) ----
    pub fn rt_ctx_create_multi(device_ids: *const c_int, n_devices: c_int, out_ctx: *mut *mut RtMultiCtx) -> c_int;
    pub fn rt_ctx_destroy_multi(ctx: *mut RtMultiCtx) -> c_int;
    pub fn rt_scene_upload_multi(ctx: *mut RtMultiCtx, desc: *const RtSceneDesc, out_scene: *mut *mut RtMultiScene) -> c_int;
    pub fn rt_scene_upload_multi_ex(ctx: *mut RtMultiCtx, desc: *const RtSceneDesc, options: *const RtUploadOptions,
                                    out_scene: *mut *mut RtMultiScene) -> c_int;
    pub fn rt_scene_destroy_multi(ctx: *mut RtMultiCtx, scene: *mut RtMultiScene) -> c_int;
    pub fn rt_render_multi(ctx: *mut RtMultiCtx, scene: *const RtMultiScene, cam: *const RtCamera, params: *const RtParams,
                           rgb_sum_host: *mut f32, stats: *mut RtStats) -> c_int;
    /// write_color applied on the devices: the bytes main.rs:781 stores, 3 B/pixel over xGMI
    pub fn rt_render_multi_rgb8(ctx: *mut RtMultiCtx, scene: *const RtMultiScene, cam: *const RtCamera, params: *const RtParams,
                                rgb8_host: *mut u8, stats: *mut RtStats) -> c_int;
    pub fn rt_last_error_multi(ctx: *const RtMultiCtx) -> *const c_char;

    // ---- one process per GPU (MPI / torchrun style launchers) ----
    pub fn rt_comm_unique_id(id_out: *mut u8) -> c_int;
    pub fn rt_comm_init_rank(ctx: *mut RtCtx, id: *const u8, rank: c_int, world: c_int) -> c_int;
    pub fn rt_comm_selftest(ctx: *mut RtCtx) -> c_int;
    pub fn rt_render_gather(ctx: *mut RtCtx, scene: *const RtScene, cam: *const RtCamera, params: *const RtParams,
                            output_kind: u32, frame_device: *mut c_void, stats: *mut RtStats) -> c_int;
    pub fn rt_untile_device(ctx: *mut RtCtx, params: *const RtParams, output_kind: u32, gathered_device: *const c_void,
                            frame_device: *mut c_void) -> c_int;
    pub fn rt_untile_rgb8(params: *const RtParams, gathered: *const u8, rgb8: *mut u8) -> c_int;

    // ---- the process's ROCm runtime libraries (refuses two HIP runtimes in one process); fault injection for failure-path tests ----
    pub fn rt_runtime_libraries(out: *mut c_char, cap: u64) -> c_int;
    pub fn rt_test_fail_next_renders(ctx: *mut RtCtx, n: u32) -> c_int;
    pub fn rt_test_device_workers(n_workers: c_int, rounds: c_int) -> c_int;

    // ---- scene-compiler introspection (host only) ----
    pub fn rt_scene_compile_info(desc: *const RtSceneDesc, out: *mut RtCompileInfo) -> c_int;
    pub fn rt_scene_compile_info_ex(desc: *const RtSceneDesc, options: *const RtUploadOptions, out: *mut RtCompileInfo) -> c_int;
    pub fn rt_scene_compile_dump_ex(desc: *const RtSceneDesc, options: *const RtUploadOptions, nodes: *mut c_void, cap_nodes: u64,
                                    spheres: *mut f32, sphere_meta: *mut u32, cap_spheres: u64) -> c_int;
    /// host only: the light tree of an RT_SCENE_LIGHTS_MANY scene (32-byte records), slot -> member, p and cdf by member; any output may be null
    pub fn rt_env_tables(env_map: *const RtEnvMap, marg: *mut f32, cond: *mut f32) -> c_int;
    pub fn rt_scene_light_tree_dump(desc: *const RtSceneDesc, nodes: *mut c_void, cap_nodes: u64, slot_member: *mut u32, p: *mut f32, cdf: *mut f32,
                                    cap_lights: u64, out_n_lights: *mut u64, out_n_nodes: *mut u64) -> c_int;
    pub fn rt_scene_wide_layout_check(desc: *const RtSceneDesc, out: *mut RtWideInfo) -> c_int;
    pub fn rt_scene_top_layout_check(desc: *const RtSceneDesc, max_top: u32, out_n_top: *mut u64) -> c_int;
    pub fn rt_scene_compile_dump(desc: *const RtSceneDesc, nodes: *mut c_void, cap_nodes: u64, spheres: *mut f32,
                                 sphere_meta: *mut u32, cap_spheres: u64) -> c_int;
    /// camera lists: 17 words per 8 x 8-pixel square (count or 0xFFFFFFFF = "walk", then sphere indices in leaf order); lists may be null
    /// host only: the lists of a scene compiled with the default options; *out_n_squares = 0: the lists do not serve this scene or camera
    pub fn rt_camera_lists_host(desc: *const RtSceneDesc, cam: *const RtCamera, width: u32, height: u32, lists: *mut u32, cap_words: u64,
                                out_n_squares: *mut u64) -> c_int;
    /// the lists the last render or pass of this context built on the device; *out_n_squares = 0: it built none
    pub fn rt_camera_lists_last(ctx: *mut RtCtx, lists: *mut u32, cap_words: u64, out_n_squares: *mut u64) -> c_int;
}

/// The reference's error convention is panic (main.rs:656,762,777,779): a negative status becomes one, with the library's message.
pub unsafe fn check_multi(code: c_int, ctx: *const RtMultiCtx) {
    if code != RT_OK {
        let msg = std::ffi::CStr::from_ptr(rt_last_error_multi(ctx)).to_string_lossy().into_owned();
        panic!("rt_hip error {}: {}", code, msg);
    }
}

impl From<crate::vec3::Vec3> for RtVec3 {
    fn from(v: crate::vec3::Vec3) -> Self { RtVec3 { x: v.x(), y: v.y(), z: v.z() } }
}
