// kernels.h — kernel argument blocks and launch entry points (kernels.hip <-> rt_api.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "camera_lists.h"
#include "device_types.h"

namespace rtk {

// features a scene needs beyond "static spheres + Lambertian/Metal/Dielectric + BVH"
enum : uint32_t {
    F_MOVING = 1u, F_RECT = 2u, F_TRI = 4u, F_MEDIUM = 8u, F_XFORM = 16u, F_TEX = 32u, F_LIGHTS = 64u,
    F_ALL = 127u,
    // a triangle carries per-vertex normals / texture coordinates (rt_hip.h RtTriangleAttrs). Not part of F_ALL and never seen by the plain walk:
    // only the kernels that rebuild a HitRecord have instances with it (kernels.hip with_shade_variant), every other instance is the one
    // the same scene without attributes runs. The table is found from SceneDev::tris (kernels.hip TriAttr), not through a field of its own.
    F_TRI_ATTR = 128u,
    // the lights table holds rtd::LightX records (device_types.h): RT_SCENE_LIGHTS_ALL_SHAPES and a member that is not a bare XzRect or Sphere.
    // Not part of F_ALL either: only k_shade and the drain / fused form of k_extend have instances with it, and only for the full variant.
    F_LIGHTS_EXT = 256u,
    // RT_SCENE_LIGHTS_MANY: the lights table also holds the light tree, the cdf of the area-weighted pick and the member -> slot table
    // (device_types.h); always together with F_LIGHTS_EXT. The same kernels have instances with it, and k_sample_lights one.
    F_LIGHTS_TREE = 512u,
    // the upload carried an environment map (rt_hip.h RtEnvMap): a miss returns the map's radiance, and under RT_ENV_SAMPLED the map is one more
    // member of the lights list. Not part of F_ALL; always with F_LIGHTS_EXT and never with F_LIGHTS_TREE: k_shade and the drain / fused form of
    // k_extend have two instances with it (the full variant, without and with F_TRI_ATTR), k_sample_lights one. A scene without a map runs
    // the instances it ran before the bit existed.
    F_ENV = 1024u,
    // a device triangle carries a normal map (rt_hip.h RtNormalMap). Not part of F_ALL; always with F_TRI_ATTR and F_TEX (the map is a texture record):
    // every full-variant instance with F_TRI_ATTR has a twin with it (kernels.hip with_attr_variant), which applies the map on the map bit of the
    // triangle's attribute record (kernels.hip normal_map_apply). A scene without a map runs the instances it ran before the bit existed.
    F_NORMAL_MAP = 2048u
};
#define RT_N_PRIM_TYPES_K 6
enum : uint32_t { CTR_NODE_TESTS = 0, CTR_PRIM_TESTS = 1, CTR_SAMPLES = 7, CTR_DEBUG = 8, CTR_SEGMENTS = 13, CTR_ITERATIONS = 14, CTR_COUNT = 16 };
#define RT_BG_SKY_GRADIENT_K 1
#define RT_NAN_PER_SAMPLE_K 0u

struct SceneDev {
    const rtd::Float4* nodes; uint32_t n_nodes;
    const rtd::Float4* top_nodes; uint32_t n_top;   // top of the tree staged in LDS when the scene does not fit (0: none)
    uint32_t n_records;      // records of `nodes` in all: n_nodes + DONE + IDLE + one park twin per leaf (device_types.h)
    uint32_t walk_start;     // address of the record a walk begins at: the root (0), or the park twin of the leaf every walk tests first (spheres as large as
    uint32_t first_leaf;     // the scene, scene_compile.cpp emit_bvh) — its leaf word, which M_C16 walks start with instead (they park by leaf word)
    uint32_t rec_unit, rec_b; // 32-byte records: address step from one record to the next, and from a record's first 16 bytes to its second: 32 and 16
                              // (an LDS-resident scene can be laid out otherwise for experiments: rt_api.cpp device_nodes)
    uint32_t nodes16;        // 1: `nodes` holds 16-byte compressed records (device_types.h Node16), corners on the grid below
    float grid_lo[3], grid_scale[3];
    uint32_t oct_mask;       // direction signs that select an array (x = 1, y = 2, z = 4)
    uint32_t oct_stride;     // M_C16: bytes between the record arrays of two direction octants (rt_api.cpp octant_order); 0 = one array
    uint32_t sort_rays;      // 1: k_shade orders the survivors of a workgroup by (octant, origin cell) before it writes them (scenes walked from HBM)
    const uint4* wide; uint32_t n_wide;   // 8-wide nodes (device_types.h), nullptr: the scene is walked through its binary records
    uint32_t n_prologue, prologue[rtd::MAX_PROLOGUE];   // moving spheres / media every ray meets: tested when a walk begins
    uint32_t n_prim_kinds;   // how many of {sphere, moving sphere, rect, triangle, medium} the scene holds
    const rtd::Float4* spheres; const uint32_t* sphere_meta; uint32_t n_spheres;
    const rtd::Float4* sphere_mat_a; const uint32_t* sphere_mat_b;   // small scenes: every sphere's material record beside it (mat_a/mat_b by sphere index), so
                                                                     // that k_shade asks for it together with the sphere instead of after its meta word; else nullptr
    const rtd::Float4* moving; const uint32_t* moving_meta;
    const rtd::Float4* rects; const uint32_t* rect_meta;
    const rtd::Float4* tris; const uint32_t* tri_meta;
    const rtd::Float4* boxes;   // 2 x Float4 per Box (device_types.h); in LDS behind the records when eb_boxes_on
    const rtd::Medium* media;
    const rtd::Xform* xforms;
    const rtd::Wrap* wraps;
    const rtd::Float4* mat_a; const uint32_t* mat_b;
    const rtd::Texture* textures;
    const rtd::PerlinTable* perlins;
    const rtd::Image* images; const uint8_t* image_bytes;
    const rtd::Light* lights; uint32_t n_lights;
    // k_shade's small tables as ONE blob (spheres, sphere meta, rects, rect meta, moving, moving meta, materials, transforms, wrapper
    // chains, lights, textures; every part 16-byte aligned), staged into LDS by each k_shade workgroup when it fits: the chain of
    // dependent look-ups hit -> meta -> wrap -> transform -> primitive -> material -> lights then runs at LDS, not L2, latency.
    const rtd::Float4* shade_blob; uint32_t shade_blob_bytes;   // 0: no staging
    // the same for k_extend's primitive pass on LDS-resident scenes: rects, moving spheres, transforms, media behind the records and the
    // sphere data (book-3 Cornell tests its 12 rects on every segment)
    const rtd::Float4* ext_blob; uint32_t ext_blob_bytes; uint32_t eb_rects, eb_moving, eb_xforms, eb_media, eb_boxes;
    uint32_t eb_rect_stride;   // 32: the rect table as it is (sc.rects is redirected too); 24: without the two padding words, where only that fits;
                               // 0: the rect table is not staged (a scene whose rects are mostly box sides: the boxes are staged, a lone rect reads HBM)
    uint32_t sb_perlin_only;   // 1: the blob holds the Perlin tables alone (a scene whose other tables are too big to stage: book-2 final)
    uint32_t sb_spheres, sb_sphere_meta, sb_rects, sb_rect_meta, sb_moving, sb_moving_meta, sb_mat_a, sb_mat_b, sb_xforms, sb_wraps, sb_lights, sb_textures;   // byte offsets
    // the environment map (rt_hip.h RtEnvMap; nullptr: none): env_w x env_h texels, row 0 = up, as (r, g, b, 0) so that one 128-bit load serves a
    // look-up; the marginal cdf over the rows [env_h] and the conditional cdfs within the rows [env_h * env_w] (always built; read only by the
    // instances with F_ENV when env_sampled is set); env_scale multiplies every texel. Always in HBM: a map is no small table.
    const rtd::Float4* env_texels; const float* env_marg; const float* env_cond;
    uint32_t env_w, env_h; float env_scale; uint32_t env_sampled;
};

// Path pool: structure of arrays, one lane-contiguous record per array and slot.
//   ray_o = (origin.xyz, time)   ray_d = (direction.xyz, primitive the ray starts on)   hit = (t, primitive id), written by k_extend
//   s0 = (T.rgb, work item)      sd = draws so far << 8 | depth                          s1 = (acc.rgb, sample)  multi-sample items only
// 52 bytes per path (+ 8 for the hit): T = throughput of the sample in flight, acc = sum over the finished samples of the current work
// item. The radiance of the sample in flight needs no slot (kernels.hip PathState); the pixel is decoded from the work item, and so is
// the RNG state: a path's stream is a pure function of (seed, pixel, sample), so its base is recomputed from the work item and only
// the NUMBER of draws made so far travels (round 2 carried the 64-bit counter itself: 60 bytes).
// The pool is kQueues independent queues of queue_cap slots each (slot s of queue q = record q * queue_cap + s): paths stay in
// their queue for life, every counter (pool size, queue head, next work item) exists once per queue, kQStride u32 = 128 bytes apart.
// One counter pair for the whole pool made k_shade wait on same-address atomics (one per 512 paths, ~11 ns each: 29 ms of 39).
#ifndef RT_QUEUES
#define RT_QUEUES 8       // tuning builds: 16, 32, 64 (more counters for k_shade's atomics, fewer waves per queue in k_extend: 32 cost k_extend 4 ms of 52)
#endif
constexpr uint32_t kQueues = RT_QUEUES, kQStride = 32;
constexpr uint32_t kQShift = kQueues == 8 ? 3u : kQueues == 16 ? 4u : kQueues == 32 ? 5u : kQueues == 64 ? 6u : 0u;
static_assert(kQShift != 0u && (1u << kQShift) == kQueues, "kQueues: 8, 16, 32 or 64");
struct PoolDev {
    rtd::Float4* ray_o; rtd::Float4* ray_d; uint2* hit;
    rtd::Float4* s0; uint32_t* sd; rtd::Float4* s1;
};

// Exact u32 division by a launch-invariant divisor: q = (t + ((n - t) >> s1)) >> s2 with t = umulhi(m, n)
// (Granlund-Montgomery round-up; five instructions instead of the ~35 of a hardware-less u32 divide).
struct FastDiv { uint32_t m, s1, s2, d; };
inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f{0u, 0u, 0u, d};
    if (d <= 1u) return f;                       // n / 1: t = 0, q = n
    uint32_t l = 0; while ((1ull << l) < d) ++l; // ceil(log2 d), 1..32
    f.m = (uint32_t)((((1ull << l) - d) << 32) / d + 1ull);
    f.s1 = 1u; f.s2 = l - 1u;
    return f;
}

struct RenderDev {
    // camera.rs:6-18 in f32
    float cam_origin[3], cam_llc[3], cam_horizontal[3], cam_vertical[3], cam_u[3], cam_v[3];
    float cam_lens_radius, cam_time0, cam_time1;
    uint32_t width, height, spp, max_depth;
    uint64_t seed;
    uint32_t nan_policy;
    int32_t bg_mode; float bg[3];
    // framebuffer tiling / work decomposition
    uint32_t tile_size, tiles_x, tiles_y, shard_index, shard_count;
    uint32_t block_shift;   // a work item covers 1 << block_shift consecutive samples of one pixel
    uint32_t n_blocks;      // work items per pixel = ceil(spp >> block_shift)
    uint32_t total_items;   // in-image pixels of this shard * n_blocks
    uint32_t n_init;        // work items 0 .. n_init-1 are the pool's first fill
    uint32_t lineage;       // the path that finishes work item w goes on with item w + lineage (< total_items): every slot of the first fill owns the
                            // items of its residue class, so a finished path finds its next item without asking anybody (no atomic, no barrier)
    uint32_t queue_cap;     // slots per queue
    uint32_t q_lo, q_n, q_shift;   // this launch serves queues q_lo .. q_lo + q_n - 1 (q_n = 1 << q_shift); the host always sets
                                   // 0 / kQueues / kQShift: every launch serves the whole pool (rt_api.cpp render_impl)
    uint32_t n_local_tiles;
    const uint32_t* tile_prefix;  // [n_local_tiles + 1]: in-image pixels in local tiles before lt
    uint32_t tile_slack;          // the tile of pixel q is within [q / ts^2, q / ts^2 + tile_slack] (edge tiles are clipped)
    FastDiv div_ts2, div_tiles_x, div_sq_row, div_item_tile;   // ts^2, tiles_x, ts / 8, ts^2 * n_blocks
    FastDiv div_nblocks, div_width, div_ts, div_shards;        // n_blocks, width, tile_size, shard_count: a path's item id <-> pixel <-> its slot in blocksum
    // The sphere every walk tests first (SceneDev::walk_start), tested where the ray is MADE — k_generate, k_shade: full waves — instead of
    // in the walk's first primitive pass (a third of a wave's lanes): the ray record's time slot then carries that hit's t (or inf) to k_extend.
    // Only in scenes without motion (the time is used by nothing), with ONE such sphere, and not while counting.
    uint32_t first_in_shade, first_id; float first_prim[8];      // centre + radius, or a rect's two records (a0 a1 b0 b1 | k axis)
    uint32_t tiles_all_full;      // every tile of this shard lies inside the image (4096 x 4096 in 32 x 32 tiles, any shard count): tile = item / (ts^2 * n_blocks), no table
    uint32_t row_items;           // unsharded renders: work items of one full-height row of tiles (tile_size * width * n_blocks), 0 = not used. Every
    FastDiv div_row_items;        // such row holds the same number, clipped edge tile or not, so item -> tile is arithmetic (no search in tile_prefix)
    rtd::Float4* blocksum;  // [total_items]: RGB sum of one work item's samples
    // a pass of a progressive render (rt_render_pass): samples first_sample .. spp - 1 of every pixel (spp is the pass's END, an absolute
    // index; n_blocks counts the pass's items). Every sample index that keys the RNG is absolute. rt_render: first_sample 0.
    uint32_t first_sample;
    uint32_t accumulate;    // k_resolve folds on from the value already in the output (RT_PASS_ACCUMULATE) instead of from 0
    float* sq_sum;          // k_resolve: also the sum of the squared item sums per pixel and channel, same layout as the output; nullptr = not wanted
    // a pass over a PIXEL LIST (rt_render_pass_pixels_device; n_list = 0: every pixel of the shard). Work item w = blk * n_list + i renders
    // block blk of output slot list[i], so consecutive items go to neighbouring listed pixels; list_map[slot] = i for every listed slot.
    const uint32_t* list; uint32_t n_list;
    const uint32_t* list_map;
    FastDiv div_list;       // n_list
    uint32_t* counts;       // k_resolve_list: counts[slot] = spp (the pass's end)
    // Camera lists (camera_lists.h; nullptr: none): per 8 x 8-pixel square of the image, (x >> 3, y >> 3) of the GLOBAL pixel, the spheres a camera
    // ray of that square can meet. A camera ray is tested against them where it is made (k_generate, k_shade's regeneration) instead of in a walk:
    // the kernel that made it writes its hit record and sets kRayAnswered in the ray record. Only for the sphere-only instances, the scene in LDS,
    // no counting (rt_api.cpp render_impl).
    const uint32_t* cam_lists; uint32_t cam_squares_x;
    uint32_t cam_shade;               // in-place camera shading, below (in what was padding: the block keeps its size, no kernel's hidden arguments move)
    const rtd::Float4* cam_spheres;   // the scene's spheres in HBM (camera_list_hit reads them there in every kernel)
    // In-place camera shading (cam_shade; 0: off; only with cam_lists): a camera ray that its square's list answers with a HIT is shaded by the lane that
    // made it, which holds ray, RNG, throughput and hit in registers, and the scattered ray is what gets stored (depth 1, kRayShaded set) — no
    // record and hit written, walked past by k_extend and read back by k_shade only to be shaded. kCamShadeGenerate: in k_generate;
    // kCamShadeRegen: in k_shade's regeneration. The host sets it only where such a shade always leaves a path that goes on (max_depth >= 2, no
    // DiffuseLight sphere) and the time slot of every record is >= 0 (rt_api.cpp render_impl).
};
constexpr uint32_t kCamShadeGenerate = 1u, kCamShadeRegen = 2u;
#ifndef RT_CAMERA_SHADE
#define RT_CAMERA_SHADE 3   // tuning builds: 0 = off, 1 = k_generate only, 3 = k_generate and k_shade's regeneration
#endif
// Bit 31 of a ray record's `from` word (ray_d.w): the ray's hit record is already written, k_extend's refill hands its lane no walk. Primitive ids
// are type << 28 | index with type < 8, so the bit is free; it is only ever set on camera rays (from = 0), and every reader of the word that
// can meet it masks it off (the refill of the sphere-only LDS walk, the drain's load), so `from` means downstream what it meant.
constexpr uint32_t kRayAnswered = 0x80000000u;
// The sign bit of a ray record's time slot (ray_o.w), only in renders with RenderDev::cam_shade: the segment before this ray was shaded where its
// camera ray was made, so it stood in no queue and the k_shade (or the drain) that reads this record counts it into `segments`. The slot holds
// the first sphere's t (>= 0 or +inf) or a time >= 0 in such renders, so the bit is free; every reader of the slot that can meet it takes the
// magnitude (the refill of the sphere-only LDS walk, the drain's load, k_shade's load). A k_shade workgroup's count of them leaves in the upper
// half of its ONE allocation atomic, 64 bits wide on the queue's size line: size += n_alloc, the word behind it += n_shaded. k_extend zeroes the
// lower word only, so the upper words accumulate over the render and the host adds them to CTR_SEGMENTS (rt_api.cpp render_impl).
constexpr uint32_t kRayShaded = 0x80000000u;

struct LaunchCfg {
    uint32_t n_cu;            // k_extend runs as a persistent grid: n_cu x (resident workgroups per CU)
    uint32_t* extend_geometry;   // optional out: resident workgroups per CU for 256- and 512-thread groups
    uint32_t features;        // F_* the scene needs
    bool scene_in_lds;
    uint32_t max_rays;        // upper bound of the rays in the queue of this launch of k_extend (sizes its grid when the queue is short)
};

// what a launcher has to say about the error it has just returned (nullptr: nothing beyond hipGetErrorString)
const char* launch_note();
// the camera lists of a frame: one thread per square (kernels.hip k_camera_lists); `order`: the tree's spheres in the order the record array
// reaches their leaves (rt_api.cpp camera_order); lists: n_squares * rtcl::kListWords words
struct CamListsDev { rtcl::Camera cam; const float* spheres; const uint32_t* order; uint32_t n_order; uint32_t* lists; uint32_t n_squares; };
hipError_t launch_camera_lists(const CamListsDev& cl, hipStream_t stream);
// whether the kernels a scene of these features runs are the ones compiled to honour kRayAnswered (the sphere-only variant)
bool camera_lists_fit(uint32_t features);
// sc: the scene, for the in-place shade of the instances with camera lists (RenderDev::cam_shade)
hipError_t launch_generate(const SceneDev& sc, const PoolDev& pool, const RenderDev& rd, uint32_t n_init, uint32_t* out_count, hipStream_t stream);
// One wavefront iteration = launch_extend then launch_shade. No memsets in between: k_extend zeroes
// the count the following k_shade appends to, k_shade zeroes the queue head of the next k_extend.
hipError_t launch_extend(const LaunchCfg& cfg, const SceneDev& sc, const PoolDev& pool, const RenderDev& rd, const uint32_t* count_ptr,
                         uint32_t* head, uint32_t* count_out_to_zero, unsigned long long* counters, bool count, hipStream_t stream);
// The rest of a render in one launch: every path of `pool` (at most max_count) is carried to its end by one lane (kernels.hip DRAIN).
hipError_t launch_drain(const LaunchCfg& cfg, const SceneDev& sc, const PoolDev& pool, const RenderDev& rd, uint32_t max_count, const uint32_t* count_ptr,
                        uint32_t* head, uint32_t* count_out_to_zero, unsigned long long* counters, bool count, hipStream_t stream);
hipError_t launch_shade(const LaunchCfg& cfg, const SceneDev& sc, const PoolDev& in, const PoolDev& out, const RenderDev& rd, uint32_t max_count,
                        const uint32_t* count_in, uint32_t* count_out, uint32_t* head_to_zero, unsigned long long* counters,
                        bool count, hipStream_t stream);
// whether the kernels compiled for these features can test the first sphere where a ray is made (RenderDev::first_in_shade)
bool can_test_first_in_shade(uint32_t features);
hipError_t launch_resolve(const RenderDev& rd, float* out, uint32_t n_valid_pixels, hipStream_t stream);
// adaptive sampling (kernels.hip: the list pass's resolve; adaptive.hip: list check, slot -> list index map, selection, per-pixel write_color)
hipError_t launch_resolve_list(const RenderDev& rd, float* out, hipStream_t stream);
hipError_t launch_list_check(const uint32_t* list, uint32_t n, const uint32_t* counts, uint32_t first_sample, uint32_t width, uint32_t height, uint32_t shard_count,
                             uint32_t shard_index, uint32_t tile_size, uint32_t tiles_x, uint32_t slots, uint32_t* verdict, hipStream_t stream);
hipError_t launch_list_map(const uint32_t* list, uint32_t n, uint32_t* map, hipStream_t stream);
struct SelectArgs {
    const float* rgb; const float* sq; const uint32_t* counts;
    uint32_t slots, first_sample, frame_samples, m, min_samples;
    double rel_error, abs_error;
    uint32_t width, height, shard_count, shard_index, tile_size, tiles_x;   // slot -> pixel: clipped slots of edge tiles are never selected
};
// wave ballots (masks: slots / 64 rounded up), one-workgroup scan of their popcounts (offsets, *n_out), scatter into out
hipError_t launch_select(const SelectArgs& a, unsigned long long* masks, uint32_t* offsets, uint32_t* out, uint32_t* n_out, hipStream_t stream);
// write_color (main.rs:141-169) of one channel sum, in the reference's f64, operation for operation (host/rt_host.hpp rt::write_color is
// the definition): the body of k_write_color (kernels.hip) and of k_write_color_counts (adaptive.hip). In f32 the byte is off by one on
// sums next to a byte's boundary (1703 of 10023 such inputs), a handful per 1200 x 800 frame.
__device__ inline uint8_t write_color_byte(float sum, uint32_t spp) {
    double c = (double)sum;
    if (c != c) c = 0.0;
    const double scale = 1.0 / (double)spp;
    c = sqrt(scale * c);
    c = c < 0.0 ? 0.0 : (c > 0.999 ? 0.999 : c);
    const double q = 256.0 * c;
    return q != q ? (uint8_t)0 : (uint8_t)q;   // Rust `as u8`: saturating, NaN -> 0
}
hipError_t launch_write_color_counts(const float* rgb_sum, const uint32_t* counts, uint32_t n_pixels, uint8_t* rgb8, hipStream_t stream);
hipError_t launch_write_color(const float* rgb_sum, uint32_t n_pixels, uint32_t spp, uint8_t* rgb8, hipStream_t stream);
// ray queries (kernels.hip "ray queries"). RaySrcDev: the RtHittable record every primitive came from, by kind (scene_compile.hpp) — its own
// block, not part of SceneDev: no render kernel's arguments change.
struct RaySrcDev { const uint32_t* sphere; const uint32_t* moving; const uint32_t* rect; const uint32_t* tri; };
// rays [first, first + n) of the list (RtRay records) into `pool`, spread over its queues; `counts` (zeroed by the caller) receives the queues'
// sizes, counters[CTR_SEGMENTS] counts the rays stored. n <= kQueues * queue_cap, queue_cap % 512 == 0. An invalid ray gets its answer at once:
// its RtRayHit in `answers`, or with `occlusion` (kernels.hip "occlusion queries") its byte, RT_RAYHIT_INVALID_RAY. limit_in_d (occlusion only) =
// !extend_any_is_closest(scene): the record carries the ray's limit where the any-hit walk reads it.
hipError_t launch_rays_import(const void* rays, uint32_t first, uint32_t n, const PoolDev& pool, uint32_t queue_cap, uint32_t* counts, void* answers,
                              unsigned long long* counters, bool occlusion, bool limit_in_d, hipStream_t stream);
// after launch_extend: one RtRayHit per pool slot, at its ray's index (max_count: upper bound of the rays in one queue)
hipError_t launch_rays_export(const LaunchCfg& cfg, const SceneDev& sc, const RaySrcDev& src, const PoolDev& pool, uint32_t queue_cap, uint32_t max_count,
                              const uint32_t* counts, void* hits, hipStream_t stream);
// occlusion queries: launch_extend_any is the any-hit k_extend, or the closest-hit k_extend_wide for a scene uploaded with the 8-wide tree; the
// export writes 0 / RT_RAYHIT_HIT at every stored ray's index.
bool extend_any_is_closest(const SceneDev& sc);
hipError_t launch_extend_any(const LaunchCfg& cfg, const SceneDev& sc, const PoolDev& pool, const RenderDev& rd, const uint32_t* count_ptr,
                             uint32_t* head, uint32_t* count_out_to_zero, unsigned long long* counters, hipStream_t stream);
hipError_t launch_occluded_export(const PoolDev& pool, uint32_t queue_cap, uint32_t max_count, const uint32_t* counts, void* occluded, hipStream_t stream);
// light-sample queries (kernels.hip "light-sample queries"): n RtLightQuery records -> n RtLightSample records, one lane each, no pool. features: the
// scene's (F_LIGHTS_EXT: the lights table holds rtd::LightX records; F_LIGHTS_TREE: and the light tree). The scene has lights (n_lights > 0).
hipError_t launch_sample_lights(const SceneDev& sc, uint32_t features, const void* queries, void* results, uint32_t n, hipStream_t stream);
// first-hit features (kernels.hip "first-hit features"). FeatDev: one chunk of a feature pass — samples [k0, k0 + nk) of the pass, of output
// slots [slot0, slot0 + ns) — and where its results go; its own block, like RaySrcDev. Ray r = k * ns + s of the chunk is sample
// first_sample + k0 + k of slot slot0 + s; its 32-byte record is rec[2 r], rec[2 r + 1].
struct FeatDev {
    uint32_t first_sample, k0, nk, slot0, ns; FastDiv div_ns;
    uint32_t accumulate;        // the fold starts from the planes' values instead of 0
    rtd::Float4* rec;           // [2 * ns * nk], owned by the context
    float* albedo; float* normal; float* depth; uint32_t* hits;   // the caller's planes, nullptr = not wanted
};
// the chunk's camera rays (RenderDev: camera, frame, tiling, seed, queue geometry) into `pool`; `counts` (zeroed by the caller) receives the queues'
// sizes, counters[CTR_SEGMENTS] counts the rays. ns * nk <= kQueues * rd.queue_cap, rd.queue_cap % 512 == 0.
hipError_t launch_features_import(const RenderDev& rd, const FeatDev& fd, const PoolDev& pool, uint32_t* counts, unsigned long long* counters, hipStream_t stream);
// after launch_extend: one feature record per pool slot (max_count: upper bound of the rays in one queue); then the per-slot fold into the planes
hipError_t launch_features_export(const LaunchCfg& cfg, const SceneDev& sc, const RenderDev& rd, const FeatDev& fd, const PoolDev& pool, uint32_t max_count,
                                  const uint32_t* counts, hipStream_t stream);
// moments (rt_hip.h "first-hit features, second moments"): the caller's squared-sum planes beside the sums, nullptr = not wanted. Its own block
// beside FeatDev, so that the kernels which take FeatDev alone keep their arguments.
struct FeatMomDev { float* albedo_sq; float* normal_sq; float* depth_sq; };
hipError_t launch_features_fold(const RenderDev& rd, const FeatDev& fd, const FeatMomDev* moments, hipStream_t stream);
// radiance queries (kernels.hip "radiance queries"). RadianceDev: one chunk of a query — samples [rd.first_sample, rd.first_sample + n_samples)
// of rays [ray0, ray0 + n) of the caller's list — as a pixel-list pass over a virtual unsharded frame whose pixel index is the ray's STREAM:
// item blk * n + i is sample blk of ray ray0 + i, which runs on stream (pixel) stream0 + i. Its own block, like RaySrcDev and FeatDev.
struct RadianceDev {
    const void* rays;           // the caller's RtPathRay records (32 bytes each), the whole list
    uint64_t ray0;              // first ray of the chunk
    uint32_t n, n_samples;      // rays and samples of the chunk; n * n_samples <= kQueues * rd.queue_cap
    FastDiv div_n;
    uint32_t stream0;           // stream of ray ray0; (stream0 + n) * n_samples <= 2^32 - 1 (the item id, kernels.hip item_id)
    uint32_t* iota;             // [n], written here: iota[i] = i. The pass's rd.list is this table and its rd.list_map is (iota - stream0)
    uint8_t* invalid;           // the caller's flag bytes, the whole list (nullptr = not wanted)
};
// the chunk's rays as full path records into `pool` (T = 1, the ray starts on nothing, first_draw draws made), spread over its queues; `counts`
// (zeroed by the caller) receives the queues' sizes, counters[CTR_SAMPLES] counts the paths DROPPED. An invalid ray is dropped: its flag byte is
// written, and its items' sums in rd.blocksum are zero. rd: the pass's RenderDev (n_blocks = n_samples, queue geometry, blocksum, first_in_shade).
hipError_t launch_radiance_import(const RenderDev& rd, const RadianceDev& qd, const PoolDev& pool, uint32_t* counts, unsigned long long* counters, hipStream_t stream);
// multi-GPU root: gathered shard buffers -> full frame (rt_multi.cpp)
hipError_t launch_untile_f32(const float* gathered, float* frame, uint32_t width, uint32_t height, uint32_t ts, uint32_t tiles_x, uint32_t world, uint64_t per_shard,
                             hipStream_t stream);
hipError_t launch_untile_u8(const uint8_t* gathered, uint8_t* frame, uint32_t width, uint32_t height, uint32_t ts, uint32_t tiles_x, uint32_t world, uint64_t per_shard,
                            hipStream_t stream);

}  // namespace rtk
