/*
 * rt_hip.h — C ABI of the MI355X path-tracing hot path.
 *
 * This is the drop-in boundary for the reference renderer's per-pixel sample loop
 * (reference: raytracer/src/main.rs:730-784 — the two pixel loops, minus write_color and the
 * pixel store). Scene construction (main.rs:668-718), tone-map (main.rs:141-169) and image encode
 * (main.rs:791-796) stay on the host side of this boundary.
 *
 * A scene crosses the boundary as the reference's own object graph, serialised into flat arrays:
 * one RtHittable per `Arc<dyn Hittable>` (hittable.rs:51-60), one RtMaterial per
 * `Arc<dyn Material>` (material.rs:11-21), one RtTexture per `Arc<dyn Texture>` (texture.rs:7-9).
 * The library compiles that graph into its device layout (threaded BVH + per-type primitive
 * arrays) at upload; the caller never sees device structures.
 *
 * Plain C: pointers and sizes only, no C++ or torch types. All geometry is f64 at the boundary
 * (the reference is f64 throughout, vec3.rs:5-8); the device path computes in f32.
 *
 * Error convention: every entry point returns 0 on success or a negative RtStatus; a message is
 * available from rt_last_error(). Nothing aborts and no C++ exception crosses the boundary
 * (the reference panics instead: main.rs:656,762,777,779).
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 3u

typedef enum RtStatus {
    RT_OK = 0,
    RT_ERR_INVALID = -1,      /* bad argument / malformed scene graph */
    RT_ERR_UNSUPPORTED = -2,  /* graph shape the device compiler does not handle */
    RT_ERR_DEVICE = -3,       /* HIP runtime error (message has hipGetErrorString) */
    RT_ERR_NO_DEVICE = -4,    /* no usable GPU: the product path has no CPU fallback */
    RT_ERR_OOM = -5,
    RT_ERR_PEER = -6          /* a collective render (rt_render_gather / rt_render_multi) was called off because ANOTHER rank failed
                                 its part; the message names the rank. Every rank of the collective returns — none waits for a
                                 shard that will not come (the reference's convention is to panic: main.rs:762,777) */
} RtStatus;

/* vec3.rs:5-8 */
typedef struct RtVec3 { double x, y, z; } RtVec3;

/* camera.rs:6-18, field for field. Filled by the host-side Camera::new (camera.rs:21-59). */
typedef struct RtCamera {
    RtVec3 origin;
    RtVec3 lower_left_corner;
    RtVec3 horizontal;
    RtVec3 vertical;
    RtVec3 u, v, w;
    double lens_radius;
    double time0, time1;
} RtCamera;

/* texture.rs */
typedef enum RtTextureKind {
    RT_TEX_SOLID = 0,    /* texture.rs:12-38  */
    RT_TEX_CHECKER = 1,  /* texture.rs:41-69  */
    RT_TEX_NOISE = 2,    /* texture.rs:72-96  */
    RT_TEX_IMAGE = 3     /* texture.rs:99-140 */
} RtTextureKind;

typedef struct RtTexture {
    int32_t kind;
    int32_t a;      /* checker: `even` texture id; noise: perlin id; image: image id (-1 = empty) */
    int32_t b;      /* checker: `odd` texture id */
    int32_t _pad;
    RtVec3 color;   /* solid: color_value */
    double scale;   /* noise: scale */
} RtTexture;

/* perlin.rs:7-12 — tables are built on the host (perlin.rs:14-25,53-66) */
typedef struct RtPerlin {
    double ranvec[256][3];
    uint32_t perm_x[256];
    uint32_t perm_y[256];
    uint32_t perm_z[256];
} RtPerlin;

/* texture.rs:99-104 — RGB8, row-major, bytes_per_scanline = 3*width */
typedef struct RtImage {
    const uint8_t* data;
    uint32_t width;
    uint32_t height;
} RtImage;

/* material.rs */
typedef enum RtMaterialKind {
    RT_MAT_LAMBERTIAN = 0,     /* material.rs:23-72   */
    RT_MAT_METAL = 1,          /* material.rs:74-108  */
    RT_MAT_DIELECTRIC = 2,     /* material.rs:110-156 */
    RT_MAT_DIFFUSE_LIGHT = 3,  /* material.rs:158-191 */
    RT_MAT_ISOTROPIC = 4       /* material.rs:193-220 (commented out in the reference: spec only) */
} RtMaterialKind;

typedef struct RtMaterial {
    int32_t kind;
    int32_t texture;  /* lambertian albedo / diffuse-light emit / isotropic albedo: texture id */
    RtVec3 albedo;    /* metal */
    double fuzz;      /* metal; the constructor clamps to <= 1 (material.rs:90) */
    double ir;        /* dielectric */
} RtMaterial;

/* One record per `Arc<dyn Hittable>` of the reference graph. */
typedef enum RtHittableKind {
    RT_HIT_SPHERE = 0,          /* sphere.rs:11-24         p = center[3], radius                     */
    RT_HIT_MOVING_SPHERE = 1,   /* moving_sphere.rs:8-34   p = center0[3], center1[3], time0, time1, radius */
    RT_HIT_XY_RECT = 2,         /* aarect.rs:10-29         p = x0, x1, y0, y1, k                      */
    RT_HIT_XZ_RECT = 3,         /* aarect.rs:60-79         p = x0, x1, z0, z1, k                      */
    RT_HIT_YZ_RECT = 4,         /* aarect.rs:129-148       p = y0, y1, z0, z1, k                      */
    RT_HIT_TRIANGLE = 5,        /* not in the reference (README.md:151-153): p = v0[3], v1[3], v2[3]  */
    RT_HIT_BOX = 6,             /* boxes.rs:11-75          p = p0[3], p1[3]  (six rects, boxes.rs order) */
    RT_HIT_LIST = 7,            /* hittable_list.rs:11-36  children                                   */
    RT_HIT_BVH = 8,             /* bvh.rs:10-14,74         children, p = time0, time1                 */
    RT_HIT_TRANSLATE = 9,       /* hittable.rs:62-74       first_child = child id, p = offset[3]      */
    RT_HIT_ROTATE_Y = 10,       /* hittable.rs:98-145      first_child = child id, p = angle (degrees) */
    RT_HIT_FLIP_FACE = 11,      /* hittable.rs:183-193     first_child = child id                     */
    RT_HIT_CONSTANT_MEDIUM = 12 /* constant_medium.rs:9-29 (commented spec) first_child = boundary id,
                                   material = phase function (isotropic), p = density                 */
} RtHittableKind;

typedef struct RtHittable {
    int32_t kind;
    int32_t material;      /* material id for primitives, boxes and media; -1 otherwise */
    int32_t first_child;   /* LIST/BVH: offset into children[]; wrappers/medium: child hittable id */
    int32_t n_children;    /* LIST/BVH: number of children; wrappers/medium: 1; primitives: 0 */
    double p[10];
} RtHittable;

typedef enum RtBackgroundMode {
    RT_BG_CONSTANT = 0,     /* main.rs:692 `background` colour returned on a miss (main.rs:74-76) */
    RT_BG_SKY_GRADIENT = 1  /* book-1 sky: (1-t)*white + t*background, t = 0.5*(unit(d).y + 1);
                               not in the reference (it only has the constant colour) */
} RtBackgroundMode;

typedef enum RtBvhBuilder {
    RT_BVH_REFERENCE = 0,  /* BVHNode::construct as intended (bvh.rs:77-130): random axis, median split */
    RT_BVH_SAH = 1         /* binned surface-area heuristic: same pictures (a BVH only culls), far fewer
                              node visits on large scenes; SURVEY.md 8(f) rank 1 */
} RtBvhBuilder;

/* ---- RtSceneDesc.scene_flags --------------------------------------------------------------------------------------------------------------
 * RT_SCENE_LIGHTS_ALL_SHAPES: every member of the lights list is sampled as a light. The reference implements pdf_value / random for XzRect
 * and Sphere only (aarect.rs:107-125, sphere.rs:75-90); every other member takes the trait defaults (pdf 0, direction (1,0,0):
 * hittable.rs:54-59), which is what the library does with the flag clear, bit for bit. With the flag set a member may be
 *   - an XY, XZ or YZ rect: two draws, range(a0, a1) then range(b0, b1), the point on the plane; pdf = t^2 |v|^2 / (|cos| area);
 *   - a triangle: two draws r1 then r2, s = sqrt(r1), the point (1 - s) v0 + s (1 - r2) v1 + s r2 v2; pdf = t^2 |v|^2 / (|cos| area) with
 *     the hit test the walk uses (closed edges);
 *   - a box: one next64() % 6 pick of a side in boxes.rs order (z1 z0 y1 y0 x1 x0), then that rect's two draws; pdf_value = 1/6 of the sum
 *     over the sides the ray meets (the list rule, hittable_list.rs:73-84, applied to the box's own sides);
 *   - a sphere, as ever;
 *   - any chain of up to 6 Translate / RotateY / FlipFace above one of these: the chain is composed into one rigid map at upload, the pdf
 *     is evaluated in the member's own space (a rigid map keeps it), a drawn direction is rotated back; FlipFace changes nothing.
 * Anything else in the lights list — a moving sphere, a medium, a nested list, a BVH, a rect or triangle of zero area, a deeper chain — is
 * RT_ERR_INVALID with the reason, and nothing is uploaded. The list semantics stay the reference's: the pick is next64() % n, uniform over
 * the members whatever their size, and the list's pdf is the mean of the members' pdfs, occluded or not.
 * LIMIT (of RT_SCENE_LIGHTS_ALL_SHAPES alone): the cost is linear in the number of lights per Lambertian bounce (every member's pdf is
 * evaluated for every scattered ray) and the pick ignores the members' size; an emissive mesh of thousands of triangles is slow and noisy.
 * With this flag alone there is no light BVH and no area-weighted pick. RT_SCENE_LIGHTS_MANY brings both; what stays: the pick weighs by area, not by emitted power, and a leaf of the light tree holds one member.
 * RtStats.prim_tests counts the light tests with their kind: triangles in the triangle slot, rects and boxes (six each) in the rect slot,
 * spheres in the sphere slot. A list of bare XZ rects and spheres runs the same kernels and uploads the same bytes with the flag as without.
 *
 * RT_SCENE_LIGHTS_MANY (needs RT_SCENE_LIGHTS_ALL_SHAPES: alone it is RT_ERR_INVALID; value 2 stays an unknown bit): the list for many lights.
 * Every refusal above applies unchanged. What changes:
 *   - PICK. A member is picked with probability proportional to its surface area, from the desc's f64 parameters: rect |(a1-a0)(b1-b0)|,
 *     triangle 0.5 |e1 x e2|, box 2 (dx dy + dy dz + dz dx), sphere 4 pi r^2. Host rule, f64, list order: total = the sequential sum of the
 *     areas; p_k = (float)(A_k / total); cdf_k = (float)((A_0 + .. + A_k) / total), summed sequentially; cdf_{n-1} = 1.0f exactly. Device
 *     rule: u = ONE rnd() draw (where the uniform pick spends one next64()), k = the first index with cdf_k > u (binary search). The member's
 *     own `random` is unchanged, the box's uniform side pick included. RtLightSample.light stays the member's index in the caller's list.
 *   - PDF. The list's pdf at (p, d) is sum_k p_k pdf_k(p, d) over all members, occluded or not: with the pick above the estimator stays
 *     unbiased. It is evaluated through a binary tree over the members' padded world-space boxes (built on the host, deterministic; one
 *     member per leaf, 2n - 1 records in pre-order with skip links): a member whose box the ray (t > 0.001) misses is not tested. The
 *     tree only culls; the sum runs over the members in the tree's leaf order with one fmaf per member, whichever way it is evaluated
 *     (RT_LIGHTQ_LINEAR below). rt_scene_light_tree_dump shows the records, the order and the weights.
 *   - The scene always takes the extended light records (RtCompileInfo.features has 256 and 512), also for a list of bare XZ rects and spheres.
 *   - RtStats.prim_tests counts the member tests that are made, by kind, as above; the light tree's own box tests are NOT counted into
 *     node_tests (that figure stays the world walk's). */
enum { RT_SCENE_LIGHTS_ALL_SHAPES = 1u, RT_SCENE_LIGHTS_MANY = 4u };

typedef struct RtSceneDesc {
    uint32_t abi_version;   /* RT_ABI_VERSION */
    uint32_t scene_flags;   /* RT_SCENE_*; an unknown bit is RT_ERR_INVALID. 0 = the reference's behaviour */
    const RtHittable* hittables;  uint64_t n_hittables;
    const int32_t*    children;   uint64_t n_children;
    const RtMaterial* materials;  uint64_t n_materials;
    const RtTexture*  textures;   uint64_t n_textures;
    const RtPerlin*   perlins;    uint64_t n_perlins;
    const RtImage*    images;     uint64_t n_images;
    int32_t world;            /* root hittable id (main.rs:668 `world`) */
    int32_t lights;           /* root of the lights list (main.rs:669-686) or -1: no lights, the
                                 integrator then samples CosinePdf only (book-1/2 behaviour) */
    int32_t background_mode;  /* RtBackgroundMode */
    int32_t bvh_builder;      /* RtBvhBuilder: how RT_HIT_BVH objects are built on the device side */
    RtVec3 background;        /* constant colour, or the sky gradient's far colour (0.5,0.7,1.0) */
    uint64_t bvh_seed;        /* seeds the per-node axis draw of BVHNode::construct (bvh.rs:87) */
} RtSceneDesc;

typedef enum RtNanPolicy {
    RT_NAN_PER_SAMPLE = 0,  /* a non-finite sample contributes 0 (documented deviation) */
    RT_NAN_REFERENCE = 1    /* samples are summed as they are; write_color scrubs the pixel SUM
                               (main.rs:146-155): one NaN sample blacks the pixel */
} RtNanPolicy;

enum {
    RT_FLAG_COUNTERS = 1u,  /* count AABB tests and primitive tests on the device (slower) */
    RT_FLAG_TIMING = 2u,    /* bracket every kernel launch with HIP events (RtStats *_ms) */
    RT_FLAG_SAMPLE_BLOCKS = 4u, /* work items of 16 consecutive samples of a pixel, as for images of 2^32 - 2^28 samples and more
                                   (default below that: one sample per item). Per-pixel sums then differ in the last bits. */
    RT_FLAG_FUSED = 8u,         /* diagnostic: the whole render by the fused per-path kernel that normally carries only the tail (one
                                   lane per path from first ray to last bounce). Bit-identical frame, slower. */
    RT_FLAG_NO_CAMERA_LISTS = 16u /* camera rays are walked through the tree like every other ray instead of being tested, where they are made,
                                   against the list of spheres their 8 x 8-pixel square can meet (sphere-only scenes in LDS). Bit-identical
                                   frame; for A/B runs and tests. An unknown bit in flags is RT_ERR_INVALID. */
};

typedef struct RtParams {
    uint32_t width, height;       /* main.rs:660-661 */
    uint32_t samples_per_pixel;   /* main.rs:662 */
    uint32_t max_depth;           /* main.rs:663 */
    uint64_t seed;                /* render seed: output is a pure function of (scene, camera, params) */
    uint32_t nan_policy;          /* RtNanPolicy */
    uint32_t flags;               /* RT_FLAG_* */
    /* framebuffer sharding (one process per GPU): the image is cut into tile_size x tile_size
       tiles, numbered row-major; this call renders tiles t with t % shard_count == shard_index.
       shard_count <= 1 renders the whole image. */
    uint32_t tile_size;           /* 0 = default (32) */
    uint32_t shard_index;
    uint32_t shard_count;
    uint32_t pool_slots;          /* paths in flight; 0 = one per work item, up to 2^28 and to 70 % of the free device memory */
    uint32_t tail_paths;          /* once at most this many paths are alive, ONE launch of the per-path kernel carries each of them to its end
                                     instead of one launch pair per bounce (same frame bit for bit). 0 = default (2^18); 1 = never */
    uint32_t _pad;
} RtParams;

#define RT_N_PRIM_TYPES 6  /* sphere, moving sphere, rect, triangle, medium, instance transform */

typedef struct RtStats {
    double render_ms;         /* first launch to framebuffer resident at the destination */
    double extend_ms;         /* sum of traversal-kernel durations (HIP events; RT_FLAG_TIMING) */
    double shade_ms;          /* sum of shade-kernel durations */
    double other_ms;          /* generate / resolve kernels */
    uint64_t samples;         /* camera paths traced */
    uint64_t segments;        /* ray segments traced (world.hit calls, main.rs:74) */
    uint64_t node_tests;      /* box tests the device made (RT_FLAG_COUNTERS). They are the reference's Aabb::hit evaluations when the scene was
                                 uploaded under RT_LAYOUT_REFERENCE_COUNTERS; the default layouts cull HittableList
                                 members behind boxes of their own and visit BVH children near-first: same hits, fewer tests */
    uint64_t prim_tests[RT_N_PRIM_TYPES];   /* primitive hit() evaluations, by kind (a Box counts its six rects) */
    uint32_t iterations;      /* wavefront iterations */
    uint32_t extend_launches;
    uint32_t shade_launches;
    uint32_t pool_slots;
    uint64_t scene_nodes;     /* threaded-BVH nodes on the device */
    uint64_t scene_prims;
    uint64_t scene_bytes;     /* device bytes of nodes + primitives */
    uint32_t bvh_in_lds;      /* 1 if the whole node/primitive set is staged in LDS */
    uint32_t _pad;
    uint64_t debug[8];        /* diagnostic builds only (in-kernel cycle stamps); 0 otherwise */
    double gather_ms;         /* multi-GPU: RCCL gather + untile on the root device (HIP events on the root's stream) */
    uint32_t n_devices;       /* GPUs that took part (1 for rt_render / rt_render_device) */
    uint32_t lds_top_nodes;   /* node records of the top of the tree staged in LDS when the whole scene does not fit (0 otherwise) */
    double drain_ms;          /* duration of the fused kernel that carries the last paths to their end (RT_FLAG_TIMING) */
    uint32_t drain_paths;     /* upper bound of the paths handed to it (0: the wavefront loop ran to the end) */
    uint32_t _pad2;
} RtStats;

typedef struct RtCtx RtCtx;      /* one per (process, device, stream); not re-entrant (one render at a time per context; distinct
                                    contexts may be used from distinct host threads) */
typedef struct RtScene RtScene;  /* device-resident compiled scene, owned by the library */

/* Create a context on `device_id`. `stream` is a hipStream_t to launch on (so a caller such as
   PyTorch can order the work with its own), or NULL for a stream owned by the library. */
int rt_ctx_create(int device_id, void* stream, RtCtx** out_ctx);
int rt_ctx_destroy(RtCtx* ctx);

/* Compile the graph and copy it to the device. The caller keeps ownership of every pointer in
   `desc`; nothing in it is retained after the call returns. */
int rt_scene_upload(RtCtx* ctx, const RtSceneDesc* desc, RtScene** out_scene);
int rt_scene_destroy(RtCtx* ctx, RtScene* scene);

/* ---- how a scene is laid out on the device: per upload, in the ABI (a host with threads cannot set process environment per scene) ----
 * None of these changes a picture: they trade box tests, primitive tests and memory against each other. (Exactly: a ray that meets two
 * primitives at the SAME t — a sphere at its point of contact with the plane it rests on — is given to the one tested later, here as in
 * the reference, hittable_list.rs:40-47; layouts test in different orders. In the 1 M-sphere scene, where every sphere rests on the
 * ground rect, 2e-4 of the pixels hold such a sample; in the books' scenes none does.) The defaults are what
 * the library measures fastest; RT_LAYOUT_REFERENCE_COUNTERS is the layout whose RtStats test counts are the reference's own
 * (HittableList::hit probing every member, hittable_list.rs:39-51; BVHNode::hit visiting left then right, bvh.rs:134-143) — the
 * parity tests compare those counts with the CPU oracle's. Environment variables of the same names as in scripts/ still exist
 * as overrides for experiments; no test and no host depends on them. */
enum {
    RT_LAYOUT_LISTS_AS_REFERENCE = 1u,   /* every HittableList member in front of every ray, nothing tested at the start of a walk (default: members every ray
                                            meets anyway — a moving sphere, an all-enclosing medium, a sphere of the root BVH as large as the scene — are tested
                                            when a walk begins and left out of the tree) */
    RT_LAYOUT_LISTS_CULLED = 2u,         /* members behind culling boxes even in a scene that is only a list (default: when the scene holds a BVH of >= 32 members) */
    RT_LAYOUT_NO_MEMBER_BOXES = 4u,      /* the two members of a span-2 BVH node tested directly, as bvh.rs:99-107 does (default: a sphere gets a box of its own in LDS-sized scenes) */
    RT_LAYOUT_MEMBER_BOXES = 8u,         /* ... boxes of their own in any scene */
    RT_LAYOUT_CHILD_ORDER_AS_REFERENCE = 16u, /* one record array, left child before right (default for scenes in HBM: one array per direction octant, near child first) */
    RT_LAYOUT_SCENE_IN_HBM = 32u,        /* do not stage a small scene in LDS */
    RT_LAYOUT_NODES_32B = 64u,           /* scenes in HBM: 32-byte f32 records (with the top of the tree in LDS) instead of compressed ones */
    RT_LAYOUT_NO_SHADE_TABLES_IN_LDS = 128u,
    RT_LAYOUT_NO_EXTEND_TABLES_IN_LDS = 256u,
    RT_LAYOUT_WIDE_NODES = 512u,         /* static BVH in HBM: walk an 8-wide tree, 8 lanes to a ray, one 128-byte node per visit (measured slower than
                                            the default binary records on MI355X — VALU-bound at 8 rays per wave, DESIGN.md section 5 — kept as an option) */
    RT_LAYOUT_ALL_BOX_NODES = 1024u,     /* keep every box record of the tree (default, in a scene staged in LDS: an inner box that most rays which reach it pass anyway
                                            is left out and its children take its place — fewer box tests, the same leaves in the same order; off by itself under
                                            LISTS_AS_REFERENCE, NO_MEMBER_BOXES, SCENE_IN_HBM and WIDE_NODES) */
    RT_LAYOUT_REFERENCE_COUNTERS = 1u | 4u | 16u
};
/* ---- triangle attributes: per-vertex normals and texture coordinates ------------------------------------------------------------------------
 * RtSceneDesc stays the reference's graph; what a mesh carries beyond its positions travels beside it, keyed by hittable id, in
 * RtUploadOptions. A record names ONE RT_HIT_TRIANGLE of the desc; a triangle the graph reaches several times (under different wrappers)
 * carries its attributes in every copy. A record with flags == 0 is legal and changes nothing.
 * Semantics, with (bu, bv) the barycentrics of the hit after the closed-edge clamp (the values RtRayHit.u, v report for a plain triangle)
 * and w0 = 1 - bu - bv, all in f32 on the device:
 *   RT_TRI_NORMALS  ns = unit(w0 n0 + bu n1 + bv n2) takes the place of the facet's geometric normal in the HitRecord and nothing downstream
 *                   changes: front_face = dot(d, ns) < 0, normal = +-ns, and the Translate / RotateY / FlipFace replay runs on it as it
 *                   runs on the geometric normal; "the normal opposes the ray" holds for every material. Vertex normals need not be unit:
 *                   they are normalised in f64 at upload, then rounded to f32. Where the f32 squared length of the sum is not a positive
 *                   normal number (the vertex normals cancel) the hit falls back to the geometric normal.
 *   RT_TRI_UVS      u = u0 + bu (u1 - u0) + bv (u2 - u0), v likewise: uv = (0,0), (1,0), (0,1) returns exactly (bu, bv). Without the flag the
 *                   barycentrics are (u, v), as for a plain triangle.
 * Intersection stays purely geometric: t, p, hit / miss, the closed edges, occlusion queries and the primitive a scattered ray leaves are
 * untouched. Documented limit: a direction scattered about ns can point below the facet; it is traced like any other ray and skips only
 * the triangle it leaves (no terminator fix). Renders (every kernel form, passes, pixel lists), rt_trace_rays* (n, u, v, FRONT_FACE) and
 * rt_render_features* (normal; albedo through the texture) use the interpolated values.
 * Refused with RT_ERR_INVALID and a reason, nothing uploaded: a hittable id out of range or not an RT_HIT_TRIANGLE, an id listed twice, an
 * unknown flag bit, a non-finite normal or uv whose flag is set, a vertex normal of zero length under RT_TRI_NORMALS, n_triangle_attrs > 0
 * with a NULL pointer. */
enum { RT_TRI_NORMALS = 1u, RT_TRI_UVS = 2u };
typedef struct RtTriangleAttrs {      /* 68 B */
    int32_t  hittable;                /* id of an RT_HIT_TRIANGLE record of the desc */
    uint32_t flags;                   /* RT_TRI_*; an unknown bit is RT_ERR_INVALID */
    float    n[3][3];                 /* normal at v0, v1, v2, in the triangle's own (pre-wrapper) space; need not be unit */
    float    uv[3][2];                /* texture coordinates at v0, v1, v2 */
} RtTriangleAttrs;

/* ---- environment map: an HDR equirectangular image as background and, with RT_ENV_SAMPLED, as a light ----------------------------------------
 * Travels beside the scene in RtUploadOptionsEnv.env_map, the grown options record below (rt_scene_upload_ex, rt_scene_upload_multi_ex, rt_scene_compile_info_ex). When it is
 * present a ray that leaves the scene returns the map's radiance; RtSceneDesc.background_mode and background are then not read. The map is
 * served by everything that shades a miss: renders in every kernel form, passes and pixel lists, radiance queries, rt_render_features* (the
 * albedo of a miss is the map's radiance, as it is the background's without a map) and rt_sample_lights. The pointers are the caller's;
 * nothing is retained after the upload returns. A scene uploaded without a map runs exactly the kernels it runs without this struct.
 *
 * LOOKUP, f32 on the device. The image texture's rule, so that a map equals that image on an enclosing sphere: ud = unit(d);
 *   u = (atan2(-ud.z, ud.x) + pi) / (2 pi), v = acos(-ud.y) / pi (sphere.rs:32-37); then texture.rs:117-140: u, v clamped to [0, 1],
 *   v := 1 - v, i = (uint)(u W), j = (uint)(v H), each clamped to W - 1, H - 1. Radiance = scale * rgb[(j W + i) * 3 ..]. Row 0 is up (+y);
 *   column 0 begins at -x and the columns turn towards +z.
 *   LIMITS: the nearest texel, no filtering; no rotation of the map.
 * TABLES, on the host in f64, sequentially (the style of the RT_SCENE_LIGHTS_MANY cdf): f_ij = (0.2126 R + 0.7152 G + 0.0722 B) *
 *   sin(pi (j + 0.5) / H) from the texels as given (scale left out: it cancels). Row sum r_j = f_j0 + f_j1 + ..; total = r_0 + r_1 + ..;
 *   marg[j] = (float)((r_0 + .. + r_j) / total), a sequential running sum, marg[H-1] = 1.0f exactly; cond[j][i] = (float)((f_j0 + .. + f_ji)
 *   / r_j), cond[j][W-1] = 1.0f exactly; a row with r_j = 0 gets the uniform cdf (float)((i + 1) / W). A map whose total is 0 gets the
 *   uniform marginal as well (and cannot be sampled, below). rt_env_tables returns the tables as the upload builds them.
 * DRAW, exactly two rnd(): u1 gives j = the first index with marg[j] > u1, u2 gives i = the first index with cond[j][i] > u2 (binary
 *   searches). fy = (u1 - lo) / (hi - lo) with lo, hi the cdf entries before and at j (lo = 0 for j = 0), fx likewise. With a = (i + fx) / W
 *   and b = (j + fy) / H the direction is the inverse of the lookup: d = (-sin(pi b) cos(2 pi a), cos(pi b), sin(pi b) sin(2 pi a)).
 * PDF, always from the direction, by the LOOKUP's texel (i, j), never from the drawn texel: mass_ij W H / (2 pi^2 sin_theta) with mass_ij
 *   = (marg[j] - marg[j-1]) (cond[j][i] - cond[j][i-1]) in f32 (entry -1 = 0) and sin_theta = sqrt(1 - ud.y^2); 0 where sin_theta is 0.
 * RT_ENV_SAMPLED: the map is one more member of the lights list, after the caller's n members: the pick is next64() % (n + 1), the list's pdf
 *   is the mean over the n + 1 members, RtLightSample.light is n for the map, and RtSceneDesc.lights = -1 gives a list of the map alone.
 *   Without the flag the map is found by the cosine draws only (and by the other lights' directions that happen to miss everything).
 * A scene with a map always takes the extended light records, as RT_SCENE_LIGHTS_MANY does (RtCompileInfo.features has 256 and 1024); the
 *   lights list keeps the semantics its scene_flags give it.
 * LIMIT: RT_ENV_SAMPLED together with RT_SCENE_LIGHTS_MANY is RT_ERR_INVALID: the pick of that list weighs by area and the map has none.
 *   (An unsampled map with RT_SCENE_LIGHTS_MANY is refused too, for now: the map's kernels carry no light tree.)
 * COST: a sampled map costs the light half of the Lambertian bounces two binary searches, log2 H + log2 W dependent loads (about 25 for a
 *   4096 x 2048 map), and every bounce one pdf evaluation (four loads). An alias table would make the draw two loads; it is not built.
 * REFUSED with RT_ERR_INVALID, the reason in rt_last_error, nothing uploaded: struct_bytes < sizeof(RtEnvMap); an unknown flag; a width or
 * height of 0 or above 16384; NULL rgb; a texel or a scale that is not finite or is negative; RT_ENV_SAMPLED on a map of zero total weight;
 * a map together with RT_SCENE_LIGHTS_MANY. */
enum { RT_ENV_SAMPLED = 1u };
typedef struct RtEnvMap {
    uint32_t struct_bytes, flags;      /* sizeof(RtEnvMap) as the caller compiled it; RT_ENV_*, an unknown bit is RT_ERR_INVALID */
    uint32_t width, height;            /* equirectangular, row 0 = up (+y), 1..16384 each */
    const float* rgb;                  /* width * height * 3 f32, linear radiance, finite, >= 0 */
    float scale;                       /* multiplies every texel; finite, >= 0 */
    uint32_t _pad;
} RtEnvMap;
/* Host only, no device: the map checked as an upload checks it (without a scene: the RT_SCENE_LIGHTS_MANY rule is the upload's), and the two
 * tables as the upload builds them: marg[height], cond[height * width]. Either pointer may be NULL = not wanted. */
int rt_env_tables(const RtEnvMap* env_map, float* marg, float* cond);

/* Checked, not dropped: a layout bit this library does not know, a switch set both ways (LISTS_AS_REFERENCE with LISTS_CULLED,
 * NO_MEMBER_BOXES with MEMBER_BOXES), struct_bytes < 8 or a negative list_park_cost is RT_ERR_INVALID with the reason in rt_last_error. */
typedef struct RtUploadOptions {
    uint32_t struct_bytes;     /* sizeof(RtUploadOptions) as the caller compiled it (the struct may grow at its end) */
    uint32_t layout_flags;     /* RT_LAYOUT_* */
    uint32_t lds_top_records;  /* RT_LAYOUT_NODES_32B: records of the top of the tree kept in LDS; 0 = default (1024) */
    uint32_t octant_axes;      /* near-first record arrays: 0 = the library picks the axes that matter; else 8 | mask (x = 1, y = 2, z = 4) */
    uint32_t leaf_collapse;    /* a box node whose subtree is <= n primitives of one kind becomes a leaf; 0/1 = off (default). Measured slower on every
                                  BASELINE scene (more primitive tests). The one switch that can move a sample: a ray that grazes a sphere within the
                                  rounding of its box is culled by that box in the other layouts and tested here (a handful of samples in 5e8) */
    float    list_park_cost;   /* cost of a stop at a leaf in primitive tests, for the grouping of culled list members; 0 = default (6) */
    /* read only when struct_bytes covers them (a caller compiled against the 24-byte struct keeps working): */
    const RtTriangleAttrs* triangle_attrs;   /* per-vertex normals / texture coordinates of RT_HIT_TRIANGLE records, see RtTriangleAttrs above */
    uint64_t n_triangle_attrs;               /* records in triangle_attrs; > 0 with a NULL pointer is RT_ERR_INVALID */
} RtUploadOptions;
/* The options record grown at its end, under its struct_bytes rule: the 40 bytes above, then what newer callers add. Every entry point that
 * takes a const RtUploadOptions* takes &x.base of one of these with x.base.struct_bytes = sizeof(RtUploadOptionsEnv); what lies behind the
 * 40 bytes is read only when struct_bytes covers it, so a caller compiled against RtUploadOptions (24 or 40 bytes) keeps working, and
 * sizeof(RtUploadOptions) stays what those callers compiled. */
typedef struct RtUploadOptionsEnv {
    RtUploadOptions base;                    /* base.struct_bytes = sizeof(RtUploadOptionsEnv) */
    const RtEnvMap* env_map;                 /* an environment map, see RtEnvMap above; NULL = none */
} RtUploadOptionsEnv;

/* ---- normal maps: tangent-space shading normals on triangle meshes ---------------------------------------------------------------------------
 * A map is bound to a MATERIAL of the desc; its texels are an RtImage of the desc (8-bit RGB). The binding travels beside the desc like the
 * triangle attributes and the environment map, in RtUploadOptionsMaps, the options record grown once more at its end (rt_scene_upload_ex,
 * rt_scene_upload_multi_ex, rt_scene_compile_info_ex, rt_scene_compile_dump_ex). The pointers are the caller's; nothing is retained.
 * The rules apply on a hit of an RT_HIT_TRIANGLE whose material has a map, in f32 on the device, AFTER the RT_TRI_NORMALS and RT_TRI_UVS steps
 * above. N is the unit normal those steps leave (interpolated, or the facet's unit(cross(e1, e2))); (u, v) the texture coordinates they leave
 * (attributes, or the barycentrics); uv_k the vertices' coordinates (the attributes, or (0,0), (1,0), (0,1) without RT_TRI_UVS: a triangle
 * without attributes is mapped too).
 *   1 TEXEL   the image texture's own rule (texture.rs:117-140, as the environment map's LOOKUP): u, v clamped to [0, 1], v := 1 - v,
 *             i = (uint)(u W), j = (uint)(v H), clamped to W - 1, H - 1; c = rgb8[(j W + i) 3 ..]. The nearest texel, no filtering: a map
 *             lines up texel for texel with an albedo image on the same mesh.
 *   2 DECODE  m = c (2 / 255) - 1 per channel; x = strength m.r, y = strength m.g (negated under RT_NMAP_FLIP_GREEN), z = m.b.
 *   3 FRAME   e1 = v1 - v0, e2 = v2 - v0, (du1, dv1) = uv1 - uv0, (du2, dv2) = uv2 - uv0, det = du1 dv2 - du2 dv1;
 *             T = dv2 e1 - dv1 e2, B = du1 e2 - du2 e1, both negated when det < 0; t = unit(T - N (N.T)); b = +-cross(N, t) with the sign
 *             that makes dot(b, B) >= 0. Red is +u; green is +v, which is towards row 0 of the image.
 *   4 RESULT  ns = unit(x t + y b + z N) takes the place of N and nothing downstream changes: front_face = dot(d, ns) < 0, normal = +-ns,
 *             then the Translate / RotateY / FlipFace replay and the materials. ns lives in the triangle's own space, as vertex normals do.
 *   5 FALLBACKS  N stays when det is 0 or not finite, when the squared length of T - N (N.T) is not a positive normal f32, or when the
 *             squared length of x t + y b + z N is not a positive normal f32.
 * UNCHANGED: t, p, hit / miss, the closed edges, occlusion queries, the primitive a scattered ray leaves and every light's pdf_value /
 * random stay geometric; the documented limit of RT_TRI_NORMALS applies (a direction scattered about ns may point below the facet).
 * SERVED BY renders in every kernel form (wavefront, drain tail, fused, passes, pixel lists), radiance queries, rt_trace_rays* (n,
 * FRONT_FACE) and rt_render_features* / rt_render_feature_moments* (normal). A triangle the graph reaches under several wrappers is mapped
 * in every copy. A scene with a map runs the all-features kernels (RtCompileInfo.features has 32, and 2048 when a device triangle is
 * mapped; n_tri_attrs counts every device triangle that carries a record, mapped ones without attributes included).
 * LIMITS: the nearest texel with clamped u, v; per-triangle tangents, no per-vertex tangents; triangles only.
 * REFUSED with RT_ERR_INVALID, the reason in rt_last_error, nothing uploaded: n_normal_maps > 0 with a NULL pointer; a material id out of
 * range; a material listed twice; an image id out of range, or an image with NULL data or a zero dimension; a strength that is not finite
 * or is negative; an unknown flag; a material of kind RT_MAT_DIFFUSE_LIGHT or RT_MAT_ISOTROPIC; a mapped material used by a primitive that
 * is not a triangle (sphere, moving sphere, rect, box, medium), for now — by any such record of RtSceneDesc.hittables, whether the world
 * reaches it or not: the rule is checked on the desc, before the graph is walked. A mapped material that no record uses is legal and changes
 * nothing; a scene uploaded without maps is uploaded byte for byte as before. */
enum { RT_NMAP_FLIP_GREEN = 1u };        /* maps authored with green pointing down (-v) */
typedef struct RtNormalMap {             /* 16 B */
    int32_t  material;                   /* id of an RtMaterial of the desc */
    int32_t  image;                      /* id of an RtImage of the desc */
    float    strength;                   /* scales the tangent-plane components; finite, >= 0 */
    uint32_t flags;                      /* RT_NMAP_*; an unknown bit is RT_ERR_INVALID */
} RtNormalMap;
typedef struct RtUploadOptionsMaps {
    RtUploadOptionsEnv base;             /* base.base.struct_bytes = sizeof(RtUploadOptionsMaps) */
    const RtNormalMap* normal_maps;      /* read only when struct_bytes covers both fields (callers of the 24-, 40- and 48-byte records keep working) */
    uint64_t n_normal_maps;              /* records in normal_maps; > 0 with a NULL pointer is RT_ERR_INVALID */
} RtUploadOptionsMaps;
int rt_scene_upload_ex(RtCtx* ctx, const RtSceneDesc* desc, const RtUploadOptions* options /* NULL = defaults */, RtScene** out_scene);

/* Number of floats rt_render writes: 3 * pixels covered by this shard's tiles. For
   shard_count <= 1 this is 3*width*height. */
int rt_output_floats(const RtParams* params, uint64_t* out_n);

/* Replaces the body of the pixel loops main.rs:731-784 (without write_color). Writes per-pixel
   RGB *sums* over the samples (what main.rs:772 accumulates), f32:
     - shard_count <= 1: rgb_sum[(y*width + x)*3 + c], row 0 = top of the image, i.e. the
       reference's j = height-1-y (main.rs:733);
     - sharded: this shard's tiles back to back, each tile_size*tile_size*3 floats row-major
       (pixels outside the image are 0); rt_untile() on the host puts gathered shards in place.
       Shards may differ by one tile; a gather uses equal buffers of shard 0's size
       (rt_output_floats with shard_index 0), which is what rt_untile expects.
   rt_render copies to a host buffer; rt_render_device leaves the result in device memory the
   caller owns (e.g. a torch tensor that RCCL then gathers). Both block until done. */
int rt_render(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* params,
              float* rgb_sum_host, RtStats* stats);
int rt_render_device(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* params,
                     void* rgb_sum_device, RtStats* stats);

/* ---- progressive rendering: a frame in resumable sample passes, with per-pixel second moments ----------------------------------------
 *
 * A PASS renders samples first_sample .. first_sample + params->samples_per_pixel - 1 of every pixel of the shard, into the layout
 * rt_render writes (full frame, or this shard's tiles back to back; rt_output_floats floats).
 *   - RT_PASS_ACCUMULATE unset: the pass overwrites the output buffer(s).
 *   - RT_PASS_ACCUMULATE set: the pass adds into them; its per-pixel fold starts from the value already there.
 *   - frame_samples = the samples per pixel the whole frame will have. It fixes how samples are grouped into work items (m samples per
 *     item, rt_pass_check), exactly as rt_render groups them for samples_per_pixel = frame_samples.
 * A sample's random stream is a pure function of (seed, pixel, ABSOLUTE sample index), and each pixel's sums are folded sequentially in
 * sample order in f32. Hence the guarantee: passes that cover [0, N) in order, all with frame_samples = N, the first without ACCUMULATE
 * and the rest with it, leave in the buffer EXACTLY (bit for bit) what rt_render with samples_per_pixel = N writes — in every layout
 * (sharded / tile-compact included) and with every RtParams flag, tail_paths, pool_slots and NaN policy rt_render accepts.
 * Constraints (anything else is RT_ERR_INVALID, with the reason in rt_last_error, and the output is left untouched):
 *   - first_sample is a multiple of m; the pass ends on a multiple of m or at frame_samples;
 *   - first_sample + samples_per_pixel <= frame_samples < 2^32;
 *   - struct_bytes >= sizeof(RtPassOptions) as this header declares it; no unknown bit in flags.
 *
 * Optional second output sq_sum (NULL = not wanted): the same layout and size as rgb_sum. Per pixel and channel it holds the sum of the
 * SQUARED item sums over the items folded so far, accumulated under the same rule (a series of passes gives the bits of one pass over
 * [0, N)). With m = 1 (the default below 2^32 - 2^28 samples per image) that is the sum of L^2 over the samples; with m > 1 it is the
 * batch-means second moment. With S = rgb_sum, Q = sq_sum and k = items folded (samples / m, rounded up), the standard error of the
 * pixel MEAN is
 *     SE = sqrt((Q - S^2 / k) / (k (k - 1))) / m.
 * Q - S^2/k cancels in f32 for near-constant pixels (a pixel that sees only the sky has a meaningless SE at the level of the rounding):
 * compute it in f64 and clamp it at 0.
 *
 * RtStats.samples counts the pass's samples. The host variant uploads the caller's sums before the fold when ACCUMULATE is set and
 * copies them back after it. Passes do not go through the collective entry points (rt_render_multi*, rt_render_gather): a one-process-
 * per-GPU caller accumulates its shard's passes with rt_render_pass_device and gathers once at the end (rt_untile_device). */
enum { RT_PASS_ACCUMULATE = 1u };
typedef struct RtPassOptions {
    uint32_t struct_bytes;    /* sizeof(RtPassOptions) as the caller compiled it (the struct may grow at its end) */
    uint32_t flags;           /* RT_PASS_*; an unknown bit is RT_ERR_INVALID */
    uint32_t first_sample;    /* first sample index of the pass (absolute) */
    uint32_t frame_samples;   /* samples per pixel of the whole frame, >= first_sample + params->samples_per_pixel */
} RtPassOptions;
/* Host only, no device: validates (params, options) and reports the samples per work item m of the frame. */
int rt_pass_check(const RtParams* params, const RtPassOptions* options, uint32_t* out_samples_per_item);
int rt_render_pass(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* params, const RtPassOptions* options,
                   float* rgb_sum_host, float* sq_sum_host /* NULL = not wanted */, RtStats* stats);
int rt_render_pass_device(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* params, const RtPassOptions* options,
                          void* rgb_sum_device, void* sq_sum_device /* NULL = not wanted */, RtStats* stats);

/* ---- adaptive sampling: passes over the pixels that are still noisy ---------------------------------------------------------------------
 *
 * OUTPUT SLOTS are the pixels of the rgb_sum layout: rt_output_floats / 3 of them (the full frame, slot = y * width + x; or this shard's
 * tiles back to back, slot = local tile * tile_size^2 + row-major position in the tile). Clipped pixels of edge tiles are slots too, but
 * never image pixels: they are never selected and never accepted in a list.
 * The caller owns a COUNTS buffer, one uint32_t per slot: the samples each pixel holds. Invariant: every pixel's rgb_sum / sq_sum equals,
 * bit for bit, what ONE rt_render_pass over [0, counts[p]) (same frame_samples) writes for that pixel. A frame starts with counts 0.
 *
 * rt_adaptive_select writes the ACTIVE LIST: the in-image slots p, ascending, with
 *     counts[p] == first_sample  (the pixel took every pass so far: a pixel that stopped never comes back),
 *     first_sample < frame_samples, and
 *     counts[p] < min_samples, or the pixel is not converged.
 * Converged, per channel, in f64 and in this order (m = samples per work item of the frame, k = counts / m rounded up):
 *     S = rgb_sum, Q = sq_sum;  var = max(Q - S*S/k, 0) / (k (k - 1));  tol = abs_error + rel_error * |S / counts|;  var / (m*m) <= tol*tol
 * (the standard error above, squared); a non-finite S or Q, or k < 2, is not converged. The list does not depend on any atomic ordering.
 *
 * rt_render_pass_pixels_device renders samples [first_sample, first_sample + spp) of the listed pixels only, under the RtPassOptions
 * rules of a pass (ACCUMULATE per listed pixel), sets counts[p] = first_sample + spp for them and leaves every other slot's rgb, sq and
 * count untouched (clipped slots included). Before anything is rendered a device kernel checks the list: every entry an in-image slot,
 * strictly ascending, counts[entry] == first_sample. A list that fails is RT_ERR_INVALID with the reason, and nothing is written.
 * n_pixels == 0 is a no-op. RtStats.samples = n_pixels * spp. The loop of a frame is: select, pass, select, pass, ... until the list is
 * empty, then rt_resolve_counts_device. Stopping on a pixel's own samples is a (small) bias: the invariant holds, an unbiased mean does not. */
typedef struct RtAdaptiveOptions {
    uint32_t struct_bytes;    /* sizeof(RtAdaptiveOptions) as the caller compiled it (the struct may grow at its end) */
    uint32_t min_samples;     /* every pixel takes at least this many samples; >= 2 m */
    double rel_error;         /* tolerance of the standard error relative to the pixel mean, >= 0 and finite */
    double abs_error;         /* absolute tolerance of the standard error, >= 0 and finite */
} RtAdaptiveOptions;
/* Host only, no device: validates (params, options, first_sample, frame_samples): first_sample on a work-item boundary, <= frame_samples. */
int rt_adaptive_check(const RtParams* params, const RtAdaptiveOptions* options, uint32_t first_sample, uint32_t frame_samples);
/* pixels_device_out: room for rt_output_floats / 3 entries; *n_out = the list's length. Blocks until done. A shard that owns no tile has
 * no slots: RT_OK, *n_out = 0, no buffer is read or written. */
int rt_adaptive_select(RtCtx* ctx, const RtParams* params, const RtAdaptiveOptions* options, uint32_t first_sample, uint32_t frame_samples,
                       const void* rgb_sum_device, const void* sq_sum_device, const void* counts_device, void* pixels_device_out, uint32_t* n_out);
int rt_render_pass_pixels_device(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* params, const RtPassOptions* options,
                                 const void* pixels_device, uint32_t n_pixels, void* rgb_sum_device, void* sq_sum_device /* NULL = not wanted */,
                                 void* counts_device, RtStats* stats);
/* write_color with every pixel's own count (full frame, width * height counts): spp = counts[p]; a count of 0 gives (0, 0, 0). */
int rt_resolve_counts_device(RtCtx* ctx, const void* rgb_sum_device, const void* counts_device, uint32_t width, uint32_t height, void* rgb8_device);

/* ---- denoising: non-local means over the sample variance ---------------------------------------------------------------------------------
 *
 * A filtered preview of a low-sample frame from nothing but what a pass already leaves: rgb_sum, sq_sum and the sample count (uniform, or
 * the adaptive COUNTS buffer). Non-local means with the patch distance normalised by the per-pixel variance of the mean (Rousselle, Knaus,
 * Zwicker 2012). Full frame, row-major, width x height; S = rgb_sum, Q = sq_sum, n_p = the pixel's samples, m = samples per work item
 * (rt_pass_check), k_p = n_p / m rounded up.
 * PREPARE, per pixel and channel, in f64, rounded to f32:  u = S / n_p;  v = max(Q - S^2 / k_p, 0) / (k_p (k_p - 1)) / m^2  (SE squared).
 * A pixel is INVALID when n_p == 0, k_p < 2, or one of its S, Q is not finite.
 * FILTER, with window radius r, patch radius f, strength k, variance cancellation alpha and eps; for a valid pixel p and every VALID q of
 * the image with |q - p|_inf <= r:
 *     t      = ((u[p+o] - u[q+o])^2 - alpha (v[p+o] + min(v[p+o], v[q+o]))) / (eps + k^2 (v[p+o] + v[q+o]))
 *     d(p,q) = the mean of t over the patch offsets |o|_inf <= f whose p+o and q+o are both valid image pixels, and the three channels
 *     w(p,q) = exp(-max(d, 0))                    (w(p,p) = 1)
 *     out[p] = sum_q w(p,q) u[q] / sum_q w(p,q)   per channel
 * An invalid pixel is copied through (out = u, or 0 with no sample) and is nobody's neighbour. The filter step runs in f32.
 * mean_out: width * height * 3 floats, the MEAN radiance (not sums), device memory the caller owns, not one of the inputs; the inputs are
 * never written. RGB8 of it: rt_resolve_device with samples_per_pixel = 1.
 * A field left 0 takes its default: window_radius 10, patch_radius 3, strength 0.45, alpha 1, eps 1e-10 (the paper's values), so a
 * negative or non-finite strength / alpha / eps is RT_ERR_INVALID. Caps: window_radius <= 16, patch_radius <= 4 — a workgroup stages its
 * 32 x 32 tile plus an (r + f) halo of u and v in LDS (72 x 72 x 24 B = 122 KiB at the caps, plus 22 KiB of box-sum buffers, of 160 KiB).
 * The result does not depend on the launch shape and is the same bits on every call. */
#define RT_DENOISE_MAX_WINDOW_RADIUS 16
#define RT_DENOISE_MAX_PATCH_RADIUS 4
typedef struct RtDenoiseOptions {
    uint32_t struct_bytes;      /* sizeof(RtDenoiseOptions) as the caller compiled it (the struct may grow at its end) */
    uint32_t window_radius;     /* r; 0 = 10 */
    uint32_t patch_radius;      /* f; 0 = 3 */
    uint32_t samples_per_item;  /* m of the frame the sums belong to (rt_pass_check); 0 = 1 */
    double strength;            /* k; 0 = 0.45 */
    double alpha;               /* 0 = 1 */
    double eps;                 /* 0 = 1e-10 */
} RtDenoiseOptions;
/* Host only, no device: validates (width, height, options; NULL = defaults) and reports the reason through rt_last_error. */
int rt_denoise_check(uint32_t width, uint32_t height, const RtDenoiseOptions* options);
/* samples: every pixel's count when counts_device is NULL (>= 1); else counts_device holds width * height uint32_t. Two kernels on the
   context's stream; blocks until done. A refused call writes nothing. */
int rt_denoise_device(RtCtx* ctx, const RtDenoiseOptions* options /* NULL = defaults */, uint32_t width, uint32_t height, const void* rgb_sum_device,
                      const void* sq_sum_device, uint32_t samples, const void* counts_device /* NULL = uniform `samples` */, void* mean_out_device);

/* ---- denoising, guided: the same filter with its weights joined with first-hit features ----------------------------------------------------
 *
 * rt_denoise_device's inputs plus full-frame feature planes as rt_render_features_device writes them with shard_count <= 1: albedo_sum and
 * normal_sum (3 f32 per pixel), depth_sum (1 f32), hits (1 u32), folded over feature_samples = n_f >= 1 samples per pixel (uniform,
 * independent of the radiance counts). The sample variance cannot tell a noisy pixel from a texture or geometry edge at low counts; the
 * features, nearly noise-free, can.
 * COLOUR PART: u, v, validity and the patch distance d(p,q) are exactly those above; PREPARE and FILTER do not change.
 * GUIDE, per pixel, computed in f64, rounded to f32, then to IEEE binary16 (round to nearest even) and clamped to +-65504; h = hits:
 *     A_c = albedo_sum_c / n_f / sigma_albedo        c = 0..2
 *     N_c = normal_sum_c / n_f / sigma_normal        c = 0..2; over ALL samples, not over the hits: a pixel partly on the background has
 *                                                    a shorter mean normal, so coverage is part of the guide
 *     Z   = ln(max(depth_sum / h, 1e-30)) / sigma_depth   when h > 0, else 0 (log depth: a plain difference is a relative depth difference)
 *     g(p,q) = the sum over the 7 components of (F_p - F_q)^2, formed in f32 from the binary16 values; pointwise, no patch
 *     w(p,q) = exp(-(max(d(p,q), 0) + g(p,q)))       (w(p,p) = 1)
 *     out[p] = sum_q w(p,q) u[q] / sum_q w(p,q)      accumulated as differences from u[p]: a constant frame returns bit for bit
 * A plane pointer that is NULL makes its components 0. depth_sum requires hits. All three guide planes NULL is RT_ERR_INVALID (that
 * filter is rt_denoise_device). A pixel is additionally INVALID when one of its feature sums is not finite or hits > n_f; invalid pixels
 * behave as above: copied through, nobody's neighbour, no patch tap.
 * Sigmas: a field left 0 takes its default (sigma_albedo 0.2, sigma_normal 0.5, sigma_depth 0.2: the best triple of the grid measured in
 * DESIGN.md §10); a negative, NaN, infinite or -0.0 value, or one whose f32 reciprocal is not finite and positive, is RT_ERR_INVALID.
 * Caps: patch_radius <= 4 as above; window_radius <= RT_DENOISE_GUIDED_MAX_WINDOW_RADIUS = 10, refused above: the guide records of the
 * tile plus an r halo are staged in LDS beside the colour planes (at r 10, f 4: 60 x 60 x 24 B + 52 x 52 x 16 B + 23,040 B of box-sum
 * buffers = 152,704 B of 163,840 B), and the binary16 records are what makes them fit.
 * Determinism: the result is a function of the inputs and options alone — not of where tiles fall or of the call count; no atomics, every
 * pixel folds in one fixed order. mean_out must not be one of the inputs, the feature planes included; the inputs are never written. */
#define RT_DENOISE_GUIDED_MAX_WINDOW_RADIUS 10
typedef struct RtDenoiseGuide {
    uint32_t struct_bytes;      /* sizeof(RtDenoiseGuide) as the caller compiled it (the struct may grow at its end) */
    uint32_t feature_samples;   /* n_f >= 1: the samples per pixel the planes were folded over */
    const void* albedo_sum;     /* device, width * height * 3 f32; NULL = not used */
    const void* normal_sum;     /* device, width * height * 3 f32; NULL = not used */
    const void* depth_sum;      /* device, width * height f32; NULL = not used; needs hits */
    const void* hits;           /* device, width * height u32; NULL = none */
    double sigma_albedo;        /* 0 = 0.2 */
    double sigma_normal;        /* 0 = 0.5 */
    double sigma_depth;         /* 0 = 0.2 */
} RtDenoiseGuide;
/* Host only, no device: validates (width, height, options; NULL = defaults, guide) and reports the reason through rt_last_error. The plane
   pointers are only tested against NULL. */
int rt_denoise_guided_check(uint32_t width, uint32_t height, const RtDenoiseOptions* options, const RtDenoiseGuide* guide);
/* Three kernels on the context's stream; blocks until done. A refused call writes nothing. */
int rt_denoise_guided_device(RtCtx* ctx, const RtDenoiseOptions* options /* NULL = defaults */, const RtDenoiseGuide* guide, uint32_t width, uint32_t height,
                             const void* rgb_sum_device, const void* sq_sum_device, uint32_t samples, const void* counts_device /* NULL = uniform `samples` */,
                             void* mean_out_device);

/* ---- denoising, guided with feature variances: g(p,q) variance-cancelled and variance-normalised ----------------------------------------------
 *
 * rt_denoise_guided_device's inputs plus the SQUARED sums of the features as rt_render_feature_moments_device writes them with
 * shard_count <= 1: albedo_sq_sum and normal_sq_sum (3 f32 per pixel), depth_sq_sum (1 f32), over the same n_f >= 2 samples. At a few
 * samples per pixel the features are themselves noisy where a pixel sees several surfaces (small spheres, silhouettes, light edges); the
 * plain squared distance of the guided filter then separates pixels the patch distance would rightly average. Here the feature distance
 * takes the form the colour distance already has (Rousselle, Knaus, Zwicker 2012, 2013): the expected squared difference of two noisy
 * means is subtracted, and what is left is damped where the features are uncertain.
 * COLOUR PART: u, v, validity and the patch distance d(p,q) are exactly those of rt_denoise_device.
 * GUIDE, per pixel, in f64; h = hits, S a sum, Q its squared sum:
 *     var(S, Q) = max(Q - S^2 / n_f, 0) / (n_f (n_f - 1))          the variance of the mean over ALL n_f samples
 *     a_c = albedo_sum_c / n_f     n_c = normal_sum_c / n_f     md = max(depth_sum / h, 1e-30)     z = ln(md) when h > 0, else 0
 *     VA = sum_c var(albedo_sum_c, albedo_sq_sum_c)     VN = sum_c var(normal_sum_c, normal_sq_sum_c)
 *     VZ = var(depth_sum, depth_sq_sum) (n_f / h)^2 / md^2 when h > 0, else 0       the delta method on the log; over all samples, so partial
 *                                                                                   coverage inflates it and the guide weakens on silhouettes
 *   The record holds TEN components, each over its group's sigma: A_c = a_c / sigma_albedo, N_c = n_c / sigma_normal, Z = z / sigma_depth and
 *   the standard errors sA = sqrt(VA) / sigma_albedo, sN = sqrt(VN) / sigma_normal, sZ = sqrt(VZ) / sigma_depth (roots: a variance of 1e-8
 *   is below binary16's range, its root is not). Each goes f64 -> f32 -> binary16 (round to nearest even), clamped to +-65504.
 * FILTER, in f32 from the binary16 values, with V_j = s_j^2 and kappa = variance_strength:
 *     g(p,q) = sum over j in {A, N, Z} of  max(|F_j,p - F_j,q|^2 - (V_j,p + min(V_j,p, V_j,q)), 0) / (1 + kappa (V_j,p + V_j,q))
 *     w(p,q) = exp(-(max(d(p,q), 0) + g(p,q)))       (w(p,p) = 1)     |.|^2 over the group's components
 *     out[p] = sum_q w(p,q) u[q] / sum_q w(p,q)      accumulated as differences from u[p]: a constant frame returns bit for bit
 * A sum plane that is NULL zeroes its group (components and variance); a squared plane that is NULL zeroes its group's variance — with all
 * three NULL, g is rt_denoise_guided_device's. depth_sum requires hits. All three sum planes NULL is RT_ERR_INVALID. A pixel is
 * additionally INVALID when a given feature sum or squared sum is not finite or hits > n_f; invalid pixels behave as above.
 * Defaults: a field left 0 takes its default — sigma_albedo 0.01, sigma_normal 0.025, sigma_depth 0.01, variance_strength 64: the best point
 * of the grid measured in DESIGN.md §10 (scripts/cpu_guided_moments.py) — and a negative, NaN, infinite or -0.0 value, a sigma whose f32
 * reciprocal is not finite and positive, or a variance_strength that is not finite in f32 is RT_ERR_INVALID. feature_samples < 2 is
 * RT_ERR_INVALID (no variance).
 * Caps: patch_radius <= 4; window_radius <= RT_DENOISE_GUIDED_MOMENTS_MAX_WINDOW_RADIUS = 8, refused above, and for THIS entry point
 * window_radius 0 means 8: per pixel of the tile plus an r halo the LDS holds the 16-byte record and an 8-byte one (sA, sN, sZ, 0) beside
 * the colour planes (at r 8, f 4: 56 x 56 x 24 B + 48 x 48 x 24 B + 23,040 B = 153,600 B of 163,840 B; r 9 does not fit).
 * Determinism and aliasing: as rt_denoise_guided_device — a function of the inputs and options alone; mean_out must not be one of the
 * inputs (rgb_sum, sq_sum, counts, the four sum planes, hits among them, and the three squared planes); the inputs are never written. */
#define RT_DENOISE_GUIDED_MOMENTS_MAX_WINDOW_RADIUS 8
#define RT_DENOISE_MOMENTS_SIGMA_ALBEDO 0.01
#define RT_DENOISE_MOMENTS_SIGMA_NORMAL 0.025
#define RT_DENOISE_MOMENTS_SIGMA_DEPTH 0.01
#define RT_DENOISE_MOMENTS_VARIANCE_STRENGTH 64.0
typedef struct RtDenoiseGuideMoments {
    uint32_t struct_bytes;      /* sizeof(RtDenoiseGuideMoments) as the caller compiled it (the struct may grow at its end) */
    uint32_t feature_samples;   /* n_f >= 2: the samples per pixel the planes were folded over */
    const void* albedo_sum;     /* device, width * height * 3 f32; NULL = not used */
    const void* normal_sum;     /* device, width * height * 3 f32; NULL = not used */
    const void* depth_sum;      /* device, width * height f32; NULL = not used; needs hits */
    const void* hits;           /* device, width * height u32; NULL = none */
    const void* albedo_sq_sum;  /* device, width * height * 3 f32; NULL = variance 0 */
    const void* normal_sq_sum;  /* device, width * height * 3 f32; NULL = variance 0 */
    const void* depth_sq_sum;   /* device, width * height f32; NULL = variance 0 */
    double sigma_albedo;        /* 0 = RT_DENOISE_MOMENTS_SIGMA_ALBEDO */
    double sigma_normal;        /* 0 = RT_DENOISE_MOMENTS_SIGMA_NORMAL */
    double sigma_depth;         /* 0 = RT_DENOISE_MOMENTS_SIGMA_DEPTH */
    double variance_strength;   /* kappa; 0 = RT_DENOISE_MOMENTS_VARIANCE_STRENGTH */
} RtDenoiseGuideMoments;
/* Host only, no device: validates (width, height, options; NULL = defaults, guide) and reports the reason through rt_last_error. The plane
   pointers are only tested against NULL. */
int rt_denoise_guided_moments_check(uint32_t width, uint32_t height, const RtDenoiseOptions* options, const RtDenoiseGuideMoments* guide);
/* Three kernels on the context's stream; blocks until done. A refused call writes nothing. */
int rt_denoise_guided_moments_device(RtCtx* ctx, const RtDenoiseOptions* options /* NULL = defaults */, const RtDenoiseGuideMoments* guide, uint32_t width,
                                     uint32_t height, const void* rgb_sum_device, const void* sq_sum_device, uint32_t samples,
                                     const void* counts_device /* NULL = uniform `samples` */, void* mean_out_device);

/* ---- ray queries: the closest hit of caller-supplied rays ----------------------------------------------------------------------------------
 *
 * hits[i] is the HitRecord that `world.hit(ray_i, 0.001, inf)` returns (main.rs:74, hittable.rs:11-19) for the uploaded scene: t, p, the
 * normal after set_face_normal and the replay of the Translate / RotateY / FlipFace wrappers above the primitive, u, v and front_face. The
 * rays go through the traversal kernels a render uses, in the layout the scene was uploaded with (every RT_LAYOUT_* answers queries).
 *   - t_min is the renderer's 0.001 and cannot be chosen. A closest hit beyond the ray's t_max is a MISS (t_max <= 0, +inf or NaN: no limit).
 *   - u, v are always computed (a render computes them for textured scenes only): sphere.rs:32-37, aarect.rs:41-42, barycentrics for a
 *     triangle, 0 for a moving sphere (moving_sphere.rs leaves them unset).
 *   - Triangles are closed: a ray through an edge or a vertex that triangles share — straight down onto a vertex of a grid-aligned mesh,
 *     or running in a plane that holds mesh edges — hits one of them, never the gap f32 barycentrics would leave between them. A
 *     barycentric outside [0, 1] by no more than its own rounding error (a few ulps of 1 for a ray that meets the triangle squarely,
 *     at most 2^-10) counts as inside, and u, v are reported on the edge. Which of the triangles reports the hit is the walk's choice.
 *   - a MISS is t = +inf, hittable = material = -1, flags = 0, every other field 0.
 *   - material: index into RtSceneDesc.materials. hittable: index of the primitive's own RtHittable record — for a side of a Box the
 *     Box's record, never a wrapper, a list or a BVH.
 *   - Rays are f32 and live in device memory for the *_device variant (n_rays records of 32 bytes, 16-byte aligned; hits: 48 bytes each,
 *     16-byte aligned). The device path computes in f32; an f32 ray is exact in the f64 of the reference.
 *   - INVALID rays never reach a traversal kernel: the kernel that reads the caller's rays drops them, and their hit is a miss with
 *     RT_RAYHIT_INVALID_RAY set. Invalid is: a non-finite origin, direction or time; or a direction whose squared length |d|^2, formed in
 *     f32, is not a positive normal number — the zero direction, and directions so short or so long that |d|^2 underflows (|d| below
 *     about 1.1e-19) or overflows (|d| above about 1.8e19), for which the walk's 1 / |d|^2 would be inf or 0.
 *   - A scene that holds a ConstantMedium is RT_ERR_UNSUPPORTED and nothing is written: a medium's hit is a random draw keyed by (path,
 *     segment, medium) and a bare ray has no path. A deliberate limit. Every query ray starts on nothing (there is no "the primitive this
 *     ray leaves" input) and there is no multi-GPU entry point. "Is anything hit at all?" is rt_occluded_rays below.
 *   - Options: an unknown bit in flags (known: RT_FLAG_TIMING), struct_bytes < sizeof(RtRayQueryOptions) or n_rays >= 2^32 is
 *     RT_ERR_INVALID with the reason in rt_last_error, and nothing is written. n_rays == 0 is a no-op. pool_slots caps the rays in flight
 *     (0 = the renderer's rule: all of them, up to 2^28 and to 70 % of the free device memory); longer lists run in chunks.
 *   - Determinism: hits[i] is a function of (scene, layout, ray i) alone — not of the chunk size, of the ray's place in the list, or of
 *     the host / device variant — and the same call gives the same bytes every time.
 *   - RtStats: samples = segments = n_rays minus the invalid ones; render_ms; with RT_FLAG_TIMING also extend_ms (the traversal kernels)
 *     and other_ms (the two kernels that read the rays and write the hits). Both variants block until done. */
typedef struct RtRay    { float o[3]; float time; float d[3]; float t_max; } RtRay;       /* 32 B; t_max <= 0 or +inf = no limit */
typedef struct RtRayHit { float t; int32_t hittable; int32_t material; uint32_t flags;    /* 48 B */
                          float p[3]; float u; float n[3]; float v; } RtRayHit;
enum { RT_RAYHIT_HIT = 1u, RT_RAYHIT_FRONT_FACE = 2u, RT_RAYHIT_INVALID_RAY = 4u };
typedef struct RtRayQueryOptions {
    uint32_t struct_bytes;    /* sizeof(RtRayQueryOptions) as the caller compiled it (the struct may grow at its end) */
    uint32_t flags;           /* RT_FLAG_TIMING; an unknown bit is RT_ERR_INVALID */
    uint32_t pool_slots;      /* rays in flight; 0 = default */
    uint32_t _pad;
} RtRayQueryOptions;
/* Host only, no device: validates (options, n_rays) and reports the reason through rt_last_error. */
int rt_ray_query_check(const RtRayQueryOptions* options /* NULL = defaults */, uint64_t n_rays);
int rt_trace_rays_device(RtCtx* ctx, const RtScene* scene, const RtRayQueryOptions* options /* NULL = defaults */, const void* rays_device, uint64_t n_rays,
                         void* hits_device, RtStats* stats);
int rt_trace_rays(RtCtx* ctx, const RtScene* scene, const RtRayQueryOptions* options /* NULL = defaults */, const RtRay* rays_host, uint64_t n_rays,
                  RtRayHit* hits_host, RtStats* stats);

/* ---- occlusion queries: any-hit rays that stop at the first blocker -------------------------------------------------------------------------
 *
 * One byte per ray: occluded[i] is RT_RAYHIT_HIT (1) when some primitive of the scene is hit at a t with 0.001 <= t <= t_max, both ends
 * inclusive as in the primitive tests, and 0 otherwise — shadow rays, ambient occlusion, line of sight, visibility baking. The answer:
 * occluded[i] == RT_RAYHIT_HIT exactly when rt_trace_rays on the same scene and layout reports a hit for ray i. What it saves is work:
 * the walk starts with the ray's own t_max as its interval, so boxes beyond the target are culled from the first node on; it stops at
 * the first primitive it accepts; and no HitRecord is rebuilt or written.
 *   - The rays are the RtRay records of rt_trace_rays (32 bytes; 16-byte aligned in device memory for the *_device variant); the output is
 *     n_rays bytes and needs no alignment. t_max <= 0, +inf or NaN means no limit; t_min stays the renderer's 0.001.
 *   - An INVALID ray — the rule is rt_trace_rays' own: a non-finite origin, direction or time, or |d|^2 not a positive normal f32 — is never
 *     traced and gets RT_RAYHIT_INVALID_RAY (4). No other bit is ever set.
 *   - RtRayQueryOptions is read as rt_trace_rays reads it and rt_ray_query_check validates it: an unknown bit in flags (known:
 *     RT_FLAG_TIMING), a short struct_bytes, n_rays >= 2^32, or a NULL rays or output pointer with n_rays > 0 is RT_ERR_INVALID with the
 *     reason in rt_last_error, and nothing is written. n_rays == 0 is a no-op. pool_slots and chunking follow rt_trace_rays' pool rule.
 *   - A scene that holds a ConstantMedium is RT_ERR_UNSUPPORTED and nothing is written: the limit of rt_trace_rays, for its reason. Every
 *     query ray starts on nothing; there is no multi-GPU entry point.
 *   - Every RT_LAYOUT_* answers. A scene uploaded with RT_LAYOUT_WIDE_NODES is answered through its closest-hit 8-wide walk: the same
 *     bytes, without the early exit (that walk is the measured-slower option and has no any-hit version).
 *   - Determinism: occluded[i] is a function of (scene, layout, ray i) alone — not of the chunk size, of the ray's place in the list, or of
 *     the host / device variant — and the same call gives the same bytes every time.
 *   - RtStats: samples = segments = n_rays minus the invalid ones; render_ms; with RT_FLAG_TIMING also extend_ms (the traversal kernels)
 *     and other_ms (the two kernels that read the rays and write the bytes). Both variants block until done. */
int rt_occluded_rays_device(RtCtx* ctx, const RtScene* scene, const RtRayQueryOptions* options /* NULL = defaults */, const void* rays_device, uint64_t n_rays,
                            void* occluded_device /* n_rays bytes */, RtStats* stats);
int rt_occluded_rays(RtCtx* ctx, const RtScene* scene, const RtRayQueryOptions* options /* NULL = defaults */, const RtRay* rays_host, uint64_t n_rays,
                     uint8_t* occluded_host, RtStats* stats);

/* ---- light-sample queries: the scene's own light sampler, query by query -------------------------------------------------------------------
 *
 * What a host that does its own direct lighting needs beside rt_occluded_rays: the directions of its shadow rays drawn from the scene's
 * lights list, and their pdf. results[i] is what the Lambertian branch of a render computes for its light half at the point p, by the same
 * device functions (not a restatement):
 *   - the device seeds the path generator with (rng_state, 0 draws); ONE pick k = next64() % n_lights (hittable_list.rs:81-84), then the
 *     picked member's `random` from p (RtSceneDesc.scene_flags has the draw orders): d = the direction (not normalised: the vector from p
 *     to the sampled point for a rect, triangle or box), light = k, n_draws = the draws consumed (pick included);
 *   - pdf = the list's pdf_value at (p, d): the mean over ALL members of each member's pdf (hittable_list.rs:73-80), 0 for a member the
 *     ray misses. Occlusion is not looked at.
 *   - RT_LIGHTQ_DIRECTION_GIVEN in a query's flags: nothing is drawn; pdf is evaluated for the caller's d, light = -1, n_draws = 0 and d
 *     is copied through. For the d of a drawn result this returns the drawn result's pdf, bit for bit.
 * Works with RT_SCENE_LIGHTS_ALL_SHAPES set or clear (clear: the reference's kinds, LK_DEFAULT members included). A scene with lights = -1
 * is RT_ERR_UNSUPPORTED. An unknown bit in RtLightQueryOptions.flags (known: RT_FLAG_TIMING), struct_bytes < sizeof(RtLightQueryOptions),
 * n >= 2^32, or a NULL queries / results pointer with n > 0 is RT_ERR_INVALID; device buffers must be 8-byte aligned; a refused call
 * writes nothing. n == 0 is a no-op. An unknown bit in a QUERY's flags is ignored.
 * RT_SCENE_LIGHTS_MANY scenes: the pick is the area-weighted one (ONE rnd() draw, RtSceneDesc.scene_flags has the rule) and pdf is the
 * weighted sum, evaluated through the light tree. RT_LIGHTQ_LINEAR in a query's flags: the pdf is evaluated by the plain loop over the
 * table instead, same order, same weights, no boxes; the two agree bit for bit unless a box culled a member the loop counts, which is
 * a bug. In any other scene the bit changes nothing. One kernel on the context's stream, one lane per
 * query, no pool; results[i] is a function of (scene, query i) alone. RtStats: samples = n; render_ms; with RT_FLAG_TIMING other_ms =
 * the kernel. Both variants block until done. */
enum { RT_LIGHTQ_DIRECTION_GIVEN = 1u, RT_LIGHTQ_LINEAR = 2u };
typedef struct RtLightQuery  { float p[3]; uint32_t flags; uint64_t rng_state; float d[3]; float _pad; } RtLightQuery;      /* 40 B */
typedef struct RtLightSample { float d[3]; float pdf; int32_t light; uint32_t n_draws; } RtLightSample;                      /* 24 B */
typedef struct RtLightQueryOptions {
    uint32_t struct_bytes;    /* sizeof(RtLightQueryOptions) as the caller compiled it (the struct may grow at its end) */
    uint32_t flags;           /* RT_FLAG_TIMING; an unknown bit is RT_ERR_INVALID */
} RtLightQueryOptions;
int rt_sample_lights_device(RtCtx* ctx, const RtScene* scene, const RtLightQueryOptions* options /* NULL = defaults */, const void* queries_device, uint64_t n,
                            void* results_device, RtStats* stats);
int rt_sample_lights(RtCtx* ctx, const RtScene* scene, const RtLightQueryOptions* options /* NULL = defaults */, const RtLightQuery* queries_host, uint64_t n,
                     RtLightSample* results_host, RtStats* stats);

/* ---- radiance queries: the path tracer itself on caller-supplied rays -----------------------------------------------------------------------
 *
 * What the other queries leave out: the radiance along a caller's own ray — a host's own camera model (fisheye, panorama, orthographic,
 * stereo, lens distortion), light probes, lightmap texels, the secondary rays of a hybrid integrator. Ray i of the list is traced S =
 * `samples` times; rgb_sum[3 i + c] receives the sum of the S samples.
 *   - SAMPLE RULE. Sample s of ray i is what ray_color (main.rs:63-139, in the scene's integrator mode) returns for the ray (o, d, time), which
 *     starts on nothing, as every query ray does. Its random stream is path_base(seed, first_stream + i, first_sample + s) — the stream a
 *     render gives sample first_sample + s of the pixel with index first_stream + i — ADVANCED BY first_draw DRAWS. first_draw is 0 for an
 *     ordinary caller; a caller who made the ray from the first draws of that very stream (as a render's camera does: jitter, lens, time)
 *     passes how many it spent, and the path goes on where it stopped. The path runs through the kernels and device functions of a render
 *     (the wavefront loop, the drain, the fold); it is not a restatement of them.
 *   - OUTPUTS. rgb_sum: 3 f32 per ray, the sum over the S samples, folded sequentially in sample order in f32 from 0 — or, under
 *     RT_RADIANCE_ACCUMULATE, from the value already there. sq_sum (NULL = not wanted): the same for the squares of the samples, formed in
 *     f32 (x * x, rounded, then added). The standard-error formula of rt_render_pass applies with m = 1 and k = the samples folded so far.
 *     invalid (NULL = not wanted): one byte per ray, RT_RAYHIT_INVALID_RAY for an invalid ray and 0 for every other.
 *   - GUARANTEES, bit for bit. out[i] is a function of (scene, layout, ray i, its stream index first_stream + i, seed, the sample range,
 *     max_depth, nan_policy) alone: not of pool_slots, tail_paths, the chunking, or the host / device variant; not of how a list is split
 *     over calls (rays [a, b) with first_stream = f + a give the bits the same rays get inside a call over [0, n) with first_stream = f);
 *     not of how a sample range is split ([0, k) and then [k, S) accumulating give one call's bits). Hence a caller shards a list over GPUs
 *     itself: there is no multi-GPU entry point.
 *   - INVALID rays: rt_trace_rays' rule (a non-finite origin, direction or time, or |d|^2 not a positive normal f32), and first_draw >= 2^16.
 *     They are never traced; their sums are 0, or untouched under RT_RADIANCE_ACCUMULATE.
 *   - SCENES. Every scene a render accepts: a ConstantMedium included (a path has a stream, which the bare ray of rt_trace_rays lacks),
 *     lights lists, RT_SCENE_LIGHTS_*, triangle attributes, every RT_LAYOUT_*. In a motionless scene the time is read by nothing, as in a
 *     render (it must still be finite).
 *   - OPTIONS are required. max_depth 1..255, nan_policy, seed, pool_slots and tail_paths mean what they mean in RtParams; pool_slots caps
 *     the paths in flight (0 = the renderer's rule), and a call of more (ray, sample) pairs runs in chunks — over rays first, then samples.
 *   - REFUSED with RT_ERR_INVALID and the reason in rt_last_error, nothing written: NULL options; struct_bytes < sizeof(RtRadianceOptions);
 *     an unknown bit in flags or in render_flags (known there: RT_FLAG_TIMING; no counters); a bad nan_policy or max_depth; samples == 0;
 *     first_sample + samples >= 2^32; first_stream + n_rays > 2^32 - 1 (a stream index is 32 bits: the exact limit — so up to 2^32 - 1 rays
 *     per call from first_stream 0); a NULL rays or rgb_sum with n_rays > 0; for the device variant rays, rgb_sum or sq_sum not 16-byte
 *     aligned (invalid needs no alignment). n_rays == 0 is a no-op.
 *   - RtStats: samples = valid rays x S; segments, render_ms, iterations, pool_slots and drain_paths as for a render; with RT_FLAG_TIMING
 *     also extend_ms, shade_ms, drain_ms and other_ms (the kernel that reads the rays, and the fold). Both variants block until done; the
 *     host variant stages rays and sums through the context's buffers (uploading the caller's sums first when accumulating). */
typedef struct RtPathRay { float o[3]; float time; float d[3]; uint32_t first_draw; } RtPathRay;   /* 32 B: RtRay with t_max's word = first_draw */
enum { RT_RADIANCE_ACCUMULATE = 1u };
typedef struct RtRadianceOptions {
    uint32_t struct_bytes;    /* sizeof(RtRadianceOptions) as the caller compiled it (the struct may grow at its end) */
    uint32_t flags;           /* RT_RADIANCE_*; an unknown bit is RT_ERR_INVALID */
    uint32_t render_flags;    /* RT_FLAG_TIMING only; any other bit is RT_ERR_INVALID */
    uint32_t nan_policy;      /* RtNanPolicy */
    uint32_t samples;         /* S >= 1 samples per ray ... */
    uint32_t first_sample;    /* ... with the absolute indices first_sample .. first_sample + S - 1 */
    uint32_t max_depth;       /* as RtParams */
    uint32_t pool_slots;      /* as RtParams */
    uint64_t seed;            /* as RtParams */
    uint64_t first_stream;    /* ray i runs on stream first_stream + i */
    uint32_t tail_paths;      /* as RtParams.tail_paths */
    uint32_t _pad;
} RtRadianceOptions;
/* Host only, no device: validates (options, n_rays) and reports the reason through rt_last_error. */
int rt_radiance_check(const RtRadianceOptions* options, uint64_t n_rays);
int rt_radiance_rays_device(RtCtx* ctx, const RtScene* scene, const RtRadianceOptions* options, const void* rays_device, uint64_t n_rays,
                            void* rgb_sum_device, void* sq_sum_device /* NULL = not wanted */, void* invalid_device /* n_rays bytes; NULL = not wanted */,
                            RtStats* stats);
int rt_radiance_rays(RtCtx* ctx, const RtScene* scene, const RtRadianceOptions* options, const RtPathRay* rays_host, uint64_t n_rays,
                     float* rgb_sum_host, float* sq_sum_host /* NULL = not wanted */, uint8_t* invalid_host /* NULL = not wanted */, RtStats* stats);

/* ---- first-hit features: albedo, normal and depth of the render's own camera rays ----------------------------------------------------------
 *
 * What a feature-guided filter or an external denoiser starts from: per-pixel SUMS, over a range of samples, of the first hit's colour,
 * normal and distance, for exactly the primary rays a render of the same (scene, camera, params) traces.
 *   - WHICH RAYS. For every output slot of the rgb_sum layout (the full frame, or this shard's tiles back to back: tile_size, shard_index
 *     and shard_count are honoured; clipped slots of edge tiles are never written) and every sample s of
 *     [first_sample, first_sample + params->samples_per_pixel): the primary ray the render traces for (seed, pixel, s) — the device function
 *     a render calls, with the same draws in the same order from the path's stream (jitter, lens offset, time). Not a restatement of it.
 *   - PER SAMPLE, from world.hit(ray, 0.001, inf) (main.rs:74):
 *       albedo  the first hit's colour: texture.value(u, v, p) for a Lambertian, albedo for a Metal, (1, 1, 1) for a Dielectric; for a
 *               DiffuseLight what `emitted` returns toward this ray (its colour on the front face, 0 on the back); on a miss the
 *               background radiance of the ray (constant, or the sky gradient);
 *       normal  the HitRecord normal as rt_trace_rays reports it: world space, after set_face_normal and the wrapper replay; 0 on a miss;
 *       depth   t * |d| in f32; 0 on a miss;
 *       hits    1 when the ray hit something.
 *   - FOLDING. Every plane holds per-slot sums, folded sequentially in sample order in f32 (hits: u32) from 0 — or, under
 *     RT_FEATURES_ACCUMULATE, from the value already in the plane. Hence passes over [0, a) and [a, N), the second accumulating, leave the
 *     bits of one pass over [0, N). No float atomics: a slot's result is a function of (scene, layout, camera, seed, width, height, pixel,
 *     sample range) alone — not of pool_slots, the chunking, the shard the pixel fell in or the call count.
 *   - Means are the caller's: albedo_sum / samples; normal_sum and depth_sum over `hits` (a miss adds 0 to both).
 *   - RtParams: max_depth and nan_policy are not read. Of flags, RT_FLAG_TIMING is honoured, RT_FLAG_SAMPLE_BLOCKS is accepted without
 *     effect (features fold per sample), RT_FLAG_COUNTERS and RT_FLAG_FUSED are RT_ERR_INVALID. RtParams.pool_slots is not read
 *     (RtFeatureOptions.pool_slots caps the rays in flight; 0 = the renderer's rule, as for ray queries; longer passes run in chunks).
 *   - REFUSED, with the reason in rt_last_error and nothing written: params rt_render refuses; struct_bytes < sizeof(RtFeatureOptions); an
 *     unknown bit in flags; first_sample + samples_per_pixel >= 2^32; all four pointers NULL; a pointer that is not 16-byte aligned. A scene
 *     that holds a ConstantMedium is RT_ERR_UNSUPPORTED: the limit of ray queries, and as deliberate. No pixel-list variant, no multi-GPU
 *     entry point, no host-memory variant (callers copy the planes).
 *   - RtStats: samples = segments = rays traced; render_ms; with RT_FLAG_TIMING also extend_ms (the traversal kernels) and other_ms (the
 *     kernels that make the rays, write the per-ray records and fold them; debug[0], [1], [2]: the three of them apart, in microseconds).
 *     The call blocks until done. */
enum { RT_FEATURES_ACCUMULATE = 1u };
typedef struct RtFeatureOptions {
    uint32_t struct_bytes;    /* sizeof(RtFeatureOptions) as the caller compiled it (the struct may grow at its end) */
    uint32_t flags;           /* RT_FEATURES_ACCUMULATE; an unknown bit is RT_ERR_INVALID */
    uint32_t first_sample;    /* absolute index of the first sample of this pass */
    uint32_t pool_slots;      /* rays in flight; 0 = the renderer's rule */
} RtFeatureOptions;
typedef struct RtFeatureBuffers {   /* device memory the caller owns; any pointer may be NULL = not wanted; 16-byte aligned */
    void* albedo_sum;         /* 3 f32 per output slot, the layout of rgb_sum (rt_output_floats floats) */
    void* normal_sum;         /* 3 f32 per slot */
    void* depth_sum;          /* 1 f32 per slot */
    void* hits;               /* 1 u32 per slot: samples of the pass range whose primary ray hit something */
} RtFeatureBuffers;
/* Host only, no device: validates (params, options) and reports the reason through rt_last_error. */
int rt_features_check(const RtParams* params, const RtFeatureOptions* options);
int rt_render_features_device(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* params, const RtFeatureOptions* options,
                              const RtFeatureBuffers* buffers, RtStats* stats);

/* ---- first-hit features, second moments: the same pass with per-slot sums of squares -------------------------------------------------------
 *
 * Everything stated for rt_render_features_device holds — rays, samples, slots, sharding, chunking, refusals — and the four sum planes
 * written here are bit for bit the ones it writes. Beside them, per output slot, three optional planes: albedo_sq_sum (3 f32),
 * normal_sq_sum (3 f32) and depth_sq_sum (1 f32), each the sum over the pass's samples of the SQUARE of that sample's value: the square is
 * formed in f32 (x * x, rounded, then added; never fused), a miss adds 0 to normal and depth. Folded sequentially in sample order in f32
 * from 0 — or, under RT_FEATURES_ACCUMULATE, from the value already in the plane — so passes over [0, a) and [a, N), the second
 * accumulating, leave the bits of one pass over [0, N), for the sums and the squares alike; and neither depends on pool_slots, the
 * chunking or the shard. What a variance-normalised guide needs (rt_denoise_guided_moments_device): the variance of a feature's mean over
 * n samples is max(Q - S^2 / n, 0) / (n (n - 1)).
 * Any pointer may be NULL = not wanted; all seven NULL, a pointer that is not 16-byte aligned, or struct_bytes <
 * sizeof(RtFeatureMomentBuffers) is RT_ERR_INVALID and nothing is written. RtStats as for rt_render_features_device. */
typedef struct RtFeatureMomentBuffers {   /* device memory the caller owns; any pointer may be NULL = not wanted; 16-byte aligned */
    uint32_t struct_bytes;    /* sizeof(RtFeatureMomentBuffers) as the caller compiled it (the struct may grow at its end) */
    uint32_t _pad;
    void* albedo_sum;         /* as RtFeatureBuffers */
    void* normal_sum;
    void* depth_sum;
    void* hits;
    void* albedo_sq_sum;      /* 3 f32 per slot */
    void* normal_sq_sum;      /* 3 f32 per slot */
    void* depth_sq_sum;       /* 1 f32 per slot */
} RtFeatureMomentBuffers;
/* Host only, no device: validates (params, options, buffers' struct_bytes) and reports the reason through rt_last_error. */
int rt_feature_moments_check(const RtParams* params, const RtFeatureOptions* options, const RtFeatureMomentBuffers* buffers);
int rt_render_feature_moments_device(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* params, const RtFeatureOptions* options,
                                     const RtFeatureMomentBuffers* buffers, RtStats* stats);

/* Host-side helper: scatter `shard_count` gathered shard buffers (each rt_output_floats long,
   in shard order) into a full-frame rgb_sum. */
int rt_untile(const RtParams* params, const float* gathered, float* rgb_sum);

/* write_color (main.rs:141-169) on the device: rgb_sum (device, full frame) -> RGB8 (device). */
int rt_resolve_device(RtCtx* ctx, const void* rgb_sum_device, uint32_t width, uint32_t height,
                      uint32_t samples_per_pixel, void* rgb8_device);

/* ---- multi-GPU: the framebuffer tile-sharded over the GPUs of one node, one RCCL gather over xGMI -----------------------
 *
 * The path shards by independent pixels (main.rs:731-784 carries no cross-pixel state): the image is cut into
 * tile_size x tile_size tiles, tile t belongs to GPU t % n, the scene is replicated, every GPU renders its tiles into a compact
 * buffer, and ONE grouped ncclSend/ncclRecv exchange moves the shards to the root, whose device puts the tiles in place. The
 * picture does not depend on n (the RNG is keyed by the global pixel index). RCCL is loaded (dlopen librccl.so.1) at the first of
 * these calls; the single-GPU entry points above never touch it.
 *
 * RT_OUT_RGB8 applies write_color (main.rs:141-169) on every shard BEFORE the gather: 3 bytes per pixel cross xGMI instead of 12. */
typedef enum RtOutputKind {
    RT_OUT_RGB_SUM_F32 = 0,  /* per-pixel RGB sums, f32 (what rt_render writes) */
    RT_OUT_RGB8 = 1          /* write_color applied: RGB8, the bytes main.rs:781 stores into the image buffer */
} RtOutputKind;

/* (a) ONE PROCESS, n GPUs — what the reference's single-process host (main.rs:651-799) binds: replaces the pixel loops
 *     main.rs:730-784 by one call. n device contexts, one host thread per device inside the call, ncclCommInitAll. */
typedef struct RtMultiCtx RtMultiCtx;
typedef struct RtMultiScene RtMultiScene;
int rt_ctx_create_multi(const int* device_ids, int n_devices, RtMultiCtx** out_ctx);
int rt_ctx_destroy_multi(RtMultiCtx* ctx);
int rt_scene_upload_multi(RtMultiCtx* ctx, const RtSceneDesc* desc, RtMultiScene** out_scene);   /* compiled once, replicated on every device */
int rt_scene_upload_multi_ex(RtMultiCtx* ctx, const RtSceneDesc* desc, const RtUploadOptions* options, RtMultiScene** out_scene);
int rt_scene_destroy_multi(RtMultiCtx* ctx, RtMultiScene* scene);
/* Full frame to HOST memory: rgb_sum_host[(y*width + x)*3 + c] f32 sums, or rgb8_host[...] after write_color.
   params->shard_index / shard_count are ignored (the library shards over its devices); tile_size 0 = 32. */
int rt_render_multi(RtMultiCtx* ctx, const RtMultiScene* scene, const RtCamera* cam, const RtParams* params,
                    float* rgb_sum_host, RtStats* stats);
int rt_render_multi_rgb8(RtMultiCtx* ctx, const RtMultiScene* scene, const RtCamera* cam, const RtParams* params,
                         uint8_t* rgb8_host, RtStats* stats);
const char* rt_last_error_multi(const RtMultiCtx* ctx);

/* (b) ONE PROCESS PER GPU (torchrun-style launchers): every rank owns an RtCtx; rank 0 makes the RCCL id, the launcher's own
 *     channel carries its 128 bytes to the other ranks, every rank attaches a communicator to its context. */
#define RT_COMM_ID_BYTES 128
int rt_comm_unique_id(uint8_t* id_out /* RT_COMM_ID_BYTES */);
int rt_comm_init_rank(RtCtx* ctx, const uint8_t* id /* RT_COMM_ID_BYTES */, int rank, int world);   /* collective over all ranks */
/* A grouped ncclSend/ncclRecv of a small buffer from this rank to itself through the context's communicator, checked byte for
   byte: proves on a one-GPU box that librccl loads, the communicator works and the exchange completes on the context's stream. */
int rt_comm_selftest(RtCtx* ctx);
/* Collective: every rank renders its shard (shard_index / shard_count of `params` are ignored, the communicator's rank / world
   are used) and sends it to rank 0; rank 0 leaves the FULL frame in `frame_device` (width*height*3 elements of f32 or u8,
   device memory the caller owns; other ranks pass NULL). Blocks until this rank's part is done. */
int rt_render_gather(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* params, uint32_t output_kind,
                     void* frame_device, RtStats* stats);
/* The root's last step on its own, for callers that gather shards themselves (e.g. with torch.distributed): `gathered_device` =
   params->shard_count shard buffers of shard 0's size back to back (f32 rgb sums or, output_kind RT_OUT_RGB8, bytes), device memory;
   `frame_device` = width*height*3 elements. One kernel on the context's stream; blocks until done. */
int rt_untile_device(RtCtx* ctx, const RtParams* params, uint32_t output_kind, const void* gathered_device, void* frame_device);
/* rt_untile for RGB8 shard buffers (host helper, same layout rules as rt_untile). */
int rt_untile_rgb8(const RtParams* params, const uint8_t* gathered, uint8_t* rgb8);

/* ---- introspection of the scene compiler: host only, never touches a GPU ---- */
typedef struct RtCompileInfo {
    uint64_t n_nodes;       /* threaded-BVH records */
    uint64_t n_box_nodes;   /* of which carry a box (= BVHNode count of the reference tree) */
    uint64_t n_spheres, n_moving, n_rects, n_tris, n_media, n_xforms, n_lights, n_materials;
    uint32_t features;      /* kernel feature bits the scene needs (128: a triangle on the device carries attributes, n_tri_attrs > 0;
                               256: RT_SCENE_LIGHTS_ALL_SHAPES and a light that is not a bare XZ rect or sphere, or RT_SCENE_LIGHTS_MANY;
                               512: RT_SCENE_LIGHTS_MANY, the lights table carries the light tree;
                               1024: the upload options carry an environment map, always with 256) */
    uint32_t fits_lds;      /* nodes + sphere records fit the LDS staging budget */
    uint32_t n_first;       /* primitives tested when a walk begins instead of being met by it (none with RT_LAYOUT_LISTS_AS_REFERENCE) ... */
    uint32_t first[4];      /* ... as leaf words: kind << 28 | count << 24 | first index (kind 1 = sphere, 2 = moving sphere, 5 = medium); they are not in the node records */
    uint32_t n_tri_attrs;   /* triangle records on the device that carry attributes (RtTriangleAttrs with a flag set; instanced copies count) */
} RtCompileInfo;
int rt_scene_compile_info(const RtSceneDesc* desc, RtCompileInfo* out);
int rt_scene_compile_info_ex(const RtSceneDesc* desc, const RtUploadOptions* options, RtCompileInfo* out);
/* Copies the compiled node records (32 B each: f32 min[3], u32 skip, f32 max[3], u32 leaf) and the
   sphere records (f32 center[3], radius) + per-sphere meta words. Any output pointer may be NULL. */
int rt_scene_compile_dump(const RtSceneDesc* desc, void* nodes, uint64_t cap_nodes,
                          float* spheres, uint32_t* sphere_meta, uint64_t cap_spheres);
int rt_scene_compile_dump_ex(const RtSceneDesc* desc, const RtUploadOptions* options, void* nodes, uint64_t cap_nodes,
                             float* spheres, uint32_t* sphere_meta, uint64_t cap_spheres);

/* Camera lists (csrc/camera_lists.h): per 8 x 8-pixel square of a width x height frame, row-major over ceil(width / 8) x ceil(height / 8)
   squares, 17 words: the number of spheres of the tree a camera ray of that square can meet (0xFFFFFFFF: more than 16, the square's rays are
   walked), then their indices into rt_scene_compile_dump's sphere records, in the order the node records reach their leaves; unused words
   are 0. A sphere tested before the tree (RtCompileInfo.first) is not in the lists.
     rt_camera_lists_host  (host only) the lists of a scene as compiled with the default options, by the predicate the device runs.
                           *out_n_squares = 0: the lists do not serve this scene (a primitive that is no static sphere) or camera (not finite).
     rt_camera_lists_last  the lists the last render or pass of this context built on the device; *out_n_squares = 0: it built none
                           (RT_FLAG_NO_CAMERA_LISTS, RT_FLAG_COUNTERS, RT_FLAG_FUSED, a scene that is not sphere-only or not walked from LDS).
   lists may be NULL (the count only); cap_words < 17 * squares is RT_ERR_INVALID. */
int rt_camera_lists_host(const RtSceneDesc* desc, const RtCamera* cam, uint32_t width, uint32_t height, uint32_t* lists, uint64_t cap_words,
                         uint64_t* out_n_squares);
int rt_camera_lists_last(RtCtx* ctx, uint32_t* lists, uint64_t cap_words, uint64_t* out_n_squares);

/* RT_SCENE_LIGHTS_MANY (host only): the light tree and the weights as the upload lays them out. n = members of the lights list.
     nodes   2n - 1 records of 32 B in pre-order, the device's form (csrc/device_types.h NodeDev): f32 cx, cy, hx, hy, cz, hz (the box is
             centre -+ half extent, pad included), u32 skip (index of the first record after this one's subtree, <= 2n - 1), u32 leaf
             (0: an inner record, its first child is the next record; else 1 + the slot of its member)
     slot_member[s]  the member (index in the caller's list) whose record is slot s of the reordered table: the leaves left to right
     p[k], cdf[k]    by member k, in list order (RtSceneDesc.scene_flags has the rule)
   Any output pointer may be NULL; *out_n_lights and *out_n_nodes are always written. cap_nodes < 2n - 1 with nodes, or cap_lights < n
   with one of the other three, is RT_ERR_INVALID; so is a scene without the flag. */
int rt_scene_light_tree_dump(const RtSceneDesc* desc, void* nodes, uint64_t cap_nodes, uint32_t* slot_member, float* p, float* cdf, uint64_t cap_lights,
                             uint64_t* out_n_lights, uint64_t* out_n_nodes);

/* Builds the layout used when a scene does not fit LDS as a whole — the array in HBM plus an LDS copy of the top of the tree (at most
   max_top records), linked in one address space — and checks it on the host: the walk that passes every box enumerates all records
   in pre-order, every skip link lands where the plain array's does, both copies of a top record agree. *out_n_top = records in
   the top (0: no top was built, e.g. the whole scene fits). */
int rt_scene_top_layout_check(const RtSceneDesc* desc, uint32_t max_top, uint64_t* out_n_top);

/* ---- the process's ROCm runtime libraries ----
 * Writes the paths of the mapped libamdhip64 / libhsa-runtime64 / librccl objects, one per line, into `out` (NUL-terminated, cut at
 * `cap`). Returns RT_ERR_DEVICE when any of them is mapped TWICE (two copies under different paths): a process then holds two HIP
 * runtimes with separate device state and dies at exit in their static destructors ("double free or corruption") — what happens when
 * PyTorch (which bundles its own copies under other file names) is imported AFTER this library has bound the system's. Load PyTorch
 * first: its copies carry the system's sonames and are then shared. rt_ctx_create makes this check itself and refuses. */
int rt_runtime_libraries(char* out, uint64_t cap);

/* Fault injection for the failure-path tests: the next `n` renders on this context fail with RT_ERR_DEVICE before any kernel is
   launched (n = 0 disarms). Lets a one-GPU box rehearse "one rank of a collective render fails". */
int rt_test_fail_next_renders(RtCtx* ctx, uint32_t n);

/* Host only (no device is touched): the per-device host threads of a multi-GPU context — started with the context, parked between
   frames — rehearsed with `n_workers` threads over `rounds` frames of counting jobs; RT_OK when every worker ran exactly once per
   frame. (rt_render_multi itself needs n > 1 devices; this is what a one-GPU box and the CPU suite can check of it.) */
int rt_test_device_workers(int n_workers, int rounds);

/* Builds the 8-wide tree a scene in HBM is walked through (a static BVH: spheres, rects, triangles, boxes under box nodes) and checks it
   on the host: every primitive sits in exactly one leaf entry of at most eight members of one kind; every entry's box, decoded with the
   device's own float arithmetic, contains everything below it; the depth fits the walk's stack. Fills `out`; RT_ERR_UNSUPPORTED when the
   scene is not of that shape (it then keeps the binary walk). */
typedef struct RtWideInfo {
    uint64_t n_nodes, n_leaf_entries, n_inner_entries, n_prims;
    uint32_t depth, _pad;
    double mean_children;      /* used child slots per node (of 8) */
    double mean_leaf_members;  /* primitives per leaf entry (of 8) */
} RtWideInfo;
int rt_scene_wide_layout_check(const RtSceneDesc* desc, RtWideInfo* out);

const char* rt_last_error(const RtCtx* ctx);  /* ctx may be NULL: last error of this thread */
uint32_t rt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_HIP_H */
