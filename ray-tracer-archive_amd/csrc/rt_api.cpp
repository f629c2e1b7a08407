// rt_api.cpp — the C ABI of include/rt_hip.h: context, scene upload, the wavefront render loop.
// There is no CPU fallback in this library: without a HIP device every entry point that would
// compute returns RT_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <limits>
#include <memory>
#include <functional>
#include <vector>

#include "rt_internal.hpp"
#include "scene_compile.hpp"
#include "wide_bvh.hpp"

using namespace rti;

namespace rti { thread_local std::string g_last_error; }

namespace {

constexpr uint64_t kMaxItems = (1ull << 32) - (1ull << 28);   // work items of one render (u32 index, with head room for the allocator's overshoot)
constexpr size_t kLdsSceneBudget = 144 * 1024;  // records + sphere data staged per workgroup (one 1024-thread group per CU then; 160 KB of LDS)

template <class T> int upload(RtCtx* ctx, DevBuf& b, const std::vector<T>& v) {
    HIP_TRY(ctx, b.ensure(v.size() * sizeof(T)));
    if (!v.empty()) HIP_TRY(ctx, hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return RT_OK;
}

}  // namespace

static uint32_t scene_features(const rtc::CompiledScene& cs) {
    uint32_t f = 0;
    if (!cs.moving_meta.empty()) f |= rtk::F_MOVING;
    if (!cs.rect_meta.empty()) f |= rtk::F_RECT;
    if (!cs.tri_meta.empty()) f |= rtk::F_TRI;
    if (!cs.media.empty()) f |= rtk::F_MEDIUM;
    if (cs.xforms.size() > 1 || cs.wraps.size() > 1) f |= rtk::F_XFORM;
    for (uint32_t mb : cs.mat_b) { const uint32_t kind = mb & 15u; if ((mb >> 4) != rtd::TEX_INLINE && kind != rtd::MK_METAL && kind != rtd::MK_DIELECTRIC) f |= rtk::F_TEX; }
    if (cs.has_lights) f |= rtk::F_LIGHTS;
    if (cs.lights_ext) f |= rtk::F_LIGHTS_EXT;
    if (cs.lights_tree) f |= rtk::F_LIGHTS_TREE;
    return f;
}

// Camera lists (csrc/camera_lists.h): the spheres of the tree in the order the threaded record array reaches their leaves, which is the
// order a list names its candidates in. Empty for a scene the lists do not serve: a primitive that is no static sphere, a sphere that bounds
// a medium, or several primitives tested before the tree (one such sphere is tested where rays are made and is not in the lists).
static std::vector<uint32_t> camera_order(const rtc::CompiledScene& cs) {
    std::vector<uint32_t> order;
    if (scene_features(cs) != 0u || !cs.prologue.empty() || cs.spheres.empty()) return order;
    if (cs.first_leaf != 0u && !((cs.first_leaf >> 28) == rtd::LT_SPHERE && ((cs.first_leaf >> 24) & 15u) == 1u)) return order;
    for (const rtd::Node& n : cs.nodes) {
        if (n.leaf == 0u) continue;
        const uint32_t type = n.leaf >> 28, cnt = (n.leaf >> 24) & 15u, first = n.leaf & rtd::LEAF_MAX_FIRST;
        if (type != rtd::LT_SPHERE) return std::vector<uint32_t>();
        for (uint32_t k = 0; k < cnt; ++k) order.push_back(first + k);
    }
    return order;
}
static rtcl::Camera camera_lists_camera(const RtCamera* cam, uint32_t width, uint32_t height) {
    rtcl::Camera c{};
    auto cp3 = [](double* d, const RtVec3& v) { d[0] = (double)(float)v.x; d[1] = (double)(float)v.y; d[2] = (double)(float)v.z; };   // the f32 values new_camera_ray reads
    cp3(c.org, cam->origin); cp3(c.llc, cam->lower_left_corner); cp3(c.hor, cam->horizontal); cp3(c.ver, cam->vertical);
    double u[3], v[3]; cp3(u, cam->u); cp3(v, cam->v);
    c.lens_radius = std::fabs((double)(float)cam->lens_radius) * rtcl::lens_reach(u, v);   // (an RtCamera filled by hand need not hold orthonormal u, v)
    c.width = width; c.height = height;
    return c;
}
static bool camera_is_finite(const RtCamera* cam) {
    const double v[] = {cam->origin.x, cam->origin.y, cam->origin.z, cam->lower_left_corner.x, cam->lower_left_corner.y, cam->lower_left_corner.z, cam->horizontal.x,
                        cam->horizontal.y, cam->horizontal.z, cam->vertical.x, cam->vertical.y, cam->vertical.z, cam->u.x, cam->u.y, cam->u.z, cam->v.x, cam->v.y, cam->v.z,
                        cam->lens_radius};
    for (double x : v) if (!std::isfinite((double)(float)x)) return false;
    return true;
}

int rti::validate_params(RtCtx* ctx, const RtParams* p) {
    if (!p) return set_err(ctx, RT_ERR_INVALID, "params is null");
    if (p->width < 2 || p->height < 2) return set_err(ctx, RT_ERR_INVALID, "width and height must be >= 2 (u = (i+rnd)/(W-1), main.rs:752)");
    if (p->width > 65536 || p->height > 65536) return set_err(ctx, RT_ERR_INVALID, "image too large");
    if ((uint64_t)p->width * p->height * 3ull > 0xFFFFFFFFull) return set_err(ctx, RT_ERR_INVALID, "image too large (width * height * 3 must fit 32 bits; shard the render)");
    if (p->samples_per_pixel == 0) return set_err(ctx, RT_ERR_INVALID, "samples_per_pixel must be >= 1");
    if (p->max_depth == 0 || p->max_depth > 255) return set_err(ctx, RT_ERR_INVALID, "max_depth must be in 1..255");
    if (p->nan_policy > 1) return set_err(ctx, RT_ERR_INVALID, "bad nan_policy");
    if (p->flags & ~(uint32_t)(RT_FLAG_COUNTERS | RT_FLAG_TIMING | RT_FLAG_SAMPLE_BLOCKS | RT_FLAG_FUSED | RT_FLAG_NO_CAMERA_LISTS))
        return set_err(ctx, RT_ERR_INVALID, "RtParams.flags holds an unknown bit");
    Tiling t;
    if (make_tiling(*p, t) != RT_OK) return set_err(ctx, RT_ERR_INVALID, "bad tile_size / shard_index / shard_count");
    return RT_OK;
}

// Samples per work item, as 1 << shift, for a frame of `frame_samples` samples per pixel: 1 whenever the whole IMAGE (all shards, so that
// every shard sums the same way) has fewer than 2^32 - 2^28 samples (what a u32 item index can address) — a path is then one sample,
// nothing is regenerated mid-flight and the radiance of every sample is stored on its own (16 B each: 64 GB for an unsharded render at
// the limit; this is a 288 GB device, and a sharded render holds its own shard's samples only). Larger renders group 2, 4, ...
// consecutive samples of a pixel into one item. rt_render and every pass of a progressive frame (rt_pass_check) group by this rule.
static uint32_t frame_block_shift(const RtParams& p, uint32_t frame_samples) {
    uint32_t block_shift = (p.flags & RT_FLAG_SAMPLE_BLOCKS) ? 4u : 0u;
    while ((1u << block_shift) > frame_samples && block_shift > 0) --block_shift;
    const uint64_t image_pixels = (uint64_t)p.width * p.height;
    while ((1u << block_shift) < frame_samples && image_pixels * ((frame_samples + (1u << block_shift) - 1) >> block_shift) >= kMaxItems) ++block_shift;
    return block_shift;
}

// The head of every options record of the ABI: struct_bytes holds the caller's sizeof of the record `name` (unset, or a shorter record of
// another header, is refused), and its flags word no bit outside `known`; known_names: what the message lists after "known:", if it lists any.
// A record without a flags word passes none.
static int check_header(RtCtx* ctx, uint32_t struct_bytes, size_t size, const std::string& name, uint32_t flags = 0u, uint32_t known = 0u, const char* known_names = nullptr) {
    if (struct_bytes < size || struct_bytes > 4096u) return set_err(ctx, RT_ERR_INVALID, name + ".struct_bytes is not set (sizeof(" + name + "))");
    if (flags & ~known) return set_err(ctx, RT_ERR_INVALID, name + ".flags holds an unknown bit" + (known_names ? std::string(" (known: ") + known_names + ")" : std::string()));
    return RT_OK;
}

// RtPassOptions against the params (rt_pass_check): the message names what is wrong. *shift = the frame's grouping.
static int check_pass(RtCtx* ctx, const RtParams* p, const RtPassOptions* o, uint32_t* shift) {
    const int v = validate_params(ctx, p); if (v != RT_OK) return v;
    if (!o) return set_err(ctx, RT_ERR_INVALID, "pass options are null");
    const int h = check_header(ctx, o->struct_bytes, sizeof(RtPassOptions), "RtPassOptions", o->flags, RT_PASS_ACCUMULATE); if (h != RT_OK) return h;
    const uint64_t end = (uint64_t)o->first_sample + p->samples_per_pixel;
    if (end > 0xFFFFFFFFull) return set_err(ctx, RT_ERR_INVALID, "first_sample + samples_per_pixel must be < 2^32");
    if (o->frame_samples < end) return set_err(ctx, RT_ERR_INVALID, "frame_samples is smaller than the end of the pass (first_sample + samples_per_pixel)");
    const uint32_t s = frame_block_shift(*p, o->frame_samples), m = 1u << s;
    if (o->first_sample & (m - 1u))
        return set_err(ctx, RT_ERR_INVALID, "first_sample is not a multiple of the samples per work item (" + std::to_string(m) + " for this frame)");
    if ((end & (m - 1u)) && end != o->frame_samples)
        return set_err(ctx, RT_ERR_INVALID, "the pass ends inside a work item of " + std::to_string(m) + " samples (end on a multiple of it, or at frame_samples)");
    if (shift) *shift = s;
    return RT_OK;
}

// a pass over a pixel list (rt_render_pass_pixels_device): `list` holds n entries the device has checked (rt_api.cpp check_list)
struct ListPass { const uint32_t* list; uint32_t n; uint32_t* counts; };
static int render_impl(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, const RtPassOptions& pass, void* d_out, void* d_sq, RtStats* stats,
                       const ListPass* lp);

// A call that fails half way (a HIP error, out of memory) must not leave work or recorded events in flight on the caller's stream:
// drain it and clear the sticky error before the code goes back, with the message of the failure, not of the drain.
static int drain_on_failure(RtCtx* ctx, int r) {
    if (r != RT_OK) { const std::string keep = ctx->err; (void)hipStreamSynchronize(ctx->stream); (void)hipGetLastError(); ctx->err = keep; g_last_error = keep; }
    return r;
}
static int render_pass_checked(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, const RtPassOptions& pass, void* d_out, void* d_sq,
                               RtStats* stats, const ListPass* lp = nullptr) {
    if (ctx->fail_renders != 0u) { --ctx->fail_renders; return set_err(ctx, RT_ERR_DEVICE, "injected failure (rt_test_fail_next_renders)"); }
    return drain_on_failure(ctx, render_impl(ctx, scene, cam, prm, pass, d_out, d_sq, stats, lp));
}

// The entry sequence of a query, host or device variant: ctx null -> the feature's own refusal (a refused call has written nothing) ->
// the stats zeroed -> nothing to do -> an injected failure, where the feature takes them (radiance queries, as the renders do:
// render_pass_checked) -> the context's device current -> the work, drained if it fails.
static int query_entry(RtCtx* ctx, RtStats* stats, bool nothing_to_do, bool injectable, const std::function<int()>& refuse, const std::function<int()>& work) {
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    const int v = refuse(); if (v != RT_OK) return v;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (nothing_to_do) return RT_OK;
    if (injectable && ctx->fail_renders != 0u) { --ctx->fail_renders; return set_err(ctx, RT_ERR_DEVICE, "injected failure (rt_test_fail_next_renders)"); }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return drain_on_failure(ctx, work());
}

// The host variant of a call: each buffer of the list grown to `bytes` and, where it has a source, filled from it; the device variant on
// those buffers; then each buffer with a destination copied out, and ONE wait. Nothing is written to caller memory when the device variant
// fails, and stats->render_ms covers the staging. An entry with neither source nor destination is a buffer the caller did not ask for.
struct Staged { DevBuf* buf; const void* src; void* dst; size_t bytes; };
static int staged_call(RtCtx* ctx, std::initializer_list<Staged> list, RtStats* stats, const std::function<int()>& device_variant) {
    const auto t0 = std::chrono::steady_clock::now();
    for (const Staged& s : list) {
        if (!s.src && !s.dst) continue;
        HIP_TRY(ctx, s.buf->ensure(s.bytes));
        if (s.src) HIP_TRY(ctx, hipMemcpyAsync(s.buf->p, s.src, s.bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    const int r = device_variant();
    if (r != RT_OK) return r;
    for (const Staged& s : list) if (s.dst) HIP_TRY(ctx, hipMemcpyAsync(s.dst, s.buf->p, s.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (stats) stats->render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return RT_OK;
}
// the whole frame as one pass that overwrites: what rt_render computes
static RtPassOptions one_shot(const RtParams* prm) { return RtPassOptions{(uint32_t)sizeof(RtPassOptions), 0u, 0u, prm->samples_per_pixel}; }
int rti::render_checked(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, void* d_out, RtStats* stats) {
    return render_pass_checked(ctx, scene, cam, prm, one_shot(prm), d_out, nullptr, stats);
}

template <class T>
static int untile_host(const RtParams* p, const T* gathered, T* frame) {
    if (!p || !gathered || !frame) return set_err(nullptr, RT_ERR_INVALID, "null argument");
    Tiling t; RtParams q = *p; q.shard_count = 1; q.shard_index = 0;
    if (make_tiling(q, t) != RT_OK) return set_err(nullptr, RT_ERR_INVALID, "bad tiling parameters");
    const uint32_t sc = p->shard_count <= 1u ? 1u : p->shard_count;
    const uint64_t ts2 = (uint64_t)t.ts * t.ts;
    // every shard buffer has the size of the largest shard (shard 0)
    const uint64_t per_shard = (uint64_t)((t.n_tiles + sc - 1) / sc) * ts2 * 3u;
    for (uint32_t tile = 0; tile < t.n_tiles; ++tile) {
        const uint32_t s = tile % sc, lt = tile / sc, tx = tile % t.tiles_x, ty = tile / t.tiles_x;
        const T* src = gathered + (uint64_t)s * per_shard + (uint64_t)lt * ts2 * 3u;
        for (uint32_t py = 0; py < t.ts; ++py) {
            const uint32_t y = ty * t.ts + py; if (y >= p->height) break;
            for (uint32_t px = 0; px < t.ts; ++px) {
                const uint32_t x = tx * t.ts + px; if (x >= p->width) break;
                const T* a = src + ((uint64_t)py * t.ts + px) * 3u;
                T* b = frame + ((uint64_t)y * p->width + x) * 3u;
                b[0] = a[0]; b[1] = a[1]; b[2] = a[2];
            }
        }
    }
    return RT_OK;
}
static int ctx_init(RtCtx* ctx, void* stream) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess) ctx->n_cu = prop.multiProcessorCount;
    if (stream) { ctx->stream = (hipStream_t)stream; ctx->own_stream = false; }
    else { HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)); ctx->own_stream = true; }
    HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_count, 4 * rtk::kQueues * sizeof(uint32_t), hipHostMallocDefault));   // ring of 4 (render_impl kRing) x (one pool size per queue)
    HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_counters, sizeof(unsigned long long) * 16, hipHostMallocDefault));
    HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_words, 128 * sizeof(uint32_t), hipHostMallocDefault));
    return RT_OK;
}

// (every rt_* entry point below is declared extern "C" by include/rt_hip.h; the definitions take their linkage from there)
uint32_t rt_abi_version(void) { return RT_ABI_VERSION; }
const char* rt_last_error(const RtCtx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int rt_ctx_create(int device_id, void* stream, RtCtx** out_ctx) {
    if (!out_ctx) return set_err(nullptr, RT_ERR_INVALID, "out_ctx is null");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return set_err(nullptr, RT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= n) return set_err(nullptr, RT_ERR_INVALID, "device_id out of range");
    {   // two HIP runtimes in one process end in heap corruption at exit ("the abort of round 2"): refuse early, with the reason
        std::string listing, why;
        if (!runtime_libraries_ok(listing, why)) return set_err(nullptr, RT_ERR_DEVICE, why);
    }
    RtCtx* ctx = new RtCtx();
    ctx->device = device_id;
    const int rc = ctx_init(ctx, stream);
    if (rc != RT_OK) { g_last_error = ctx->err; rt_ctx_destroy(ctx); return rc; }   // nothing of a half-built context survives
    *out_ctx = ctx;
    return RT_OK;
}

int rt_ctx_destroy(RtCtx* ctx) {
    if (!ctx) return RT_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    comm_release(ctx);   // before the memory its exchanges use goes
    for (hipEvent_t ev : ctx->events) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : ctx->ev_gather) if (ev) (void)hipEventDestroy(ev);
    if (ctx->h_count) (void)hipHostFree(ctx->h_count);
    if (ctx->h_counters) (void)hipHostFree(ctx->h_counters);
    if (ctx->h_words) (void)hipHostFree(ctx->h_words);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;   // every device buffer of the context frees itself here (DevBuf); hipFree needs no stream, and the device is still current
    return RT_OK;
}

// ---- device layout of the threaded BVH (device_types.h: NodeDev and the text above it) -----------------------------------------
// Every record carries BOTH of its links, as byte addresses: `hit` (where a walk goes when the box is passed) and `skip` (when it
// is not). A lane of k_extend is then nothing but its address: one select per visit, no "am I walking" test. States that used to
// be lane flags are records of their own that lead back to themselves: DONE (the walk ran off the end), IDLE (the lane holds no
// ray), and one PARK TWIN per record with a leaf payload — the leaf's `hit` link. A lane that passes a leaf's box lands on the
// twin and stays (its box cannot be passed: negative half extents) until the primitive pass reads the payload and the resume
// address out of the twin and moves the lane on.
//
//   address space:  [0, top_bytes)            LDS copy of the top of the tree (scenes that do not fit LDS as a whole; else empty)
//                   top_bytes + 32 * i         record i of the array (pre-order), i < n
//                   special = top_bytes + 32n  DONE, then IDLE, then the twins in the order of their leaves
//
// The top = every record above a depth cut (depth = number of enclosing subtrees [i, skip_i) of the threaded array), the deepest cut
// with at most `max_top` records: closed under "parent of", so a walk starts in it and re-enters it whenever a skip leads back up.
struct DevNodes {
    std::vector<unsigned char> main, top;   // main: records + DONE + IDLE + twins; top: the LDS copies (M_TOP)
    uint32_t n = 0, n_top = 0, n_twins = 0;
    uint32_t walk_start = 0;                // address of the record a walk begins at: the root, or the park twin of the leaf tested first
    uint32_t records() const { return n + 2u + n_twins; }
};
static void node_boxes(const std::vector<rtd::Node>& nodes, std::vector<rtd::NodeDev>& out) {
    // Boxes as centre c and half extent h with [c-h, c+h] containing the host box, plus the part of the device's rounding that grows with
    // the RECORD's own coordinates. The slab test (kernels.hip) computes per axis tc = fma(c, 1/d, -(o/d)), th = h*|1/d| (+ e), tc -+ th:
    // five roundings and a 1-ulp reciprocal, in all at most eps*|1/d|*(5|o| + 4(|c| + h)) with eps = 2^-24. The (|c| + h) part is paid here,
    // per record: h grows by 4 eps (|c| + h) — 1e-4 units for a box 500 units from the origin; the |o| part is the ray's (set_slab_ray: e).
    // Together they stay far below t_min * |d| (0.001), so a ray leaving a box face does not pass that box again, as in the reference.
    const float inf = std::numeric_limits<float>::infinity();
    constexpr double kEps = 5.9604644775390625e-8;
    out.resize(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) {
        const rtd::Node& n = nodes[i];
        float c[3], h[3];
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(n.mn[a]) || !std::isfinite(n.mx[a])) { c[a] = 0.f; h[a] = inf; continue; }   // a record without a box is always passed
            c[a] = (float)(0.5 * ((double)n.mn[a] + (double)n.mx[a]));
            double hd = std::max((double)n.mx[a] - (double)c[a], (double)c[a] - (double)n.mn[a]);
            hd += 4.5 * kEps * (std::fabs((double)c[a]) + hd);
            float hf = (float)hd; if ((double)hf < hd) hf = std::nextafterf(hf, inf);
            h[a] = hf;
        }
        out[i] = rtd::NodeDev{c[0], c[1], h[0], h[1], c[2], h[2], 0u, 0u};
    }
}
// Records are 32 bytes, one after the other (kernels.h SceneDev::rec_unit = 32, rec_b = 16).
// `first_leaf`: leaf word of primitives every walk tests before it enters the tree (0: none) — a park twin of its own that resumes at the root.
static bool device_nodes(const std::vector<rtd::Node>& nodes, uint32_t max_top, DevNodes& out, uint32_t first_leaf = 0u) {
    const size_t n = nodes.size();
    out = DevNodes();
    out.n = (uint32_t)n;
    constexpr uint32_t unit = 32u;
    // ---- the top (optional) ----
    std::vector<uint32_t> slot(n, 0xFFFFFFFFu);
    if (max_top != 0u && n != 0) {
        std::vector<uint32_t> depth(n), per_depth, ends;
        for (size_t i = 0; i < n; ++i) {
            while (!ends.empty() && ends.back() <= i) ends.pop_back();
            depth[i] = (uint32_t)ends.size();
            if (depth[i] >= per_depth.size()) per_depth.resize(depth[i] + 1, 0u);
            per_depth[depth[i]]++;
            if (nodes[i].skip > i + 1) ends.push_back(nodes[i].skip);
        }
        uint32_t cut = 0; uint64_t total = 0;
        while (cut < per_depth.size() && total + per_depth[cut] <= max_top) total += per_depth[cut++];
        if (cut != 0 && total < n) { uint32_t k = 0; for (size_t i = 0; i < n; ++i) if (depth[i] < cut) slot[i] = k++; out.n_top = k; }
    }
    for (const rtd::Node& nd : nodes) if (nd.leaf != 0u) out.n_twins++;
    if (first_leaf != 0u) out.n_twins++;
    const uint64_t top_bytes = (uint64_t)out.n_top * 32u, total_bytes = top_bytes + (uint64_t)out.records() * unit;
    if (total_bytes >= 0xFFFFFFF0ull) return false;                      // 32-bit byte addresses
    const uint32_t special = (uint32_t)top_bytes + (uint32_t)n * unit, done = special, idle = special + unit, twin0 = special + 2u * unit;
    auto U = [&](size_t i) -> uint32_t { return i >= n ? done : (slot[i] != 0xFFFFFFFFu ? slot[i] * 32u : (uint32_t)top_bytes + (uint32_t)i * unit); };
    std::vector<rtd::NodeDev> box;
    node_boxes(nodes, box);
    std::vector<rtd::NodeDev> recs((size_t)out.records());               // record k of the array, whatever its address
    out.top.assign((size_t)top_bytes, 0);
    auto put = [&](uint32_t address_in_main, const rtd::NodeDev& d) { recs[address_in_main / unit] = d; };
    auto self_loop = [&](uint32_t addr, uint32_t resume, uint32_t payload) {
        rtd::NodeDev d{0.f, 0.f, -1.f, -1.f, 0.f, -1.f, addr, addr};     // h < 0: lo > hi on every axis, the box is never passed
        std::memcpy(&d.cx, &resume, 4); std::memcpy(&d.cy, &payload, 4);
        return d;
    };
    uint32_t k = 0;
    for (size_t i = 0; i < n; ++i) {
        rtd::NodeDev d = box[i];
        d.skip_bytes = U(nodes[i].skip);
        if (nodes[i].leaf != 0u) {
            const uint32_t twin = twin0 + unit * k++;
            d.leaf = twin;                                                // hit link -> its park twin
            put(twin - (uint32_t)top_bytes, self_loop(twin, U(nodes[i].skip), nodes[i].leaf));   // resume = first record after the leaf
        } else d.leaf = U(i + 1);                                         // hit link -> the next record in pre-order
        put((uint32_t)i * unit, d);
        if (slot[i] != 0xFFFFFFFFu) std::memcpy(out.top.data() + (size_t)slot[i] * 32, &d, 32);
    }
    if (first_leaf != 0u) {
        const uint32_t twin = twin0 + unit * k++;
        put(twin - (uint32_t)top_bytes, self_loop(twin, U(0), first_leaf));
        out.walk_start = twin;
    } else out.walk_start = U(0);
    put((uint32_t)n * unit, self_loop(done, done, rtd::LEAF_DONE));
    put((uint32_t)n * unit + unit, self_loop(idle, idle, rtd::LEAF_IDLE));
    // the bytes as they lie in memory (and, staged by a linear copy, in LDS)
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(recs.data());
    out.main.assign(bytes, bytes + recs.size() * sizeof(rtd::NodeDev));
    return true;
}
// Compressed layout (device_types.h Node16) for scenes that do not fit LDS. The grid spans the union of the finite boxes; a corner
// is rounded outwards to the grid and moved one step further out, which covers the decode's rounding (t = q * (scale/d) + (lo - o)/d
// carries ~1e-7 of the scene's extent in space, a grid step is 1.5e-5 of it). Returns false when the scene has no finite box.
// ---- near-first record orders for the HBM walk ---------------------------------------------------------------------------------------
// A threaded walk visits the children of a node in ONE fixed order. For a ray that runs against that order the far child comes first, its
// hit does not shrink t_max for the near child, and the walk visits most of both subtrees. With 288 GB of HBM the remedy is space: the
// record array once per direction OCTANT, each with the two children of every binary box node ordered near-first for that octant (the axis on
// which the children's centres differ most decides). A walk starts in the array of its ray's octant; the arrays share the primitive
// tables. Which child is visited first changes no closest hit (BVHNode::hit, bvh.rs:134-143, keeps the nearer of both whatever the order).
static void octant_order(const std::vector<rtd::Node>& in, uint32_t oct, std::vector<rtd::Node>& out) {
    const size_t n = in.size();
    out.clear(); out.reserve(n);
    auto boxed = [&](uint32_t i) { return std::isfinite(in[i].mn[0]) && std::isfinite(in[i].mx[0]) && std::isfinite(in[i].mn[1]) && std::isfinite(in[i].mx[1]) && std::isfinite(in[i].mn[2]) && std::isfinite(in[i].mx[2]); };
    auto sub_end = [&](uint32_t i) { return (uint32_t)std::min<size_t>(std::max<size_t>(in[i].skip, (size_t)i + 1), n); };
    std::vector<uint32_t> stack, kids;
    for (uint32_t c = 0; c < n; c = sub_end(c)) kids.push_back(c);
    for (size_t k = kids.size(); k-- > 0;) stack.push_back(kids[k]);
    while (!stack.empty()) {
        const uint32_t i = stack.back(); stack.pop_back();
        const uint32_t pos = (uint32_t)out.size(), end = sub_end(i);
        out.push_back(in[i]);
        out[pos].skip = pos + (end - i);
        if (in[i].leaf != 0u || end == i + 1) continue;
        kids.clear();
        for (uint32_t c = i + 1; c < end; c = sub_end(c)) kids.push_back(c);
        if (kids.size() == 2 && boxed(kids[0]) && boxed(kids[1])) {
            int axis = 0; double best = -1.0, ca[3], cb[3];
            for (int a = 0; a < 3; ++a) {
                ca[a] = 0.5 * ((double)in[kids[0]].mn[a] + in[kids[0]].mx[a]); cb[a] = 0.5 * ((double)in[kids[1]].mn[a] + in[kids[1]].mx[a]);
                if (std::fabs(ca[a] - cb[a]) > best) { best = std::fabs(ca[a] - cb[a]); axis = a; }
            }
            const bool negative = ((oct >> axis) & 1u) != 0u;                  // the ray runs towards lower coordinates on that axis
            if (ca[axis] != cb[axis] && (ca[axis] < cb[axis]) == negative) std::swap(kids[0], kids[1]);
        }
        for (size_t k = kids.size(); k-- > 0;) stack.push_back(kids[k]);
    }
}
// The axes worth an array of their own: bit a set when axis a separates the two children of at least 10 % of the binary box nodes. A
// scene spread over a plane (config 5: a million spheres on the ground; y decides 6 % of its nodes) gets the arrays of 4 quadrants,
// not 8 octants — half the cache footprint for the same visits (8 arrays 64.9 visits per segment, 1067 Msamples/s; x and z only 65.4, 1109).
static uint32_t deciding_axes(const std::vector<rtd::Node>& in) {
    const size_t n = in.size();
    auto boxed = [&](size_t i) { for (int a = 0; a < 3; ++a) if (!std::isfinite(in[i].mn[a]) || !std::isfinite(in[i].mx[a])) return false; return true; };
    auto sub_end = [&](size_t i) { return std::min<size_t>(std::max<size_t>(in[i].skip, i + 1), n); };
    uint64_t count[3] = {0, 0, 0}, total = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t end = sub_end(i);
        if (in[i].leaf != 0u || end == i + 1) continue;
        const size_t k0 = i + 1, k1 = sub_end(k0);
        if (k1 >= end || sub_end(k1) != end || !boxed(k0) || !boxed(k1)) continue;     // exactly two children, both with a box
        int axis = 0; double best = -1.0;
        for (int a = 0; a < 3; ++a) {
            const double dc = std::fabs(0.5 * ((double)in[k0].mn[a] + in[k0].mx[a]) - 0.5 * ((double)in[k1].mn[a] + in[k1].mx[a]));
            if (dc > best) { best = dc; axis = a; }
        }
        count[axis]++; total++;
    }
    uint32_t mask = 0u;
    for (int a = 0; a < 3; ++a) if (total != 0 && count[a] * 10u >= total) mask |= 1u << a;
    return mask;
}
static bool device_nodes16(const std::vector<rtd::Node>& nodes, std::vector<rtd::Node16>& out, float grid_lo[3], float grid_scale[3], uint32_t link_base = 0u,
                           bool keep_grid = false) {
    const size_t n = nodes.size();
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (const rtd::Node& nd : nodes) for (int a = 0; a < 3; ++a) {
        if (std::isfinite(nd.mn[a])) lo[a] = std::min(lo[a], (double)nd.mn[a]);
        if (std::isfinite(nd.mx[a])) hi[a] = std::max(hi[a], (double)nd.mx[a]);
    }
    for (int a = 0; a < 3 && !keep_grid; ++a) {
        if (!(hi[a] >= lo[a])) return false;
        const double pad = 1e-6 * (std::fabs(lo[a]) + std::fabs(hi[a])) + 1e-30;
        lo[a] -= pad; hi[a] += pad;
        grid_lo[a] = (float)lo[a]; if ((double)grid_lo[a] > lo[a]) grid_lo[a] = std::nextafterf(grid_lo[a], -std::numeric_limits<float>::infinity());
        double sc = (hi[a] - (double)grid_lo[a]) / 65533.0;               // corners use 1 .. 65534 before the extra step
        grid_scale[a] = (float)sc; if ((double)grid_scale[a] < sc) grid_scale[a] = std::nextafterf(grid_scale[a], std::numeric_limits<float>::infinity());
    }
    if ((uint64_t)(n + 2) * 16ull >= 0x7FFFFFF0ull) return false;          // links are 31-bit byte offsets
    out.assign(n + 2, rtd::Node16{});
    for (size_t i = 0; i < n; ++i) {
        const rtd::Node& nd = nodes[i];
        rtd::Node16 r{};
        const bool boxed = std::isfinite(nd.mn[0]) && std::isfinite(nd.mx[0]);
        if (!boxed) { r.lo[0] = 0xFFFFu; r.hi[0] = 0u; r.lo[1] = r.lo[2] = 0u; r.hi[1] = r.hi[2] = 0xFFFFu; }
        else for (int a = 0; a < 3; ++a) {
            const double ql = std::floor(((double)nd.mn[a] - (double)grid_lo[a]) / (double)grid_scale[a]) - 1.0;
            const double qh = std::ceil(((double)nd.mx[a] - (double)grid_lo[a]) / (double)grid_scale[a]) + 1.0;
            r.lo[a] = (uint16_t)std::min(65535.0, std::max(0.0, ql));
            r.hi[a] = (uint16_t)std::min(65535.0, std::max(0.0, qh));
        }
        r.link = nd.leaf != 0u ? (0x80000000u | nd.leaf) : link_base + (uint32_t)std::min<size_t>(nd.skip, n) * 16u;
        out[i] = r;
    }
    rtd::Node16 end{};                                                      // closing record: no box, "leaf" with the DONE payload (twice: a done lane reads one further)
    end.lo[0] = 0xFFFFu; end.hi[0] = 0u; end.hi[1] = end.hi[2] = 0xFFFFu; end.link = 0x80000000u | rtd::LEAF_DONE;
    out[n] = end; out[n + 1] = end;
    return true;
}
using rtc::lds_scene_bytes;

// ---- layout options: RtUploadOptions of the ABI, resolved once per upload (the library reads no environment variable for them) -----------
struct rti::UploadOpts {
    rtc::CompileOptions compile;
    bool lds_scene = true, node16 = true, octant_order = true, shade_lds = true, extend_lds_tables = true, wide_nodes = false;
    uint32_t max_top = 1024u, octant_axes = 0u /* 0 = pick; else 8 | mask */;
};
// RtUploadOptions as the ABI promises them: unknown or contradictory switches are refused, not dropped
static int check_options(const RtUploadOptions* options, std::string& err) {
    if (options) {
        // a host built against a newer header must hear that this library does not know a switch, not have it dropped
        constexpr uint32_t kKnown = RT_LAYOUT_LISTS_AS_REFERENCE | RT_LAYOUT_LISTS_CULLED | RT_LAYOUT_NO_MEMBER_BOXES | RT_LAYOUT_MEMBER_BOXES | RT_LAYOUT_CHILD_ORDER_AS_REFERENCE |
                                    RT_LAYOUT_SCENE_IN_HBM | RT_LAYOUT_NODES_32B | RT_LAYOUT_NO_SHADE_TABLES_IN_LDS | RT_LAYOUT_NO_EXTEND_TABLES_IN_LDS | RT_LAYOUT_WIDE_NODES |
                                    RT_LAYOUT_ALL_BOX_NODES;
        if (options->struct_bytes < 8u || options->struct_bytes > 4096u) { err = "RtUploadOptions.struct_bytes is not set (sizeof(RtUploadOptions))"; return RT_ERR_INVALID; }
        const uint32_t f = options->layout_flags;
        if (f & ~kKnown) { err = "RtUploadOptions.layout_flags: unknown bit"; return RT_ERR_INVALID; }
        if (((f & RT_LAYOUT_LISTS_AS_REFERENCE) && (f & RT_LAYOUT_LISTS_CULLED)) || ((f & RT_LAYOUT_NO_MEMBER_BOXES) && (f & RT_LAYOUT_MEMBER_BOXES))) {
            err = "RtUploadOptions.layout_flags: a switch is set both ways"; return RT_ERR_INVALID;
        }
        if (options->struct_bytes >= 24u && !(options->list_park_cost >= 0.f)) { err = "RtUploadOptions.list_park_cost is negative or NaN"; return RT_ERR_INVALID; }
    }
    return RT_OK;
}

// ---- environment map (rt_hip.h RtEnvMap): checked, then its two cdf tables by the header's rule ------------------------------------------------
// the map of an options record, where the caller's struct reaches that far and names one
static const RtEnvMap* env_of(const RtUploadOptions* o) {
    static_assert(sizeof(RtUploadOptions) == 40 && offsetof(RtUploadOptionsEnv, env_map) == 40 && sizeof(RtUploadOptionsEnv) == 48, "the options record grows at its end");
    if (!o || o->struct_bytes < sizeof(RtUploadOptionsEnv)) return nullptr;
    return reinterpret_cast<const RtUploadOptionsEnv*>(o)->env_map;
}
// f64, sequential sums throughout. *total: the sum of the row sums (0: nothing to sample; both tables are then uniform)
static void env_tables(const RtEnvMap& e, float* marg, float* cond, double* total) {
    const size_t W = e.width, H = e.height;
    std::vector<double> row(H);
    std::vector<double> f(W);
    double tot = 0.0;
    for (size_t j = 0; j < H; ++j) {
        const double st = std::sin(3.14159265358979323846 * ((double)j + 0.5) / (double)H);
        double r = 0.0;
        for (size_t i = 0; i < W; ++i) {
            const float* t = e.rgb + (j * W + i) * 3;
            f[i] = (0.2126 * (double)t[0] + 0.7152 * (double)t[1] + 0.0722 * (double)t[2]) * st;
            r += f[i];
        }
        row[j] = r;
        if (cond) {
            double run = 0.0;
            for (size_t i = 0; i < W; ++i) { run += f[i]; cond[j * W + i] = r > 0.0 ? (float)(run / r) : (float)((double)(i + 1) / (double)W); }
            cond[j * W + W - 1] = 1.0f;
        }
    }
    for (size_t j = 0; j < H; ++j) tot += row[j];
    if (marg) {
        double run = 0.0;
        for (size_t j = 0; j < H; ++j) { run += row[j]; marg[j] = tot > 0.0 ? (float)(run / tot) : (float)((double)(j + 1) / (double)H); }
        marg[H - 1] = 1.0f;
    }
    if (total) *total = tot;
}
static int check_env(const RtEnvMap* e, std::string& err) {
    if (!e) return RT_OK;
    if (e->struct_bytes < sizeof(RtEnvMap) || e->struct_bytes > 4096u) { err = "RtEnvMap.struct_bytes is not set (sizeof(RtEnvMap))"; return RT_ERR_INVALID; }
    if (e->flags & ~(uint32_t)RT_ENV_SAMPLED) { err = "RtEnvMap.flags holds an unknown bit (known: RT_ENV_SAMPLED)"; return RT_ERR_INVALID; }
    if (e->width == 0u || e->height == 0u || e->width > 16384u || e->height > 16384u) { err = "RtEnvMap.width and height must be in 1..16384"; return RT_ERR_INVALID; }
    if (!e->rgb) { err = "RtEnvMap.rgb is NULL"; return RT_ERR_INVALID; }
    if (!(std::isfinite(e->scale) && e->scale >= 0.f)) { err = "RtEnvMap.scale is negative or not finite"; return RT_ERR_INVALID; }
    const size_t n = (size_t)e->width * e->height * 3;
    for (size_t k = 0; k < n; ++k)
        if (!(std::isfinite(e->rgb[k]) && e->rgb[k] >= 0.f)) { err = "RtEnvMap.rgb: texel " + std::to_string(k / 3) + " is negative or not finite"; return RT_ERR_INVALID; }
    if (e->flags & RT_ENV_SAMPLED) {
        double total = 0.0;
        env_tables(*e, nullptr, nullptr, &total);
        if (!(total > 0.0) || !std::isfinite(total)) { err = "RtEnvMap: RT_ENV_SAMPLED on a map whose total weight is not a positive finite number"; return RT_ERR_INVALID; }
    }
    return RT_OK;
}
int rt_env_tables(const RtEnvMap* env_map, float* marg, float* cond) {
    if (!env_map) return set_err(nullptr, RT_ERR_INVALID, "null argument");
    std::string err;
    { const int ok = check_env(env_map, err); if (ok != RT_OK) return set_err(nullptr, ok, err); }
    env_tables(*env_map, marg, cond, nullptr);
    return RT_OK;
}

static rti::UploadOpts resolve_options(const RtUploadOptions* o) {
    rti::UploadOpts u;
    u.compile.elide_within_lds_bytes = kLdsSceneBudget;
    u.compile.lights_ext_always = env_of(o) != nullptr;   // a scene with a map runs the instances that read extended light records (kernels.h F_ENV)
    if (o && o->struct_bytes >= 8u) {
        const uint32_t f = o->layout_flags;
        // box records are elided in the layout a scene staged in LDS gets by default only: the reference's counts (LISTS_AS_REFERENCE,
        // NO_MEMBER_BOXES) are compared record by record, and the walks from HBM (octant orders, the 8-wide tree) rely on binary nodes
        if (f & (RT_LAYOUT_ALL_BOX_NODES | RT_LAYOUT_LISTS_AS_REFERENCE | RT_LAYOUT_NO_MEMBER_BOXES | RT_LAYOUT_SCENE_IN_HBM | RT_LAYOUT_WIDE_NODES)) u.compile.elide_within_lds_bytes = 0;
        if (f & RT_LAYOUT_LISTS_AS_REFERENCE) { u.compile.cull_lists = 0; u.compile.big_spheres_first = false; }   // "nothing tested at the start of a walk"
        else if (f & RT_LAYOUT_LISTS_CULLED) u.compile.cull_lists = 1;
        if (f & RT_LAYOUT_NO_MEMBER_BOXES) u.compile.member_boxes = 0; else if (f & RT_LAYOUT_MEMBER_BOXES) u.compile.member_boxes = 1;
        u.octant_order = !(f & RT_LAYOUT_CHILD_ORDER_AS_REFERENCE);
        u.lds_scene = !(f & RT_LAYOUT_SCENE_IN_HBM);
        u.node16 = !(f & RT_LAYOUT_NODES_32B);
        u.shade_lds = !(f & RT_LAYOUT_NO_SHADE_TABLES_IN_LDS);
        u.extend_lds_tables = !(f & RT_LAYOUT_NO_EXTEND_TABLES_IN_LDS);
        u.wide_nodes = (f & RT_LAYOUT_WIDE_NODES) != 0u;
        if (u.wide_nodes) u.compile.big_spheres_first = false;      // the 8-wide walk tests nothing before the tree
        if (o->struct_bytes >= 12u && o->lds_top_records) u.max_top = o->lds_top_records;
        if (o->struct_bytes >= 16u && o->octant_axes) u.octant_axes = 8u | (o->octant_axes & 7u);
        if (o->struct_bytes >= 20u) u.compile.leaf_collapse = o->leaf_collapse;
        if (o->struct_bytes >= 24u && o->list_park_cost > 0.f) u.compile.park_cost = o->list_park_cost;
    }
    u.max_top = std::min<uint32_t>(u.max_top, (128u * 1024u) / 32u);
    return u;
}

// ---- normal maps (rt_hip.h RtNormalMap): the list of an options record, where the caller's struct reaches that far ------------------------
struct NormalMaps { const RtNormalMap* p = nullptr; uint64_t n = 0u; };
static NormalMaps maps_of(const RtUploadOptions* o) {
    static_assert(sizeof(RtNormalMap) == 16 && offsetof(RtUploadOptionsMaps, normal_maps) == 48 && sizeof(RtUploadOptionsMaps) == 64, "the options record grows at its end");
    NormalMaps m;
    if (!o || o->struct_bytes < sizeof(RtUploadOptionsMaps)) return m;
    const RtUploadOptionsMaps* x = reinterpret_cast<const RtUploadOptionsMaps*>(o);
    m.p = x->normal_maps; m.n = x->n_normal_maps;
    return m;
}
// The records checked against the desc (which compile_scene has accepted). map_of: material id -> record, -1 = none; left empty without maps.
static int check_normal_maps(const RtSceneDesc& desc, const RtUploadOptions* o, std::vector<int64_t>& map_of, std::string& err) {
    map_of.clear();
    const NormalMaps maps = maps_of(o);
    if (maps.n == 0u) return RT_OK;
    if (!maps.p) { err = "RtUploadOptionsMaps.normal_maps is NULL with n_normal_maps > 0"; return RT_ERR_INVALID; }
    map_of.assign(desc.n_materials, -1);
    for (uint64_t k = 0; k < maps.n; ++k) {
        const RtNormalMap& m = maps.p[k];
        const std::string what = "RtNormalMap[" + std::to_string(k) + "]: ";
        if (m.material < 0 || (uint64_t)m.material >= desc.n_materials) { err = what + "material id out of range"; return RT_ERR_INVALID; }
        if (map_of[m.material] >= 0) { err = what + "material " + std::to_string(m.material) + " is listed twice"; return RT_ERR_INVALID; }
        if (m.image < 0 || (uint64_t)m.image >= desc.n_images) { err = what + "image id out of range"; return RT_ERR_INVALID; }
        const RtImage& im = desc.images[m.image];
        if (!im.data || im.width == 0 || im.height == 0) { err = what + "image " + std::to_string(m.image) + " has NULL data or a zero dimension"; return RT_ERR_INVALID; }
        if (!(std::isfinite(m.strength) && m.strength >= 0.f)) { err = what + "strength is negative or not finite"; return RT_ERR_INVALID; }
        if (m.flags & ~(uint32_t)RT_NMAP_FLIP_GREEN) { err = what + "flags: unknown bit (known: RT_NMAP_FLIP_GREEN)"; return RT_ERR_INVALID; }
        const int kind = desc.materials[m.material].kind;
        if (kind == RT_MAT_DIFFUSE_LIGHT || kind == RT_MAT_ISOTROPIC) {
            err = what + "material " + std::to_string(m.material) + " is an RT_MAT_DIFFUSE_LIGHT or RT_MAT_ISOTROPIC (neither scatters about a normal)"; return RT_ERR_INVALID;
        }
        map_of[m.material] = (int64_t)k;
    }
    for (uint64_t h = 0; h < desc.n_hittables; ++h) {
        const RtHittable& H = desc.hittables[h];
        const bool prim = H.kind == RT_HIT_SPHERE || H.kind == RT_HIT_MOVING_SPHERE || H.kind == RT_HIT_XY_RECT || H.kind == RT_HIT_XZ_RECT || H.kind == RT_HIT_YZ_RECT ||
                          H.kind == RT_HIT_BOX || H.kind == RT_HIT_CONSTANT_MEDIUM;
        if (prim && H.material >= 0 && (uint64_t)H.material < desc.n_materials && map_of[H.material] >= 0) {
            err = "RtNormalMap[" + std::to_string(map_of[H.material]) + "]: material " + std::to_string(H.material) + " is used by hittable " + std::to_string(h) +
                  ", which is not an RT_HIT_TRIANGLE (normal maps are served on triangles only, for now)";
            return RT_ERR_INVALID;
        }
    }
    return RT_OK;
}

// ---- triangle attributes (rt_hip.h RtTriangleAttrs): checked against the graph, then laid out by DEVICE triangle index ---------------------
// The table is parallel to tris[]: one 64-byte record per device triangle — (n0.xyz, n1.x) (n1.yz, n2.xy) (n2.z, uv0, u1) (v1, uv2, flags) —
// so that a kernel which holds the triangle index of a hit asks for it together with the vertices (no look-up through tri_meta). The
// index -> hittable map is the one the ray queries report (CompiledScene::tri_src), which every layout keeps: leaf collapse, SAH, the
// 8-wide tree and the octant arrays reorder records, never tris[]. A triangle the graph reaches several times has one device record per
// copy, and each gets the attributes. *n_with counts the device triangles that carry some; `table` stays empty when there is none, and table == nullptr checks and counts only.
static int tri_attr_table(const RtSceneDesc& desc, const RtUploadOptions* o, rtc::CompiledScene& cs, std::vector<rtd::Float4>* table, uint32_t* n_with,
                          uint32_t* n_mapped, std::string& err) {
    if (table) table->clear();
    *n_with = 0u; *n_mapped = 0u;
    std::vector<int64_t> map_of;                   // material id -> its RtNormalMap record, -1 = none; empty = the upload gave no maps
    { const int ok = check_normal_maps(desc, o, map_of, err); if (ok != RT_OK) return ok; }
    const NormalMaps maps = maps_of(o);
    const bool has_attrs = o && o->struct_bytes >= offsetof(RtUploadOptions, n_triangle_attrs) + sizeof(uint64_t) && o->n_triangle_attrs != 0u;
    if (!has_attrs && map_of.empty()) return RT_OK;
    if (has_attrs && !o->triangle_attrs) { err = "RtUploadOptions.triangle_attrs is NULL with n_triangle_attrs > 0"; return RT_ERR_INVALID; }
    std::vector<int64_t> by_id(desc.n_hittables, -1);
    for (uint64_t k = 0; has_attrs && k < o->n_triangle_attrs; ++k) {
        const RtTriangleAttrs& a = o->triangle_attrs[k];
        const std::string what = "RtTriangleAttrs[" + std::to_string(k) + "]: ";
        if (a.hittable < 0 || (uint64_t)a.hittable >= desc.n_hittables) { err = what + "hittable id out of range"; return RT_ERR_INVALID; }
        if (desc.hittables[a.hittable].kind != RT_HIT_TRIANGLE) { err = what + "hittable " + std::to_string(a.hittable) + " is not an RT_HIT_TRIANGLE"; return RT_ERR_INVALID; }
        if (by_id[a.hittable] >= 0) { err = what + "hittable " + std::to_string(a.hittable) + " is listed twice"; return RT_ERR_INVALID; }
        if (a.flags & ~(uint32_t)(RT_TRI_NORMALS | RT_TRI_UVS)) { err = what + "flags: unknown bit"; return RT_ERR_INVALID; }
        if (a.flags & RT_TRI_NORMALS) for (int v = 0; v < 3; ++v) {
            double l2 = 0.0;
            for (int c = 0; c < 3; ++c) { if (!std::isfinite(a.n[v][c])) { err = what + "a normal is not finite"; return RT_ERR_INVALID; } l2 += (double)a.n[v][c] * (double)a.n[v][c]; }
            if (!(l2 > 0.0)) { err = what + "a vertex normal has zero length"; return RT_ERR_INVALID; }
        }
        if (a.flags & RT_TRI_UVS) for (int v = 0; v < 3; ++v) for (int c = 0; c < 2; ++c)
            if (!std::isfinite(a.uv[v][c])) { err = what + "a texture coordinate is not finite"; return RT_ERR_INVALID; }
        by_id[a.hittable] = (int64_t)k;
    }
    // the device triangles that carry attributes: a record for a triangle the world does not reach attaches to nothing
    const size_t n = cs.tri_src.size();
    auto record_of = [&](size_t i) -> const RtTriangleAttrs* {
        const int64_t k = cs.tri_src[i] < by_id.size() ? by_id[cs.tri_src[i]] : -1;
        return k >= 0 && o->triangle_attrs[k].flags != 0u ? &o->triangle_attrs[k] : nullptr;
    };
    // ... and the ones whose material has a normal map (tri_meta names the material of every device triangle): a mapped triangle without
    // attributes gets a record with only the map bits
    auto map_of_tri = [&](size_t i) -> int64_t {
        const uint32_t m = cs.tri_meta[i] & rtd::META_MAT_MASK;
        return m < map_of.size() ? map_of[m] : -1;
    };
    for (size_t i = 0; i < n; ++i) {
        const bool mapped = map_of_tri(i) >= 0;
        if (record_of(i) || mapped) ++*n_with;
        if (mapped) ++*n_mapped;
    }
    if (!table || *n_with == 0u) return RT_OK;
    // Each map in use becomes one more rtd::Texture record behind the desc's textures (TK_IMAGE, a = the image, scale = the strength), so that
    // it reaches the kernels through a table they already hold and is staged in k_shade's LDS blob with the others; the triangle's record names
    // it in the high bits of its flags word (device_types.h TRI_ATTR_*). A map no device triangle uses adds nothing.
    std::vector<int64_t> tex_of(maps.n, -1);
    for (size_t i = 0; i < n; ++i) {
        const int64_t k = map_of_tri(i);
        if (k < 0 || tex_of[k] >= 0) continue;
        if (cs.textures.size() >= (1u << (32u - rtd::TRI_ATTR_MAP_TEX_SHIFT))) { err = "RtNormalMap: too many textures"; return RT_ERR_UNSUPPORTED; }
        rtd::Texture t{};
        t.kind = rtd::TK_IMAGE; t.a = maps.p[k].image; t.b = -1; t.scale = maps.p[k].strength;
        tex_of[k] = (int64_t)cs.textures.size();
        cs.textures.push_back(t);
    }
    table->assign(4 * n, rtd::Float4{0.f, 0.f, 0.f, 0.f});
    for (size_t i = 0; i < n; ++i) {
        const RtTriangleAttrs* ap = record_of(i);
        const int64_t k = map_of_tri(i);
        if (!ap && k < 0) continue;
        float f[16] = {0.f};
        uint32_t flags = 0u;
        if (ap) {
            const RtTriangleAttrs& a = *ap;
            if (a.flags & RT_TRI_NORMALS) for (int v = 0; v < 3; ++v) {
                const double x = a.n[v][0], y = a.n[v][1], z = a.n[v][2], l = std::sqrt(x * x + y * y + z * z);     // unit in f64, then rounded
                f[3 * v] = (float)(x / l); f[3 * v + 1] = (float)(y / l); f[3 * v + 2] = (float)(z / l);
            }
            if (a.flags & RT_TRI_UVS) for (int v = 0; v < 3; ++v) { f[9 + 2 * v] = a.uv[v][0]; f[10 + 2 * v] = a.uv[v][1]; }
            flags = a.flags;
        }
        if (k >= 0) flags |= rtd::TRI_ATTR_MAP | ((maps.p[k].flags & RT_NMAP_FLIP_GREEN) ? rtd::TRI_ATTR_MAP_FLIP_GREEN : 0u) | ((uint32_t)tex_of[k] << rtd::TRI_ATTR_MAP_TEX_SHIFT);
        std::memcpy(&f[15], &flags, 4);
        std::memcpy(&(*table)[4 * i], f, 64);
    }
    return RT_OK;
}

// What every compile of a caller's scene begins with: the options checked, the graph compiled under them, the triangle attributes checked
// against the result (tri_attr_table: `table` receives their device records, nullptr = checked and counted only).
static int compile_checked(const RtSceneDesc& desc, const RtUploadOptions* options, rtc::CompiledScene& cs, std::vector<rtd::Float4>* table, uint32_t* n_with, std::string& err,
                           uint32_t* n_mapped = nullptr) {
    { const int ok = check_options(options, err); if (ok != RT_OK) return ok; }
    { const int ok = check_env(env_of(options), err); if (ok != RT_OK) return ok; }
    if (env_of(options) && (desc.scene_flags & RT_SCENE_LIGHTS_MANY)) {
        err = "RtEnvMap: an environment map together with RT_SCENE_LIGHTS_MANY is not supported (that list weighs its members by area, and the map has none)";
        return RT_ERR_INVALID;
    }
    const int rc = rtc::compile_scene(desc, resolve_options(options).compile, cs);
    if (rc != RT_OK) { err = "scene: " + cs.error; return rc; }
    uint32_t mapped = 0u;
    const int ok = tri_attr_table(desc, options, cs, table, n_with, &mapped, err);
    if (n_mapped) *n_mapped = mapped;
    return ok;
}
// how far an entry's box of the 8-wide tree lies outside what is below it (rtw::build; rt_scene_wide_layout_check holds the tree to it)
static float wide_margin(const std::vector<rtd::Node>& nodes) {
    double extent = 0.0;
    for (int a = 0; a < 3; ++a) extent = std::max(extent, std::max(std::fabs((double)nodes[0].mn[a]), std::fabs((double)nodes[0].mx[a])));
    return (float)(6e-7 * extent);
}

// ---- the host image of a scene: everything an upload copies to a device, built ONCE (rt_scene_upload_multi uploads it n times) ---------
struct rti::SceneImage {
    rtc::CompiledScene cs;
    DevNodes dn;
    std::vector<rtd::Node16> n16;
    float grid_lo[3] = {0, 0, 0}, grid_scale[3] = {1, 1, 1};
    bool in_lds = false, c16 = false, top = false;
    uint32_t oct_stride = 0u, oct_mask = 7u;
    std::vector<unsigned char> blob, eblob;
    uint32_t sb[12] = {0}, perlin_only = 0u, eb[5] = {0}, eb_rect_stride = 32u;
    uint32_t features = 0u;
    rtw::WideTree wide; bool use_wide = false;     // 8-wide nodes for k_extend_wide (a static BVH that does not fit LDS)
    std::vector<rtd::Float4> tri_attrs;            // tri_attr_table: 4 records per device triangle, empty = the upload gave no attributes
    std::vector<rtd::Float4> env_texels;           // the environment map (kernels.h SceneDev::env_texels): (r, g, b, 0) per texel, empty = none
    std::vector<float> env_marg, env_cond;         // ... and its cdf tables (env_tables above)
    uint32_t env_w = 0u, env_h = 0u, env_sampled = 0u; float env_scale = 0.f;
};
void rti::scene_image_free(SceneImage* im) { delete im; }

int rti::scene_image_build(const RtSceneDesc* desc, const RtUploadOptions* options, SceneImage** out, std::string& err) {
    *out = nullptr;
    std::unique_ptr<SceneImage> im(new SceneImage());
    rtc::CompiledScene& cs = im->cs;
    uint32_t n_with = 0u;
    uint32_t n_mapped = 0u;
    { const int ok = compile_checked(*desc, options, cs, &im->tri_attrs, &n_with, err, &n_mapped); if (ok != RT_OK) return ok; }
    const UploadOpts opt = resolve_options(options);
    im->in_lds = opt.lds_scene && lds_scene_bytes(cs) <= kLdsSceneBudget;
    im->features = scene_features(cs);   // attributes change what is shaded, never what is walked: every test on `features` below sees the scene's own bits
    // RT_LAYOUT_WIDE_NODES: a static BVH in HBM (spheres / rects / triangles / boxes under box nodes only) walked 8 lanes to a ray over an
    // 8-wide tree (kernels.hip k_extend_wide) instead of the binary records below.
    if (!im->in_lds && opt.wide_nodes && opt.node16 && (im->features & ~(rtk::F_RECT | rtk::F_TRI)) == 0u && cs.prologue.empty() && cs.first_leaf == 0u && rtw::eligible(cs.nodes)) {   // (k_extend_wide tests nothing before the tree)
        std::string werr;
        im->use_wide = rtw::build(cs.nodes, wide_margin(cs.nodes), im->wide, werr) && im->wide.depth < rtd::WIDE_MAX_DEPTH;
        if (!im->use_wide) im->wide = rtw::WideTree();
    }
    // 16-byte compressed records for a scene that does not fit LDS (RT_LAYOUT_NODES_32B: 32-byte records with the top of the tree in LDS)
    im->c16 = !im->in_lds && opt.node16 && device_nodes16(cs.nodes, im->n16, im->grid_lo, im->grid_scale);
    // the record array once per direction octant (octant_order above), as long as 31-bit links reach; RT_LAYOUT_CHILD_ORDER_AS_REFERENCE: one
    // array, the reference's order (left, then right) — the order whose visit counts the tests compare with the CPU restatement's
    {
        bool octants = im->c16 && !im->use_wide && opt.octant_order && 8ull * (cs.nodes.size() + 2) * 16ull < 0x7FFFFFF0ull;   // (the wide walk orders near-first by itself)
        if (octants) {
            const uint32_t stride = (uint32_t)((cs.nodes.size() + 2) * 16);
            std::vector<rtd::Node16> all; all.reserve(8 * (cs.nodes.size() + 2));
            std::vector<rtd::Node> ordered; std::vector<rtd::Node16> one;
            uint32_t mask = (opt.octant_axes & 8u) ? (opt.octant_axes & 7u) : deciding_axes(cs.nodes);
            for (uint32_t oct = 0; oct < 8 && octants; ++oct) {
                if ((oct & ~mask) != 0u) { all.resize(all.size() + cs.nodes.size() + 2); continue; }      // never selected (kernels.hip go_root): left empty, never touched
                octant_order(cs.nodes, oct, ordered);
                octants = ordered.size() == cs.nodes.size() && device_nodes16(ordered, one, im->grid_lo, im->grid_scale, oct * stride, true);
                all.insert(all.end(), one.begin(), one.end());
            }
            if (octants) { im->n16.swap(all); im->oct_stride = stride; im->oct_mask = mask; }
        }
    }
    if (!im->c16 && !device_nodes(cs.nodes, im->in_lds ? 0u : opt.max_top, im->dn, cs.first_leaf)) { err = "scene: node array beyond 4 GB"; return RT_ERR_UNSUPPORTED; }
    im->top = !im->c16 && im->dn.n_top != 0u;
    // k_shade's small tables as one blob for LDS staging (kernels.h SceneDev::shade_blob): only when it is small
    {
        std::vector<unsigned char>& blob = im->blob; uint32_t* sb = im->sb;
        auto put = [&](const void* p, size_t bytes) { const uint32_t at = (uint32_t)blob.size(); blob.resize((blob.size() + bytes + 15) & ~(size_t)15, 0); if (bytes) std::memcpy(blob.data() + at, p, bytes); return at; };
        sb[0] = put(cs.spheres.data(), cs.spheres.size() * 16); sb[1] = put(cs.sphere_meta.data(), cs.sphere_meta.size() * 4);
        sb[2] = put(cs.rects.data(), cs.rects.size() * 16); sb[3] = put(cs.rect_meta.data(), cs.rect_meta.size() * 4);
        sb[4] = put(cs.moving.data(), cs.moving.size() * 16); sb[5] = put(cs.moving_meta.data(), cs.moving_meta.size() * 4);
        sb[6] = put(cs.mat_a.data(), cs.mat_a.size() * 16); sb[7] = put(cs.mat_b.data(), cs.mat_b.size() * 4);
        sb[8] = put(cs.xforms.data(), cs.xforms.size() * sizeof(rtd::Xform)); sb[9] = put(cs.wraps.data(), cs.wraps.size() * sizeof(rtd::Wrap));
        sb[10] = put(cs.lights.data(), cs.lights.size() * sizeof(rtd::Light)); sb[11] = put(cs.textures.data(), cs.textures.size() * sizeof(rtd::Texture));
        // every 512-path workgroup pays for the copy: measured on Cornell (1.6 KB) k_shade 87.4 -> 75.2 ms, on book-1 (19 KB) 36.8 -> 40.2 ms
        if (!(opt.shade_lds && blob.size() <= 8 * 1024)) blob.clear();
        // a scene with noise textures whose other tables are too big to stage: the Perlin tables alone (7 KB each). A turbulence is a chain of
        // 7 x 8 x 4 dependent look-ups, and a wave waits for the one lane that makes it
        if (blob.empty() && opt.shade_lds && !cs.perlins.empty() && cs.perlins.size() * sizeof(rtd::PerlinTable) <= 16 * 1024) {
            put(cs.perlins.data(), cs.perlins.size() * sizeof(rtd::PerlinTable)); im->perlin_only = 1u;
            // ... and the tables that do not grow with the primitive count, if they are small: material, texture, transform, wrapper, light
            const size_t small = cs.mat_a.size() * 20 + cs.xforms.size() * sizeof(rtd::Xform) + cs.wraps.size() * sizeof(rtd::Wrap) + cs.lights.size() * sizeof(rtd::Light) +
                                 cs.textures.size() * sizeof(rtd::Texture);
            if (small <= 4 * 1024) {
                sb[6] = put(cs.mat_a.data(), cs.mat_a.size() * 16); sb[7] = put(cs.mat_b.data(), cs.mat_b.size() * 4);
                sb[8] = put(cs.xforms.data(), cs.xforms.size() * sizeof(rtd::Xform)); sb[9] = put(cs.wraps.data(), cs.wraps.size() * sizeof(rtd::Wrap));
                sb[10] = put(cs.lights.data(), cs.lights.size() * sizeof(rtd::Light)); sb[11] = put(cs.textures.data(), cs.textures.size() * sizeof(rtd::Texture));
            } else im->perlin_only = 2u;
        }
    }
    // k_extend's primitive pass tables for LDS-resident scenes (kernels.h SceneDev::ext_blob): small ones only, inside the LDS budget
    if (im->in_lds && opt.extend_lds_tables && !(cs.rects.empty() && cs.moving.empty() && cs.media.empty())) {
        // staged once per workgroup and launch (persistent waves), so size only matters against the 160 KB of the CU: the box records
        // (32 B per Box) always; the rect table as it is (2 x 16 B per rect) where that fits too, else without its two padding words, else
        // not at all — in a scene whose rects are the sides of boxes (book-2 final: 2400 of 2401) the walk never reads them, and the one
        // lone rect comes from HBM/L2
        std::vector<unsigned char>& eblob = im->eblob; uint32_t* eb = im->eb;
        const size_t room = 160 * 1024 - lds_scene_bytes(cs);
        const size_t n_rects = cs.rects.size() / 2;
        for (uint32_t stride : {32u, 24u, 0u}) {
            eblob.clear();
            auto put = [&](const void* p, size_t bytes) { const uint32_t at = (uint32_t)eblob.size(); eblob.resize((eblob.size() + bytes + 15) & ~(size_t)15, 0); if (bytes) std::memcpy(eblob.data() + at, p, bytes); return at; };
            eb[4] = put(cs.boxes.data(), cs.boxes.size() * 16);
            if (stride == 0u) eb[0] = 0u;
            else if (stride == 32u) eb[0] = put(cs.rects.data(), n_rects * 32);
            else {
                std::vector<float> packed(n_rects * 6);
                for (size_t i = 0; i < n_rects; ++i) { std::memcpy(&packed[6 * i], &cs.rects[2 * i], 16); std::memcpy(&packed[6 * i + 4], &cs.rects[2 * i + 1], 8); }
                eb[0] = put(packed.data(), packed.size() * 4);
            }
            eb[1] = put(cs.moving.data(), cs.moving.size() * 16);
            eb[2] = put(cs.xforms.data(), cs.xforms.size() * sizeof(rtd::Xform)); eb[3] = put(cs.media.data(), cs.media.size() * sizeof(rtd::Medium));
            im->eb_rect_stride = stride;
            if (eblob.size() <= room) break;
            eblob.clear();
        }
    }
    if (!im->tri_attrs.empty()) im->features |= rtk::F_TRI_ATTR;
    if (n_mapped != 0u) im->features |= rtk::F_TEX | rtk::F_NORMAL_MAP;   // the map is a texture record: the full variant, in its instances with the map's bit (kernels.hip with_attr_variant)
    if (const RtEnvMap* e = env_of(options)) {     // (checked by compile_checked)
        const size_t n = (size_t)e->width * e->height;
        im->env_texels.resize(n);
        for (size_t k = 0; k < n; ++k) im->env_texels[k] = rtd::Float4{e->rgb[3 * k], e->rgb[3 * k + 1], e->rgb[3 * k + 2], 0.f};
        im->env_marg.resize(e->height); im->env_cond.resize(n);
        env_tables(*e, im->env_marg.data(), im->env_cond.data(), nullptr);
        im->env_w = e->width; im->env_h = e->height; im->env_scale = e->scale; im->env_sampled = (e->flags & RT_ENV_SAMPLED) ? 1u : 0u;
        im->features |= rtk::F_LIGHTS_EXT | rtk::F_ENV;   // like F_TRI_ATTR: what is shaded, never what is walked
    }
    *out = im.release();
    return RT_OK;
}

int rti::scene_image_upload(RtCtx* ctx, const SceneImage& im, RtScene** out_scene) {
    *out_scene = nullptr;
    const rtc::CompiledScene& cs = im.cs;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RtScene* s = new RtScene();
    int r = RT_OK;
    auto up = [&](auto& buf, const auto& vec) { if (r == RT_OK) r = upload(ctx, buf, vec); };
    // A scene with triangle attributes keeps them in the triangles' own allocation, IN FRONT of tris[] and in reverse: the record of
    // triangle i is the four Float4 at tris - 4 (i + 1). SceneDev is an argument of every kernel and its layout is part of their code; this
    // way it does not change, and the kernels compiled with F_TRI_ATTR find the table from the pointer they already hold.
    const size_t n_tri = cs.tri_meta.size(), tri_front = im.tri_attrs.empty() ? 0 : 4 * n_tri;
    std::vector<rtd::Float4> tris_with_attrs;
    auto up_tris = [&]() {
        if (tri_front == 0) { up(s->tris, cs.tris); return; }
        tris_with_attrs.resize(tri_front + cs.tris.size());
        for (size_t i = 0; i < n_tri; ++i) std::memcpy(&tris_with_attrs[tri_front - 4 * (i + 1)], &im.tri_attrs[4 * i], 64);
        std::memcpy(tris_with_attrs.data() + tri_front, cs.tris.data(), cs.tris.size() * sizeof(rtd::Float4));
        up(s->tris, tris_with_attrs);
    };
    if (im.top) up(s->top_nodes, im.dn.top);
    if (im.c16) up(s->nodes, im.n16); else up(s->nodes, im.dn.main);
    up(s->spheres, cs.spheres); up(s->sphere_meta, cs.sphere_meta); up(s->moving, cs.moving); up(s->moving_meta, cs.moving_meta);
    up(s->rects, cs.rects); up(s->rect_meta, cs.rect_meta); up_tris(); up(s->tri_meta, cs.tri_meta); up(s->boxes, cs.boxes); up(s->media, cs.media);
    up(s->xforms, cs.xforms); up(s->wraps, cs.wraps); up(s->mat_a, cs.mat_a); up(s->mat_b, cs.mat_b); up(s->textures, cs.textures); up(s->perlins, cs.perlins);
    up(s->images, cs.images); up(s->image_bytes, cs.image_bytes); up(s->lights, cs.lights);
    up(s->sphere_src, cs.sphere_src); up(s->moving_src, cs.moving_src); up(s->rect_src, cs.rect_src); up(s->tri_src, cs.tri_src);
    // a small scene whose shading tables are not staged in LDS: the material record of every sphere by SPHERE index (one dependent load fewer in
    // k_shade: book-1 waits ~700 cycles of a wave's ~20 000 for the material's record after the sphere's)
    std::vector<rtd::Float4> sphere_ma; std::vector<uint32_t> sphere_mb;
    if (im.blob.empty() && !cs.spheres.empty() && cs.spheres.size() <= 65536) {
        sphere_ma.resize(cs.spheres.size()); sphere_mb.resize(cs.spheres.size());
        for (size_t k = 0; k < cs.spheres.size(); ++k) { const uint32_t m = cs.sphere_meta[k] & rtd::META_MAT_MASK; sphere_ma[k] = cs.mat_a[m]; sphere_mb[k] = cs.mat_b[m]; }
        up(s->sphere_mat_a, sphere_ma); up(s->sphere_mat_b, sphere_mb);
    }
    if (im.use_wide) up(s->wide, im.wide.words);
    const std::vector<uint32_t> cam_order = im.in_lds ? camera_order(cs) : std::vector<uint32_t>();
    if (!cam_order.empty()) up(s->cam_order, cam_order);
    if (!im.blob.empty()) up(s->shade_blob, im.blob);
    if (!im.eblob.empty()) up(s->ext_blob, im.eblob);
    if (!im.env_texels.empty()) { up(s->env_texels, im.env_texels); up(s->env_marg, im.env_marg); up(s->env_cond, im.env_cond); }
    if (r == RT_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) r = set_err(ctx, RT_ERR_DEVICE, "scene upload failed");   // the image is the caller's: its vectors outlive this wait
    if (r != RT_OK) { rt_scene_destroy(ctx, s); return r; }
    rtk::SceneDev& d = s->dev;
    const uint32_t* sb = im.sb; const uint32_t* eb = im.eb;
    d.nodes = (const rtd::Float4*)s->nodes.p; d.n_nodes = (uint32_t)cs.nodes.size();
    d.top_nodes = im.top ? (const rtd::Float4*)s->top_nodes.p : nullptr; d.n_top = im.top ? im.dn.n_top : 0u; d.n_records = im.c16 ? (uint32_t)im.n16.size() : im.dn.records();
    d.rec_unit = im.c16 ? 16u : 32u; d.rec_b = im.c16 ? 0u : 16u;
    d.walk_start = im.c16 ? 0u : im.dn.walk_start; d.first_leaf = cs.first_leaf;
    d.oct_stride = im.oct_stride; d.oct_mask = im.oct_mask;
    d.sort_rays = im.c16 ? 1u : 0u;
    d.wide = im.use_wide ? (const uint4*)s->wide.p : nullptr; d.n_wide = im.use_wide ? im.wide.n_nodes : 0u;
    d.nodes16 = im.c16 ? 1u : 0u; for (int a = 0; a < 3; ++a) { d.grid_lo[a] = im.grid_lo[a]; d.grid_scale[a] = im.grid_scale[a]; }
    d.n_prologue = (uint32_t)cs.prologue.size();
    for (uint32_t k = 0; k < rtd::MAX_PROLOGUE; ++k) d.prologue[k] = k < cs.prologue.size() ? cs.prologue[k] : 0u;
    d.n_prim_kinds = (cs.sphere_meta.empty() ? 0u : 1u) + (cs.moving_meta.empty() ? 0u : 1u) + (cs.rect_meta.empty() ? 0u : 1u) +
                     (cs.tri_meta.empty() ? 0u : 1u) + (cs.media.empty() ? 0u : 1u);   // (a Box counts with the rects: their sides)
    d.spheres = (const rtd::Float4*)s->spheres.p; d.sphere_meta = (const uint32_t*)s->sphere_meta.p; d.n_spheres = (uint32_t)cs.spheres.size();
    if (!sphere_ma.empty()) { d.sphere_mat_a = (const rtd::Float4*)s->sphere_mat_a.p; d.sphere_mat_b = (const uint32_t*)s->sphere_mat_b.p; }
    d.moving = (const rtd::Float4*)s->moving.p; d.moving_meta = (const uint32_t*)s->moving_meta.p;
    d.rects = (const rtd::Float4*)s->rects.p; d.rect_meta = (const uint32_t*)s->rect_meta.p;
    d.tris = (const rtd::Float4*)s->tris.p + tri_front; d.tri_meta = (const uint32_t*)s->tri_meta.p; d.boxes = (const rtd::Float4*)s->boxes.p;
    d.media = (const rtd::Medium*)s->media.p; d.xforms = (const rtd::Xform*)s->xforms.p; d.wraps = (const rtd::Wrap*)s->wraps.p;
    d.mat_a = (const rtd::Float4*)s->mat_a.p; d.mat_b = (const uint32_t*)s->mat_b.p;
    d.textures = (const rtd::Texture*)s->textures.p; d.perlins = (const rtd::PerlinTable*)s->perlins.p;
    d.images = (const rtd::Image*)s->images.p; d.image_bytes = (const uint8_t*)s->image_bytes.p;
    d.lights = (const rtd::Light*)s->lights.p; d.n_lights = cs.n_lights;
    d.shade_blob = im.blob.empty() ? nullptr : (const rtd::Float4*)s->shade_blob.p; d.shade_blob_bytes = (uint32_t)im.blob.size();
    d.sb_spheres = sb[0]; d.sb_sphere_meta = sb[1]; d.sb_rects = sb[2]; d.sb_rect_meta = sb[3]; d.sb_moving = sb[4]; d.sb_moving_meta = sb[5];
    d.ext_blob = im.eblob.empty() ? nullptr : (const rtd::Float4*)s->ext_blob.p; d.ext_blob_bytes = (uint32_t)im.eblob.size();
    d.eb_rect_stride = im.eb_rect_stride; d.eb_rects = eb[0]; d.eb_moving = eb[1]; d.eb_xforms = eb[2]; d.eb_media = eb[3]; d.eb_boxes = eb[4];
    d.sb_perlin_only = im.perlin_only;
    d.sb_mat_a = sb[6]; d.sb_mat_b = sb[7]; d.sb_xforms = sb[8]; d.sb_wraps = sb[9]; d.sb_lights = sb[10]; d.sb_textures = sb[11];
    if (!im.env_texels.empty()) {
        d.env_texels = (const rtd::Float4*)s->env_texels.p; d.env_marg = (const float*)s->env_marg.p; d.env_cond = (const float*)s->env_cond.p;
        d.env_w = im.env_w; d.env_h = im.env_h; d.env_scale = im.env_scale; d.env_sampled = im.env_sampled;
    }
    s->src = rtk::RaySrcDev{(const uint32_t*)s->sphere_src.p, (const uint32_t*)s->moving_src.p, (const uint32_t*)s->rect_src.p, (const uint32_t*)s->tri_src.p};
    s->features = im.features;
    // a sphere with a DiffuseLight material: a camera ray can end on it, so such a scene's camera rays are not shaded where they are made (render_impl)
    for (const uint32_t meta : cs.sphere_meta) if ((cs.mat_b[meta & rtd::META_MAT_MASK] & 15u) == rtd::MK_DIFFUSE_LIGHT) s->sphere_emits = true;
    s->in_lds = im.in_lds; s->lds_bytes = lds_scene_bytes(cs);
    s->bg_mode = cs.background_mode; for (int i = 0; i < 3; ++i) s->bg[i] = cs.background[i];
    if (cs.first_leaf != 0u && ((cs.first_leaf >> 24) & 15u) == 1u) {
        const uint32_t k = cs.first_leaf & rtd::LEAF_MAX_FIRST, type = cs.first_leaf >> 28;
        if (type == rtd::LT_SPHERE) {
            s->first_id = (rtd::LT_SPHERE << 28) | k;
            s->first_prim[0] = cs.spheres[k].x; s->first_prim[1] = cs.spheres[k].y; s->first_prim[2] = cs.spheres[k].z; s->first_prim[3] = cs.spheres[k].w;
        } else if (type == rtd::LT_RECT) {
            s->first_id = (rtd::LT_RECT << 28) | k;
            std::memcpy(s->first_prim, &cs.rects[2 * k], 32);
        }
    }
    s->n_cam_order = (uint32_t)cam_order.size();
    s->n_nodes = cs.nodes.size();
    s->n_prims = cs.sphere_meta.size() + cs.moving_meta.size() + cs.rect_meta.size() + cs.tri_meta.size() + cs.media.size();
    s->bytes = cs.nodes.size() * 32 + cs.spheres.size() * 16 + cs.moving.size() * 16 + cs.rects.size() * 16 + (cs.tris.size() + tri_front) * 16 +
               4 * (cs.sphere_meta.size() + cs.moving_meta.size() + cs.rect_meta.size() + cs.tri_meta.size());
    *out_scene = s;
    return RT_OK;
}

int rt_scene_upload_ex(RtCtx* ctx, const RtSceneDesc* desc, const RtUploadOptions* options, RtScene** out_scene) {
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    if (!desc || !out_scene) return set_err(ctx, RT_ERR_INVALID, "desc / out_scene is null");
    *out_scene = nullptr;
    SceneImage* im = nullptr; std::string err;
    const int rc = scene_image_build(desc, options, &im, err);
    if (rc != RT_OK) return set_err(ctx, rc, err);
    const int r = scene_image_upload(ctx, *im, out_scene);
    scene_image_free(im);
    return r;
}
int rt_scene_upload(RtCtx* ctx, const RtSceneDesc* desc, RtScene** out_scene) { return rt_scene_upload_ex(ctx, desc, nullptr, out_scene); }

int rt_scene_destroy(RtCtx* ctx, RtScene* s) {
    if (!s) return RT_OK;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    delete s;
    return RT_OK;
}

int rt_output_floats(const RtParams* p, uint64_t* out_n) {
    if (!p || !out_n) return set_err(nullptr, RT_ERR_INVALID, "null argument");
    Tiling t;
    if (make_tiling(*p, t) != RT_OK) return set_err(nullptr, RT_ERR_INVALID, "bad tiling parameters");
    if (p->shard_count <= 1u) *out_n = (uint64_t)p->width * p->height * 3u;
    else *out_n = (uint64_t)t.n_local * t.ts * t.ts * 3u;
    return RT_OK;
}

// a launcher's own explanation (kernels.h launch_note) in front of the HIP error string
#define LAUNCH_TRY(call)                                                                                                        \
    do {                                                                                                                        \
        hipError_t e_ = (call);                                                                                                 \
        if (e_ != hipSuccess) return set_err(ctx, RT_ERR_DEVICE, std::string(rtk::launch_note() ? rtk::launch_note() : #call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ---- what the launch paths below (render_impl, trace_rays_impl, features_impl) decide in one place each --------------------------------

// The path pool's arrays, bytes per slot: ray_o ray_d hit s0 sd, and s1 = (acc, sample) for items of several samples (kernels.h PoolDev).
// A caller names how many of them it uses: 5, or all 6.
constexpr size_t kPoolRec[6] = {16, 16, 8, 16, 4, 16};
static size_t pool_slot_bytes(int n_arrays) { size_t b = 0; for (int a = 0; a < n_arrays; ++a) b += kPoolRec[a]; return b; }
static size_t pool_held_bytes(const RtCtx* ctx, int k, int n_arrays) { size_t b = 0; for (int a = 0; a < n_arrays; ++a) b += ctx->pool[k][a].bytes; return b; }
// the first n_arrays arrays of pool k, grown to P slots
static int pool_bind(RtCtx* ctx, int k, uint32_t P, int n_arrays, rtk::PoolDev& pd) {
    DevBuf* b = ctx->pool[k];
    for (int a = 0; a < n_arrays; ++a) HIP_TRY(ctx, b[a].ensure((size_t)P * kPoolRec[a]));
    pd = rtk::PoolDev{(rtd::Float4*)b[0].p, (rtd::Float4*)b[1].p, (uint2*)b[2].p, (rtd::Float4*)b[3].p, (uint32_t*)b[4].p, n_arrays > 5 ? (rtd::Float4*)b[5].p : nullptr};
    return RT_OK;
}
// Pool size: as many slots as there are items, up to `asked`; unasked (0) up to 2^28, halved while above 2^20 slots and larger than 70 %
// of the device memory the pool may take — what is free and what the buffers about to be resized hold already (`held`) — less `set_aside`.
static uint32_t pool_size(uint32_t asked, uint64_t items, size_t slot_bytes, size_t held, size_t set_aside) {
    uint32_t P = (uint32_t)std::min<uint64_t>(asked ? asked : (1u << 28), items);
    size_t free_b = 0, total_b = 0;
    if (!asked && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const size_t avail = (free_b + held) * 7 / 10, budget = avail > set_aside ? avail - set_aside : 0;
        while (P > (1u << 20) && (size_t)P * slot_bytes > budget) P >>= 1;
    }
    return P;
}
// kQueues queues of queue_cap slots, filled 512 at a time in turn (k_generate, the imports): a pool is a multiple of 512 * kQueues slots
static uint32_t pool_grain(uint32_t P) {
    constexpr uint32_t kGrain = 512u * rtk::kQueues;
    return std::max<uint32_t>(kGrain, (uint32_t)std::min<uint64_t>(((uint64_t)P + kGrain - 1u) / kGrain * kGrain, 0xFFFFF000ull));
}

// The context's counter block. Every counter the workgroups hit with atomics has a 128-byte line of its own, one per queue: four groups of
// kQueues lines, then the 16 64-bit statistics (kernels.h CTR_*). Group 0 is unused since round 3 (it held the queues' next-work-item
// counters; a path now finds its next item by itself, kernels.h RenderDev::lineage), group 1 holds the queue heads, groups 2 and 3 the
// sizes of the two pools. A chunk loop has one pool: count[0] is its queues' sizes, count[1] what k_extend zeroes for a k_shade that never runs.
struct CounterBlock {
    static constexpr size_t kLine = 128, kGroup = rtk::kQueues * kLine, kQueueLines = 4 * kGroup, kStats = sizeof(unsigned long long) * rtk::CTR_COUNT;
    static_assert(rtk::kQStride * sizeof(uint32_t) == kLine, "queue counters are one line apart");
    char* base = nullptr; hipStream_t stream = nullptr;
    uint32_t* head = nullptr; uint32_t* count[2] = {nullptr, nullptr}; unsigned long long* c64 = nullptr;
    hipError_t ensure(RtCtx* ctx) {
        const hipError_t e = ctx->counters.ensure(kQueueLines + kStats);
        if (e != hipSuccess) return e;
        base = (char*)ctx->counters.p; stream = ctx->stream;
        head = (uint32_t*)(base + 1 * kGroup); count[0] = (uint32_t*)(base + 2 * kGroup); count[1] = (uint32_t*)(base + 3 * kGroup);
        c64 = (unsigned long long*)(base + kQueueLines);
        return hipSuccess;
    }
    hipError_t zero_all() const { return hipMemsetAsync(base, 0, kQueueLines + kStats, stream); }
    hipError_t zero_queue_lines() const { return hipMemsetAsync(base, 0, kQueueLines, stream); }   // between chunks: heads and sizes go, the statistics stay
    hipError_t read_stats(RtCtx* ctx) const { return hipMemcpyAsync(ctx->h_counters, c64, kStats, hipMemcpyDeviceToHost, stream); }
};

// Device times of a call's kernels: events on the context's stream (the context keeps them for the next call), spans between two of them
// with a kind of the caller's choosing, and after the call's final synchronise the milliseconds of every kind.
struct StreamTimer {
    RtCtx* ctx; size_t used = 0;
    struct Span { hipEvent_t a, b; int kind; };
    std::vector<Span> spans;
    hipError_t mark(hipEvent_t& ev) {
        if (used == ctx->events.size()) { hipEvent_t e; hipError_t r = hipEventCreate(&e); if (r != hipSuccess) return r; ctx->events.push_back(e); }
        ev = ctx->events[used++];
        return hipEventRecord(ev, ctx->stream);
    }
    void span(hipEvent_t a, hipEvent_t b, int kind) { spans.push_back({a, b, kind}); }
    void sum(double* ms_by_kind) const { for (const Span& s : spans) { float ms = 0.f; if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) ms_by_kind[s.kind] += ms; } }
};

// the part of RtStats that the scene and the launch configuration decide, the same after every kind of call
static void scene_stats(RtStats* stats, const RtScene* scene, const uint32_t extend_geometry[2]) {
    stats->debug[6] = extend_geometry[0]; stats->debug[7] = extend_geometry[1];   // k_extend: threads per workgroup, resident workgroups per CU
    stats->n_devices = 1u; stats->lds_top_nodes = scene->dev.n_top;
    stats->scene_nodes = scene->n_nodes; stats->scene_prims = scene->n_prims; stats->scene_bytes = scene->bytes; stats->bvh_in_lds = scene->in_lds ? 1u : 0u;
}

// the launch configuration a scene's kernels take on this context; extend_geometry receives what k_extend was launched with (scene_stats)
static rtk::LaunchCfg scene_launch_cfg(const RtCtx* ctx, const RtScene* scene, uint32_t extend_geometry[2]) {
    rtk::LaunchCfg cfg{};
    cfg.n_cu = (uint32_t)ctx->n_cu; cfg.extend_geometry = extend_geometry; cfg.features = scene->features; cfg.scene_in_lds = scene->in_lds;
    return cfg;
}
// the queue geometry of a pool of P slots (pool_grain): all kQueues queues, each with its share of the slots
static void set_queue_geometry(rtk::RenderDev& rd, uint32_t P) { rd.queue_cap = P / rtk::kQueues; rd.q_lo = 0u; rd.q_n = rtk::kQueues; rd.q_shift = rtk::kQShift; }
// what an export scans of every queue after a chunk of n rays: a queue holds at most its share of the chunk's 512-ray groups
static uint32_t export_bound(uint32_t queue_cap, uint32_t n) { return std::min<uint32_t>(queue_cap, ((n + 511u) / 512u + rtk::kQueues - 1u) / rtk::kQueues * 512u); }
// The end of a chunk loop: the counters come back and the host waits, once per call. Then what every kind of call reports: the times of
// its kernels by the kinds of its spans, the segments, the k_extend launches, the pool, the scene's part and the wall time since t_begin.
static int finish_call(RtCtx* ctx, const CounterBlock& cb, const StreamTimer& tm, double* part_ms, std::chrono::steady_clock::time_point t_begin, const RtScene* scene,
                       const rtk::LaunchCfg& cfg, uint32_t P, uint32_t launched, RtStats* stats) {
    HIP_TRY(ctx, cb.read_stats(ctx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!stats) return RT_OK;
    stats->render_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    tm.sum(part_ms);
    stats->segments = ctx->h_counters[rtk::CTR_SEGMENTS];
    stats->extend_launches = launched; stats->pool_slots = P;
    scene_stats(stats, scene, cfg.extend_geometry);
    return RT_OK;
}

// camera, frame, seed, background and tiling: what new_camera_ray and the slot <-> pixel decodes of every kernel read (kernels.h RenderDev)
static rtk::RenderDev frame_render_dev(const RtScene* scene, const RtCamera* cam, const RtParams* prm, const Tiling& tl) {
    rtk::RenderDev rd{};
    auto cp3 = [](float* d, const RtVec3& v) { d[0] = (float)v.x; d[1] = (float)v.y; d[2] = (float)v.z; };
    cp3(rd.cam_origin, cam->origin); cp3(rd.cam_llc, cam->lower_left_corner); cp3(rd.cam_horizontal, cam->horizontal); cp3(rd.cam_vertical, cam->vertical);
    cp3(rd.cam_u, cam->u); cp3(rd.cam_v, cam->v);
    rd.cam_lens_radius = (float)cam->lens_radius; rd.cam_time0 = (float)cam->time0; rd.cam_time1 = (float)cam->time1;
    rd.width = prm->width; rd.height = prm->height; rd.seed = prm->seed;
    rd.bg_mode = scene->bg_mode; for (int i = 0; i < 3; ++i) rd.bg[i] = scene->bg[i];
    rd.tile_size = tl.ts; rd.tiles_x = tl.tiles_x; rd.tiles_y = tl.tiles_y; rd.n_local_tiles = tl.n_local;
    rd.shard_count = prm->shard_count <= 1u ? 1u : prm->shard_count; rd.shard_index = prm->shard_count <= 1u ? 0u : prm->shard_index;
    rd.div_width = rtk::make_fastdiv(prm->width); rd.div_ts = rtk::make_fastdiv(tl.ts); rd.div_ts2 = rtk::make_fastdiv(tl.ts * tl.ts); rd.div_tiles_x = rtk::make_fastdiv(tl.tiles_x);
    return rd;
}

// The tail of a wavefront loop goes to the drain kernel: once at most this many paths are alive, ONE launch carries each of them to its end
// (kernels.hip DRAIN). `fused` (RT_FLAG_FUSED) hands the whole render to it (a diagnostic: bit-identical frame, slower).
// Measured on the bench workload (LDS-resident scene): hand-over at 2^18 paths 103.2 ms, never 104.1, at 2^21 106.5, at 2^24 121. Scene in
// HBM (config-5 stand-in, 2048^2 x 32, near-first record orders): 2^18 126.0 ms, 2^20 126.2, 2^21 131.7, 2^22 143.4, 2^24 193.8. (With ONE
// record order a k_extend launch of that scene did not get shorter than 1.5-2 ms however few rays it carried — the longest far-first walk
// of the launch — and 2^21 was the best hand-over: 185.9 ms against 211.5 at 2^18.)
static uint32_t drain_threshold(const RtScene* scene, uint32_t tail_paths, bool fused) {
    uint32_t drain_at = tail_paths ? tail_paths : (1u << 18);                    // RtParams.tail_paths (1 = never: a pool holds 8 queues of >= 1 path)
    // the 8-wide walk resolves hits that tie within rounding in its own way; handing a tail to the per-path kernel (binary records) would
    // make such pixels depend on WHEN the hand-over happens, so a wide scene's wavefront loop runs to its end
    if (scene->dev.wide != nullptr) drain_at = 0u;
    if (fused) drain_at = 0xFFFFFFFFu;
    return drain_at;
}

// The wavefront loop over the pool's kQueues queues, from a first fill of n_init paths in pd[0] (whose queue sizes are in cb.count[0]) until no
// path is alive: launch pairs of k_extend and k_shade, then the drain (render_impl and radiance_impl; rd is the pass's RenderDev).
// launched += the launch pairs; drained = the bound of the paths handed to the drain kernel (0: the loop ran to its end).
// The host never waits for an iteration it has just enqueued: the kernels read the pool size from device memory and size-check
// themselves, so the host only needs (a) an UPPER BOUND of the pool size to size k_shade's grid and (b) to learn that it has
// reached 0. After every iteration the size is copied to a pinned ring slot behind an event; before enqueuing the next
// iteration the host takes whatever copies have landed (the size never grows, so an older value is a valid bound) and blocks
// only when it is kAhead iterations ahead. (Batches of 4, 8, 16, 32 iterations with a blocking read in between sized eight
// launches of k_shade by the 268 M paths of the start while 5 M were alive — 0.6 ms each for empty workgroups.)
static int wavefront_loop(RtCtx* ctx, const RtScene* scene, const rtk::RenderDev& rd, const rtk::PoolDev pd[2], const CounterBlock& cb, rtk::LaunchCfg& cfg, StreamTimer& tm,
                          bool timing, bool counting, uint32_t drain_at, uint32_t n_init, uint32_t& launched, uint32_t& drained) {
    constexpr uint32_t kAhead = 3, kRing = 4;
    // upper bound of the size of the LARGEST queue from here on (a queue never grows): it sizes the grids, and 0 ends the render
    uint32_t live = std::min<uint32_t>(rd.queue_cap, (n_init + rtk::kQueues - 1u) / rtk::kQueues + 512u);
    uint32_t iterations = 0u;
    int cur = 0;
    struct Pending { hipEvent_t ev; uint32_t ring; };
    std::vector<Pending> pending; size_t head = 0;
    auto take = [&](const Pending& pd_) {
        uint32_t m = 0; for (uint32_t k = 0; k < rtk::kQueues; ++k) m = std::max(m, ctx->h_count[pd_.ring * rtk::kQueues + k]);
        live = std::min(live, m);
    };
    for (;;) {
        while (head < pending.size() && hipEventQuery(pending[head].ev) == hipSuccess) take(pending[head++]);
        if (live != 0u && pending.size() - head >= kAhead) {
            HIP_TRY(ctx, hipEventSynchronize(pending[head].ev));
            take(pending[head++]);
        }
        if (live == 0u) break;
        if ((uint64_t)live * rtk::kQueues <= drain_at) {
            hipEvent_t ea = nullptr, eb = nullptr;
            if (timing) HIP_TRY(ctx, tm.mark(ea));
            LAUNCH_TRY(rtk::launch_drain(cfg, scene->dev, pd[cur], rd, live, cb.count[cur], cb.head, cb.count[1 - cur], cb.c64, counting, ctx->stream));
            if (timing) { HIP_TRY(ctx, tm.mark(eb)); tm.span(ea, eb, 3); }
            drained = live * rtk::kQueues;
            break;
        }
        hipEvent_t ea = nullptr, eb = nullptr, ec = nullptr;
        if (timing) HIP_TRY(ctx, tm.mark(ea));
        cfg.max_rays = (uint32_t)std::min<uint64_t>((uint64_t)live * rtk::kQueues, 0xFFFFFFFFull);
        LAUNCH_TRY(rtk::launch_extend(cfg, scene->dev, pd[cur], rd, cb.count[cur], cb.head, cb.count[1 - cur], cb.c64, counting, ctx->stream));
        if (timing) HIP_TRY(ctx, tm.mark(eb));
        HIP_TRY(ctx, rtk::launch_shade(cfg, scene->dev, pd[cur], pd[1 - cur], rd, live, cb.count[cur], cb.count[1 - cur], cb.head, cb.c64, counting, ctx->stream));
        if (timing) { HIP_TRY(ctx, tm.mark(ec)); tm.span(ea, eb, 0); tm.span(eb, ec, 1); }
        cur = 1 - cur;
        const uint32_t ring = iterations % kRing;
        HIP_TRY(ctx, hipMemcpy2DAsync(ctx->h_count + ring * rtk::kQueues, sizeof(uint32_t), cb.count[cur], CounterBlock::kLine, sizeof(uint32_t), rtk::kQueues, hipMemcpyDeviceToHost,
                                      ctx->stream));   // the kQueues pool sizes, one per line
        hipEvent_t ev = nullptr;
        HIP_TRY(ctx, tm.mark(ev));
        pending.push_back({ev, ring});
        ++launched;
        if (++iterations > 100000000u) return set_err(ctx, RT_ERR_DEVICE, "render loop did not terminate");
    }
    return RT_OK;
}

static int render_impl(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, const RtPassOptions& pass, void* d_out, void* d_sq, RtStats* stats,
                       const ListPass* lp) {
    using clk = std::chrono::steady_clock;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Tiling tl; make_tiling(*prm, tl);
    rtk::RenderDev rd = frame_render_dev(scene, cam, prm, tl);
    const uint32_t sc = rd.shard_count, si = rd.shard_index;
    // a pass renders samples first_sample .. first_sample + samples_per_pixel - 1: rd.spp is its END (absolute), n_blocks its items per pixel
    rd.spp = pass.first_sample + prm->samples_per_pixel; rd.max_depth = prm->max_depth; rd.nan_policy = prm->nan_policy;
    rd.first_sample = pass.first_sample; rd.accumulate = (pass.flags & RT_PASS_ACCUMULATE) ? 1u : 0u; rd.sq_sum = (float*)d_sq;
    // in-image pixels per local tile (edge tiles are clipped) -> prefix table
    std::vector<uint32_t> prefix(tl.n_local + 1, 0u);
    uint64_t valid_pixels = 0;
    for (uint32_t lt = 0; lt < tl.n_local; ++lt) {
        const uint32_t tile = si + lt * sc, tx = tile % tl.tiles_x, ty = tile / tl.tiles_x;
        const uint32_t w = std::min(tl.ts, prm->width - tx * tl.ts), h = std::min(tl.ts, prm->height - ty * tl.ts);
        valid_pixels += (uint64_t)w * h;
        if (valid_pixels > 0xFFFFFFFFull) return set_err(ctx, RT_ERR_INVALID, "more than 2^32 - 1 pixels in one shard (shard the image further)");
        prefix[lt + 1] = (uint32_t)valid_pixels;
    }
    // samples per work item: the frame's grouping (frame_block_shift); the pass starts on an item boundary (check_pass)
    const uint32_t block_shift = frame_block_shift(*prm, pass.frame_samples);
    rd.block_shift = block_shift; rd.n_blocks = (prm->samples_per_pixel + (1u << block_shift) - 1) >> block_shift;
    const uint64_t total_items = (lp ? (uint64_t)lp->n : valid_pixels) * rd.n_blocks;
    if (total_items >= kMaxItems) return set_err(ctx, RT_ERR_INVALID, "too many work items for one shard (image too large)");
    rd.total_items = (uint32_t)total_items;
    {   // launch-invariant divisors of the item -> (tile, pixel, sample) decode, and how far clipped edge tiles can move a tile index
        const uint64_t ts2 = (uint64_t)tl.ts * tl.ts, item_tile = ts2 * rd.n_blocks;
        rd.div_nblocks = rtk::make_fastdiv(rd.n_blocks); rd.div_shards = rtk::make_fastdiv(sc); rd.div_sq_row = rtk::make_fastdiv(std::max(1u, tl.ts >> 3));
        const bool fits = item_tile <= 0xFFFFFFFFull;
        rd.div_item_tile = rtk::make_fastdiv(fits ? (uint32_t)item_tile : 0xFFFFFFFFu);
        const uint64_t clipped = (uint64_t)tl.n_local * ts2 - valid_pixels;
        rd.tile_slack = fits ? (uint32_t)std::min<uint64_t>(tl.n_local, clipped / ts2 + 1) : tl.n_local;
        // one device, every tile: item -> tile by arithmetic (kernels.h RenderDev::row_items)
        const uint64_t row_items = (uint64_t)tl.ts * prm->width * rd.n_blocks;
        const bool by_rows = sc == 1u && fits && row_items <= 0xFFFFFFFFull;
        rd.row_items = by_rows ? (uint32_t)row_items : 0u;
        // any shard whose tiles all lie inside the image: the table is a multiplication (the 4096^2 strong-scaling frame at every shard count)
        rd.tiles_all_full = fits && clipped == 0 ? 1u : 0u;
        rd.div_row_items = rtk::make_fastdiv(by_rows ? (uint32_t)row_items : 1u);
    }

    if (stats) { std::memset(stats, 0, sizeof(*stats)); }
    const auto t_begin = clk::now();
    if (total_items == 0) { if (stats) stats->render_ms = 0.0; return RT_OK; }

    // Pool: as many paths in flight as there are work items, up to 2^28 (45 GB for the two pools) and to what the
    // device has free. Launches then carry hundreds of millions of rays: few launches, short tails.
    // Both pools and blocksum count as held; blocksum (16 bytes per item, whatever the pool's size) is set aside.
    const int n_arrays = block_shift ? 6 : 5;
    uint32_t P = pool_size(prm->pool_slots, total_items, 2 * pool_slot_bytes(n_arrays), ctx->blocksum.bytes + pool_held_bytes(ctx, 0, 6) + pool_held_bytes(ctx, 1, 6),
                            (size_t)total_items * 16);
    // Every slot of the first fill owns a LINEAGE of work items — w, w + P, w + 2P, ... — which its path works through one after the other
    // (kernels.h RenderDev::lineage). So that all lineages are equally long (and the pool stays full until the last generation), P is
    // not the cap itself but total / k for the smallest k that fits the cap: 480 M items under a cap of 2^28 run as 2 x 240 M.
    if (!prm->pool_slots && P < total_items) { const uint64_t k = (total_items + P - 1u) / P; P = (uint32_t)((total_items + k - 1u) / k); }
    P = pool_grain(P);
    set_queue_geometry(rd, P);
    rtk::PoolDev pd[2];
    for (int k = 0; k < 2; ++k) { const int r = pool_bind(ctx, k, P, n_arrays, pd[k]); if (r != RT_OK) return r; }
    HIP_TRY(ctx, ctx->blocksum.ensure((size_t)total_items * 16));
    rd.blocksum = (rtd::Float4*)ctx->blocksum.p;
    HIP_TRY(ctx, ctx->tile_prefix.ensure(prefix.size() * 4));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->tile_prefix.p, prefix.data(), prefix.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // `prefix` is a stack vector
    rd.tile_prefix = (const uint32_t*)ctx->tile_prefix.p;
    if (lp) {   // list pass: work item w = blk * n + i renders block blk of slot list[i]; list_map[slot] = i takes a finished item back (kernels.hip item_slot)
        HIP_TRY(ctx, ctx->list_map.ensure((size_t)tl.n_local * tl.ts * tl.ts * 4u));
        HIP_TRY(ctx, rtk::launch_list_map(lp->list, lp->n, (uint32_t*)ctx->list_map.p, ctx->stream));
        rd.list = lp->list; rd.n_list = lp->n; rd.list_map = (const uint32_t*)ctx->list_map.p; rd.div_list = rtk::make_fastdiv(lp->n); rd.counts = lp->counts;
    }
    CounterBlock cb;
    HIP_TRY(ctx, cb.ensure(ctx));
    HIP_TRY(ctx, cb.zero_all());

    const bool counting = (prm->flags & RT_FLAG_COUNTERS) != 0, timing = (prm->flags & RT_FLAG_TIMING) != 0;
    uint32_t extend_geometry[2] = {0u, 0u};
    rtk::LaunchCfg cfg = scene_launch_cfg(ctx, scene, extend_geometry);

    StreamTimer tm{ctx};

    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (timing) HIP_TRY(ctx, tm.mark(e0));
    const uint32_t n_init = (uint32_t)std::min<uint64_t>(P, total_items);
    rd.n_init = n_init; rd.lineage = P;
    // the ground sphere tested where a ray is made (kernels.h RenderDev::first_in_shade): a scene without motion, one such sphere, no counting
    rd.first_in_shade = scene->first_id != 0u && rtk::can_test_first_in_shade(scene->features) && !counting ? 1u : 0u;
    rd.first_id = scene->first_id; for (int k = 0; k < 8; ++k) rd.first_prim[k] = scene->first_prim[k];
    // Camera lists (kernels.h RenderDev::cam_lists), rebuilt for this camera and frame: the sphere-only instances over a scene in LDS, not while
    // counting (the counts are the walk's), not for the fused diagnostic, and a finite camera. Keyed by the global pixel, so a shard, a pass
    // and a pixel list use the same lists. Otherwise the render is what it was.
    ctx->cam_squares = 0u;
    if (scene->n_cam_order != 0u && scene->in_lds && rtk::camera_lists_fit(scene->features) && !counting &&
        (prm->flags & (RT_FLAG_FUSED | RT_FLAG_NO_CAMERA_LISTS)) == 0u && camera_is_finite(cam)) {
        rtk::CamListsDev cl{};
        cl.cam = camera_lists_camera(cam, prm->width, prm->height);
        cl.n_squares = rtcl::squares_x(prm->width) * rtcl::squares_y(prm->height);
        HIP_TRY(ctx, ctx->cam_lists.ensure((size_t)cl.n_squares * rtcl::kListWords * 4u));
        cl.spheres = (const float*)scene->dev.spheres; cl.order = (const uint32_t*)scene->cam_order.p; cl.n_order = scene->n_cam_order; cl.lists = (uint32_t*)ctx->cam_lists.p;
        LAUNCH_TRY(rtk::launch_camera_lists(cl, ctx->stream));
        rd.cam_lists = cl.lists; rd.cam_squares_x = rtcl::squares_x(prm->width); rd.cam_spheres = scene->dev.spheres;
        ctx->cam_squares = cl.n_squares;
        // In-place camera shading (kernels.h RenderDev::cam_shade): only where the shade of a camera ray that hit a sphere always leaves a path
        // that goes on — it cannot reach the depth limit (max_depth >= 2) and cannot end on an emitter (no DiffuseLight sphere; a throughput that
        // is not finite still scatters) — so the first fill gets no holes. The mark of such a record is the sign of its time slot (kRayShaded):
        // that slot is the first sphere's t, or the camera's time, which then must not be negative.
        if (prm->max_depth >= 2u && !scene->sphere_emits && (rd.first_in_shade != 0u || (rd.cam_time0 >= 0.f && rd.cam_time1 >= 0.f))) rd.cam_shade = RT_CAMERA_SHADE;
    }
    HIP_TRY(ctx, rtk::launch_generate(scene->dev, pd[0], rd, n_init, cb.count[0], ctx->stream));
    if (timing) { HIP_TRY(ctx, tm.mark(e1)); tm.span(e0, e1, 2); }
    uint32_t launched = 0u, drained = 0u;
    { const int r = wavefront_loop(ctx, scene, rd, pd, cb, cfg, tm, timing, counting, drain_threshold(scene, prm->tail_paths, (prm->flags & RT_FLAG_FUSED) != 0u), n_init, launched, drained);
      if (r != RT_OK) return r; }
    hipEvent_t r0 = nullptr, r1 = nullptr;
    if (timing) HIP_TRY(ctx, tm.mark(r0));
    if (sc > 1 && !rd.accumulate && !lp) {   // clipped pixels of edge tiles stay 0 (an accumulating pass finds them 0 from its first pass; a list pass writes listed slots only)
        HIP_TRY(ctx, hipMemsetAsync(d_out, 0, (size_t)tl.n_local * tl.ts * tl.ts * 3 * sizeof(float), ctx->stream));
        if (d_sq) HIP_TRY(ctx, hipMemsetAsync(d_sq, 0, (size_t)tl.n_local * tl.ts * tl.ts * 3 * sizeof(float), ctx->stream));
    }
    if (lp) HIP_TRY(ctx, rtk::launch_resolve_list(rd, (float*)d_out, ctx->stream));
    else HIP_TRY(ctx, rtk::launch_resolve(rd, (float*)d_out, (uint32_t)valid_pixels, ctx->stream));
    if (timing) { HIP_TRY(ctx, tm.mark(r1)); tm.span(r0, r1, 2); }
    // the segments shaded where their camera ray was made stood in no queue: k_shade counted them into the word behind every queue size
    // (kernels.h kRayShaded). The wavefront loop has read its last ring slot by now, so the ring (4 x kQueues words) takes the 2 x kQueues.
    if (rd.cam_shade != 0u && stats)
        HIP_TRY(ctx, hipMemcpy2DAsync(ctx->h_count, sizeof(uint32_t), cb.count[0] + 1, CounterBlock::kLine, sizeof(uint32_t), 2u * rtk::kQueues, hipMemcpyDeviceToHost, ctx->stream));
    double part_ms[4] = {0.0, 0.0, 0.0, 0.0};                         // extend, shade, generate and resolve, drain
    { const int r = finish_call(ctx, cb, tm, part_ms, t_begin, scene, cfg, P, launched, stats); if (r != RT_OK) return r; }
    if (stats) {
        if (rd.cam_shade != 0u) for (uint32_t k = 0; k < 2u * rtk::kQueues; ++k) stats->segments += ctx->h_count[k];
        stats->extend_ms = part_ms[0]; stats->shade_ms = part_ms[1]; stats->other_ms = part_ms[2]; stats->drain_ms = part_ms[3];
        stats->samples = (lp ? (uint64_t)lp->n : valid_pixels) * prm->samples_per_pixel;
#if defined(RT_STAMPS) || defined(RT_SHADE_STAMPS)
        const bool copy_counts = true;    // k_extend's pass statistics travel in these slots (scripts/gpu_stamps.py)
#else
        const bool copy_counts = counting;
#endif
        if (copy_counts) {
            stats->node_tests = ctx->h_counters[rtk::CTR_NODE_TESTS];
            for (int k = 0; k < RT_N_PRIM_TYPES; ++k) stats->prim_tests[k] = ctx->h_counters[rtk::CTR_PRIM_TESTS + k];
        }
        for (int k = 0; k < 5; ++k) stats->debug[k] = ctx->h_counters[rtk::CTR_DEBUG + k];
#ifdef RT_STAMPS
        stats->debug[5] = ctx->h_counters[rtk::CTR_SAMPLES];       // node steps of all waves (scripts/gpu_stamps.py)
#endif
        stats->iterations = (uint32_t)ctx->h_counters[rtk::CTR_ITERATIONS]; stats->shade_launches = launched; stats->drain_paths = drained;
    }
    return RT_OK;
}

int rt_pass_check(const RtParams* params, const RtPassOptions* options, uint32_t* out_samples_per_item) {
    uint32_t shift = 0;
    const int r = check_pass(nullptr, params, options, &shift);
    if (r != RT_OK) return r;
    if (out_samples_per_item) *out_samples_per_item = 1u << shift;
    return RT_OK;
}

int rt_render_pass_device(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, const RtPassOptions* options, void* rgb_sum_device,
                          void* sq_sum_device, RtStats* stats) {
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    if (!scene || !cam || !rgb_sum_device) return set_err(ctx, RT_ERR_INVALID, "scene / cam / output is null");
    const int v = check_pass(ctx, prm, options, nullptr); if (v != RT_OK) return v;
    return render_pass_checked(ctx, scene, cam, prm, *options, rgb_sum_device, sq_sum_device, stats);
}

int rt_render_pass(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, const RtPassOptions* options, float* rgb_sum_host,
                   float* sq_sum_host, RtStats* stats) {
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    if (!scene || !cam || !rgb_sum_host) return set_err(ctx, RT_ERR_INVALID, "scene / cam / output is null");
    const int v = check_pass(ctx, prm, options, nullptr); if (v != RT_OK) return v;
    uint64_t n = 0; rt_output_floats(prm, &n);
    const size_t bytes = n * sizeof(float);
    const bool acc = (options->flags & RT_PASS_ACCUMULATE) != 0u;   // the fold then goes on from the caller's sums
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return staged_call(ctx, {{&ctx->out_tmp, acc ? rgb_sum_host : nullptr, rgb_sum_host, bytes}, {&ctx->sq_tmp, acc ? sq_sum_host : nullptr, sq_sum_host, bytes}}, stats,
                       [&] { return render_pass_checked(ctx, scene, cam, prm, *options, ctx->out_tmp.p, sq_sum_host ? ctx->sq_tmp.p : nullptr, stats); });
}

// ---- adaptive sampling (include/rt_hip.h): selection of the active list, passes over a pixel list, per-pixel write_color ----------------
static int check_adaptive(RtCtx* ctx, const RtParams* p, const RtAdaptiveOptions* o, uint32_t first_sample, uint32_t frame_samples, uint32_t* samples_per_item) {
    const int v = validate_params(ctx, p); if (v != RT_OK) return v;
    if (!o) return set_err(ctx, RT_ERR_INVALID, "adaptive options are null");
    const int h = check_header(ctx, o->struct_bytes, sizeof(RtAdaptiveOptions), "RtAdaptiveOptions"); if (h != RT_OK) return h;
    if (!(std::isfinite(o->rel_error) && o->rel_error >= 0.0)) return set_err(ctx, RT_ERR_INVALID, "RtAdaptiveOptions.rel_error must be finite and >= 0");
    if (!(std::isfinite(o->abs_error) && o->abs_error >= 0.0)) return set_err(ctx, RT_ERR_INVALID, "RtAdaptiveOptions.abs_error must be finite and >= 0");
    if (frame_samples == 0u) return set_err(ctx, RT_ERR_INVALID, "frame_samples must be >= 1");
    if (first_sample > frame_samples) return set_err(ctx, RT_ERR_INVALID, "first_sample is beyond frame_samples");
    const uint32_t m = 1u << frame_block_shift(*p, frame_samples);
    if ((uint64_t)o->min_samples < 2ull * m)
        return set_err(ctx, RT_ERR_INVALID, "RtAdaptiveOptions.min_samples must be >= 2 work items (" + std::to_string(2ull * m) + " samples for this frame)");
    if (first_sample & (m - 1u)) return set_err(ctx, RT_ERR_INVALID, "first_sample is not a multiple of the samples per work item (" + std::to_string(m) + " for this frame)");
    if (samples_per_item) *samples_per_item = m;
    return RT_OK;
}

int rt_adaptive_check(const RtParams* params, const RtAdaptiveOptions* options, uint32_t first_sample, uint32_t frame_samples) {
    return check_adaptive(nullptr, params, options, first_sample, frame_samples, nullptr);
}

static uint32_t output_slots(const RtParams* p) { uint64_t n = 0; rt_output_floats(p, &n); return (uint32_t)(n / 3u); }

int rt_adaptive_select(RtCtx* ctx, const RtParams* prm, const RtAdaptiveOptions* options, uint32_t first_sample, uint32_t frame_samples, const void* rgb_sum_device,
                       const void* sq_sum_device, const void* counts_device, void* pixels_device_out, uint32_t* n_out) {
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    if (!rgb_sum_device || !sq_sum_device || !counts_device || !pixels_device_out || !n_out) return set_err(ctx, RT_ERR_INVALID, "a buffer or n_out is null");
    uint32_t m = 1u;
    const int v = check_adaptive(ctx, prm, options, first_sample, frame_samples, &m); if (v != RT_OK) return v;
    *n_out = 0u;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Tiling tl; make_tiling(*prm, tl);
    rtk::SelectArgs a{};
    a.rgb = (const float*)rgb_sum_device; a.sq = (const float*)sq_sum_device; a.counts = (const uint32_t*)counts_device;
    a.slots = output_slots(prm); a.first_sample = first_sample; a.frame_samples = frame_samples; a.m = m; a.min_samples = options->min_samples;
    a.rel_error = options->rel_error; a.abs_error = options->abs_error;
    a.width = prm->width; a.height = prm->height; a.shard_count = prm->shard_count <= 1u ? 1u : prm->shard_count; a.shard_index = prm->shard_count <= 1u ? 0u : prm->shard_index;
    a.tile_size = tl.ts; a.tiles_x = tl.tiles_x;
    if (a.slots == 0u) return RT_OK;   // a shard that owns no tile: no kernel runs, so no count comes back (the word holds an earlier call's)
    const size_t n_waves = (a.slots + 63u) / 64u;
    HIP_TRY(ctx, ctx->sel_masks.ensure(n_waves * 8u));
    HIP_TRY(ctx, ctx->sel_offsets.ensure(n_waves * 4u));
    HIP_TRY(ctx, ctx->adaptive_word.ensure(4u));
    HIP_TRY(ctx, rtk::launch_select(a, (unsigned long long*)ctx->sel_masks.p, (uint32_t*)ctx->sel_offsets.p, (uint32_t*)pixels_device_out, (uint32_t*)ctx->adaptive_word.p,
                                    ctx->stream));
    uint32_t n = 0u;
    HIP_TRY(ctx, hipMemcpyAsync(&n, ctx->adaptive_word.p, 4u, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_out = n;
    return RT_OK;
}

// The device checks a pixel list before any kernel uses its entries as addresses: every entry an in-image slot, strictly ascending,
// counts[entry] == first_sample. RT_ERR_INVALID with the reason otherwise; nothing has been written then.
static int check_list(RtCtx* ctx, const RtParams* prm, const uint32_t* list, uint32_t n, const uint32_t* counts, uint32_t first_sample, uint32_t slots) {
    Tiling tl; make_tiling(*prm, tl);
    HIP_TRY(ctx, ctx->adaptive_word.ensure(4u));
    HIP_TRY(ctx, hipMemsetAsync(ctx->adaptive_word.p, 0, 4u, ctx->stream));
    HIP_TRY(ctx, rtk::launch_list_check(list, n, counts, first_sample, prm->width, prm->height, prm->shard_count <= 1u ? 1u : prm->shard_count,
                                        prm->shard_count <= 1u ? 0u : prm->shard_index, tl.ts, tl.tiles_x, slots, (uint32_t*)ctx->adaptive_word.p, ctx->stream));
    uint32_t verdict = 0u;
    HIP_TRY(ctx, hipMemcpyAsync(&verdict, ctx->adaptive_word.p, 4u, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (verdict == 0u) return RT_OK;
    std::string why = "pixel list:";
    if (verdict & 1u) why += " an entry is >= the number of output slots (" + std::to_string(slots) + ");";
    if (verdict & 8u) why += " an entry is a clipped slot of an edge tile, not an image pixel;";
    if (verdict & 2u) why += " the entries are not strictly ascending (or repeat);";
    if (verdict & 4u) why += " counts[entry] != first_sample for an entry (the pixel did not take every pass so far);";
    why.pop_back();
    return set_err(ctx, RT_ERR_INVALID, why);
}

int rt_render_pass_pixels_device(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, const RtPassOptions* options, const void* pixels_device,
                                 uint32_t n_pixels, void* rgb_sum_device, void* sq_sum_device, void* counts_device, RtStats* stats) {
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    if (!scene || !cam || !rgb_sum_device || !counts_device) return set_err(ctx, RT_ERR_INVALID, "scene / cam / output / counts is null");
    const int v = check_pass(ctx, prm, options, nullptr); if (v != RT_OK) return v;
    const uint32_t slots = output_slots(prm);
    if (n_pixels > slots) return set_err(ctx, RT_ERR_INVALID, "n_pixels is larger than the number of output slots (" + std::to_string(slots) + ")");
    if (n_pixels == 0u) { if (stats) std::memset(stats, 0, sizeof(*stats)); return RT_OK; }
    if (!pixels_device) return set_err(ctx, RT_ERR_INVALID, "pixel list is null");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int c = check_list(ctx, prm, (const uint32_t*)pixels_device, n_pixels, (const uint32_t*)counts_device, options->first_sample, slots);
    if (c != RT_OK) return c;
    const ListPass lp{(const uint32_t*)pixels_device, n_pixels, (uint32_t*)counts_device};
    return render_pass_checked(ctx, scene, cam, prm, *options, rgb_sum_device, sq_sum_device, stats, &lp);
}

int rt_resolve_counts_device(RtCtx* ctx, const void* rgb_sum_device, const void* counts_device, uint32_t width, uint32_t height, void* rgb8_device) {
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    if (!rgb_sum_device || !counts_device || !rgb8_device) return set_err(ctx, RT_ERR_INVALID, "bad argument");
    if (width == 0 || height == 0 || (uint64_t)width * height * 3u > 0xFFFFFFFFull) return set_err(ctx, RT_ERR_INVALID, "bad image size");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, rtk::launch_write_color_counts((const float*)rgb_sum_device, (const uint32_t*)counts_device, width * height, (uint8_t*)rgb8_device, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

// the one-shot entry points are the pass {first_sample 0, frame_samples spp, overwrite}: one code path
int rt_render_device(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, void* rgb_sum_device, RtStats* stats) {
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    if (!scene || !cam || !rgb_sum_device) return set_err(ctx, RT_ERR_INVALID, "scene / cam / output is null");
    if (!prm) return validate_params(ctx, prm);
    const RtPassOptions one = one_shot(prm);
    return rt_render_pass_device(ctx, scene, cam, prm, &one, rgb_sum_device, nullptr, stats);
}

int rt_render(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, float* rgb_sum_host, RtStats* stats) {
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    if (!scene || !cam || !rgb_sum_host) return set_err(ctx, RT_ERR_INVALID, "scene / cam / output is null");
    if (!prm) return validate_params(ctx, prm);
    const RtPassOptions one = one_shot(prm);
    return rt_render_pass(ctx, scene, cam, prm, &one, rgb_sum_host, nullptr, stats);
}

// ---- ray queries (include/rt_hip.h): caller's rays through the traversal kernels of a render, one RtRayHit each ---------------------------
static_assert(sizeof(RtRay) == 32 && sizeof(RtRayHit) == 48 && sizeof(RtRayQueryOptions) == 16, "ray query records: 32, 48 and 16 bytes");
static int check_ray_query(RtCtx* ctx, const RtRayQueryOptions* o, uint64_t n_rays) {
    if (o) { const int h = check_header(ctx, o->struct_bytes, sizeof(RtRayQueryOptions), "RtRayQueryOptions", o->flags, RT_FLAG_TIMING, "RT_FLAG_TIMING"); if (h != RT_OK) return h; }
    if (n_rays > 0xFFFFFFFFull) return set_err(ctx, RT_ERR_INVALID, "n_rays must be < 2^32 (split the list)");
    return RT_OK;
}
int rt_ray_query_check(const RtRayQueryOptions* options, uint64_t n_rays) { return check_ray_query(nullptr, options, n_rays); }

// The chunk loop: import -> k_extend (the scene's own launch configuration, every layout) -> export, all on the context's stream; the host
// waits once, at the end. A chunk's kernels read its queue sizes from device memory, so nothing comes back to the host in between.
// any_hit (rt_occluded_rays): the same loop with the occlusion kernels — its own import, the any-hit walk, the byte export; d_hits is then
// the caller's n_rays bytes.
static int trace_rays_impl(RtCtx* ctx, const RtScene* scene, const RtRayQueryOptions* opt, const void* d_rays, uint64_t n_rays, void* d_hits, RtStats* stats,
                           bool any_hit) {
    using clk = std::chrono::steady_clock;
    const auto t_begin = clk::now();
    const bool timing = opt && (opt->flags & RT_FLAG_TIMING) != 0u;
    // one pool, every ray in flight
    const uint32_t P = pool_grain(pool_size(opt ? opt->pool_slots : 0u, n_rays, pool_slot_bytes(5), pool_held_bytes(ctx, 0, 5), 0));
    const uint32_t queue_cap = P / rtk::kQueues;
    rtk::PoolDev pd{};
    { const int r = pool_bind(ctx, 0, P, 5, pd); if (r != RT_OK) return r; }
    CounterBlock cb;   // one pool: count[0] the queues' sizes, count[1] what k_extend zeroes for a k_shade that never runs here
    HIP_TRY(ctx, cb.ensure(ctx));
    HIP_TRY(ctx, cb.zero_all());

    rtk::RenderDev rd{};                     // a walk needs the queue geometry only; first_in_shade = 0: the record's time slot is the ray's time
    set_queue_geometry(rd, P);
    rd.div_nblocks = rtk::make_fastdiv(1u); rd.n_blocks = 1u;
    uint32_t extend_geometry[2] = {0u, 0u};
    rtk::LaunchCfg cfg = scene_launch_cfg(ctx, scene, extend_geometry);

    StreamTimer tm{ctx};
    uint32_t launched = 0u;
    for (uint64_t first = 0; first < n_rays; first += P) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(P, n_rays - first);
        hipEvent_t ea = nullptr, eb = nullptr, ec = nullptr, ed = nullptr;
        if (first != 0u) HIP_TRY(ctx, cb.zero_queue_lines());
        if (timing) HIP_TRY(ctx, tm.mark(ea));
        LAUNCH_TRY(rtk::launch_rays_import(d_rays, (uint32_t)first, n, pd, queue_cap, cb.count[0], d_hits, cb.c64, any_hit, !rtk::extend_any_is_closest(scene->dev), ctx->stream));
        if (timing) HIP_TRY(ctx, tm.mark(eb));
        cfg.max_rays = n;
        if (any_hit) LAUNCH_TRY(rtk::launch_extend_any(cfg, scene->dev, pd, rd, cb.count[0], cb.head, cb.count[1], cb.c64, ctx->stream));
        else LAUNCH_TRY(rtk::launch_extend(cfg, scene->dev, pd, rd, cb.count[0], cb.head, cb.count[1], cb.c64, false, ctx->stream));
        if (timing) HIP_TRY(ctx, tm.mark(ec));
        const uint32_t per_queue = export_bound(queue_cap, n);
        if (any_hit) LAUNCH_TRY(rtk::launch_occluded_export(pd, queue_cap, per_queue, cb.count[0], d_hits, ctx->stream));
        else LAUNCH_TRY(rtk::launch_rays_export(cfg, scene->dev, scene->src, pd, queue_cap, per_queue, cb.count[0], d_hits, ctx->stream));
        if (timing) { HIP_TRY(ctx, tm.mark(ed)); tm.span(ea, eb, 1); tm.span(eb, ec, 0); tm.span(ec, ed, 1); }
        ++launched;
    }
    double part_ms[2] = {0.0, 0.0};                                   // extend, import and export
    { const int r = finish_call(ctx, cb, tm, part_ms, t_begin, scene, cfg, P, launched, stats); if (r != RT_OK) return r; }
    if (stats) {
        stats->extend_ms = part_ms[0]; stats->other_ms = part_ms[1];
        stats->samples = stats->segments; stats->iterations = launched;
    }
    return RT_OK;
}

// The two kinds of query differ in the kernels (trace_rays_impl any_hit) and in what a ray's result is: an RtRayHit record, or one byte.
struct RayQueryKind { bool any_hit; size_t out_bytes; uintptr_t out_align; };
constexpr RayQueryKind kClosestHit{false, sizeof(RtRayHit), 16u}, kOcclusion{true, 1u, 1u};

// the argument checks of both variants: a refused call has written nothing. out_align: the alignment a device output needs
static int trace_rays_refuse(RtCtx* ctx, const RtScene* scene, const RtRayQueryOptions* options, const void* rays, uint64_t n_rays, const void* out, bool device,
                             uintptr_t out_align) {
    if (!scene) return set_err(ctx, RT_ERR_INVALID, "scene is null");
    const int v = check_ray_query(ctx, options, n_rays); if (v != RT_OK) return v;
    if (scene->features & rtk::F_MEDIUM)
        return set_err(ctx, RT_ERR_UNSUPPORTED, "ray queries: the scene holds a ConstantMedium, whose hit is a random draw keyed by a path; a bare ray has none");
    if (n_rays != 0u && (!rays || !out)) return set_err(ctx, RT_ERR_INVALID, "rays / hits is null");
    if (device && ((((uintptr_t)rays) & 15u) | (((uintptr_t)out) & (out_align - 1u)))) return set_err(ctx, RT_ERR_INVALID, "rays / hits must be 16-byte aligned");
    return RT_OK;
}

static int ray_query_device(RtCtx* ctx, const RtScene* scene, const RtRayQueryOptions* options, const void* rays_device, uint64_t n_rays, void* out_device, RtStats* stats,
                            const RayQueryKind& kind) {
    return query_entry(ctx, stats, n_rays == 0u, false, [&] { return trace_rays_refuse(ctx, scene, options, rays_device, n_rays, out_device, true, kind.out_align); },
                       [&] { return trace_rays_impl(ctx, scene, options, rays_device, n_rays, out_device, stats, kind.any_hit); });
}
// the host variant: the rays staged in, the device variant on the context's own buffers, the results staged out (host buffers are copied: no alignment asked)
static int ray_query_host(RtCtx* ctx, const RtScene* scene, const RtRayQueryOptions* options, const RtRay* rays_host, uint64_t n_rays, void* out_host, RtStats* stats,
                          const RayQueryKind& kind) {
    return query_entry(ctx, stats, n_rays == 0u, false, [&] { return trace_rays_refuse(ctx, scene, options, rays_host, n_rays, out_host, false, kind.out_align); }, [&] {
        return staged_call(ctx, {{&ctx->rays_tmp, rays_host, nullptr, (size_t)n_rays * sizeof(RtRay)}, {&ctx->hits_tmp, nullptr, out_host, (size_t)n_rays * kind.out_bytes}}, stats,
                           [&] { return ray_query_device(ctx, scene, options, ctx->rays_tmp.p, n_rays, ctx->hits_tmp.p, stats, kind); });
    });
}

int rt_trace_rays_device(RtCtx* ctx, const RtScene* scene, const RtRayQueryOptions* options, const void* rays_device, uint64_t n_rays, void* hits_device, RtStats* stats) {
    return ray_query_device(ctx, scene, options, rays_device, n_rays, hits_device, stats, kClosestHit);
}
int rt_trace_rays(RtCtx* ctx, const RtScene* scene, const RtRayQueryOptions* options, const RtRay* rays_host, uint64_t n_rays, RtRayHit* hits_host, RtStats* stats) {
    return ray_query_host(ctx, scene, options, rays_host, n_rays, hits_host, stats, kClosestHit);
}
// occlusion queries: the two entry points above with the any-hit kernels and one byte per ray
int rt_occluded_rays_device(RtCtx* ctx, const RtScene* scene, const RtRayQueryOptions* options, const void* rays_device, uint64_t n_rays, void* occluded_device, RtStats* stats) {
    return ray_query_device(ctx, scene, options, rays_device, n_rays, occluded_device, stats, kOcclusion);
}
int rt_occluded_rays(RtCtx* ctx, const RtScene* scene, const RtRayQueryOptions* options, const RtRay* rays_host, uint64_t n_rays, uint8_t* occluded_host, RtStats* stats) {
    return ray_query_host(ctx, scene, options, rays_host, n_rays, occluded_host, stats, kOcclusion);
}

// ---- light-sample queries (include/rt_hip.h): the scene's own light sampler, one RtLightSample per RtLightQuery ---------------------------------
// One kernel, one lane per query, no pool and no counters: the launch, timing and failure rules of the other query paths (the context's
// stream, StreamTimer under RT_FLAG_TIMING, drain_on_failure, one wait at the end).
static_assert(sizeof(RtLightQuery) == 40 && sizeof(RtLightSample) == 24 && sizeof(RtLightQueryOptions) == 8, "light query records: 40, 24 and 8 bytes");
static int light_query_refuse(RtCtx* ctx, const RtScene* scene, const RtLightQueryOptions* o, const void* queries, uint64_t n, const void* results, bool device) {
    if (!scene) return set_err(ctx, RT_ERR_INVALID, "scene is null");
    if (o) { const int h = check_header(ctx, o->struct_bytes, sizeof(RtLightQueryOptions), "RtLightQueryOptions", o->flags, RT_FLAG_TIMING, "RT_FLAG_TIMING"); if (h != RT_OK) return h; }
    if (n > 0xFFFFFFFFull) return set_err(ctx, RT_ERR_INVALID, "n must be < 2^32 (split the list)");
    const bool env_member = (scene->features & rtk::F_ENV) != 0u && scene->dev.env_sampled != 0u;   // a sampled map is a list by itself
    if (((scene->features & rtk::F_LIGHTS) == 0u || scene->dev.n_lights == 0u) && !env_member)
        return set_err(ctx, RT_ERR_UNSUPPORTED, "light-sample queries: the scene was uploaded without a lights list (RtSceneDesc.lights = -1)");
    if (n != 0u && (!queries || !results)) return set_err(ctx, RT_ERR_INVALID, "queries / results is null");
    if (device && ((((uintptr_t)queries) | ((uintptr_t)results)) & 7u)) return set_err(ctx, RT_ERR_INVALID, "queries / results must be 8-byte aligned");
    return RT_OK;
}
static int sample_lights_impl(RtCtx* ctx, const RtScene* scene, const RtLightQueryOptions* opt, const void* d_queries, uint64_t n, void* d_results, RtStats* stats) {
    using clk = std::chrono::steady_clock;
    const auto t_begin = clk::now();
    const bool timing = opt && (opt->flags & RT_FLAG_TIMING) != 0u;
    StreamTimer tm{ctx};
    hipEvent_t ea = nullptr, eb = nullptr;
    if (timing) HIP_TRY(ctx, tm.mark(ea));
    LAUNCH_TRY(rtk::launch_sample_lights(scene->dev, scene->features, d_queries, d_results, (uint32_t)n, ctx->stream));
    if (timing) { HIP_TRY(ctx, tm.mark(eb)); tm.span(ea, eb, 1); }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (stats) {
        double part_ms[2] = {0.0, 0.0};
        tm.sum(part_ms);
        stats->other_ms = part_ms[1];
        stats->samples = n;
        const uint32_t none[2] = {0u, 0u};
        scene_stats(stats, scene, none);
        stats->render_ms = std::chrono::duration<double, std::milli>(clk::now() - t_begin).count();
    }
    return RT_OK;
}
int rt_sample_lights_device(RtCtx* ctx, const RtScene* scene, const RtLightQueryOptions* options, const void* queries_device, uint64_t n, void* results_device, RtStats* stats) {
    return query_entry(ctx, stats, n == 0u, false, [&] { return light_query_refuse(ctx, scene, options, queries_device, n, results_device, true); },
                       [&] { return sample_lights_impl(ctx, scene, options, queries_device, n, results_device, stats); });
}
// (host buffers are copied: no alignment asked)
int rt_sample_lights(RtCtx* ctx, const RtScene* scene, const RtLightQueryOptions* options, const RtLightQuery* queries_host, uint64_t n, RtLightSample* results_host, RtStats* stats) {
    return query_entry(ctx, stats, n == 0u, false, [&] { return light_query_refuse(ctx, scene, options, queries_host, n, results_host, false); }, [&] {
        return staged_call(ctx, {{&ctx->rays_tmp, queries_host, nullptr, (size_t)n * sizeof(RtLightQuery)}, {&ctx->hits_tmp, nullptr, results_host, (size_t)n * sizeof(RtLightSample)}}, stats,
                           [&] { return rt_sample_lights_device(ctx, scene, options, ctx->rays_tmp.p, n, ctx->hits_tmp.p, stats); });
    });
}

// ---- radiance queries (include/rt_hip.h): caller's rays through the render's own path loop, per-ray sums over a sample range ------------------
static_assert(sizeof(RtPathRay) == 32 && sizeof(RtRadianceOptions) == 56, "radiance query records: 32 and 56 bytes");
// first_stream + n_rays may reach this: a path's 32-bit item id is stream * (samples in its chunk) + sample of the chunk (radiance_impl), and a
// chunk of one sample must be able to hold the call's last stream
constexpr uint64_t kMaxStreams = 0xFFFFFFFFull;
static int check_radiance(RtCtx* ctx, const RtRadianceOptions* o, uint64_t n_rays) {
    if (!o) return set_err(ctx, RT_ERR_INVALID, "radiance options are null");
    const int h = check_header(ctx, o->struct_bytes, sizeof(RtRadianceOptions), "RtRadianceOptions", o->flags, RT_RADIANCE_ACCUMULATE); if (h != RT_OK) return h;
    if (o->render_flags & ~(uint32_t)RT_FLAG_TIMING) return set_err(ctx, RT_ERR_INVALID, "RtRadianceOptions.render_flags holds an unknown bit (known: RT_FLAG_TIMING)");
    if (o->nan_policy > 1) return set_err(ctx, RT_ERR_INVALID, "bad nan_policy");
    if (o->samples == 0u) return set_err(ctx, RT_ERR_INVALID, "samples must be >= 1");
    if ((uint64_t)o->first_sample + o->samples > 0xFFFFFFFFull) return set_err(ctx, RT_ERR_INVALID, "first_sample + samples must be < 2^32");
    if (o->max_depth == 0 || o->max_depth > 255) return set_err(ctx, RT_ERR_INVALID, "max_depth must be in 1..255");
    if (n_rays > kMaxStreams || o->first_stream > kMaxStreams || o->first_stream + n_rays > kMaxStreams)
        return set_err(ctx, RT_ERR_INVALID, "first_stream + n_rays must be <= 2^32 - 1 (a stream index is 32 bits; split the list, or choose streams below that)");
    return RT_OK;
}
int rt_radiance_check(const RtRadianceOptions* options, uint64_t n_rays) { return check_radiance(nullptr, options, n_rays); }

// The chunk loop. A chunk — rays [r0, r0 + n) x samples [s0, s0 + sc) of the call — is a pixel-list pass of the render loop over a virtual
// unsharded frame 65536 pixels wide whose pixel index is the ray's stream (kernels.hip "radiance queries"): k_radiance_import fills the pool
// (no k_generate: the rays are the caller's), wavefront_loop runs it empty, k_resolve_list folds the chunk's item sums into the caller's
// sums. The list of such a pass is the run of streams [stream0, stream0 + n): rd.list is the iota table (entry i -> output slot i of the
// buffers offset to r0), and rd.list_map, which takes a stream back to its entry, is the same table addressed from stream0 entries before
// its start — never dereferenced outside [stream0, stream0 + n). Rays are chunked first and samples second, so that every path of a chunk
// is in flight at once (lineage = the chunk's items: nothing is ever regenerated) and (stream0 + n) * sc fits the 32-bit item id; a later
// sample chunk accumulates on the earlier ones, which continues the same sequential fold: the sums do not depend on the chunking.
static int radiance_impl(RtCtx* ctx, const RtScene* scene, const RtRadianceOptions* opt, const void* d_rays, uint64_t n_rays, void* d_rgb, void* d_sq, void* d_invalid,
                         RtStats* stats) {
    using clk = std::chrono::steady_clock;
    const auto t_begin = clk::now();
    const bool timing = (opt->render_flags & RT_FLAG_TIMING) != 0u;
    const uint32_t S = opt->samples;
    // the ray queries' pool rule over the call's items; per slot: both pools, the item's sum, and its share of the tables below
    const uint64_t items = n_rays * (uint64_t)S;
    const uint32_t P = pool_grain(pool_size(opt->pool_slots, items, 2 * pool_slot_bytes(5) + 16 + 8,
                                            ctx->blocksum.bytes + ctx->list_map.bytes + pool_held_bytes(ctx, 0, 5) + pool_held_bytes(ctx, 1, 5), 0));
    rtk::PoolDev pd[2];
    for (int k = 0; k < 2; ++k) { const int r = pool_bind(ctx, k, P, 5, pd[k]); if (r != RT_OK) return r; }
    const uint32_t n_chunk = (uint32_t)std::min<uint64_t>(n_rays, P);                       // rays of a chunk
    const uint32_t s_chunk = (uint32_t)std::min<uint64_t>(S, std::max<uint32_t>(1u, P / n_chunk));   // samples of a chunk, at most
    HIP_TRY(ctx, ctx->blocksum.ensure((size_t)n_chunk * s_chunk * 16));
    HIP_TRY(ctx, ctx->list_map.ensure((size_t)n_chunk * 8u));   // [0, n): the iota table; [n, 2n): where k_resolve_list's counts[] go (nobody reads them)
    CounterBlock cb;
    HIP_TRY(ctx, cb.ensure(ctx));
    HIP_TRY(ctx, cb.zero_all());

    rtk::RenderDev rd{};
    rd.width = 65536u; rd.height = 65536u; rd.div_width = rtk::make_fastdiv(65536u);       // pixel (stream) = y * 65536 + x, every u32
    rd.shard_count = 1u; rd.shard_index = 0u; rd.tile_size = 32u; rd.tiles_x = 2048u; rd.tiles_y = 2048u;
    rd.div_ts = rtk::make_fastdiv(32u); rd.div_ts2 = rtk::make_fastdiv(1024u); rd.div_tiles_x = rtk::make_fastdiv(2048u); rd.div_shards = rtk::make_fastdiv(1u);
    rd.div_sq_row = rtk::make_fastdiv(4u); rd.div_item_tile = rtk::make_fastdiv(1024u); rd.div_row_items = rtk::make_fastdiv(1u);
    rd.seed = opt->seed; rd.max_depth = opt->max_depth; rd.nan_policy = opt->nan_policy;
    rd.bg_mode = scene->bg_mode; for (int i = 0; i < 3; ++i) rd.bg[i] = scene->bg[i];
    rd.block_shift = 0u;                                                                     // one sample per item: nothing regenerates, no camera is read
    set_queue_geometry(rd, P);
    rd.first_in_shade = scene->first_id != 0u && rtk::can_test_first_in_shade(scene->features) ? 1u : 0u;
    rd.first_id = scene->first_id; for (int k = 0; k < 8; ++k) rd.first_prim[k] = scene->first_prim[k];
    rd.blocksum = (rtd::Float4*)ctx->blocksum.p;
    uint32_t* const iota = (uint32_t*)ctx->list_map.p;
    rd.list = iota; rd.counts = iota + n_chunk;

    uint32_t extend_geometry[2] = {0u, 0u};
    rtk::LaunchCfg cfg = scene_launch_cfg(ctx, scene, extend_geometry);
    const uint32_t drain_at = drain_threshold(scene, opt->tail_paths, false);
    StreamTimer tm{ctx};
    uint32_t launched = 0u, drained = 0u;
    bool first_chunk = true;
    for (uint64_t r0 = 0; r0 < n_rays; r0 += n_chunk) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(n_chunk, n_rays - r0);
        const uint64_t stream0 = opt->first_stream + r0;
        for (uint32_t s0 = 0; s0 < S;) {
            const uint32_t sc = (uint32_t)std::min<uint64_t>(std::min<uint32_t>(s_chunk, S - s0), 0xFFFFFFFFull / (stream0 + n));   // >= 1: check_radiance
            rd.first_sample = opt->first_sample + s0; rd.spp = rd.first_sample + sc;
            rd.n_blocks = sc; rd.div_nblocks = rtk::make_fastdiv(sc);
            rd.total_items = n * sc; rd.n_init = rd.total_items; rd.lineage = rd.total_items;
            rd.n_list = n; rd.div_list = rtk::make_fastdiv(n);
            rd.list_map = (const uint32_t*)((uintptr_t)iota - 4ull * stream0);   // list_map[stream0 + i] = iota[i] = i
            rd.accumulate = ((opt->flags & RT_RADIANCE_ACCUMULATE) != 0u || s0 != 0u) ? 1u : 0u;
            rd.sq_sum = d_sq ? (float*)d_sq + 3ull * r0 : nullptr;
            rtk::RadianceDev qd{};
            qd.rays = d_rays; qd.ray0 = r0; qd.n = n; qd.n_samples = sc; qd.div_n = rtk::make_fastdiv(n); qd.stream0 = (uint32_t)stream0;
            qd.iota = iota; qd.invalid = (uint8_t*)d_invalid;
            hipEvent_t ea = nullptr, eb = nullptr, ec = nullptr, ed = nullptr;
            if (!first_chunk) HIP_TRY(ctx, cb.zero_queue_lines());
            first_chunk = false;
            if (timing) HIP_TRY(ctx, tm.mark(ea));
            LAUNCH_TRY(rtk::launch_radiance_import(rd, qd, pd[0], cb.count[0], cb.c64, ctx->stream));
            if (timing) { HIP_TRY(ctx, tm.mark(eb)); tm.span(ea, eb, 2); }
            { const int r = wavefront_loop(ctx, scene, rd, pd, cb, cfg, tm, timing, false, drain_at, rd.n_init, launched, drained); if (r != RT_OK) return r; }
            if (timing) HIP_TRY(ctx, tm.mark(ec));
            HIP_TRY(ctx, rtk::launch_resolve_list(rd, (float*)d_rgb + 3ull * r0, ctx->stream));
            if (timing) { HIP_TRY(ctx, tm.mark(ed)); tm.span(ec, ed, 2); }
            s0 += sc;
        }
    }
    double part_ms[4] = {0.0, 0.0, 0.0, 0.0};                         // extend, shade, import and fold, drain
    { const int r = finish_call(ctx, cb, tm, part_ms, t_begin, scene, cfg, P, launched, stats); if (r != RT_OK) return r; }
    if (stats) {
        stats->extend_ms = part_ms[0]; stats->shade_ms = part_ms[1]; stats->other_ms = part_ms[2]; stats->drain_ms = part_ms[3];
        stats->samples = items - ctx->h_counters[rtk::CTR_SAMPLES];    // less the paths the imports dropped: valid rays x samples
        stats->iterations = (uint32_t)ctx->h_counters[rtk::CTR_ITERATIONS]; stats->shade_launches = launched; stats->drain_paths = drained;
    }
    return RT_OK;
}

// the argument checks of both variants: a refused call has written nothing
static int radiance_refuse(RtCtx* ctx, const RtScene* scene, const RtRadianceOptions* options, const void* rays, uint64_t n_rays, const void* rgb, const void* sq, bool device) {
    if (!scene) return set_err(ctx, RT_ERR_INVALID, "scene is null");
    const int v = check_radiance(ctx, options, n_rays); if (v != RT_OK) return v;
    if (n_rays != 0u && (!rays || !rgb)) return set_err(ctx, RT_ERR_INVALID, "rays / rgb_sum is null");
    if (device && ((((uintptr_t)rays) | ((uintptr_t)rgb) | ((uintptr_t)sq)) & 15u)) return set_err(ctx, RT_ERR_INVALID, "rays / rgb_sum / sq_sum must be 16-byte aligned");
    return RT_OK;
}

int rt_radiance_rays_device(RtCtx* ctx, const RtScene* scene, const RtRadianceOptions* options, const void* rays_device, uint64_t n_rays, void* rgb_sum_device,
                            void* sq_sum_device, void* invalid_device, RtStats* stats) {
    return query_entry(ctx, stats, n_rays == 0u, true, [&] { return radiance_refuse(ctx, scene, options, rays_device, n_rays, rgb_sum_device, sq_sum_device, true); },
                       [&] { return radiance_impl(ctx, scene, options, rays_device, n_rays, rgb_sum_device, sq_sum_device, invalid_device, stats); });
}
// the host variant: rays (and, accumulating, the caller's sums) staged in, the device variant on the context's own buffers, the sums and flag
// bytes staged out (host buffers are copied: no alignment asked)
int rt_radiance_rays(RtCtx* ctx, const RtScene* scene, const RtRadianceOptions* options, const RtPathRay* rays_host, uint64_t n_rays, float* rgb_sum_host,
                     float* sq_sum_host, uint8_t* invalid_host, RtStats* stats) {
    return query_entry(ctx, stats, n_rays == 0u, false, [&] { return radiance_refuse(ctx, scene, options, rays_host, n_rays, rgb_sum_host, sq_sum_host, false); }, [&] {
        const size_t bytes = (size_t)n_rays * 3u * sizeof(float);
        const bool acc = (options->flags & RT_RADIANCE_ACCUMULATE) != 0u;   // the fold then goes on from the caller's sums
        return staged_call(ctx, {{&ctx->rays_tmp, rays_host, nullptr, (size_t)n_rays * sizeof(RtPathRay)}, {&ctx->out_tmp, acc ? rgb_sum_host : nullptr, rgb_sum_host, bytes},
                                 {&ctx->sq_tmp, acc ? sq_sum_host : nullptr, sq_sum_host, bytes}, {&ctx->hits_tmp, nullptr, invalid_host, (size_t)n_rays}}, stats, [&] {
            return rt_radiance_rays_device(ctx, scene, options, ctx->rays_tmp.p, n_rays, ctx->out_tmp.p, sq_sum_host ? ctx->sq_tmp.p : nullptr,
                                           invalid_host ? ctx->hits_tmp.p : nullptr, stats);
        });
    });
}

// ---- first-hit features (include/rt_hip.h): albedo, normal and depth of the render's own camera rays, as per-pixel sums ---------------------
static_assert(sizeof(RtFeatureOptions) == 16 && sizeof(RtFeatureBuffers) == 4 * sizeof(void*), "feature records: 16 bytes and four pointers");
static int check_features(RtCtx* ctx, const RtParams* p, const RtFeatureOptions* o) {
    const int v = validate_params(ctx, p); if (v != RT_OK) return v;
    if (!o) return set_err(ctx, RT_ERR_INVALID, "feature options are null");
    const int h = check_header(ctx, o->struct_bytes, sizeof(RtFeatureOptions), "RtFeatureOptions", o->flags, RT_FEATURES_ACCUMULATE, "RT_FEATURES_ACCUMULATE"); if (h != RT_OK) return h;
    if ((uint64_t)o->first_sample + p->samples_per_pixel > 0xFFFFFFFFull) return set_err(ctx, RT_ERR_INVALID, "first_sample + samples_per_pixel must be < 2^32");
    if (p->flags & (RT_FLAG_COUNTERS | RT_FLAG_FUSED)) return set_err(ctx, RT_ERR_INVALID, "a feature pass takes neither RT_FLAG_COUNTERS nor RT_FLAG_FUSED");
    return RT_OK;
}
int rt_features_check(const RtParams* params, const RtFeatureOptions* options) { return check_features(nullptr, params, options); }

// The chunk loop, modelled on trace_rays_impl: import (the camera rays of a chunk) -> k_extend (the scene's own launch configuration) ->
// export (one feature record per ray) -> fold (per-slot sums), all on the context's stream; the host waits once, at the end. A chunk holds
// the whole sample run of as many slots as the pool has room for; only a pass with more samples per pixel than pool slots is cut along the
// samples too, its later parts folding on from the planes — the same additions in the same order, so the cut does not show.
static int features_impl(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, const RtFeatureOptions* opt, const RtFeatureBuffers* out, RtStats* stats,
                         const rtk::FeatMomDev* moments) {                // moments: the squared-sum planes of rt_render_feature_moments_device; the fold is then k_features_fold<true>
    using clk = std::chrono::steady_clock;
    const auto t_begin = clk::now();
    const bool timing = (prm->flags & RT_FLAG_TIMING) != 0u;
    Tiling tl; make_tiling(*prm, tl);
    rtk::RenderDev rd = frame_render_dev(scene, cam, prm, tl);
    rd.div_nblocks = rtk::make_fastdiv(1u); rd.n_blocks = 1u;                 // (a walk needs the queue geometry only; first_in_shade = 0: the record's time slot is the ray's time)
    const uint64_t n_slots = rd.shard_count <= 1u ? (uint64_t)prm->width * prm->height : (uint64_t)tl.n_local * tl.ts * tl.ts;
    if (n_slots == 0u) return RT_OK;
    if (n_slots > 0xFFFFFFFFull) return set_err(ctx, RT_ERR_INVALID, "more than 2^32 - 1 output slots in one shard (shard the image further)");
    const uint64_t spp = prm->samples_per_pixel, n_rays = n_slots * spp;

    // one pool, every ray in flight, plus 32 bytes of feature record per slot
    const uint32_t P = pool_grain(pool_size(opt->pool_slots, n_rays, pool_slot_bytes(5) + 32, pool_held_bytes(ctx, 0, 5) + ctx->feature_rec.bytes, 0));
    set_queue_geometry(rd, P);
    rtk::PoolDev pd{};
    { const int r = pool_bind(ctx, 0, P, 5, pd); if (r != RT_OK) return r; }
    HIP_TRY(ctx, ctx->feature_rec.ensure((size_t)P * 32u));
    CounterBlock cb;   // one pool: count[0] the queues' sizes, count[1] what k_extend zeroes for a k_shade that never runs here
    HIP_TRY(ctx, cb.ensure(ctx));
    HIP_TRY(ctx, cb.zero_all());

    uint32_t extend_geometry[2] = {0u, 0u};
    rtk::LaunchCfg cfg = scene_launch_cfg(ctx, scene, extend_geometry);
    rtk::FeatDev fd{};
    fd.first_sample = opt->first_sample; fd.rec = (rtd::Float4*)ctx->feature_rec.p;
    fd.albedo = (float*)out->albedo_sum; fd.normal = (float*)out->normal_sum; fd.depth = (float*)out->depth_sum; fd.hits = (uint32_t*)out->hits;

    StreamTimer tm{ctx};
    uint32_t launched = 0u;
    const uint32_t nk_max = (uint32_t)std::min<uint64_t>(spp, P), ns_max = P / nk_max;      // samples and slots of a chunk: nk * ns <= P
    for (uint64_t k0 = 0; k0 < spp; k0 += nk_max) {
        fd.k0 = (uint32_t)k0; fd.nk = (uint32_t)std::min<uint64_t>(nk_max, spp - k0);
        fd.accumulate = (opt->flags & RT_FEATURES_ACCUMULATE) != 0u || k0 != 0u ? 1u : 0u;
        for (uint64_t slot0 = 0; slot0 < n_slots; slot0 += ns_max) {
            fd.slot0 = (uint32_t)slot0; fd.ns = (uint32_t)std::min<uint64_t>(ns_max, n_slots - slot0); fd.div_ns = rtk::make_fastdiv(fd.ns);
            const uint32_t n = fd.ns * fd.nk;
            hipEvent_t ea = nullptr, eb = nullptr, ec = nullptr, ed = nullptr, ee = nullptr;
            if (launched != 0u) HIP_TRY(ctx, cb.zero_queue_lines());
            if (timing) HIP_TRY(ctx, tm.mark(ea));
            LAUNCH_TRY(rtk::launch_features_import(rd, fd, pd, cb.count[0], cb.c64, ctx->stream));
            if (timing) HIP_TRY(ctx, tm.mark(eb));
            cfg.max_rays = n;
            LAUNCH_TRY(rtk::launch_extend(cfg, scene->dev, pd, rd, cb.count[0], cb.head, cb.count[1], cb.c64, false, ctx->stream));
            if (timing) HIP_TRY(ctx, tm.mark(ec));
            LAUNCH_TRY(rtk::launch_features_export(cfg, scene->dev, rd, fd, pd, export_bound(rd.queue_cap, n), cb.count[0], ctx->stream));
            if (timing) HIP_TRY(ctx, tm.mark(ed));
            LAUNCH_TRY(rtk::launch_features_fold(rd, fd, moments, ctx->stream));
            if (timing) { HIP_TRY(ctx, tm.mark(ee)); tm.span(ea, eb, 1); tm.span(eb, ec, 0); tm.span(ec, ed, 2); tm.span(ed, ee, 3); }
            ++launched;
        }
    }
    double part_ms[4] = {0.0, 0.0, 0.0, 0.0};                         // extend, import, export, fold
    { const int r = finish_call(ctx, cb, tm, part_ms, t_begin, scene, cfg, P, launched, stats); if (r != RT_OK) return r; }
    if (stats) {
        stats->extend_ms = part_ms[0]; stats->other_ms = part_ms[1] + part_ms[2] + part_ms[3];
        for (int k = 0; k < 3; ++k) stats->debug[k] = (uint64_t)(part_ms[k + 1] * 1000.0 + 0.5);     // microseconds of the import, export and fold kernels
        stats->samples = stats->segments; stats->iterations = launched;
    }
    return RT_OK;
}

// What both feature entry points check, in two parts because the moments variant checks its own record in between: the call (a refused
// call has written nothing), then the caller's planes — one wanted at least, each 16-byte aligned.
static int features_refuse(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, const RtFeatureOptions* options) {
    if (!scene || !cam) return set_err(ctx, RT_ERR_INVALID, "scene / cam is null");
    const int v = check_features(ctx, prm, options); if (v != RT_OK) return v;
    if (scene->features & rtk::F_MEDIUM)
        return set_err(ctx, RT_ERR_UNSUPPORTED, "first-hit features: the scene holds a ConstantMedium (the limit of ray queries: its hit is a draw of the path's medium stream)");
    return RT_OK;
}
static int feature_planes_refuse(RtCtx* ctx, std::initializer_list<const void*> planes, const char* none_wanted) {
    uintptr_t any = 0; for (const void* p : planes) any |= (uintptr_t)p;
    if (!any) return set_err(ctx, RT_ERR_INVALID, none_wanted);
    if (any & 15u) return set_err(ctx, RT_ERR_INVALID, "feature buffers must be 16-byte aligned");
    return RT_OK;
}

int rt_render_features_device(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, const RtFeatureOptions* options, const RtFeatureBuffers* buffers,
                              RtStats* stats) {
    const RtFeatureBuffers none{nullptr, nullptr, nullptr, nullptr}, &b = buffers ? *buffers : none;
    return query_entry(ctx, stats, false, false, [&] {
        const int v = features_refuse(ctx, scene, cam, prm, options);
        return v != RT_OK ? v : feature_planes_refuse(ctx, {b.albedo_sum, b.normal_sum, b.depth_sum, b.hits}, "no feature buffer is wanted (all four pointers are null)");
    }, [&] { return features_impl(ctx, scene, cam, prm, options, buffers, stats, nullptr); });
}

// ---- first-hit features, second moments (include/rt_hip.h): the same pass, with the per-slot sums of squares beside the sums ---------------
static_assert(sizeof(RtFeatureMomentBuffers) == 8 * sizeof(void*), "feature moment buffers: struct_bytes (padded) and seven pointers");
static int check_moment_buffers(RtCtx* ctx, const RtFeatureMomentBuffers* b) {
    if (!b) return set_err(ctx, RT_ERR_INVALID, "feature moment buffers are null");
    return check_header(ctx, b->struct_bytes, sizeof(RtFeatureMomentBuffers), "RtFeatureMomentBuffers");
}
int rt_feature_moments_check(const RtParams* params, const RtFeatureOptions* options, const RtFeatureMomentBuffers* buffers) {
    const int v = check_features(nullptr, params, options);
    return v != RT_OK ? v : check_moment_buffers(nullptr, buffers);
}

int rt_render_feature_moments_device(RtCtx* ctx, const RtScene* scene, const RtCamera* cam, const RtParams* prm, const RtFeatureOptions* options,
                                     const RtFeatureMomentBuffers* b, RtStats* stats) {
    return query_entry(ctx, stats, false, false, [&] {
        int v = features_refuse(ctx, scene, cam, prm, options);
        if (v == RT_OK) v = check_moment_buffers(ctx, b);
        return v != RT_OK ? v : feature_planes_refuse(ctx, {b->albedo_sum, b->normal_sum, b->depth_sum, b->hits, b->albedo_sq_sum, b->normal_sq_sum, b->depth_sq_sum},
                                                      "no feature buffer is wanted (all seven pointers are null)");
    }, [&] {
        const RtFeatureBuffers sums{b->albedo_sum, b->normal_sum, b->depth_sum, b->hits};
        const rtk::FeatMomDev fm{(float*)b->albedo_sq_sum, (float*)b->normal_sq_sum, (float*)b->depth_sq_sum};
        return features_impl(ctx, scene, cam, prm, options, &sums, stats, &fm);
    });
}

int rt_untile(const RtParams* p, const float* gathered, float* rgb_sum) { return untile_host<float>(p, gathered, rgb_sum); }
int rt_untile_rgb8(const RtParams* p, const uint8_t* gathered, uint8_t* rgb8) { return untile_host<uint8_t>(p, gathered, rgb8); }

int rt_scene_compile_info(const RtSceneDesc* desc, RtCompileInfo* out) { return rt_scene_compile_info_ex(desc, nullptr, out); }
int rt_scene_compile_info_ex(const RtSceneDesc* desc, const RtUploadOptions* options, RtCompileInfo* out) {
    if (!desc || !out) return set_err(nullptr, RT_ERR_INVALID, "null argument");
    rtc::CompiledScene cs; std::string why; uint32_t n_with = 0u, n_mapped = 0u;
    { const int ok = compile_checked(*desc, options, cs, nullptr, &n_with, why, &n_mapped); if (ok != RT_OK) return set_err(nullptr, ok, why); }
    out->n_nodes = cs.nodes.size(); out->n_box_nodes = cs.n_box_nodes; out->n_spheres = cs.sphere_meta.size(); out->n_moving = cs.moving_meta.size();
    out->n_rects = cs.rect_meta.size(); out->n_tris = cs.tri_meta.size(); out->n_media = cs.media.size(); out->n_xforms = cs.xforms.size();
    out->n_lights = cs.n_lights; out->n_materials = cs.mat_b.size();
    out->features = scene_features(cs) | (n_with != 0u ? rtk::F_TRI_ATTR : 0u) | (env_of(options) ? rtk::F_LIGHTS_EXT | rtk::F_ENV : 0u) |
                    (n_mapped != 0u ? rtk::F_TEX | rtk::F_NORMAL_MAP : 0u);
    out->n_tri_attrs = n_with;
    out->fits_lds = lds_scene_bytes(cs) <= kLdsSceneBudget ? 1u : 0u;
    {   // what a walk tests before it enters the tree: the root list's every-ray members, then the root BVH's scene-sized spheres
        std::vector<uint32_t> first = cs.prologue;
        if (cs.first_leaf != 0u) first.push_back(cs.first_leaf);
        out->n_first = (uint32_t)std::min<size_t>(first.size(), 4);
        for (uint32_t k = 0; k < 4u; ++k) out->first[k] = k < first.size() ? first[k] : 0u;
    }
    return RT_OK;
}

int rt_scene_light_tree_dump(const RtSceneDesc* desc, void* nodes, uint64_t cap_nodes, uint32_t* slot_member, float* p, float* cdf, uint64_t cap_lights,
                             uint64_t* out_n_lights, uint64_t* out_n_nodes) {
    if (!desc || !out_n_lights || !out_n_nodes) return set_err(nullptr, RT_ERR_INVALID, "null argument");
    *out_n_lights = 0; *out_n_nodes = 0;
    rtc::CompiledScene cs;
    const int rc = rtc::compile_scene(*desc, cs);
    if (rc != RT_OK) return set_err(nullptr, rc, "scene: " + cs.error);
    if (!cs.lights_tree) return set_err(nullptr, RT_ERR_INVALID, "the scene has no light tree (RtSceneDesc.scene_flags without RT_SCENE_LIGHTS_MANY, or no lights list)");
    const uint64_t n = cs.n_lights, n_nodes = rtd::light_tree_nodes(cs.n_lights);
    *out_n_lights = n; *out_n_nodes = n_nodes;
    if ((nodes && cap_nodes < n_nodes) || ((slot_member || p || cdf) && cap_lights < n)) return set_err(nullptr, RT_ERR_INVALID, "capacity too small");
    if (nodes) std::memcpy(nodes, cs.lights.data() + 3 * n, n_nodes * sizeof(rtd::NodeDev));   // the records as the upload copies them
    if (slot_member) std::memcpy(slot_member, cs.light_slot_member.data(), n * 4);
    if (p) std::memcpy(p, cs.light_p.data(), n * 4);
    if (cdf) std::memcpy(cdf, cs.light_cdf.data(), n * 4);
    return RT_OK;
}

int rt_camera_lists_host(const RtSceneDesc* desc, const RtCamera* cam, uint32_t width, uint32_t height, uint32_t* lists, uint64_t cap_words, uint64_t* out_n_squares) {
    if (!desc || !cam || !out_n_squares) return set_err(nullptr, RT_ERR_INVALID, "null argument");
    *out_n_squares = 0;
    if (width < 2u || height < 2u || width > 65536u || height > 65536u) return set_err(nullptr, RT_ERR_INVALID, "width and height must be in 2..65536");
    rtc::CompiledScene cs;
    const int rc = rtc::compile_scene(*desc, cs);
    if (rc != RT_OK) return set_err(nullptr, rc, "scene: " + cs.error);
    const std::vector<uint32_t> order = camera_order(cs);
    if (order.empty() || !camera_is_finite(cam)) return RT_OK;                 // a scene or camera the lists do not serve: no squares
    const rtcl::Camera c = camera_lists_camera(cam, width, height);
    const uint32_t sqx = rtcl::squares_x(width), n = sqx * rtcl::squares_y(height);
    *out_n_squares = n;
    if (!lists) return RT_OK;
    if (cap_words < (uint64_t)n * rtcl::kListWords) return set_err(nullptr, RT_ERR_INVALID, "capacity too small");
    for (uint32_t i = 0; i < n; ++i) rtcl::build_list(c, i % sqx, i / sqx, &cs.spheres[0].x, order.data(), (uint32_t)order.size(), lists + (size_t)i * rtcl::kListWords);
    return RT_OK;
}

int rt_camera_lists_last(RtCtx* ctx, uint32_t* lists, uint64_t cap_words, uint64_t* out_n_squares) {
    if (!ctx || !out_n_squares) return set_err(ctx, RT_ERR_INVALID, "null argument");
    *out_n_squares = ctx->cam_squares;
    if (!lists || ctx->cam_squares == 0u) return RT_OK;
    if (cap_words < (uint64_t)ctx->cam_squares * rtcl::kListWords) return set_err(ctx, RT_ERR_INVALID, "capacity too small");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(lists, ctx->cam_lists.p, (size_t)ctx->cam_squares * rtcl::kListWords * 4u, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_scene_top_layout_check(const RtSceneDesc* desc, uint32_t max_top, uint64_t* out_n_top) {
    if (!desc) return set_err(nullptr, RT_ERR_INVALID, "null argument");
    rtc::CompiledScene cs;
    const int rc = rtc::compile_scene(*desc, cs);
    if (rc != RT_OK) return set_err(nullptr, rc, "scene: " + cs.error);
    DevNodes dn;
    if (out_n_top) *out_n_top = 0;
    if (!device_nodes(cs.nodes, max_top, dn)) return set_err(nullptr, RT_ERR_UNSUPPORTED, "node array beyond 4 GB");
    if (out_n_top) *out_n_top = dn.n_top;
    const size_t n = cs.nodes.size();
    const uint32_t top_bytes = dn.n_top * 32u, special = top_bytes + (uint32_t)n * 32u, done = special, idle = special + 32u, end = top_bytes + dn.records() * 32u;
    auto rec = [&](uint32_t addr) -> rtd::NodeDev {
        rtd::NodeDev d;
        std::memcpy(&d, addr < top_bytes ? dn.top.data() + addr : dn.main.data() + (addr - top_bytes), 32);
        return d;
    };
    auto word = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
    auto parks = [&](uint32_t addr, uint32_t resume, uint32_t payload) {
        if (addr < special || addr + 32u > end) return false;
        const rtd::NodeDev t = rec(addr);
        return t.skip_bytes == addr && t.leaf == addr && t.hx < 0.f && t.hy < 0.f && t.hz < 0.f && word(t.cx) == resume && word(t.cy) == payload;
    };
    // the walk that passes every box (and is moved on from every twin) must enumerate the records in pre-order
    std::vector<uint32_t> addr(n + 1);
    uint32_t a = 0;
    for (size_t i = 0; i < n; ++i) {
        addr[i] = a;
        if (a >= special) return set_err(nullptr, RT_ERR_DEVICE, "walk left the records early");
        const rtd::NodeDev d = rec(a), h = rec(top_bytes + (uint32_t)i * 32u);
        if (std::memcmp(&d, &h, 32) != 0) return set_err(nullptr, RT_ERR_DEVICE, "top copy differs from the array's record");
        if (cs.nodes[i].leaf != 0u) {
            if (!parks(d.leaf, d.skip_bytes, cs.nodes[i].leaf)) return set_err(nullptr, RT_ERR_DEVICE, "park twin of record " + std::to_string(i));
            a = d.skip_bytes;                                         // the twin's resume address
        } else a = d.leaf;
    }
    addr[n] = a;
    if (a != done || !parks(done, done, rtd::LEAF_DONE) || !parks(idle, idle, rtd::LEAF_IDLE)) return set_err(nullptr, RT_ERR_DEVICE, "closing records");
    for (size_t i = 0; i < n; ++i)
        if (rec(addr[i]).skip_bytes != addr[std::min<size_t>(cs.nodes[i].skip, n)]) return set_err(nullptr, RT_ERR_DEVICE, "skip link of record " + std::to_string(i));
    return RT_OK;
}

int rt_scene_compile_dump(const RtSceneDesc* desc, void* nodes, uint64_t cap_nodes, float* spheres, uint32_t* sphere_meta, uint64_t cap_spheres) {
    return rt_scene_compile_dump_ex(desc, nullptr, nodes, cap_nodes, spheres, sphere_meta, cap_spheres);
}
int rt_scene_compile_dump_ex(const RtSceneDesc* desc, const RtUploadOptions* options, void* nodes, uint64_t cap_nodes, float* spheres, uint32_t* sphere_meta,
                             uint64_t cap_spheres) {
    if (!desc) return set_err(nullptr, RT_ERR_INVALID, "null argument");
    rtc::CompiledScene cs; std::string why; uint32_t n_with = 0u;
    { const int ok = compile_checked(*desc, options, cs, nullptr, &n_with, why); if (ok != RT_OK) return set_err(nullptr, ok, why); }
    if ((nodes && cap_nodes < cs.nodes.size()) || ((spheres || sphere_meta) && cap_spheres < cs.sphere_meta.size())) return set_err(nullptr, RT_ERR_INVALID, "capacity too small");
    if (nodes) std::memcpy(nodes, cs.nodes.data(), cs.nodes.size() * sizeof(rtd::Node));
    if (spheres) std::memcpy(spheres, cs.spheres.data(), cs.spheres.size() * sizeof(rtd::Float4));
    if (sphere_meta) std::memcpy(sphere_meta, cs.sphere_meta.data(), cs.sphere_meta.size() * 4);
    return RT_OK;
}

int rt_scene_wide_layout_check(const RtSceneDesc* desc, RtWideInfo* out) {
    if (!desc || !out) return set_err(nullptr, RT_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    rtc::CompiledScene cs;
    rtc::CompileOptions copt; copt.big_spheres_first = false;      // (the 8-wide walk tests nothing before the tree)
    const int rc = rtc::compile_scene(*desc, copt, cs);
    if (rc != RT_OK) return set_err(nullptr, rc, "scene: " + cs.error);
    if (!rtw::eligible(cs.nodes)) return set_err(nullptr, RT_ERR_UNSUPPORTED, "not a static BVH: the scene keeps the binary walk");
    const float margin = wide_margin(cs.nodes);
    rtw::WideTree wt; std::string err;
    if (!rtw::build(cs.nodes, margin, wt, err)) return set_err(nullptr, RT_ERR_UNSUPPORTED, err);
    // true box of one primitive (f64 from the compiled f32 data: what the kernel's tests see)
    struct B { double mn[3], mx[3]; };
    auto prim_box = [&](uint32_t type, uint32_t idx, B& b) {
        auto set = [&](int a, double lo, double hi) { b.mn[a] = lo; b.mx[a] = hi; };
        if (type == rtd::LT_SPHERE) { const rtd::Float4 s = cs.spheres[idx]; const double r = std::fabs((double)s.w); set(0, s.x - r, s.x + r); set(1, s.y - r, s.y + r); set(2, s.z - r, s.z + r); }
        else if (type == rtd::LT_TRI) {
            for (int a = 0; a < 3; ++a) { double lo = 1e300, hi = -1e300; for (int v = 0; v < 3; ++v) { const rtd::Float4 p = cs.tris[3 * idx + v]; const double c = a == 0 ? p.x : a == 1 ? p.y : p.z; lo = std::min(lo, c); hi = std::max(hi, c); } set(a, lo, hi); }
        } else if (type == rtd::LT_RECT) {
            const rtd::Float4 r0 = cs.rects[2 * idx], r1 = cs.rects[2 * idx + 1]; const int k = (int)r1.y, ia = k == 0 ? 1 : 0, ib = k == 2 ? 1 : 2;
            set(k, r1.x, r1.x); set(ia, r0.x, r0.y); set(ib, r0.z, r0.w);
        } else { const rtd::Float4 b0 = cs.boxes[2 * idx], b1 = cs.boxes[2 * idx + 1]; set(0, b0.x, b0.y); set(1, b0.z, b0.w); set(2, b1.x, b1.y); }
    };
    std::vector<uint8_t> seen[8];
    seen[rtd::LT_SPHERE].assign(cs.sphere_meta.size(), 0); seen[rtd::LT_TRI].assign(cs.tri_meta.size(), 0);
    seen[rtd::LT_RECT].assign(cs.rect_meta.size(), 0); seen[rtd::LT_BOX].assign(cs.boxes.size() / 2, 0);
    std::string bad;
    uint64_t used_slots = 0;
    // content box of a wide node, bottom-up; every entry's decoded box must contain the content below it
    std::vector<int> state(wt.n_nodes, 0);
    std::function<bool(uint32_t, B&, uint32_t)> walk = [&](uint32_t w, B& content, uint32_t depth) -> bool {
        if (w >= wt.n_nodes || state[w] != 0) { bad = "a wide node is referenced twice or out of range"; return false; }
        state[w] = 1;
        if (depth >= rtd::WIDE_MAX_DEPTH) { bad = "deeper than the walk's stack"; return false; }
        const uint32_t* W = wt.words.data() + (size_t)w * 32u;
        float org[3]; std::memcpy(&org[0], &W[3], 4); std::memcpy(&org[1], &W[7], 4); std::memcpy(&org[2], &W[11], 4);
        float scl[3]; for (int a = 0; a < 3; ++a) { const uint32_t bits = ((W[15] >> (8 * a)) & 0xFFu) << 23; std::memcpy(&scl[a], &bits, 4); }
        for (int a = 0; a < 3; ++a) { content.mn[a] = 1e300; content.mx[a] = -1e300; }
        for (int k = 0; k < 8; ++k) {
            const uint32_t* c = W + 4 * k;
            if (c[0] == 0u) continue;
            ++used_slots;
            const uint32_t q[6] = {c[1] & 0xFFu, (c[1] >> 8) & 0xFFu, (c[1] >> 16) & 0xFFu, c[1] >> 24, c[2] & 0xFFu, (c[2] >> 8) & 0xFFu};
            B below;
            if (c[0] >> 31) {
                const uint32_t type = (c[0] >> 28) & 7u, cnt = (c[0] >> 24) & 15u, first = c[0] & rtd::LEAF_MAX_FIRST;
                if (cnt == 0u || cnt > 8u || seen[type].empty()) { bad = "leaf entry with a bad kind or count"; return false; }
                for (int a = 0; a < 3; ++a) { below.mn[a] = 1e300; below.mx[a] = -1e300; }
                for (uint32_t m = 0; m < cnt; ++m) {
                    if (first + m >= seen[type].size() || seen[type][first + m]++) { bad = "a primitive is in two leaf entries or out of range"; return false; }
                    B pb; prim_box(type, first + m, pb);
                    for (int a = 0; a < 3; ++a) { below.mn[a] = std::min(below.mn[a], pb.mn[a]); below.mx[a] = std::max(below.mx[a], pb.mx[a]); }
                }
                out->n_prims += cnt;
            } else if (!walk(c[0] - 1u, below, depth + 1)) return false;
            for (int a = 0; a < 3; ++a) {
                const double lo = (double)std::fmaf((float)q[a], scl[a], org[a]), hi = (double)std::fmaf((float)q[3 + a], scl[a], org[a]);
                if (!(lo <= below.mn[a] - margin && hi >= below.mx[a] + margin)) { bad = "an entry's decoded box does not contain what is below it"; return false; }
                content.mn[a] = std::min(content.mn[a], below.mn[a]); content.mx[a] = std::max(content.mx[a], below.mx[a]);
            }
        }
        return true;
    };
    B all;
    if (!walk(0u, all, 0u)) return set_err(nullptr, RT_ERR_DEVICE, "wide tree: " + bad);
    for (uint32_t t : {(uint32_t)rtd::LT_SPHERE, (uint32_t)rtd::LT_TRI, (uint32_t)rtd::LT_RECT, (uint32_t)rtd::LT_BOX})
        for (size_t i = 0; i < seen[t].size(); ++i) {
            // (spheres that only bound a medium, and the rects that are a Box's sides, are not in any leaf: a static BVH has no media, and box sides are reached through their Box)
            if (seen[t][i] == 0 && !(t == rtd::LT_RECT && !cs.boxes.empty())) return set_err(nullptr, RT_ERR_DEVICE, "wide tree: a primitive is in no leaf entry");
        }
    for (uint32_t w = 0; w < wt.n_nodes; ++w) if (!state[w]) return set_err(nullptr, RT_ERR_DEVICE, "wide tree: an unreachable node");
    out->n_nodes = wt.n_nodes; out->n_leaf_entries = wt.n_leaf_entries; out->n_inner_entries = wt.n_inner_entries; out->depth = wt.depth;
    out->mean_children = wt.n_nodes ? (double)used_slots / wt.n_nodes : 0.0;
    out->mean_leaf_members = wt.n_leaf_entries ? (double)out->n_prims / wt.n_leaf_entries : 0.0;
    return RT_OK;
}

int rt_test_fail_next_renders(RtCtx* ctx, uint32_t n) {
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    ctx->fail_renders = n;
    return RT_OK;
}

int rt_resolve_device(RtCtx* ctx, const void* rgb_sum_device, uint32_t width, uint32_t height, uint32_t spp, void* rgb8_device) {
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    if (!rgb_sum_device || !rgb8_device || spp == 0) return set_err(ctx, RT_ERR_INVALID, "bad argument");
    if (width == 0 || height == 0 || (uint64_t)width * height * 3u > 0xFFFFFFFFull) return set_err(ctx, RT_ERR_INVALID, "bad image size");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, rtk::launch_write_color((const float*)rgb_sum_device, width * height, spp, (uint8_t*)rgb8_device, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

