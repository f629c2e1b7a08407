// oracle.cpp — CPU restatement of the reference renderer's hot path.  TEST INFRASTRUCTURE ONLY.
//
//   * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library.
//     The product path (ray-tracer-archive_amd/) never links, imports or calls it.
//   * PARITY UNPINNED at the sample level: the reference (Rust, /root/reference/raytracer/src)
//     cannot be built here (no cargo/rustc, crates not vendored), draws every random number from
//     an OS-seeded thread-local generator (rt_weekend.rs:8-19) and ships no tests, golden vectors
//     or output images of its own.  What pins this file instead are the analytic known-answer
//     tests derived from the reference source (tests/test_oracle_kat.py) and
//     distribution-level checks (furnace test, f32-vs-f64 converged means).
//     The DEVICE, in turn, is pinned to this file sample by sample: orc_render_paths records every sample's path (segments, how
//     it ended, which branches it took, how closely its thresholds were decided), with an option to perturb every traced ray —
//     tests/paths.py builds the decidability rule and tests/test_gpu_paths.py the comparison from it.
//
// It follows the reference file by file — every function cites the lines it restates — with the
// same object model (virtual Hittable / Material / Texture / Pdf, recursive ray_color), templated
// on the arithmetic type (double = the reference's f64, float = what the device computes in).
// Deliberate differences, all listed in SURVEY.md §8(a'):
//   - rand::random is replaced by a counter-based generator (SplitMix64 over a per-path counter)
//     consumed in the reference's draw order;
//   - BVHNode::construct sorts the sub-range [start,end) (bvh.rs:108 sorts the whole vector, a bug
//     that loses objects) and a span-1 node tests its object once (bvh.rs:96-98 tests it twice);
//   - Aabb::hit carries the interval across axes (aabb.rs:48-49 shadows it per axis);
//   - Sphere / MovingSphere::bounding_box use |radius| (sphere.rs:66-73 turns the box of a negative-radius sphere inside out);
//   - ConstantMedium and Isotropic are restated from the commented-out code
//     (constant_medium.rs:31-71, material.rs:193-220) under the live scatter signature; the
//     medium's free-path draw is keyed by (path, segment, medium) instead of taken from the
//     sequential stream so that closest-hit does not depend on list order;
//   - Triangle and the book-1 sky gradient do not exist in the reference and are defined here;
//   - RtSceneDesc.scene_flags (lights of every shape, the area-weighted pick) and triangle attributes (per-vertex normals and uv) do not
//     exist in the reference either: LightList and Triangle::hit restate include/rt_hip.h's statement of them, not the kernels' text. With
//     scene_flags == 0 and no attributes every entry point computes what it computed before they were added.
//
// Build: make -C oracle   (g++ -O2 -ffp-contract=off, see Makefile)

#include "../include/rt_hip.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <thread>
#include <vector>

namespace orc {

// ------------------------------------------------------------------------------------------------
// RNG: replaces rand::random (rt_weekend.rs:8-19, bvh.rs:87, hittable_list.rs:83).
// SplitMix64 finaliser over a 64-bit counter; one stream per camera path.
// ------------------------------------------------------------------------------------------------
static const uint64_t GAMMA = 0x9E3779B97F4A7C15ull;

static inline uint64_t fin(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static inline uint64_t path_base(uint64_t seed, uint64_t pixel_index, uint64_t sample_index) {
    uint64_t h = fin(seed + GAMMA * (pixel_index + 1));
    return fin(h + 0xD1B54A32D192ED03ull * (sample_index + 1));
}

static inline uint64_t medium_bits(uint64_t base, uint32_t segment, uint32_t medium_id) {
    return fin(base ^ fin(0xA0761D6478BD642Full * (uint64_t)(segment + 1) +
                          0xE7037ED1A0B428DBull * (uint64_t)(medium_id + 1)));
}

struct Counters {
    uint64_t samples = 0, segments = 0, node_tests = 0, draws = 0;
    uint64_t prim_tests[RT_N_PRIM_TYPES] = {0, 0, 0, 0, 0, 0};
    uint64_t nonfinite_samples = 0;
    void add(const Counters& o) {
        samples += o.samples; segments += o.segments; node_tests += o.node_tests; draws += o.draws;
        for (int i = 0; i < RT_N_PRIM_TYPES; ++i) prim_tests[i] += o.prim_tests[i];
        nonfinite_samples += o.nonfinite_samples;
    }
};
enum { PT_SPHERE = 0, PT_MOVING = 1, PT_RECT = 2, PT_TRI = 3, PT_MEDIUM = 4, PT_INSTANCE = 5 };

// Path records (orc_render_paths): which branch every segment of a path took, how it ended, and how closely its random-number
// thresholds were decided. Filled only where Ctx::path / Rng::margin are set; null on every other entry point, whose arithmetic they
// do not touch.
enum : uint64_t {
    EV_LAMB_COSINE_ONLY = 1u << 0, EV_LAMB_LIGHT_XZRECT = 1u << 1, EV_LAMB_LIGHT_SPHERE = 1u << 2, EV_LAMB_MIX_COSINE = 1u << 3,
    EV_METAL = 1u << 4, EV_DIEL_REFRACT = 1u << 5, EV_DIEL_REFLECT_SCHLICK = 1u << 6, EV_DIEL_REFLECT_TIR = 1u << 7, EV_DIEL_BACK_FACE = 1u << 8,
    EV_ISOTROPIC = 1u << 9, EV_MEDIUM_SCATTERED = 1u << 10, EV_MEDIUM_PASSED = 1u << 11,
    EV_TEX_SOLID = 1u << 12, EV_TEX_CHECKER = 1u << 13, EV_TEX_NOISE = 1u << 14, EV_TEX_IMAGE = 1u << 15, EV_TEX_EMPTY_IMAGE = 1u << 16,
    EV_HIT_SPHERE = 1u << 17, EV_HIT_MOVING = 1u << 18, EV_HIT_RECT = 1u << 19, EV_HIT_TRI = 1u << 20, EV_HIT_BOX_SIDE = 1u << 21,
    EV_UNDER_TRANSLATE = 1u << 22, EV_UNDER_ROTATE_Y = 1u << 23, EV_UNDER_FLIP_FACE = 1u << 24, EV_LENS = 1u << 25, EV_TIME = 1u << 26,
    // RtSceneDesc.scene_flags and triangle attributes (rt_hip.h): the light half drew from an XY or YZ rect, a triangle, a box, a member under a
    // wrapper chain; the pick was the area-weighted one; a hit used an interpolated normal, kept the geometric one because the vertex normals
    // cancelled, used an interpolated uv
    EV_LAMB_LIGHT_XY_YZ_RECT = 1ull << 27, EV_LAMB_LIGHT_TRI = 1ull << 28, EV_LAMB_LIGHT_BOX = 1ull << 29, EV_LAMB_LIGHT_WRAPPED = 1ull << 30,
    EV_LAMB_LIGHT_CDF_PICK = 1ull << 31, EV_NORMAL_INTERP = 1ull << 32, EV_NORMAL_FALLBACK = 1ull << 33, EV_UV_INTERP = 1ull << 34
};
enum : uint32_t { TERM_MISS = 0, TERM_EMITTER_FRONT = 1, TERM_EMITTER_BACK = 2, TERM_DEPTH = 3, TERM_NONFINITE = 4 };
struct PathRec {
    uint64_t events = 0; uint32_t terminal = TERM_MISS;
    double margin = std::numeric_limits<double>::infinity();   // smallest distance by which a random-number threshold was decided
    double tmin_margin = std::numeric_limits<double>::infinity();   // smallest |root - t_min| * |d . n| of a primitive test: how far along the
                                                                    // normal the ray's origin would have to move to carry a root across t_min
    // list-pdf evaluations against a light of a kind the reference has not (rt_hip.h RT_SCENE_LIGHTS_ALL_SHAPES): the smallest distance of a
    // crossing from the member's edge (rects: scene units; triangles: barycentrics; near misses count) and the smallest |cos| at a member met
    double light_edge = std::numeric_limits<double>::infinity(), light_cos = std::numeric_limits<double>::infinity();
    // RT_TRI_NORMALS: smallest | |sum|^2 - FLT_MIN | / (largest term)^2 over the interpolated normals of the path
    double normal_margin = std::numeric_limits<double>::infinity();
    int r_ulps = 0; int sign[3] = {1, 1, 1};                   // perturbation of every traced ray's direction (0: none)
};

template <class R> struct Uni;  // u64 -> uniform [0,1)
template <> struct Uni<double> { static double cv(uint64_t z) { return (double)(z >> 11) * (1.0 / 9007199254740992.0); } };
template <> struct Uni<float>  { static float  cv(uint64_t z) { return (float)(z >> 40) * (1.0f / 16777216.0f); } };

template <class R> struct Rng {
    uint64_t state = 0, base = 0;
    uint32_t segment = 0;  // index of the world.hit call on this path (for medium draws)
    Counters* cnt = nullptr;
    double* margin = nullptr;   // PathRec::margin of the path this stream belongs to, or null
    double* tmin = nullptr;     // PathRec::tmin_margin, or null
    void decided_by(double d) { if (margin && d < *margin) *margin = d; }
    void root_at(double root, double t_min, double d_dot_n) { if (tmin) { double m = std::fabs(root - t_min) * std::fabs(d_dot_n); if (m < *tmin) *tmin = m; } }
    uint64_t next64() { state += GAMMA; if (cnt) cnt->draws++; return fin(state); }
    bool u24 = false;           // orc_sample_lights: every uniform is the device's 24-bit one, at either precision
    R random_double() { const uint64_t z = next64(); return u24 ? (R)Uni<float>::cv(z) : Uni<R>::cv(z); }   // rt_weekend.rs:8-11
    R random_double_range(R lo, R hi) { return lo + (hi - lo) * random_double(); }        // rt_weekend.rs:13-15
    uint32_t random_int(uint32_t lo, uint32_t hi) {                                       // rt_weekend.rs:16-19
        return lo + (uint32_t)std::floor(random_double() * (R)(hi - lo + 1));
    }
    uint32_t random_u32() { return (uint32_t)(next64() >> 32); }                          // rand::random::<u32>()
    uint64_t random_usize() { return next64(); }                                          // rand::random::<usize>()
};

// ------------------------------------------------------------------------------------------------
// vec3.rs
// ------------------------------------------------------------------------------------------------
template <class R> struct Vec3 {
    R e[3];
    Vec3() : e{0, 0, 0} {}
    Vec3(R a, R b, R c) : e{a, b, c} {}
    R x() const { return e[0]; } R y() const { return e[1]; } R z() const { return e[2]; }
    R length_squared() const { return e[0] * e[0] + e[1] * e[1] + e[2] * e[2]; }   // vec3.rs:26-28
    R length() const { return std::sqrt(length_squared()); }                        // vec3.rs:23-25
    Vec3 unit() const { return *this / length(); }                                  // vec3.rs:29-31
    bool near_zero() const { R s = (R)1e-8; return std::fabs(e[0]) < s && std::fabs(e[1]) < s && std::fabs(e[2]) < s; }
    Vec3 operator-() const { return Vec3(-e[0], -e[1], -e[2]); }
    Vec3 operator+(const Vec3& o) const { return Vec3(e[0] + o.e[0], e[1] + o.e[1], e[2] + o.e[2]); }
    Vec3 operator-(const Vec3& o) const { return Vec3(e[0] - o.e[0], e[1] - o.e[1], e[2] - o.e[2]); }
    Vec3 operator*(const Vec3& o) const { return Vec3(e[0] * o.e[0], e[1] * o.e[1], e[2] * o.e[2]); }
    Vec3 operator*(R t) const { return Vec3(e[0] * t, e[1] * t, e[2] * t); }
    Vec3 operator/(R t) const { return Vec3(e[0] / t, e[1] / t, e[2] / t); }   // vec3.rs:181-189: component-wise divide
    Vec3& operator+=(const Vec3& o) { e[0] += o.e[0]; e[1] += o.e[1]; e[2] += o.e[2]; return *this; }
    Vec3& operator*=(R t) { e[0] *= t; e[1] *= t; e[2] *= t; return *this; }
};
template <class R> Vec3<R> operator*(R t, const Vec3<R>& v) { return v * t; }
template <class R> R dot(const Vec3<R>& u, const Vec3<R>& v) { return u.e[0] * v.e[0] + u.e[1] * v.e[1] + u.e[2] * v.e[2]; }  // vec3.rs:64-66
template <class R> Vec3<R> cross(const Vec3<R>& u, const Vec3<R>& v) {                                                         // vec3.rs:68-76
    return Vec3<R>(u.e[1] * v.e[2] - u.e[2] * v.e[1], -(u.e[0] * v.e[2] - u.e[2] * v.e[0]), u.e[0] * v.e[1] - u.e[1] * v.e[0]);
}
template <class R> Vec3<R> reflect(const Vec3<R>& v, const Vec3<R>& n) { return v - (R)2 * dot(v, n) * n; }                    // vec3.rs:115-117
template <class R> Vec3<R> refract(const Vec3<R>& uv, const Vec3<R>& n, R etai_over_etat) {                                    // vec3.rs:246-251
    R cos_theta = std::min(dot(-uv, n), (R)1);
    Vec3<R> r_out_perp = etai_over_etat * (uv + cos_theta * n);
    Vec3<R> r_out_parallel = -std::sqrt(std::fabs((R)1 - r_out_perp.length_squared())) * n;
    return r_out_perp + r_out_parallel;
}
template <class R> Vec3<R> random_vec(Rng<R>& g) { R a = g.random_double(), b = g.random_double(), c = g.random_double(); return Vec3<R>(a, b, c); }  // vec3.rs:48-52
template <class R> Vec3<R> random_vec_range(Rng<R>& g, R lo, R hi) {                                                            // vec3.rs:53-61
    R a = g.random_double_range(lo, hi), b = g.random_double_range(lo, hi), c = g.random_double_range(lo, hi);
    return Vec3<R>(a, b, c);
}
template <class R> Vec3<R> random_in_unit_sphere(Rng<R>& g) {                                                                   // vec3.rs:78-86
    for (;;) {
        Vec3<R> p = random_vec_range(g, (R)-1, (R)1);
        g.decided_by(std::fabs((double)p.length_squared() - 1.0));
        if (p.length_squared() >= (R)1) continue;
        return p;
    }
}
template <class R> Vec3<R> random_in_unit_disk(Rng<R>& g) {                                                                     // vec3.rs:101-113
    for (;;) {
        R a = g.random_double_range((R)-1, (R)1), b = g.random_double_range((R)-1, (R)1);
        Vec3<R> p(a, b, 0);
        g.decided_by(std::fabs((double)p.length_squared() - 1.0));
        if (p.length_squared() >= (R)1) continue;
        return p;
    }
}
template <class R> R pi() { return (R)3.14159265358979323846264338327950288; }
template <class R> Vec3<R> random_cosine_direction(Rng<R>& g) {                                                                 // vec3.rs:253-262
    R r1 = g.random_double(), r2 = g.random_double();
    R z = std::sqrt((R)1 - r2);
    R phi = (R)2 * pi<R>() * r1;
    R x = std::cos(phi) * std::sqrt(r2);
    R y = std::sin(phi) * std::sqrt(r2);
    return Vec3<R>(x, y, z);
}
template <class R> Vec3<R> random_to_sphere(Rng<R>& g, R radius, R distance_sq) {                                               // pdf.rs:82-91
    R r1 = g.random_double(), r2 = g.random_double();
    R z = (R)1 + r2 * (std::sqrt((R)1 - radius * radius / distance_sq) - (R)1);
    R phi = (R)2 * pi<R>() * r1;
    R x = std::cos(phi) * std::sqrt((R)1 - z * z);
    R y = std::sin(phi) * std::sqrt((R)1 - z * z);
    return Vec3<R>(x, y, z);
}

// ray.rs:6-10
template <class R> struct Ray {
    Vec3<R> orig, dir; R tm = 0;
    Ray() {}
    Ray(const Vec3<R>& o, const Vec3<R>& d, R t) : orig(o), dir(d), tm(t) {}
    Vec3<R> at(R t) const { return orig + dir * t; }   // ray.rs:27-29
};

// onb.rs:19-42
template <class R> struct Onb {
    Vec3<R> axis[3];
    static Onb build_from_w(const Vec3<R>& n) {
        Onb o;
        o.axis[2] = n.unit();
        Vec3<R> a = (std::fabs(o.axis[2].x()) > (R)0.9) ? Vec3<R>(0, 1, 0) : Vec3<R>(1, 0, 0);
        o.axis[1] = cross(o.axis[2], a).unit();
        o.axis[0] = cross(o.axis[2], o.axis[1]);
        return o;
    }
    Vec3<R> local(const Vec3<R>& a) const { return a.x() * axis[0] + a.y() * axis[1] + a.z() * axis[2]; }
};

// aabb.rs
template <class R> struct Aabb {
    Vec3<R> mn, mx;
    Aabb() {}
    Aabb(const Vec3<R>& a, const Vec3<R>& b) : mn(a), mx(b) {}
    // The slab test aabb.rs:31-55 was meant to be (its own commented lines 151-155 of the
    // listing): the interval is carried across the three axes.
    bool hit(const Ray<R>& r, R t_min, R t_max) const {
        for (int a = 0; a < 3; ++a) {
            R inv_d = (R)1 / r.dir.e[a];
            R t0 = (mn.e[a] - r.orig.e[a]) * inv_d;
            R t1 = (mx.e[a] - r.orig.e[a]) * inv_d;
            if (inv_d < (R)0) std::swap(t0, t1);
            t_min = t_min > t0 ? t_min : t0;   // NaN-conservative like the reference: a NaN t0/t1
            t_max = t_max < t1 ? t_max : t1;   // compares false and leaves the interval unchanged
            if (t_max <= t_min) return false;
        }
        return true;
    }
    // aabb.rs:31-55 literally (quirk F7: `let t_min`/`let t_max` shadow the parameters, so each
    // axis is tested against the ORIGINAL interval). Kept for the known-answer test only.
    bool hit_reference_quirk(const Ray<R>& r, R t_min, R t_max) const {
        for (int a = 0; a < 3; ++a) {
            R inv_d = (R)1 / r.dir.e[a];
            R t0 = (mn.e[a] - r.orig.e[a]) * inv_d;
            R t1 = (mx.e[a] - r.orig.e[a]) * inv_d;
            if (inv_d < (R)0) std::swap(t0, t1);
            R lo = t_min > t0 ? t_min : t0;
            R hi = t_max < t1 ? t_max : t1;
            if (hi <= lo) return false;
        }
        return true;
    }
    static Aabb surrounding_box(const Aabb& a, const Aabb& b) {   // aabb.rs:57-69
        return Aabb(Vec3<R>(std::min(a.mn.x(), b.mn.x()), std::min(a.mn.y(), b.mn.y()), std::min(a.mn.z(), b.mn.z())),
                    Vec3<R>(std::max(a.mx.x(), b.mx.x()), std::max(a.mx.y(), b.mx.y()), std::max(a.mx.z(), b.mx.z())));
    }
};

// ------------------------------------------------------------------------------------------------
// texture.rs, perlin.rs
// ------------------------------------------------------------------------------------------------
template <class R> struct Texture {
    virtual ~Texture() {}
    virtual Vec3<R> value(R u, R v, const Vec3<R>& p, uint64_t* ev = nullptr) const = 0;   // texture.rs:7-9 (ev: a path record's event mask, or null)
};
template <class R> struct SolidColor : Texture<R> {               // texture.rs:34-38
    Vec3<R> c;
    explicit SolidColor(const Vec3<R>& c_) : c(c_) {}
    Vec3<R> value(R, R, const Vec3<R>&, uint64_t* ev) const override { if (ev) *ev |= EV_TEX_SOLID; return c; }
};
template <class R> struct CheckerTexture : Texture<R> {           // texture.rs:60-69
    std::shared_ptr<Texture<R>> even, odd;
    Vec3<R> value(R u, R v, const Vec3<R>& p, uint64_t* ev) const override {
        if (ev) *ev |= EV_TEX_CHECKER;
        R sines = std::sin((R)10 * p.x()) * std::sin((R)10 * p.y()) * std::sin((R)10 * p.z());
        return sines < (R)0 ? odd->value(u, v, p, ev) : even->value(u, v, p, ev);
    }
};
template <class R> struct Perlin {                                 // perlin.rs
    Vec3<R> ranvec[256];
    uint32_t perm_x[256], perm_y[256], perm_z[256];
    static R perlin_interp(const Vec3<R> c[2][2][2], R u, R v, R w) {   // perlin.rs:67-85
        R uu = u * u * ((R)3 - (R)2 * u);
        R vv = v * v * ((R)3 - (R)2 * v);
        R ww = w * w * ((R)3 - (R)2 * w);
        R accum = 0;
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j)
                for (int k = 0; k < 2; ++k) {
                    Vec3<R> weight_v(u - (R)i, v - (R)j, w - (R)k);
                    accum += ((R)i * uu + ((R)1 - (R)i) * ((R)1 - uu)) *
                             ((R)j * vv + ((R)1 - (R)j) * ((R)1 - vv)) *
                             ((R)k * ww + ((R)1 - (R)k) * ((R)1 - ww)) * dot(c[i][j][k], weight_v);
                }
        return accum;
    }
    R noise(const Vec3<R>& p) const {                              // perlin.rs:26-52
        R u = p.x() - std::floor(p.x());
        R v = p.y() - std::floor(p.y());
        R w = p.z() - std::floor(p.z());
        // the reference smooths here (perlin.rs:30-32) AND again inside perlin_interp (:68-70),
        // and feeds the once-smoothed value into weight_v: kept, it changes pixels.
        u = u * u * ((R)3 - (R)2 * u);
        v = v * v * ((R)3 - (R)2 * v);
        w = w * w * ((R)3 - (R)2 * w);
        int i = (int)std::floor(p.x()), j = (int)std::floor(p.y()), k = (int)std::floor(p.z());
        Vec3<R> c[2][2][2];
        for (int di = 0; di < 2; ++di)
            for (int dj = 0; dj < 2; ++dj)
                for (int dk = 0; dk < 2; ++dk)
                    c[di][dj][dk] = ranvec[perm_x[(i + di) & 255] ^ perm_y[(j + dj) & 255] ^ perm_z[(k + dk) & 255]];
        return perlin_interp(c, u, v, w);
    }
    R turb(const Vec3<R>& p) const {                               // perlin.rs:86-98
        R accum = 0; Vec3<R> temp_p = p; R weight = 1;
        for (int i = 0; i < 7; ++i) { accum += weight * noise(temp_p); weight *= (R)0.5; temp_p *= (R)2; }
        return std::fabs(accum);
    }
};
template <class R> struct NoiseTexture : Texture<R> {             // texture.rs:90-96
    std::shared_ptr<Perlin<R>> noise; R scale = 1;
    Vec3<R> value(R, R, const Vec3<R>& p, uint64_t* ev) const override {
        if (ev) *ev |= EV_TEX_NOISE;
        return Vec3<R>(1, 1, 1) * (R)0.5 * ((R)1 + std::sin(scale * p.z() + (R)10 * noise->turb(p)));
    }
};
template <class R> static R clamp(R x, R lo, R hi) { return x < lo ? lo : (x > hi ? hi : x); }   // rt_weekend.rs:21-29
template <class R> struct ImageTexture : Texture<R> {             // texture.rs:117-140
    std::vector<uint8_t> data; uint32_t width = 0, height = 0;
    Vec3<R> value(R u, R v, const Vec3<R>&, uint64_t* ev) const override {
        if (ev) *ev |= data.empty() ? EV_TEX_EMPTY_IMAGE : EV_TEX_IMAGE;
        if (data.empty()) return Vec3<R>(0, 1, 1);
        u = clamp(u, (R)0, (R)1);
        v = (R)1 - clamp(v, (R)0, (R)1);
        uint32_t i = (uint32_t)(u * (R)width), j = (uint32_t)(v * (R)height);
        if (i >= width) i = width - 1;
        if (j >= height) j = height - 1;
        R color_scale = (R)1 / (R)255;
        size_t idx = (size_t)j * (size_t)(width * 3) + (size_t)i * 3;
        return Vec3<R>(color_scale * (R)data[idx], color_scale * (R)data[idx + 1], color_scale * (R)data[idx + 2]);
    }
};

// ------------------------------------------------------------------------------------------------
// hittable.rs, material.rs, pdf.rs
// ------------------------------------------------------------------------------------------------
template <class R> struct Material;
template <class R> struct HitRecord {                             // hittable.rs:11-19
    Vec3<R> p, normal; const Material<R>* mat_ptr = nullptr; R t = 0, u = 0, v = 0; bool front_face = false;
    uint64_t tags = 0;   // EV_HIT_* of the primitive, EV_UNDER_* of the wrappers above it, EV_MEDIUM_SCATTERED (path records only)
    void set_face_normal(const Ray<R>& r, const Vec3<R>& outward_normal) {   // hittable.rs:41-48
        front_face = dot(r.dir, outward_normal) < (R)0;
        normal = front_face ? outward_normal : -outward_normal;
    }
};

// What the reference reads from thread-local state: the RNG; plus our counters.
template <class R> struct Ctx {
    Rng<R>* rng; Counters* cnt; int order; PathRec* path;   // path: null unless a path record is being filled
    void ev(uint64_t bits) { if (path) path->events |= bits; }
    uint64_t* evp() { return path ? &path->events : nullptr; }
};

template <class R> struct Hittable {                              // hittable.rs:51-60
    virtual ~Hittable() {}
    virtual bool hit(const Ray<R>& r, R t_min, R t_max, HitRecord<R>& rec, Ctx<R>& cx) const = 0;
    virtual bool bounding_box(R time0, R time1, Aabb<R>& out) const = 0;
    virtual R pdf_value(const Vec3<R>&, const Vec3<R>&, Ctx<R>&) const { return 0; }
    virtual Vec3<R> random(const Vec3<R>&, Ctx<R>&) const { return Vec3<R>(1, 0, 0); }
};

template <class R> struct Pdf {                                   // pdf.rs:7-10
    virtual ~Pdf() {}
    virtual R value(const Vec3<R>& direction, Ctx<R>& cx) const = 0;
    virtual Vec3<R> generate(Ctx<R>& cx) const = 0;
};
template <class R> struct CosinePdf : Pdf<R> {                    // pdf.rs:13-35
    Onb<R> uvw;
    explicit CosinePdf(const Vec3<R>& w) : uvw(Onb<R>::build_from_w(w)) {}
    R value(const Vec3<R>& direction, Ctx<R>&) const override {
        R cosine = dot(direction.unit(), uvw.axis[2]);
        return cosine <= (R)0 ? (R)0 : cosine / pi<R>();
    }
    Vec3<R> generate(Ctx<R>& cx) const override { return uvw.local(random_cosine_direction(*cx.rng)); }
};
template <class R> struct HittablePdf : Pdf<R> {                  // pdf.rs:38-57
    Vec3<R> o; const Hittable<R>* ptr;
    HittablePdf(const Hittable<R>* p, const Vec3<R>& origin) : o(origin), ptr(p) {}
    R value(const Vec3<R>& direction, Ctx<R>& cx) const override { return ptr->pdf_value(o, direction, cx); }
    Vec3<R> generate(Ctx<R>& cx) const override { return ptr->random(o, cx); }
};
template <class R> struct MixturePdf : Pdf<R> {                   // pdf.rs:59-80
    const Pdf<R>* p[2];
    MixturePdf(const Pdf<R>* p0, const Pdf<R>* p1) { p[0] = p0; p[1] = p1; }
    R value(const Vec3<R>& direction, Ctx<R>& cx) const override {
        return (R)0.5 * p[0]->value(direction, cx) + (R)0.5 * p[1]->value(direction, cx);
    }
    Vec3<R> generate(Ctx<R>& cx) const override {
        if (cx.rng->random_double() < (R)0.5) return p[0]->generate(cx);   // (f32 and f64 uniforms share their top bit: no margin)
        cx.ev(EV_LAMB_MIX_COSINE);
        return p[1]->generate(cx);
    }
};

template <class R> struct ScatterRecord {                         // material.rs:222-227
    Ray<R> specular_ray; bool is_specular = false; Vec3<R> attenuation; std::shared_ptr<Pdf<R>> pdf_ptr;
};
template <class R> struct Material {                              // material.rs:11-21
    virtual ~Material() {}
    virtual bool scatter(const Ray<R>&, const HitRecord<R>&, ScatterRecord<R>&, Ctx<R>&) const { return false; }
    virtual Vec3<R> emitted(const Ray<R>&, const HitRecord<R>&, R, R, const Vec3<R>&, Ctx<R>&) const { return Vec3<R>(0, 0, 0); }
    virtual R scattering_pdf(const Ray<R>&, const HitRecord<R>&, const Ray<R>&) const { return 0; }
};
template <class R> struct Lambertian : Material<R> {              // material.rs:47-72
    std::shared_ptr<Texture<R>> albedo;
    bool scatter(const Ray<R>&, const HitRecord<R>& rec, ScatterRecord<R>& srec, Ctx<R>& cx) const override {
        srec.is_specular = false;
        srec.attenuation = albedo->value(rec.u, rec.v, rec.p, cx.evp());
        srec.pdf_ptr = std::make_shared<CosinePdf<R>>(rec.normal);
        return true;
    }
    R scattering_pdf(const Ray<R>&, const HitRecord<R>& rec, const Ray<R>& scattered) const override {
        R cosine = dot(rec.normal, scattered.dir.unit());
        return cosine < (R)0 ? (R)0 : cosine / pi<R>();
    }
};
template <class R> struct Metal : Material<R> {                   // material.rs:95-108
    Vec3<R> albedo; R fuzz = 0;
    bool scatter(const Ray<R>& r_in, const HitRecord<R>& rec, ScatterRecord<R>& srec, Ctx<R>& cx) const override {
        cx.ev(EV_METAL);
        Vec3<R> reflected = reflect(r_in.dir.unit(), rec.normal);
        // random_in_unit_sphere() is drawn even when fuzz == 0; the ray's time is 0.0, not r_in.time()
        srec.specular_ray = Ray<R>(rec.p, reflected + fuzz * random_in_unit_sphere(*cx.rng), (R)0);
        srec.attenuation = albedo;
        srec.is_specular = true;
        srec.pdf_ptr = nullptr;
        return true;
    }
};
template <class R> struct Dielectric : Material<R> {              // material.rs:123-156
    R ir = (R)1.5;
    static R reflectance(R cosine, R ref_idx) {                   // material.rs:123-127
        R r0 = ((R)1 - ref_idx) / ((R)1 + ref_idx);
        r0 *= r0;
        R m = (R)1 - cosine;
        return r0 + ((R)1 - r0) * (m * m * m * m * m);            // powi(5)
    }
    bool scatter(const Ray<R>& r_in, const HitRecord<R>& rec, ScatterRecord<R>& srec, Ctx<R>& cx) const override {
        srec.is_specular = true;
        srec.pdf_ptr = nullptr;
        srec.attenuation = Vec3<R>(1, 1, 1);
        R refraction_ratio = rec.front_face ? (R)1 / ir : ir;
        Vec3<R> unit_direction = r_in.dir.unit();
        R cos_theta = std::min(dot(-unit_direction, rec.normal), (R)1);
        R sin_theta = std::sqrt((R)1 - cos_theta * cos_theta);
        bool cannot_refract = refraction_ratio * sin_theta > (R)1;
        // `||` short-circuits: no draw on total internal reflection (material.rs:146-147)
        bool reflects = cannot_refract;
        if (!rec.front_face) cx.ev(EV_DIEL_BACK_FACE);
        if (!cannot_refract) {
            const R refl = reflectance(cos_theta, refraction_ratio), draw = cx.rng->random_double();
            cx.rng->decided_by(std::fabs((double)refl - (double)draw));
            reflects = refl > draw;
        }
        cx.ev(cannot_refract ? EV_DIEL_REFLECT_TIR : (reflects ? EV_DIEL_REFLECT_SCHLICK : EV_DIEL_REFRACT));
        Vec3<R> direction = reflects ? reflect(unit_direction, rec.normal) : refract(unit_direction, rec.normal, refraction_ratio);
        srec.specular_ray = Ray<R>(rec.p, direction, r_in.tm);
        return true;
    }
};
template <class R> struct DiffuseLight : Material<R> {            // material.rs:174-191
    std::shared_ptr<Texture<R>> emit;
    Vec3<R> emitted(const Ray<R>&, const HitRecord<R>& rec, R u, R v, const Vec3<R>& p, Ctx<R>& cx) const override {
        return rec.front_face ? emit->value(u, v, p, cx.evp()) : Vec3<R>(0, 0, 0);
    }
};
// material.rs:193-220 is commented out and written against the pre-book-3 signature
// (attenuation, scattered). Under the live signature the scattered ray is fixed by the material,
// so it is returned as a "specular" ray, which the integrator follows without a pdf.
template <class R> struct Isotropic : Material<R> {
    std::shared_ptr<Texture<R>> albedo;
    bool scatter(const Ray<R>& r_in, const HitRecord<R>& rec, ScatterRecord<R>& srec, Ctx<R>& cx) const override {
        cx.ev(EV_ISOTROPIC);
        srec.specular_ray = Ray<R>(rec.p, random_in_unit_sphere(*cx.rng), r_in.tm);   // material.rs:216
        srec.attenuation = albedo->value(rec.u, rec.v, rec.p, cx.evp());                     // material.rs:217
        srec.is_specular = true;
        srec.pdf_ptr = nullptr;
        return true;
    }
};

// sphere.rs
template <class R> struct Sphere : Hittable<R> {
    Vec3<R> center; R radius = 0; const Material<R>* mat_ptr = nullptr;
    static void get_sphere_uv(const Vec3<R>& p, R& u, R& v) {     // sphere.rs:32-37
        R theta = std::acos(-p.y());
        R phi = std::atan2(-p.z(), p.x()) + pi<R>();
        u = phi / ((R)2 * pi<R>());
        v = theta / pi<R>();
    }
    bool hit(const Ray<R>& r, R t_min, R t_max, HitRecord<R>& rec, Ctx<R>& cx) const override {   // sphere.rs:41-65
        if (cx.cnt) cx.cnt->prim_tests[PT_SPHERE]++;
        Vec3<R> oc = r.orig - center;
        R a = r.dir.length_squared();
        R half_b = dot(oc, r.dir);
        R c = oc.length_squared() - radius * radius;
        R det = half_b * half_b - a * c;
        if (det < (R)0) return false;
        R sqrtd = std::sqrt(det);
        R root = (-half_b - sqrtd) / a;
        if (cx.rng->tmin) cx.rng->root_at(root, t_min, dot(r.dir, (r.at(root) - center) / radius));
        if (root < t_min || t_max < root) {
            root = (-half_b + sqrtd) / a;
            if (cx.rng->tmin) cx.rng->root_at(root, t_min, dot(r.dir, (r.at(root) - center) / radius));
            if (root < t_min || t_max < root) return false;
        }
        rec.t = root;
        rec.p = r.at(rec.t);
        Vec3<R> outward_normal = (rec.p - center) / radius;
        rec.set_face_normal(r, outward_normal);
        get_sphere_uv(outward_normal, rec.u, rec.v);
        rec.mat_ptr = mat_ptr;
        rec.tags = EV_HIT_SPHERE;
        return true;
    }
    bool bounding_box(R, R, Aabb<R>& out) const override {        // sphere.rs:66-73
        // sphere.rs:66-73 forms centre -+ radius with the signed radius: the inner sphere of a hollow glass ball (radius < 0) gets a box
        // turned inside out, and whether a ray then finds it depends on which boxes the tree happens to pair it with. |radius| here (and
        // in MovingSphere): the BVH stays a pure accelerator, as with F6.
        const R ar = std::fabs(radius);
        out = Aabb<R>(center - Vec3<R>(ar, ar, ar), center + Vec3<R>(ar, ar, ar));
        return true;
    }
    R pdf_value(const Vec3<R>& o, const Vec3<R>& v, Ctx<R>& cx) const override {   // sphere.rs:75-84
        HitRecord<R> rec;
        if (!hit(Ray<R>(o, v, 0), (R)0.001, std::numeric_limits<R>::infinity(), rec, cx)) return 0;
        R cos_theta_max = std::sqrt((R)1 - radius * radius / (center - o).length_squared());
        R solid_angle = (R)2 * pi<R>() * ((R)1 - cos_theta_max);
        return (R)1 / solid_angle;
    }
    Vec3<R> random(const Vec3<R>& o, Ctx<R>& cx) const override { // sphere.rs:85-90
        Vec3<R> direction = center - o;
        R distance_sq = direction.length_squared();
        Onb<R> uvw = Onb<R>::build_from_w(direction);
        cx.ev(EV_LAMB_LIGHT_SPHERE);
        return uvw.local(random_to_sphere(*cx.rng, radius, distance_sq));
    }
};

// moving_sphere.rs
template <class R> struct MovingSphere : Hittable<R> {
    Vec3<R> center0, center1; R time0 = 0, time1 = 1, radius = 0; const Material<R>* mat_ptr = nullptr;
    Vec3<R> center(R time) const { return center0 + ((time - time0) / (time1 - time0)) * (center1 - center0); }   // :36-39
    bool hit(const Ray<R>& r, R t_min, R t_max, HitRecord<R>& rec, Ctx<R>& cx) const override {                   // :43-66
        if (cx.cnt) cx.cnt->prim_tests[PT_MOVING]++;
        Vec3<R> oc = r.orig - center(r.tm);
        R a = r.dir.length_squared();
        R half_b = dot(oc, r.dir);
        R c = oc.length_squared() - radius * radius;
        R det = half_b * half_b - a * c;
        if (det < (R)0) return false;
        R sqrtd = std::sqrt(det);
        R root = (-half_b - sqrtd) / a;
        if (cx.rng->tmin) cx.rng->root_at(root, t_min, dot(r.dir, (r.at(root) - center(r.tm)) / radius));
        if (root < t_min || t_max < root) {
            root = (-half_b + sqrtd) / a;
            if (cx.rng->tmin) cx.rng->root_at(root, t_min, dot(r.dir, (r.at(root) - center(r.tm)) / radius));
            if (root < t_min || t_max < root) return false;
        }
        rec.t = root;
        rec.p = r.at(rec.t);
        Vec3<R> outward_normal = (rec.p - center(r.tm)) / radius;
        rec.set_face_normal(r, outward_normal);
        // u,v are NOT set by the reference (stale temp_rec values, hittable_list.rs:40-48); defined as 0.
        rec.u = 0; rec.v = 0;
        rec.mat_ptr = mat_ptr;
        rec.tags = EV_HIT_MOVING;
        return true;
    }
    bool bounding_box(R t0, R t1, Aabb<R>& out) const override {  // :67-78
        Vec3<R> rv(std::fabs(radius), std::fabs(radius), std::fabs(radius));
        Aabb<R> b0(center(t0) - rv, center(t0) + rv), b1(center(t1) - rv, center(t1) + rv);
        out = Aabb<R>::surrounding_box(b0, b1);
        return true;
    }
};

// aarect.rs — one class, axis = the constant axis (2: XyRect, 1: XzRect, 0: YzRect)
template <class R> struct AARect : Hittable<R> {
    int kaxis = 2; R a0 = 0, a1 = 0, b0 = 0, b1 = 0, k = 0; const Material<R>* mp = nullptr; bool box_side = false;
    void axes(int& ia, int& ib) const { if (kaxis == 2) { ia = 0; ib = 1; } else if (kaxis == 1) { ia = 0; ib = 2; } else { ia = 1; ib = 2; } }
    bool hit(const Ray<R>& r, R t_min, R t_max, HitRecord<R>& rec, Ctx<R>& cx) const override {   // aarect.rs:31-48, 81-98, 150-167
        if (cx.cnt) cx.cnt->prim_tests[PT_RECT]++;
        int ia, ib; axes(ia, ib);
        R t = (k - r.orig.e[kaxis]) / r.dir.e[kaxis];
        if (cx.rng->tmin && std::isfinite(t)) {
            const R pa = r.orig.e[ia] + t * r.dir.e[ia], pb = r.orig.e[ib] + t * r.dir.e[ib];
            if (!(pa < a0 || pa > a1 || pb < b0 || pb > b1)) cx.rng->root_at(t, t_min, r.dir.e[kaxis]);
        }
        if (t < t_min || t > t_max) return false;
        if (!std::isfinite(t)) return false;   // measure-zero hazard (SURVEY §8a'): never accept t = inf/NaN
        R a = r.orig.e[ia] + t * r.dir.e[ia];
        R b = r.orig.e[ib] + t * r.dir.e[ib];
        if (a < a0 || a > a1 || b < b0 || b > b1) return false;
        rec.u = (a - a0) / (a1 - a0);
        rec.v = (b - b0) / (b1 - b0);
        rec.t = t;
        Vec3<R> n(0, 0, 0); n.e[kaxis] = 1;
        rec.set_face_normal(r, n);
        rec.mat_ptr = mp;
        rec.tags = box_side ? EV_HIT_BOX_SIDE : EV_HIT_RECT;
        rec.p = r.at(t);
        return true;
    }
    bool bounding_box(R, R, Aabb<R>& out) const override {        // aarect.rs:49-56, 99-106, 168-175
        int ia, ib; axes(ia, ib);
        Vec3<R> lo, hi;
        lo.e[ia] = a0; hi.e[ia] = a1; lo.e[ib] = b0; hi.e[ib] = b1;
        lo.e[kaxis] = k - (R)0.0001; hi.e[kaxis] = k + (R)0.0001;
        out = Aabb<R>(lo, hi);
        return true;
    }
    // Only XzRect implements these (aarect.rs:107-125); Xy/Yz inherit the trait defaults.
    R pdf_value(const Vec3<R>& origin, const Vec3<R>& v, Ctx<R>& cx) const override {
        if (kaxis != 1) return 0;
        HitRecord<R> rec;
        if (!hit(Ray<R>(origin, v, 0), (R)0.001, std::numeric_limits<R>::infinity(), rec, cx)) return 0;
        R area = (a1 - a0) * (b1 - b0);
        R distance_squared = rec.t * rec.t * v.length_squared();
        R cosine = std::fabs(dot(v, rec.normal) / v.length());
        return distance_squared / cosine / area;
    }
    Vec3<R> random(const Vec3<R>& origin, Ctx<R>& cx) const override {
        if (kaxis != 1) return Vec3<R>(1, 0, 0);
        cx.ev(EV_LAMB_LIGHT_XZRECT);
        R rx = cx.rng->random_double_range(a0, a1);
        R rz = cx.rng->random_double_range(b0, b1);
        return Vec3<R>(rx, k, rz) - origin;
    }
};

// Triangle: NOT in the reference (README.md:151-153 lists OBJ as an undone optional task).
// Defined here: Moeller-Trumbore, the same inclusive [t_min,t_max] convention as the rects,
// geometric normal cross(v1-v0, v2-v0) through set_face_normal, (u,v) = barycentrics.
//
// CLOSED EDGES. A triangle is a closed set, and two triangles that share an edge leave no gap; the three barycentric tests in
// floating point do: a ray through (or within rounding of) a shared edge can compute u + v = 1 + 1e-7 in one triangle and
// v = -1e-7 in its neighbour and pass between them. So a barycentric that fails its test by no more than the test's own rounding
// error still counts as inside, and is clamped onto the edge. The bound (u0 = the unit roundoff of R, A_i = |d_j||e2_k| + |d_k||e2_j|,
// B_i = |tv_j||e1_k| + |tv_k||e1_j|: the cross products with every term taken absolutely):
//   e1, e2, tv are rounded differences (relative u0 per component); a cross product's component adds a product and a subtraction, a
//   dot product a product and two additions. So |d pv_i| <= 3 u0 A_i, |d qv_i| <= 4 u0 B_i, and the three numerators
//   Nu = tv . pv, Nv = d . qv, det = e1 . pv are each good to 7 u0 S with Su = sum |tv_i| A_i, Sv = sum |d_i| B_i, Sd = sum |e1_i| A_i.
//   u = Nu / det near 0 is then good to 7 u0 Su / |det|, v likewise, and u + v near 1 to 7 u0 (Su + Sv + Sd) / |det| plus the
//   roundings of 1 / det (2.5 u0 on the device), the two products and the sum: under 6 u0.
//   With |x| the 1-norm, sum A_i <= |d||e2| and sum B_i <= |tv||e1|, so Su + Sv + Sd <= S = |d| (|e2| (|tv| + |e1|) + |tv||e1|):
//   four norms, which is what the device can afford in registers.
//   tol = 8 u0 (S / |det| + 1) covers each of them, second-order terms included.
// Some ten ulps of 1 for a ray that meets the triangle squarely from nearby, more as the ray grazes its plane (det -> 0) or comes from
// far away (|tv|), where the barycentrics really are that uncertain; never more than 2^-10, which lets the device leave early
// without forming the bound.
// The device's tri_hit (csrc/kernels.hip) is this rule in f32, operation for operation.
template <class R> constexpr R kTriSlackMax = (R)0.0009765625;
template <class R> inline R norm1(const Vec3<R>& a) { return std::fabs(a.x()) + std::fabs(a.y()) + std::fabs(a.z()); }
template <class R> inline bool tri_close_edges(R nd, R n1, R n2, R ntv, R inv, R& u, R& v) {
    if (u < -kTriSlackMax<R> || v < -kTriSlackMax<R> || u + v > (R)1 + kTriSlackMax<R>) return false;
    const R s = nd * (n2 * (ntv + n1) + ntv * n1);
    const R tol = std::min((R)8 * (std::numeric_limits<R>::epsilon() / (R)2) * (s * std::fabs(inv) + (R)1), kTriSlackMax<R>);
    if (!(u >= -tol && v >= -tol && u + v <= (R)1 + tol)) return false;
    u = std::min(std::max(u, (R)0), (R)1);
    v = std::min(std::max(v, (R)0), (R)1 - u);
    return true;
}
template <class R> struct Triangle : Hittable<R> {
    Vec3<R> v0, v1, v2; const Material<R>* mp = nullptr;
    uint32_t aflags = 0; Vec3<R> vn[3]; R uv[3][2] = {{0, 0}, {0, 0}, {0, 0}};   // RtTriangleAttrs: flags, unit vertex normals (f32 values), uv
    bool hit(const Ray<R>& r, R t_min, R t_max, HitRecord<R>& rec, Ctx<R>& cx) const override {
        if (cx.cnt) cx.cnt->prim_tests[PT_TRI]++;
        Vec3<R> e1 = v1 - v0, e2 = v2 - v0;
        Vec3<R> pv = cross(r.dir, e2);
        R det = dot(e1, pv);
        if (det == (R)0) return false;
        R inv = (R)1 / det;
        Vec3<R> tv = r.orig - v0;
        R u = dot(tv, pv) * inv;
        if (u < -kTriSlackMax<R> || u > (R)1 + (R)2 * kTriSlackMax<R>) return false;
        Vec3<R> qv = cross(tv, e1);
        R v = dot(r.dir, qv) * inv;
        if ((u < (R)0 || u > (R)1 || v < (R)0 || u + v > (R)1) && !tri_close_edges(norm1(r.dir), norm1(e1), norm1(e2), norm1(tv), inv, u, v)) return false;
        R t = dot(e2, qv) * inv;
        if (cx.rng->tmin && std::isfinite(t)) cx.rng->root_at(t, t_min, dot(r.dir, cross(e1, e2).unit()));
        if (t < t_min || t > t_max || !std::isfinite(t)) return false;
        rec.t = t; rec.u = u; rec.v = v;
        rec.p = r.at(t);
        rec.tags = EV_HIT_TRI;
        Vec3<R> outward = cross(e1, e2).unit();
        // rt_hip.h "triangle attributes": (u, v) are the barycentrics after the closed-edge clamp
        if (aflags & RT_TRI_NORMALS) {
            const R w0 = (R)1 - u - v;
            const Vec3<R> a = w0 * vn[0], b = u * vn[1], c = v * vn[2];
            const Vec3<R> s = a + b + c;
            const R l2 = s.length_squared();
            // "not a positive normal f32 number": below FLT_MIN (zero, subnormal, negative cannot be), infinite or NaN
            const bool usable = l2 >= (R)1.17549435e-38f && l2 < std::numeric_limits<R>::infinity();
            if (usable) { outward = s.unit(); rec.tags |= EV_NORMAL_INTERP; } else rec.tags |= EV_NORMAL_FALLBACK;
            if (cx.path) {
                const double big = std::max((double)a.length_squared(), std::max((double)b.length_squared(), (double)c.length_squared()));
                const double m = std::fabs((double)l2 - 1.17549435e-38) / big;
                if (!(m >= cx.path->normal_margin)) cx.path->normal_margin = m;   // (a NaN margin sticks: undecidable)
            }
        }
        if (aflags & RT_TRI_UVS) {
            rec.u = uv[0][0] + u * (uv[1][0] - uv[0][0]) + v * (uv[2][0] - uv[0][0]);
            rec.v = uv[0][1] + u * (uv[1][1] - uv[0][1]) + v * (uv[2][1] - uv[0][1]);
            rec.tags |= EV_UV_INTERP;
        }
        rec.set_face_normal(r, outward);
        rec.mat_ptr = mp;
        return true;
    }
    bool bounding_box(R, R, Aabb<R>& out) const override {
        Vec3<R> lo, hi;
        for (int a = 0; a < 3; ++a) {
            lo.e[a] = std::min(v0.e[a], std::min(v1.e[a], v2.e[a])) - (R)0.0001;
            hi.e[a] = std::max(v0.e[a], std::max(v1.e[a], v2.e[a])) + (R)0.0001;
        }
        out = Aabb<R>(lo, hi);
        return true;
    }
};

// hittable_list.rs
template <class R> struct HittableList : Hittable<R> {
    std::vector<const Hittable<R>*> objects;
    bool hit(const Ray<R>& r, R t_min, R t_max, HitRecord<R>& rec, Ctx<R>& cx) const override {   // :39-51
        HitRecord<R> temp_rec; bool hit_anything = false; R closest_so_far = t_max;
        for (const Hittable<R>* object : objects) {
            if (object->hit(r, t_min, closest_so_far, temp_rec, cx)) {
                hit_anything = true; closest_so_far = temp_rec.t; rec = temp_rec;
            }
        }
        return hit_anything;
    }
    bool bounding_box(R t0, R t1, Aabb<R>& out) const override {  // :52-72
        if (objects.empty()) return false;
        Aabb<R> temp_box; bool first_box = true;
        for (const Hittable<R>* object : objects) {
            if (!object->bounding_box(t0, t1, temp_box)) return false;
            out = first_box ? temp_box : Aabb<R>::surrounding_box(out, temp_box);
            first_box = false;
        }
        return true;
    }
    R pdf_value(const Vec3<R>& o, const Vec3<R>& v, Ctx<R>& cx) const override {   // :73-80
        R weight = (R)1 / (R)objects.size(); R sum = 0;
        for (const Hittable<R>* object : objects) sum += weight * object->pdf_value(o, v, cx);
        return sum;
    }
    Vec3<R> random(const Vec3<R>& o, Ctx<R>& cx) const override {                  // :81-84
        uint64_t int_size = objects.size();
        return objects[cx.rng->random_usize() % int_size]->random(o, cx);
    }
};

// boxes.rs:17-83 — six rects in a HittableList, in the reference's order
template <class R> struct BoxObj : Hittable<R> {
    Vec3<R> box_min, box_max; HittableList<R> sides; std::vector<std::unique_ptr<AARect<R>>> own;
    BoxObj(const Vec3<R>& p0, const Vec3<R>& p1, const Material<R>* m) : box_min(p0), box_max(p1) {
        auto add = [&](int kaxis, R a0, R a1, R b0, R b1, R k) {
            auto q = std::make_unique<AARect<R>>();
            q->kaxis = kaxis; q->a0 = a0; q->a1 = a1; q->b0 = b0; q->b1 = b1; q->k = k; q->mp = m; q->box_side = true;
            sides.objects.push_back(q.get()); own.push_back(std::move(q));
        };
        add(2, p0.x(), p1.x(), p0.y(), p1.y(), p1.z());
        add(2, p0.x(), p1.x(), p0.y(), p1.y(), p0.z());
        add(1, p0.x(), p1.x(), p0.z(), p1.z(), p1.y());
        add(1, p0.x(), p1.x(), p0.z(), p1.z(), p0.y());
        add(0, p0.y(), p1.y(), p0.z(), p1.z(), p1.x());
        add(0, p0.y(), p1.y(), p0.z(), p1.z(), p0.x());
    }
    bool hit(const Ray<R>& r, R t_min, R t_max, HitRecord<R>& rec, Ctx<R>& cx) const override { return sides.hit(r, t_min, t_max, rec, cx); }
    bool bounding_box(R, R, Aabb<R>& out) const override { out = Aabb<R>(box_min, box_max); return true; }
};

// hittable.rs:62-96
template <class R> struct Translate : Hittable<R> {
    const Hittable<R>* ptr = nullptr; Vec3<R> offset;
    bool hit(const Ray<R>& r, R t_min, R t_max, HitRecord<R>& rec, Ctx<R>& cx) const override {
        if (cx.cnt) cx.cnt->prim_tests[PT_INSTANCE]++;
        Ray<R> moved_r(r.orig - offset, r.dir, r.tm);
        if (!ptr->hit(moved_r, t_min, t_max, rec, cx)) return false;
        rec.p += offset;
        Vec3<R> norm = rec.normal;
        rec.set_face_normal(moved_r, norm);   // normal already opposes the ray => front_face forced true
        rec.tags |= EV_UNDER_TRANSLATE;
        return true;
    }
    bool bounding_box(R t0, R t1, Aabb<R>& out) const override {
        if (!ptr->bounding_box(t0, t1, out)) return false;
        out = Aabb<R>(out.mn + offset, out.mx + offset);
        return true;
    }
};
// hittable.rs:98-181
template <class R> struct RotateY : Hittable<R> {
    const Hittable<R>* ptr = nullptr; R sin_theta = 0, cos_theta = 1; bool hasbox = false; Aabb<R> bbox;
    void construct(const Hittable<R>* p, R angle) {               // :107-144
        ptr = p;
        R radians = angle * pi<R>() / (R)180;                     // rt_weekend.rs:4-6
        sin_theta = std::sin(radians); cos_theta = std::cos(radians);
        hasbox = p->bounding_box(0, 1, bbox);
        R inf = std::numeric_limits<R>::infinity();
        Vec3<R> mini(inf, inf, inf), maxi(-inf, -inf, -inf);
        for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) for (int k = 0; k < 2; ++k) {
            R x = (R)i * bbox.mx.x() + ((R)1 - (R)i) * bbox.mn.x();
            R y = (R)j * bbox.mx.y() + ((R)1 - (R)j) * bbox.mn.y();
            R z = (R)k * bbox.mx.z() + ((R)1 - (R)k) * bbox.mn.z();
            R newx = cos_theta * x + sin_theta * z;
            R newz = -sin_theta * x + cos_theta * z;
            Vec3<R> tester(newx, y, newz);
            for (int c = 0; c < 3; ++c) { mini.e[c] = std::min(mini.e[c], tester.e[c]); maxi.e[c] = std::max(maxi.e[c], tester.e[c]); }
        }
        bbox = Aabb<R>(mini, maxi);
    }
    bool hit(const Ray<R>& r, R t_min, R t_max, HitRecord<R>& rec, Ctx<R>& cx) const override {   // :147-176
        if (cx.cnt) cx.cnt->prim_tests[PT_INSTANCE]++;
        Vec3<R> origin = r.orig, direction = r.dir;
        origin.e[0] = cos_theta * r.orig.e[0] - sin_theta * r.orig.e[2];
        origin.e[2] = sin_theta * r.orig.e[0] + cos_theta * r.orig.e[2];
        direction.e[0] = cos_theta * r.dir.e[0] - sin_theta * r.dir.e[2];
        direction.e[2] = sin_theta * r.dir.e[0] + cos_theta * r.dir.e[2];
        Ray<R> rotated_r(origin, direction, r.tm);
        if (!ptr->hit(rotated_r, t_min, t_max, rec, cx)) return false;
        Vec3<R> p = rec.p, normal = rec.normal;
        p.e[0] = cos_theta * rec.p.e[0] + sin_theta * rec.p.e[2];
        p.e[2] = -sin_theta * rec.p.e[0] + cos_theta * rec.p.e[2];
        normal.e[0] = cos_theta * rec.normal.e[0] + sin_theta * rec.normal.e[2];
        normal.e[2] = -sin_theta * rec.normal.e[0] + cos_theta * rec.normal.e[2];
        rec.p = p;
        rec.set_face_normal(rotated_r, normal);
        rec.tags |= EV_UNDER_ROTATE_Y;
        return true;
    }
    bool bounding_box(R, R, Aabb<R>& out) const override { out = bbox; return hasbox; }
};
// hittable.rs:183-205
template <class R> struct FlipFace : Hittable<R> {
    const Hittable<R>* ptr = nullptr;
    bool hit(const Ray<R>& r, R t_min, R t_max, HitRecord<R>& rec, Ctx<R>& cx) const override {
        if (!ptr->hit(r, t_min, t_max, rec, cx)) return false;
        rec.front_face = !rec.front_face;   // the flag only; the normal is untouched (:199)
        rec.tags |= EV_UNDER_FLIP_FACE;
        return true;
    }
    bool bounding_box(R t0, R t1, Aabb<R>& out) const override { return ptr->bounding_box(t0, t1, out); }
};

// ------------------------------------------------------------------------------------------------
// RtSceneDesc.scene_flags (rt_hip.h): the lights list of a scene with RT_SCENE_LIGHTS_ALL_SHAPES, and with RT_SCENE_LIGHTS_MANY. NOT in the
// reference, which samples XzRect and Sphere only; restated from the header. A member is one shape and one rigid map, the composition of the
// wrapper chain above it, as the upload makes them: the shape's parameters and the map's sine, cosine and offset are the desc's f64 values
// rounded to f32 (at either precision: it is the upload's rule, as for the vertex normals), the areas of the weighted pick are the desc's own
// f64. The member's hit test is the walk's own (AARect, Triangle with its closed edges, Sphere). With MANY the checker builds no tree: the
// list's pdf is the plain sum over all members, so a member the device's tree culls wrongly shows as a wrong sample.
// ------------------------------------------------------------------------------------------------
enum { LX_RECT = 0, LX_TRI = 1, LX_BOX = 2, LX_SPHERE = 3 };
template <class R> struct LightX {
    int kind = LX_RECT; bool wrapped = false, has_xform = false; R sin_t = 0, cos_t = 1; Vec3<R> off;
    double area = 0; float p_k = 0, cdf_k = 0;
    AARect<R> rect; Triangle<R> tri; Sphere<R> sph; R box[6] = {0, 0, 0, 0, 0, 0};   // box: x0 x1 y0 y1 z0 z1
    // side s of the box in boxes.rs order (z1 z0 y1 y0 x1 x0)
    AARect<R> side(int s) const {
        AARect<R> q; q.box_side = true;
        q.kaxis = s < 2 ? 2 : (s < 4 ? 1 : 0);
        q.a0 = s < 4 ? box[0] : box[2]; q.a1 = s < 4 ? box[1] : box[3];
        q.b0 = s < 2 ? box[2] : box[4]; q.b1 = s < 2 ? box[3] : box[5];
        q.k = s == 0 ? box[5] : s == 1 ? box[4] : s == 2 ? box[3] : s == 3 ? box[2] : s == 4 ? box[1] : box[0];
        return q;
    }
    bool new_kind() const { return kind == LX_TRI || kind == LX_BOX || (kind == LX_RECT && (rect.kaxis != 1 || wrapped)) || (kind == LX_SPHERE && wrapped); }
    Vec3<R> to_local_point(const Vec3<R>& o) const {
        if (!has_xform) return o;
        const Vec3<R> m = o - off;
        return Vec3<R>(cos_t * m.x() - sin_t * m.z(), m.y(), sin_t * m.x() + cos_t * m.z());
    }
    Vec3<R> to_local_dir(const Vec3<R>& v) const { return has_xform ? Vec3<R>(cos_t * v.x() - sin_t * v.z(), v.y(), sin_t * v.x() + cos_t * v.z()) : v; }
    Vec3<R> dir_back(const Vec3<R>& d) const { return has_xform ? Vec3<R>(cos_t * d.x() + sin_t * d.z(), d.y(), -sin_t * d.x() + cos_t * d.z()) : d; }
};
constexpr double kLightNear = 1e-4;   // a crossing this close to a member's edge is recorded even where it misses (tests/lights_cases.py EDGE_MIN)
template <class R> static void light_margins(Ctx<R>& cx, bool record, double edge, double cosine) {
    if (!record || !cx.path) return;
    if (edge < cx.path->light_edge) cx.path->light_edge = edge;
    if (cosine < cx.path->light_cos) cx.path->light_cos = cosine;
}
// aarect.rs:107-117 for every orientation: pdf = t^2 |v|^2 / (|cos| area)
template <class R> static R rectx_pdf_value(const AARect<R>& q, const Vec3<R>& o, const Vec3<R>& v, Ctx<R>& cx, bool record) {
    const R inf = std::numeric_limits<R>::infinity();
    if (record && cx.path) {
        int ia, ib; q.axes(ia, ib);
        const double t = ((double)q.k - (double)o.e[q.kaxis]) / (double)v.e[q.kaxis];
        if (!(t < 0.001) && std::isfinite(t)) {
            const double a = (double)o.e[ia] + t * (double)v.e[ia], b = (double)o.e[ib] + t * (double)v.e[ib];
            if (a > (double)q.a0 - kLightNear && a < (double)q.a1 + kLightNear && b > (double)q.b0 - kLightNear && b < (double)q.b1 + kLightNear)
                light_margins(cx, true, std::min(std::min(std::fabs(a - (double)q.a0), std::fabs((double)q.a1 - a)), std::min(std::fabs(b - (double)q.b0), std::fabs((double)q.b1 - b))), inf);
        }
    }
    HitRecord<R> rec;
    if (!q.hit(Ray<R>(o, v, 0), (R)0.001, inf, rec, cx)) return 0;
    const R area = (q.a1 - q.a0) * (q.b1 - q.b0);
    const R distance_squared = rec.t * rec.t * v.length_squared();
    const R cosine = std::fabs(dot(v, rec.normal) / v.length());
    light_margins(cx, record, inf, (double)cosine);
    return distance_squared / cosine / area;
}
template <class R> static R trix_pdf_value(const Triangle<R>& tr, const Vec3<R>& o, const Vec3<R>& v, Ctx<R>& cx, bool record) {
    const R inf = std::numeric_limits<R>::infinity();
    const Vec3<R> e1 = tr.v1 - tr.v0, e2 = tr.v2 - tr.v0;
    if (record && cx.path) {   // how far the crossing lies from the lines that decide hit or miss: the edges, and the edges moved out by the f32 rule's own bound
        const Vec3<R> pv = cross(v, e2), tv = o - tr.v0, qv = cross(tv, e1);
        const double det = (double)dot(e1, pv);
        if (det != 0.0) {
            const double inv = 1.0 / det, u = (double)dot(tv, pv) * inv, w = (double)dot(v, qv) * inv, t = (double)dot(e2, qv) * inv;
            if (!(t < 0.001) && std::isfinite(t)) {
                const double s = (double)norm1(v) * ((double)norm1(e2) * ((double)norm1(tv) + (double)norm1(e1)) + (double)norm1(tv) * (double)norm1(e1));
                const double tol = std::min(8.0 * 5.9604644775390625e-8 * (s * std::fabs(inv) + 1.0), (double)kTriSlackMax<R>);
                if (u > -tol - kLightNear && w > -tol - kLightNear && u + w < 1.0 + kLightNear + tol) {
                    double edge = std::min(std::min(std::fabs(u), std::fabs(w)), std::fabs(1.0 - (u + w)));
                    edge = std::min(edge, std::min(std::min(std::fabs(u + tol), std::fabs(w + tol)), std::fabs(1.0 + tol - (u + w))));
                    // between an edge and the edge moved out by the f32 bound the closed-edge rule answers by precision (the walk's bound is
                    // that of its own arithmetic): a hit in f32, a miss in f64, however far from both lines
                    const bool outside = u < 0.0 || w < 0.0 || u + w > 1.0;
                    if (outside && u >= -tol && w >= -tol && u + w <= 1.0 + tol) edge = 0.0;
                    light_margins(cx, true, edge, inf);
                }
            }
        }
    }
    HitRecord<R> rec;
    if (!tr.hit(Ray<R>(o, v, 0), (R)0.001, inf, rec, cx)) return 0;
    const Vec3<R> nn = cross(e1, e2);
    const R ln = nn.length();
    const R distance_squared = rec.t * rec.t * v.length_squared();
    const R cosine = std::fabs(dot(v, nn) / (v.length() * ln));
    light_margins(cx, record, inf, (double)cosine);
    return distance_squared / cosine / ((R)0.5 * ln);
}
template <class R> static Vec3<R> rectx_random(const AARect<R>& q, const Vec3<R>& o, Ctx<R>& cx) {   // aarect.rs:118-125 for every orientation
    const R ra = cx.rng->random_double_range(q.a0, q.a1);
    const R rb = cx.rng->random_double_range(q.b0, q.b1);
    return (q.kaxis == 0 ? Vec3<R>(q.k, ra, rb) : q.kaxis == 1 ? Vec3<R>(ra, q.k, rb) : Vec3<R>(ra, rb, q.k)) - o;
}
template <class R> struct LightList : Hittable<R> {
    std::vector<LightX<R>> members; bool many = false;
    bool hit(const Ray<R>&, R, R, HitRecord<R>&, Ctx<R>&) const override { return false; }   // the list is sampled, never traced
    bool bounding_box(R, R, Aabb<R>&) const override { return false; }
    R member_pdf(const LightX<R>& l, const Vec3<R>& ow, const Vec3<R>& vw, Ctx<R>& cx) const {
        const Vec3<R> o = l.to_local_point(ow), v = l.to_local_dir(vw);
        const bool record = l.new_kind();
        if (l.kind == LX_RECT) return rectx_pdf_value(l.rect, o, v, cx, record);
        if (l.kind == LX_TRI) return trix_pdf_value(l.tri, o, v, cx, record);
        if (l.kind == LX_BOX) {                                  // the list rule (hittable_list.rs:73-80) over the box's own sides
            R sum = 0;
            for (int s = 0; s < 6; ++s) sum += ((R)1 / (R)6) * rectx_pdf_value(l.side(s), o, v, cx, record);
            return sum;
        }
        return l.sph.pdf_value(o, v, cx);
    }
    Vec3<R> member_random(const LightX<R>& l, const Vec3<R>& ow, Ctx<R>& cx) const {
        const Vec3<R> o = l.to_local_point(ow);
        Vec3<R> d;
        if (l.wrapped) cx.ev(EV_LAMB_LIGHT_WRAPPED);
        if (l.kind == LX_RECT) { cx.ev(l.rect.kaxis == 1 ? EV_LAMB_LIGHT_XZRECT : EV_LAMB_LIGHT_XY_YZ_RECT); d = rectx_random(l.rect, o, cx); }
        else if (l.kind == LX_TRI) {
            cx.ev(EV_LAMB_LIGHT_TRI);
            const R r1 = cx.rng->random_double(), r2 = cx.rng->random_double();
            const R s = std::sqrt(r1);
            d = (((R)1 - s) * l.tri.v0 + (s * ((R)1 - r2)) * l.tri.v1 + (s * r2) * l.tri.v2) - o;
        } else if (l.kind == LX_BOX) {
            cx.ev(EV_LAMB_LIGHT_BOX);
            const int s = (int)(cx.rng->random_usize() % 6ull);   // hittable_list.rs:81-84 over the sides
            d = rectx_random(l.side(s), o, cx);
        } else d = l.sph.random(o, cx);
        return l.dir_back(d);
    }
    R pdf_value(const Vec3<R>& o, const Vec3<R>& v, Ctx<R>& cx) const override {
        const R weight = (R)1 / (R)members.size(); R sum = 0;
        for (const LightX<R>& l : members) sum += (many ? (R)l.p_k : weight) * member_pdf(l, o, v, cx);
        return sum;
    }
    // the pick: next64() % n, or with MANY one draw and the first member whose cdf exceeds it. That draw is the device's 24-bit uniform at
    // either precision: the pick is a look-up in an f32 table, not arithmetic that precision 64 refines.
    size_t pick(Ctx<R>& cx) const {
        if (!many) return (size_t)(cx.rng->random_usize() % (uint64_t)members.size());
        cx.ev(EV_LAMB_LIGHT_CDF_PICK);
        const float u = Uni<float>::cv(cx.rng->next64());
        size_t k = 0;
        while (k + 1 < members.size() && !(members[k].cdf_k > u)) ++k;
        for (size_t j = 0; j + 1 < members.size(); ++j) cx.rng->decided_by(std::fabs((double)u - (double)members[j].cdf_k));
        return k;
    }
    Vec3<R> random(const Vec3<R>& o, Ctx<R>& cx) const override { return member_random(members[pick(cx)], o, cx); }
};

// constant_medium.rs:31-71 (commented-out spec)
template <class R> struct ConstantMedium : Hittable<R> {
    const Hittable<R>* boundary = nullptr; const Material<R>* phase_function = nullptr; R neg_inv_density = 0; uint32_t medium_id = 0;
    bool hit(const Ray<R>& r, R t_min, R t_max, HitRecord<R>& rec, Ctx<R>& cx) const override {
        if (cx.cnt) cx.cnt->prim_tests[PT_MEDIUM]++;
        HitRecord<R> rec1, rec2;
        R inf = std::numeric_limits<R>::infinity();
        Counters* saved = cx.cnt; cx.cnt = nullptr;   // the two boundary probes are part of this one medium test
        double* saved_tmin = cx.rng->tmin; cx.rng->tmin = nullptr;   // (and their t_min is not the path's)
        bool h1 = boundary->hit(r, -inf, inf, rec1, cx);
        bool h2 = h1 && boundary->hit(r, rec1.t + (R)0.0001, inf, rec2, cx);
        cx.cnt = saved; cx.rng->tmin = saved_tmin;
        if (!h1 || !h2) return false;
        if (rec1.t < t_min) rec1.t = t_min;
        if (rec2.t > t_max) rec2.t = t_max;
        if (rec1.t >= rec2.t) return false;
        if (rec1.t < (R)0) rec1.t = 0;
        R ray_length = r.dir.length();
        R distance_inside_boundary = (rec2.t - rec1.t) * ray_length;
        // constant_medium.rs:57 draws random_double() from the sequential stream here, i.e. inside
        // traversal; this restatement keys the draw by (path, segment, medium) instead.
        R xi = Uni<R>::cv(medium_bits(cx.rng->base, cx.rng->segment, medium_id));
        R hit_distance = neg_inv_density * std::log(xi);
        cx.rng->decided_by(std::fabs((double)hit_distance - (double)distance_inside_boundary) / (double)distance_inside_boundary);
        if (hit_distance > distance_inside_boundary) { cx.ev(EV_MEDIUM_PASSED); return false; }
        rec.t = rec1.t + hit_distance / ray_length;
        rec.p = r.at(rec.t);
        rec.normal = Vec3<R>(1, 0, 0);
        rec.front_face = true;
        rec.u = 0; rec.v = 0;
        rec.mat_ptr = phase_function;
        rec.tags = EV_MEDIUM_SCATTERED;
        return true;
    }
    bool bounding_box(R t0, R t1, Aabb<R>& out) const override { return boundary->bounding_box(t0, t1, out); }
};

// bvh.rs
template <class R> struct BVHNode : Hittable<R> {
    const Hittable<R>* left = nullptr; const Hittable<R>* right = nullptr; Aabb<R> aabb;
    static R key(const Hittable<R>* h, int axis) { Aabb<R> b; h->bounding_box(0, 0, b); return b.mn.e[axis]; }   // box_compare, bvh.rs:16-55
    // bvh.rs:77-130 with the sub-range sort (F6) — `objects` is shared and sorted in place per range
    static const Hittable<R>* construct(std::vector<const Hittable<R>*>& objects, size_t start, size_t end, R time0, R time1,
                                        uint64_t& axis_state, std::vector<std::unique_ptr<Hittable<R>>>& pool) {
        axis_state += GAMMA;
        int axis = (int)((uint32_t)(fin(axis_state) >> 32) % 3u);   // bvh.rs:87
        size_t object_span = end - start;
        auto node = std::make_unique<BVHNode<R>>();
        if (object_span == 1) {
            node->left = objects[start]; node->right = nullptr;   // bvh.rs:96-98 stores it twice; tested once here
        } else if (object_span == 2) {
            if (key(objects[start], axis) < key(objects[start + 1], axis)) { node->left = objects[start]; node->right = objects[start + 1]; }
            else { node->left = objects[start + 1]; node->right = objects[start]; }
        } else {
            std::stable_sort(objects.begin() + start, objects.begin() + end,
                             [axis](const Hittable<R>* a, const Hittable<R>* b) { return key(a, axis) < key(b, axis); });
            size_t mid = start + object_span / 2;
            node->left = construct(objects, start, mid, time0, time1, axis_state, pool);
            node->right = construct(objects, mid, end, time0, time1, axis_state, pool);
        }
        Aabb<R> box_left, box_right;
        node->left->bounding_box(time0, time1, box_left);
        if (node->right) { node->right->bounding_box(time0, time1, box_right); node->aabb = Aabb<R>::surrounding_box(box_left, box_right); }
        else node->aabb = box_left;
        const Hittable<R>* out = node.get();
        pool.push_back(std::move(node));
        return out;
    }
    bool hit(const Ray<R>& r, R t_min, R t_max, HitRecord<R>& rec, Ctx<R>& cx) const override {   // bvh.rs:134-143
        if (cx.cnt) cx.cnt->node_tests++;
        if (!aabb.hit(r, t_min, t_max)) return false;
        bool hit_left = left->hit(r, t_min, t_max, rec, cx);
        bool hit_right = right ? right->hit(r, t_min, hit_left ? rec.t : t_max, rec, cx) : false;
        return hit_left || hit_right;
    }
    bool bounding_box(R, R, Aabb<R>& out) const override { out = aabb; return true; }
};

// camera.rs
template <class R> struct Camera {
    Vec3<R> origin, lower_left_corner, horizontal, vertical, u, v, w; R lens_radius = 0, time0 = 0, time1 = 0;
    Ray<R> get_ray(R s, R t, Rng<R>& g) const {                   // camera.rs:60-70
        Vec3<R> rd = lens_radius * random_in_unit_disk(g);        // drawn even when lens_radius == 0
        Vec3<R> offset = u * rd.x() + v * rd.y();
        Vec3<R> o = origin + offset;
        Vec3<R> d = lower_left_corner + horizontal * s + vertical * t - origin - offset;
        R tm = g.random_double_range(time0, time1);               // drawn even when time0 == time1
        return Ray<R>(o, d, tm);
    }
};

// ------------------------------------------------------------------------------------------------
// Scene: the RtSceneDesc graph instantiated as reference-shaped objects
// ------------------------------------------------------------------------------------------------
template <class R> static Vec3<R> V(const RtVec3& v) { return Vec3<R>((R)v.x, (R)v.y, (R)v.z); }
template <class R> static Vec3<R> V(const double* p) { return Vec3<R>((R)p[0], (R)p[1], (R)p[2]); }

template <class R> struct Scene {
    std::vector<std::shared_ptr<Texture<R>>> textures;
    std::vector<std::shared_ptr<Perlin<R>>> perlins;
    std::vector<std::unique_ptr<Material<R>>> materials;
    std::vector<const Hittable<R>*> by_id;
    std::vector<std::unique_ptr<Hittable<R>>> pool;
    const Hittable<R>* world = nullptr; const Hittable<R>* lights = nullptr;
    int background_mode = 0; Vec3<R> background;
    uint32_t n_media = 0;
    std::string error;

    std::shared_ptr<Texture<R>> build_texture(const RtSceneDesc& d, int id, int depth = 0) {
        if (id < 0 || (uint64_t)id >= d.n_textures || depth > 64) { error = "bad texture id"; return std::make_shared<SolidColor<R>>(Vec3<R>()); }
        if (textures[id]) return textures[id];
        const RtTexture& t = d.textures[id];
        std::shared_ptr<Texture<R>> out;
        switch (t.kind) {
        case RT_TEX_SOLID: out = std::make_shared<SolidColor<R>>(V<R>(t.color)); break;
        case RT_TEX_CHECKER: { auto c = std::make_shared<CheckerTexture<R>>(); c->even = build_texture(d, t.a, depth + 1); c->odd = build_texture(d, t.b, depth + 1); out = c; break; }
        case RT_TEX_NOISE: {
            auto n = std::make_shared<NoiseTexture<R>>(); n->scale = (R)t.scale;
            if (t.a < 0 || (uint64_t)t.a >= d.n_perlins) { error = "bad perlin id"; n->noise = std::make_shared<Perlin<R>>(); }
            else n->noise = perlins[t.a];
            out = n; break;
        }
        case RT_TEX_IMAGE: {
            auto im = std::make_shared<ImageTexture<R>>();
            if (t.a >= 0 && (uint64_t)t.a < d.n_images && d.images[t.a].data) {
                const RtImage& I = d.images[t.a];
                im->width = I.width; im->height = I.height; im->data.assign(I.data, I.data + (size_t)I.width * I.height * 3);
            }
            out = im; break;
        }
        default: error = "bad texture kind"; out = std::make_shared<SolidColor<R>>(Vec3<R>());
        }
        textures[id] = out;
        return out;
    }

    const Material<R>* mat(const RtSceneDesc& d, int id) {
        if (id < 0 || (uint64_t)id >= d.n_materials) { error = "bad material id"; return materials.empty() ? nullptr : materials[0].get(); }
        return materials[id].get();
    }

    const Hittable<R>* build(const RtSceneDesc& d, int id, int depth = 0) {
        if (id < 0 || (uint64_t)id >= d.n_hittables || depth > 256) { error = "bad hittable id"; return nullptr; }
        if (by_id[id]) return by_id[id];   // shared Arc (e.g. a boundary that is also in the world)
        const RtHittable& h = d.hittables[id];
        const double* p = h.p;
        std::unique_ptr<Hittable<R>> out;
        auto children = [&](std::vector<const Hittable<R>*>& v) {
            for (int c = 0; c < h.n_children; ++c) {
                uint64_t ci = (uint64_t)h.first_child + c;
                if (ci >= d.n_children) { error = "children out of range"; return; }
                const Hittable<R>* ch = build(d, d.children[ci], depth + 1);
                if (ch) v.push_back(ch);
            }
        };
        switch (h.kind) {
        case RT_HIT_SPHERE: { auto s = std::make_unique<Sphere<R>>(); s->center = V<R>(p); s->radius = (R)p[3]; s->mat_ptr = mat(d, h.material); out = std::move(s); break; }
        case RT_HIT_MOVING_SPHERE: {
            auto s = std::make_unique<MovingSphere<R>>(); s->center0 = V<R>(p); s->center1 = V<R>(p + 3);
            s->time0 = (R)p[6]; s->time1 = (R)p[7]; s->radius = (R)p[8]; s->mat_ptr = mat(d, h.material); out = std::move(s); break;
        }
        case RT_HIT_XY_RECT: case RT_HIT_XZ_RECT: case RT_HIT_YZ_RECT: {
            auto q = std::make_unique<AARect<R>>();
            q->kaxis = h.kind == RT_HIT_XY_RECT ? 2 : (h.kind == RT_HIT_XZ_RECT ? 1 : 0);
            q->a0 = (R)p[0]; q->a1 = (R)p[1]; q->b0 = (R)p[2]; q->b1 = (R)p[3]; q->k = (R)p[4]; q->mp = mat(d, h.material);
            out = std::move(q); break;
        }
        case RT_HIT_TRIANGLE: {
            auto t = std::make_unique<Triangle<R>>(); t->v0 = V<R>(p); t->v1 = V<R>(p + 3); t->v2 = V<R>(p + 6); t->mp = mat(d, h.material);
            if (!attr_of.empty() && attr_of[id] >= 0) set_attrs(*t, tri_attrs[attr_of[id]]);
            out = std::move(t); break;
        }
        case RT_HIT_BOX: out = std::make_unique<BoxObj<R>>(V<R>(p), V<R>(p + 3), mat(d, h.material)); break;
        case RT_HIT_LIST: { auto l = std::make_unique<HittableList<R>>(); children(l->objects); out = std::move(l); break; }
        case RT_HIT_BVH: {
            std::vector<const Hittable<R>*> objs; children(objs);
            if (objs.empty()) { error = "empty BVH"; return nullptr; }
            uint64_t axis_state = fin(d.bvh_seed + GAMMA * (uint64_t)(id + 1));
            const Hittable<R>* root = BVHNode<R>::construct(objs, 0, objs.size(), (R)p[0], (R)p[1], axis_state, pool);
            by_id[id] = root;
            return root;
        }
        case RT_HIT_TRANSLATE: { auto t = std::make_unique<Translate<R>>(); t->ptr = build(d, h.first_child, depth + 1); t->offset = V<R>(p); if (!t->ptr) return nullptr; out = std::move(t); break; }
        case RT_HIT_ROTATE_Y: { auto r = std::make_unique<RotateY<R>>(); const Hittable<R>* c = build(d, h.first_child, depth + 1); if (!c) return nullptr; r->construct(c, (R)p[0]); out = std::move(r); break; }
        case RT_HIT_FLIP_FACE: { auto f = std::make_unique<FlipFace<R>>(); f->ptr = build(d, h.first_child, depth + 1); if (!f->ptr) return nullptr; out = std::move(f); break; }
        case RT_HIT_CONSTANT_MEDIUM: {
            auto m = std::make_unique<ConstantMedium<R>>(); m->boundary = build(d, h.first_child, depth + 1); if (!m->boundary) return nullptr;
            m->neg_inv_density = (R)(-1.0 / p[0]);   // constant_medium.rs:25
            m->phase_function = mat(d, h.material);
            m->medium_id = (uint32_t)id;
            n_media++;
            out = std::move(m); break;
        }
        default: error = "bad hittable kind"; return nullptr;
        }
        by_id[id] = out.get();
        pool.push_back(std::move(out));
        return by_id[id];
    }

    // ---- triangle attributes (rt_hip.h RtTriangleAttrs): checked as the upload checks them, then read where the triangle is built ----
    const RtTriangleAttrs* tri_attrs = nullptr; std::vector<int64_t> attr_of;   // hittable id -> index into tri_attrs, or -1
    bool check_attrs(const RtSceneDesc& d, const RtTriangleAttrs* attrs, uint64_t n) {
        if (n == 0) return true;
        if (!attrs) { error = "n_triangle_attrs > 0 with a NULL pointer"; return false; }
        tri_attrs = attrs; attr_of.assign(d.n_hittables, -1);
        for (uint64_t i = 0; i < n; ++i) {
            const RtTriangleAttrs& a = attrs[i];
            if (a.hittable < 0 || (uint64_t)a.hittable >= d.n_hittables || d.hittables[a.hittable].kind != RT_HIT_TRIANGLE) { error = "triangle attributes: not an RT_HIT_TRIANGLE"; return false; }
            if (attr_of[a.hittable] >= 0) { error = "triangle attributes: an id listed twice"; return false; }
            if (a.flags & ~(uint32_t)(RT_TRI_NORMALS | RT_TRI_UVS)) { error = "triangle attributes: unknown flag bit"; return false; }
            for (int v = 0; v < 3; ++v) {
                if (a.flags & RT_TRI_NORMALS) {
                    const double l2 = (double)a.n[v][0] * a.n[v][0] + (double)a.n[v][1] * a.n[v][1] + (double)a.n[v][2] * a.n[v][2];
                    if (!std::isfinite(l2)) { error = "triangle attributes: a non-finite normal"; return false; }
                    if (l2 == 0.0) { error = "triangle attributes: a vertex normal of zero length"; return false; }
                }
                if ((a.flags & RT_TRI_UVS) && !(std::isfinite(a.uv[v][0]) && std::isfinite(a.uv[v][1]))) { error = "triangle attributes: a non-finite uv"; return false; }
            }
            attr_of[a.hittable] = (int64_t)i;
        }
        return true;
    }
    static void set_attrs(Triangle<R>& t, const RtTriangleAttrs& a) {
        t.aflags = a.flags;
        for (int v = 0; v < 3; ++v) {
            if (a.flags & RT_TRI_NORMALS) {   // made unit in f64, then rounded to f32: the upload's rule, at either precision
                const double x = a.n[v][0], y = a.n[v][1], z = a.n[v][2], l = std::sqrt(x * x + y * y + z * z);
                t.vn[v] = Vec3<R>((R)(float)(x / l), (R)(float)(y / l), (R)(float)(z / l));
            }
            t.uv[v][0] = (R)a.uv[v][0]; t.uv[v][1] = (R)a.uv[v][1];
        }
    }

    // ---- the lights list under RtSceneDesc.scene_flags: one LightX per member, or an error for what the header says is refused ----
    static R f32(double x) { return (R)(float)x; }
    const Hittable<R>* build_lights(const RtSceneDesc& d) {
        if (d.lights < 0 || (uint64_t)d.lights >= d.n_hittables) { error = "bad lights id"; return nullptr; }
        auto list = std::make_unique<LightList<R>>();
        list->many = (d.scene_flags & RT_SCENE_LIGHTS_MANY) != 0;
        const RtHittable& L = d.hittables[d.lights];
        std::vector<int32_t> ids;
        if (L.kind == RT_HIT_LIST) {
            for (int c = 0; c < L.n_children; ++c) {
                const uint64_t ci = (uint64_t)L.first_child + c;
                if (ci >= d.n_children) { error = "children out of range"; return nullptr; }
                ids.push_back(d.children[ci]);
            }
        } else ids.push_back(d.lights);
        if (ids.empty()) { error = "an empty lights list"; return nullptr; }
        for (int32_t hid : ids) {
            if (hid < 0 || (uint64_t)hid >= d.n_hittables) { error = "bad hittable id"; return nullptr; }
            const RtHittable* h = &d.hittables[hid];
            double theta = 0.0, off[3] = {0, 0, 0}; int ops = 0; bool identity = true;
            while (h->kind == RT_HIT_TRANSLATE || h->kind == RT_HIT_ROTATE_Y || h->kind == RT_HIT_FLIP_FACE) {
                if (h->kind == RT_HIT_TRANSLATE) {                  // the offset, turned into the frame of the rotations above it
                    const double s = std::sin(theta), k = std::cos(theta);
                    const double x = off[0] + k * h->p[0] + s * h->p[2], y = off[1] + h->p[1], z = off[2] - s * h->p[0] + k * h->p[2];
                    off[0] = x; off[1] = y; off[2] = z; identity = false;
                } else if (h->kind == RT_HIT_ROTATE_Y) { theta += h->p[0] * 3.14159265358979323846264338327950288 / 180.0; identity = false; }
                if (++ops > 6) { error = "lights list: a chain of more than 6 wrappers"; return nullptr; }
                if (h->first_child < 0 || (uint64_t)h->first_child >= d.n_hittables) { error = "bad hittable id"; return nullptr; }
                h = &d.hittables[h->first_child];
            }
            LightX<R> l; const double* p = h->p;
            switch (h->kind) {
            case RT_HIT_XY_RECT: case RT_HIT_XZ_RECT: case RT_HIT_YZ_RECT:
                if ((p[1] - p[0]) * (p[3] - p[2]) == 0.0) { error = "lights list: a rect of zero area"; return nullptr; }
                l.kind = LX_RECT; l.rect.kaxis = h->kind == RT_HIT_XY_RECT ? 2 : (h->kind == RT_HIT_XZ_RECT ? 1 : 0);
                l.rect.a0 = f32(p[0]); l.rect.a1 = f32(p[1]); l.rect.b0 = f32(p[2]); l.rect.b1 = f32(p[3]); l.rect.k = f32(p[4]);
                l.area = std::fabs((p[1] - p[0]) * (p[3] - p[2]));
                break;
            case RT_HIT_TRIANGLE: {
                const Vec3<double> a(p[3] - p[0], p[4] - p[1], p[5] - p[2]), b(p[6] - p[0], p[7] - p[1], p[8] - p[2]), n = cross(a, b);
                if (n.x() == 0.0 && n.y() == 0.0 && n.z() == 0.0) { error = "lights list: a triangle of zero area"; return nullptr; }
                l.kind = LX_TRI; l.tri.v0 = Vec3<R>(f32(p[0]), f32(p[1]), f32(p[2])); l.tri.v1 = Vec3<R>(f32(p[3]), f32(p[4]), f32(p[5])); l.tri.v2 = Vec3<R>(f32(p[6]), f32(p[7]), f32(p[8]));
                l.area = 0.5 * std::sqrt(n.length_squared());
                break;
            }
            case RT_HIT_BOX: {
                const double dx = std::fabs(p[3] - p[0]), dy = std::fabs(p[4] - p[1]), dz = std::fabs(p[5] - p[2]);
                if (dx == 0.0 || dy == 0.0 || dz == 0.0) { error = "lights list: a box with sides of zero area"; return nullptr; }
                l.kind = LX_BOX; l.box[0] = f32(p[0]); l.box[1] = f32(p[3]); l.box[2] = f32(p[1]); l.box[3] = f32(p[4]); l.box[4] = f32(p[2]); l.box[5] = f32(p[5]);
                l.area = 2.0 * (dx * dy + dy * dz + dz * dx);
                break;
            }
            case RT_HIT_SPHERE:
                l.kind = LX_SPHERE; l.sph.center = Vec3<R>(f32(p[0]), f32(p[1]), f32(p[2])); l.sph.radius = f32(p[3]);
                l.area = 4.0 * 3.14159265358979323846264338327950288 * p[3] * p[3];
                break;
            default: error = "lights list: a member that cannot be sampled as a light"; return nullptr;
            }
            l.wrapped = ops > 0; l.has_xform = !identity;
            l.sin_t = f32(std::sin(theta)); l.cos_t = f32(std::cos(theta)); l.off = Vec3<R>(f32(off[0]), f32(off[1]), f32(off[2]));
            list->members.push_back(std::move(l));
        }
        if (list->many) {   // rt_hip.h PICK: sequential f64 sums in list order, each quotient cast to float, the last cdf entry exactly 1
            double total = 0.0;
            for (const LightX<R>& l : list->members) total += l.area;
            if (!(total > 0.0 && std::isfinite(total))) { error = "lights list: the total area is not a positive finite number"; return nullptr; }
            double run = 0.0;
            for (LightX<R>& l : list->members) { run += l.area; l.p_k = (float)(l.area / total); l.cdf_k = (float)(run / total); }
            list->members.back().cdf_k = 1.0f;
        }
        const Hittable<R>* out = list.get();
        pool.push_back(std::move(list));
        return out;
    }

    bool load(const RtSceneDesc& d, const RtTriangleAttrs* attrs = nullptr, uint64_t n_attrs = 0) {
        if (d.abi_version != RT_ABI_VERSION) { error = "abi version mismatch"; return false; }
        if (d.scene_flags & ~(uint32_t)(RT_SCENE_LIGHTS_ALL_SHAPES | RT_SCENE_LIGHTS_MANY)) { error = "scene_flags: unknown bit"; return false; }
        if ((d.scene_flags & RT_SCENE_LIGHTS_MANY) && !(d.scene_flags & RT_SCENE_LIGHTS_ALL_SHAPES)) { error = "scene_flags: RT_SCENE_LIGHTS_MANY needs RT_SCENE_LIGHTS_ALL_SHAPES"; return false; }
        if (!check_attrs(d, attrs, n_attrs)) return false;
        for (uint64_t i = 0; i < d.n_perlins; ++i) {
            auto pl = std::make_shared<Perlin<R>>();
            for (int k = 0; k < 256; ++k) {
                pl->ranvec[k] = Vec3<R>((R)d.perlins[i].ranvec[k][0], (R)d.perlins[i].ranvec[k][1], (R)d.perlins[i].ranvec[k][2]);
                pl->perm_x[k] = d.perlins[i].perm_x[k]; pl->perm_y[k] = d.perlins[i].perm_y[k]; pl->perm_z[k] = d.perlins[i].perm_z[k];
            }
            perlins.push_back(pl);
        }
        textures.assign(d.n_textures, nullptr);
        for (uint64_t i = 0; i < d.n_textures; ++i) build_texture(d, (int)i);
        for (uint64_t i = 0; i < d.n_materials; ++i) {
            const RtMaterial& m = d.materials[i];
            switch (m.kind) {
            case RT_MAT_LAMBERTIAN: { auto x = std::make_unique<Lambertian<R>>(); x->albedo = build_texture(d, m.texture); materials.push_back(std::move(x)); break; }
            case RT_MAT_METAL: { auto x = std::make_unique<Metal<R>>(); x->albedo = V<R>(m.albedo); x->fuzz = (R)m.fuzz; materials.push_back(std::move(x)); break; }
            case RT_MAT_DIELECTRIC: { auto x = std::make_unique<Dielectric<R>>(); x->ir = (R)m.ir; materials.push_back(std::move(x)); break; }
            case RT_MAT_DIFFUSE_LIGHT: { auto x = std::make_unique<DiffuseLight<R>>(); x->emit = build_texture(d, m.texture); materials.push_back(std::move(x)); break; }
            case RT_MAT_ISOTROPIC: { auto x = std::make_unique<Isotropic<R>>(); x->albedo = build_texture(d, m.texture); materials.push_back(std::move(x)); break; }
            default: error = "bad material kind"; return false;
            }
        }
        by_id.assign(d.n_hittables, nullptr);
        world = build(d, d.world);
        if (d.lights >= 0) { lights = d.scene_flags ? build_lights(d) : build(d, d.lights); if (!lights) return false; }
        background_mode = d.background_mode; background = V<R>(d.background);
        return world != nullptr && error.empty();
    }
};

// ------------------------------------------------------------------------------------------------
// main.rs:63-139 ray_color — recursive, as in the reference
// ------------------------------------------------------------------------------------------------
template <class R> Vec3<R> background_color(const Scene<R>& sc, const Ray<R>& r) {
    if (sc.background_mode == RT_BG_SKY_GRADIENT) {   // book-1 sky; the reference returns the constant (main.rs:75)
        Vec3<R> ud = r.dir.unit();
        R t = (R)0.5 * (ud.y() + (R)1);
        return ((R)1 - t) * Vec3<R>(1, 1, 1) + t * sc.background;
    }
    return sc.background;
}

// A path record's perturbation: the direction rounded to f32 and moved by +-r_ulps f32 ulps per component (tests/rays.py does the same to
// a single ray) — what an f32 kernel's rounding can do to every ray of a path, not only to the first.
template <class R> Ray<R> perturbed(const Ray<R>& r, const PathRec& pr) {
    Ray<R> q = r;
    for (int c = 0; c < 3; ++c) {
        const float f = (float)r.dir.e[c], a = std::fabs(f);
        const float step = (float)pr.r_ulps * (std::nextafter(a, std::numeric_limits<float>::infinity()) - a);
        q.dir.e[c] = (R)(f + (float)pr.sign[c] * step);
    }
    return q;
}

template <class R> Vec3<R> ray_color(const Ray<R>& r_in, const Scene<R>& sc, int depth, Ctx<R>& cx) {
    HitRecord<R> rec;
    if (depth <= 0) { if (cx.path) cx.path->terminal = TERM_DEPTH; return Vec3<R>(); }       // main.rs:71-73
    Ray<R> moved;
    if (cx.path && cx.path->r_ulps > 0) moved = perturbed(r_in, *cx.path);
    const Ray<R>& r = (cx.path && cx.path->r_ulps > 0) ? moved : r_in;
    if (cx.cnt) cx.cnt->segments++;
    bool h = sc.world->hit(r, (R)0.001, std::numeric_limits<R>::infinity(), rec, cx);        // main.rs:74
    cx.rng->segment++;
    if (!h) { if (cx.path) cx.path->terminal = TERM_MISS; return background_color(sc, r); }  // main.rs:75
    cx.ev(rec.tags);
    ScatterRecord<R> srec;
    Vec3<R> emitted = rec.mat_ptr->emitted(r, rec, rec.u, rec.v, rec.p, cx);                 // main.rs:80-84
    if (!rec.mat_ptr->scatter(r, rec, srec, cx)) {                                           // main.rs:85-87
        if (cx.path) cx.path->terminal = rec.front_face ? TERM_EMITTER_FRONT : TERM_EMITTER_BACK;
        return emitted;
    }
    if (srec.is_specular) return srec.attenuation * ray_color(srec.specular_ray, sc, depth - 1, cx);   // main.rs:89-92
    Ray<R> scattered; R pdf_val;
    if (sc.lights) {
        HittablePdf<R> light_pdf(sc.lights, rec.p);                                          // main.rs:94
        MixturePdf<R> p(&light_pdf, srec.pdf_ptr.get());                                     // main.rs:95
        scattered = Ray<R>(rec.p, p.generate(cx), r.tm);                                     // main.rs:96
        pdf_val = p.value(scattered.dir, cx);                                                // main.rs:97
    } else {
        // no lights list: the reference's estimator would divide by zero (hittable_list.rs:74,82);
        // book-1/2 behaviour = sample the material's own CosinePdf (main.rs:119-121, commented)
        cx.ev(EV_LAMB_COSINE_ONLY);
        scattered = Ray<R>(rec.p, srec.pdf_ptr->generate(cx), r.tm);
        pdf_val = srec.pdf_ptr->value(scattered.dir, cx);
    }
    R spdf = rec.mat_ptr->scattering_pdf(r, rec, scattered);
    Vec3<R> rc = ray_color(scattered, sc, depth - 1, cx);
    return emitted + srec.attenuation * spdf * rc / pdf_val;                                 // main.rs:130-138
}

// main.rs:141-169
static void write_color(const double* pixel_color, uint32_t samples_per_pixel, uint8_t out[3]) {
    double c[3] = {pixel_color[0], pixel_color[1], pixel_color[2]};
    for (int i = 0; i < 3; ++i) {
        if (c[i] != c[i]) c[i] = 0.0;
        double scale = 1.0 / (double)samples_per_pixel;
        c[i] = std::sqrt(scale * c[i]);
        const double q = 256.0 * clamp(c[i], 0.0, 0.999);
        out[i] = q != q ? 0 : (uint8_t)q;   // Rust `as u8` saturates and maps NaN to 0
    }
}

}  // namespace orc

// ------------------------------------------------------------------------------------------------
// C interface (ctypes)
// ------------------------------------------------------------------------------------------------
extern "C" {

typedef struct OrcOpts {
    int32_t precision;   /* 64 = reference arithmetic, 32 = device arithmetic */
    int32_t n_threads;   /* rows are dealt round-robin to threads */
    int32_t x0, y0, x1, y1;  /* pixel rectangle to render (x1/y1 exclusive); 0,0,0,0 = full frame */
    int32_t count;       /* 1 = fill the traversal counters */
    int32_t _pad;
} OrcOpts;

typedef struct OrcStats {
    uint64_t samples, segments, node_tests, draws, nonfinite_samples;
    uint64_t prim_tests[RT_N_PRIM_TYPES];
    double seconds;
} OrcStats;

static thread_local std::string g_err;
const char* orc_last_error(void) { return g_err.c_str(); }

}  // extern "C"

namespace orc {

template <class R>
static Camera<R> camera_from(const RtCamera* cam_d) {
    Camera<R> cam;
    cam.origin = V<R>(cam_d->origin); cam.lower_left_corner = V<R>(cam_d->lower_left_corner);
    cam.horizontal = V<R>(cam_d->horizontal); cam.vertical = V<R>(cam_d->vertical);
    cam.u = V<R>(cam_d->u); cam.v = V<R>(cam_d->v); cam.w = V<R>(cam_d->w);
    cam.lens_radius = (R)cam_d->lens_radius; cam.time0 = (R)cam_d->time0; cam.time1 = (R)cam_d->time1;
    return cam;
}

// The sample loop main.rs:731-784 over the pixel rectangle [x0,x1) x [y0,y1). `compact`: rgb_sum holds the rectangle
// only (row-major, (y1-y0) x (x1-x0) x 3) instead of the whole H x W frame.
// Where orc_render_paths wants its per-sample records: arrays of [n_pixels_in_rect][spp], and the perturbation of every traced ray.
struct PathOut { uint32_t* segments; uint32_t* terminal; uint64_t* events; double* margin; double* tmin_margin; int r_ulps; int sign[3];
                 double* light_edge; double* light_cos; double* normal_margin; };   // the last three: or null

template <class R>
static int render_rect(const Scene<R>& sc, const Camera<R>& cam, const RtParams* prm, int nt, bool count, int x0, int y0, int x1, int y1, bool compact,
                       double* rgb_sum, OrcStats* st, double* per_sample /* optional: [n_pixels_in_rect][spp][3] */, const PathOut* po = nullptr) {
    const uint32_t W = prm->width, H = prm->height, spp = prm->samples_per_pixel;
    if (x0 < 0 || y0 < 0 || x1 > (int)W || y1 > (int)H || x1 <= x0 || y1 <= y0) { g_err = "bad rectangle"; return -1; }
    nt = std::max(1, nt);
    std::vector<Counters> tc(nt);
    auto t_begin = std::chrono::steady_clock::now();
    auto work = [&](int tid) {
        Counters& cnt = tc[tid];
        for (int y = y0 + tid; y < y1; y += nt) {
            const int j = (int)H - 1 - y;                                   // main.rs:733: image row y = H-1-j
            for (int x = x0; x < x1; ++x) {
                double sum[3] = {0, 0, 0};
                const uint64_t pixel_index = (uint64_t)y * W + (uint64_t)x;
                for (uint32_t s = 0; s < spp; ++s) {
                    Rng<R> g; g.base = path_base(prm->seed, pixel_index, s); g.state = g.base; g.segment = 0; g.cnt = count ? &cnt : nullptr;
                    PathRec pr;
                    if (po) { pr.r_ulps = po->r_ulps; pr.sign[0] = po->sign[0]; pr.sign[1] = po->sign[1]; pr.sign[2] = po->sign[2]; g.margin = &pr.margin; g.tmin = &pr.tmin_margin; }
                    Ctx<R> cx{&g, count ? &cnt : nullptr, 0, po ? &pr : nullptr};
                    if (cam.lens_radius > (R)0) cx.ev(EV_LENS);
                    if (cam.time0 < cam.time1) cx.ev(EV_TIME);
                    R ju = g.random_double(), jv = g.random_double();
                    R u = ((R)x + ju) / (R)(W - 1);                         // main.rs:752
                    R v = ((R)j + jv) / (R)(H - 1);                         // main.rs:753
                    Ray<R> r = cam.get_ray(u, v, g);                        // main.rs:754
                    Vec3<R> c = ray_color(r, sc, (int)prm->max_depth, cx);  // main.rs:755-761
                    cnt.samples++;
                    double cd[3] = {(double)c.e[0], (double)c.e[1], (double)c.e[2]};
                    bool finite = std::isfinite(cd[0]) && std::isfinite(cd[1]) && std::isfinite(cd[2]);
                    if (!finite) { cnt.nonfinite_samples++; if (prm->nan_policy == RT_NAN_PER_SAMPLE) cd[0] = cd[1] = cd[2] = 0.0; }
                    sum[0] += cd[0]; sum[1] += cd[1]; sum[2] += cd[2];     // main.rs:772
                    if (per_sample) {
                        size_t pi = (size_t)(y - y0) * (size_t)(x1 - x0) + (size_t)(x - x0);
                        double* o = per_sample + (pi * spp + s) * 3; o[0] = cd[0]; o[1] = cd[1]; o[2] = cd[2];
                    }
                    if (po) {
                        size_t k = ((size_t)(y - y0) * (size_t)(x1 - x0) + (size_t)(x - x0)) * spp + s;
                        po->segments[k] = g.segment; po->terminal[k] = finite ? pr.terminal : TERM_NONFINITE; po->events[k] = pr.events; po->margin[k] = pr.margin; po->tmin_margin[k] = pr.tmin_margin;
                        if (po->light_edge) po->light_edge[k] = pr.light_edge;
                        if (po->light_cos) po->light_cos[k] = pr.light_cos;
                        if (po->normal_margin) po->normal_margin[k] = pr.normal_margin;
                    }
                }
                double* o = compact ? rgb_sum + ((size_t)(y - y0) * (size_t)(x1 - x0) + (size_t)(x - x0)) * 3 : rgb_sum + ((size_t)y * W + x) * 3;
                o[0] = sum[0]; o[1] = sum[1]; o[2] = sum[2];
            }
        }
    };
    if (nt == 1) work(0);
    else { std::vector<std::thread> th; for (int t = 0; t < nt; ++t) th.emplace_back(work, t); for (auto& t : th) t.join(); }
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    if (st) {
        Counters all; for (auto& c : tc) all.add(c);
        st->samples = all.samples; st->segments = all.segments; st->node_tests = all.node_tests; st->draws = all.draws;
        st->nonfinite_samples = all.nonfinite_samples;
        for (int i = 0; i < RT_N_PRIM_TYPES; ++i) st->prim_tests[i] = all.prim_tests[i];
        st->seconds = secs;
    }
    return 0;
}

template <class R>
static int render_t(const RtSceneDesc* desc, const RtCamera* cam_d, const RtParams* prm, const OrcOpts* opt, double* rgb_sum, OrcStats* st,
                    double* per_sample, const PathOut* po = nullptr, const RtTriangleAttrs* attrs = nullptr, uint64_t n_attrs = 0) {
    Scene<R> sc;
    if (!sc.load(*desc, attrs, n_attrs)) { g_err = "scene: " + sc.error; return -1; }
    const Camera<R> cam = camera_from<R>(cam_d);
    int x0 = opt->x0, y0 = opt->y0, x1 = opt->x1, y1 = opt->y1;
    if (x1 <= x0 || y1 <= y0) { x0 = 0; y0 = 0; x1 = (int)prm->width; y1 = (int)prm->height; }
    return render_rect<R>(sc, cam, prm, opt->n_threads, opt->count != 0, x0, y0, x1, y1, false, rgb_sum, st, per_sample, po);
}

// The reference's own driver shape, main.rs:730-778: ONE PIXEL AT A TIME, `thread_num` threads spawned per pixel, each tracing
// spp / thread_num samples; the main thread adds the threads' samples in receiver order (thread 0's first) and joins them
// (the reference needs thread_num | spp: assert_eq!(cnt, SAMPLES_PER_PIXEL), main.rs:779). A timing data point only: it shows
// what the reference's threading costs beside the row-parallel port. Thread t traces samples [t*k, (t+1)*k) of the counter RNG,
// so the pixel sums equal render_rect's up to the order of the f64 additions — which is the same order (sample 0, 1, 2, ...).
template <class R>
static int render_reference_shaped(const Scene<R>& sc, const Camera<R>& cam, const RtParams* prm, int thread_num, int x0, int y0, int x1, int y1,
                                   double* rgb_sum /* compact */, OrcStats* st) {
    const uint32_t W = prm->width, H = prm->height, spp = prm->samples_per_pixel;
    if (thread_num < 1 || spp % (uint32_t)thread_num != 0) { g_err = "thread_num must divide samples_per_pixel (main.rs:779)"; return -1; }
    if (x0 < 0 || y0 < 0 || x1 > (int)W || y1 > (int)H || x1 <= x0 || y1 <= y0) { g_err = "bad rectangle"; return -1; }
    const uint32_t k = spp / (uint32_t)thread_num;
    auto t_begin = std::chrono::steady_clock::now();
    uint64_t samples = 0;
    std::vector<std::vector<Vec3<R>>> received((size_t)thread_num, std::vector<Vec3<R>>(k));
    for (int y = y0; y < y1; ++y) {                      // main.rs:731 runs j from the top row down: the same order
        const int j = (int)H - 1 - y;
        for (int x = x0; x < x1; ++x) {
            const uint64_t pixel_index = (uint64_t)y * W + (uint64_t)x;
            std::vector<std::thread> handles;
            for (int t = 0; t < thread_num; ++t) {
                handles.emplace_back([&, t] {              // main.rs:750 thread::spawn
                    for (uint32_t q = 0; q < k; ++q) {
                        const uint32_t s = (uint32_t)t * k + q;
                        Rng<R> g; g.base = path_base(prm->seed, pixel_index, s); g.state = g.base; g.segment = 0; g.cnt = nullptr;
                        Ctx<R> cx{&g, nullptr, 0, nullptr};
                        R ju = g.random_double(), jv = g.random_double();
                        R u = ((R)x + ju) / (R)(W - 1), v = ((R)j + jv) / (R)(H - 1);
                        Ray<R> r = cam.get_ray(u, v, g);
                        received[(size_t)t][q] = ray_color(r, sc, (int)prm->max_depth, cx);   // tx.send(...)
                    }
                });
            }
            for (auto& h : handles) h.join();                // the channels are drained in receiver order below (main.rs:769-775)
            double sum[3] = {0, 0, 0};
            for (int t = 0; t < thread_num; ++t)
                for (uint32_t q = 0; q < k; ++q) {
                    double cd[3] = {(double)received[(size_t)t][q].e[0], (double)received[(size_t)t][q].e[1], (double)received[(size_t)t][q].e[2]};
                    const bool finite = std::isfinite(cd[0]) && std::isfinite(cd[1]) && std::isfinite(cd[2]);
                    if (!finite && prm->nan_policy == RT_NAN_PER_SAMPLE) cd[0] = cd[1] = cd[2] = 0.0;
                    sum[0] += cd[0]; sum[1] += cd[1]; sum[2] += cd[2];
                    ++samples;
                }
            double* o = rgb_sum + ((size_t)(y - y0) * (size_t)(x1 - x0) + (size_t)(x - x0)) * 3;
            o[0] = sum[0]; o[1] = sum[1]; o[2] = sum[2];
        }
    }
    if (st) { std::memset(st, 0, sizeof(*st)); st->samples = samples; st->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); }
    return 0;
}

// Several rectangles of one frame with ONE scene build (the 1 M-primitive scene of BASELINE config 5 takes seconds to
// build): rects = n x (x0, y0, x1, y1); out = the rectangles back to back, compact; stats[n] = counters per rectangle.
template <class R>
static int render_crops_t(const RtSceneDesc* desc, const RtCamera* cam_d, const RtParams* prm, const OrcOpts* opt, int n_rects, const int32_t* rects,
                          double* out, OrcStats* stats) {
    Scene<R> sc;
    if (!sc.load(*desc)) { g_err = "scene: " + sc.error; return -1; }
    const Camera<R> cam = camera_from<R>(cam_d);
    size_t at = 0;
    for (int k = 0; k < n_rects; ++k) {
        const int32_t* q = rects + 4 * k;
        const int rc = render_rect<R>(sc, cam, prm, opt->n_threads, opt->count != 0, q[0], q[1], q[2], q[3], true, out + at, stats ? stats + k : nullptr, nullptr);
        if (rc != 0) return rc;
        at += (size_t)(q[2] - q[0]) * (size_t)(q[3] - q[1]) * 3;
    }
    return 0;
}

// world.hit for a list of rays with ONE scene build (orc_world_hit builds per call: 8 s for 1,536 rays of a 2,650-primitive scene).
template <class R>
static int world_hit_many(const RtSceneDesc* desc, uint64_t n, const double* o, const double* d, const double* tm, double t_min, const double* t_max,
                          double t_max_all, double* out10, uint8_t* hit, const RtTriangleAttrs* attrs = nullptr, uint64_t n_attrs = 0) {
    Scene<R> sc;
    if (!sc.load(*desc, attrs, n_attrs)) { g_err = "scene: " + sc.error; return -1; }
    for (uint64_t i = 0; i < n; ++i) {
        Rng<R> g; Ctx<R> cx{&g, nullptr, 0, nullptr};                        // per ray, as orc_world_hit makes them
        HitRecord<R> rec;
        const Ray<R> r(V<R>(o + 3 * i), V<R>(d + 3 * i), (R)tm[i]);
        hit[i] = sc.world->hit(r, (R)t_min, (R)(t_max ? t_max[i] : t_max_all), rec, cx) ? 1 : 0;
        if (!hit[i]) continue;
        double* q = out10 + 10 * i;
        q[0] = (double)rec.t; for (int a = 0; a < 3; ++a) { q[1 + a] = (double)rec.p.e[a]; q[4 + a] = (double)rec.normal.e[a]; }
        q[7] = (double)rec.u; q[8] = (double)rec.v; q[9] = rec.front_face ? 1.0 : 0.0;
    }
    return 0;
}

template <class R>
static int sample_lights(const RtSceneDesc* desc, uint64_t n, const float* points, const uint64_t* states, const float* dirs, double* d3, double* pdf,
                         int32_t* light, uint32_t* n_draws, double* edge, double* cosine) {
    Scene<R> sc;
    if (!sc.load(*desc)) { g_err = "scene: " + sc.error; return -1; }
    const auto* list = dynamic_cast<const LightList<R>*>(sc.lights);
    if (!list) { g_err = "no lights list"; return -1; }
    for (uint64_t i = 0; i < n; ++i) {
        Counters cnt;
        Rng<R> g; g.u24 = true; g.cnt = &cnt; if (states) { g.state = states[i]; g.base = states[i]; }
        PathRec pr;
        Ctx<R> cx{&g, nullptr, 0, &pr};
        const Vec3<R> o((R)points[3 * i], (R)points[3 * i + 1], (R)points[3 * i + 2]);
        Vec3<R> d;
        if (dirs) { d = Vec3<R>((R)dirs[3 * i], (R)dirs[3 * i + 1], (R)dirs[3 * i + 2]); light[i] = -1; }
        else { const size_t k = list->pick(cx); light[i] = (int32_t)k; d = list->member_random(list->members[k], o, cx); }
        n_draws[i] = (uint32_t)cnt.draws;
        pdf[i] = (double)list->pdf_value(o, d, cx);
        for (int a = 0; a < 3; ++a) d3[3 * i + a] = (double)d.e[a];
        if (edge) edge[i] = pr.light_edge;
        if (cosine) cosine[i] = pr.light_cos;
    }
    return 0;
}

}  // namespace orc

extern "C" {

/* Render rgb_sum(H*W*3 doubles, row 0 = top; only the requested rectangle is written). */
int orc_render(const RtSceneDesc* desc, const RtCamera* cam, const RtParams* prm, const OrcOpts* opt, double* rgb_sum, OrcStats* st) {
    if (!desc || !cam || !prm || !opt || !rgb_sum) { g_err = "null argument"; return -1; }
    if (opt->precision == 32) return orc::render_t<float>(desc, cam, prm, opt, rgb_sum, st, nullptr);
    return orc::render_t<double>(desc, cam, prm, opt, rgb_sum, st, nullptr);
}

/* Same, and also every sample's radiance: per_sample[(pixel_in_rect*spp + s)*3 + c]. */
int orc_render_samples(const RtSceneDesc* desc, const RtCamera* cam, const RtParams* prm, const OrcOpts* opt, double* rgb_sum, double* per_sample, OrcStats* st) {
    if (!desc || !cam || !prm || !opt || !rgb_sum || !per_sample) { g_err = "null argument"; return -1; }
    if (opt->precision == 32) return orc::render_t<float>(desc, cam, prm, opt, rgb_sum, st, per_sample);
    return orc::render_t<double>(desc, cam, prm, opt, rgb_sum, st, per_sample);
}

/* orc_render_samples, and for every sample the record of its path: the number of world.hit calls, how it ended (0 miss -> background,
 * 1 emitter seen from the front, 2 from the back, 3 depth exhausted, 4 non-finite: the radiance is scrubbed under RT_NAN_PER_SAMPLE), the
 * mask of the branches it took (the EV_* bits above; oracle/binding.py names them) and the smallest margin by which one of its
 * random-number thresholds was decided: | |p|^2 - 1 | of every rejection test, |reflectance - draw|, |free path - distance| / distance.
 * tmin_margin: the smallest |root - t_min| * |d . n| over the primitive tests of the path (n the unit normal at that root): the distance by
 * which the ray's origin would have to move along the normal to carry that root across t_min (a medium's boundary probes left out).
 * r_ulps > 0 rounds the direction of every ray the path traces to f32 and moves it by sign[c] * r_ulps f32 ulps per component.
 * Arrays of [pixels in rect][spp]; radiance is f64 at either precision. */
int orc_render_paths(const RtSceneDesc* desc, const RtCamera* cam, const RtParams* prm, const OrcOpts* opt, int32_t r_ulps, const int32_t* sign3, double* rgb_sum,
                     double* per_sample, uint32_t* segments, uint32_t* terminal, uint32_t* events, double* margin, double* tmin_margin, OrcStats* st) {
    if (!desc || !cam || !prm || !opt || !rgb_sum || !per_sample || !segments || !terminal || !events || !margin || !tmin_margin || (r_ulps > 0 && !sign3) || r_ulps < 0) {
        g_err = "null argument"; return -1;
    }
    int x0 = opt->x0, y0 = opt->y0, x1 = opt->x1, y1 = opt->y1;
    if (x1 <= x0 || y1 <= y0) { x0 = 0; y0 = 0; x1 = (int)prm->width; y1 = (int)prm->height; }
    std::vector<uint64_t> wide((size_t)std::max(0, x1 - x0) * (size_t)std::max(0, y1 - y0) * prm->samples_per_pixel);
    orc::PathOut po{segments, terminal, wide.data(), margin, tmin_margin, r_ulps, {1, 1, 1}, nullptr, nullptr, nullptr};
    if (r_ulps > 0) for (int c = 0; c < 3; ++c) po.sign[c] = sign3[c] < 0 ? -1 : 1;
    const int rc = opt->precision == 32 ? orc::render_t<float>(desc, cam, prm, opt, rgb_sum, st, per_sample, &po)
                                        : orc::render_t<double>(desc, cam, prm, opt, rgb_sum, st, per_sample, &po);
    if (rc == 0) for (size_t k = 0; k < wide.size(); ++k) events[k] = (uint32_t)wide[k];   // the bits this entry point has always had
    return rc;
}

/* orc_render_paths for scenes with RtSceneDesc.scene_flags and triangle attributes (attrs: the RtTriangleAttrs array that travels beside the
 * desc, or NULL with n_attrs 0). events is 64 bits wide (bits 27 and up: oracle/binding.py names them). Three more margins per sample:
 * light_edge / light_cos: over the list-pdf evaluations against lights of a kind the reference has not, the smallest distance of a crossing
 * from the member's edge (rects: scene units, triangles: barycentrics; near misses count) and the smallest |cos| at a member that is met;
 * normal_margin: over the interpolated normals, the smallest | |sum|^2 - FLT_MIN | / (largest term)^2. inf where nothing was recorded. */
int orc_render_paths_ex(const RtSceneDesc* desc, const RtCamera* cam, const RtParams* prm, const OrcOpts* opt, const RtTriangleAttrs* attrs, uint64_t n_attrs,
                        int32_t r_ulps, const int32_t* sign3, double* rgb_sum, double* per_sample, uint32_t* segments, uint32_t* terminal, uint64_t* events,
                        double* margin, double* tmin_margin, double* light_edge, double* light_cos, double* normal_margin, OrcStats* st) {
    if (!desc || !cam || !prm || !opt || !rgb_sum || !per_sample || !segments || !terminal || !events || !margin || !tmin_margin || !light_edge || !light_cos ||
        !normal_margin || (r_ulps > 0 && !sign3) || r_ulps < 0) {
        g_err = "null argument"; return -1;
    }
    orc::PathOut po{segments, terminal, events, margin, tmin_margin, r_ulps, {1, 1, 1}, light_edge, light_cos, normal_margin};
    if (r_ulps > 0) for (int c = 0; c < 3; ++c) po.sign[c] = sign3[c] < 0 ? -1 : 1;
    if (opt->precision == 32) return orc::render_t<float>(desc, cam, prm, opt, rgb_sum, st, per_sample, &po, attrs, n_attrs);
    return orc::render_t<double>(desc, cam, prm, opt, rgb_sum, st, per_sample, &po, attrs, n_attrs);
}

/* n_rects rectangles (x0, y0, x1, y1 each) of one frame, scene built once; out = the rectangles back to back (compact). */
int orc_render_crops(const RtSceneDesc* desc, const RtCamera* cam, const RtParams* prm, const OrcOpts* opt, int32_t n_rects, const int32_t* rects, double* out,
                     OrcStats* stats) {
    if (!desc || !cam || !prm || !opt || !rects || !out || n_rects <= 0) { g_err = "null argument"; return -1; }
    if (opt->precision == 32) return orc::render_crops_t<float>(desc, cam, prm, opt, n_rects, rects, out, stats);
    return orc::render_crops_t<double>(desc, cam, prm, opt, n_rects, rects, out, stats);
}

/* main.rs:730-778 as written: one pixel at a time, thread_num threads per pixel (f64). out = the rectangle, compact. */
int orc_render_reference_shaped(const RtSceneDesc* desc, const RtCamera* cam, const RtParams* prm, int32_t thread_num, const int32_t* rect4, double* out,
                                OrcStats* st) {
    if (!desc || !cam || !prm || !rect4 || !out) { g_err = "null argument"; return -1; }
    orc::Scene<double> sc;
    if (!sc.load(*desc)) { g_err = "scene: " + sc.error; return -1; }
    const orc::Camera<double> c = orc::camera_from<double>(cam);
    return orc::render_reference_shaped<double>(sc, c, prm, thread_num, rect4[0], rect4[1], rect4[2], rect4[3], out, st);
}

void orc_write_color(const double* pixel_color, uint32_t samples_per_pixel, uint8_t* out3) { orc::write_color(pixel_color, samples_per_pixel, out3); }

/* ---- known-answer-test hooks: one reference function each, f64 ---- */
using VD = orc::Vec3<double>;

/* camera.rs:21-59 Camera::new */
void orc_camera_new(const double* lookfrom, const double* lookat, const double* vup, const double* scope4, double time0, double time1, RtCamera* out) {
    double vfov = scope4[0], aspect_ratio = scope4[1], aperture = scope4[2], focus_dist = scope4[3];
    double theta = vfov * orc::pi<double>() / 180.0;
    double h = std::tan(theta / 2.0);
    double viewport_height = 2.0 * h, viewport_width = aspect_ratio * viewport_height;
    VD lf(lookfrom[0], lookfrom[1], lookfrom[2]), la(lookat[0], lookat[1], lookat[2]), up(vup[0], vup[1], vup[2]);
    VD w = (lf - la).unit();
    VD u = orc::cross(up, w).unit();
    VD v = orc::cross(w, u);
    VD origin = lf, horizontal = focus_dist * viewport_width * u, vertical = focus_dist * viewport_height * v;
    VD llc = origin - horizontal / 2.0 - vertical / 2.0 - focus_dist * w;
    auto S = [](RtVec3& d, const VD& s) { d.x = s.e[0]; d.y = s.e[1]; d.z = s.e[2]; };
    S(out->origin, origin); S(out->lower_left_corner, llc); S(out->horizontal, horizontal); S(out->vertical, vertical);
    S(out->u, u); S(out->v, v); S(out->w, w);
    out->lens_radius = aperture / 2.0; out->time0 = time0; out->time1 = time1;
}

/* sphere.rs:41-65 — out = t, p[3], normal[3], u, v, front_face */
int orc_sphere_hit(const double* center, double radius, const double* o, const double* d, double tm, double t_min, double t_max, double* out10) {
    orc::Sphere<double> s; s.center = VD(center[0], center[1], center[2]); s.radius = radius;
    orc::Rng<double> g; orc::Ctx<double> cx{&g, nullptr, 0, nullptr};
    orc::HitRecord<double> rec;
    if (!s.hit(orc::Ray<double>(VD(o[0], o[1], o[2]), VD(d[0], d[1], d[2]), tm), t_min, t_max, rec, cx)) return 0;
    out10[0] = rec.t; for (int i = 0; i < 3; ++i) { out10[1 + i] = rec.p.e[i]; out10[4 + i] = rec.normal.e[i]; }
    out10[7] = rec.u; out10[8] = rec.v; out10[9] = rec.front_face ? 1.0 : 0.0;
    return 1;
}
double orc_sphere_pdf_value(const double* center, double radius, const double* o, const double* v) {
    orc::Sphere<double> s; s.center = VD(center[0], center[1], center[2]); s.radius = radius;
    orc::Rng<double> g; orc::Ctx<double> cx{&g, nullptr, 0, nullptr};
    return s.pdf_value(VD(o[0], o[1], o[2]), VD(v[0], v[1], v[2]), cx);
}
/* aarect.rs — kaxis 2/1/0 = Xy/Xz/Yz; out as orc_sphere_hit */
int orc_rect_hit(int kaxis, const double* abk5, const double* o, const double* d, double t_min, double t_max, double* out10) {
    orc::AARect<double> q; q.kaxis = kaxis; q.a0 = abk5[0]; q.a1 = abk5[1]; q.b0 = abk5[2]; q.b1 = abk5[3]; q.k = abk5[4];
    orc::Rng<double> g; orc::Ctx<double> cx{&g, nullptr, 0, nullptr};
    orc::HitRecord<double> rec;
    if (!q.hit(orc::Ray<double>(VD(o[0], o[1], o[2]), VD(d[0], d[1], d[2]), 0), t_min, t_max, rec, cx)) return 0;
    out10[0] = rec.t; for (int i = 0; i < 3; ++i) { out10[1 + i] = rec.p.e[i]; out10[4 + i] = rec.normal.e[i]; }
    out10[7] = rec.u; out10[8] = rec.v; out10[9] = rec.front_face ? 1.0 : 0.0;
    return 1;
}
double orc_xzrect_pdf_value(const double* abk5, const double* o, const double* v) {
    orc::AARect<double> q; q.kaxis = 1; q.a0 = abk5[0]; q.a1 = abk5[1]; q.b0 = abk5[2]; q.b1 = abk5[3]; q.k = abk5[4];
    orc::Rng<double> g; orc::Ctx<double> cx{&g, nullptr, 0, nullptr};
    return q.pdf_value(VD(o[0], o[1], o[2]), VD(v[0], v[1], v[2]), cx);
}
void orc_onb_build_from_w(const double* n, double* out9) {
    orc::Onb<double> o = orc::Onb<double>::build_from_w(VD(n[0], n[1], n[2]));
    for (int a = 0; a < 3; ++a) for (int i = 0; i < 3; ++i) out9[a * 3 + i] = o.axis[a].e[i];
}
double orc_reflectance(double cosine, double ref_idx) { return orc::Dielectric<double>::reflectance(cosine, ref_idx); }
void orc_refract(const double* uv, const double* n, double ratio, double* out3) {
    VD r = orc::refract(VD(uv[0], uv[1], uv[2]), VD(n[0], n[1], n[2]), ratio); out3[0] = r.e[0]; out3[1] = r.e[1]; out3[2] = r.e[2];
}
void orc_reflect(const double* v, const double* n, double* out3) {
    VD r = orc::reflect(VD(v[0], v[1], v[2]), VD(n[0], n[1], n[2])); out3[0] = r.e[0]; out3[1] = r.e[1]; out3[2] = r.e[2];
}
/* aabb.rs:31-55: quirk=1 evaluates the literal per-axis-shadowed test, quirk=0 the carried interval */
int orc_aabb_hit(const double* mn, const double* mx, const double* o, const double* d, double t_min, double t_max, int quirk) {
    orc::Aabb<double> b(VD(mn[0], mn[1], mn[2]), VD(mx[0], mx[1], mx[2]));
    orc::Ray<double> r(VD(o[0], o[1], o[2]), VD(d[0], d[1], d[2]), 0);
    return quirk ? b.hit_reference_quirk(r, t_min, t_max) : b.hit(r, t_min, t_max);
}
/* world.hit on a scene graph, f64: returns 1 and t, p, normal, u, v, front_face */
int orc_world_hit(const RtSceneDesc* desc, const double* o, const double* d, double tm, double t_min, double t_max, double* out10) {
    orc::Scene<double> sc;
    if (!sc.load(*desc)) { g_err = "scene: " + sc.error; return -1; }
    orc::Rng<double> g; orc::Ctx<double> cx{&g, nullptr, 0, nullptr};
    orc::HitRecord<double> rec;
    if (!sc.world->hit(orc::Ray<double>(VD(o[0], o[1], o[2]), VD(d[0], d[1], d[2]), tm), t_min, t_max, rec, cx)) return 0;
    out10[0] = rec.t; for (int i = 0; i < 3; ++i) { out10[1 + i] = rec.p.e[i]; out10[4 + i] = rec.normal.e[i]; }
    out10[7] = rec.u; out10[8] = rec.v; out10[9] = rec.front_face ? 1.0 : 0.0;
    return 1;
}
/* world.hit for n rays of ONE scene, loaded (BVH build included) once: o, d are n x 3, tm is n; t_max is per ray, or NULL for the scalar
   t_max_all. precision 64 runs orc_world_hit's own code path ray by ray (same bits); 32 the Scene<float> instance, its record widened.
   Writes out10[10 * i ..] as orc_world_hit does (untouched on a miss) and hit[i] = 0 / 1. Returns 0, or -1 with the reason in orc_last_error. */
int orc_world_hit_many(const RtSceneDesc* desc, uint64_t n, const double* o, const double* d, const double* tm, double t_min, const double* t_max,
                       double t_max_all, int precision, double* out10, uint8_t* hit) {
    if (!desc || (n && (!o || !d || !tm || !out10 || !hit))) { g_err = "null argument"; return -1; }
    if (precision != 64 && precision != 32) { g_err = "precision must be 64 or 32"; return -1; }
    return precision == 64 ? orc::world_hit_many<double>(desc, n, o, d, tm, t_min, t_max, t_max_all, out10, hit)
                           : orc::world_hit_many<float>(desc, n, o, d, tm, t_min, t_max, t_max_all, out10, hit);
}
/* orc_world_hit_many with triangle attributes: normal, u, v and front_face of a hit on a triangle that carries some are the interpolated ones */
int orc_world_hit_many_ex(const RtSceneDesc* desc, const RtTriangleAttrs* attrs, uint64_t n_attrs, uint64_t n, const double* o, const double* d, const double* tm,
                          double t_min, const double* t_max, double t_max_all, int precision, double* out10, uint8_t* hit) {
    if (!desc || (n && (!o || !d || !tm || !out10 || !hit))) { g_err = "null argument"; return -1; }
    if (precision != 64 && precision != 32) { g_err = "precision must be 64 or 32"; return -1; }
    return precision == 64 ? orc::world_hit_many<double>(desc, n, o, d, tm, t_min, t_max, t_max_all, out10, hit, attrs, n_attrs)
                           : orc::world_hit_many<float>(desc, n, o, d, tm, t_min, t_max, t_max_all, out10, hit, attrs, n_attrs);
}
/* The lights list of a scene with scene_flags set, queried as rt_sample_lights queries it: for point i (f32) and generator state i one pick,
 * the picked member's draw and the list's pdf of the drawn direction; with dirs (f32, n x 3) the list's pdf of the given directions and no
 * draw (light -1). Every uniform is the device's 24-bit one at either precision. d (n x 3) and pdf are widened to f64. edge, cosine (or NULL):
 * the margins orc_render_paths_ex calls light_edge and light_cos, for the one evaluation of the list's pdf. */
int orc_sample_lights(const RtSceneDesc* desc, uint64_t n, const float* points, const uint64_t* states, const float* dirs, int precision, double* d3, double* pdf,
                      int32_t* light, uint32_t* n_draws, double* edge, double* cosine) {
    if (!desc || (n && (!points || (!states && !dirs) || !d3 || !pdf || !light || !n_draws))) { g_err = "null argument"; return -1; }
    if (precision != 64 && precision != 32) { g_err = "precision must be 64 or 32"; return -1; }
    if (!desc->scene_flags || desc->lights < 0) { g_err = "orc_sample_lights needs a lights list and scene_flags"; return -1; }
    return precision == 64 ? orc::sample_lights<double>(desc, n, points, states, dirs, d3, pdf, light, n_draws, edge, cosine)
                           : orc::sample_lights<float>(desc, n, points, states, dirs, d3, pdf, light, n_draws, edge, cosine);
}
/* p and cdf of the weighted pick (RT_SCENE_LIGHTS_MANY), by member in list order; returns the number of members, or -1 */
int orc_light_weights(const RtSceneDesc* desc, float* p, float* cdf, uint64_t cap) {
    if (!desc || !p || !cdf) { g_err = "null argument"; return -1; }
    orc::Scene<double> sc;
    if (!sc.load(*desc)) { g_err = "scene: " + sc.error; return -1; }
    const auto* list = dynamic_cast<const orc::LightList<double>*>(sc.lights);
    if (!list || !list->many) { g_err = "not a scene with RT_SCENE_LIGHTS_MANY"; return -1; }
    if (list->members.size() > cap) { g_err = "cap too small"; return -1; }
    for (size_t k = 0; k < list->members.size(); ++k) { p[k] = list->members[k].p_k; cdf[k] = list->members[k].cdf_k; }
    return (int)list->members.size();
}
/* texture value of texture `id` of a scene, f64 */
int orc_texture_value(const RtSceneDesc* desc, int id, double u, double v, const double* p, double* out3) {
    orc::Scene<double> sc;
    if (!sc.load(*desc)) { g_err = "scene: " + sc.error; return -1; }
    if (id < 0 || (size_t)id >= sc.textures.size()) { g_err = "bad texture id"; return -1; }
    VD c = sc.textures[id]->value(u, v, VD(p[0], p[1], p[2])); out3[0] = c.e[0]; out3[1] = c.e[1]; out3[2] = c.e[2];
    return 0;
}
/* the first n uniform draws of path (seed, pixel_index, sample_index), f64 and f32 conversions */
void orc_rng_stream(uint64_t seed, uint64_t pixel_index, uint64_t sample_index, uint32_t n, uint64_t* raw, double* as_f64, float* as_f32) {
    uint64_t state = orc::path_base(seed, pixel_index, sample_index);
    for (uint32_t i = 0; i < n; ++i) {
        state += orc::GAMMA; uint64_t z = orc::fin(state);
        if (raw) raw[i] = z;
        if (as_f64) as_f64[i] = orc::Uni<double>::cv(z);
        if (as_f32) as_f32[i] = orc::Uni<float>::cv(z);
    }
}
/* leaves of BVH hittable `id` in left-to-right order (for builder parity): writes hittable ids */
int orc_bvh_leaf_order(const RtSceneDesc* desc, int id, int32_t* out_ids, uint64_t cap);

}  // extern "C"

namespace orc {
template <class R> static void collect_leaves(const Hittable<R>* h, const std::vector<const Hittable<R>*>& by_id, std::vector<int32_t>& out) {
    if (auto n = dynamic_cast<const BVHNode<R>*>(h)) { collect_leaves(n->left, by_id, out); if (n->right) collect_leaves(n->right, by_id, out); return; }
    for (size_t i = 0; i < by_id.size(); ++i) if (by_id[i] == h) { out.push_back((int32_t)i); return; }
    out.push_back(-1);
}
}  // namespace orc

extern "C" int orc_bvh_leaf_order(const RtSceneDesc* desc, int id, int32_t* out_ids, uint64_t cap) {
    orc::Scene<double> sc;
    if (!sc.load(*desc)) { g_err = "scene: " + sc.error; return -1; }
    if (id < 0 || (size_t)id >= sc.by_id.size() || !sc.by_id[id]) { g_err = "bad id"; return -1; }
    std::vector<int32_t> v;
    // nested BVHs are leaves of this one: hide the root's own id while matching
    std::vector<const orc::Hittable<double>*> ids = sc.by_id; ids[id] = nullptr;
    orc::collect_leaves<double>(sc.by_id[id], ids, v);
    if (v.size() > cap) { g_err = "cap too small"; return -1; }
    for (size_t i = 0; i < v.size(); ++i) out_ids[i] = v[i];
    return (int)v.size();
}
