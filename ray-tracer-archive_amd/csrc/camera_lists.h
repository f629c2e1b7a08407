// camera_lists.h — which spheres can a camera ray of one 8 x 8-pixel square of the image meet? ("Camera lists")
// ONE predicate, in f64, for the host (rt_api.cpp rt_camera_lists_host) and the device (kernels.hip k_camera_lists): under -ffp-contract=off
// both evaluate the same IEEE operations in the same order and give the same lists.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_CL_HD __host__ __device__
#else
#define RT_CL_HD
#endif

namespace rtcl {

constexpr uint32_t kSquare = 8u;             // a square is 8 x 8 pixels, keyed by the GLOBAL pixel: (x >> 3, y >> 3)
constexpr uint32_t kListMax = 16u;           // K: spheres a list holds
constexpr uint32_t kListWords = kListMax + 1u;   // a list: its count, then K sphere indices in the order the walk reaches their leaves
constexpr uint32_t kWalk = 0xFFFFFFFFu;      // count word of a square with more than K candidates: its rays are walked as without lists

// the camera as new_camera_ray reads it (RenderDev: the f32 values, widened), and the frame. lens_radius is the radius of the ball around
// `org` that holds every ray origin: new_camera_ray offsets the origin by R (u px + v py) with (px, py) in the unit disk, so it is R times
// the largest singular value of [u v] (lens_reach below) — R itself for the orthonormal u, v of Camera::new, and right for any others.
struct Camera { double org[3], llc[3], hor[3], ver[3], lens_radius; uint32_t width, height; };
// max |u px + v py| over the unit disk: the root of the larger eigenvalue of the Gram matrix [[u.u, u.v], [u.v, v.v]]
inline double lens_reach(const double u[3], const double v[3]) {
    const double a = u[0] * u[0] + u[1] * u[1] + u[2] * u[2], c = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], b = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
    const double h = 0.5 * (a - c);
    return sqrt(0.5 * (a + c) + sqrt(h * h + b * b));
}

// What bounds the rays of one square. Every ray is the line through a lens point A, |A - O| <= R (R = Camera::lens_radius), and a point Q of the focal plane,
// |Q - Qc| <= rho, so at parameter u (the ray's own t: d = Q - A) it is the point A + u (Q - A) = X(u) + (1 - u)(A - O) + u (Q - Qc) with
// X(u) = O + u (Qc - O) on the AXIS of the square: it stays within  slack(u) = |1 - u| R + u rho  of X(u).
struct Cone {
    double o[3], e[3];     // lens centre O; unit direction of the axis, (Qc - O) / L
    double L, R, rho;      // |Qc - O|; lens radius and half diagonal of the square's patch of the focal plane, each with the rounding allowance
    uint32_t ok;           // 0: no bound (a frame one pixel wide or high, or a lens as large as the focus distance): every sphere is kept
};

RT_CL_HD inline Cone square_cone(const Camera& c, uint32_t sx, uint32_t sy) {
    Cone k{};
    if (c.width < 2u || c.height < 2u) return k;
    // pixels [x0, x1] x [y0, y1]; u = (x + ju) / (W - 1), v = (H - 1 - y + jv) / (H - 1) with ju, jv in [0, 1] (a jitter below 1 can round
    // the f32 sum up to the next integer: the interval is closed)
    const uint32_t x0 = sx * kSquare, y0 = sy * kSquare;
    const uint32_t x1 = x0 + kSquare - 1u < c.width - 1u ? x0 + kSquare - 1u : c.width - 1u, y1 = y0 + kSquare - 1u < c.height - 1u ? y0 + kSquare - 1u : c.height - 1u;
    const double wu = (double)(c.width - 1u), hv = (double)(c.height - 1u);
    const double u_lo = (double)x0 / wu, u_hi = (double)(x1 + 1u) / wu, v_lo = (double)(c.height - 1u - y1) / hv, v_hi = (double)(c.height - y0) / hv;
    const double uc = 0.5 * (u_lo + u_hi), vc = 0.5 * (v_lo + v_hi), du = 0.5 * (u_hi - u_lo), dv = 0.5 * (v_hi - v_lo);
    double D[3], mag = fabs(c.lens_radius);
    for (int a = 0; a < 3; ++a) {
        D[a] = c.llc[a] + uc * c.hor[a] + vc * c.ver[a] - c.org[a];
        mag += fabs(c.llc[a]) + fabs(c.hor[a]) + fabs(c.ver[a]) + fabs(c.org[a]);
    }
    const double lh = sqrt(c.hor[0] * c.hor[0] + c.hor[1] * c.hor[1] + c.hor[2] * c.hor[2]);
    const double lv = sqrt(c.ver[0] * c.ver[0] + c.ver[1] * c.ver[1] + c.ver[2] * c.ver[2]);
    // The device makes the ray in f32: origin and direction each carry at most 16 * 2^-24 * mag of rounding (five sums of terms below mag,
    // u and v good to 2 ulp, a factor sqrt 3 from components to length). eps = twice that is added to R and to rho: slack(u) then grows
    // by eps (|1 - u| + u) >= eps / 2 (1 + u), the offset of the f32 ray from the exact one at parameter u.
    const double eps = 32.0 * 5.9604644775390625e-8 * mag;
    k.L = sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]);
    k.R = fabs(c.lens_radius) + eps;
    k.rho = du * lh + dv * lv + eps;          // >= the half diagonal, whatever the angle between horizontal and vertical
    if (!(k.L - k.R - k.rho > 1e-9 * mag)) return k;       // (also NaN)
    for (int a = 0; a < 3; ++a) { k.o[a] = c.org[a]; k.e[a] = D[a] / k.L; }
    k.ok = 1u;
    return k;
}

// Can a ray of the square meet the sphere (centre, radius) at t > 0? Conservative: "no" is proven, "yes" is not.
// If the ray is inside the sphere at parameter u > 0, then (1) the axis point X(u) is within r + slack(u) of the centre, and (2) projected
// on the axis, u L - |1 - u| R - u rho <= m + r with m = (centre - O) . e, so u <= u_hi = max(1, (m + r - R) / (L - R - rho)). slack is
// convex, so on [0, u_hi] it is at most S = max(slack(0), slack(u_hi)) = max(R, (u_hi - 1) R + u_hi rho). Hence the centre lies within
// r + S of the axis RAY {X(u), u >= 0}; a sphere whose centre does not is dropped. (A sphere that contains the lens centre passes: its
// distance to X(0) is below r.) The comparison is made on squares, with a relative margin for its own rounding.
RT_CL_HD inline bool may_meet(const Cone& k, double cx, double cy, double cz, double radius) {
    if (k.ok == 0u) return true;
    const double r = fabs(radius);
    const double px = cx - k.o[0], py = cy - k.o[1], pz = cz - k.o[2];
    const double m = px * k.e[0] + py * k.e[1] + pz * k.e[2];
    const double far = (m + r - k.R) / (k.L - k.R - k.rho);
    const double u_hi = far > 1.0 ? far : 1.0;
    const double s_far = (u_hi - 1.0) * k.R + u_hi * k.rho, S = s_far > k.R ? s_far : k.R;
    const double mm = m > 0.0 ? m : 0.0;                           // the nearest point of the axis ray is X(mm / L)
    const double qx = px - mm * k.e[0], qy = py - mm * k.e[1], qz = pz - mm * k.e[2];
    const double dist2 = qx * qx + qy * qy + qz * qz, reach = r + S;
    return !(dist2 > reach * reach * (1.0 + 1e-9));                // (NaN: kept)
}

// squares of a frame
RT_CL_HD inline uint32_t squares_x(uint32_t width) { return (width + kSquare - 1u) / kSquare; }
RT_CL_HD inline uint32_t squares_y(uint32_t height) { return (height + kSquare - 1u) / kSquare; }

// The list of square (sx, sy): `order` names the candidates (sphere indices) in the order the threaded record array reaches their leaves,
// so the list comes out sorted that way. Writes kListWords words.
RT_CL_HD inline void build_list(const Camera& c, uint32_t sx, uint32_t sy, const float* spheres /* x y z r */, const uint32_t* order, uint32_t n_order, uint32_t* list) {
    const Cone k = square_cone(c, sx, sy);
    uint32_t n = 0u;
    for (uint32_t i = 0; i < n_order; ++i) {
        const uint32_t s = order[i];
        if (!may_meet(k, (double)spheres[4u * s], (double)spheres[4u * s + 1u], (double)spheres[4u * s + 2u], (double)spheres[4u * s + 3u])) continue;
        if (n < kListMax) list[1u + n] = s;
        ++n;
    }
    for (uint32_t j = n < kListMax ? n : kListMax; j < kListMax; ++j) list[1u + j] = 0u;
    list[0] = n <= kListMax ? n : kWalk;
}

}  // namespace rtcl
