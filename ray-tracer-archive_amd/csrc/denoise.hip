// denoise.hip — non-local means over the sample variance (include/rt_hip.h, "denoising"): the kernels and their two entry points.
//   k_nlm_prepare : rgb_sum, sq_sum, sample counts -> per pixel the mean u and the variance of the mean v (f64, rounded to f32), three
//                   float2 planes (u0,u1) (u2,v0) (v1,v2); an invalid pixel carries v0 = -1 (a variance is never negative)
//   k_nlm<F>      : one 32 x 32 output tile per workgroup. The planes of the tile plus an (r + f) halo are staged in LDS once; then, per
//                   window offset: the pointwise term on the tile plus an f halo, its patch sum as a separable box sum through LDS, the
//                   weight, and the sums of w and w (u[q] - u[p]) in registers. No atomics; every pixel's sums are folded in one fixed
//                   order (window rows, then columns; patch taps ascending), so the result does not depend on where tiles fall.
//   k_nlm_guide_prepare / k_nlm_guided<F> : the guided filter (rt_hip.h, "denoising, guided"): per pixel one 16-byte record of 7 binary16
//                   guide components; k_nlm's loop with the records of the tile plus an r halo staged beside the planes and
//                   g(p,q) added to the patch distance in step (C). k_nlm and nlm_window are pinned (text and ISA), so the guided loop
//                   is a second function beside them, not a flag in them.
//   k_nlm_guide_moments_prepare / k_nlm_guided_moments<F> : the guided filter with feature variances (rt_hip.h, "denoising, guided with
//                   feature variances"): beside the 16-byte record an 8-byte one of three binary16 standard errors, staged as a second
//                   LDS array; g(p,q) per group variance-cancelled and variance-normalised. A third loop beside the two pinned ones.
// The entry points live here, not in rt_api.cpp: nothing the render path is built from changes with this file.
#include <hip/hip_runtime.h>
#include <math.h>

#include <cmath>

#include "rt_internal.hpp"

namespace rtk {

namespace {

constexpr int kTile = 32;              // output tile edge; kTile * kTile = kThreads: one output pixel per thread
constexpr int kThreads = 1024;
constexpr int kMaxWindow = 16, kMaxPatch = 4;   // RT_DENOISE_MAX_WINDOW_RADIUS / RT_DENOISE_MAX_PATCH_RADIUS (static_assert below)

struct NlmArgs {
    const float2* planes;   // 3 planes of width * height float2
    float* out;             // mean radiance, 3 floats per pixel
    uint32_t width, height;
    int r;                  // window radius
    float k2, alpha, eps;
};

__global__ void __launch_bounds__(256) k_nlm_prepare(const float* __restrict__ rgb, const float* __restrict__ sq, const uint32_t* __restrict__ counts, uint32_t samples,
                                                     uint32_t m, uint32_t n_pixels, float2* __restrict__ planes) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const uint32_t n = counts ? counts[p] : samples;
    const uint32_t items = (uint32_t)(((uint64_t)n + m - 1u) / m);
    const double k = (double)items, nn = (double)n, mm = (double)m * (double)m;
    float u[3], v[3];
    bool valid = n > 0u && items >= 2u;
    for (int c = 0; c < 3; ++c) {
        const double S = (double)rgb[(uint64_t)p * 3u + c], Q = (double)sq[(uint64_t)p * 3u + c];
        if (!isfinite(S) || !isfinite(Q)) valid = false;
        u[c] = n > 0u ? (float)(S / nn) : 0.f;
        double d = Q - S * S / k;
        d = d > 0.0 ? d : 0.0;
        v[c] = (float)(d / (k * (k - 1.0)) / mm);
    }
    if (!valid) { v[0] = -1.f; v[1] = 0.f; v[2] = 0.f; }
    planes[p] = make_float2(u[0], u[1]);
    planes[(uint64_t)n_pixels + p] = make_float2(u[2], v[0]);
    planes[2ull * n_pixels + p] = make_float2(v[1], v[2]);
}

// one channel's term of the patch distance (rt_hip.h); ua, va belong to p + o, uq, vq to q + o
__device__ inline float nlm_term(float ua, float va, float uq, float vq, float k2, float alpha, float eps) {
    const float du = ua - uq;
    const float num = fmaf(du, du, -(alpha * (va + fminf(va, vq))));
    const float den = fmaf(k2, va + vq, eps);
    return num * __builtin_amdgcn_rcpf(den);
}

// The window loop. MASKED: some pixel of the staged region is invalid or outside the image, so the number of patch taps that take part
// is box-summed beside the terms; otherwise it is the constant 3 (2F + 1)^2. Both forms divide by the count the same way.
template <int F, bool MASKED>
__device__ inline void nlm_window(const NlmArgs& a, const float2* P0, const float2* P1, const float2* P2, float* bT, float* bH, float* bTM, float* bHM, int EW,
                                  bool p_valid, int ep, float up0, float up1, float up2, float& sw, float& s0, float& s1, float& s2) {
    constexpr int AW = kTile + 2 * F, AH = kTile + 2 * F, TAPS = 2 * F + 1;
    const int tid = (int)threadIdx.x, r = a.r;
    const int px = tid & (kTile - 1), py = tid / kTile;
    // the points p + o this thread owns (at most two: AW * AH <= 2 * kThreads), their planes in registers for the whole loop
    int ae[2]; bool a_on[2], a_valid[2]; float ua[2][3], va[2][3];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = tid + s * kThreads;
        a_on[s] = i < AW * AH;
        const int ay = a_on[s] ? i / AW : 0, ax = a_on[s] ? i - ay * AW : 0;
        ae[s] = (ay + r) * EW + ax + r;
        const float2 q0 = P0[ae[s]], q1 = P1[ae[s]], q2 = P2[ae[s]];
        ua[s][0] = q0.x; ua[s][1] = q0.y; ua[s][2] = q1.x; va[s][0] = q1.y; va[s][1] = q2.x; va[s][2] = q2.y;
        a_valid[s] = a_on[s] && q1.y >= 0.f;
    }
    const float inv_all = __builtin_amdgcn_rcpf((float)(3 * TAPS * TAPS));
    for (int dy = -r; dy <= r; ++dy) {
        for (int dx = -r; dx <= r; ++dx) {
            const int off = dy * EW + dx;
            // the pointwise term on the tile plus its F halo
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (!a_on[s]) continue;
                const int e = ae[s] + off;
                const float2 q0 = P0[e], q1 = P1[e], q2 = P2[e];
                const bool part = a_valid[s] && q1.y >= 0.f;
                const float t = nlm_term(ua[s][0], va[s][0], q0.x, q1.y, a.k2, a.alpha, a.eps) + nlm_term(ua[s][1], va[s][1], q0.y, q2.x, a.k2, a.alpha, a.eps) +
                                nlm_term(ua[s][2], va[s][2], q1.x, q2.y, a.k2, a.alpha, a.eps);
                bT[tid + s * kThreads] = part ? t : 0.f;
                if (MASKED) bTM[tid + s * kThreads] = part ? 1.f : 0.f;
            }
            __syncthreads();
            // box sum along x: AH rows of kTile sums
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int j = tid + s * kThreads;
                if (j >= AH * kTile) continue;
                const int row = j / kTile, x = j & (kTile - 1);
                const float* src = bT + row * AW + x;
                float h = src[0];
#pragma unroll
                for (int t = 1; t < TAPS; ++t) h += src[t];
                bH[j] = h;
                if (MASKED) {
                    const float* srm = bTM + row * AW + x;
                    float hm = srm[0];
#pragma unroll
                    for (int t = 1; t < TAPS; ++t) hm += srm[t];
                    bHM[j] = hm;
                }
            }
            __syncthreads();
            // box sum along y, the weight, the sums. (The next offset's terms overwrite bT only: its last readers passed the barrier above;
            // bH is rewritten behind the next offset's first barrier, which this read precedes.)
            const float* col = bH + py * kTile + px;
            float D = col[0];
#pragma unroll
            for (int t = 1; t < TAPS; ++t) D += col[t * kTile];
            float inv = inv_all;
            if (MASKED) {
                const float* cm = bHM + py * kTile + px;
                float cnt = cm[0];
#pragma unroll
                for (int t = 1; t < TAPS; ++t) cnt += cm[t * kTile];
                inv = __builtin_amdgcn_rcpf(3.f * fmaxf(cnt, 1.f));
            }
            const float2 q0 = P0[ep + off], q1 = P1[ep + off];
            if (p_valid && q1.y >= 0.f) {
                const float d = D * inv;
                const float w = __expf(-fmaxf(d, 0.f));
                sw += w;
                s0 = fmaf(w, q0.x - up0, s0);
                s1 = fmaf(w, q0.y - up1, s1);
                s2 = fmaf(w, q1.x - up2, s2);
            }
        }
    }
}

template <int F>
__global__ void __launch_bounds__(kThreads) k_nlm(NlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int AW = kTile + 2 * F, AH = kTile + 2 * F;
    const int halo = a.r + F, EW = kTile + 2 * halo, EH = EW, tid = (int)threadIdx.x;
    float2* P0 = (float2*)smem; float2* P1 = P0 + EW * EH; float2* P2 = P1 + EW * EH;
    float* bT = (float*)(P2 + EW * EH); float* bH = bT + AW * AH; float* bTM = bH + AH * kTile; float* bHM = bTM + AW * AH;
    const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile, W = (int)a.width, H = (int)a.height;
    const uint64_t n_px = (uint64_t)a.width * a.height;
    int any_invalid = 0;
    for (int i = tid; i < EW * EH; i += kThreads) {
        const int ey = i / EW, ex = i - ey * EW, gx = x0 - halo + ex, gy = y0 - halo + ey;
        float2 p0 = make_float2(0.f, 0.f), p1 = make_float2(0.f, -1.f), p2 = make_float2(0.f, 0.f);
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const uint64_t g = (uint64_t)gy * a.width + (uint32_t)gx;
            p0 = a.planes[g]; p1 = a.planes[n_px + g]; p2 = a.planes[2ull * n_px + g];
        }
        P0[i] = p0; P1[i] = p1; P2[i] = p2;
        any_invalid |= p1.y < 0.f ? 1 : 0;
    }
    const int masked = __syncthreads_or(any_invalid);
    const int px = tid & (kTile - 1), py = tid / kTile, ep = (py + halo) * EW + px + halo;
    const float2 c0 = P0[ep], c1 = P1[ep];
    const bool p_valid = c1.y >= 0.f;
    float sw = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (masked) nlm_window<F, true>(a, P0, P1, P2, bT, bH, bTM, bHM, EW, p_valid, ep, c0.x, c0.y, c1.x, sw, s0, s1, s2);
    else nlm_window<F, false>(a, P0, P1, P2, bT, bH, bTM, bHM, EW, p_valid, ep, c0.x, c0.y, c1.x, sw, s0, s1, s2);
    const int gx = x0 + px, gy = y0 + py;
    if (gx >= W || gy >= H) return;
    float o0 = c0.x, o1 = c0.y, o2 = c1.x;            // an invalid pixel is copied through
    if (p_valid) { o0 += s0 / sw; o1 += s1 / sw; o2 += s2 / sw; }   // sw >= 1: the pixel's own weight
    float* o = a.out + ((uint64_t)gy * a.width + (uint32_t)gx) * 3u;
    o[0] = o0; o[1] = o1; o[2] = o2;
}

size_t nlm_lds_bytes(int r, int f) {
    const size_t e = (size_t)(kTile + 2 * (r + f)), aw = (size_t)(kTile + 2 * f);
    return e * e * 3u * sizeof(float2) + 2u * (aw * aw + aw * kTile) * sizeof(float);
}
static_assert((kTile + 2 * (kMaxWindow + kMaxPatch)) * (kTile + 2 * (kMaxWindow + kMaxPatch)) * 24 +
                      2 * ((kTile + 2 * kMaxPatch) * (kTile + 2 * kMaxPatch) + (kTile + 2 * kMaxPatch) * kTile) * 4 <= 160 * 1024,
              "the staged tile plus halo and the box-sum buffers must fit the 160 KiB LDS at the caps");
static_assert((kTile + 2 * kMaxPatch) * (kTile + 2 * kMaxPatch) <= 2 * kThreads, "two term points per thread");
static_assert(kMaxWindow == RT_DENOISE_MAX_WINDOW_RADIUS && kMaxPatch == RT_DENOISE_MAX_PATCH_RADIUS, "caps as the header states them");

template <int F>
hipError_t launch_nlm_f(const NlmArgs& a, hipStream_t stream) {
    const size_t lds = nlm_lds_bytes(a.r, F);
    hipError_t e = hipFuncSetAttribute((const void*)k_nlm<F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_nlm<F>, dim3((a.width + kTile - 1) / kTile, (a.height + kTile - 1) / kTile), dim3(kThreads), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_nlm(const NlmArgs& a, int f, hipStream_t stream) {
    switch (f) {
        case 1: return launch_nlm_f<1>(a, stream);
        case 2: return launch_nlm_f<2>(a, stream);
        case 3: return launch_nlm_f<3>(a, stream);
        case 4: return launch_nlm_f<4>(a, stream);
    }
    return hipErrorInvalidValue;
}

struct NlmOptions { int r, f; uint32_t m; double strength, alpha, eps; };

// options with the defaults filled in; RT_ERR_INVALID with the reason otherwise
int nlm_options(RtCtx* ctx, uint32_t width, uint32_t height, const RtDenoiseOptions* o, NlmOptions& out) {
    using rti::set_err;
    out = NlmOptions{10, 3, 1u, 0.45, 1.0, 1e-10};
    if (width == 0u || height == 0u || (uint64_t)width * height * 3u > 0xFFFFFFFFull) return set_err(ctx, RT_ERR_INVALID, "denoise: bad image size (width, height >= 1, width * height * 3 < 2^32)");
    if (!o) return RT_OK;
    if (o->struct_bytes < sizeof(RtDenoiseOptions) || o->struct_bytes > 4096u) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseOptions.struct_bytes is not set (sizeof(RtDenoiseOptions))");
    if (o->window_radius > (uint32_t)kMaxWindow) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseOptions.window_radius is above RT_DENOISE_MAX_WINDOW_RADIUS (16)");
    if (o->patch_radius > (uint32_t)kMaxPatch) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseOptions.patch_radius is above RT_DENOISE_MAX_PATCH_RADIUS (4)");
    if (!(std::isfinite(o->strength) && o->strength >= 0.0) || std::signbit(o->strength)) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseOptions.strength must be finite and > 0 (0 = the default)");
    if (!(std::isfinite(o->alpha) && o->alpha >= 0.0) || std::signbit(o->alpha)) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseOptions.alpha must be finite and >= 0 (0 = the default)");
    if (!(std::isfinite(o->eps) && o->eps >= 0.0) || std::signbit(o->eps)) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseOptions.eps must be finite and > 0 (0 = the default)");
    if (o->window_radius) out.r = (int)o->window_radius;
    if (o->patch_radius) out.f = (int)o->patch_radius;
    if (o->samples_per_item) out.m = o->samples_per_item;
    if (o->strength != 0.0) out.strength = o->strength;
    if (o->alpha != 0.0) out.alpha = o->alpha;
    if (o->eps != 0.0) out.eps = o->eps;
    if (!((float)out.eps > 0.f) || !std::isfinite((float)(out.strength * out.strength))) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseOptions.eps / strength is outside the f32 range the filter computes in");
    return RT_OK;
}


// ---- guided: the weights joined with first-hit features (rt_hip.h, "denoising, guided") ------------------------------------------------------
constexpr int kMaxWindowGuided = 10;   // RT_DENOISE_GUIDED_MAX_WINDOW_RADIUS (static_assert below)

struct GuideArgs {
    const float* albedo; const float* normal; const float* depth; const uint32_t* hits;   // any may be null (depth needs hits)
    uint32_t n_f;
    double sigma_albedo, sigma_normal, sigma_depth;
};

// f64 -> f32 -> binary16 (v_cvt_f16_f32, round to nearest even), clamped to +-65504. The clamp is made on the f32 value: every f32 in
// (65504, 65520) rounds to 65504 and everything from 65520 on to inf, which the clamp brings back to 65504, so the two orders agree.
__device__ inline uint32_t guide_half(double x) {
    const float f = fminf(fmaxf((float)x, -65504.f), 65504.f);
    return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)f);
}

// One thread per pixel, f64: the pixel's guide record (A0 A1 A2 N0 N1 N2 Z 0 as binary16). A pixel the guide makes invalid is marked in
// the colour planes k_nlm_prepare left (v0 = -1), so staging the tile sees one kind of invalid pixel; its record is 0.
__global__ void __launch_bounds__(256) k_nlm_guide_prepare(GuideArgs g, uint32_t n_pixels, uint4* __restrict__ rec, float2* __restrict__ planes) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const double nf = (double)g.n_f;
    double F[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool valid = true;
    for (int c = 0; c < 3; ++c) {
        if (g.albedo) { const double s = (double)g.albedo[(uint64_t)p * 3u + c]; valid = valid && isfinite(s); F[c] = s / nf / g.sigma_albedo; }
        if (g.normal) { const double s = (double)g.normal[(uint64_t)p * 3u + c]; valid = valid && isfinite(s); F[3 + c] = s / nf / g.sigma_normal; }
    }
    const uint32_t h = g.hits ? g.hits[p] : 0u;
    if (h > g.n_f) valid = false;
    if (g.depth) {
        const double s = (double)g.depth[p];
        valid = valid && isfinite(s);
        if (h > 0u) F[6] = log(fmax(s / (double)h, 1e-30)) / g.sigma_depth;
    }
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (valid) {
        r.x = guide_half(F[0]) | (guide_half(F[1]) << 16); r.y = guide_half(F[2]) | (guide_half(F[3]) << 16);
        r.z = guide_half(F[4]) | (guide_half(F[5]) << 16); r.w = guide_half(F[6]);
    } else {
        planes[(uint64_t)n_pixels + p].y = -1.f;
        planes[2ull * n_pixels + p] = make_float2(0.f, 0.f);
    }
    rec[p] = r;
}

__device__ inline float half_lo(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu)); }
__device__ inline float half_hi(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
__device__ inline void guide_unpack(const uint4& r, float f[7]) {
    f[0] = half_lo(r.x); f[1] = half_hi(r.x); f[2] = half_lo(r.y); f[3] = half_hi(r.y); f[4] = half_lo(r.z); f[5] = half_hi(r.z); f[6] = half_lo(r.w);
}

// nlm_window with the guide: steps (A) and (B) are nlm_window's; step (C) reads the partner's record (one ds_read_b128; a wave's 64 records
// are two rows of 32 contiguous 16-byte slots: no bank conflict) and adds g(p,q) to max(d, 0). G: (kTile + 2 r)^2 records, this thread's at gp.
template <int F, bool MASKED>
__device__ inline void nlm_guided_window(const NlmArgs& a, const float2* P0, const float2* P1, const float2* P2, const uint4* G, float* bT, float* bH, float* bTM,
                                         float* bHM, int EW, int GW, bool p_valid, int ep, int gp, float up0, float up1, float up2, float& sw, float& s0,
                                         float& s1, float& s2) {
    constexpr int AW = kTile + 2 * F, AH = kTile + 2 * F, TAPS = 2 * F + 1;
    const int tid = (int)threadIdx.x, r = a.r;
    const int px = tid & (kTile - 1), py = tid / kTile;
    int ae[2]; bool a_on[2], a_valid[2]; float ua[2][3], va[2][3];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = tid + s * kThreads;
        a_on[s] = i < AW * AH;
        const int ay = a_on[s] ? i / AW : 0, ax = a_on[s] ? i - ay * AW : 0;
        ae[s] = (ay + r) * EW + ax + r;
        const float2 q0 = P0[ae[s]], q1 = P1[ae[s]], q2 = P2[ae[s]];
        ua[s][0] = q0.x; ua[s][1] = q0.y; ua[s][2] = q1.x; va[s][0] = q1.y; va[s][1] = q2.x; va[s][2] = q2.y;
        a_valid[s] = a_on[s] && q1.y >= 0.f;
    }
    float fp[7];
    guide_unpack(G[gp], fp);
    const float inv_all = __builtin_amdgcn_rcpf((float)(3 * TAPS * TAPS));
    for (int dy = -r; dy <= r; ++dy) {
        for (int dx = -r; dx <= r; ++dx) {
            const int off = dy * EW + dx;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (!a_on[s]) continue;
                const int e = ae[s] + off;
                const float2 q0 = P0[e], q1 = P1[e], q2 = P2[e];
                const bool part = a_valid[s] && q1.y >= 0.f;
                const float t = nlm_term(ua[s][0], va[s][0], q0.x, q1.y, a.k2, a.alpha, a.eps) + nlm_term(ua[s][1], va[s][1], q0.y, q2.x, a.k2, a.alpha, a.eps) +
                                nlm_term(ua[s][2], va[s][2], q1.x, q2.y, a.k2, a.alpha, a.eps);
                bT[tid + s * kThreads] = part ? t : 0.f;
                if (MASKED) bTM[tid + s * kThreads] = part ? 1.f : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int j = tid + s * kThreads;
                if (j >= AH * kTile) continue;
                const int row = j / kTile, x = j & (kTile - 1);
                const float* src = bT + row * AW + x;
                float h = src[0];
#pragma unroll
                for (int t = 1; t < TAPS; ++t) h += src[t];
                bH[j] = h;
                if (MASKED) {
                    const float* srm = bTM + row * AW + x;
                    float hm = srm[0];
#pragma unroll
                    for (int t = 1; t < TAPS; ++t) hm += srm[t];
                    bHM[j] = hm;
                }
            }
            __syncthreads();
            const float* col = bH + py * kTile + px;
            float D = col[0];
#pragma unroll
            for (int t = 1; t < TAPS; ++t) D += col[t * kTile];
            float inv = inv_all;
            if (MASKED) {
                const float* cm = bHM + py * kTile + px;
                float cnt = cm[0];
#pragma unroll
                for (int t = 1; t < TAPS; ++t) cnt += cm[t * kTile];
                inv = __builtin_amdgcn_rcpf(3.f * fmaxf(cnt, 1.f));
            }
            const float2 q0 = P0[ep + off], q1 = P1[ep + off];
            const uint4 gq = G[gp + dy * GW + dx];
            if (p_valid && q1.y >= 0.f) {
                float fq[7];
                guide_unpack(gq, fq);
                float g = 0.f;
#pragma unroll
                for (int c = 0; c < 7; ++c) { const float d = fp[c] - fq[c]; g = fmaf(d, d, g); }
                const float w = __expf(-(fmaxf(D * inv, 0.f) + g));
                sw += w;
                s0 = fmaf(w, q0.x - up0, s0);
                s1 = fmaf(w, q0.y - up1, s1);
                s2 = fmaf(w, q1.x - up2, s2);
            }
        }
    }
}

template <int F>
__global__ void __launch_bounds__(kThreads) k_nlm_guided(NlmArgs a, const uint4* __restrict__ guide) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int AW = kTile + 2 * F, AH = kTile + 2 * F;
    const int halo = a.r + F, EW = kTile + 2 * halo, EH = EW, GW = kTile + 2 * a.r, tid = (int)threadIdx.x;
    float2* P0 = (float2*)smem; float2* P1 = P0 + EW * EH; float2* P2 = P1 + EW * EH;
    uint4* G = (uint4*)(P2 + EW * EH);            // EW is even: 24 EW^2 is a multiple of 16
    float* bT = (float*)(G + GW * GW); float* bH = bT + AW * AH; float* bTM = bH + AH * kTile; float* bHM = bTM + AW * AH;
    const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile, W = (int)a.width, H = (int)a.height;
    const uint64_t n_px = (uint64_t)a.width * a.height;
    int any_invalid = 0;
    for (int i = tid; i < EW * EH; i += kThreads) {
        const int ey = i / EW, ex = i - ey * EW, gx = x0 - halo + ex, gy = y0 - halo + ey;
        float2 p0 = make_float2(0.f, 0.f), p1 = make_float2(0.f, -1.f), p2 = make_float2(0.f, 0.f);
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const uint64_t g = (uint64_t)gy * a.width + (uint32_t)gx;
            p0 = a.planes[g]; p1 = a.planes[n_px + g]; p2 = a.planes[2ull * n_px + g];
        }
        P0[i] = p0; P1[i] = p1; P2[i] = p2;
        any_invalid |= p1.y < 0.f ? 1 : 0;
    }
    for (int i = tid; i < GW * GW; i += kThreads) {
        const int ey = i / GW, ex = i - ey * GW, gx = x0 - a.r + ex, gy = y0 - a.r + ey;
        uint4 rec = make_uint4(0u, 0u, 0u, 0u);
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) rec = guide[(uint64_t)gy * a.width + (uint32_t)gx];
        G[i] = rec;
    }
    const int masked = __syncthreads_or(any_invalid);
    const int px = tid & (kTile - 1), py = tid / kTile, ep = (py + halo) * EW + px + halo, gp = (py + a.r) * GW + px + a.r;
    const float2 c0 = P0[ep], c1 = P1[ep];
    const bool p_valid = c1.y >= 0.f;
    float sw = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (masked) nlm_guided_window<F, true>(a, P0, P1, P2, G, bT, bH, bTM, bHM, EW, GW, p_valid, ep, gp, c0.x, c0.y, c1.x, sw, s0, s1, s2);
    else nlm_guided_window<F, false>(a, P0, P1, P2, G, bT, bH, bTM, bHM, EW, GW, p_valid, ep, gp, c0.x, c0.y, c1.x, sw, s0, s1, s2);
    const int gx = x0 + px, gy = y0 + py;
    if (gx >= W || gy >= H) return;
    float o0 = c0.x, o1 = c0.y, o2 = c1.x;            // an invalid pixel is copied through
    if (p_valid) { o0 += s0 / sw; o1 += s1 / sw; o2 += s2 / sw; }   // sw >= 1: the pixel's own weight
    float* o = a.out + ((uint64_t)gy * a.width + (uint32_t)gx) * 3u;
    o[0] = o0; o[1] = o1; o[2] = o2;
}

size_t nlm_guided_lds_bytes(int r, int f) {
    const size_t gw = (size_t)(kTile + 2 * r);
    return nlm_lds_bytes(r, f) + gw * gw * sizeof(uint4);
}
// at the caps (r 10, f 4): 60^2 x 24 B of colour planes + 52^2 x 16 B of guide records + 23,040 B of box-sum buffers = 152,704 B
static_assert((kTile + 2 * (kMaxWindowGuided + kMaxPatch)) * (kTile + 2 * (kMaxWindowGuided + kMaxPatch)) * 24 +
                      (kTile + 2 * kMaxWindowGuided) * (kTile + 2 * kMaxWindowGuided) * 16 +
                      2 * ((kTile + 2 * kMaxPatch) * (kTile + 2 * kMaxPatch) + (kTile + 2 * kMaxPatch) * kTile) * 4 == 152704 &&
                      152704 <= 160 * 1024,
              "colour planes, guide records and box-sum buffers must fit the 160 KiB LDS at the guided caps");
static_assert(kMaxWindowGuided == RT_DENOISE_GUIDED_MAX_WINDOW_RADIUS && sizeof(uint4) == 16, "cap as the header states it; 16-byte records");

template <int F>
hipError_t launch_nlm_guided_f(const NlmArgs& a, const uint4* guide, hipStream_t stream) {
    const size_t lds = nlm_guided_lds_bytes(a.r, F);
    hipError_t e = hipFuncSetAttribute((const void*)k_nlm_guided<F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_nlm_guided<F>, dim3((a.width + kTile - 1) / kTile, (a.height + kTile - 1) / kTile), dim3(kThreads), lds, stream, a, guide);
    return hipGetLastError();
}

hipError_t launch_nlm_guided(const NlmArgs& a, const uint4* guide, int f, hipStream_t stream) {
    switch (f) {
        case 1: return launch_nlm_guided_f<1>(a, guide, stream);
        case 2: return launch_nlm_guided_f<2>(a, guide, stream);
        case 3: return launch_nlm_guided_f<3>(a, guide, stream);
        case 4: return launch_nlm_guided_f<4>(a, guide, stream);
    }
    return hipErrorInvalidValue;
}

// a sigma with its default filled in; false for a value the contract refuses
bool guide_sigma(double given, double dflt, double& out) {
    if (!(std::isfinite(given) && given >= 0.0) || std::signbit(given)) return false;
    out = given != 0.0 ? given : dflt;
    const float inv = 1.f / (float)out;
    return std::isfinite(inv) && inv > 0.f;
}

// options (window cap of the guided path included) and the guide with its defaults filled in; RT_ERR_INVALID with the reason otherwise
int nlm_guided_options(RtCtx* ctx, uint32_t width, uint32_t height, const RtDenoiseOptions* o, const RtDenoiseGuide* g, NlmOptions& out, GuideArgs& ga) {
    using rti::set_err;
    const int v = nlm_options(ctx, width, height, o, out); if (v != RT_OK) return v;
    if (out.r > kMaxWindowGuided) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseOptions.window_radius is above RT_DENOISE_GUIDED_MAX_WINDOW_RADIUS (10): the guide records of a larger halo do not fit the LDS beside the colour planes");
    if (!g) return set_err(ctx, RT_ERR_INVALID, "denoise: guide is null (the filter without a guide is rt_denoise_device)");
    if (g->struct_bytes < sizeof(RtDenoiseGuide) || g->struct_bytes > 4096u) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuide.struct_bytes is not set (sizeof(RtDenoiseGuide))");
    if (g->feature_samples == 0u) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuide.feature_samples must be >= 1");
    if (!g->albedo_sum && !g->normal_sum && !g->depth_sum) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuide: albedo_sum, normal_sum and depth_sum are all null (the filter without a guide is rt_denoise_device)");
    if (g->depth_sum && !g->hits) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuide.depth_sum needs hits (the depth is a mean over the samples that hit)");
    ga = GuideArgs{(const float*)g->albedo_sum, (const float*)g->normal_sum, (const float*)g->depth_sum, (const uint32_t*)g->hits, g->feature_samples, 0.0, 0.0, 0.0};
    if (!guide_sigma(g->sigma_albedo, 0.2, ga.sigma_albedo)) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuide.sigma_albedo must be finite and > 0 with a finite f32 reciprocal (0 = the default)");
    if (!guide_sigma(g->sigma_normal, 0.5, ga.sigma_normal)) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuide.sigma_normal must be finite and > 0 with a finite f32 reciprocal (0 = the default)");
    if (!guide_sigma(g->sigma_depth, 0.2, ga.sigma_depth)) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuide.sigma_depth must be finite and > 0 with a finite f32 reciprocal (0 = the default)");
    return RT_OK;
}


// ---- guided, with feature variances (rt_hip.h, "denoising, guided with feature variances") -------------------------------------------------
constexpr int kMaxWindowMoments = 8;   // RT_DENOISE_GUIDED_MOMENTS_MAX_WINDOW_RADIUS (static_assert below)

struct GuideMomArgs {
    GuideArgs g;                                                            // the sum planes, n_f >= 2, the sigmas
    const float* albedo_sq; const float* normal_sq; const float* depth_sq;  // any may be null: that group's variance is 0
    float kappa;
};

// the variance of the mean over all n_f samples, from a sum and a sum of squares
__device__ inline double moment_var(double S, double Q, double nf) {
    const double d = Q - S * S / nf;
    return (d > 0.0 ? d : 0.0) / (nf * (nf - 1.0));
}

// One thread per pixel, f64: k_nlm_guide_prepare's 16-byte record (A0 A1 A2 N0 N1 N2 Z 0) and beside it an 8-byte one (sA sN sZ 0), the
// standard errors of the three groups over their sigmas — roots, because a variance of 1e-8 is below binary16's range. An invalid pixel
// is marked in the colour planes as k_nlm_guide_prepare marks it; both its records are 0.
__global__ void __launch_bounds__(256) k_nlm_guide_moments_prepare(GuideMomArgs m, uint32_t n_pixels, uint4* __restrict__ rec, uint2* __restrict__ rec2,
                                                                   float2* __restrict__ planes) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const GuideArgs& g = m.g;
    const double nf = (double)g.n_f;
    double F[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, VA = 0.0, VN = 0.0, VZ = 0.0;
    bool valid = true;
    for (int c = 0; c < 3; ++c) {
        double qa = 0.0, qn = 0.0;
        if (m.albedo_sq) { qa = (double)m.albedo_sq[(uint64_t)p * 3u + c]; valid = valid && isfinite(qa); }
        if (m.normal_sq) { qn = (double)m.normal_sq[(uint64_t)p * 3u + c]; valid = valid && isfinite(qn); }
        if (g.albedo) {
            const double s = (double)g.albedo[(uint64_t)p * 3u + c]; valid = valid && isfinite(s); F[c] = s / nf / g.sigma_albedo;
            if (m.albedo_sq) VA += moment_var(s, qa, nf);
        }
        if (g.normal) {
            const double s = (double)g.normal[(uint64_t)p * 3u + c]; valid = valid && isfinite(s); F[3 + c] = s / nf / g.sigma_normal;
            if (m.normal_sq) VN += moment_var(s, qn, nf);
        }
    }
    const uint32_t h = g.hits ? g.hits[p] : 0u;
    if (h > g.n_f) valid = false;
    double qz = 0.0;
    if (m.depth_sq) { qz = (double)m.depth_sq[p]; valid = valid && isfinite(qz); }
    if (g.depth) {
        const double s = (double)g.depth[p];
        valid = valid && isfinite(s);
        if (h > 0u) {
            const double mean = fmax(s / (double)h, 1e-30);                 // the mean depth ln is taken of
            F[6] = log(mean) / g.sigma_depth;
            if (m.depth_sq) { const double k = nf / (double)h; VZ = moment_var(s, qz, nf) * (k * k) / (mean * mean); }      // the delta method on the log
        }
    }
    uint4 r = make_uint4(0u, 0u, 0u, 0u); uint2 r2 = make_uint2(0u, 0u);
    if (valid) {
        r.x = guide_half(F[0]) | (guide_half(F[1]) << 16); r.y = guide_half(F[2]) | (guide_half(F[3]) << 16);
        r.z = guide_half(F[4]) | (guide_half(F[5]) << 16); r.w = guide_half(F[6]);
        r2.x = guide_half(sqrt(VA) / g.sigma_albedo) | (guide_half(sqrt(VN) / g.sigma_normal) << 16); r2.y = guide_half(sqrt(VZ) / g.sigma_depth);
    } else {
        planes[(uint64_t)n_pixels + p].y = -1.f;
        planes[2ull * n_pixels + p] = make_float2(0.f, 0.f);
    }
    rec[p] = r; rec2[p] = r2;
}

// one group's term of g(p,q): d2 = |F_p - F_q|^2 over the group, vp and vq the two variances (s^2, formed in f32)
__device__ inline float guide_moment_term(float d2, float vp, float vq, float kappa) {
    const float num = fmaxf(d2 - (vp + fminf(vp, vq)), 0.f);
    return num * __builtin_amdgcn_rcpf(fmaf(kappa, vp + vq, 1.f));
}

// nlm_guided_window with the variance form of g. Step (C) reads the partner's two records: one ds_read_b128 from G and one ds_read_b64
// from G2. A wave's 64 partners are two rows of 32 neighbours: in G2 two runs of 32 contiguous 8-byte slots, 256 B each — what one half
// wave of a ds_read_b64 fetches, one dword from each of the 64 banks: no conflict, as for the 16-byte array (four quarter waves of 256 B).
template <int F, bool MASKED>
__device__ inline void nlm_guided_moments_window(const NlmArgs& a, float kappa, const float2* P0, const float2* P1, const float2* P2, const uint4* G, const uint2* G2,
                                                 float* bT, float* bH, float* bTM, float* bHM, int EW, int GW, bool p_valid, int ep, int gp, float up0, float up1,
                                                 float up2, float& sw, float& s0, float& s1, float& s2) {
    constexpr int AW = kTile + 2 * F, AH = kTile + 2 * F, TAPS = 2 * F + 1;
    const int tid = (int)threadIdx.x, r = a.r;
    const int px = tid & (kTile - 1), py = tid / kTile;
    int ae[2]; bool a_on[2], a_valid[2]; float ua[2][3], va[2][3];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = tid + s * kThreads;
        a_on[s] = i < AW * AH;
        const int ay = a_on[s] ? i / AW : 0, ax = a_on[s] ? i - ay * AW : 0;
        ae[s] = (ay + r) * EW + ax + r;
        const float2 q0 = P0[ae[s]], q1 = P1[ae[s]], q2 = P2[ae[s]];
        ua[s][0] = q0.x; ua[s][1] = q0.y; ua[s][2] = q1.x; va[s][0] = q1.y; va[s][1] = q2.x; va[s][2] = q2.y;
        a_valid[s] = a_on[s] && q1.y >= 0.f;
    }
    float fp[7];
    guide_unpack(G[gp], fp);
    const uint2 mp = G2[gp];
    const float sAp = half_lo(mp.x), sNp = half_hi(mp.x), sZp = half_lo(mp.y);
    const float vAp = sAp * sAp, vNp = sNp * sNp, vZp = sZp * sZp;
    const float inv_all = __builtin_amdgcn_rcpf((float)(3 * TAPS * TAPS));
    for (int dy = -r; dy <= r; ++dy) {
        for (int dx = -r; dx <= r; ++dx) {
            const int off = dy * EW + dx;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (!a_on[s]) continue;
                const int e = ae[s] + off;
                const float2 q0 = P0[e], q1 = P1[e], q2 = P2[e];
                const bool part = a_valid[s] && q1.y >= 0.f;
                const float t = nlm_term(ua[s][0], va[s][0], q0.x, q1.y, a.k2, a.alpha, a.eps) + nlm_term(ua[s][1], va[s][1], q0.y, q2.x, a.k2, a.alpha, a.eps) +
                                nlm_term(ua[s][2], va[s][2], q1.x, q2.y, a.k2, a.alpha, a.eps);
                bT[tid + s * kThreads] = part ? t : 0.f;
                if (MASKED) bTM[tid + s * kThreads] = part ? 1.f : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int j = tid + s * kThreads;
                if (j >= AH * kTile) continue;
                const int row = j / kTile, x = j & (kTile - 1);
                const float* src = bT + row * AW + x;
                float h = src[0];
#pragma unroll
                for (int t = 1; t < TAPS; ++t) h += src[t];
                bH[j] = h;
                if (MASKED) {
                    const float* srm = bTM + row * AW + x;
                    float hm = srm[0];
#pragma unroll
                    for (int t = 1; t < TAPS; ++t) hm += srm[t];
                    bHM[j] = hm;
                }
            }
            __syncthreads();
            const float* col = bH + py * kTile + px;
            float D = col[0];
#pragma unroll
            for (int t = 1; t < TAPS; ++t) D += col[t * kTile];
            float inv = inv_all;
            if (MASKED) {
                const float* cm = bHM + py * kTile + px;
                float cnt = cm[0];
#pragma unroll
                for (int t = 1; t < TAPS; ++t) cnt += cm[t * kTile];
                inv = __builtin_amdgcn_rcpf(3.f * fmaxf(cnt, 1.f));
            }
            const float2 q0 = P0[ep + off], q1 = P1[ep + off];
            const int gq_at = gp + dy * GW + dx;
            const uint4 gq = G[gq_at];
            const uint2 mq = G2[gq_at];
            if (p_valid && q1.y >= 0.f) {
                float fq[7];
                guide_unpack(gq, fq);
                const float sAq = half_lo(mq.x), sNq = half_hi(mq.x), sZq = half_lo(mq.y);
                float dA = 0.f, dN = 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) { const float d = fp[c] - fq[c]; dA = fmaf(d, d, dA); const float e = fp[3 + c] - fq[3 + c]; dN = fmaf(e, e, dN); }
                const float dz = fp[6] - fq[6];
                const float g = guide_moment_term(dA, vAp, sAq * sAq, kappa) + guide_moment_term(dN, vNp, sNq * sNq, kappa) + guide_moment_term(dz * dz, vZp, sZq * sZq, kappa);
                const float w = __expf(-(fmaxf(D * inv, 0.f) + g));
                sw += w;
                s0 = fmaf(w, q0.x - up0, s0);
                s1 = fmaf(w, q0.y - up1, s1);
                s2 = fmaf(w, q1.x - up2, s2);
            }
        }
    }
}

template <int F>
__global__ void __launch_bounds__(kThreads) k_nlm_guided_moments(NlmArgs a, float kappa, const uint4* __restrict__ guide, const uint2* __restrict__ guide2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int AW = kTile + 2 * F, AH = kTile + 2 * F;
    const int halo = a.r + F, EW = kTile + 2 * halo, EH = EW, GW = kTile + 2 * a.r, tid = (int)threadIdx.x;
    float2* P0 = (float2*)smem; float2* P1 = P0 + EW * EH; float2* P2 = P1 + EW * EH;
    uint4* G = (uint4*)(P2 + EW * EH);            // EW is even: 24 EW^2 is a multiple of 16
    uint2* G2 = (uint2*)(G + GW * GW);            // two arrays, not one of 24-byte records: the partner read stays one b128 and one b64
    float* bT = (float*)(G2 + GW * GW); float* bH = bT + AW * AH; float* bTM = bH + AH * kTile; float* bHM = bTM + AW * AH;
    const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile, W = (int)a.width, H = (int)a.height;
    const uint64_t n_px = (uint64_t)a.width * a.height;
    int any_invalid = 0;
    for (int i = tid; i < EW * EH; i += kThreads) {
        const int ey = i / EW, ex = i - ey * EW, gx = x0 - halo + ex, gy = y0 - halo + ey;
        float2 p0 = make_float2(0.f, 0.f), p1 = make_float2(0.f, -1.f), p2 = make_float2(0.f, 0.f);
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const uint64_t g = (uint64_t)gy * a.width + (uint32_t)gx;
            p0 = a.planes[g]; p1 = a.planes[n_px + g]; p2 = a.planes[2ull * n_px + g];
        }
        P0[i] = p0; P1[i] = p1; P2[i] = p2;
        any_invalid |= p1.y < 0.f ? 1 : 0;
    }
    for (int i = tid; i < GW * GW; i += kThreads) {
        const int ey = i / GW, ex = i - ey * GW, gx = x0 - a.r + ex, gy = y0 - a.r + ey;
        uint4 rec = make_uint4(0u, 0u, 0u, 0u); uint2 rec2 = make_uint2(0u, 0u);
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) { const uint64_t g = (uint64_t)gy * a.width + (uint32_t)gx; rec = guide[g]; rec2 = guide2[g]; }
        G[i] = rec; G2[i] = rec2;
    }
    const int masked = __syncthreads_or(any_invalid);
    const int px = tid & (kTile - 1), py = tid / kTile, ep = (py + halo) * EW + px + halo, gp = (py + a.r) * GW + px + a.r;
    const float2 c0 = P0[ep], c1 = P1[ep];
    const bool p_valid = c1.y >= 0.f;
    float sw = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (masked) nlm_guided_moments_window<F, true>(a, kappa, P0, P1, P2, G, G2, bT, bH, bTM, bHM, EW, GW, p_valid, ep, gp, c0.x, c0.y, c1.x, sw, s0, s1, s2);
    else nlm_guided_moments_window<F, false>(a, kappa, P0, P1, P2, G, G2, bT, bH, bTM, bHM, EW, GW, p_valid, ep, gp, c0.x, c0.y, c1.x, sw, s0, s1, s2);
    const int gx = x0 + px, gy = y0 + py;
    if (gx >= W || gy >= H) return;
    float o0 = c0.x, o1 = c0.y, o2 = c1.x;            // an invalid pixel is copied through
    if (p_valid) { o0 += s0 / sw; o1 += s1 / sw; o2 += s2 / sw; }   // sw >= 1: the pixel's own weight
    float* o = a.out + ((uint64_t)gy * a.width + (uint32_t)gx) * 3u;
    o[0] = o0; o[1] = o1; o[2] = o2;
}

size_t nlm_guided_moments_lds_bytes(int r, int f) {
    const size_t gw = (size_t)(kTile + 2 * r);
    return nlm_lds_bytes(r, f) + gw * gw * (sizeof(uint4) + sizeof(uint2));
}
// at the caps (r 8, f 4): 56^2 x 24 B of colour planes + 48^2 x (16 + 8) B of guide records + 23,040 B of box-sum buffers = 153,600 B; the
// barrier with OR holds 256 B more. r 9 misses by 192 B, r 10 by far (60^2 x 24 + 52^2 x 24 + 23,040 = 174,336 B).
static_assert((kTile + 2 * (kMaxWindowMoments + kMaxPatch)) * (kTile + 2 * (kMaxWindowMoments + kMaxPatch)) * 24 +
                      (kTile + 2 * kMaxWindowMoments) * (kTile + 2 * kMaxWindowMoments) * 24 +
                      2 * ((kTile + 2 * kMaxPatch) * (kTile + 2 * kMaxPatch) + (kTile + 2 * kMaxPatch) * kTile) * 4 == 153600 &&
                      153600 + 256 <= 160 * 1024,
              "colour planes, both guide records and box-sum buffers must fit the 160 KiB LDS at the caps of the variance-guided path");
static_assert(kMaxWindowMoments == RT_DENOISE_GUIDED_MOMENTS_MAX_WINDOW_RADIUS && sizeof(uint2) == 8, "cap as the header states it; 8-byte records");

template <int F>
hipError_t launch_nlm_guided_moments_f(const NlmArgs& a, float kappa, const uint4* guide, const uint2* guide2, hipStream_t stream) {
    const size_t lds = nlm_guided_moments_lds_bytes(a.r, F);
    hipError_t e = hipFuncSetAttribute((const void*)k_nlm_guided_moments<F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_nlm_guided_moments<F>, dim3((a.width + kTile - 1) / kTile, (a.height + kTile - 1) / kTile), dim3(kThreads), lds, stream, a, kappa, guide, guide2);
    return hipGetLastError();
}

hipError_t launch_nlm_guided_moments(const NlmArgs& a, float kappa, const uint4* guide, const uint2* guide2, int f, hipStream_t stream) {
    switch (f) {
        case 1: return launch_nlm_guided_moments_f<1>(a, kappa, guide, guide2, stream);
        case 2: return launch_nlm_guided_moments_f<2>(a, kappa, guide, guide2, stream);
        case 3: return launch_nlm_guided_moments_f<3>(a, kappa, guide, guide2, stream);
        case 4: return launch_nlm_guided_moments_f<4>(a, kappa, guide, guide2, stream);
    }
    return hipErrorInvalidValue;
}

// options (window_radius 0 = 8 here, capped at 8) and the guide with its defaults filled in; RT_ERR_INVALID with the reason otherwise
int nlm_guided_moments_options(RtCtx* ctx, uint32_t width, uint32_t height, const RtDenoiseOptions* o, const RtDenoiseGuideMoments* g, NlmOptions& out, GuideMomArgs& ma) {
    using rti::set_err;
    const int v = nlm_options(ctx, width, height, o, out); if (v != RT_OK) return v;
    if (!o || o->window_radius == 0u) out.r = kMaxWindowMoments;
    if (out.r > kMaxWindowMoments) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseOptions.window_radius is above RT_DENOISE_GUIDED_MOMENTS_MAX_WINDOW_RADIUS (8): both guide records of a larger halo do not fit the LDS beside the colour planes");
    if (!g) return set_err(ctx, RT_ERR_INVALID, "denoise: guide is null (the filter without a guide is rt_denoise_device)");
    if (g->struct_bytes < sizeof(RtDenoiseGuideMoments) || g->struct_bytes > 4096u) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuideMoments.struct_bytes is not set (sizeof(RtDenoiseGuideMoments))");
    if (g->feature_samples < 2u) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuideMoments.feature_samples must be >= 2 (a variance needs two samples)");
    if (!g->albedo_sum && !g->normal_sum && !g->depth_sum) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuideMoments: albedo_sum, normal_sum and depth_sum are all null (the filter without a guide is rt_denoise_device)");
    if (g->depth_sum && !g->hits) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuideMoments.depth_sum needs hits (the depth is a mean over the samples that hit)");
    ma.g = GuideArgs{(const float*)g->albedo_sum, (const float*)g->normal_sum, (const float*)g->depth_sum, (const uint32_t*)g->hits, g->feature_samples, 0.0, 0.0, 0.0};
    ma.albedo_sq = (const float*)g->albedo_sq_sum; ma.normal_sq = (const float*)g->normal_sq_sum; ma.depth_sq = (const float*)g->depth_sq_sum;
    if (!guide_sigma(g->sigma_albedo, RT_DENOISE_MOMENTS_SIGMA_ALBEDO, ma.g.sigma_albedo)) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuideMoments.sigma_albedo must be finite and > 0 with a finite f32 reciprocal (0 = the default)");
    if (!guide_sigma(g->sigma_normal, RT_DENOISE_MOMENTS_SIGMA_NORMAL, ma.g.sigma_normal)) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuideMoments.sigma_normal must be finite and > 0 with a finite f32 reciprocal (0 = the default)");
    if (!guide_sigma(g->sigma_depth, RT_DENOISE_MOMENTS_SIGMA_DEPTH, ma.g.sigma_depth)) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuideMoments.sigma_depth must be finite and > 0 with a finite f32 reciprocal (0 = the default)");
    const double k = g->variance_strength;
    if (!(std::isfinite(k) && k >= 0.0) || std::signbit(k) || !std::isfinite((float)k)) return set_err(ctx, RT_ERR_INVALID, "RtDenoiseGuideMoments.variance_strength must be finite in f32 and > 0 (0 = the default)");
    ma.kappa = (float)(k != 0.0 ? k : RT_DENOISE_MOMENTS_VARIANCE_STRENGTH);
    return RT_OK;
}

}  // namespace

}  // namespace rtk

int rt_denoise_check(uint32_t width, uint32_t height, const RtDenoiseOptions* options) {
    rtk::NlmOptions o;
    return rtk::nlm_options(nullptr, width, height, options, o);
}

int rt_denoise_device(RtCtx* ctx, const RtDenoiseOptions* options, uint32_t width, uint32_t height, const void* rgb_sum_device, const void* sq_sum_device,
                      uint32_t samples, const void* counts_device, void* mean_out_device) {
    using rti::set_err;
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    if (!rgb_sum_device || !sq_sum_device || !mean_out_device) return set_err(ctx, RT_ERR_INVALID, "denoise: rgb_sum / sq_sum / mean_out is null");
    if (mean_out_device == rgb_sum_device || mean_out_device == sq_sum_device) return set_err(ctx, RT_ERR_INVALID, "denoise: mean_out must not be an input buffer");
    rtk::NlmOptions o;
    const int v = rtk::nlm_options(ctx, width, height, options, o); if (v != RT_OK) return v;
    if (!counts_device && samples == 0u) return set_err(ctx, RT_ERR_INVALID, "denoise: samples must be >= 1 when there is no counts buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t n_pixels = width * height;
    HIP_TRY(ctx, ctx->denoise_planes.ensure((size_t)n_pixels * 3u * sizeof(float2)));
    hipLaunchKernelGGL(rtk::k_nlm_prepare, dim3((n_pixels + 255u) / 256u), dim3(256), 0, ctx->stream, (const float*)rgb_sum_device, (const float*)sq_sum_device,
                       (const uint32_t*)counts_device, samples, o.m, n_pixels, (float2*)ctx->denoise_planes.p);
    HIP_TRY(ctx, hipGetLastError());
    rtk::NlmArgs a{};
    a.planes = (const float2*)ctx->denoise_planes.p; a.out = (float*)mean_out_device; a.width = width; a.height = height; a.r = o.r;
    a.k2 = (float)(o.strength * o.strength); a.alpha = (float)o.alpha; a.eps = (float)o.eps;
    HIP_TRY(ctx, rtk::launch_nlm(a, o.f, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_denoise_guided_check(uint32_t width, uint32_t height, const RtDenoiseOptions* options, const RtDenoiseGuide* guide) {
    rtk::NlmOptions o; rtk::GuideArgs g;
    return rtk::nlm_guided_options(nullptr, width, height, options, guide, o, g);
}

int rt_denoise_guided_device(RtCtx* ctx, const RtDenoiseOptions* options, const RtDenoiseGuide* guide, uint32_t width, uint32_t height, const void* rgb_sum_device,
                             const void* sq_sum_device, uint32_t samples, const void* counts_device, void* mean_out_device) {
    using rti::set_err;
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    if (!rgb_sum_device || !sq_sum_device || !mean_out_device) return set_err(ctx, RT_ERR_INVALID, "denoise: rgb_sum / sq_sum / mean_out is null");
    rtk::NlmOptions o; rtk::GuideArgs g;
    const int v = rtk::nlm_guided_options(ctx, width, height, options, guide, o, g); if (v != RT_OK) return v;
    for (const void* in : {rgb_sum_device, sq_sum_device, counts_device, (const void*)g.albedo, (const void*)g.normal, (const void*)g.depth, (const void*)g.hits})
        if (in && in == mean_out_device) return set_err(ctx, RT_ERR_INVALID, "denoise: mean_out must not be an input buffer (the feature planes included)");
    if (!counts_device && samples == 0u) return set_err(ctx, RT_ERR_INVALID, "denoise: samples must be >= 1 when there is no counts buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t n_pixels = width * height;
    HIP_TRY(ctx, ctx->denoise_planes.ensure((size_t)n_pixels * 3u * sizeof(float2)));
    HIP_TRY(ctx, ctx->denoise_guide.ensure((size_t)n_pixels * sizeof(uint4)));
    hipLaunchKernelGGL(rtk::k_nlm_prepare, dim3((n_pixels + 255u) / 256u), dim3(256), 0, ctx->stream, (const float*)rgb_sum_device, (const float*)sq_sum_device,
                       (const uint32_t*)counts_device, samples, o.m, n_pixels, (float2*)ctx->denoise_planes.p);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(rtk::k_nlm_guide_prepare, dim3((n_pixels + 255u) / 256u), dim3(256), 0, ctx->stream, g, n_pixels, (uint4*)ctx->denoise_guide.p,
                       (float2*)ctx->denoise_planes.p);
    HIP_TRY(ctx, hipGetLastError());
    rtk::NlmArgs a{};
    a.planes = (const float2*)ctx->denoise_planes.p; a.out = (float*)mean_out_device; a.width = width; a.height = height; a.r = o.r;
    a.k2 = (float)(o.strength * o.strength); a.alpha = (float)o.alpha; a.eps = (float)o.eps;
    HIP_TRY(ctx, rtk::launch_nlm_guided(a, (const uint4*)ctx->denoise_guide.p, o.f, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_denoise_guided_moments_check(uint32_t width, uint32_t height, const RtDenoiseOptions* options, const RtDenoiseGuideMoments* guide) {
    rtk::NlmOptions o; rtk::GuideMomArgs g;
    return rtk::nlm_guided_moments_options(nullptr, width, height, options, guide, o, g);
}

int rt_denoise_guided_moments_device(RtCtx* ctx, const RtDenoiseOptions* options, const RtDenoiseGuideMoments* guide, uint32_t width, uint32_t height,
                                     const void* rgb_sum_device, const void* sq_sum_device, uint32_t samples, const void* counts_device, void* mean_out_device) {
    using rti::set_err;
    if (!ctx) return set_err(nullptr, RT_ERR_INVALID, "ctx is null");
    if (!rgb_sum_device || !sq_sum_device || !mean_out_device) return set_err(ctx, RT_ERR_INVALID, "denoise: rgb_sum / sq_sum / mean_out is null");
    rtk::NlmOptions o; rtk::GuideMomArgs g;
    const int v = rtk::nlm_guided_moments_options(ctx, width, height, options, guide, o, g); if (v != RT_OK) return v;
    for (const void* in : {rgb_sum_device, sq_sum_device, counts_device, (const void*)g.g.albedo, (const void*)g.g.normal, (const void*)g.g.depth, (const void*)g.g.hits,
                           (const void*)g.albedo_sq, (const void*)g.normal_sq, (const void*)g.depth_sq})
        if (in && in == mean_out_device) return set_err(ctx, RT_ERR_INVALID, "denoise: mean_out must not be an input buffer (the feature planes included)");
    if (!counts_device && samples == 0u) return set_err(ctx, RT_ERR_INVALID, "denoise: samples must be >= 1 when there is no counts buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t n_pixels = width * height;
    HIP_TRY(ctx, ctx->denoise_planes.ensure((size_t)n_pixels * 3u * sizeof(float2)));
    HIP_TRY(ctx, ctx->denoise_guide.ensure((size_t)n_pixels * (sizeof(uint4) + sizeof(uint2))));      // the 16-byte records, then the 8-byte ones
    uint4* rec = (uint4*)ctx->denoise_guide.p; uint2* rec2 = (uint2*)(rec + n_pixels);
    hipLaunchKernelGGL(rtk::k_nlm_prepare, dim3((n_pixels + 255u) / 256u), dim3(256), 0, ctx->stream, (const float*)rgb_sum_device, (const float*)sq_sum_device,
                       (const uint32_t*)counts_device, samples, o.m, n_pixels, (float2*)ctx->denoise_planes.p);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(rtk::k_nlm_guide_moments_prepare, dim3((n_pixels + 255u) / 256u), dim3(256), 0, ctx->stream, g, n_pixels, rec, rec2, (float2*)ctx->denoise_planes.p);
    HIP_TRY(ctx, hipGetLastError());
    rtk::NlmArgs a{};
    a.planes = (const float2*)ctx->denoise_planes.p; a.out = (float*)mean_out_device; a.width = width; a.height = height; a.r = o.r;
    a.k2 = (float)(o.strength * o.strength); a.alpha = (float)o.alpha; a.eps = (float)o.eps;
    HIP_TRY(ctx, rtk::launch_nlm_guided_moments(a, g.kappa, rec, rec2, o.f, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}
