// denoise.hip — non-local means over the sample variance (include/rt_hip.h, "denoising"): the kernels and their two entry points.
//   k_nlm_prepare : rgb_sum, sq_sum, sample counts -> per pixel the mean u and the variance of the mean v (f64, rounded to f32), three
//                   float2 planes (u0,u1) (u2,v0) (v1,v2); an invalid pixel carries v0 = -1 (a variance is never negative)
//   k_nlm<F>      : one 32 x 32 output tile per workgroup. The planes of the tile plus an (r + f) halo are staged in LDS once; then, per
//                   window offset: the pointwise term on the tile plus an f halo, its patch sum as a separable box sum through LDS, the
//                   weight, and the sums of w and w (u[q] - u[p]) in registers. No atomics; every pixel's sums are folded in one fixed
//                   order (window rows, then columns; patch taps ascending), so the result does not depend on where tiles fall.
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
