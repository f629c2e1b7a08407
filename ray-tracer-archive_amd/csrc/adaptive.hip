// adaptive.hip — the device side of adaptive sampling (include/rt_hip.h, "adaptive sampling"), outside the render's hot path:
//   k_list_check       : a pixel list before a list pass reads it (in-image slots, strictly ascending, counts == first_sample)
//   k_list_map         : output slot -> list index, for the list pass's item_slot (kernels.hip)
//   k_select_*         : the active list, by a deterministic stream compaction (wave ballots, one scan, scatter)
//   k_write_color_counts: write_color with every pixel's own sample count
#include <hip/hip_runtime.h>
#include <math.h>

#include "kernels.h"

namespace rtk {

namespace {

// the pixel of an output slot lies inside the image (clipped slots of edge tiles do not); slot < slots is the caller's
__device__ inline bool slot_in_image(uint32_t slot, uint32_t width, uint32_t height, uint32_t shard_count, uint32_t shard_index, uint32_t ts, uint32_t tiles_x) {
    if (shard_count <= 1u) return slot < width * height;
    const uint32_t ts2 = ts * ts, lt = slot / ts2, r = slot - lt * ts2, py = r / ts, px = r - py * ts;
    const uint32_t tile = shard_index + lt * shard_count, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    return tx * ts + px < width && ty * ts + py < height;
}

enum : uint32_t { BAD_RANGE = 1u, BAD_ORDER = 2u, BAD_COUNT = 4u, BAD_CLIPPED = 8u };

// Reads list[0 .. n) and counts only at in-range slots; ORs what is wrong into *verdict (0: the list is good).
__global__ void __launch_bounds__(256) k_list_check(const uint32_t* __restrict__ list, uint32_t n, const uint32_t* __restrict__ counts, uint32_t first_sample,
                                                    uint32_t width, uint32_t height, uint32_t shard_count, uint32_t shard_index, uint32_t ts, uint32_t tiles_x,
                                                    uint32_t slots, uint32_t* __restrict__ verdict) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = list[i];
    uint32_t bad = 0u;
    if (s >= slots) bad |= BAD_RANGE;
    else if (!slot_in_image(s, width, height, shard_count, shard_index, ts, tiles_x)) bad |= BAD_CLIPPED;
    else if (counts[s] != first_sample) bad |= BAD_COUNT;
    if (i > 0u && list[i - 1u] >= s) bad |= BAD_ORDER;
    if (bad != 0u) atomicOr(verdict, bad);
}

__global__ void __launch_bounds__(256) k_list_map(const uint32_t* __restrict__ list, uint32_t n, uint32_t* __restrict__ map) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) map[list[i]] = i;
}

// the selection criterion of include/rt_hip.h, op for op (adaptive.py select_reference restates it in numpy)
__device__ inline bool selected(const SelectArgs& a, uint32_t p) {
    const uint32_t c = a.counts[p];
    if (c != a.first_sample || a.first_sample >= a.frame_samples) return false;
    if (!slot_in_image(p, a.width, a.height, a.shard_count, a.shard_index, a.tile_size, a.tiles_x)) return false;
    if (c < a.min_samples) return true;
    const uint32_t items = (c + a.m - 1u) / a.m;
    if (items < 2u) return true;
    const double k = (double)items, n = (double)c, mm = (double)a.m * (double)a.m;
    for (int ch = 0; ch < 3; ++ch) {
        const double S = (double)a.rgb[(uint64_t)p * 3u + ch], Q = (double)a.sq[(uint64_t)p * 3u + ch];
        if (!isfinite(S) || !isfinite(Q)) return true;
        double d = Q - S * S / k;
        d = d > 0.0 ? d : 0.0;
        const double var = d / (k * (k - 1.0));
        const double tol = a.abs_error + a.rel_error * fabs(S / n);
        if (!(var / mm <= tol * tol)) return true;
    }
    return false;
}

// one bit per slot, one 64-bit ballot per wave (256-thread groups: wave w covers slots 64 w .. 64 w + 63)
__global__ void __launch_bounds__(256) k_select_ballot(SelectArgs a, unsigned long long* __restrict__ masks) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = p < a.slots && selected(a, p);
    const unsigned long long m = __ballot(on);
    if ((threadIdx.x & 63u) == 0u && p < a.slots) masks[p >> 6] = m;
}

// exclusive scan of the waves' popcounts by ONE workgroup: thread t owns a run of consecutive waves; *n_out = the list's length
constexpr uint32_t kScanThreads = 1024u;
__global__ void __launch_bounds__(kScanThreads) k_select_scan(const unsigned long long* __restrict__ masks, uint32_t n_waves, uint32_t* __restrict__ offsets,
                                                             uint32_t* __restrict__ n_out) {
    __shared__ uint32_t part[kScanThreads];
    const uint32_t t = threadIdx.x, run = (n_waves + kScanThreads - 1u) / kScanThreads;
    const uint32_t lo = min(n_waves, t * run), hi = min(n_waves, lo + run);
    uint32_t sum = 0u;
    for (uint32_t w = lo; w < hi; ++w) sum += (uint32_t)__popcll(masks[w]);
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1u; d < kScanThreads; d <<= 1) {   // inclusive Hillis-Steele scan of the runs' sums
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t at = part[t] - sum;
    for (uint32_t w = lo; w < hi; ++w) { offsets[w] = at; at += (uint32_t)__popcll(masks[w]); }
    if (t == kScanThreads - 1u) *n_out = part[t];
}

__global__ void __launch_bounds__(256) k_select_scatter(const unsigned long long* __restrict__ masks, const uint32_t* __restrict__ offsets, uint32_t slots,
                                                        uint32_t* __restrict__ out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= slots) return;
    const unsigned long long m = masks[p >> 6];
    if (((m >> (p & 63u)) & 1ull) == 0ull) return;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));   // set bits of the lanes below this one
    out[offsets[p >> 6] + below] = p;
}

// k_write_color (kernels.hip) with spp = counts[pixel]: the same write_color_byte (kernels.h); a pixel without a sample is black
__global__ void __launch_bounds__(256) k_write_color_counts(const float* __restrict__ rgb_sum, const uint32_t* __restrict__ counts, uint32_t n_pixels,
                                                            uint8_t* __restrict__ rgb8) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels * 3u) return;
    const uint32_t spp = counts[i / 3u];
    rgb8[i] = spp == 0u ? (uint8_t)0 : write_color_byte(rgb_sum[i], spp);
}

}  // namespace

hipError_t launch_list_check(const uint32_t* list, uint32_t n, const uint32_t* counts, uint32_t first_sample, uint32_t width, uint32_t height, uint32_t shard_count,
                             uint32_t shard_index, uint32_t tile_size, uint32_t tiles_x, uint32_t slots, uint32_t* verdict, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_list_check, dim3((n + 255u) / 256u), dim3(256), 0, stream, list, n, counts, first_sample, width, height, shard_count, shard_index, tile_size,
                       tiles_x, slots, verdict);
    return hipGetLastError();
}

hipError_t launch_list_map(const uint32_t* list, uint32_t n, uint32_t* map, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_list_map, dim3((n + 255u) / 256u), dim3(256), 0, stream, list, n, map);
    return hipGetLastError();
}

hipError_t launch_select(const SelectArgs& a, unsigned long long* masks, uint32_t* offsets, uint32_t* out, uint32_t* n_out, hipStream_t stream) {
    const uint32_t blocks = (a.slots + 255u) / 256u, n_waves = (a.slots + 63u) / 64u;
    if (blocks == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_select_ballot, dim3(blocks), dim3(256), 0, stream, a, masks);
    hipError_t e = hipGetLastError(); if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(kScanThreads), 0, stream, masks, n_waves, offsets, n_out);
    e = hipGetLastError(); if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_select_scatter, dim3(blocks), dim3(256), 0, stream, masks, offsets, a.slots, out);
    return hipGetLastError();
}

hipError_t launch_write_color_counts(const float* rgb_sum, const uint32_t* counts, uint32_t n_pixels, uint8_t* rgb8, hipStream_t stream) {
    const uint32_t blocks = (n_pixels * 3u + 255u) / 256u;
    if (blocks == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_write_color_counts, dim3(blocks), dim3(256), 0, stream, rgb_sum, counts, n_pixels, rgb8);
    return hipGetLastError();
}

}  // namespace rtk
