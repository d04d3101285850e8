// Search-window kernels of the window tracker (tracker/WOFT_window.py): the flows run on a rectangle of the frame, so the
// per-frame glue touches the rectangle only --
//   * the pre-warp of the frame, written for the window's pixels alone (warp_pixel.h: the full-frame kernel's own arithmetic),
//   * rectangle copies (template / frame crops),
//   * the bounding box of a mask (Bbox.from_mask, utils/geom_utils.py:46-64), optionally of the template mask carried to the
//     previous frame by a nearest-neighbour warp, produced and measured in one launch.
// Bandwidth-trivial: what counts is launches and bytes touched.
#include <limits.h>
#include <cmath>
#include "common.h"
#include "warp_pixel.h"

namespace {

__global__ void warp_window_kernel(const uint8_t* __restrict__ img, int h, int w, int c, H9 hi, int y0, int x0, int hw, int ww,
                                   uint8_t* __restrict__ out, uint8_t* __restrict__ valid, int nearest) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= (int64_t)hw * ww) return;
    const int j = (int)(o / ww), i = (int)(o - (int64_t)j * ww);
    warp_pixel(img, h, w, c, hi, x0 + i, y0 + j, o, out, valid, nearest);
}

// One thread per 4 output bytes (the output is contiguous: one aligned 32-bit store); a rectangle's rows start anywhere in the
// source, so that side is read by bytes.
__global__ void crop_kernel(const uint8_t* __restrict__ img, int64_t src_pitch, int64_t row_bytes, int64_t n_bytes,
                            uint8_t* __restrict__ out) {
    const int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (b >= n_bytes) return;
    int64_t r = b / row_bytes, k = b - r * row_bytes;
    uint8_t v[4] = {0, 0, 0, 0};
    const int m = (int)((n_bytes - b) < 4 ? (n_bytes - b) : 4);
    for (int e = 0; e < m; ++e) {
        v[e] = img[r * src_pitch + k];
        if (++k == row_bytes) { k = 0; ++r; }
    }
    if (m == 4 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(out + b) = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
    } else {
        for (int e = 0; e < m; ++e) out[b + e] = v[e];
    }
}

// ---- mask bounding box ----------------------------------------------------------------------------------------------------
// Every extreme is kept as a MAXIMUM of a positive code, so that a zeroed scratch means "no pixel seen":
//   e[0] = h - rmin, e[1] = rmax + 1, e[2] = w - cmin, e[3] = cmax + 1      (0: none).
// Threads fold their pixels, a wave folds its lanes by shuffles, lane 0 of a wave that saw a pixel issues four atomic maxima on
// the scratch; the workgroup that draws the last ticket decodes the scratch into bbox and leaves the scratch zeroed.
constexpr int BBOX_WS_INTS = 8;          // e[0..3], ticket, 3 spare

__device__ __forceinline__ void bbox_fold(int (&e)[4], int h, int w, int y, int x) {
    e[0] = max(e[0], h - y);
    e[1] = max(e[1], y + 1);
    e[2] = max(e[2], w - x);
    e[3] = max(e[3], x + 1);
}

__device__ __forceinline__ void bbox_finish(int (&e)[4], int h, int w, int* __restrict__ ws, int32_t* __restrict__ bbox) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) e[q] = max(e[q], __shfl_xor(e[q], off, 64));
    }
    if ((threadIdx.x & 63) == 0 && e[1] > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) atomicMax(&ws[q], e[q]);
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned ticket = (unsigned)atomicAdd(&ws[4], 1);
    if (ticket != gridDim.x - 1) return;
    __threadfence();
    int r[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = atomicExch(&ws[q], 0);        // (read at the L2, where the atomics landed; and reset)
    atomicExch(&ws[4], 0);
    const bool any = r[1] > 0;
    bbox[0] = any ? h - r[0] : 0;
    bbox[1] = any ? r[1] - 1 : 0;
    bbox[2] = any ? w - r[2] : 0;
    bbox[3] = any ? r[3] - 1 : 0;
    bbox[4] = any ? 1 : 0;
}

// 4 consecutive pixels per thread and step (one 32-bit load where the mask is 4-byte aligned), grid-stride.
__global__ __launch_bounds__(256) void mask_bbox_kernel(const uint8_t* __restrict__ mask, int h, int w, int* __restrict__ ws,
                                                        int32_t* __restrict__ bbox) {
    const int64_t n = (int64_t)h * w;
    const bool aligned = (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
    int e[4] = {0, 0, 0, 0};
    for (int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; p < n; p += (int64_t)gridDim.x * blockDim.x * 4) {
        uint32_t v = 0;
        if (aligned && p + 4 <= n) {
            v = *reinterpret_cast<const uint32_t*>(mask + p);
        } else {
            for (int q = 0; q < 4 && p + q < n; ++q) v |= (uint32_t)mask[p + q] << (8 * q);
        }
        if (v == 0) continue;
        int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
        for (int q = 0; q < 4; ++q) {
            if ((v >> (8 * q)) & 0xffu) bbox_fold(e, h, w, y, x);
            if (++x == w) { x = 0; ++y; }
        }
    }
    bbox_finish(e, h, w, ws, bbox);
}

// The mask measured is the nearest-neighbour warp of `mask` (never materialised unless `warped` is given).
__global__ __launch_bounds__(256) void warp_mask_bbox_kernel(const uint8_t* __restrict__ mask, int h, int w, H9 hi,
                                                             uint8_t* __restrict__ warped, int* __restrict__ ws,
                                                             int32_t* __restrict__ bbox) {
    const int64_t n = (int64_t)h * w;
    int e[4] = {0, 0, 0, 0};
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
        const int64_t s = warp_nearest_index(h, w, hi, x, y);
        const uint8_t v = s >= 0 ? mask[s] : (uint8_t)0;
        if (warped != nullptr) warped[p] = v;
        if (v) bbox_fold(e, h, w, y, x);
    }
    bbox_finish(e, h, w, ws, bbox);
}

// ---- the boxes of K carried masks (woft_mask_bbox_multi) ----------------------------------------------------
// The K inverse homographies travel by value in the kernel's arguments (2 304 B at 32 targets), as the occluders of hsynth.hip do.
struct H9Set {
    H9 h[WOFT_MULTI_MAX_TARGETS];
};

// ws: e[t][0..3] of every target, then the ticket and 3 spare ints
inline int64_t bbox_multi_ws_ints(int n_targets) { return 4 * (int64_t)n_targets + 4; }

// warp_mask_bbox_kernel for n_targets masks held as one bit plane: the same pixel loop, the same warp_nearest_index and the same
// codes, once per target that is not skipped (t is block-uniform: every lane reaches the shuffles).  One ticket for all targets;
// the workgroup that draws the last one decodes every row -- a skipped target's scratch was never touched: {0, 0, 0, 0, 0}.
__global__ __launch_bounds__(256) void mask_bbox_multi_kernel(const uint32_t* __restrict__ tbits, int h, int w, int n_targets,
                                                              uint32_t skip, H9Set hs, int* __restrict__ ws,
                                                              int32_t* __restrict__ bbox) {
    const int64_t n = (int64_t)h * w;
    int* const ticket = ws + 4 * n_targets;
    for (int t = 0; t < n_targets; ++t) {
        if ((skip >> t) & 1u) continue;
        const H9 hi = hs.h[t];
        int e[4] = {0, 0, 0, 0};
        for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
            const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
            const int64_t s = warp_nearest_index(h, w, hi, x, y);
            if (s >= 0 && ((tbits[s] >> t) & 1u)) bbox_fold(e, h, w, y, x);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) e[q] = max(e[q], __shfl_xor(e[q], off, 64));
        }
        if ((threadIdx.x & 63) == 0 && e[1] > 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) atomicMax(&ws[4 * t + q], e[q]);
        }
    }
    __threadfence();
    __syncthreads();
    __shared__ int last;
    if (threadIdx.x == 0) last = (unsigned)atomicAdd(ticket, 1) == gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    __threadfence();
    const int t = (int)threadIdx.x;
    if (t < n_targets) {
        int r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = atomicExch(&ws[4 * t + q], 0);   // (read at the L2, where the atomics landed; and reset)
        const bool any = r[1] > 0;
        bbox[5 * t + 0] = any ? h - r[0] : 0;
        bbox[5 * t + 1] = any ? r[1] - 1 : 0;
        bbox[5 * t + 2] = any ? w - r[2] : 0;
        bbox[5 * t + 3] = any ? r[3] - 1 : 0;
        bbox[5 * t + 4] = any ? 1 : 0;
    }
    if (t == 0) atomicExch(ticket, 0);
}

bool rect_ok(int32_t h, int32_t w, int32_t y0, int32_t x0, int32_t hw, int32_t ww) {
    return h > 0 && w > 0 && hw > 0 && ww > 0 && y0 >= 0 && x0 >= 0 && (int64_t)y0 + hw <= h && (int64_t)x0 + ww <= w;
}

}  // namespace

extern "C" int woft_warp_perspective_window_u8(const uint8_t* img, int32_t h, int32_t w, int32_t c, const double* hinv,
                                               int32_t y0, int32_t x0, int32_t hw, int32_t ww, uint8_t* out, uint8_t* valid,
                                               int32_t nearest, void* stream) {
    if (!img || !hinv || (!out && !valid) || c <= 0 || c > 4 || !rect_ok(h, w, y0, x0, hw, ww)) return WOFT_EINVAL;
    if (nearest && !out) return WOFT_EINVAL;
    H9 hi;
    for (int i = 0; i < 9; ++i) hi.v[i] = hinv[i];
    const int64_t n = (int64_t)hw * ww;
    hipLaunchKernelGGL(warp_window_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, (hipStream_t)stream, img, h, w,
                       c, hi, y0, x0, hw, ww, out, valid, nearest);
    return woft_launch_status();
}

extern "C" int woft_crop_u8(const uint8_t* img, int32_t h, int32_t w, int32_t c, int32_t y0, int32_t x0, int32_t hw,
                            int32_t ww, uint8_t* out, void* stream) {
    if (!img || !out || c <= 0 || c > 4 || !rect_ok(h, w, y0, x0, hw, ww)) return WOFT_EINVAL;
    const int64_t row_bytes = (int64_t)ww * c, n_bytes = row_bytes * hw;
    const uint8_t* src = img + ((int64_t)y0 * w + x0) * c;
    hipLaunchKernelGGL(crop_kernel, dim3((unsigned)ceil_div64(ceil_div64(n_bytes, 4), 256)), dim3(256), 0, (hipStream_t)stream,
                       src, (int64_t)w * c, row_bytes, n_bytes, out);
    return woft_launch_status();
}

extern "C" int64_t woft_mask_bbox_ws_bytes(void) { return (int64_t)BBOX_WS_INTS * (int64_t)sizeof(int); }

extern "C" int woft_mask_bbox(const uint8_t* mask, int32_t h, int32_t w, const double* hinv, uint8_t* warped, void* ws,
                              int32_t* bbox, void* stream) {
    if (!mask || !ws || !bbox || h <= 0 || w <= 0 || (warped && !hinv)) return WOFT_EINVAL;
    const int64_t n = (int64_t)h * w;
    if (hinv != nullptr) {
        H9 hi;
        for (int i = 0; i < 9; ++i) hi.v[i] = hinv[i];
        const int64_t blocks = ceil_div64(n, 256);
        hipLaunchKernelGGL(warp_mask_bbox_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0,
                           (hipStream_t)stream, mask, h, w, hi, warped, (int*)ws, bbox);
    } else {
        const int64_t blocks = ceil_div64(ceil_div64(n, 4), 256);
        hipLaunchKernelGGL(mask_bbox_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0,
                           (hipStream_t)stream, mask, h, w, (int*)ws, bbox);
    }
    return woft_launch_status();
}

extern "C" int64_t woft_mask_bbox_multi_ws_bytes(int32_t n_targets) {
    if (n_targets < 1 || n_targets > WOFT_MULTI_MAX_TARGETS) return -1;
    return bbox_multi_ws_ints(n_targets) * (int64_t)sizeof(int);
}

extern "C" int woft_mask_bbox_multi(const uint32_t* tbits, int32_t h, int32_t w, int32_t n_targets, const double* hinv, uint32_t skip,
                                    void* ws, int32_t* bbox, void* stream) {
    if (!tbits || !hinv || !ws || !bbox || h <= 0 || w <= 0 || n_targets < 1 || n_targets > WOFT_MULTI_MAX_TARGETS) return WOFT_EINVAL;
    H9Set hs = {};
    for (int t = 0; t < n_targets; ++t) {
        if ((skip >> t) & 1u) continue;
        for (int i = 0; i < 9; ++i) {
            if (!std::isfinite(hinv[9 * t + i])) return WOFT_EINVAL;
            hs.h[t].v[i] = hinv[9 * t + i];
        }
    }
    // the grid of woft_mask_bbox's warp form; every block walks the targets in turn
    const int64_t blocks = ceil_div64((int64_t)h * w, 256);
    hipLaunchKernelGGL(mask_bbox_multi_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream,
                       tbits, h, w, n_targets, skip, hs, (int*)ws, bbox);
    return woft_launch_status();
}
