// One destination pixel of the perspective warp: shared by the full-frame kernel (upsample.hip) and the windowed /
// mask-measuring kernels (window.hip), so that every one of them writes the same bytes for the same destination pixel.
#pragma once
#include "common.h"

struct H9 { double v[9]; };

// Source coordinates of the destination point (x, y): Hinv (x, y, 1), de-homogenised, in fp64; -> the denominator.  (A pixel's
// integer coordinates convert to double exactly, so the full-frame kernels and the callers with a non-integer point share this.)
__device__ __forceinline__ double warp_source(const H9& hi, double x, double y, double& sx, double& sy) {
    const double d = hi.v[6] * x + hi.v[7] * y + hi.v[8];
    sx = (hi.v[0] * x + hi.v[1] * y + hi.v[2]) / d;
    sy = (hi.v[3] * x + hi.v[4] * y + hi.v[5]) / d;
    return d;
}

// The four bilinear taps of source point (sx, sy) in an h x w image: fractions, in-image flags (zero border) and clamped indices.
struct WarpTaps {
    float fx, fy, m00, m01, m10, m11;
    int cx0, cx1, cy0, cy1;
};

__device__ __forceinline__ WarpTaps warp_taps(int h, int w, double sx, double sy) {
    WarpTaps t;
    double fx0 = floor(sx), fy0 = floor(sy);
    t.fx = (float)(sx - fx0);
    t.fy = (float)(sy - fy0);
    fx0 = fmin(fmax(fx0, -4.0), (double)w + 4.0);
    fy0 = fmin(fmax(fy0, -4.0), (double)h + 4.0);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const bool okx0 = x0 >= 0 && x0 < w, okx1 = x0 + 1 >= 0 && x0 + 1 < w;
    const bool oky0 = y0 >= 0 && y0 < h, oky1 = y0 + 1 >= 0 && y0 + 1 < h;
    t.m00 = (okx0 && oky0) ? 1.f : 0.f, t.m01 = (okx1 && oky0) ? 1.f : 0.f;
    t.m10 = (okx0 && oky1) ? 1.f : 0.f, t.m11 = (okx1 && oky1) ? 1.f : 0.f;
    t.cx0 = min(max(x0, 0), w - 1), t.cx1 = min(max(x0 + 1, 0), w - 1);
    t.cy0 = min(max(y0, 0), h - 1), t.cy1 = min(max(y0 + 1, 0), h - 1);
    return t;
}

// Bilinear combination of four tap values (already multiplied by their flags), un-rounded.
__device__ __forceinline__ float warp_blend(const WarpTaps& t, float t00, float t01, float t10, float t11) {
    const float top = t00 * (1.f - t.fx) + t01 * t.fx, bot = t10 * (1.f - t.fx) + t11 * t.fx;
    return top * (1.f - t.fy) + bot * t.fy;
}

// Channel k of a c-channel uint8 image at source point taps t, un-rounded (what warp_pixel rounds).
__device__ __forceinline__ float warp_sample(const uint8_t* __restrict__ img, int w, int c, const WarpTaps& t, int k) {
    const float t00 = t.m00 * (float)img[((int64_t)t.cy0 * w + t.cx0) * c + k];
    const float t01 = t.m01 * (float)img[((int64_t)t.cy0 * w + t.cx1) * c + k];
    const float t10 = t.m10 * (float)img[((int64_t)t.cy1 * w + t.cx0) * c + k];
    const float t11 = t.m11 * (float)img[((int64_t)t.cy1 * w + t.cx1) * c + k];
    return warp_blend(t, t00, t01, t10, t11);
}

// Nearest-neighbour source pixel of (x, y): -1 outside the h x w image, else its index y * w + x.
__device__ __forceinline__ int64_t warp_nearest_index(int h, int w, const H9& hi, int x, int y) {
    double sx, sy;
    warp_source(hi, x, y, sx, sy);
    const double rx = rint(sx), ry = rint(sy);
    const bool ok = rx >= 0 && rx < w && ry >= 0 && ry < h;
    return ok ? (int64_t)ry * w + (int64_t)rx : (int64_t)-1;
}

// dst(x, y) = src(Hinv (x, y)) written at pixel index o of `out` (c bytes) / `valid` (1 byte): bilinear with zero border
// (or nearest).  `valid` = warp(ones) > 0.
__device__ __forceinline__ void warp_pixel(const uint8_t* __restrict__ img, int h, int w, int c, const H9& hi, int x, int y,
                                           int64_t o, uint8_t* __restrict__ out, uint8_t* __restrict__ valid, int nearest) {
    if (nearest) {
        const int64_t s = warp_nearest_index(h, w, hi, x, y);
        const bool ok = s >= 0;
        for (int k = 0; k < c; ++k) out[o * c + k] = ok ? img[s * c + k] : 0;
        if (valid) valid[o] = ok ? 1 : 0;
        return;
    }
    double sx, sy;
    warp_source(hi, x, y, sx, sy);
    const WarpTaps t = warp_taps(h, w, sx, sy);
    if (out != nullptr) {
        for (int k = 0; k < c; ++k) out[o * c + k] = (uint8_t)fminf(fmaxf(rintf(warp_sample(img, w, c, t, k)), 0.f), 255.f);
    }
    if (valid != nullptr) valid[o] = warp_blend(t, t.m00, t.m01, t.m10, t.m11) > 0.f ? 1 : 0;
}
