// One destination pixel of the perspective warp: shared by the full-frame kernel (upsample.hip) and the windowed /
// mask-measuring kernels (window.hip), so that every one of them writes the same bytes for the same destination pixel.
#pragma once
#include "common.h"

struct H9 { double v[9]; };

// Source coordinates of destination pixel (x, y): Hinv (x, y, 1), de-homogenised, in fp64.
__device__ __forceinline__ void warp_source(const H9& hi, int x, int y, double& sx, double& sy) {
    const double d = hi.v[6] * x + hi.v[7] * y + hi.v[8];
    sx = (hi.v[0] * x + hi.v[1] * y + hi.v[2]) / d;
    sy = (hi.v[3] * x + hi.v[4] * y + hi.v[5]) / d;
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
    double fx0 = floor(sx), fy0 = floor(sy);
    const float fx = (float)(sx - fx0), fy = (float)(sy - fy0);
    fx0 = fmin(fmax(fx0, -4.0), (double)w + 4.0);
    fy0 = fmin(fmax(fy0, -4.0), (double)h + 4.0);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const bool okx0 = x0 >= 0 && x0 < w, okx1 = x0 + 1 >= 0 && x0 + 1 < w;
    const bool oky0 = y0 >= 0 && y0 < h, oky1 = y0 + 1 >= 0 && y0 + 1 < h;
    const float m00 = (okx0 && oky0) ? 1.f : 0.f, m01 = (okx1 && oky0) ? 1.f : 0.f;
    const float m10 = (okx0 && oky1) ? 1.f : 0.f, m11 = (okx1 && oky1) ? 1.f : 0.f;
    const int cx0 = min(max(x0, 0), w - 1), cx1 = min(max(x0 + 1, 0), w - 1);
    const int cy0 = min(max(y0, 0), h - 1), cy1 = min(max(y0 + 1, 0), h - 1);
    if (out != nullptr) {
        for (int k = 0; k < c; ++k) {
            const float t00 = m00 * (float)img[((int64_t)cy0 * w + cx0) * c + k];
            const float t01 = m01 * (float)img[((int64_t)cy0 * w + cx1) * c + k];
            const float t10 = m10 * (float)img[((int64_t)cy1 * w + cx0) * c + k];
            const float t11 = m11 * (float)img[((int64_t)cy1 * w + cx1) * c + k];
            const float top = t00 * (1.f - fx) + t01 * fx, bot = t10 * (1.f - fx) + t11 * fx;
            const float v = top * (1.f - fy) + bot * fy;
            out[o * c + k] = (uint8_t)fminf(fmaxf(rintf(v), 0.f), 255.f);
        }
    }
    if (valid != nullptr) {
        const float top = m00 * (1.f - fx) + m01 * fx, bot = m10 * (1.f - fx) + m11 * fx;
        valid[o] = (top * (1.f - fy) + bot * fy) > 0.f ? 1 : 0;
    }
}
