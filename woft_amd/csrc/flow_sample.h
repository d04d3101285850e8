// The edge-exact sampler and the per-pixel launch geometry shared by flow_chain.hip and flow_multi.hip (DESIGN.md sections 16, 18).
//
// The EDGE-EXACT sampler interpolates on the closed rectangle [0, w-1] x [0, h-1] (the last row / column return the data there)
// and calls everything else invalid.
//
// Addresses: every integer index is converted from a float that was first forced into [0, w-1] (or [0, h-1]) by two ordered
// compares that a NaN fails into the lower bound; w - 1 and h - 1 are exact in fp32 (w, h <= 2^24 is checked by the entry
// points).  No coordinate, finite or not, can produce an address outside the plane.
#pragma once
#include <math.h>

#include "common.h"

namespace {

constexpr int FC_T = 256;
// the per-pixel kernels: a workgroup is FC_TY rows of FC_TX pixels (one wave per row segment: coalesced reads of the pixel's own
// planes and writes), rows beyond 65535 * FC_TY by a grid-stride loop -- the pixel's (x, y) comes from the launch geometry, no
// division
constexpr int FC_TX = 64, FC_TY = 4;
constexpr int32_t FC_MAX_SIDE = 1 << 24;          // (float)(side - 1) is exact up to here

// v forced into [0, hi]; NaN -> 0, +inf -> hi, -inf -> 0
__device__ __forceinline__ float clamp_plane(float v, float hi) {
    const float lo = v >= 0.f ? v : 0.f;
    return lo <= hi ? lo : hi;
}

// where q = (qx, qy) lands in an h x w plane: validity, the four tap offsets (always inside the plane) and the weights
struct TapAt {
    bool valid;
    int64_t i00, i01, i10, i11;
    float ax, ay, bx, by;
};

__device__ __forceinline__ TapAt tap_at(int h, int w, float qx, float qy) {
    const float wm = (float)(w - 1), hm = (float)(h - 1);
    TapAt t;
    t.valid = qx >= 0.f && qx <= wm && qy >= 0.f && qy <= hm;              // (a NaN fails)
    const float x0f = clamp_plane(floorf(qx), wm), y0f = clamp_plane(floorf(qy), hm);   // (valid: floor(q) itself)
    const int x0 = (int)x0f, y0 = (int)y0f;
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    t.ax = qx - x0f, t.ay = qy - y0f;
    t.bx = 1.f - t.ax, t.by = 1.f - t.ay;
    t.i00 = (int64_t)y0 * w + x0, t.i01 = (int64_t)y0 * w + x1, t.i10 = (int64_t)y1 * w + x0, t.i11 = (int64_t)y1 * w + x1;
    return t;
}

// one plane at the taps of t: (1-ay)*((1-ax)*d00 + ax*d01) + ay*((1-ax)*d10 + ax*d11), every product and sum rounded on its own
__device__ __forceinline__ float tap_plane(const float* __restrict__ f, const TapAt& t) {
    return t.by * (t.bx * f[t.i00] + t.ax * f[t.i01]) + t.ay * (t.bx * f[t.i10] + t.ax * f[t.i11]);
}

// ---- the edge-exact sampler of a [2][h][w] flow at q ---------------------------------------------------------------------
struct Tap {
    bool valid;
    float sx, sy;
};

__device__ __forceinline__ Tap sample_flow(const float* __restrict__ f, int h, int w, int64_t plane, float qx, float qy) {
    const TapAt a = tap_at(h, w, qx, qy);
    Tap t;
    t.valid = a.valid;
    t.sx = tap_plane(f, a);
    t.sy = tap_plane(f + plane, a);
    return t;
}

inline dim3 pixel_grid(int32_t h, int32_t w) {
    const int64_t gy = ceil_div64(h, FC_TY);
    return dim3((unsigned)ceil_div64(w, FC_TX), (unsigned)(gy < 65535 ? gy : 65535));
}

inline bool bad_side(int32_t h, int32_t w) { return h <= 0 || w <= 0 || h > FC_MAX_SIDE || w > FC_MAX_SIDE; }

}  // namespace
