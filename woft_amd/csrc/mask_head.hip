// MaskHead input (weighted_raft.py:295-309): the target feature map warped onto the source grid by the final coordinates,
//   warped = bilinear_sampler(fmap2, coords1)   (raft_core/utils/utils.py:59-73: grid_sample, align_corners=True, zeros)
// The head's convolutions themselves run on the conv kernels (first layer two-source: [fmap1 | warped]), its closing 1x1 conv
// on woft_wh_reduce and its upsampling on woft_convex_upsample / woft_upflow8 (engine.py).
#include "common.h"

namespace {

// a + k * v in fused multiply-adds (the library is built with -ffp-contract=off: a plain `a += k * v` rounds twice)
__device__ __forceinline__ f32x4 fma4_(float k, const f32x4 v, f32x4 a) {
    return f32x4{fmaf(k, v[0], a[0]), fmaf(k, v[1], a[1]), fmaf(k, v[2], a[2]), fmaf(k, v[3], a[3])};
}

// One wavefront holds 64 / lpp pixels, lpp = lanes per pixel (a power of two >= c / 4, at most 64); a lane owns float4
// channel groups q, q + lpp, ... of its pixel: a 256-channel row is one 1 KiB coalesced load per corner.
// Coordinates take the reference's normalise / un-normalise round trip in the same fp32 operations:
//   g = 2 x / (W - 1) - 1             (utils.py:63-64)
//   ix = ((g + 1) / 2) * (W - 1)      (grid_sample, align_corners=True; equal to (g + 1) * ((W - 1) / 2): both halvings exact)
// then ix0 = floor(ix), wx = ix - ix0, and each of the four corners contributes with weight 0 when it lies outside the map
// (zero padding: no clamping).  The bounds are tested on the float corners, so coordinates far outside (or NaN) never
// form an index.
__global__ __launch_bounds__(256) void warp_features_kernel(const float* __restrict__ f, int h, int w, int c, int cs,
                                                            const float* __restrict__ coords, int64_t n_pix,
                                                            float* __restrict__ out, int ld_out, int lpp) {
    const int lane = threadIdx.x & 63;
    const int64_t p = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / lpp) + lane / lpp;
    if (p >= n_pix) return;
    const int sub = lane & (lpp - 1);
    const float x = coords[2 * p], y = coords[2 * p + 1];
    const float gx = 2.f * x / (float)(w - 1) - 1.f, gy = 2.f * y / (float)(h - 1) - 1.f;
    const float ix = ((gx + 1.f) / 2.f) * (float)(w - 1), iy = ((gy + 1.f) / 2.f) * (float)(h - 1);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float wx = ix - x0f, wy = iy - y0f;
    const float ex = 1.f - wx, ny = 1.f - wy;
    const bool vx0 = x0f >= 0.f && x0f <= (float)(w - 1), vx1 = x0f >= -1.f && x0f <= (float)(w - 2);
    const bool vy0 = y0f >= 0.f && y0f <= (float)(h - 1), vy1 = y0f >= -1.f && y0f <= (float)(h - 2);
    // grid_sample's corner weights: nw = (1 - wy)(1 - wx), ne = (1 - wy) wx, sw = wy (1 - wx), se = wy wx
    const float k00 = (vy0 && vx0) ? ny * ex : 0.f, k01 = (vy0 && vx1) ? ny * wx : 0.f;
    const float k10 = (vy1 && vx0) ? wy * ex : 0.f, k11 = (vy1 && vx1) ? wy * wx : 0.f;
    // (row offsets only for valid corners: the others are never dereferenced)
    const int xi = (vx0 || vx1) ? (int)x0f : 0, yi = (vy0 || vy1) ? (int)y0f : 0;
    const int64_t r00 = ((int64_t)yi * w + xi) * cs, r10 = r00 + (int64_t)w * cs;
    float* o = out + p * (int64_t)ld_out;
    for (int q = sub; q < c / 4; q += lpp) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (k00 != 0.f) a = fma4_(k00, *(const f32x4*)(f + r00 + 4 * q), a);
        if (k01 != 0.f) a = fma4_(k01, *(const f32x4*)(f + r00 + cs + 4 * q), a);
        if (k10 != 0.f) a = fma4_(k10, *(const f32x4*)(f + r10 + 4 * q), a);
        if (k11 != 0.f) a = fma4_(k11, *(const f32x4*)(f + r10 + cs + 4 * q), a);
        *(f32x4*)(o + 4 * q) = a;
    }
}

}  // namespace

extern "C" int woft_warp_features(const float* f, int32_t h, int32_t w, int32_t c, int32_t cs, const float* coords,
                                  int64_t n_pix, float* out, int32_t ld_out, void* stream) {
    if (!f || !coords || !out || c <= 0 || c % 4 != 0 || cs < c || cs % 4 != 0 || ld_out < c || ld_out % 4 != 0 || h < 2 ||
        w < 2 || n_pix < 0)
        return WOFT_EINVAL;
    if (((uintptr_t)f | (uintptr_t)out) % 16 != 0) return WOFT_EINVAL;
    if (n_pix == 0) return WOFT_OK;
    int lpp = 1;
    while (lpp < 64 && lpp < c / 4) lpp *= 2;
    const int64_t per_block = 4 * (64 / lpp);
    hipLaunchKernelGGL(warp_features_kernel, dim3((unsigned)ceil_div64(n_pix, per_block)), dim3(256), 0, (hipStream_t)stream,
                       f, h, w, c, cs, coords, n_pix, out, ld_out, lpp);
    return woft_launch_status();
}
