// Synthetic-homography training pairs: the warped, photometrically changed, occluded second frame of an
// image and the labels a loss needs (flow, visibility, valid), each in one launch.  The per-pixel sampling is warp_pixel.h's, so
// the render without occluders writes the bytes of the full-frame warp (upsample.hip), and the labels sample the same continuous
// alpha field that the render composites.
#include "common.h"
#include "warp_pixel.h"

namespace {

struct OccSet {
    const uint8_t* tex[WOFT_HSYNTH_MAX_OCC];
    int ho[WOFT_HSYNTH_MAX_OCC], wo[WOFT_HSYNTH_MAX_OCC];
    H9 hinv[WOFT_HSYNTH_MAX_OCC];
    int n;
};

struct Photo { float gain[3], bias[3]; };

// The background behind the plane (woft_hsynth_render_bg): an image and the homography destination frame -> image.
struct Backdrop {
    const uint8_t* img;
    int hb, wb;
    H9 hinv;
};

// One BGRA tap of an occluder, premultiplied: a = m * (alpha / 255), p[c] = a * colour[c].
__device__ __forceinline__ void occ_tap(const uint8_t* __restrict__ tex, int wo, int cy, int cx, float m, float& a, float* p) {
    const uint32_t q = *reinterpret_cast<const uint32_t*>(tex + ((int64_t)cy * wo + cx) * 4);
    a = m * ((float)(q >> 24) / 255.f);
    p[0] = a * (float)(q & 255u);
    p[1] = a * (float)((q >> 8) & 255u);
    p[2] = a * (float)((q >> 16) & 255u);
}

// Alpha A_k of occluder k at destination point (x, y); with COLOUR also the premultiplied colour O_k.
template <bool COLOUR>
__device__ __forceinline__ float occ_sample(const OccSet& oc, int k, double x, double y, float* O) {
    double sx, sy;
    warp_source(oc.hinv[k], x, y, sx, sy);
    const WarpTaps t = warp_taps(oc.ho[k], oc.wo[k], sx, sy);
    float a00, a01, a10, a11, p00[3], p01[3], p10[3], p11[3];
    occ_tap(oc.tex[k], oc.wo[k], t.cy0, t.cx0, t.m00, a00, p00);
    occ_tap(oc.tex[k], oc.wo[k], t.cy0, t.cx1, t.m01, a01, p01);
    occ_tap(oc.tex[k], oc.wo[k], t.cy1, t.cx0, t.m10, a10, p10);
    occ_tap(oc.tex[k], oc.wo[k], t.cy1, t.cx1, t.m11, a11, p11);
    if (COLOUR) {
#pragma unroll
        for (int c = 0; c < 3; ++c) O[c] = warp_blend(t, p00[c], p01[c], p10[c], p11[c]);
    }
    return warp_blend(t, a00, a01, a10, a11);
}

// Channels g[0..2] of the background at destination pixel (x, y): replicate border (every tap counts, at its clamped index), zero
// where the denominator is not positive or a coordinate is not finite.
__device__ __forceinline__ void backdrop_sample(const Backdrop& bg, int x, int y, float* g) {
    double gx, gy;
    const double d = warp_source(bg.hinv, x, y, gx, gy);
    g[0] = g[1] = g[2] = 0.f;
    if (!(d > 0.0) || !isfinite(gx) || !isfinite(gy)) return;
    WarpTaps t = warp_taps(bg.hb, bg.wb, gx, gy);
    t.m00 = t.m01 = t.m10 = t.m11 = 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = warp_sample(bg.img, bg.wb, 3, t, c);
}

// Thread i renders pixels 4i .. 4i+3 of the flattened (h, w) frame: 12 bytes of out_u8, 12 floats of out_f32, 4 of cover, stored
// as 3 dwords / 3 + 1 float4 when `vec` (every output base aligned; n a multiple of 4 or the thread not the last one).  BG: the
// background composited behind the plane and the plane's coverage written next to cover (woft_hsynth_render_bg); without it the
// instructions of woft_hsynth_render.
template <bool BG>
__global__ __launch_bounds__(256) void hsynth_render_kernel(const uint8_t* __restrict__ base, int hs, int ws, H9 hi, Photo ph,
                                                            OccSet oc, Backdrop bg, uint8_t* __restrict__ out_u8,
                                                            float* __restrict__ out_f32, float* __restrict__ cover,
                                                            float* __restrict__ plane, int h, int w, int vec) {
    const int64_t n = (int64_t)h * w, o0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (o0 >= n) return;
    float v[12], cv[4], pv[4];
    int y = (int)(o0 / w), x = (int)(o0 - (int64_t)y * w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (o0 + j < n) {
            double sx, sy;
            const double den = warp_source(hi, x, y, sx, sy);
            const WarpTaps t = warp_taps(hs, ws, sx, sy);
            float u[3];
            if (BG) {
                const float P = den > 0.0 ? warp_blend(t, t.m00, t.m01, t.m10, t.m11) : 0.f;
                const float behind = 1.f - P;
                float g[3];
                backdrop_sample(bg, x, y, g);
#pragma unroll
                for (int c = 0; c < 3; ++c) u[c] = ph.gain[c] * (warp_sample(base, ws, 3, t, c) + behind * g[c]) + ph.bias[c];
                pv[j] = P;
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) u[c] = ph.gain[c] * warp_sample(base, ws, 3, t, c) + ph.bias[c];
            }
            float keep = 1.f;
#pragma unroll
            for (int k = 0; k < WOFT_HSYNTH_MAX_OCC; ++k) {
                if (k < oc.n) {
                    float O[3];
                    const float A = occ_sample<true>(oc, k, x, y, O);
#pragma unroll
                    for (int c = 0; c < 3; ++c) u[c] = (1.f - A) * u[c] + O[c];
                    keep = keep * (1.f - A);
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 * j + c] = u[c];
            cv[j] = 1.f - keep;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 * j + c] = 0.f;
            cv[j] = 0.f;
            if (BG) pv[j] = 0.f;
        }
        if (++x == w) { x = 0; ++y; }
    }
    if (vec && o0 + 4 <= n) {
        uint32_t d[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            d[q] = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                d[q] |= (uint32_t)(uint8_t)fminf(fmaxf(rintf(v[4 * q + b]), 0.f), 255.f) << (8 * b);
        }
        uint32_t* o32 = reinterpret_cast<uint32_t*>(out_u8 + o0 * 3);
        o32[0] = d[0], o32[1] = d[1], o32[2] = d[2];
        if (out_f32 != nullptr) {
            f32x4* of = reinterpret_cast<f32x4*>(out_f32 + o0 * 3);
#pragma unroll
            for (int q = 0; q < 3; ++q) of[q] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
        }
        if (cover != nullptr) *reinterpret_cast<f32x4*>(cover + o0) = f32x4{cv[0], cv[1], cv[2], cv[3]};
        if (BG && plane != nullptr) *reinterpret_cast<f32x4*>(plane + o0) = f32x4{pv[0], pv[1], pv[2], pv[3]};
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (o0 + j >= n) break;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            out_u8[(o0 + j) * 3 + c] = (uint8_t)fminf(fmaxf(rintf(v[3 * j + c]), 0.f), 255.f);
            if (out_f32 != nullptr) out_f32[(o0 + j) * 3 + c] = v[3 * j + c];
        }
        if (cover != nullptr) cover[o0 + j] = cv[j];
        if (BG && plane != nullptr) plane[o0 + j] = pv[j];
    }
}

// Thread i labels template pixels 4i .. 4i+3 of the flattened (hs, ws) base image.
__global__ __launch_bounds__(256) void hsynth_labels_kernel(int hs, int ws, H9 hf, OccSet oc, int h, int w, float lo, float hi,
                                                            float* __restrict__ flow, float* __restrict__ visible,
                                                            uint8_t* __restrict__ valid, int vec) {
    const int64_t n = (int64_t)hs * ws, o0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (o0 >= n) return;
    float fxv[4], fyv[4], vis[4];
    uint32_t ok[4];
    int y = (int)(o0 / ws), x = (int)(o0 - (int64_t)y * ws);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        fxv[j] = fyv[j] = vis[j] = 0.f;
        ok[j] = 0;
        if (o0 + j < n) {
            double px, py;
            const double d = warp_source(hf, x, y, px, py);
            fxv[j] = (float)(px - (double)x);
            fyv[j] = (float)(py - (double)y);
            const bool inside = d > 0.0 && px >= 0.0 && px <= (double)(w - 1) && py >= 0.0 && py <= (double)(h - 1);
            if (!inside) {
                ok[j] = 1;
            } else {
                float keep = 1.f;
#pragma unroll
                for (int k = 0; k < WOFT_HSYNTH_MAX_OCC; ++k)
                    if (k < oc.n) keep = keep * (1.f - occ_sample<false>(oc, k, px, py, nullptr));
                const float T = 1.f - keep;
                if (T <= lo) {
                    vis[j] = 1.f;
                    ok[j] = 1;
                } else if (T >= hi) {
                    ok[j] = 1;
                }
            }
        }
        if (++x == ws) { x = 0; ++y; }
    }
    if (vec && o0 + 4 <= n) {
        *reinterpret_cast<f32x4*>(flow + o0) = f32x4{fxv[0], fxv[1], fxv[2], fxv[3]};
        *reinterpret_cast<f32x4*>(flow + n + o0) = f32x4{fyv[0], fyv[1], fyv[2], fyv[3]};
        *reinterpret_cast<f32x4*>(visible + o0) = f32x4{vis[0], vis[1], vis[2], vis[3]};
        *reinterpret_cast<uint32_t*>(valid + o0) = ok[0] | (ok[1] << 8) | (ok[2] << 16) | (ok[3] << 24);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (o0 + j >= n) break;
        flow[o0 + j] = fxv[j];
        flow[n + o0 + j] = fyv[j];
        visible[o0 + j] = vis[j];
        valid[o0 + j] = (uint8_t)ok[j];
    }
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Sizes and the occluder array, checked and copied by value; false = reject.
bool hsynth_args(int hs, int ws, const woft_hsynth_occluder* occ, int n_occ, int h, int w, OccSet& oc) {
    if (hs <= 0 || ws <= 0 || h <= 0 || w <= 0 || n_occ < 0 || n_occ > WOFT_HSYNTH_MAX_OCC || (n_occ > 0 && !occ)) return false;
    if ((int64_t)hs * ws >= (1ll << 31) || (int64_t)h * w >= (1ll << 31)) return false;
    oc.n = n_occ;
    for (int k = 0; k < WOFT_HSYNTH_MAX_OCC; ++k) {
        const bool on = k < n_occ;
        if (on && (!occ[k].tex || !aligned_to(occ[k].tex, 4) || occ[k].ho <= 0 || occ[k].wo <= 0)) return false;
        oc.tex[k] = on ? occ[k].tex : nullptr;
        oc.ho[k] = on ? occ[k].ho : 1;
        oc.wo[k] = on ? occ[k].wo : 1;
        for (int i = 0; i < 9; ++i) oc.hinv[k].v[i] = on ? occ[k].hinv[i] : 0.0;
    }
    return true;
}

// Both render entries: arguments checked, one launch of the kernel with or without the background.
int hsynth_render(const uint8_t* base, int hs, int ws, const double* hinv, const float* gain, const float* bias,
                  const woft_hsynth_occluder* occ, int n_occ, const Backdrop* bg, uint8_t* out_u8, float* out_f32, float* cover,
                  float* plane, int h, int w, void* stream) {
    OccSet oc;
    if (!base || !hinv || !out_u8 || !hsynth_args(hs, ws, occ, n_occ, h, w, oc)) return WOFT_EINVAL;
    H9 hi;
    for (int i = 0; i < 9; ++i) hi.v[i] = hinv[i];
    Photo ph;
    for (int c = 0; c < 3; ++c) ph.gain[c] = gain ? gain[c] : 1.f, ph.bias[c] = bias ? bias[c] : 0.f;
    const int vec = aligned_to(out_u8, 4) && aligned_to(out_f32, 16) && aligned_to(cover, 16) && aligned_to(plane, 16);
    const int64_t n4 = ceil_div64((int64_t)h * w, 4);
    const dim3 grid((unsigned)ceil_div64(n4, 256));
    if (bg != nullptr)
        hipLaunchKernelGGL(hsynth_render_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, base, hs, ws, hi, ph, oc, *bg,
                           out_u8, out_f32, cover, plane, h, w, vec);
    else
        hipLaunchKernelGGL(hsynth_render_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, base, hs, ws, hi, ph, oc,
                           Backdrop{}, out_u8, out_f32, cover, plane, h, w, vec);
    return woft_launch_status();
}

}  // namespace

extern "C" int woft_hsynth_render(const uint8_t* base, int32_t hs, int32_t ws, const double* hinv, const float* gain,
                                  const float* bias, const woft_hsynth_occluder* occ, int32_t n_occ, uint8_t* out_u8,
                                  float* out_f32, float* cover, int32_t h, int32_t w, void* stream) {
    return hsynth_render(base, hs, ws, hinv, gain, bias, occ, n_occ, nullptr, out_u8, out_f32, cover, nullptr, h, w, stream);
}

extern "C" int woft_hsynth_render_bg(const uint8_t* base, int32_t hs, int32_t ws, const double* hinv, const float* gain,
                                     const float* bias, const woft_hsynth_occluder* occ, int32_t n_occ, const uint8_t* bg,
                                     int32_t hb, int32_t wb, const double* hinv_bg, uint8_t* out_u8, float* out_f32, float* cover,
                                     float* plane, int32_t h, int32_t w, void* stream) {
    if (!bg || !hinv_bg || hb <= 0 || wb <= 0 || (int64_t)hb * wb >= (1ll << 31)) return WOFT_EINVAL;
    Backdrop b;
    b.img = bg, b.hb = hb, b.wb = wb;
    for (int i = 0; i < 9; ++i) b.hinv.v[i] = hinv_bg[i];
    return hsynth_render(base, hs, ws, hinv, gain, bias, occ, n_occ, &b, out_u8, out_f32, cover, plane, h, w, stream);
}

extern "C" int woft_hsynth_labels(int32_t hs, int32_t ws, const double* hfwd, const woft_hsynth_occluder* occ, int32_t n_occ,
                                  int32_t h, int32_t w, float lo, float hi, float* flow, float* visible, uint8_t* valid,
                                  void* stream) {
    OccSet oc;
    if (!hfwd || !flow || !visible || !valid || !hsynth_args(hs, ws, occ, n_occ, h, w, oc)) return WOFT_EINVAL;
    if (!(0.f <= lo && lo < hi && hi <= 1.f)) return WOFT_EINVAL;
    H9 hf;
    for (int i = 0; i < 9; ++i) hf.v[i] = hfwd[i];
    // (flow's second plane starts hs * ws floats in: 16-byte aligned with the first one only when hs * ws is a multiple of 4)
    const int vec = aligned_to(flow, 16) && aligned_to(visible, 16) && aligned_to(valid, 4) && ((int64_t)hs * ws) % 4 == 0;
    const int64_t n4 = ceil_div64((int64_t)hs * ws, 4);
    hipLaunchKernelGGL(hsynth_labels_kernel, dim3((unsigned)ceil_div64(n4, 256)), dim3(256), 0, (hipStream_t)stream, hs, ws, hf,
                       oc, h, w, lo, hi, flow, visible, valid, vec);
    return woft_launch_status();
}
