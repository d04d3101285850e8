// Using one flow together with another (utils/interpolation.py: bilinear_interpolate_torch, flow_warp_coords, chain_flow):
// the reference's point sampler bit for bit, flow chaining, and the forward-backward consistency check.  DESIGN.md section 16.
// Three streaming kernels with a local gather, one point / pixel per lane: no LDS, no atomics, no workspace.
//
// Two samplers, on purpose.  The REFERENCE sampler (interpolation.py:92-133) clamps both corners to the plane and takes the
// weights from the clamped corners, so a point on the last row / column (x0 == x1 after the clamp) samples 0: kept as it is,
// because woft_sample_bilinear stands in for that function.  The EDGE-EXACT sampler of the chain and the check interpolates on
// the closed rectangle [0, w-1] x [0, h-1] (the last row / column return the data there) and calls everything else invalid.
//
// It lives in flow_sample.h (shared with flow_multi.hip), where the address rule is stated: no coordinate, finite or not, can
// produce an address outside the plane.
#include "flow_sample.h"

namespace {

// ---- interpolation.py:92-133, operation for operation in fp32 (every product and sum rounded on its own) ---------------
__global__ __launch_bounds__(FC_T) void sample_bilinear_kernel(const float* __restrict__ data, int c, int h, int w,
                                                               const float* __restrict__ x, const float* __restrict__ y,
                                                               int64_t n, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * FC_T + threadIdx.x;
    if (i >= n) return;
    const float xv = x[i], yv = y[i];
    const float wm = (float)(w - 1), hm = (float)(h - 1);
    const float fx = floorf(xv), fy = floorf(yv);
    // x0 = floor(x), x1 = x0 + 1, both clamped (the reference clamps int64 values; for |x| <= 1e9 the float clamp is the same)
    const float x0 = clamp_plane(fx, wm), x1 = clamp_plane(__fadd_rn(fx, 1.f), wm);
    const float y0 = clamp_plane(fy, hm), y1 = clamp_plane(__fadd_rn(fy, 1.f), hm);
    const int ix0 = (int)x0, ix1 = (int)x1, iy0 = (int)y0, iy1 = (int)y1;
    const float dx1 = __fsub_rn(x1, xv), dx0 = __fsub_rn(xv, x0), dy1 = __fsub_rn(y1, yv), dy0 = __fsub_rn(yv, y0);
    const float wa = __fmul_rn(dx1, dy1), wb = __fmul_rn(dx1, dy0), wc = __fmul_rn(dx0, dy1), wd = __fmul_rn(dx0, dy0);
    const int64_t plane = (int64_t)h * w;
    const int64_t ia = (int64_t)iy0 * w + ix0, ib = (int64_t)iy1 * w + ix0, ic = (int64_t)iy0 * w + ix1,
                  id = (int64_t)iy1 * w + ix1;
    for (int ch = 0; ch < c; ++ch) {
        const float* p = data + ch * plane;
        float r = __fadd_rn(__fmul_rn(wa, p[ia]), __fmul_rn(wb, p[ib]));
        r = __fadd_rn(r, __fmul_rn(wc, p[ic]));
        r = __fadd_rn(r, __fmul_rn(wd, p[id]));
        out[ch * n + i] = r;
    }
}

__global__ __launch_bounds__(FC_T) void flow_chain_kernel(const float* __restrict__ fab, const float* __restrict__ fbc, int h,
                                                          int w, float* __restrict__ fac) {
    const int64_t plane = (int64_t)h * w;
    const int x = (int)blockIdx.x * FC_TX + (int)threadIdx.x;
    if (x >= w) return;
    for (int y = (int)blockIdx.y * FC_TY + (int)threadIdx.y; y < h; y += (int)gridDim.y * FC_TY) {
        const int64_t i = (int64_t)y * w + x;
        const float fx = fab[i], fy = fab[plane + i];
        const float qx = (float)x + fx, qy = (float)y + fy;
        const Tap t = sample_flow(fbc, h, w, plane, qx, qy);
        fac[i] = t.valid ? fx + t.sx : NAN;
        fac[plane + i] = t.valid ? fy + t.sy : NAN;
    }
}

__global__ __launch_bounds__(FC_T) void flow_fb_kernel(const float* __restrict__ fab, const float* __restrict__ fba, int h, int w,
                                                       float alpha, float beta, float* __restrict__ err,
                                                       float* __restrict__ ok) {
    const int64_t plane = (int64_t)h * w;
    const int x = (int)blockIdx.x * FC_TX + (int)threadIdx.x;
    if (x >= w) return;
    for (int y = (int)blockIdx.y * FC_TY + (int)threadIdx.y; y < h; y += (int)gridDim.y * FC_TY) {
        const int64_t i = (int64_t)y * w + x;
        const float fx = fab[i], fy = fab[plane + i];
        const float qx = (float)x + fx, qy = (float)y + fy;
        const Tap t = sample_flow(fba, h, w, plane, qx, qy);
        const float dx = fx + t.sx, dy = fy + t.sy;
        const float e2 = dx * dx + dy * dy;
        const float bound = alpha * ((fx * fx + fy * fy) + (t.sx * t.sx + t.sy * t.sy)) + beta;
        if (err != nullptr) err[i] = t.valid ? sqrtf(e2) : INFINITY;
        if (ok != nullptr) ok[i] = (t.valid && e2 <= bound) ? 1.f : 0.f;  // (a NaN e2 or bound fails the compare)
    }
}

}  // namespace

extern "C" int woft_sample_bilinear(const float* data, int32_t c, int32_t h, int32_t w, const float* x, const float* y,
                                    int64_t n, float* out, void* stream) {
    if (!data || !x || !y || !out || c <= 0 || n < 0 || bad_side(h, w)) return WOFT_EINVAL;
    if (ceil_div64(n, FC_T) > (int64_t)0x7fffffff) return WOFT_EINVAL;
    if (n == 0) return WOFT_OK;
    hipLaunchKernelGGL(sample_bilinear_kernel, dim3((unsigned)ceil_div64(n, FC_T)), dim3(FC_T), 0, (hipStream_t)stream, data,
                       c, h, w, x, y, n, out);
    return woft_launch_status();
}

extern "C" int woft_flow_chain(const float* fab, const float* fbc, int32_t h, int32_t w, float* fac, void* stream) {
    if (!fab || !fbc || !fac || bad_side(h, w)) return WOFT_EINVAL;
    hipLaunchKernelGGL(flow_chain_kernel, pixel_grid(h, w), dim3(FC_TX, FC_TY), 0, (hipStream_t)stream, fab, fbc, h, w, fac);
    return woft_launch_status();
}

extern "C" int woft_flow_fb(const float* fab, const float* fba, int32_t h, int32_t w, float alpha, float beta, float* err,
                            float* ok, void* stream) {
    if (!fab || !fba || (!err && !ok) || bad_side(h, w)) return WOFT_EINVAL;
    if (!(alpha >= 0.f) || !(beta >= 0.f) || isinf(alpha) || isinf(beta)) return WOFT_EINVAL;       // (NaN fails >=)
    hipLaunchKernelGGL(flow_fb_kernel, pixel_grid(h, w), dim3(FC_TX, FC_TY), 0, (hipStream_t)stream, fab, fba, h, w, alpha,
                       beta, err, ok);
    return woft_launch_status();
}
