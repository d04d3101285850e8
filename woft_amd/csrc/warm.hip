// RAFT warm start (weighted_raft.py:184,223-224 / raft.py: coords1 = coords1 + flow_init; raft_core/utils/utils.py:28-56:
// forward_interpolate): the initial coordinates from a caller's flow, and the forward projection that carries the flow of
// one frame pair to the next.  DESIGN.md section 13.
#include <math.h>

#include "common.h"

namespace {

// ---- coords1 = grid + flow_init; flow4 / flow_cat = flow_init itself (no (grid + f) - grid round trip) ---------------
__global__ void coords_init_flow_kernel(float* __restrict__ coords1, const float* __restrict__ flow_init, int wf,
                                        int64_t n_pix, float* __restrict__ flow4, float* __restrict__ flow_cat,
                                        int ld_cat) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pix) return;
    const float fx = flow_init[i], fy = flow_init[n_pix + i];
    coords1[i * 2] = (float)(i % wf) + fx;
    coords1[i * 2 + 1] = (float)(i / wf) + fy;
    if (flow4 != nullptr) {
        f32x4 f = {fx, fy, 0.f, 0.f};
        *(f32x4*)(flow4 + i * 4) = f;
    }
    if (flow_cat != nullptr) {
        flow_cat[i * ld_cat] = fx;
        flow_cat[i * ld_cat + 1] = fy;
    }
}

// ---- forward_interpolate: nearest valid projected point per grid cell, brute force, exact ----------------------------
// Point i (row-major, at (x0, y0)) lands at (x1, y1) = (x0 + dx, y0 + dy) in fp64 (fp32 + integer: exact) and is valid iff
// 0 < x1 < wf and 0 < y1 < hf, strictly.  Cell c takes (dx, dy) of the valid point with the smallest
// (cx - x1)^2 + (cy - y1)^2 (fp64: two products, one sum, no contraction); of equal distances the LOWEST point index wins
// (points are visited in index order, the running minimum is replaced on a strict <).  No valid point: zeros.
// A workgroup of FI_T threads owns FI_T cells (one per lane) and walks ALL points in chunks of FI_CHUNK staged through LDS as
// (x1, y1) doubles -- an invalid point is staged as +inf, whose distance +inf never beats a running minimum that starts at
// +inf.  Every lane of a wave reads the same LDS address in the scan (a broadcast: no bank conflicts).  8 KiB of LDS per
// workgroup; 1/8-resolution grids of 1080p / 4K frames give 254 / 1013 workgroups.  No atomics, no cross-lane reduction.
constexpr int FI_T = 128, FI_CHUNK = 512;
__global__ __launch_bounds__(FI_T) void forward_interpolate_kernel(const float* __restrict__ flow, int hf, int wf,
                                                                   float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double sx[FI_CHUNK], sy[FI_CHUNK];
    const int P = hf * wf;
    const int cell = (int)blockIdx.x * FI_T + (int)threadIdx.x;
    const double cx = (double)(cell % wf), cy = (double)(cell / wf);
    const double inf = (double)INFINITY;
    double best = inf;
    int best_i = -1;
    for (int base = 0; base < P; base += FI_CHUNK) {
        const int n = min(FI_CHUNK, P - base);           // (uniform over the workgroup: every thread reaches the barriers)
        __syncthreads();                                 // (the previous chunk is consumed)
        for (int k = (int)threadIdx.x; k < n; k += FI_T) {
            const int i = base + k;
            const double x1 = (double)(i % wf) + (double)flow[i], y1 = (double)(i / wf) + (double)flow[P + i];
            const bool ok = x1 > 0.0 && x1 < (double)wf && y1 > 0.0 && y1 < (double)hf;      // (NaN: not valid)
            sx[k] = ok ? x1 : inf;
            sy[k] = ok ? y1 : inf;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < n; ++k) {
            const double ddx = cx - sx[k], ddy = cy - sy[k];
            const double d = ddx * ddx + ddy * ddy;
            if (d < best) {
                best = d;
                best_i = base + k;
            }
        }
    }
    if (cell < P) {
        out[cell] = best_i >= 0 ? flow[best_i] : 0.f;
        out[P + cell] = best_i >= 0 ? flow[P + best_i] : 0.f;
    }
}

}  // namespace

extern "C" int woft_coords_init_flow(float* coords1, const float* flow_init, int32_t hf, int32_t wf, float* flow4,
                                     float* flow_cat, int32_t ld_cat, void* stream) {
    if (!coords1 || !flow_init || hf <= 0 || wf <= 0) return WOFT_EINVAL;
    const int64_t n = (int64_t)hf * wf;
    hipLaunchKernelGGL(coords_init_flow_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       coords1, flow_init, wf, n, flow4, flow_cat, ld_cat);
    return woft_launch_status();
}

extern "C" int woft_forward_interpolate(const float* flow, int32_t hf, int32_t wf, float* out, void* stream) {
    if (!flow || !out || flow == out || hf <= 0 || wf <= 0 || (int64_t)hf * wf > (int64_t)1 << 30) return WOFT_EINVAL;
    const int64_t n = (int64_t)hf * wf;
    hipLaunchKernelGGL(forward_interpolate_kernel, dim3((unsigned)ceil_div64(n, FI_T)), dim3(FI_T), 0, (hipStream_t)stream,
                       flow, hf, wf, out);
    return woft_launch_status();
}
