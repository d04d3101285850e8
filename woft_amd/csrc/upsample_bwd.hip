// Dense adjoint of the x8 convex upsampling (upsample.hip: convex_upsample_kernel, its wout output) with respect to the
// 1/8-resolution map wlow: what carries a gradient of the full-resolution visibility map back to the MaskHead's logits
// (weighted_raft.py:92-103, 305-308).
//   forward:  v[pixel] = (sum_k s_k * (8 * wlow[n + d_k])) / 8,  s = softmax_k(mask[n][k * 64 + lane]),  out = v or sigmoid(v)
//   backward: g_wlow[q] = sum_{n, k : n + d_k = q} sum_{lanes of n inside the crop window} ((g_up * dsig) / 8) * (s_k * 8)
// Two launches.  The mask -- 576 floats per cell, the one large operand -- is read once: one wavefront per SENDING cell n takes
// the forward's view of it (lane = fine position), forms the nine products a lane sends to the cell's nine neighbours and adds
// each over the 64 lanes by a fixed butterfly: part[n][k].  Then one thread per RECEIVING cell q adds the (at most nine)
// partials addressed to it in k order.  No atomics; the order of every sum is fixed by the indices alone.
#include "common.h"

namespace {

// sum over the 64 lanes of a wavefront, the same value in every lane: a butterfly whose order does not depend on anything but
// the lane numbers
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// One wavefront per 1/8-res cell n = (hc, wc); lane = fine position i*8 + j inside its 8x8 cell (as convex_upsample_kernel).
__global__ __launch_bounds__(256) void convex_upsample_bwd_part_kernel(
    const float* __restrict__ g_up, const float* __restrict__ mask, int ld_mask, const float* __restrict__ wlow, int hf, int wf,
    int crop_top, int crop_left, int h, int w, int do_sigmoid, float* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t pix = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pix >= (int64_t)hf * wf) return;                       // (a whole wavefront leaves: the shuffles below stay complete)
    const int hc = (int)(pix / wf), wc = (int)(pix - (int64_t)hc * wf);
    const float* m = mask + pix * ld_mask + lane;
    float e[9];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        e[k] = m[k * 64];
        mx = fmaxf(mx, e[k]);
    }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        e[k] = expf(e[k] - mx);
        den += e[k];
    }
    const int y = 8 * hc + (lane >> 3) - crop_top, x = 8 * wc + (lane & 7) - crop_left;
    const bool inside = y >= 0 && y < h && x >= 0 && x < w;
    float g = inside ? g_up[(int64_t)y * w + x] : 0.f;        // fine pixels outside the crop window send nothing
    if (do_sigmoid) {                                          // the forward's value, in its order of operations
        float aw = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int ny = hc + k / 3 - 1, nx = wc + k % 3 - 1;
            float vw = 0.f;
            if (ny >= 0 && ny < hf && nx >= 0 && nx < wf) vw = 8.f * wlow[(int64_t)ny * wf + nx];
            aw += (e[k] / den) * vw;
        }
        const float sg = sigmoidf_(aw / 8.f);
        g = inside ? g * (sg * (1.f - sg)) : 0.f;
    }
    const float g8 = g / 8.f;
    float mine = 0.f;                                          // lane k keeps sum k: one 36-byte store per cell
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float s = wave_sum(g8 * ((e[k] / den) * 8.f));
        mine = (lane == k) ? s : mine;
    }
    if (lane < 9) part[pix * 9 + lane] = mine;
}

// g_wlow[q] = sum_k part[q - d_k][k] in k order; a sender outside the map does not exist (the forward's zero padding).
__global__ void convex_upsample_bwd_sum_kernel(const float* __restrict__ part, int hf, int wf, float* __restrict__ g_wlow) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)hf * wf) return;
    const int qy = (int)(q / wf), qx = (int)(q - (int64_t)qy * wf);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int ny = qy - (k / 3 - 1), nx = qx - (k % 3 - 1);
        if (ny >= 0 && ny < hf && nx >= 0 && nx < wf) acc += part[((int64_t)ny * wf + nx) * 9 + k];
    }
    g_wlow[q] = acc;
}

bool bwd_map_ok(int hf, int wf) { return hf > 0 && wf > 0 && (int64_t)hf * wf < (1ll << 28); }

}  // namespace

extern "C" int64_t woft_convex_upsample_bwd_ws_bytes(int32_t hf, int32_t wf) {
    if (!bwd_map_ok(hf, wf)) return WOFT_EINVAL;
    return 9 * (int64_t)hf * wf * (int64_t)sizeof(float);
}

extern "C" int woft_convex_upsample_bwd(const float* g_up, const float* mask, int32_t ld_mask, const float* wlow, int32_t hf,
                                        int32_t wf, int32_t crop_top, int32_t crop_left, int32_t h, int32_t w,
                                        int32_t do_sigmoid, float* ws, float* g_wlow, void* stream) {
    if (!g_up || !mask || !ws || !g_wlow || !bwd_map_ok(hf, wf) || h <= 0 || w <= 0 || ld_mask < 576) return WOFT_EINVAL;
    if (crop_top < 0 || crop_left < 0 || crop_top + h > 8 * hf || crop_left + w > 8 * wf) return WOFT_EINVAL;
    if (do_sigmoid && !wlow) return WOFT_EINVAL;
    const int64_t n = (int64_t)hf * wf;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(convex_upsample_bwd_part_kernel, dim3((unsigned)ceil_div64(n, 4)), dim3(256), 0, s, g_up, mask, ld_mask,
                       wlow, hf, wf, crop_top, crop_left, h, w, do_sigmoid, ws);
    hipLaunchKernelGGL(convex_upsample_bwd_sum_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, s, (const float*)ws, hf,
                       wf, g_wlow);
    return woft_launch_status();
}
