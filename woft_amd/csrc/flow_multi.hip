// Multi-delta flow chaining: one candidate chain folded into a running per-pixel best (the combination step of a dense
// long-term tracker that chains flows over several temporal strides and keeps, per pixel, the most reliable chain).
// DESIGN.md section 18.  One streaming kernel with a local gather, one template pixel per lane: no LDS, no atomics, no workspace.
//
// The sampler, its address rule and the launch geometry are those of flow_chain.hip (flow_sample.h): every tap address derives
// from a clamped float, so no input, finite or not, addresses outside a plane; the pixel's own planes are read at (x, y) of the
// launch geometry.
#include "flow_sample.h"

namespace {

// softplus(-l) = log(1 + exp(-l)) without overflow: for l < 0 it is -l + log(1 + exp(l))
__device__ __forceinline__ float softplus_neg(float l) { return l < 0.f ? -l + log1pf(expf(l)) : log1pf(expf(-l)); }

__global__ __launch_bounds__(FC_T) void flow_chain_fold_kernel(const float* __restrict__ prev_flow, const float* __restrict__ prev_cost,
                                                               const float* __restrict__ prev_vis, const float* __restrict__ step_flow,
                                                               const float* __restrict__ step_wlogit,
                                                               const float* __restrict__ step_mlogit, int h, int w, float unit_cost,
                                                               float vis_thr, int k, int first, float* __restrict__ best_flow,
                                                               float* __restrict__ best_cost, float* __restrict__ best_vis,
                                                               int32_t* __restrict__ best_sel) {
    const int64_t plane = (int64_t)h * w;
    const int x = (int)blockIdx.x * FC_TX + (int)threadIdx.x;
    if (x >= w) return;
    for (int y = (int)blockIdx.y * FC_TY + (int)threadIdx.y; y < h; y += (int)gridDim.y * FC_TY) {
        const int64_t i = (int64_t)y * w + x;
        // the stored result template -> s at this pixel (a null prev: s is the template itself)
        float pfx = 0.f, pfy = 0.f, pc = 0.f, pv = 1.f;
        if (prev_flow != nullptr) {
            pfx = prev_flow[i], pfy = prev_flow[plane + i];
            pc = prev_cost[i], pv = prev_vis[i];
        }
        const float qx = (float)x + pfx, qy = (float)y + pfy;
        const TapAt t = tap_at(h, w, qx, qy);
        const float fx = pfx + tap_plane(step_flow, t), fy = pfy + tap_plane(step_flow + plane, t);
        // the logits are interpolated, then converted; a non-finite interpolated logit makes the candidate invalid
        bool ok = t.valid;
        float cost = pc + unit_cost, vis = pv;
        if (step_wlogit != nullptr) {
            const float l = tap_plane(step_wlogit, t);
            ok = ok && isfinite(l);
            cost = pc + softplus_neg(l);
        }
        if (step_mlogit != nullptr) {
            const float m = tap_plane(step_mlogit, t);
            ok = ok && isfinite(m);
            vis = pv * sigmoidf_(m);
        }
        ok = ok && isfinite(fx) && isfinite(fy) && isfinite(cost) && isfinite(vis);
        // key (occluded, cost), lexicographic; an equal key keeps the earlier fold
        bool replace = ok;
        if (ok && !first && best_sel[i] >= 0) {
            const float bc = best_cost[i];
            const bool bocc = best_vis[i] < vis_thr, occ = vis < vis_thr;
            replace = (bocc && !occ) || (bocc == occ && cost < bc);
        }
        if (replace) {
            best_flow[i] = fx, best_flow[plane + i] = fy;
            best_cost[i] = cost, best_vis[i] = vis, best_sel[i] = k;
        } else if (first) {
            best_flow[i] = NAN, best_flow[plane + i] = NAN;
            best_cost[i] = INFINITY, best_vis[i] = 0.f, best_sel[i] = -1;
        }
    }
}

// [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uint64_t pa = (uint64_t)(uintptr_t)a, pb = (uint64_t)(uintptr_t)b;
    return a != nullptr && b != nullptr && pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" int woft_flow_chain_fold(const float* prev_flow, const float* prev_cost, const float* prev_vis, const float* step_flow,
                                    const float* step_wlogit, const float* step_mlogit, int32_t h, int32_t w, float unit_cost,
                                    float vis_thr, int32_t k, int32_t first, float* best_flow, float* best_cost, float* best_vis,
                                    int32_t* best_sel, void* stream) {
    if (!step_flow || !best_flow || !best_cost || !best_vis || !best_sel || bad_side(h, w)) return WOFT_EINVAL;
    const int n_prev = (prev_flow != nullptr) + (prev_cost != nullptr) + (prev_vis != nullptr);
    if (n_prev != 0 && n_prev != 3) return WOFT_EINVAL;
    if (!(unit_cost >= 0.f) || !(vis_thr >= 0.f && vis_thr <= 1.f) || k < 0 || k > 127) return WOFT_EINVAL;    // (NaN fails)
    // the running best is written while the inputs are still being gathered: it may share no byte with an input or with itself
    const uint64_t pb = (uint64_t)h * (uint64_t)w * 4u;
    const void* outs[4] = {best_flow, best_cost, best_vis, best_sel};
    const void* ins[6] = {prev_flow, prev_cost, prev_vis, step_flow, step_wlogit, step_mlogit};
    for (int a = 0; a < 4; ++a) {
        const uint64_t na = a == 0 ? 2 * pb : pb;
        for (int b = 0; b < 6; ++b)
            if (overlap(outs[a], na, ins[b], (b == 0 || b == 3) ? 2 * pb : pb)) return WOFT_EINVAL;
        for (int b = a + 1; b < 4; ++b)
            if (overlap(outs[a], na, outs[b], pb)) return WOFT_EINVAL;
    }
    hipLaunchKernelGGL(flow_chain_fold_kernel, pixel_grid(h, w), dim3(FC_TX, FC_TY), 0, (hipStream_t)stream, prev_flow, prev_cost,
                       prev_vis, step_flow, step_wlogit, step_mlogit, h, w, unit_cost, vis_thr, k, first != 0, best_flow, best_cost,
                       best_vis, best_sel);
    return woft_launch_status();
}
