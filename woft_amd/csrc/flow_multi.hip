// Multi-delta flow chaining: one candidate chain folded into a running per-pixel best (the combination step of a dense
// long-term tracker that chains flows over several temporal strides and keeps, per pixel, the most reliable chain).
// DESIGN.md section 18.  One streaming kernel with a local gather, one template pixel per lane: no LDS, no atomics, no workspace.
// Below it, the step from a fold result to the planar fit's correspondences (woft_chain_tc): streaming, no
// gather, the 130 integer counters of its histogram in LDS.
// Both have a form on rectangles (woft_flow_chain_fold_window, woft_chain_tc_window): flows on search windows;
// so has the multi-target form of the second (woft_chain_tc_multi_window).  Each piece of pixel work is
// written once: flow_chain_fold_kernel<FORM> for the fold's forms, CHAIN_TC_PIXEL for both histogram schemes of the
// second; fold_launch and outputs_alias hold what the entry points check alike.
//
// The sampler, its address rule and the launch geometry are those of flow_chain.hip (flow_sample.h): every tap address derives
// from a clamped float, so no input, finite or not, addresses outside a plane; the pixel's own planes are read at (x, y) of the
// launch geometry.
#include "flow_sample.h"

namespace {

// softplus(-l) = log(1 + exp(-l)) without overflow: for l < 0 it is -l + log(1 + exp(l))
__device__ __forceinline__ float softplus_neg(float l) { return l < 0.f ? -l + log1pf(expf(l)) : log1pf(expf(-l)); }

// The closing homography of the fold's POST form: nine host doubles passed by value (no device buffer, no workspace).
struct PostH {
    double h[9];
};

// The forms of the fold kernel.  FRAME (woft_flow_chain_fold): every plane is the [th][tw] frame, a pixel is
// its own coordinate; the instantiation carries no origin arithmetic and no fp64.  RECT (woft_flow_chain_fold_window, DESIGN.md
// section 26): the prev / best planes are the [th][tw] rectangle of the template with origin (tx0, ty0), the step planes the
// [sh][sw] rectangle with origin (sx0, sy0) of frames s and t; flows stay displacements in frame coordinates.  q is formed in frame
// coordinates, u = q - (step origin) is exact wherever the tap is valid, and the taps are those of u in the step planes: every
// address still derives from a float clamped into [0, sw-1] x [0, sh-1].  RECT_POST: the candidate's landing also goes through a
// homography in fp64 (den <= 0 or a non-finite image: invalid), one rounding back to the fp32 flow.
enum class Fold { FRAME, RECT, RECT_POST };

template <Fold FORM>
__global__ __launch_bounds__(FC_T) void flow_chain_fold_kernel(
    const float* __restrict__ prev_flow, const float* __restrict__ prev_cost, const float* __restrict__ prev_vis, int th, int tw, int ty0,
    int tx0, const float* __restrict__ step_flow, const float* __restrict__ step_wlogit, const float* __restrict__ step_mlogit, int sh,
    int sw, int sy0, int sx0, PostH H, float unit_cost, float vis_thr, int k, int first, float* __restrict__ best_flow,
    float* __restrict__ best_cost, float* __restrict__ best_vis, int32_t* __restrict__ best_sel) {
    constexpr bool RECT = FORM != Fold::FRAME;
    const int64_t plane = (int64_t)th * tw, splane = RECT ? (int64_t)sh * sw : plane;
    const int x = (int)blockIdx.x * FC_TX + (int)threadIdx.x;
    if (x >= tw) return;
    // the pixel in frame coordinates (px, py) and the step planes' origin; FRAME: the pixel's own (x, y), and no origin
    [[maybe_unused]] float px = (float)x, ox = 0.f, oy = 0.f;
    if constexpr (RECT) px = (float)(tx0 + x), ox = (float)sx0, oy = (float)sy0;
    for (int y = (int)blockIdx.y * FC_TY + (int)threadIdx.y; y < th; y += (int)gridDim.y * FC_TY) {
        const int64_t i = (int64_t)y * tw + x;
        // the stored result template -> s at this pixel (a null prev: s is the template itself)
        float pfx = 0.f, pfy = 0.f, pc = 0.f, pv = 1.f;
        if (prev_flow != nullptr) {
            pfx = prev_flow[i], pfy = prev_flow[plane + i];
            pc = prev_cost[i], pv = prev_vis[i];
        }
        float py = (float)y;
        if constexpr (RECT) py = (float)(ty0 + y);
        const float qx = px + pfx, qy = py + pfy;
        TapAt t;
        if constexpr (RECT)
            t = tap_at(sh, sw, qx - ox, qy - oy);
        else
            t = tap_at(th, tw, qx, qy);
        float fx = pfx + tap_plane(step_flow, t), fy = pfy + tap_plane(step_flow + splane, t);
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
        if constexpr (FORM == Fold::RECT_POST) {
            const double Px = (double)px, Py = (double)py;
            const double rx = Px + (double)fx, ry = Py + (double)fy;
            const double den = H.h[6] * rx + H.h[7] * ry + H.h[8];
            const double mx = (H.h[0] * rx + H.h[1] * ry + H.h[2]) / den, my = (H.h[3] * rx + H.h[4] * ry + H.h[5]) / den;
            ok = ok && den > 0.0 && isfinite(mx) && isfinite(my);                  // (a NaN fails)
            fx = (float)(mx - Px), fy = (float)(my - Py);
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

constexpr unsigned CHAIN_TC_BLOCKS = 2048;        // blocks of a launch with a histogram: 256 CUs x 8 blocks of 4 waves

// A fold result turned into what the planar fit reads: target coordinates, the fit weight exp(-cost), the
// 0/1 occlusion gate and the histogram of winning candidates under the template mask.  The fold's geometry: the pixel's (x, y)
// comes from the launch geometry and addresses everything; `sel` is the only input value used as an index, range-checked first,
// and it indexes the LDS counters alone.  A wave is one row segment (FC_TX = 64 lanes), so y and the loop's trip count are
// wave-uniform and every lane of a wave reaches the ballots below.
// WINDOW (woft_chain_tc_window): the planes are the rectangle with origin (tx0, ty0) of a frame_h x frame_w
// frame and tmask is the cropped mask; dst (window coordinates), w and hist are unchanged, ok is additionally 0 where the landing in
// FRAME coordinates fails the selection kernels' in-frame rule, so the planar stage needs no bounds check of its own.
//
// CHAIN_TC_PIXEL is the pixel work of both kernels below, in their names (flow .. ok, plane, x, y, gw, bin and WINDOW's arguments):
// pixel (x, y)'s reads, its dst, w and ok stores, and -- where COUNTED, the kernel's own test that a mask holds the pixel -- the
// counter it adds to, left in `bin`.  The counter is chosen by `seen`, not by the window's gate, so the histograms -- and the
// ballots and LDS atomics that build them -- see the same lanes and values in both instantiations.  It is text, not a __device__
// function: through an inlined function (with or without __restrict__, returning the counter, a struct, or taking the test as a
// callable) this compiler schedules all four kernels differently and spends 2 to 3 more VGPRs on each; as text three of them keep
// their instruction streams and chain_tc_kernel<true> keeps its instruction count on fewer registers.
#define CHAIN_TC_PIXEL(COUNTED)                                                                                                    \
    const int64_t i = (int64_t)y * gw + x;                                                                                         \
    const float fx = flow[i], fy = flow[plane + i], c = cost[i], v = vis[i];                                                       \
    const int32_t s = sel[i];                                                                                                      \
    const bool valid = s >= 0 && s < WOFT_CHAIN_HIST - 2 && isfinite(fx) && isfinite(fy) && isfinite(c) && isfinite(v);            \
    const bool seen = valid && !(v < vis_thr); /* the fold's occlusion rule */                                                     \
    dst[i] = valid ? (float)x + fx : NAN;                                                                                          \
    dst[plane + i] = valid ? (float)y + fy : NAN;                                                                                  \
    if (w != nullptr) w[i] = valid ? expf(-c) : 0.f;                                                                               \
    bool gate = seen;                                                                                                              \
    if constexpr (WINDOW) {                                                                                                        \
        const float X = (float)(tx0 + x) + fx, Y = (float)(ty0 + y) + fy;                                                          \
        gate = seen && !(X < 0.f || Y < 0.f || rintf(X) >= frame_w || rintf(Y) >= frame_h);                                        \
    }                                                                                                                              \
    ok[i] = gate ? 1.f : 0.f;                                                                                                      \
    if (COUNTED) bin = !valid ? WOFT_CHAIN_HIST - 2 : (seen ? s : WOFT_CHAIN_HIST - 1)

template <bool WINDOW>
__global__ __launch_bounds__(FC_T) void chain_tc_kernel(const float* __restrict__ flow, const float* __restrict__ cost,
                                                        const float* __restrict__ vis, const int32_t* __restrict__ sel,
                                                        const uint8_t* __restrict__ tmask, int gh, int gw, int mw, int ty0, int tx0,
                                                        float frame_h, float frame_w, float vis_thr, float* __restrict__ dst,
                                                        float* __restrict__ w, float* __restrict__ ok, int32_t* __restrict__ hist) {
    __shared__ int32_t bins[WOFT_CHAIN_HIST];
    const int tid = (int)threadIdx.y * FC_TX + (int)threadIdx.x;
    if (hist != nullptr) {
        if (tid < WOFT_CHAIN_HIST) bins[tid] = 0;
        __syncthreads();
    }
    const int64_t plane = (int64_t)gh * gw;
    const int x = (int)blockIdx.x * FC_TX + (int)threadIdx.x;
    const bool in = x < gw;
    for (int y = (int)blockIdx.y * FC_TY + (int)threadIdx.y; y < gh; y += (int)gridDim.y * FC_TY) {
        int bin = -1;                                 // the counter this lane adds to (-1: none)
        if (in) {
            CHAIN_TC_PIXEL(hist != nullptr && (tmask == nullptr || tmask[(int64_t)y * mw + x] != 0));
        }
        if (hist != nullptr) {
            // one LDS add per distinct counter of the wave (a frame's pixels mostly agree on it), by the first lane that holds it
            uint64_t todo = __ballot(bin >= 0);
            while (todo != 0) {
                const int lead = __ffsll((unsigned long long)todo) - 1;
                const int b = __shfl(bin, lead);
                const uint64_t same = __ballot(bin == b);
                if ((int)threadIdx.x == lead) atomicAdd(&bins[b], (int32_t)__popcll(same));
                todo &= ~same;
            }
        }
    }
    if (hist != nullptr) {
        __syncthreads();
        if (tid < WOFT_CHAIN_HIST && bins[tid] != 0) atomicAdd(&hist[tid], bins[tid]);
    }
}

// chain_tc_kernel for n_targets masks held as one bit plane: CHAIN_TC_PIXEL's work, so the same dst, w, ok;
// the pixel's counter is the same for every target, its mask bits say which targets count it.  Per distinct counter of the wave,
// one ballot per target gives that target's number of lanes; lane t keeps target t's, so the wave ends in ONE LDS atomic
// instruction per distinct counter (lanes 0 .. n_targets-1, one counter each).  LDS: n_targets * 130 counters, 16 640 B at 32.
// WINDOW (woft_chain_tc_multi_window): the planes are the rectangle with origin (tx0, ty0) and tbits is the
// cropped bit plane.
template <bool WINDOW>
__global__ __launch_bounds__(FC_T) void chain_tc_multi_kernel(const float* __restrict__ flow, const float* __restrict__ cost,
                                                              const float* __restrict__ vis, const int32_t* __restrict__ sel,
                                                              const uint32_t* __restrict__ tbits, int gh, int gw, int mw,
                                                              int n_targets, int ty0, int tx0, float frame_h, float frame_w,
                                                              float vis_thr, float* __restrict__ dst, float* __restrict__ w,
                                                              float* __restrict__ ok, int32_t* __restrict__ hist) {
    __shared__ int32_t bins[WOFT_MULTI_MAX_TARGETS * WOFT_CHAIN_HIST];
    const int tid = (int)threadIdx.y * FC_TX + (int)threadIdx.x;
    const int n_bins = n_targets * WOFT_CHAIN_HIST;
    for (int k = tid; k < n_bins; k += FC_T) bins[k] = 0;
    __syncthreads();
    const uint32_t live = n_targets >= 32 ? 0xffffffffu : ((1u << n_targets) - 1u);
    const int64_t plane = (int64_t)gh * gw;
    const int x = (int)blockIdx.x * FC_TX + (int)threadIdx.x;
    const bool in = x < gw;
    for (int y = (int)blockIdx.y * FC_TY + (int)threadIdx.y; y < gh; y += (int)gridDim.y * FC_TY) {
        int bin = -1;                                 // the counter this lane adds to (-1: none)
        uint32_t bits = 0;                            // the targets whose mask holds this pixel
        if (in) {
            CHAIN_TC_PIXEL((bits = tbits[(int64_t)y * mw + x] & live) != 0);
        }
        uint64_t todo = __ballot(bin >= 0);
        while (todo != 0) {
            const int lead = __ffsll((unsigned long long)todo) - 1;
            const int b = __shfl(bin, lead);
            const bool here = bin == b;
            int mine = 0;
            for (int t = 0; t < n_targets; ++t) {
                const uint64_t m = __ballot(here && ((bits >> t) & 1u));
                if ((int)threadIdx.x == t) mine = (int)__popcll(m);
            }
            if (mine != 0) atomicAdd(&bins[(int)threadIdx.x * WOFT_CHAIN_HIST + b], mine);   // (mine != 0 only for lanes < n_targets)
            todo &= ~__ballot(here);
        }
    }
    __syncthreads();
    for (int k = tid; k < n_bins; k += FC_T)
        if (bins[k] != 0) atomicAdd(&hist[k], bins[k]);
}

// [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uint64_t pa = (uint64_t)(uintptr_t)a, pb = (uint64_t)(uintptr_t)b;
    return a != nullptr && b != nullptr && pa < pb + nb && pb < pa + na;
}

// The overlap rule of every entry point below: a pixel's outputs are written while other pixels' inputs are still unread (the fold
// even gathers them), so no output (outs[a], nout[a] bytes) may share a byte with an input (ins[b], nin[b] bytes) or with another
// output; a NULL passes.
template <int N_OUT, int N_IN>
bool outputs_alias(const void* const (&outs)[N_OUT], const uint64_t (&nout)[N_OUT], const void* const (&ins)[N_IN],
                   const uint64_t (&nin)[N_IN]) {
    for (int a = 0; a < N_OUT; ++a) {
        for (int b = 0; b < N_IN; ++b)
            if (overlap(outs[a], nout[a], ins[b], nin[b])) return true;
        for (int b = a + 1; b < N_OUT; ++b)
            if (overlap(outs[a], nout[a], outs[b], nout[b])) return true;
    }
    return false;
}

// a rectangle's origin and side on one axis: origin >= 0, side >= 1, origin + side <= 2^24 (every coordinate is exact in fp32)
inline bool bad_span(int32_t origin, int32_t side) { return origin < 0 || side <= 0 || (int64_t)origin + side > FC_MAX_SIDE; }

// What woft_flow_chain_fold and woft_flow_chain_fold_window check alike -- the pointers, the prev triple, the constants, the overlap
// rule (each plane with its own size) -- and the launch of the form's instantiation; the sides and spans are the caller's.
int fold_launch(Fold form, const float* prev_flow, const float* prev_cost, const float* prev_vis, int32_t th, int32_t tw, int32_t ty0,
                int32_t tx0, const float* step_flow, const float* step_wlogit, const float* step_mlogit, int32_t sh, int32_t sw,
                int32_t sy0, int32_t sx0, const PostH& H, float unit_cost, float vis_thr, int32_t k, int32_t first, float* best_flow,
                float* best_cost, float* best_vis, int32_t* best_sel, void* stream) {
    if (!step_flow || !best_flow || !best_cost || !best_vis || !best_sel) return WOFT_EINVAL;
    const int n_prev = (prev_flow != nullptr) + (prev_cost != nullptr) + (prev_vis != nullptr);
    if (n_prev != 0 && n_prev != 3) return WOFT_EINVAL;
    if (!(unit_cost >= 0.f) || !(vis_thr >= 0.f && vis_thr <= 1.f) || k < 0 || k > 127) return WOFT_EINVAL;    // (NaN fails)
    const uint64_t tb = (uint64_t)th * (uint64_t)tw * 4u, sb = (uint64_t)sh * (uint64_t)sw * 4u;
    const void* const outs[4] = {best_flow, best_cost, best_vis, best_sel};
    const uint64_t nout[4] = {2 * tb, tb, tb, tb};
    const void* const ins[6] = {prev_flow, prev_cost, prev_vis, step_flow, step_wlogit, step_mlogit};
    const uint64_t nin[6] = {2 * tb, tb, tb, 2 * sb, sb, sb};
    if (outputs_alias(outs, nout, ins, nin)) return WOFT_EINVAL;
    // three instantiations: whole frames carry no origin arithmetic, and only a closing homography carries fp64 code
    auto kernel = form == Fold::FRAME ? flow_chain_fold_kernel<Fold::FRAME>
                                      : (form == Fold::RECT ? flow_chain_fold_kernel<Fold::RECT> : flow_chain_fold_kernel<Fold::RECT_POST>);
    hipLaunchKernelGGL(kernel, pixel_grid(th, tw), dim3(FC_TX, FC_TY), 0, (hipStream_t)stream, prev_flow, prev_cost, prev_vis, th, tw,
                       ty0, tx0, step_flow, step_wlogit, step_mlogit, sh, sw, sy0, sx0, H, unit_cost, vis_thr, k, first != 0, best_flow,
                       best_cost, best_vis, best_sel);
    return woft_launch_status();
}

}  // namespace

extern "C" int woft_flow_chain_fold(const float* prev_flow, const float* prev_cost, const float* prev_vis, const float* step_flow,
                                    const float* step_wlogit, const float* step_mlogit, int32_t h, int32_t w, float unit_cost,
                                    float vis_thr, int32_t k, int32_t first, float* best_flow, float* best_cost, float* best_vis,
                                    int32_t* best_sel, void* stream) {
    if (bad_side(h, w)) return WOFT_EINVAL;
    return fold_launch(Fold::FRAME, prev_flow, prev_cost, prev_vis, h, w, 0, 0, step_flow, step_wlogit, step_mlogit, h, w, 0, 0, PostH{},
                       unit_cost, vis_thr, k, first, best_flow, best_cost, best_vis, best_sel, stream);
}

namespace {

// the checks and the launch of woft_chain_tc and woft_chain_tc_window (WINDOW: the rectangle's origin and the frame's size)
template <bool WINDOW>
int chain_tc_launch(const float* flow, const float* cost, const float* vis, const int32_t* sel, const uint8_t* tmask, int32_t gh,
                    int32_t gw, int32_t mh, int32_t mw, int32_t ty0, int32_t tx0, int32_t frame_h, int32_t frame_w, float vis_thr,
                    float* dst, float* w, float* ok, int32_t* hist, void* stream) {
    if (!flow || !cost || !vis || !sel || !dst || !ok || bad_side(gh, gw)) return WOFT_EINVAL;
    if (WINDOW && (bad_span(ty0, gh) || bad_span(tx0, gw) || bad_side(frame_h, frame_w))) return WOFT_EINVAL;
    if (tmask != nullptr && (mh < gh || mw < gw)) return WOFT_EINVAL;
    if (!(vis_thr >= 0.f && vis_thr <= 1.f)) return WOFT_EINVAL;                                                  // (NaN fails)
    const uint64_t pb = (uint64_t)gh * (uint64_t)gw * 4u;
    const void* const outs[4] = {dst, w, ok, hist};
    const uint64_t nout[4] = {2 * pb, pb, pb, WOFT_CHAIN_HIST * sizeof(int32_t)};
    const void* const ins[5] = {flow, cost, vis, sel, tmask};
    const uint64_t nin[5] = {2 * pb, pb, pb, pb, tmask ? (uint64_t)mh * (uint64_t)mw : 0u};
    if (outputs_alias(outs, nout, ins, nin)) return WOFT_EINVAL;
    if (hist != nullptr && hipMemsetAsync(hist, 0, WOFT_CHAIN_HIST * sizeof(int32_t), (hipStream_t)stream) != hipSuccess)
        return WOFT_ELAUNCH;
    // With a histogram every block ends in a few atomics on the same handful of counters, and those serialise: one block per
    // 64 x 4 tile (8 100 at 1080p) spent more time there than streaming.  So the grid is cut to about one resident set of blocks
    // and the row loop does the rest: same tiles, same addresses, a quarter of the atomics at 1080p.
    dim3 grid = pixel_grid(gh, gw);
    if (hist != nullptr) {
        const unsigned rows = CHAIN_TC_BLOCKS / grid.x;
        grid.y = grid.y < rows ? grid.y : (rows > 0 ? rows : 1u);
    }
    hipLaunchKernelGGL(chain_tc_kernel<WINDOW>, grid, dim3(FC_TX, FC_TY), 0, (hipStream_t)stream, flow, cost, vis, sel, tmask, gh, gw,
                       tmask ? mw : gw, ty0, tx0, (float)frame_h, (float)frame_w, vis_thr, dst, w, ok, hist);
    return woft_launch_status();
}

}  // namespace

extern "C" int woft_chain_tc(const float* flow, const float* cost, const float* vis, const int32_t* sel, const uint8_t* tmask,
                             int32_t gh, int32_t gw, int32_t mh, int32_t mw, float vis_thr, float* dst, float* w, float* ok,
                             int32_t* hist, void* stream) {
    return chain_tc_launch<false>(flow, cost, vis, sel, tmask, gh, gw, mh, mw, 0, 0, 0, 0, vis_thr, dst, w, ok, hist, stream);
}

extern "C" int woft_chain_tc_window(const float* flow, const float* cost, const float* vis, const int32_t* sel, const uint8_t* tmask,
                                    int32_t gh, int32_t gw, int32_t mh, int32_t mw, int32_t ty0, int32_t tx0, int32_t frame_h,
                                    int32_t frame_w, float vis_thr, float* dst, float* w, float* ok, int32_t* hist, void* stream) {
    return chain_tc_launch<true>(flow, cost, vis, sel, tmask, gh, gw, mh, mw, ty0, tx0, frame_h, frame_w, vis_thr, dst, w, ok, hist,
                                 stream);
}

namespace {

// the checks and the launch of woft_chain_tc_multi and woft_chain_tc_multi_window (WINDOW: the rectangle's origin and the frame's size)
template <bool WINDOW>
int chain_tc_multi_launch(const float* flow, const float* cost, const float* vis, const int32_t* sel, const uint32_t* tbits, int32_t gh,
                          int32_t gw, int32_t mh, int32_t mw, int32_t n_targets, int32_t ty0, int32_t tx0, int32_t frame_h,
                          int32_t frame_w, float vis_thr, float* dst, float* w, float* ok, int32_t* hist, void* stream) {
    if (!flow || !cost || !vis || !sel || !tbits || !dst || !ok || !hist || bad_side(gh, gw)) return WOFT_EINVAL;
    if (WINDOW && (bad_span(ty0, gh) || bad_span(tx0, gw) || bad_side(frame_h, frame_w))) return WOFT_EINVAL;
    if (mh < gh || mw < gw || n_targets < 1 || n_targets > WOFT_MULTI_MAX_TARGETS) return WOFT_EINVAL;
    if (!(vis_thr >= 0.f && vis_thr <= 1.f)) return WOFT_EINVAL;                                                  // (NaN fails)
    const uint64_t pb = (uint64_t)gh * (uint64_t)gw * 4u;
    const uint64_t hist_bytes = (uint64_t)n_targets * WOFT_CHAIN_HIST * sizeof(int32_t);
    const void* const outs[4] = {dst, w, ok, hist};
    const uint64_t nout[4] = {2 * pb, pb, pb, hist_bytes};
    const void* const ins[5] = {flow, cost, vis, sel, tbits};
    const uint64_t nin[5] = {2 * pb, pb, pb, pb, (uint64_t)mh * (uint64_t)mw * 4u};
    if (outputs_alias(outs, nout, ins, nin)) return WOFT_EINVAL;
    if (hipMemsetAsync(hist, 0, hist_bytes, (hipStream_t)stream) != hipSuccess) return WOFT_ELAUNCH;
    // the grid of woft_chain_tc with a histogram: about one resident set of blocks, the row loop does the rest
    dim3 grid = pixel_grid(gh, gw);
    const unsigned rows = CHAIN_TC_BLOCKS / grid.x;
    grid.y = grid.y < rows ? grid.y : (rows > 0 ? rows : 1u);
    hipLaunchKernelGGL(chain_tc_multi_kernel<WINDOW>, grid, dim3(FC_TX, FC_TY), 0, (hipStream_t)stream, flow, cost, vis, sel, tbits, gh,
                       gw, mw, n_targets, ty0, tx0, (float)frame_h, (float)frame_w, vis_thr, dst, w, ok, hist);
    return woft_launch_status();
}

}  // namespace

extern "C" int woft_chain_tc_multi(const float* flow, const float* cost, const float* vis, const int32_t* sel, const uint32_t* tbits,
                                   int32_t gh, int32_t gw, int32_t mh, int32_t mw, int32_t n_targets, float vis_thr, float* dst,
                                   float* w, float* ok, int32_t* hist, void* stream) {
    return chain_tc_multi_launch<false>(flow, cost, vis, sel, tbits, gh, gw, mh, mw, n_targets, 0, 0, 0, 0, vis_thr, dst, w, ok, hist,
                                        stream);
}

extern "C" int woft_chain_tc_multi_window(const float* flow, const float* cost, const float* vis, const int32_t* sel,
                                          const uint32_t* tbits, int32_t gh, int32_t gw, int32_t mh, int32_t mw, int32_t n_targets,
                                          int32_t ty0, int32_t tx0, int32_t frame_h, int32_t frame_w, float vis_thr, float* dst,
                                          float* w, float* ok, int32_t* hist, void* stream) {
    return chain_tc_multi_launch<true>(flow, cost, vis, sel, tbits, gh, gw, mh, mw, n_targets, ty0, tx0, frame_h, frame_w, vis_thr, dst,
                                       w, ok, hist, stream);
}

extern "C" int woft_flow_chain_fold_window(const float* prev_flow, const float* prev_cost, const float* prev_vis, int32_t th, int32_t tw,
                                           int32_t ty0, int32_t tx0, const float* step_flow, const float* step_wlogit,
                                           const float* step_mlogit, int32_t sh, int32_t sw, int32_t sy0, int32_t sx0,
                                           const double* post_H, float unit_cost, float vis_thr, int32_t k, int32_t first,
                                           float* best_flow, float* best_cost, float* best_vis, int32_t* best_sel, void* stream) {
    if (bad_span(ty0, th) || bad_span(tx0, tw) || bad_span(sy0, sh) || bad_span(sx0, sw)) return WOFT_EINVAL;
    PostH H = {};
    if (post_H != nullptr) {
        for (int j = 0; j < 9; ++j) {
            if (!std::isfinite(post_H[j])) return WOFT_EINVAL;
            H.h[j] = post_H[j];
        }
        if (post_H[8] != 1.0) return WOFT_EINVAL;
    }
    // (the chained candidates, with no post_H, carry no fp64 code)
    return fold_launch(post_H != nullptr ? Fold::RECT_POST : Fold::RECT, prev_flow, prev_cost, prev_vis, th, tw, ty0, tx0, step_flow,
                       step_wlogit, step_mlogit, sh, sw, sy0, sx0, H, unit_cost, vis_thr, k, first, best_flow, best_cost, best_vis,
                       best_sel, stream);
}
