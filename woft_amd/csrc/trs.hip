// RANSAC similarity (translation, rotation, scale) estimator: what cv2.estimateAffinePartial2D(src, dst, method=cv2.RANSAC,
// ransacReprojThreshold, maxIters, confidence) does in utils/least_squares_H.py:349-363 (`find_homography_TRS`), restated from
// OpenCV's published behaviour -- OpenCV's source is not pinned here ("TRS").
//
// Semantics (the host restatement tests/trs_host.py follows them step for step):
//   * n < 2: status 1 (the Python entry raises AssertionError before any launch).
//   * n == 2: the direct two-point model; no sampling, no refit.
//   * hypothesis k = 0 .. max_iters-1: two distinct indices from the stream of ransac.hip, draw c of hypothesis k being
//       u = splitmix64(splitmix64(seed) ^ ((k << 32) | c)),   index = ((u >> 32) * n) >> 32,
//     c counting every draw (a duplicate index is drawn again with the next c).  cv2 applies no subset check to two points, so
//     every hypothesis has a sample.
//   * model, fp64, points as complex numbers: q = (B1 - B0) conj(A1 - A0) / |A1 - A0|^2, t = B0 - q A0,
//     H = [[Re q, -Im q, Re t], [Im q, Re q, Im t], [0, 0, 1]].  |A1 - A0|^2 == 0 (or a non-finite model) is degenerate: score 0.
//   * score: #{i : err_i <= thr^2} with cv2's fp32 error dx = h0 x + h1 y + h2 - X, dy = h3 x + h4 y + h5 - Y,
//     err = dx^2 + dy^2, the model cast to fp32 first (thr^2 rounded to fp32 once).
//   * selection = cv2's sequential loop with two model points: a new best needs count > max(best, 1); after it,
//     niters = RANSACUpdateNumIters(conf, (n - count) / n, 2, niters); the loop ends at the first k >= niters.
//   * refit (refine != 0 and more than 2 inliers): the closed-form least-squares similarity over the inliers of the best
//     hypothesis, fp64: centroids abar, bbar, q = sum (b_i - bbar) conj(a_i - abar) / sum |a_i - abar|^2, t = bbar - q abar --
//     the optimum of the linear objective cv2's 10 Levenberg-Marquardt iterations descend.  Inliers whose A all coincide
//     (sum |a_i - abar|^2 == 0) keep the two-point model.
//   * no model (no hypothesis with >= 2 inliers): H all NaN, status 2, best k -1.
//
// Launches (fixed count, no host synchronisation, every hand-off at a kernel boundary):
//   score  (hypothesis block x point chunk workgroups, the chunk's points staged in LDS; partial counts by integer atomicAdd
//           when there is more than one chunk: exact, so deterministic)
//   ->  select (one workgroup: ransac_common.h's rebuild of the sequential loop, then the best model)
//   ->  final  (one workgroup: inlier mask, refit with a fixed-order fp64 reduction, outputs).
#include "ransac_common.h"
#include <algorithm>

namespace {

constexpr int TT = 256;             // threads of a scoring workgroup: 64 hypotheses x 4 point slices (one wave per slice)
constexpr int TH = 64;              // hypotheses per scoring workgroup
constexpr int TCHUNK = 2048;        // points per scoring workgroup (gridDim.y = ceil(n_max / TCHUNK)); 32 KiB of LDS
constexpr int FINT = 1024;          // threads of the final workgroup

struct TState {                     // in the workspace, written by the select kernel, read by final
    int status, best_k, n_inl, iters;
    double m[4];                    // best model: Re q, Im q, Re t, Im t
};

struct TWs {
    int* counts;
    TState* st;
};

inline TWs ws_layout(void* ws, int max_iters) {
    TWs o;
    char* p = (char*)ws;
    o.counts = (int*)p;
    p += align256((int64_t)max_iters * 4);
    o.st = (TState*)p;
    return o;
}

// the two distinct indices of hypothesis k
__device__ __forceinline__ void draw_pair(uint64_t key, int k, int n, int& i0, int& i1) {
    uint32_t c = 0;
    i0 = draw_index(key, k, c++, n);
    do {
        i1 = draw_index(key, k, c++, n);
    } while (i1 == i0);
}

// two-point similarity (a0, a1) -> (b0, b1), fp64 -> m = {Re q, Im q, Re t, Im t}; false when degenerate
__device__ __forceinline__ bool model2(float2 a0, float2 a1, float2 b0, float2 b1, double (&m)[4]) {
    const double dax = (double)a1.x - (double)a0.x, day = (double)a1.y - (double)a0.y;
    const double dbx = (double)b1.x - (double)b0.x, dby = (double)b1.y - (double)b0.y;
    const double den = dax * dax + day * day;
    if (den == 0.0) return false;
    const double qr = (dbx * dax + dby * day) / den, qi = (dby * dax - dbx * day) / den;
    m[0] = qr;
    m[1] = qi;
    m[2] = (double)b0.x - (qr * (double)a0.x - qi * (double)a0.y);
    m[3] = (double)b0.y - (qi * (double)a0.x + qr * (double)a0.y);
    return isfinite(m[0]) && isfinite(m[1]) && isfinite(m[2]) && isfinite(m[3]);
}

struct ModelF {                     // the model as cv2 scores it: fp32, rows (h0 h1 h2) (h3 h4 h5)
    float h0, h1, h2, h3, h4, h5;
};

__device__ __forceinline__ ModelF to_f32(const double (&m)[4]) {
    const float qr = (float)m[0], qi = (float)m[1];
    return {qr, -qi, (float)m[2], qi, qr, (float)m[3]};
}

__device__ __forceinline__ float reproj_err(const ModelF& h, float ax, float ay, float bx, float by) {
    const float dx = h.h0 * ax + h.h1 * ay + h.h2 - bx;
    const float dy = h.h3 * ax + h.h4 * ay + h.h5 - by;
    return dx * dx + dy * dy;
}

// counts[k] = inliers of hypothesis k (0: degenerate model)
__global__ __launch_bounds__(TT) void trs_score_kernel(const float2* __restrict__ pa, const float2* __restrict__ pb, int n_max,
                                                       const int* __restrict__ count, int max_iters, uint64_t key, float thr2,
                                                       int multi, int* __restrict__ counts) {
    __shared__ float4 pts[TCHUNK];                          // (ax, ay, bx, by) of this chunk: every lane of a wave reads one entry
    __shared__ int part[4][TH];
    const int n = fit_n(count, n_max);
    const int64_t p0 = (int64_t)blockIdx.y * TCHUNK;
    if (n <= 2 || p0 >= n) return;                          // (workgroup-uniform)
    const int np = (int)min((int64_t)TCHUNK, (int64_t)n - p0);
    for (int i = threadIdx.x; i < np; i += TT) {
        const float2 a = pa[p0 + i], b = pb[p0 + i];
        pts[i] = make_float4(a.x, a.y, b.x, b.y);
    }
    const int hl = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int k = blockIdx.x * TH + hl;
    bool ok = false;
    ModelF h = {};
    if (k < max_iters) {
        int i0, i1;
        draw_pair(key, k, n, i0, i1);
        double m[4];
        ok = model2(pa[i0], pa[i1], pb[i0], pb[i1], m);
        if (ok) h = to_f32(m);
    }
    __syncthreads();
    int cnt = 0;
    if (ok)
        for (int i = slice; i < np; i += 4) {
            const float4 p = pts[i];
            cnt += reproj_err(h, p.x, p.y, p.z, p.w) <= thr2;
        }
    part[slice][hl] = cnt;
    __syncthreads();
    if (slice != 0 || k >= max_iters) return;
    const int tot = part[0][hl] + part[1][hl] + part[2][hl] + part[3][hl];
    if (!multi) {
        counts[k] = tot;
    } else if (tot != 0) {
        atomicAdd(&counts[k], tot);
    }
}

// one workgroup: the sequential loop's stop, best hypothesis and model, from counts[]
__global__ __launch_bounds__(SELT) void trs_select_kernel(const float2* __restrict__ pa, const float2* __restrict__ pb, int n_max,
                                                          const int* __restrict__ count, int max_iters, uint64_t key, double conf,
                                                          const int* __restrict__ counts, TState* __restrict__ st) {
    const int n = fit_n(count, n_max);
    const int tid = threadIdx.x;
    if (n < 2) {
        if (tid == 0) { st->status = 1; st->best_k = -1; st->n_inl = 0; st->iters = 0; }
        return;
    }
    if (n == 2) {
        if (tid == 0) {
            double m[4] = {0.0, 0.0, 0.0, 0.0};
            const bool ok = model2(pa[0], pa[1], pb[0], pb[1], m);
            for (int i = 0; i < 4; ++i) st->m[i] = m[i];
            st->status = ok ? 0 : 2; st->best_k = ok ? 0 : -1; st->n_inl = ok ? 2 : 0; st->iters = 0;
        }
        return;
    }
    int S, best;
    sequential_select<2>(counts, max_iters, conf, n, S, best);
    if (tid == 0) {
        st->iters = S;
        st->best_k = best;
        if (best < 0) {
            st->status = 2; st->n_inl = 0;
            return;
        }
        int i0, i1;
        draw_pair(key, best, n, i0, i1);
        double m[4];
        model2(pa[i0], pa[i1], pb[i0], pb[i1], m);
        for (int i = 0; i < 4; ++i) st->m[i] = m[i];
        st->n_inl = counts[best];
        st->status = 0;
    }
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sums of NV per-lane fp64 values over the workgroup, in a fixed order (lanes by xor shuffle, waves in sequence) -> out[NV] (LDS)
template <int NV>
__device__ void block_sum_d(const double (&v)[NV], double* red /* [FINT / 64][NV] */, double* out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < NV; ++t) {
        const double s = wave_sum_d(v[t]);
        if (lane == 0) red[wave * NV + t] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < NV) {
        double s = 0.0;
        for (int wv = 0; wv < FINT / 64; ++wv) s += red[wv * NV + threadIdx.x];
        out[threadIdx.x] = s;
    }
    __syncthreads();
}

// one workgroup: inlier mask of the best model, closed-form refit over it (refine, more than 2 inliers) and the outputs
__global__ __launch_bounds__(FINT) void trs_final_kernel(const float2* __restrict__ pa, const float2* __restrict__ pb, int n_max,
                                                         const int* __restrict__ count, float thr2, int refine,
                                                         const TState* __restrict__ st, float* __restrict__ Hout,
                                                         int* __restrict__ status, int* __restrict__ info,
                                                         uint8_t* __restrict__ mask) {
    __shared__ double red[(FINT / 64) * 5];
    __shared__ double cen[5], mom[3];
    const int n = fit_n(count, n_max);
    const int tid = threadIdx.x;
    const int stt = st->status;
    if (stt != 0) {
        if (mask)
            for (int i = tid; i < n_max; i += FINT) mask[i] = 0;
        if (tid == 0) {
            for (int i = 0; i < 9; ++i) Hout[i] = nanf("");
            status[0] = stt;
            if (info) { info[0] = 0; info[1] = -1; info[2] = st->iters; }
        }
        return;
    }
    double m[4] = {st->m[0], st->m[1], st->m[2], st->m[3]};
    const ModelF h = to_f32(m);
    const bool refit = refine && n > 2 && st->n_inl > 2;    // (workgroup-uniform)
    // pass 1: the mask, and the inliers' count and coordinate sums
    double s1[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n_max; i += FINT) {
        bool in = false;
        if (i < n) {
            const float2 a = pa[i], b = pb[i];
            in = n == 2 || reproj_err(h, a.x, a.y, b.x, b.y) <= thr2;
            if (in) {
                s1[0] += 1.0; s1[1] += (double)a.x; s1[2] += (double)a.y; s1[3] += (double)b.x; s1[4] += (double)b.y;
            }
        }
        if (mask) mask[i] = in ? 1 : 0;
    }
    if (refit) {
        block_sum_d<5>(s1, red, cen);
        const double cnt = cen[0];
        const double cax = cen[1] / cnt, cay = cen[2] / cnt, cbx = cen[3] / cnt, cby = cen[4] / cnt;
        // pass 2: sum (b - bbar) conj(a - abar) and sum |a - abar|^2 over the same inliers
        double s2[3] = {0.0, 0.0, 0.0};
        for (int i = tid; i < n; i += FINT) {
            const float2 a = pa[i], b = pb[i];
            if (reproj_err(h, a.x, a.y, b.x, b.y) <= thr2) {
                const double ax = (double)a.x - cax, ay = (double)a.y - cay, bx = (double)b.x - cbx, by = (double)b.y - cby;
                s2[0] += bx * ax + by * ay;
                s2[1] += by * ax - bx * ay;
                s2[2] += ax * ax + ay * ay;
            }
        }
        block_sum_d<3>(s2, red, mom);
        if (mom[2] > 0.0) {
            const double qr = mom[0] / mom[2], qi = mom[1] / mom[2];
            const double tx = cbx - (qr * cax - qi * cay), ty = cby - (qi * cax + qr * cay);
            if (isfinite(qr) && isfinite(qi) && isfinite(tx) && isfinite(ty)) {
                m[0] = qr; m[1] = qi; m[2] = tx; m[3] = ty;
            }
        }
    }
    if (tid == 0) {
        Hout[0] = (float)m[0]; Hout[1] = -(float)m[1]; Hout[2] = (float)m[2];
        Hout[3] = (float)m[1]; Hout[4] = (float)m[0]; Hout[5] = (float)m[3];
        Hout[6] = 0.f; Hout[7] = 0.f; Hout[8] = 1.f;
        status[0] = 0;
        if (info) { info[0] = st->n_inl; info[1] = st->best_k; info[2] = st->iters; }
    }
}

}  // namespace

extern "C" int64_t woft_trs_ws_bytes(int32_t n_max, int32_t max_iters) {
    if (n_max < 0 || max_iters < 1) return WOFT_EINVAL;
    return align256((int64_t)max_iters * 4) + align256(sizeof(TState));
}

extern "C" int woft_trs(const float* pa, const float* pb, int32_t n_max, const int32_t* count, int32_t max_iters, double thr,
                        double conf, uint64_t seed, int32_t refine, void* ws, float* Hout, int32_t* status, int32_t* info,
                        uint8_t* inlier_mask, void* stream) {
    if (!pa || !pb || !ws || !Hout || !status || n_max < 0 || max_iters < 1 || !(thr > 0.0) || !(conf >= 0.0 && conf <= 1.0))
        return WOFT_EINVAL;
    const int64_t chunks = std::max<int64_t>(1, ((int64_t)n_max + TCHUNK - 1) / TCHUNK);
    if (chunks > 65535) return WOFT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const TWs o = ws_layout(ws, max_iters);
    const float thr2 = (float)(thr * thr);
    const uint64_t key = splitmix64(seed);                   // (keys every hypothesis' stream)
    const auto pa2 = (const float2*)pa, pb2 = (const float2*)pb;
    if (chunks > 1) (void)hipMemsetAsync(o.counts, 0, (size_t)max_iters * 4, s);
    hipLaunchKernelGGL(trs_score_kernel, dim3((max_iters + TH - 1) / TH, (unsigned)chunks), dim3(TT), 0, s, pa2, pb2, n_max, count,
                       max_iters, key, thr2, chunks > 1 ? 1 : 0, o.counts);
    hipLaunchKernelGGL(trs_select_kernel, dim3(1), dim3(SELT), 0, s, pa2, pb2, n_max, count, max_iters, key, conf,
                       (const int*)o.counts, o.st);
    hipLaunchKernelGGL(trs_final_kernel, dim3(1), dim3(FINT), 0, s, pa2, pb2, n_max, count, thr2, refine ? 1 : 0,
                       (const TState*)o.st, Hout, status, info, inlier_mask);
    return woft_launch_status();
}
