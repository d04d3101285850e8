// RANSAC homography estimator: what cv2.findHomography(src, dst, cv2.RANSAC, thr, maxIters, confidence) does
// (utils/least_squares_H.py:366-396, `find_homography_cvransac`, and the configs that call it: ..._cvransac.py, ablation_09.py),
// restated from OpenCV's published behaviour -- OpenCV's source is not pinned here ("RANSAC").
//
// Semantics (the host restatement tests/ransac_host.py follows them step for step):
//   * n < 4: status 1 (the Python entry raises AssertionError before any launch on host inputs).
//   * n == 4: the direct 4-point solution; no sampling, no refinement (cv2's count == modelPoints branch).
//   * hypothesis k = 0 .. max_iters-1: four distinct indices, draw c of hypothesis k being
//       u = splitmix64(splitmix64(seed) ^ ((k << 32) | c)),   index = ((u >> 32) * n) >> 32,
//     c counting every draw of the hypothesis (a duplicate index is drawn again with the next c).  The sample must pass cv2's
//     checkSubset: no three of the four points collinear in either set (|dx2 dy1 - dy2 dx1| <= FLT_EPSILON (|dx1|+|dx2|+|dy1|+|dy2|),
//     differences in fp32 as cv2 forms them from Point2f, the test in fp64), and the orientation signs of the triangles
//     {012, 123, 023, 013} all agree between the two sets or all flip.  A failed check draws a new sample, up to 1000 attempts; a
//     hypothesis without a sample is "no sample" (cv2 breaks its loop there, or fails when k == 0).
//   * model: H = Q_b adj(Q_a) in fp64 (Q: the unit square -> quad map of the 4 points), h33 = 1.  A singular model scores 0.
//   * score: #{i : err_i <= thr^2} with cv2's fp32 error: ww = 1 / (h6 x + h7 y + 1), dx = (h0 x + h1 y + h2) ww - X, dy alike,
//     err = dx^2 + dy^2 (thr^2 rounded to fp32 once, as cv2 does).
//   * selection = cv2's sequential loop: a new best needs count > max(best, 3); after it, niters = RANSACUpdateNumIters(conf,
//     (n - count) / n, 4, niters); the loop ends at the first k >= niters or at the first "no sample" hypothesis.
//   * refinement (n > 4): the unweighted DLT over the inliers (woft_hfit with the 0/1 inlier vector as w), then 10
//     Levenberg-Marquardt iterations on h0..h7 (h33 = 1) of sum |proj(H, a) - b|^2 over the inliers, fp64, one workgroup.
//   * no model (no hypothesis with >= 4 inliers): H all NaN, status 2 (the reference raises a TypeError on None[2, 2]).
//
// Launches (fixed count, no host synchronisation, every hand-off at a kernel boundary):
//   score  (hypothesis block x point chunk workgroups; partial counts by integer atomicAdd when there is more than one chunk:
//           exact, so deterministic)  ->  select (one workgroup rebuilds the sequential loop from counts[]: prefix maxima,
//           records, stop, best)  ->  mask (0/1 weights + optional uint8 mask)  ->  woft_hfit (DLT)  ->  final (LM + outputs).
#include "ransac_common.h"
#include <algorithm>

namespace {

constexpr int RT = 256;             // threads of a scoring workgroup: 64 hypotheses x 4 point slices (one wave per slice)
constexpr int RH = 64;              // hypotheses per scoring workgroup
constexpr int RCHUNK = 2048;        // points per scoring workgroup (gridDim.y = ceil(n_max / RCHUNK))
constexpr int MAX_ATTEMPTS = 1000;  // cv2's maxAttempts of getSubset
constexpr int LMT = 512;            // threads of the refinement workgroup (45 fp64 accumulators per lane)
constexpr int LM_ITERS = 10;

struct RState {                     // in the workspace, written by the select kernel, read by mask / final
    int status, best_k, n_inl, iters;
    int hstatus, pad0, pad1, pad2;
    double Hb[9];                   // best RANSAC model (h33 = 1)
    float Hdlt[9];                  // the DLT over the inliers (woft_hfit output)
};

struct RWs {
    int* counts;
    RState* st;
    float* w;
    void* hws;
};

inline bool need_hws(int n_max) { return n_max > WOFT_HFIT_SINGLE_MAX; }

inline RWs ws_layout(void* ws, int n_max, int max_iters) {
    RWs o;
    char* p = (char*)ws;
    o.counts = (int*)p;
    p += align256((int64_t)max_iters * 4);
    o.st = (RState*)p;
    p += align256(sizeof(RState));
    o.w = (float*)p;
    p += align256((int64_t)n_max * 4);
    o.hws = need_hws(n_max) ? (void*)p : nullptr;
    return o;
}

// cv2 haveCollinearPoints for the triple (pivot i, j, k): differences of Point2f in fp32, the test in fp64
__device__ __forceinline__ bool collinear(float2 pi, float2 pj, float2 pk) {
    const double dx1 = (double)(pj.x - pi.x), dy1 = (double)(pj.y - pi.y);
    const double dx2 = (double)(pk.x - pi.x), dy2 = (double)(pk.y - pi.y);
    return fabs(dx2 * dy1 - dy2 * dx1) <= (double)FLT_EPSILON * (fabs(dx1) + fabs(dx2) + fabs(dy1) + fabs(dy2));
}

__device__ __forceinline__ bool any_collinear(const float2 (&p)[4]) {
    return collinear(p[2], p[1], p[0]) || collinear(p[3], p[1], p[0]) || collinear(p[3], p[2], p[0]) ||
           collinear(p[3], p[2], p[1]);
}

// determinant of [[x0 y0 1] [x1 y1 1] [x2 y2 1]] in fp64, cofactor expansion along the first row
__device__ __forceinline__ double orient(float2 a, float2 b, float2 c) {
    const double x0 = a.x, y0 = a.y, x1 = b.x, y1 = b.y, x2 = c.x, y2 = c.y;
    return x0 * (y1 - y2) - y0 * (x1 - x2) + (x1 * y2 - x2 * y1);
}

__device__ bool check_subset(const float2 (&a)[4], const float2 (&b)[4]) {
    if (any_collinear(a) || any_collinear(b)) return false;
    int neg = 0;
    neg += orient(a[0], a[1], a[2]) * orient(b[0], b[1], b[2]) < 0.0;
    neg += orient(a[1], a[2], a[3]) * orient(b[1], b[2], b[3]) < 0.0;
    neg += orient(a[0], a[2], a[3]) * orient(b[0], b[2], b[3]) < 0.0;
    neg += orient(a[0], a[1], a[3]) * orient(b[0], b[1], b[3]) < 0.0;
    return neg == 0 || neg == 4;
}

// -> true with the sample's points when a sample passing check_subset is found within MAX_ATTEMPTS
__device__ bool draw_sample(const float2* __restrict__ pa, const float2* __restrict__ pb, int n, uint64_t key, int k,
                            float2 (&a)[4], float2 (&b)[4]) {
    uint32_t c = 0;
    for (int att = 0; att < MAX_ATTEMPTS; ++att) {
        int idx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bool dup;
            do {
                idx[i] = draw_index(key, k, c++, n);
                dup = false;
#pragma unroll
                for (int j = 0; j < i; ++j) dup |= (idx[j] == idx[i]);
            } while (dup);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[i] = pa[idx[i]];
            b[i] = pb[idx[i]];
        }
        if (check_subset(a, b)) return true;
    }
    return false;
}

// unit square (0,0) (1,0) (1,1) (0,1) -> quad p0 p1 p2 p3 (Heckbert's closed form; the affine case needs no branch)
__device__ __forceinline__ bool square_to_quad(const float2 (&p)[4], double (&q)[9]) {
    const double x0 = p[0].x, y0 = p[0].y, x1 = p[1].x, y1 = p[1].y, x2 = p[2].x, y2 = p[2].y, x3 = p[3].x, y3 = p[3].y;
    const double sx = x0 - x1 + x2 - x3, sy = y0 - y1 + y2 - y3;
    const double dx1 = x1 - x2, dx2 = x3 - x2, dy1 = y1 - y2, dy2 = y3 - y2;
    const double den = dx1 * dy2 - dx2 * dy1;
    if (den == 0.0) return false;
    const double g = (sx * dy2 - dx2 * sy) / den, h = (dx1 * sy - sx * dy1) / den;
    q[0] = x1 - x0 + g * x1; q[1] = x3 - x0 + h * x3; q[2] = x0;
    q[3] = y1 - y0 + g * y1; q[4] = y3 - y0 + h * y3; q[5] = y0;
    q[6] = g; q[7] = h; q[8] = 1.0;
    return true;
}

// exact 4-point model a -> b: H = Q_b adj(Q_a), scaled to h33 = 1; false when singular
__device__ bool model4(const float2 (&a)[4], const float2 (&b)[4], double (&H)[9]) {
    double qa[9], qb[9];
    if (!square_to_quad(a, qa) || !square_to_quad(b, qb)) return false;
    const double adj[9] = {qa[4] * qa[8] - qa[5] * qa[7], qa[2] * qa[7] - qa[1] * qa[8], qa[1] * qa[5] - qa[2] * qa[4],
                           qa[5] * qa[6] - qa[3] * qa[8], qa[0] * qa[8] - qa[2] * qa[6], qa[2] * qa[3] - qa[0] * qa[5],
                           qa[3] * qa[7] - qa[4] * qa[6], qa[1] * qa[6] - qa[0] * qa[7], qa[0] * qa[4] - qa[1] * qa[3]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) H[r * 3 + c] = qb[r * 3] * adj[c] + qb[r * 3 + 1] * adj[3 + c] + qb[r * 3 + 2] * adj[6 + c];
    const double s = H[8];
    if (s == 0.0) return false;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        H[i] = H[i] / s;
        ok = ok && isfinite(H[i]);
    }
    H[8] = 1.0;
    return ok;
}

__device__ __forceinline__ float reproj_err(const float (&hf)[8], float2 a, float2 b) {
    const float ww = 1.f / (hf[6] * a.x + hf[7] * a.y + 1.f);
    const float dx = (hf[0] * a.x + hf[1] * a.y + hf[2]) * ww - b.x;
    const float dy = (hf[3] * a.x + hf[4] * a.y + hf[5]) * ww - b.y;
    return dx * dx + dy * dy;
}

// counts[k] = inliers of hypothesis k (0: singular model, -1: no sample)
__global__ __launch_bounds__(RT) void ransac_score_kernel(const float2* __restrict__ pa, const float2* __restrict__ pb, int n_max,
                                                          const int* __restrict__ count, int max_iters, uint64_t key, float thr2,
                                                          int multi, int* __restrict__ counts) {
    __shared__ int part[4][RH];
    const int n = fit_n(count, n_max);
    const int64_t p0 = (int64_t)blockIdx.y * RCHUNK;
    if (n <= 4 || p0 >= n) return;                          // (workgroup-uniform)
    const int64_t p1 = min((int64_t)n, p0 + RCHUNK);
    const int hl = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int k = blockIdx.x * RH + hl;
    int cnt = 0;
    bool sampled = true;
    if (k < max_iters) {
        float2 a[4], b[4];
        double H[9];
        sampled = draw_sample(pa, pb, n, key, k, a, b);
        if (sampled && model4(a, b, H)) {
            float hf[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) hf[i] = (float)H[i];
            for (int64_t i = p0 + slice; i < p1; i += 4) cnt += reproj_err(hf, pa[i], pb[i]) <= thr2;
        }
    }
    part[slice][hl] = cnt;
    __syncthreads();
    if (slice != 0 || k >= max_iters) return;
    const int tot = part[0][hl] + part[1][hl] + part[2][hl] + part[3][hl];
    if (!multi) {
        counts[k] = sampled ? tot : -1;
    } else if (!sampled) {
        if (blockIdx.y == 0) atomicAdd(&counts[k], -1);
    } else if (tot != 0) {
        atomicAdd(&counts[k], tot);
    }
}

// one workgroup: the sequential loop's stop, best hypothesis and model, from counts[]
__global__ __launch_bounds__(SELT) void ransac_select_kernel(const float2* __restrict__ pa, const float2* __restrict__ pb,
                                                             int n_max, const int* __restrict__ count, int max_iters, uint64_t key,
                                                             double conf, const int* __restrict__ counts, RState* __restrict__ st) {
    const int n = fit_n(count, n_max);
    const int tid = threadIdx.x;
    if (n < 4) {
        if (tid == 0) { st->status = 1; st->best_k = -1; st->n_inl = 0; st->iters = 0; }
        return;
    }
    if (n == 4) {
        if (tid == 0) {
            float2 a[4], b[4];
            for (int i = 0; i < 4; ++i) { a[i] = pa[i]; b[i] = pb[i]; }
            double H[9];
            const bool ok = model4(a, b, H);
            for (int i = 0; i < 9; ++i) st->Hb[i] = H[i];
            st->status = ok ? 0 : 2; st->best_k = ok ? 0 : -1; st->n_inl = ok ? 4 : 0; st->iters = 0;
        }
        return;
    }
    int S, best;
    sequential_select<4>(counts, max_iters, conf, n, S, best);
    if (tid == 0) {
        st->iters = S;
        st->best_k = best;
        if (best < 0) {
            st->status = 2; st->n_inl = 0;
            return;
        }
        float2 a[4], b[4];
        double H[9];
        draw_sample(pa, pb, n, key, best, a, b);
        model4(a, b, H);
        for (int i = 0; i < 9; ++i) st->Hb[i] = H[i];
        st->n_inl = counts[best];
        st->status = 0;
    }
}

// inlier vector of the best model: w (0/1 float, the DLT's weights) and the optional uint8 mask; zero beyond n
__global__ __launch_bounds__(256) void ransac_mask_kernel(const float2* __restrict__ pa, const float2* __restrict__ pb, int n_max,
                                                          const int* __restrict__ count, float thr2, const RState* __restrict__ st,
                                                          float* __restrict__ w, uint8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_max) return;
    const int n = fit_n(count, n_max);
    bool in = false;
    if (i < n && st->status == 0) {
        if (n == 4) {
            in = true;
        } else {
            float hf[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) hf[k] = (float)st->Hb[k];
            in = reproj_err(hf, pa[i], pb[i]) <= thr2;
        }
    }
    w[i] = in ? 1.f : 0.f;
    if (mask) mask[i] = in ? 1 : 0;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

constexpr int NACC = 36 + 8 + 1;    // upper triangle of J^T J, J^T r, sum r^2

// J^T J, J^T r and the squared error of h over the inliers (w != 0), fp64, fixed-order reduction -> out[NACC] (LDS)
__device__ void lm_accumulate(const float2* __restrict__ pa, const float2* __restrict__ pb, const float* __restrict__ w, int n,
                              const double* h, double* red /* [LMT/64][NACC] */, double* out) {
    double acc[NACC];
#pragma unroll
    for (int t = 0; t < NACC; ++t) acc[t] = 0.0;
    const double h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6], h7 = h[7];
    for (int i = threadIdx.x; i < n; i += LMT) {
        if (w[i] == 0.f) continue;
        const float2 a = pa[i], b = pb[i];
        const double x = a.x, y = a.y;
        const double inv = 1.0 / (h6 * x + h7 * y + 1.0);
        const double u = (h0 * x + h1 * y + h2) * inv, v = (h3 * x + h4 * y + h5) * inv;
        const double ru = u - (double)b.x, rv = v - (double)b.y;
        const double xi = x * inv, yi = y * inv;
        const double ju[8] = {xi, yi, inv, 0.0, 0.0, 0.0, -u * xi, -u * yi};
        const double jv[8] = {0.0, 0.0, 0.0, xi, yi, inv, -v * xi, -v * yi};
        int t = 0;
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int q = p; q < 8; ++q, ++t) acc[t] += ju[p] * ju[q] + jv[p] * jv[q];
#pragma unroll
        for (int p = 0; p < 8; ++p) acc[36 + p] += ju[p] * ru + jv[p] * rv;
        acc[44] += ru * ru + rv * rv;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < NACC; ++t) {
        const double s = wave_sum_d(acc[t]);
        if (lane == 0) red[wave * NACC + t] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < NACC) {
        double s = 0.0;
        for (int wv = 0; wv < LMT / 64; ++wv) s += red[wv * NACC + threadIdx.x];
        out[threadIdx.x] = s;
    }
    __syncthreads();
}

// (A + lambda diag(A)) d = -g by fp64 Cholesky; A packed upper triangle
__device__ bool lm_step(const double* acc, double lambda, double* d) {
    double A[8][8], L[8][8], z[8];
    int t = 0;
    for (int p = 0; p < 8; ++p)
        for (int q = p; q < 8; ++q, ++t) A[p][q] = A[q][p] = acc[t];
    for (int p = 0; p < 8; ++p) A[p][p] += lambda * A[p][p];
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = A[i][j];
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            if (i == j) {
                if (!(s > 0.0)) return false;
                L[i][i] = sqrt(s);
            } else {
                L[i][j] = s / L[j][j];
            }
        }
    for (int i = 0; i < 8; ++i) {
        double s = -acc[36 + i];
        for (int k = 0; k < i; ++k) s -= L[i][k] * z[k];
        z[i] = s / L[i][i];
    }
    for (int i = 7; i >= 0; --i) {
        double s = z[i];
        for (int k = i + 1; k < 8; ++k) s -= L[k][i] * d[k];
        d[i] = s / L[i][i];
    }
    return true;
}

// one workgroup: Levenberg-Marquardt refinement (n > 4, refine) and the outputs
__global__ __launch_bounds__(LMT) void ransac_final_kernel(const float2* __restrict__ pa, const float2* __restrict__ pb,
                                                           const float* __restrict__ w, int n_max, const int* __restrict__ count,
                                                           int refine, const RState* __restrict__ st, float* __restrict__ Hout,
                                                           int* __restrict__ status, int* __restrict__ info) {
    __shared__ double red[(LMT / 64) * NACC];
    __shared__ double cur[NACC], cand[NACC];
    __shared__ double h_s[8], hc_s[8];
    __shared__ int go_s;
    const int n = fit_n(count, n_max);
    const int tid = threadIdx.x;
    const int stt = st->status;
    if (stt != 0) {
        if (tid == 0) {
            for (int i = 0; i < 9; ++i) Hout[i] = nanf("");
            status[0] = stt;
            if (info) { info[0] = 0; info[1] = -1; info[2] = st->iters; }
        }
        return;
    }
    if (tid == 0) {
        bool dlt = refine && n > 4 && st->hstatus == 0;
        double hd[8];
        if (dlt) {
            const double s = (double)st->Hdlt[8];
            for (int i = 0; i < 8; ++i) {
                hd[i] = (double)st->Hdlt[i] / s;
                dlt = dlt && isfinite(hd[i]);
            }
        }
        for (int i = 0; i < 8; ++i) h_s[i] = dlt ? hd[i] : st->Hb[i];
    }
    __syncthreads();
    if (refine && n > 4) {
        lm_accumulate(pa, pb, w, n, h_s, red, cur);
        double lambda = 1e-3;
        for (int it = 0; it < LM_ITERS; ++it) {
            __syncthreads();                                 // (everyone has read the previous go_s)
            if (tid == 0) {
                double d[8];
                go_s = lm_step(cur, lambda, d) ? 1 : 0;
                if (go_s) {
                    double dn = 0.0, hn = 0.0;
                    for (int i = 0; i < 8; ++i) {
                        hc_s[i] = h_s[i] + d[i];
                        dn += d[i] * d[i];
                        hn += h_s[i] * h_s[i];
                    }
                    if (sqrt(dn) <= (double)FLT_EPSILON * (sqrt(hn) + (double)FLT_EPSILON)) go_s = 2;   // step below FLT_EPSILON
                }
            }
            __syncthreads();
            const int go = go_s;
            if (go == 2) break;
            if (go == 0) {                                   // singular damped system: more damping
                lambda *= 10.0;
                continue;
            }
            lm_accumulate(pa, pb, w, n, hc_s, red, cand);
            const double e0 = cur[44], e1 = cand[44];
            bool stop = false;
            if (e1 < e0) {
                stop = (e0 - e1) <= (double)FLT_EPSILON * e0;  // relative change below FLT_EPSILON
                __syncthreads();
                if (tid < NACC) cur[tid] = cand[tid];
                if (tid < 8) h_s[tid] = hc_s[tid];
                lambda *= 0.1;
            } else {
                lambda *= 10.0;
            }
            __syncthreads();
            if (stop) break;
        }
    }
    if (tid == 0) {
        for (int i = 0; i < 8; ++i) Hout[i] = (float)h_s[i];
        Hout[8] = 1.f;
        status[0] = 0;
        if (info) { info[0] = st->n_inl; info[1] = st->best_k; info[2] = st->iters; }
    }
}

}  // namespace

extern "C" int64_t woft_ransac_ws_bytes(int32_t n_max, int32_t max_iters) {
    if (n_max < 0 || max_iters < 1) return WOFT_EINVAL;
    int64_t b = align256((int64_t)max_iters * 4) + align256(sizeof(RState)) + align256((int64_t)n_max * 4);
    if (need_hws(n_max)) b += woft_hfit_ws_bytes();
    return b;
}

extern "C" int woft_ransac(const float* pa, const float* pb, int32_t n_max, const int32_t* count, int32_t max_iters, double thr,
                           double conf, uint64_t seed, int32_t refine, void* ws, float* Hout, int32_t* status, int32_t* info,
                           uint8_t* inlier_mask, void* stream) {
    if (!pa || !pb || !ws || !Hout || !status || n_max < 0 || max_iters < 1 || !(thr > 0.0) || !(conf >= 0.0 && conf <= 1.0))
        return WOFT_EINVAL;
    const int64_t chunks = std::max<int64_t>(1, ((int64_t)n_max + RCHUNK - 1) / RCHUNK);
    if (chunks > 65535) return WOFT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const RWs o = ws_layout(ws, n_max, max_iters);
    const float thr2 = (float)(thr * thr);
    const uint64_t key = splitmix64(seed);                   // (keys every hypothesis' stream)
    const auto pa2 = (const float2*)pa, pb2 = (const float2*)pb;
    if (chunks > 1) (void)hipMemsetAsync(o.counts, 0, (size_t)max_iters * 4, s);
    hipLaunchKernelGGL(ransac_score_kernel, dim3((max_iters + RH - 1) / RH, (unsigned)chunks), dim3(RT), 0, s, pa2, pb2, n_max,
                       count, max_iters, key, thr2, chunks > 1 ? 1 : 0, o.counts);
    hipLaunchKernelGGL(ransac_select_kernel, dim3(1), dim3(SELT), 0, s, pa2, pb2, n_max, count, max_iters, key, conf,
                       (const int*)o.counts, o.st);
    if (n_max > 0)
        hipLaunchKernelGGL(ransac_mask_kernel, dim3((unsigned)((n_max + 255) / 256)), dim3(256), 0, s, pa2, pb2, n_max, count,
                           thr2, (const RState*)o.st, o.w, inlier_mask);
    if (refine) {
        const int rc = woft_hfit(pa, pb, o.w, n_max, count, 0, 0.f, 0, o.hws, o.st->Hdlt, &o.st->hstatus, stream);
        if (rc != WOFT_OK) return rc;
    }
    hipLaunchKernelGGL(ransac_final_kernel, dim3(1), dim3(LMT), 0, s, pa2, pb2, (const float*)o.w, n_max, count, refine ? 1 : 0,
                       (const RState*)o.st, Hout, status, info);
    return woft_launch_status();
}
