// Photometric refinement of a fitted homography: inverse-compositional Gauss-Newton on the template's
// pixels with an optional gain and bias.  Two kernels: `photo_accum_kernel` turns (template, mask, frame, state) into one partial
// of the normal equations per workgroup, `photo_step_kernel` (one workgroup) sums the partials in index order, applies the
// control rules, solves and steps the state on the device.  A refinement is iters + 1 pairs of them enqueued back to back; after
// a stop the remaining launches return on a uniform branch.  Coordinates, the sample, every per-pixel term and every sum are
// fp64; every product is followed by its add (the build passes -ffp-contract=off); no atomics: two calls give equal bytes.
// The multi-target forms run K targets of one template and one frame through the same two device
// functions on a (partials, K) and a K grid: the same chunks summed in the same order, so a target's bytes are the single form's.
#include <math.h>
#include "common.h"

namespace {

constexpr int NU_MAX = 10;                       // unknowns with gain and bias (8 without)
constexpr int NACC = WOFT_PHOTO_NACC;            // doubles per partial: upper triangle of G, r, sum weight*rho, sum weight, n
constexpr int THREADS = 256, ITEMS = WOFT_PHOTO_CHUNK / THREADS;
constexpr int REC = WOFT_PHOTO_REC;              // doubles per iterate record (and of the result block's header)
static_assert(NU_MAX * (NU_MAX + 1) / 2 + NU_MAX + 3 == NACC, "partial layout");
static_assert(ITEMS * THREADS == WOFT_PHOTO_CHUNK, "chunk");

// The pixel set's strided grid (nx x ny candidates from (x0, y0)), the two image sizes and the normalisation x~ = (x - cx) / s.
struct Geom {
    int h, w, hf, wf, x0, y0, nx, ny, stride;
    double cx, cy, s;
};
// M (normalised template coordinates -> frame pixels), gain, bias (in units of S = c0 + c1 + c2).
struct State { double m[9], g, b; };

// Device state behind the partials in the workspace: 16 doubles (M, g, b, best cost), then int32 {stop, best, conv_at}.
constexpr int ST_DOUBLES = 16, ST_BEST_COST = 11;

__device__ __forceinline__ double sum3(const uint8_t* p) { return (double)((int)p[0] + (int)p[1] + (int)p[2]); }
__device__ __forceinline__ double sum3(const float* p) { return ((double)p[0] + (double)p[1]) + (double)p[2]; }

__device__ __forceinline__ State load_state(const double* st) {
    State s;
#pragma unroll
    for (int i = 0; i < 9; ++i) s.m[i] = st[i];
    s.g = st[9], s.b = st[10];
    return s;
}

typedef double f64x4 __attribute__((ext_vector_type(4)));

// The mask test: a uint8 mask, or bit t of the multi-target bit plane (unsigned words: target 31 is the top bit).
__device__ __forceinline__ bool in_mask(const uint8_t* m, int64_t o, int) { return m[o] != 0; }
__device__ __forceinline__ bool in_mask(const uint32_t* m, int64_t o, int t) { return ((m[o] >> t) & 1u) != 0u; }

// Candidate idx of the strided grid (row-major) -> its row x of the 16-column system whose Gram matrix carries every sum:
//   x[0 .. NU) = sqrt(omega) a,  x[NU] = sqrt(omega) e,  x[NU + 1] = sqrt(weight rho),  x[NU + 2] = sqrt(weight),  x[NU + 3] = 1,
// so that G = X^T X restricted to NU x NU, r = its column NU, sum weight rho, sum weight and n = the last three diagonal
// entries.  false (x untouched): the candidate is outside the grid, the template's interior, the mask or the frame.
// k3 = 3 * huber_k, < 0: no Huber.
template <typename TT, typename TF, typename TM, int NU>
__device__ __forceinline__ bool pixel_row(const TT* __restrict__ tmpl, const TM* __restrict__ mask, int tbit,
                                          const float* __restrict__ weights, const TF* __restrict__ frame, const Geom& gm,
                                          const State& st, double k3, int64_t idx, double* x_out) {
    {
        if (idx >= (int64_t)gm.nx * gm.ny) return false;
        const int iy = (int)(idx / gm.nx), ix = (int)(idx - (int64_t)iy * gm.nx);
        const int x = gm.x0 + ix * gm.stride, y = gm.y0 + iy * gm.stride;
        if (x < 1 || x > gm.w - 2 || y < 1 || y > gm.h - 2) return false;
        const int64_t o = (int64_t)y * gm.w + x;
        if (!in_mask(mask, o, tbit)) return false;
        const double xn = ((double)x - gm.cx) / gm.s, yn = ((double)y - gm.cy) / gm.s;
        const double qx = st.m[0] * xn + st.m[1] * yn + st.m[2];
        const double qy = st.m[3] * xn + st.m[4] * yn + st.m[5];
        const double qz = st.m[6] * xn + st.m[7] * yn + st.m[8];
        const double u = qx / qz, v = qy / qz;
        if (!(qz > 0.0 && u >= 0.0 && u < (double)(gm.wf - 1) && v >= 0.0 && v < (double)(gm.hf - 1))) return false;
        const double fu = floor(u), fv = floor(v), fx = u - fu, fy = v - fv;
        const int64_t fo = (int64_t)fv * gm.wf + (int64_t)fu;     // (0 <= fu <= wf - 2, 0 <= fv <= hf - 2: all four taps inside)
        const double s00 = sum3(frame + fo * 3), s01 = sum3(frame + (fo + 1) * 3);
        const double s10 = sum3(frame + (fo + gm.wf) * 3), s11 = sum3(frame + (fo + gm.wf + 1) * 3);
        const double I = (1.0 - fy) * ((1.0 - fx) * s00 + fx * s01) + fy * ((1.0 - fx) * s10 + fx * s11);
        const double T = sum3(tmpl + o * 3);
        const double gxn = gm.s * ((sum3(tmpl + (o + 1) * 3) - sum3(tmpl + (o - 1) * 3)) * 0.5);
        const double gyn = gm.s * ((sum3(tmpl + (o + gm.w) * 3) - sum3(tmpl + (o - gm.w) * 3)) * 0.5);
        const double e = I - st.g * T - st.b;
        const double wt = weights != nullptr ? (double)weights[o] : 1.0;
        const double ae = fabs(e);
        double om = wt, rho = e * e;
        if (k3 >= 0.0 && ae > k3) {
            om = wt * (k3 / ae);
            rho = 2.0 * k3 * ae - k3 * k3;
        }
        const double d = gxn * xn + gyn * yn;
        double a[NU];
        a[0] = st.g * (gxn * xn), a[1] = st.g * (gxn * yn), a[2] = st.g * gxn;
        a[3] = st.g * (gyn * xn), a[4] = st.g * (gyn * yn), a[5] = st.g * gyn;
        a[6] = st.g * (-xn * d), a[7] = st.g * (-yn * d);
        if (NU == 10) a[NU - 2] = T, a[NU - 1] = 1.0;
        const double sq = sqrt(om);
#pragma unroll
        for (int i = 0; i < NU; ++i) x_out[i] = sq * a[i];
        x_out[NU] = sq * e, x_out[NU + 1] = sqrt(wt * rho), x_out[NU + 2] = sqrt(wt), x_out[NU + 3] = 1.0;
        return true;
    }
}

// One partial of (G upper triangle row-major, r, sum weight*rho, sum weight, n) per workgroup -> part[blockIdx.x * NACC ..].
// A turn: every lane builds the row of candidate blockIdx.x * CHUNK + j * THREADS + tid (zeros when there is none) and stages it
// in LDS; each wavefront then folds its 64 rows into its 16 x 16 fp64 Gram accumulator with 16 v_mfma_f64_16x16x4_f64, four rows
// each, lane (c = lane & 15, k = lane >> 4) supplying element c of row k as BOTH operands (the form of hfit.hip's Gram) -- 4
// accumulator registers per lane where one accumulator per entry and lane took 2 x 68, and no cross-lane reduction at the end.
// Rows are ROW_LD = 17 doubles apart: the 32 lanes of a half wave write their rows to distinct banks.
constexpr int ROW_LD = 17;
// The partial of chunk `chunk` of the pixel set (gm, mask -- bit tbit of it when it is a bit plane) at the state st -> part[0 .. NACC).
template <typename TT, typename TF, typename TM, int NU>
__device__ __forceinline__ void accum_chunk(const TT* __restrict__ tmpl, const TM* __restrict__ mask, int tbit,
                                            const float* __restrict__ weights, const TF* __restrict__ frame, const Geom& gm,
                                            const State& st, double k3, int chunk, double* __restrict__ part) {
    constexpr int TRI = NU * (NU + 1) / 2, LIVE = NU + 4;
    static_assert(LIVE <= 16, "the system's columns fit one MFMA tile");
    __shared__ double rows[THREADS * ROW_LD];
    __shared__ double red[THREADS / 64][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* mine = rows + tid * ROW_LD;
#pragma unroll
    for (int c = LIVE; c < 16; ++c) mine[c] = 0.0;               // (the padding columns, once)
    const double* tile = rows + wave * 64 * ROW_LD + (lane >> 4) * ROW_LD + (lane & 15);
    f64x4 g4 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int j = 0; j < ITEMS; ++j) {
        double x[LIVE];
#pragma unroll
        for (int c = 0; c < LIVE; ++c) x[c] = 0.0;
        pixel_row<TT, TF, TM, NU>(tmpl, mask, tbit, weights, frame, gm, st, k3, (int64_t)chunk * WOFT_PHOTO_CHUNK + j * THREADS + tid, x);
#pragma unroll
        for (int c = 0; c < LIVE; ++c) mine[c] = x[c];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const double val = tile[4 * m * ROW_LD];
            g4 = __builtin_amdgcn_mfma_f64_16x16x4f64(val, val, g4, 0, 0, 0);
        }
        __syncthreads();
    }
    // D layout of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * reg; the four wavefronts in order
#pragma unroll
    for (int q = 0; q < 4; ++q) red[wave][((lane >> 4) + 4 * q) * 16 + (lane & 15)] = g4[q];
    __syncthreads();
    const int i = tid >> 4, c = tid & 15;
    int slot = -1;
    if (i <= c && c < NU) slot = i * NU - i * (i - 1) / 2 + (c - i);
    else if (c == NU && i < NU) slot = TRI + i;
    else if (i == c && i > NU && i < LIVE) slot = TRI + NU + (i - NU - 1);
    if (slot >= 0) {
        double v = red[0][tid];
#pragma unroll
        for (int q = 1; q < THREADS / 64; ++q) v = v + red[q][tid];
        part[slot] = v;
    }
}

template <typename TT, typename TF, int NU>
__global__ __launch_bounds__(THREADS) void photo_accum_kernel(const TT* __restrict__ tmpl, const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ weights, const TF* __restrict__ frame,
                                                              Geom gm, State init, const double* st_dev, const int* stop,
                                                              double k3, double* __restrict__ part) {
    if (stop != nullptr && *stop != 0) return;                   // (uniform: the refinement has stopped)
    const State st = st_dev != nullptr ? load_state(st_dev) : init;
    accum_chunk<TT, TF, uint8_t, NU>(tmpl, mask, 0, weights, frame, gm, st, k3, (int)blockIdx.x, part + (int64_t)blockIdx.x * NACC);
}

// ---- K targets of one template and one frame ---------------------------------------------------------------
// What differs per target travels by value in the kernels' arguments (3 584 B at 32 targets, as the homographies of
// mask_bbox_multi_kernel do): the box, the threshold, the number of partials (0: the target is inactive) and the starting state.
struct Tgt {
    int x0, y0, x1, y1, n_need, n_part;
    double m[9], g, b;
};
struct TgtSet {
    Tgt t[WOFT_MULTI_MAX_TARGETS];
};
static_assert(sizeof(TgtSet) == 112 * WOFT_MULTI_MAX_TARGETS, "the targets fit the kernel arguments");

// Target t's slice of the workspace: p_max partials, then the 16 + 2 doubles of its device state (the single form's layout).
__device__ __host__ __forceinline__ int64_t slice_doubles(int p_max) { return (int64_t)p_max * NACC + ST_DOUBLES + 2; }

// `shared` (the image sizes and the stride) completed with a target's box: the arithmetic of prepare(), every value exact.
__device__ __forceinline__ Geom target_geom(const Geom& shared, int x0, int y0, int x1, int y1) {
    Geom gm = shared;
    gm.x0 = x0, gm.y0 = y0;
    gm.nx = (x1 - x0) / gm.stride + 1, gm.ny = (y1 - y0) / gm.stride + 1;
    gm.cx = (x0 + x1) / 2.0, gm.cy = (y0 + y1) / 2.0;
    const int ext = (x1 - x0) > (y1 - y0) ? (x1 - x0) : (y1 - y0);
    gm.s = (ext > 1 ? ext : 1) / 2.0;
    return gm;
}

// Workgroup (p, t): partial p of target t, by accum_chunk on bit t of the plane; p past the target's partials, an inactive or a
// stopped target: a uniform return.  first: the state is the arguments' (iterate 0, or an evaluation), else the slice's.
template <typename TT, typename TF, int NU>
__global__ __launch_bounds__(THREADS) void photo_accum_multi_kernel(const TT* __restrict__ tmpl, const uint32_t* __restrict__ bits,
                                                                    const float* __restrict__ weights,
                                                                    const TF* __restrict__ frame, Geom shared, TgtSet ts, int p_max,
                                                                    int first, double k3, double* __restrict__ ws) {
    const int t = (int)blockIdx.y, p = (int)blockIdx.x;
    if (p >= ts.t[t].n_part) return;
    double* part = ws + (int64_t)t * slice_doubles(p_max);
    const double* st_dev = part + (int64_t)p_max * NACC;
    if (!first && *reinterpret_cast<const int*>(st_dev + ST_DOUBLES) != 0) return;
    State st;
    if (first) {
#pragma unroll
        for (int i = 0; i < 9; ++i) st.m[i] = ts.t[t].m[i];
        st.g = ts.t[t].g, st.b = ts.t[t].b;
    } else {
        st = load_state(st_dev);
    }
    const Geom gm = target_geom(shared, ts.t[t].x0, ts.t[t].y0, ts.t[t].x1, ts.t[t].y1);
    accum_chunk<TT, TF, uint32_t, NU>(tmpl, bits, t, weights, frame, gm, st, k3, p, part + (int64_t)p * NACC);
}

// acc[t] = the sum over the n_part partials of value t, in index order.  One lane per value adding n_part numbers straight from
// memory waits a memory latency per few of them (0.3 us per partial, measured: 159 us at 507 partials); so the workgroup stages
// SUM_TILE partials at a time in LDS with all of its lanes (contiguous, independent loads) and the one lane per value adds from
// there (7.6 us at 254 partials, 25.5 us at 1013).
constexpr int SUM_THREADS = 256, SUM_TILE = 96, SUM_LOADS = (SUM_TILE * NACC + SUM_THREADS - 1) / SUM_THREADS;
__device__ __forceinline__ void sum_partials(const double* __restrict__ part, int n_part, int nacc, double* tile, double* acc) {
    const int t = threadIdx.x;
    double v = 0.0;
    for (int p0 = 0; p0 < n_part; p0 += SUM_TILE) {
        const int np = n_part - p0 < SUM_TILE ? n_part - p0 : SUM_TILE;
        const double* src = part + (int64_t)p0 * NACC;
        double buf[SUM_LOADS];                                   // (every load of the tile in flight before the first store)
#pragma unroll
        for (int q = 0; q < SUM_LOADS; ++q) buf[q] = t + q * SUM_THREADS < np * NACC ? src[t + q * SUM_THREADS] : 0.0;
#pragma unroll
        for (int q = 0; q < SUM_LOADS; ++q)
            if (t + q * SUM_THREADS < np * NACC) tile[t + q * SUM_THREADS] = buf[q];
        __syncthreads();
        if (t < nacc) {
            int p = 0;
            for (; p + 8 <= np; p += 8) {                        // (eight LDS reads in flight, then their adds in order)
                double a[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) a[q] = tile[(p + q) * NACC + t];
#pragma unroll
                for (int q = 0; q < 8; ++q) v = v + a[q];
            }
            for (; p < np; ++p) v = v + tile[p * NACC + t];
        }
        __syncthreads();
    }
    if (t < nacc) acc[t] = v;
    __syncthreads();
}

// The single evaluation's second launch: the summed (G, r, sum weight*rho, sum weight, n) -> out[0 .. nacc).
__global__ __launch_bounds__(SUM_THREADS) void photo_sum_kernel(const double* __restrict__ part, int n_part, int nacc, double* out) {
    __shared__ double acc[NACC];
    __shared__ double tile[SUM_TILE * NACC];
    sum_partials(part, n_part, nacc, tile, acc);
    if ((int)threadIdx.x < nacc) out[threadIdx.x] = acc[threadIdx.x];
}

// The batched evaluation's second launch, one workgroup per target: out[t * NACC ..] = the sum of target t's partials.
__global__ __launch_bounds__(SUM_THREADS) void photo_sum_multi_kernel(TgtSet ts, int p_max, int nacc, const double* __restrict__ ws,
                                                                      double* out) {
    const int t = (int)blockIdx.x, n_part = ts.t[t].n_part;
    if (n_part == 0) return;
    __shared__ double acc[NACC];
    __shared__ double tile[SUM_TILE * NACC];
    sum_partials(ws + (int64_t)t * slice_doubles(p_max), n_part, nacc, tile, acc);
    if ((int)threadIdx.x < nacc) out[(int64_t)t * NACC + threadIdx.x] = acc[threadIdx.x];
}

// (x, y) in normalised template coordinates through m, de-homogenised.
__device__ __forceinline__ void project(const double* m, double xn, double yn, double& u, double& v) {
    const double z = m[6] * xn + m[7] * yn + m[8];
    u = (m[0] * xn + m[1] * yn + m[2]) / z;
    v = (m[3] * xn + m[4] * yn + m[5]) / z;
}

// Iterate k of a refinement: sum the partials, record the iterate, apply the control rules in their order, solve G delta = r by
// Cholesky and step the state.  st: the device state (written by iterate 0 from `init`); result: the block the host reads.
// The solve runs on one lane with the system in registers (NU is a template argument, every loop unrolled): with run-time
// indices into LDS the factorisation alone took 27 us of dependent LDS round trips.
template <int NU>
__device__ __forceinline__ void step_iterate(const double* __restrict__ part, int n_part, int k, int iters, const Geom& gm,
                                             const State& init, int x1, int y1, int n_need, double eps, double* st,
                                             double* result) {
    constexpr int nu = NU;
    int* ctl = reinterpret_cast<int*>(st + ST_DOUBLES);
    if (k > 0 && ctl[0] != 0) return;                            // (uniform: the refinement has stopped)
    __shared__ double acc[NACC];
    __shared__ double tile[SUM_TILE * NACC];
    constexpr int tri = nu * (nu + 1) / 2;
    sum_partials(part, n_part, tri + nu + 3, tile, acc);
    if (threadIdx.x != 0) return;
    State s = k == 0 ? init : load_state(st);
    int best = k == 0 ? -1 : ctl[1];
    const int conv_at = k == 0 ? -1 : ctl[2];
    const double best_cost = k == 0 ? 0.0 : st[ST_BEST_COST];
    const double cs = acc[tri + nu], wsum = acc[tri + nu + 1], n = acc[tri + nu + 2];
    const double cost = sqrt(cs / wsum) / 3.0;
    // the record: W_k = M_k N / h33 with N: (x, y) -> ((x - cx) / s, (y - cy) / s)
    double W[9];
    for (int row = 0; row < 3; ++row) {
        const double a = s.m[3 * row] / gm.s, b = s.m[3 * row + 1] / gm.s;
        W[3 * row] = a, W[3 * row + 1] = b, W[3 * row + 2] = s.m[3 * row + 2] - (gm.cx * a + gm.cy * b);
    }
    const double h33 = W[8];
    double* rec = result + REC * (1 + k);
    for (int i = 0; i < 9; ++i) rec[i] = W[i] = W[i] / h33;
    rec[9] = s.g, rec[10] = s.b / 3.0, rec[11] = cost, rec[12] = n, rec[13] = nan(""), rec[14] = 0.0, rec[15] = 0.0;
    result[2] = (double)(k + 1);
    int stop = -1;                                               // (a status once the iteration stops)
    if (n < (double)n_need || !(wsum > 0.0)) stop = WOFT_PHOTO_TOO_FEW;
    if (stop < 0) {
        bool finite = isfinite(cost);
        for (int i = 0; i < tri + nu; ++i) finite = finite && isfinite(acc[i]);
        if (!finite) stop = WOFT_PHOTO_NONFINITE;
    }
    if (stop < 0) {
        if (best < 0 || cost < best_cost) {
            best = k;
            st[ST_BEST_COST] = cost;
            for (int i = 0; i < 9; ++i) result[3 + i] = W[i];
        }
        if (k == iters) stop = WOFT_PHOTO_MAX_ITERS_REACHED;
        else if (k == conv_at) stop = WOFT_PHOTO_CONVERGED;
    }
    double delta[NU_MAX];
    if (stop < 0) {
        // Cholesky G = L L^T in place (L(i, j) takes the slot of G(j, i) in the row-major upper triangle), no ridge; a pivot that
        // is not finite or <= 2^-40 of its diagonal entry: singular
        auto at = [](int j, int i) { return j * NU - j * (j - 1) / 2 + (i - j); };       // G(j, i), j <= i
        double A[tri], y[NU];
#pragma unroll
        for (int i = 0; i < tri; ++i) A[i] = acc[i];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
#pragma unroll
            for (int i = j; i < NU; ++i) {
                double v = A[at(j, i)];
#pragma unroll
                for (int q = 0; q < j; ++q) v = v - A[at(q, i)] * A[at(q, j)];
                if (i == j) {
                    ok = ok && isfinite(v) && v > A[at(j, j)] * 0x1p-40;
                    A[at(j, j)] = sqrt(v);
                } else {
                    A[at(j, i)] = v / A[at(j, j)];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NU; ++i) {                           // L y = r
            double v = acc[tri + i];
#pragma unroll
            for (int q = 0; q < i; ++q) v = v - A[at(q, i)] * y[q];
            y[i] = v / A[at(i, i)];
        }
#pragma unroll
        for (int i = NU - 1; i >= 0; --i) {                      // L^T delta = y
            double v = y[i];
#pragma unroll
            for (int q = i + 1; q < NU; ++q) v = v - A[at(i, q)] * y[q];
            y[i] = v / A[at(i, i)];
        }
#pragma unroll
        for (int i = 0; i < NU_MAX; ++i) delta[i] = 0.0;
#pragma unroll
        for (int i = 0; i < NU; ++i) {
            delta[i] = y[i];
            ok = ok && isfinite(y[i]);
        }
        if (!ok) stop = WOFT_PHOTO_SINGULAR;
    }
    if (stop < 0) {
        // M <- M Delta^-1, Delta = I + [[d0, d1, d2], [d3, d4, d5], [d6, d7, 0]]: the adjugate over the determinant
        const double a = 1.0 + delta[0], b = delta[1], c = delta[2], d = delta[3], e = 1.0 + delta[4], f = delta[5];
        const double g = delta[6], h = delta[7], i9 = 1.0;
        const double det = a * (e * i9 - f * h) - b * (d * i9 - f * g) + c * (d * h - e * g);
        double inv[9] = {(e * i9 - f * h) / det, (c * h - b * i9) / det, (b * f - c * e) / det,
                         (f * g - d * i9) / det, (a * i9 - c * g) / det, (c * d - a * f) / det,
                         (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
        State nx = s;
        for (int row = 0; row < 3; ++row)
            for (int col = 0; col < 3; ++col)
                nx.m[3 * row + col] = s.m[3 * row] * inv[col] + s.m[3 * row + 1] * inv[3 + col] + s.m[3 * row + 2] * inv[6 + col];
        nx.g = s.g + delta[8], nx.b = s.b + delta[9];
        // the largest move, in frame pixels, of the four corners of the mask's box
        double step = 0.0;
        for (int q = 0; q < 4; ++q) {
            const double px = (q == 1 || q == 2) ? (double)x1 : (double)gm.x0, py = q >= 2 ? (double)y1 : (double)gm.y0;
            const double xn = (px - gm.cx) / gm.s, yn = (py - gm.cy) / gm.s;
            double u0, v0, u1, v1;
            project(s.m, xn, yn, u0, v0);
            project(nx.m, xn, yn, u1, v1);
            const double dist = sqrt((u1 - u0) * (u1 - u0) + (v1 - v0) * (v1 - v0));
            step = (dist > step || dist != dist) ? dist : step;  // (a NaN sticks)
        }
        rec[13] = step;
        for (int i = 0; i < 9; ++i) st[i] = nx.m[i];
        st[9] = nx.g, st[10] = nx.b;
        ctl[2] = step < eps ? k + 1 : conv_at;
    } else if (k == 0) {
        ctl[2] = -1;
    }
    ctl[1] = best;
    result[1] = (double)best;
    if (stop >= 0) result[0] = (double)stop;
    ctl[0] = stop >= 0 ? 1 : 0;
}

template <int NU>
__global__ __launch_bounds__(SUM_THREADS) void photo_step_kernel(const double* __restrict__ part, int n_part, int k, int iters,
                                                                 Geom gm, State init, int x1, int y1, int n_need, double eps,
                                                                 double* st, double* result) {
    step_iterate<NU>(part, n_part, k, iters, gm, init, x1, y1, n_need, eps, st, result);
}

// Workgroup t: iterate k of target t on its own slice and result block -- its own state, stop, best and rule-6 iterate.  An
// inactive target's block gets {WOFT_PHOTO_SKIPPED, -1, 0} at iterate 0 and nothing else.
template <int NU>
__global__ __launch_bounds__(SUM_THREADS) void photo_step_multi_kernel(TgtSet ts, Geom shared, int p_max, int k, int iters,
                                                                       double eps, double* ws, double* result) {
    const int t = (int)blockIdx.x, n_part = ts.t[t].n_part;
    double* res = result + (int64_t)t * (REC * (iters + 2));
    if (n_part == 0) {
        if (k == 0 && threadIdx.x == 0) res[0] = (double)WOFT_PHOTO_SKIPPED, res[1] = -1.0, res[2] = 0.0;
        return;
    }
    double* part = ws + (int64_t)t * slice_doubles(p_max);
    State init;
#pragma unroll
    for (int i = 0; i < 9; ++i) init.m[i] = ts.t[t].m[i];
    init.g = ts.t[t].g, init.b = ts.t[t].b;
    const Geom gm = target_geom(shared, ts.t[t].x0, ts.t[t].y0, ts.t[t].x1, ts.t[t].y1);
    step_iterate<NU>(part, n_part, k, iters, gm, init, ts.t[t].x1, ts.t[t].y1, ts.t[t].n_need, eps, part + (int64_t)p_max * NACC, res);
}

int64_t n_partials(int32_t box_w, int32_t box_h, int32_t stride) {
    const int64_t nx = (box_w - 1) / stride + 1, ny = (box_h - 1) / stride + 1;
    return ceil_div64(nx * ny, WOFT_PHOTO_CHUNK);
}

template <typename TT, typename TF>
void launch_accum(int nu, const void* tmpl, const uint8_t* mask, const float* weights, const void* frame, const Geom& gm,
                  const State& init, const double* st_dev, const int* stop, double k3, double* part, int n_part, hipStream_t s) {
    const TT* t = static_cast<const TT*>(tmpl);
    const TF* f = static_cast<const TF*>(frame);
    if (nu == 10)
        hipLaunchKernelGGL((photo_accum_kernel<TT, TF, 10>), dim3((unsigned)n_part), dim3(THREADS), 0, s, t, mask, weights, f, gm,
                           init, st_dev, stop, k3, part);
    else
        hipLaunchKernelGGL((photo_accum_kernel<TT, TF, 8>), dim3((unsigned)n_part), dim3(THREADS), 0, s, t, mask, weights, f, gm,
                           init, st_dev, stop, k3, part);
}

void accum(int tmpl_f32, int frame_f32, int nu, const void* tmpl, const uint8_t* mask, const float* weights, const void* frame,
           const Geom& gm, const State& init, const double* st_dev, const int* stop, double k3, double* part, int n_part,
           hipStream_t s) {
    if (tmpl_f32 && frame_f32) launch_accum<float, float>(nu, tmpl, mask, weights, frame, gm, init, st_dev, stop, k3, part, n_part, s);
    else if (tmpl_f32) launch_accum<float, uint8_t>(nu, tmpl, mask, weights, frame, gm, init, st_dev, stop, k3, part, n_part, s);
    else if (frame_f32) launch_accum<uint8_t, float>(nu, tmpl, mask, weights, frame, gm, init, st_dev, stop, k3, part, n_part, s);
    else launch_accum<uint8_t, uint8_t>(nu, tmpl, mask, weights, frame, gm, init, st_dev, stop, k3, part, n_part, s);
}

// The checks every entry shares -> the geometry, the starting state (M = W N^-1) and the number of partials; false: WOFT_EINVAL.
bool prepare(const void* tmpl, const uint8_t* mask, int32_t h, int32_t w, const void* frame, int32_t hf, int32_t wf,
             const int32_t* box, int32_t stride, const double* W, double gain, double bias, double huber_k, const void* ws,
             Geom& gm, State& st, int& n_part) {
    if (!tmpl || !mask || !frame || !box || !W || !ws) return false;
    if (h < 3 || w < 3 || hf < 1 || wf < 1 || (int64_t)h * w >= (1ll << 31) || (int64_t)hf * wf >= (1ll << 31)) return false;
    const int x0 = box[0], y0 = box[1], x1 = box[2], y1 = box[3];
    if (x0 < 0 || y0 < 0 || x1 < x0 || y1 < y0 || x1 > w - 1 || y1 > h - 1 || stride < 1) return false;
    if (!(huber_k > 0.0) && !(huber_k < 0.0)) return false;                       // (negative: no Huber; zero, NaN: rejected)
    if (!isfinite(gain) || !isfinite(bias)) return false;
    for (int i = 0; i < 9; ++i)
        if (!isfinite(W[i])) return false;
    const int64_t np = n_partials(x1 - x0 + 1, y1 - y0 + 1, stride);
    if (np > 0x7fffffff) return false;
    n_part = (int)np;
    gm.h = h, gm.w = w, gm.hf = hf, gm.wf = wf, gm.x0 = x0, gm.y0 = y0, gm.stride = stride;
    gm.nx = (x1 - x0) / stride + 1, gm.ny = (y1 - y0) / stride + 1;
    gm.cx = (x0 + x1) / 2.0, gm.cy = (y0 + y1) / 2.0;
    const int ext = (x1 - x0) > (y1 - y0) ? (x1 - x0) : (y1 - y0);
    gm.s = (ext > 1 ? ext : 1) / 2.0;
    for (int row = 0; row < 3; ++row) {                                           // N^-1 = [[s, 0, cx], [0, s, cy], [0, 0, 1]]
        const double a = W[3 * row], b = W[3 * row + 1], c = W[3 * row + 2];
        st.m[3 * row] = gm.s * a, st.m[3 * row + 1] = gm.s * b, st.m[3 * row + 2] = (gm.cx * a + gm.cy * b) + c;
    }
    st.g = gain, st.b = bias;
    return true;
}

template <typename TT, typename TF>
void launch_accum_multi(int nu, const void* tmpl, const uint32_t* bits, const float* weights, const void* frame, const Geom& shared,
                        const TgtSet& ts, int n_targets, int p_max, int first, double k3, double* ws, hipStream_t s) {
    const TT* t = static_cast<const TT*>(tmpl);
    const TF* f = static_cast<const TF*>(frame);
    const dim3 grid((unsigned)p_max, (unsigned)n_targets);
    if (nu == 10)
        hipLaunchKernelGGL((photo_accum_multi_kernel<TT, TF, 10>), grid, dim3(THREADS), 0, s, t, bits, weights, f, shared, ts, p_max,
                           first, k3, ws);
    else
        hipLaunchKernelGGL((photo_accum_multi_kernel<TT, TF, 8>), grid, dim3(THREADS), 0, s, t, bits, weights, f, shared, ts, p_max,
                           first, k3, ws);
}

void accum_multi(int tmpl_f32, int frame_f32, int nu, const void* tmpl, const uint32_t* bits, const float* weights,
                 const void* frame, const Geom& shared, const TgtSet& ts, int n_targets, int p_max, int first, double k3, double* ws,
                 hipStream_t s) {
    if (tmpl_f32 && frame_f32)
        launch_accum_multi<float, float>(nu, tmpl, bits, weights, frame, shared, ts, n_targets, p_max, first, k3, ws, s);
    else if (tmpl_f32)
        launch_accum_multi<float, uint8_t>(nu, tmpl, bits, weights, frame, shared, ts, n_targets, p_max, first, k3, ws, s);
    else if (frame_f32)
        launch_accum_multi<uint8_t, float>(nu, tmpl, bits, weights, frame, shared, ts, n_targets, p_max, first, k3, ws, s);
    else
        launch_accum_multi<uint8_t, uint8_t>(nu, tmpl, bits, weights, frame, shared, ts, n_targets, p_max, first, k3, ws, s);
}

// prepare() for K targets: every target's box, state and threshold checked -- active or not -- and laid out for the kernels;
// p_max = the largest number of partials of any of the K boxes (the workspace's layout), any = some target is active.
// gains, biases, n_need: NULL = 1, 0, 0 for every target.  false: WOFT_EINVAL.
bool prepare_multi(const void* tmpl, const uint32_t* bits, int32_t h, int32_t w, const void* frame, int32_t hf, int32_t wf,
                   int32_t n_targets, const int32_t* boxes, int32_t stride, const double* W, const double* gains,
                   const double* biases, const int32_t* n_need, const int32_t* active, double huber_k, const void* ws, Geom& shared,
                   TgtSet& ts, int& p_max, bool& any) {
    if (!tmpl || !bits || !frame || !boxes || !W || !active || !ws) return false;
    if (n_targets < 1 || n_targets > WOFT_MULTI_MAX_TARGETS) return false;
    p_max = 0, any = false;
    for (int t = 0; t < n_targets; ++t) {
        Geom gm;
        State st;
        int n_part = 0;
        // (the mask argument of the single form's checks is only tested against NULL)
        if (!prepare(tmpl, reinterpret_cast<const uint8_t*>(bits), h, w, frame, hf, wf, boxes + 4 * t, stride, W + 9 * t,
                     gains ? gains[t] : 1.0, biases ? biases[t] : 0.0, huber_k, ws, gm, st, n_part))
            return false;
        if (n_need && n_need[t] < 0) return false;
        Tgt& tg = ts.t[t];
        tg.x0 = boxes[4 * t], tg.y0 = boxes[4 * t + 1], tg.x1 = boxes[4 * t + 2], tg.y1 = boxes[4 * t + 3];
        tg.n_need = n_need ? n_need[t] : 0;
        tg.n_part = active[t] != 0 ? n_part : 0;
        for (int i = 0; i < 9; ++i) tg.m[i] = st.m[i];
        tg.g = st.g, tg.b = st.b;
        p_max = n_part > p_max ? n_part : p_max;
        any = any || active[t] != 0;
        if (t == 0) shared = gm;                                                  // (h, w, hf, wf, stride: the shared fields)
    }
    return true;
}

}  // namespace

extern "C" int64_t woft_photo_ws_bytes(int32_t box_w, int32_t box_h, int32_t stride) {
    if (box_w < 1 || box_h < 1 || stride < 1) return -1;
    const int64_t np = n_partials(box_w, box_h, stride);
    if (np > 0x7fffffff) return -1;
    return (np * NACC + ST_DOUBLES + 2) * (int64_t)sizeof(double);
}

extern "C" int woft_photo_eval(const void* tmpl, int32_t tmpl_f32, const uint8_t* mask, int32_t h, int32_t w, const float* weights,
                               const void* frame, int32_t frame_f32, int32_t hf, int32_t wf, const int32_t* box, int32_t stride,
                               const double* W, double gain, double bias, int32_t gain_bias, double huber_k, void* ws, double* out,
                               void* stream) {
    Geom gm;
    State st;
    int n_part = 0;
    if (!out || !prepare(tmpl, mask, h, w, frame, hf, wf, box, stride, W, gain, bias, huber_k, ws, gm, st, n_part))
        return WOFT_EINVAL;
    const int nu = gain_bias ? 10 : 8;
    double* part = static_cast<double*>(ws);
    hipStream_t s = (hipStream_t)stream;
    accum(tmpl_f32, frame_f32, nu, tmpl, mask, weights, frame, gm, st, nullptr, nullptr, huber_k > 0.0 ? 3.0 * huber_k : -1.0, part,
          n_part, s);
    hipLaunchKernelGGL(photo_sum_kernel, dim3(1), dim3(SUM_THREADS), 0, s, part, n_part, nu * (nu + 1) / 2 + nu + 3, out);
    return woft_launch_status();
}

extern "C" int woft_photo_refine(const void* tmpl, int32_t tmpl_f32, const uint8_t* mask, int32_t h, int32_t w,
                                 const float* weights, const void* frame, int32_t frame_f32, int32_t hf, int32_t wf,
                                 const int32_t* box, int32_t stride, const double* W0, int32_t iters, int32_t gain_bias,
                                 double huber_k, int32_t n_need, double eps, void* ws, double* result, void* stream) {
    Geom gm;
    State st;
    int n_part = 0;
    if (!result || iters < 0 || iters > WOFT_PHOTO_MAX_ITERS || n_need < 0 || !(eps >= 0.0) || !isfinite(eps)) return WOFT_EINVAL;
    if (!prepare(tmpl, mask, h, w, frame, hf, wf, box, stride, W0, 1.0, 0.0, huber_k, ws, gm, st, n_part)) return WOFT_EINVAL;
    const int nu = gain_bias ? 10 : 8;
    const double k3 = huber_k > 0.0 ? 3.0 * huber_k : -1.0;
    double* part = static_cast<double*>(ws);
    double* st_dev = part + (int64_t)n_part * NACC;
    const int* stop = reinterpret_cast<const int*>(st_dev + ST_DOUBLES);
    hipStream_t s = (hipStream_t)stream;
    for (int k = 0; k <= iters; ++k) {
        accum(tmpl_f32, frame_f32, nu, tmpl, mask, weights, frame, gm, st, k == 0 ? nullptr : st_dev, k == 0 ? nullptr : stop, k3,
              part, n_part, s);
        if (nu == 10)
            hipLaunchKernelGGL(photo_step_kernel<10>, dim3(1), dim3(SUM_THREADS), 0, s, part, n_part, k, iters, gm, st, box[2], box[3],
                               n_need, eps, st_dev, result);
        else
            hipLaunchKernelGGL(photo_step_kernel<8>, dim3(1), dim3(SUM_THREADS), 0, s, part, n_part, k, iters, gm, st, box[2], box[3],
                               n_need, eps, st_dev, result);
    }
    return woft_launch_status();
}

extern "C" int64_t woft_photo_multi_ws_bytes(int32_t n_targets, int32_t p_max) {
    if (n_targets < 1 || p_max < 1) return -1;
    return (int64_t)n_targets * slice_doubles(p_max) * (int64_t)sizeof(double);
}

extern "C" int woft_photo_eval_multi(const void* tmpl, int32_t tmpl_f32, const uint32_t* bits, int32_t h, int32_t w,
                                     const float* weights, const void* frame, int32_t frame_f32, int32_t hf, int32_t wf,
                                     int32_t n_targets, const int32_t* boxes, int32_t stride, const double* W, const double* gains,
                                     const double* biases, const int32_t* active, int32_t gain_bias, double huber_k, void* ws,
                                     double* out, void* stream) {
    Geom shared;
    TgtSet ts = {};
    int p_max = 0;
    bool any = false;
    if (!out || !gains || !biases) return WOFT_EINVAL;
    if (!prepare_multi(tmpl, bits, h, w, frame, hf, wf, n_targets, boxes, stride, W, gains, biases, nullptr, active, huber_k, ws,
                       shared, ts, p_max, any))
        return WOFT_EINVAL;
    if (!any) return 0;
    const int nu = gain_bias ? 10 : 8;
    hipStream_t s = (hipStream_t)stream;
    accum_multi(tmpl_f32, frame_f32, nu, tmpl, bits, weights, frame, shared, ts, n_targets, p_max, 1,
                huber_k > 0.0 ? 3.0 * huber_k : -1.0, static_cast<double*>(ws), s);
    hipLaunchKernelGGL(photo_sum_multi_kernel, dim3((unsigned)n_targets), dim3(SUM_THREADS), 0, s, ts, p_max,
                       nu * (nu + 1) / 2 + nu + 3, static_cast<const double*>(ws), out);
    return woft_launch_status();
}

extern "C" int woft_photo_refine_multi(const void* tmpl, int32_t tmpl_f32, const uint32_t* bits, int32_t h, int32_t w,
                                       const float* weights, const void* frame, int32_t frame_f32, int32_t hf, int32_t wf,
                                       int32_t n_targets, const int32_t* boxes, int32_t stride, const double* W0,
                                       const int32_t* n_need, const int32_t* active, int32_t iters, int32_t gain_bias, double huber_k,
                                       double eps, void* ws, double* result, void* stream) {
    Geom shared;
    TgtSet ts = {};
    int p_max = 0;
    bool any = false;
    if (!result || !n_need || iters < 0 || iters > WOFT_PHOTO_MAX_ITERS || !(eps >= 0.0) || !isfinite(eps)) return WOFT_EINVAL;
    if (!prepare_multi(tmpl, bits, h, w, frame, hf, wf, n_targets, boxes, stride, W0, nullptr, nullptr, n_need, active, huber_k, ws,
                       shared, ts, p_max, any))
        return WOFT_EINVAL;
    if (!any) return 0;
    const int nu = gain_bias ? 10 : 8;
    const double k3 = huber_k > 0.0 ? 3.0 * huber_k : -1.0;
    double* wsd = static_cast<double*>(ws);
    hipStream_t s = (hipStream_t)stream;
    for (int k = 0; k <= iters; ++k) {
        accum_multi(tmpl_f32, frame_f32, nu, tmpl, bits, weights, frame, shared, ts, n_targets, p_max, k == 0, k3, wsd, s);
        if (nu == 10)
            hipLaunchKernelGGL(photo_step_multi_kernel<10>, dim3((unsigned)n_targets), dim3(SUM_THREADS), 0, s, ts, shared, p_max, k,
                               iters, eps, wsd, result);
        else
            hipLaunchKernelGGL(photo_step_multi_kernel<8>, dim3((unsigned)n_targets), dim3(SUM_THREADS), 0, s, ts, shared, p_max, k,
                               iters, eps, wsd, result);
    }
    return woft_launch_status();
}
