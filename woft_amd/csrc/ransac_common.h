// What the RANSAC estimators share (ransac.hip: homography, 4 model points; trs.hip: similarity, 2 model points): the SplitMix64
// index stream, cv2's adaptive iteration count and the rebuild of cv2's sequential selection loop from per-hypothesis counts.
#pragma once
#include "common.h"
#include <float.h>

namespace {

constexpr int SELT = 1024;          // threads of the selection workgroup

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

__device__ __forceinline__ int fit_n(const int* count, int n_max) { return count ? min(count[0], n_max) : n_max; }

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ int draw_index(uint64_t key, int k, uint32_t c, int n) {
    const uint64_t u = splitmix64(key ^ (((uint64_t)(uint32_t)k << 32) | c));
    return (int)(((u >> 32) * (uint64_t)n) >> 32);
}

// RANSACUpdateNumIters(conf, (n - m) / n, MP, max_iters), the published formula; (1 - ep)^MP by squarings (MP = 2 or 4)
template <int MP>
__device__ int update_num_iters(double conf, int n, int m, int max_iters) {
    static_assert(MP == 2 || MP == 4, "model points");
    const double p = fmin(fmax(conf, 0.0), 1.0);
    const double ep = fmin(fmax((double)(n - m) / (double)n, 0.0), 1.0);
    const double t = 1.0 - ep, t2 = t * t;
    double num = fmax(1.0 - p, DBL_MIN);
    double denom = 1.0 - (MP == 4 ? t2 * t2 : t2);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return (denom >= 0.0 || -num >= (double)max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}

template <int MP>
__device__ __forceinline__ int niters_after(int m, double conf, int n, int max_iters) {
    return m > MP - 1 ? min(max_iters, update_num_iters<MP>(conf, n, m, max_iters)) : max_iters;
}

// One workgroup of SELT threads, all of them calling: cv2's sequential loop over counts[0 .. max_iters) (a new best needs
// count > max(best, MP - 1); niters is updated after it; the loop ends at the first k >= niters or at the first negative count,
// a hypothesis without a sample) -> stop = iterations run, best = the last new best before the stop (-1: none).
template <int MP>
__device__ void sequential_select(const int* __restrict__ counts, int max_iters, double conf, int n, int& stop, int& best) {
    __shared__ int scan[SELT];
    __shared__ int stop_s, best_s;
    const int tid = threadIdx.x;
    const int per = (max_iters + SELT - 1) / SELT;
    const int b0 = min(max_iters, tid * per), b1 = min(max_iters, b0 + per);
    int segmax = 0;
    for (int k = b0; k < b1; ++k) segmax = max(segmax, counts[k]);
    scan[tid] = segmax;
    if (tid == 0) { stop_s = max_iters; best_s = -1; }
    __syncthreads();
    for (int o = 1; o < SELT; o <<= 1) {                    // inclusive prefix max
        const int v = tid >= o ? scan[tid - o] : 0;
        __syncthreads();
        scan[tid] = max(scan[tid], v);
        __syncthreads();
    }
    const int before = tid > 0 ? scan[tid - 1] : 0;          // max of the counts ahead of this thread's segment
    // stop: the first k with k >= niters(after k-1) or no sample at k
    int m = before;
    for (int k = b0; k < b1; ++k) {
        const int c = counts[k];
        if (k >= niters_after<MP>(m, conf, n, max_iters) || c < 0) {
            atomicMin(&stop_s, k);
            break;
        }
        m = max(m, c);
    }
    __syncthreads();
    const int S = stop_s;
    // best: the last record (count > max(best, MP - 1)) before the stop = the first index reaching the final maximum
    m = before;
    int last = -1;
    for (int k = b0; k < min(b1, S); ++k) {
        const int c = counts[k];
        if (c > max(m, MP - 1)) { m = c; last = k; }
    }
    if (last >= 0) atomicMax(&best_s, last);
    __syncthreads();
    stop = S;
    best = best_s;
}

}  // namespace
