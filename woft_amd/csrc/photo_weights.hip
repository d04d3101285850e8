// A fold result as the weight map of the photometric refinement (woft_photo_weights): per template pixel the
// gate (or the soft weight exp(-cost) * vis) of the chained fold, eroded by a (2 radius + 1)^2 minimum, and per target the number
// of its mask's pixels the map leaves positive.  Streaming: 8 B of planes and 4 B of bits read, 4 B of map written per pixel.  One
// 64 x 16 tile plus its halo goes through LDS, the minimum is separable: rows first, then columns.  The map has one writer per
// pixel and the counts are integer sums (ballot + population count, integer atomics), so two calls give equal bytes.
#include <math.h>
#include "common.h"

namespace {

constexpr int TW = 64, TH = 16, THREADS = 256, ROWS_PER_LANE = TH / (THREADS / TW);
constexpr int RMAX = WOFT_PHOTO_WEIGHTS_MAX_RADIUS;
// Every workgroup ends in up to n_targets atomics on the same counters, and those serialise (the lesson of woft_chain_tc's
// histogram): the grid is cut to about this many workgroups and a workgroup walks the remaining tiles of its column.
constexpr int PW_BLOCKS = 2048;
static_assert(TW == 64, "a wavefront is one row of a tile: the ballots below count a row's 64 pixels");
static_assert(WOFT_MULTI_MAX_TARGETS <= 64, "lane t keeps target t's count");

struct Planes {
    const float* cost;
    const float* vis;
    int rows, cols, ry, rx, h, w;
    float vis_thr;
    int soft;
};

// raw(x, y) of the header; +inf outside the template: the minimum ignores it.
__device__ __forceinline__ float raw_at(const Planes& P, int x, int y) {
    if (x < 0 || x >= P.w || y < 0 || y >= P.h) return INFINITY;
    const int yy = y - P.ry, xx = x - P.rx;
    if (yy < 0 || yy >= P.rows || xx < 0 || xx >= P.cols) return 0.f;
    const int64_t p = (int64_t)yy * P.cols + xx;
    const float c = P.cost[p], v = P.vis[p];
    if (!(isfinite(c) && v >= P.vis_thr)) return 0.f;            // (a NaN v fails the comparison)
    if (!P.soft) return 1.f;
    const float r = expf(-c) * v;
    return (isfinite(r) && r > 0.f) ? r : 0.f;
}

__device__ __forceinline__ float min2(float a, float b) { return b < a ? b : a; }    // (no NaN reaches it)

template <int R>
__global__ __launch_bounds__(THREADS) void photo_weights_kernel(Planes P, const uint32_t* __restrict__ bits, int n_targets,
                                                                float* __restrict__ map, int32_t* __restrict__ support) {
    constexpr int LW = TW + 2 * R, LH = TH + 2 * R;
    __shared__ float s_raw[LH * LW];
    __shared__ float s_row[LH * TW];                             // the minimum over a row's 2 R + 1 neighbours
    __shared__ int32_t s_cnt[WOFT_MULTI_MAX_TARGETS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < WOFT_MULTI_MAX_TARGETS) s_cnt[tid] = 0;
    const uint32_t live = n_targets >= 32 ? 0xffffffffu : ((1u << n_targets) - 1u);
    const int x0 = (int)blockIdx.x * TW;
    const int tiles_y = (P.h + TH - 1) / TH;
    int mine = 0;                                                // lane t: target t's count over this wavefront's rows
    for (int ty = (int)blockIdx.y; ty < tiles_y; ty += (int)gridDim.y) {
        const int y0 = ty * TH;
        if (R > 0) {
            for (int i = tid; i < LH * LW; i += THREADS) {
                const int ly = i / LW, lx = i - ly * LW;
                s_raw[i] = raw_at(P, x0 - R + lx, y0 - R + ly);
            }
            __syncthreads();
            for (int i = tid; i < LH * TW; i += THREADS) {
                const int ly = i / TW, lx = i - ly * TW;
                float m = s_raw[ly * LW + lx];
#pragma unroll
                for (int d = 1; d <= 2 * R; ++d) m = min2(m, s_raw[ly * LW + lx + d]);
                s_row[i] = m;
            }
            __syncthreads();
        }
        // (the next tile's writes of s_raw and s_row come after its own barriers: each has one between it and these reads)
        const int x = x0 + lane;
#pragma unroll
        for (int j = 0; j < ROWS_PER_LANE; ++j) {
            const int ly = wave + j * (THREADS / TW), y = y0 + ly;
            uint32_t b = 0;
            if (x < P.w && y < P.h) {
                float m;
                if (R > 0) {
                    m = s_row[ly * TW + lane];
#pragma unroll
                    for (int d = 1; d <= 2 * R; ++d) m = min2(m, s_row[(ly + d) * TW + lane]);
                } else {
                    m = raw_at(P, x, y);
                }
                const int64_t o = (int64_t)y * P.w + x;
                map[o] = m;
                if (n_targets > 0 && m > 0.f) b = bits[o] & live;
            }
            if (n_targets > 0) {
                // one ballot per target PRESENT in the wavefront's row, not per target: the targets of the first lane that still
                // has uncounted ones are taken off every lane's list (32 ballots per row were 5.3 times the streaming floor at
                // 1080p with 32 boxes of a quarter side; every value below is wavefront-uniform)
                uint32_t rest = b;
                uint64_t open;
                while ((open = __ballot(rest != 0)) != 0) {
                    const int lead = __ffsll((unsigned long long)open) - 1;
                    const uint32_t these = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)rest, lead));
                    for (uint32_t left = these; left != 0; left &= left - 1) {
                        const int t = __ffs(left) - 1;
                        const uint64_t hit = __ballot((b >> t) & 1u);
                        if (lane == t) mine += (int)__popcll(hit);
                    }
                    rest &= ~these;
                }
            }
        }
    }
    if (n_targets > 0) {
        __syncthreads();                                         // (s_cnt's zeros)
        if (mine != 0) atomicAdd(&s_cnt[lane], mine);            // (mine != 0 only for lanes < n_targets)
        __syncthreads();
        if (tid < n_targets && s_cnt[tid] != 0) atomicAdd(&support[tid], s_cnt[tid]);
    }
}

// [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uint64_t pa = (uint64_t)(uintptr_t)a, pb = (uint64_t)(uintptr_t)b;
    return a != nullptr && b != nullptr && pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" int woft_photo_weights(const float* cost, const float* vis, int32_t rows, int32_t cols, int32_t ry, int32_t rx, int32_t h,
                                  int32_t w, const uint32_t* bits, int32_t n_targets, float vis_thr, int32_t mode, int32_t radius,
                                  float* map, int32_t* support, void* stream) {
    if (!cost || !vis || !map || rows < 1 || cols < 1 || h < 1 || w < 1 || (int64_t)h * w >= (1ll << 31)) return WOFT_EINVAL;
    if (ry < 0 || rx < 0 || (int64_t)ry + rows > h || (int64_t)rx + cols > w) return WOFT_EINVAL;
    if (n_targets < 0 || n_targets > WOFT_MULTI_MAX_TARGETS || (n_targets > 0 && (!bits || !support))) return WOFT_EINVAL;
    if (!(vis_thr >= 0.f && vis_thr <= 1.f) || (mode != 0 && mode != 1) || radius < 0 || radius > RMAX) return WOFT_EINVAL;
    // the map is written while other pixels' inputs are still unread
    const uint64_t mb = (uint64_t)h * (uint64_t)w * 4u, pb = (uint64_t)rows * (uint64_t)cols * 4u;
    const uint64_t sb = (uint64_t)n_targets * sizeof(int32_t);
    if (overlap(map, mb, cost, pb) || overlap(map, mb, vis, pb)) return WOFT_EINVAL;
    if (n_targets > 0 && (overlap(map, mb, bits, mb) || overlap(map, mb, support, sb) || overlap(support, sb, bits, mb) ||
                          overlap(support, sb, cost, pb) || overlap(support, sb, vis, pb)))
        return WOFT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n_targets > 0 && hipMemsetAsync(support, 0, sb, s) != hipSuccess) return WOFT_ELAUNCH;
    const Planes P = {cost, vis, rows, cols, ry, rx, h, w, vis_thr, mode};
    const unsigned tiles_x = (unsigned)((w + TW - 1) / TW), tiles_y = (unsigned)((h + TH - 1) / TH);
    const unsigned per_col = PW_BLOCKS / tiles_x;
    const dim3 grid(tiles_x, tiles_y < per_col ? tiles_y : (per_col > 0 ? per_col : 1u));
    const uint32_t* b = n_targets > 0 ? bits : nullptr;
    switch (radius) {
    case 0: hipLaunchKernelGGL(photo_weights_kernel<0>, grid, dim3(THREADS), 0, s, P, b, n_targets, map, support); break;
    case 1: hipLaunchKernelGGL(photo_weights_kernel<1>, grid, dim3(THREADS), 0, s, P, b, n_targets, map, support); break;
    case 2: hipLaunchKernelGGL(photo_weights_kernel<2>, grid, dim3(THREADS), 0, s, P, b, n_targets, map, support); break;
    case 3: hipLaunchKernelGGL(photo_weights_kernel<3>, grid, dim3(THREADS), 0, s, P, b, n_targets, map, support); break;
    default: hipLaunchKernelGGL(photo_weights_kernel<4>, grid, dim3(THREADS), 0, s, P, b, n_targets, map, support); break;
    }
    return woft_launch_status();
}
