// Correspondence masking + order-preserving compaction + Sobol subsampling on the device
// (tracker/YAOF_tracker_single_control.py:287-327 `_mask_coords` / `_mask_coords_flow`;
//  configs/YAOFT_single_control_repRAFT_sub500_noreliableinl_wLSq.py:31-53 `subsampler`).
//
// Reference semantics reproduced exactly:
//   keep[i] = tmask[y_i][x_i]                                   (source pixel i = y_i * gw + x_i inside the mask)
//             and, when check_dst:  not (dx < 0 or dy < 0 or rint(dx) >= W or rint(dy) >= H)
//                                   and (pwmask == NULL or pwmask[rint(dy)][rint(dx)])
//   N = number kept; if n_draw == 0 or n_draw >= N: every kept correspondence is selected, else the
//   selected ranks are the DISTINCT values of (int32) rint(float32(N) * u_k), k < n_draw, in increasing
//   order (the reference sets a boolean mask: original order, duplicates collapse).
// Visibility (this project's own rule, not the reference's; DESIGN.md "Visibility mask in the tracker"): with a per-source-pixel
// probability vis[i] the GATE adds `and vis[i] > thr` to keep[i] (strict fp32 compare: NaN is dropped), the WEIGHT rule leaves
// keep[i] alone and writes w[k] * vis (vis alone without weights).  Both are template arguments of the kernels below: the
// instantiations without them are the code of the entry points that take no visibility.
// Three launches, no host round trip: (a) flags + per-1024 counts, (b) one workgroup: scan of the
// counts, N, sorted unique rank list, (c) ranks -> output slots.  Outputs are in the H-fit kernel's
// format: pa[k] = (dst_x, dst_y), pb[k] = (src_x, src_y), w[k].
#include "common.h"

namespace {

constexpr int CHUNK = 1024;          // pixels per workgroup in (a) and (c): 256 threads x 4 consecutive
constexpr int MAX_DRAW = 1024;

struct Ws {                          // int32 workspace layout
    int* hdr;                        // [0] N kept, [1] M selected, [2] all-mode
    int* counts;                     // [nb]
    int* offsets;                    // [nb]
    int* sel;                        // [MAX_DRAW] sorted unique ranks
    uint8_t* flags;                  // [n]
};
__host__ __device__ inline Ws ws_layout(int* ws, int nb) {
    Ws o;
    o.hdr = ws;
    o.counts = ws + 4;
    o.offsets = ws + 4 + nb;
    o.sel = ws + 4 + 2 * nb;
    o.flags = (uint8_t*)(ws + 4 + 2 * nb + MAX_DRAW);
    return o;
}

__device__ __forceinline__ int block_exclusive_scan(int v, int* total) {
    // 256 threads; returns exclusive prefix of v, *total = block sum
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < wave; ++k) base += wsum[k];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return base + inc - v;
}

// The correspondences live on the flow grid (gh x gw: the frame, or the frame cropped to a multiple of 8 with
// padding_mode 'crop', optical_flow/raft.py:235-247); the masks have the frame's size (mh x mw).
struct Geo {
    int gh, gw, mh, mw;
};

// the visibility gate: vis[i] is read only where the template mask (a byte) has already passed
struct Gate {
    const float* vis;
    float thr;
};

template <bool GATE>
__device__ __forceinline__ bool keep_flag(const float* __restrict__ dst, const uint8_t* __restrict__ tmask,
                                          const uint8_t* __restrict__ pwmask, const Geo g, int check_dst, int64_t i,
                                          int64_t n, const Gate v) {
    const int64_t mi = (g.gw == g.mw) ? i : (i / g.gw) * g.mw + (i % g.gw);
    bool keep = tmask[mi] != 0;
    if (GATE) {
        if (keep) keep = v.vis[i] > v.thr;           // (NaN compares false: dropped)
    }
    if (keep && check_dst) {
        const float dx = dst[i], dy = dst[n + i];
        // NaN compares false below; treat it as out of bounds explicitly
        const bool oob = !(dx >= 0.f) || !(dy >= 0.f) || rintf(dx) >= (float)g.mw || rintf(dy) >= (float)g.mh;
        keep = !oob;
        if (keep && pwmask != nullptr) keep = pwmask[(int64_t)rintf(dy) * g.mw + (int64_t)rintf(dx)] != 0;
    }
    return keep;
}

// flags only (the tracker's generic path: the host compacts with the boolean mask, as the reference does)
template <bool GATE>
__global__ __launch_bounds__(256) void flags_kernel(const float* __restrict__ dst, const uint8_t* __restrict__ tmask,
                                                    const uint8_t* __restrict__ pwmask, Geo g, int check_dst,
                                                    uint8_t* __restrict__ flags, Gate v) {
    const int64_t n = (int64_t)g.gh * g.gw;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = keep_flag<GATE>(dst, tmask, pwmask, g, check_dst, i, n, v) ? 1 : 0;
}

template <bool GATE>
__global__ __launch_bounds__(256) void select_flags_kernel(const float* __restrict__ dst, const uint8_t* __restrict__ tmask,
                                                           const uint8_t* __restrict__ pwmask, Geo g,
                                                           int check_dst, int* ws, int nb, Gate v) {
    const Ws s = ws_layout(ws, nb);
    const int64_t n = (int64_t)g.gh * g.gw;
    const int64_t i0 = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 4;
    int cnt = 0;
    uint8_t f[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t i = i0 + e;
        if (i >= n) continue;
        f[e] = keep_flag<GATE>(dst, tmask, pwmask, g, check_dst, i, n, v) ? 1 : 0;
        cnt += f[e];
    }
    if (i0 < n) {
        if (i0 + 3 < n) *(uchar4*)(s.flags + i0) = make_uchar4(f[0], f[1], f[2], f[3]);
        else for (int e = 0; e < 4 && i0 + e < n; ++e) s.flags[i0 + e] = f[e];
    }
    int total;
    block_exclusive_scan(cnt, &total);
    if (threadIdx.x == 0) s.counts[blockIdx.x] = total;
}

// The plan of ONE selection by one workgroup of 1024 threads: the body of `select_plan_kernel` (one selection per launch) and of
// `select_plan_multi_kernel` (one per workgroup) -- one piece of integer code.  selected / kept: where count[0] / count[1] go.
__device__ __forceinline__ void select_plan(const Ws s, int nb, const float* __restrict__ sobol_u, int n_draw, int cap,
                                            int* __restrict__ selected, int* __restrict__ kept) {
    __shared__ int part[1024];
    __shared__ int keys[MAX_DRAW];
    __shared__ int carry_s;
    const int t = threadIdx.x;
    // ---- exclusive scan of the per-chunk counts (chunks of 1024 with a running carry) ----------
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int b = b0 + t;
        const int v = (b < nb) ? s.counts[b] : 0;
        part[t] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int add = (t >= o) ? part[t - o] : 0;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        const int carry = carry_s;
        if (b < nb) s.offsets[b] = carry + part[t] - v;
        __syncthreads();
        if (t == 1023) carry_s = carry + part[1023];
        __syncthreads();
    }
    const int N = carry_s;
    const bool all = (n_draw == 0) || (n_draw >= N);
    // ---- Sobol ranks: rint(float(N) * u_k) in float32, sorted, duplicates removed ---------------
    int key = 0x7fffffff;
    if (!all && t < n_draw) {
        const int r = (int)rintf(__fmul_rn((float)N, sobol_u[t]));
        if (r >= 0 && r < N) key = r;
    }
    keys[t] = key;
    __syncthreads();
    for (int k = 2; k <= MAX_DRAW; k <<= 1)            // bitonic sort, ascending
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int ixj = t ^ j;
            if (ixj > t) {
                const int a = keys[t], b = keys[ixj];
                const bool up = (t & k) == 0;
                if ((a > b) == up) { keys[t] = b; keys[ixj] = a; }
            }
            __syncthreads();
        }
    const int mine = keys[t];
    const int uniq = (!all && mine != 0x7fffffff && (t == 0 || keys[t - 1] != mine)) ? 1 : 0;
    part[t] = uniq;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int add = (t >= o) ? part[t - o] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    if (uniq) s.sel[part[t] - 1] = mine;
    if (t == 0) {
        const int M = all ? N : part[1023];
        s.hdr[0] = N;
        s.hdr[1] = M;
        s.hdr[2] = all ? 1 : 0;
        selected[0] = M < cap ? M : cap;
        kept[0] = N;
    }
}

__global__ __launch_bounds__(1024) void select_plan_kernel(int* ws, int nb, const float* __restrict__ sobol_u, int n_draw,
                                                           int cap, int* __restrict__ count) {
    select_plan(ws_layout(ws, nb), nb, sobol_u, n_draw, cap, count, count + 1);
}

template <bool VIS_WEIGHT>
__global__ __launch_bounds__(256) void select_gather_kernel(const float* __restrict__ dst, const float* __restrict__ wgt,
                                                            int h, int w, const int* ws, int nb,
                                                            float* __restrict__ pa, float* __restrict__ pb,
                                                            float* __restrict__ wo, int cap, const float* __restrict__ vis) {
    const Ws s = ws_layout(const_cast<int*>(ws), nb);
    const int64_t n = (int64_t)h * w;
    const int64_t i0 = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 4;
    int f[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (i0 + e < n) f[e] = s.flags[i0 + e];
    const int cnt = f[0] + f[1] + f[2] + f[3];
    int total;
    int rank = s.offsets[blockIdx.x] + block_exclusive_scan(cnt, &total);
    const bool all = s.hdr[2] != 0;
    const int M = s.hdr[1];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (!f[e]) continue;
        const int r = rank++;
        int slot = r;
        if (!all) {                                  // binary search r in the sorted unique rank list
            int lo = 0, hi = M - 1;
            slot = -1;
            while (lo <= hi) {
                const int mid = (lo + hi) >> 1;
                const int v = s.sel[mid];
                if (v == r) { slot = mid; break; }
                if (v < r) lo = mid + 1; else hi = mid - 1;
            }
        }
        if (slot < 0 || slot >= cap) continue;
        const int64_t i = i0 + e;
        pa[2 * slot] = dst[i];
        pa[2 * slot + 1] = dst[n + i];
        pb[2 * slot] = (float)(i % w);
        pb[2 * slot + 1] = (float)(i / w);
        if (VIS_WEIGHT) {
            if (wo != nullptr) wo[slot] = (wgt != nullptr) ? __fmul_rn(wgt[i], vis[i]) : vis[i];
        } else {
            if (wo != nullptr) wo[slot] = (wgt != nullptr) ? wgt[i] : 1.f;
        }
    }
}

// ---- the same selection for n_targets template masks held as one bit plane ---------------------------------
// Workspace: per target the header / counts / offsets / rank list of the single selection (MWS_T(nb) int32 each), then one uint32
// of keep bits per pixel.  (a) the target-independent part of the keep rule once per pixel, AND-ed onto the pixel's mask bits;
// per chunk and target a count, by ballots: no atomics; (b) workgroup t plans target t; (c) a chunk's workgroup reads its keep
// bits once and walks the targets that kept anything in the chunk.
constexpr int MAX_TARGETS = WOFT_MULTI_MAX_TARGETS;
__host__ __device__ inline int64_t mws_stride(int nb) { return 4 + 2 * (int64_t)nb + MAX_DRAW; }
__host__ __device__ inline int64_t mws_bits_at(int nb, int n_targets) { return (mws_stride(nb) * n_targets + 3) / 4 * 4; }   // (16 B)
__host__ __device__ inline uint32_t* mws_bits(int* ws, int nb, int n_targets) { return (uint32_t*)(ws + mws_bits_at(nb, n_targets)); }

template <bool GATE>
__global__ __launch_bounds__(256) void select_flags_multi_kernel(const float* __restrict__ dst, const uint32_t* __restrict__ tbits,
                                                                 Geo g, int n_targets, int check_dst, int* ws, int nb, Gate v) {
    __shared__ int wcnt[4][MAX_TARGETS];
    uint32_t* __restrict__ keepbits = mws_bits(ws, nb, n_targets);
    const uint32_t live = n_targets >= 32 ? 0xffffffffu : ((1u << n_targets) - 1u);
    const int64_t n = (int64_t)g.gh * g.gw;
    const int64_t i0 = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t f[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t i = i0 + e;
        if (i >= n) continue;
        const int64_t mi = (g.gw == g.mw) ? i : (i / g.gw) * g.mw + (i % g.gw);
        uint32_t bits = tbits[mi] & live;
        if (bits != 0) {                                 // (the rest of keep_flag, with pwmask == NULL: the same for every target)
            bool keep = true;
            if (GATE) keep = v.vis[i] > v.thr;           // (NaN compares false: dropped)
            if (keep && check_dst) {
                const float dx = dst[i], dy = dst[n + i];
                const bool oob = !(dx >= 0.f) || !(dy >= 0.f) || rintf(dx) >= (float)g.mw || rintf(dy) >= (float)g.mh;
                keep = !oob;
            }
            if (!keep) bits = 0;
        }
        f[e] = bits;
    }
    if (i0 < n) {
        if (i0 + 3 < n) *(uint4*)(keepbits + i0) = make_uint4(f[0], f[1], f[2], f[3]);
        else for (int e = 0; e < 4 && i0 + e < n; ++e) keepbits[i0 + e] = f[e];
    }
    // per target: the wave's count by four ballots, kept by lane t; then the four waves' counts through LDS
    int mine = 0;
    for (int t = 0; t < n_targets; ++t) {
        int c = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) c += (int)__popcll(__ballot((f[e] >> t) & 1u));
        if (lane == t) mine = c;
    }
    if (lane < MAX_TARGETS) wcnt[wave][lane] = mine;
    __syncthreads();
    if ((int)threadIdx.x < n_targets) {
        const int t = threadIdx.x;
        ws[mws_stride(nb) * t + 4 + blockIdx.x] = wcnt[0][t] + wcnt[1][t] + wcnt[2][t] + wcnt[3][t];
    }
}

__global__ __launch_bounds__(1024) void select_plan_multi_kernel(int* ws, int nb, int n_targets, const float* __restrict__ sobol_u,
                                                                 int n_draw, int cap, int* __restrict__ count) {
    const int t = blockIdx.x;
    select_plan(ws_layout(ws + mws_stride(nb) * t, nb), nb, sobol_u, n_draw, cap, count + t, count + n_targets + t);
}

template <bool VIS_WEIGHT>
__global__ __launch_bounds__(256) void select_gather_multi_kernel(const float* __restrict__ dst, const float* __restrict__ wgt,
                                                                  int h, int w, int n_targets, const int* ws, int nb,
                                                                  float* __restrict__ pa, float* __restrict__ pb,
                                                                  float* __restrict__ wo, int cap, const float* __restrict__ vis) {
    const uint32_t* __restrict__ keepbits = mws_bits(const_cast<int*>(ws), nb, n_targets);
    const int64_t n = (int64_t)h * w;
    const int64_t i0 = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 4;
    uint32_t bits[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (i0 + e < n) bits[e] = keepbits[i0 + e];
    for (int t = 0; t < n_targets; ++t) {
        const Ws s = ws_layout(const_cast<int*>(ws) + mws_stride(nb) * t, nb);
        if (s.counts[blockIdx.x] == 0) continue;         // (uniform over the workgroup: target t kept nothing in this chunk)
        int f[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = (int)((bits[e] >> t) & 1u);
        const int cnt = f[0] + f[1] + f[2] + f[3];
        int total;
        int rank = s.offsets[blockIdx.x] + block_exclusive_scan(cnt, &total);
        const bool all = s.hdr[2] != 0;
        const int M = s.hdr[1];
        float* __restrict__ pa_t = pa + (int64_t)t * cap * 2;
        float* __restrict__ pb_t = pb + (int64_t)t * cap * 2;
        float* __restrict__ wo_t = (wo != nullptr) ? wo + (int64_t)t * cap : nullptr;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!f[e]) continue;
            const int r = rank++;
            int slot = r;
            if (!all) {                                  // binary search r in the sorted unique rank list
                int lo = 0, hi = M - 1;
                slot = -1;
                while (lo <= hi) {
                    const int mid = (lo + hi) >> 1;
                    const int v = s.sel[mid];
                    if (v == r) { slot = mid; break; }
                    if (v < r) lo = mid + 1; else hi = mid - 1;
                }
            }
            if (slot < 0 || slot >= cap) continue;
            const int64_t i = i0 + e;
            pa_t[2 * slot] = dst[i];
            pa_t[2 * slot + 1] = dst[n + i];
            pb_t[2 * slot] = (float)(i % w);
            pb_t[2 * slot + 1] = (float)(i / w);
            if (VIS_WEIGHT) {
                if (wo_t != nullptr) wo_t[slot] = (wgt != nullptr) ? __fmul_rn(wgt[i], vis[i]) : vis[i];
            } else {
                if (wo_t != nullptr) wo_t[slot] = (wgt != nullptr) ? wgt[i] : 1.f;
            }
        }
    }
}

// [a, a + na) and [b, b + nb) share a byte (a NULL shares none)
inline bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uint64_t pa = (uint64_t)(uintptr_t)a, pb = (uint64_t)(uintptr_t)b;
    return a != nullptr && b != nullptr && pa < pb + nb && pb < pa + na;
}

enum { VIS_NONE = 0, VIS_GATE = 1, VIS_WEIGHTED = 2 };

int launch_flags(const float* dst, const uint8_t* tmask, const uint8_t* pwmask, int32_t gh, int32_t gw, int32_t mh, int32_t mw,
                 int32_t check_dst, const float* vis, int32_t vis_mode, float vis_thr, uint8_t* flags, void* stream) {
    if (!tmask || !flags || gh <= 0 || gw <= 0 || gh > mh || gw > mw || (check_dst && !dst)) return WOFT_EINVAL;
    if (vis_mode < VIS_NONE || vis_mode > VIS_WEIGHTED || vis_thr != vis_thr) return WOFT_EINVAL;
    const int64_t n = (int64_t)gh * gw;
    const Geo g = {gh, gw, mh, mw};
    const Gate v = {vis, vis_thr};
    const dim3 grid((unsigned)((n + 255) / 256));
    if (vis != nullptr && vis_mode == VIS_GATE)
        hipLaunchKernelGGL(flags_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, dst, tmask, pwmask, g, check_dst, flags, v);
    else
        hipLaunchKernelGGL(flags_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, dst, tmask, pwmask, g, check_dst, flags, v);
    return woft_launch_status();
}

int launch_select(const float* dst, const float* w, const uint8_t* tmask, const uint8_t* pwmask, int32_t gh, int32_t gw,
                  int32_t mh, int32_t mw, int32_t check_dst, const float* sobol_u, int32_t n_draw, const float* vis,
                  int32_t vis_mode, float vis_thr, void* ws, float* pa, float* pb, float* wout, int32_t cap, int32_t* count,
                  void* stream) {
    if (!dst || !tmask || !ws || !pa || !pb || !count || gh <= 0 || gw <= 0 || gh > mh || gw > mw || cap <= 0)
        return WOFT_EINVAL;
    if (n_draw < 0 || n_draw > MAX_DRAW || (n_draw > 0 && !sobol_u)) return WOFT_EINVAL;
    if (vis_mode < VIS_NONE || vis_mode > VIS_WEIGHTED || vis_thr != vis_thr) return WOFT_EINVAL;
    if (vis == nullptr) vis_mode = VIS_NONE;
    const int64_t n = (int64_t)gh * gw;
    const int nb = (int)((n + CHUNK - 1) / CHUNK);
    const Geo g = {gh, gw, mh, mw};
    const Gate v = {vis, vis_thr};
    hipStream_t s = (hipStream_t)stream;
    if (vis_mode == VIS_GATE)
        hipLaunchKernelGGL(select_flags_kernel<true>, dim3(nb), dim3(256), 0, s, dst, tmask, pwmask, g, check_dst, (int*)ws, nb, v);
    else
        hipLaunchKernelGGL(select_flags_kernel<false>, dim3(nb), dim3(256), 0, s, dst, tmask, pwmask, g, check_dst, (int*)ws, nb, v);
    hipLaunchKernelGGL(select_plan_kernel, dim3(1), dim3(1024), 0, s, (int*)ws, nb, sobol_u, n_draw, cap, count);
    if (vis_mode == VIS_WEIGHTED)
        hipLaunchKernelGGL(select_gather_kernel<true>, dim3(nb), dim3(256), 0, s, dst, w, gh, gw, (const int*)ws, nb, pa, pb,
                           wout, cap, vis);
    else
        hipLaunchKernelGGL(select_gather_kernel<false>, dim3(nb), dim3(256), 0, s, dst, w, gh, gw, (const int*)ws, nb, pa, pb,
                           wout, cap, vis);
    return woft_launch_status();
}

}  // namespace

extern "C" int64_t woft_tc_select_multi_ws_bytes(int64_t n, int32_t n_targets) {
    if (n < 0 || n_targets < 1 || n_targets > MAX_TARGETS) return -1;
    const int64_t nb = (n + CHUNK - 1) / CHUNK;
    return (mws_bits_at((int)nb, n_targets) + (n + 3) / 4 * 4) * 4;
}

extern "C" int woft_tc_select_multi(const float* dst, const float* w, const uint32_t* tbits, int32_t gh, int32_t gw, int32_t mh,
                                    int32_t mw, int32_t n_targets, int32_t check_dst, const float* sobol_u, int32_t n_draw,
                                    const float* vis, int32_t vis_mode, float vis_thr, void* ws, float* pa, float* pb, float* wout,
                                    int32_t cap, int32_t* count, void* stream) {
    if (!dst || !tbits || !ws || !pa || !pb || !count || gh <= 0 || gw <= 0 || gh > mh || gw > mw || cap <= 0) return WOFT_EINVAL;
    if (n_targets < 1 || n_targets > MAX_TARGETS) return WOFT_EINVAL;
    if (n_draw < 0 || n_draw > MAX_DRAW || (n_draw > 0 && !sobol_u)) return WOFT_EINVAL;
    if (vis_mode < VIS_NONE || vis_mode > VIS_WEIGHTED || vis_thr != vis_thr) return WOFT_EINVAL;
    if (vis == nullptr) vis_mode = VIS_NONE;
    const int64_t n = (int64_t)gh * gw;
    if (n > ((int64_t)1 << 31) - CHUNK) return WOFT_EINVAL;      // (ranks and counts are int32)
    const int nb = (int)((n + CHUNK - 1) / CHUNK);
    // the outputs are written while inputs are still unread: none may share a byte with an input or with another output
    const uint64_t slots = (uint64_t)n_targets * (uint64_t)cap;
    const void* outs[5] = {pa, pb, wout, count, ws};
    const uint64_t nout[5] = {slots * 8u, slots * 8u, slots * 4u, (uint64_t)n_targets * 8u,
                              (uint64_t)woft_tc_select_multi_ws_bytes(n, n_targets)};
    const void* ins[5] = {dst, w, vis, tbits, sobol_u};
    const uint64_t nin[5] = {(uint64_t)n * 8u, (uint64_t)n * 4u, (uint64_t)n * 4u, (uint64_t)mh * (uint64_t)mw * 4u,
                             (uint64_t)n_draw * 4u};
    for (int a = 0; a < 5; ++a) {
        for (int b = 0; b < 5; ++b)
            if (overlap(outs[a], nout[a], ins[b], nin[b])) return WOFT_EINVAL;
        for (int b = a + 1; b < 5; ++b)
            if (overlap(outs[a], nout[a], outs[b], nout[b])) return WOFT_EINVAL;
    }
    const Geo g = {gh, gw, mh, mw};
    const Gate v = {vis, vis_thr};
    hipStream_t s = (hipStream_t)stream;
    if (vis_mode == VIS_GATE)
        hipLaunchKernelGGL(select_flags_multi_kernel<true>, dim3(nb), dim3(256), 0, s, dst, tbits, g, n_targets, check_dst, (int*)ws,
                           nb, v);
    else
        hipLaunchKernelGGL(select_flags_multi_kernel<false>, dim3(nb), dim3(256), 0, s, dst, tbits, g, n_targets, check_dst, (int*)ws,
                           nb, v);
    hipLaunchKernelGGL(select_plan_multi_kernel, dim3(n_targets), dim3(1024), 0, s, (int*)ws, nb, n_targets, sobol_u, n_draw, cap,
                       count);
    if (vis_mode == VIS_WEIGHTED)
        hipLaunchKernelGGL(select_gather_multi_kernel<true>, dim3(nb), dim3(256), 0, s, dst, w, gh, gw, n_targets, (const int*)ws, nb,
                           pa, pb, wout, cap, vis);
    else
        hipLaunchKernelGGL(select_gather_multi_kernel<false>, dim3(nb), dim3(256), 0, s, dst, w, gh, gw, n_targets, (const int*)ws, nb,
                           pa, pb, wout, cap, vis);
    return woft_launch_status();
}

extern "C" int64_t woft_tc_select_ws_bytes(int64_t n) {
    const int64_t nb = (n + CHUNK - 1) / CHUNK;
    return (4 + 2 * nb + MAX_DRAW) * 4 + ((n + 15) / 16) * 16;
}

extern "C" int woft_tc_flags(const float* dst, const uint8_t* tmask, const uint8_t* pwmask, int32_t gh, int32_t gw,
                             int32_t mh, int32_t mw, int32_t check_dst, uint8_t* flags, void* stream) {
    return launch_flags(dst, tmask, pwmask, gh, gw, mh, mw, check_dst, nullptr, VIS_NONE, 0.f, flags, stream);
}

extern "C" int woft_tc_flags_vis(const float* dst, const uint8_t* tmask, const uint8_t* pwmask, int32_t gh, int32_t gw,
                                 int32_t mh, int32_t mw, int32_t check_dst, const float* vis, int32_t vis_mode, float vis_thr,
                                 uint8_t* flags, void* stream) {
    return launch_flags(dst, tmask, pwmask, gh, gw, mh, mw, check_dst, vis, vis_mode, vis_thr, flags, stream);
}

extern "C" int woft_tc_select(const float* dst, const float* w, const uint8_t* tmask, const uint8_t* pwmask, int32_t gh,
                              int32_t gw, int32_t mh, int32_t mw, int32_t check_dst, const float* sobol_u,
                              int32_t n_draw, void* ws, float* pa, float* pb, float* wout, int32_t cap, int32_t* count,
                              void* stream) {
    return launch_select(dst, w, tmask, pwmask, gh, gw, mh, mw, check_dst, sobol_u, n_draw, nullptr, VIS_NONE, 0.f, ws, pa, pb,
                         wout, cap, count, stream);
}

extern "C" int woft_tc_select_vis(const float* dst, const float* w, const uint8_t* tmask, const uint8_t* pwmask, int32_t gh,
                                  int32_t gw, int32_t mh, int32_t mw, int32_t check_dst, const float* sobol_u,
                                  int32_t n_draw, const float* vis, int32_t vis_mode, float vis_thr, void* ws, float* pa,
                                  float* pb, float* wout, int32_t cap, int32_t* count, void* stream) {
    return launch_select(dst, w, tmask, pwmask, gh, gw, mh, mw, check_dst, sobol_u, n_draw, vis, vis_mode, vis_thr, ws, pa, pb,
                         wout, cap, count, stream);
}
