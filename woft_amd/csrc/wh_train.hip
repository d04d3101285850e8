// Training of the weight head (weighted_raft.py:318-384) on a compacted list of 9x9 windows: the un-fused forward layers that
// keep their activations, and the backward of every stage from the x8 convex upsampling down to the first conv's weights
// (DESIGN.md section 17).  Exact fp32 throughout: the products run on v_mfma_f32_32x32x2_f32 (bit for bit a k-ordered fmaf chain)
// or on the vector ALUs.  Every sum is deterministic: no floating-point atomics, split reductions are written as partials and
// added in a fixed order.
//
// Layouts: activations [window][81 positions][128 channels] (the first layer's input [window][81][8], woft_wh_pack's patches);
// forward weights wt[tap = ky * 3 + kx][ci][co]; parameter gradients in the state dict's [co][ci][ky][kx].
#include "common.h"

namespace {

constexpr int WHT_NW = 9, WHT_T = 81, WHT_C = 128;
constexpr int WHT_CHUNK = WOFT_WH_TRAIN_CHUNK;             // windows per partial sum of the parameter gradients

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// row of accumulator register r in a 32x32 tile (the column is lane & 31)
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// ---- 3x3 conv CIN -> 128 on 9x9 windows, each window zero-padded on its own ---------------------------------------------------
//   y[p][t][co] = epi(sum_{tap, ci} x[p][t + tap][ci] * wt[tap][ci][co])
//   epi: + bias[co], ReLU (forward layer: bias != NULL) | * (gate[p][t][co] > 0) (data gradient: the transposed, flipped filter
//   in wt, gate = the activation the gradient flows into)
// One workgroup per window at a time: the window sits in LDS with a zero border of one position (11 x 11 positions, channel
// stride CIN + 1 floats so that the 32 positions a wave reads at one channel fall into 32 banks).  Wave w owns output channels
// 32 w .. 32 w + 31 and all three 32-position row tiles (positions 81 .. 95 are padding and are not stored).
template <int CIN>
__global__ __launch_bounds__(256) void wht_conv_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                       const float* __restrict__ bias, const float* __restrict__ gate, int n_win,
                                                       float* __restrict__ y) {
    constexpr int S = CIN + 1;
    __shared__ float xs[121 * S];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, kh = lane >> 5;
    for (int k = tid; k < 121 * S; k += 256) xs[k] = 0.f;                 // (the border stays zero: only the interior is rewritten)
    int base[3];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {
        const int m = mt * 32 + i, mm = m < WHT_T ? m : 0;
        base[mt] = ((mm / 9) * 11 + mm % 9) * S;                          // top-left of the 3x3 neighbourhood, padded coordinates
    }
    const int co = 32 * wave + i;
    for (int p = blockIdx.x; p < n_win; p += gridDim.x) {
        __syncthreads();
        const float* __restrict__ xp = x + (int64_t)p * (WHT_T * CIN);
        for (int k = tid; k < WHT_T * CIN; k += 256) {
            const int t = k / CIN, c = k - t * CIN;
            xs[((t / 9 + 1) * 11 + t % 9 + 1) * S + c] = xp[k];
        }
        __syncthreads();
        // (one fma chain per tap, CIN products long, added to the total on the vector ALUs: a single chain over all 9 * CIN
        //  products carries three times the rounding error)
        f32x16 acc[3];
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int off = ((tap / 3) * 11 + tap % 3) * S + kh;
            const float* __restrict__ wtap = wt + ((int64_t)tap * CIN + kh) * WHT_C + co;
            f32x16 part[3];
#pragma unroll
            for (int mt = 0; mt < 3; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) part[mt][r] = 0.f;
#pragma unroll 4
            for (int kk = 0; kk < CIN / 2; ++kk) {
                const float b = wtap[(2 * kk) * WHT_C];
#pragma unroll
                for (int mt = 0; mt < 3; ++mt) part[mt] = mfma32(xs[base[mt] + off + 2 * kk], b, part[mt]);
            }
#pragma unroll
            for (int mt = 0; mt < 3; ++mt) acc[mt] += part[mt];
        }
        const float bv = bias ? bias[co] : 0.f;
        const int64_t o = (int64_t)p * (WHT_T * WHT_C) + co;
#pragma unroll
        for (int mt = 0; mt < 3; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mt * 32 + acc_row(r, lane);
                if (m >= WHT_T) continue;
                float v = acc[mt][r];
                if (bias) v = fmaxf(v + bv, 0.f);
                if (gate) v = gate[o + m * WHT_C] > 0.f ? v : 0.f;
                y[o + m * WHT_C] = v;
            }
    }
}

// ---- weight gradient of a 3x3 layer CIN -> 128 ---------------------------------------------------------------------------------
//   part_w[chunk][tap][co][ci] = sum over the chunk's windows p and positions t of gy[p][t][co] * x[p][t + tap][ci]
//   part_b[chunk][co]          = sum over the chunk's windows and positions of gy[p][t][co]          (written by the tap-0 blocks)
// grid (9 taps, chunks of WHT_CHUNK windows).  Wave w owns output channels 32 w .. 32 w + 31 (the M index, operand A = gy) and
// every 32-channel tile of ci (the N index, operand B = x): a 128 x CIN fp32 accumulator per workgroup, 64 registers per lane at
// CIN = 128.  The K index runs over the positions in pairs (lane half kh takes position 2 tt + kh; position 81 is a zero pad) and
// then over the windows.
// Operand B is shared by the four waves: the window's x sits in LDS with a zero border of one position (11 x 11 positions of CIN
// floats; lanes differ in the channel, so a read is conflict free), which is also what keeps a tap from reading the window next
// to it in memory.  Operand A is private to a lane (every gy element is read by exactly one lane of the workgroup): its 41 values
// per window are loaded into registers.  Both are fetched one window ahead -- the loads of window p + 1 are issued before the
// matrix loop of window p and land while it runs.
template <int CIN>
__global__ __launch_bounds__(256) void wht_wgrad_kernel(const float* __restrict__ gy, const float* __restrict__ x, int n_win,
                                                        float* __restrict__ part_w, float* __restrict__ part_b) {
    constexpr int NT = CIN >= 32 ? CIN / 32 : 1;
    constexpr int NSTEP = (WHT_T + 1) / 2;                              // 41 K steps of two positions per window
    constexpr int NV4 = WHT_T * CIN / 4;                                // float4s of one window of x
    constexpr int NL = (NV4 + 255) / 256;                               // ... per thread
    __shared__ __attribute__((aligned(16))) float xs[121 * CIN];
    const int tap = blockIdx.x, chunk = blockIdx.y;
    const int ky = tap / 3, kx = tap % 3;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, kh = lane >> 5;
    const int co = 32 * wave + i;
    for (int k = tid; k < 121 * CIN; k += 256) xs[k] = 0.f;            // (the border stays zero: only the interior is rewritten)
    int dst[NL];                                                        // where this thread's float4s of a window go in LDS
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int e = (tid + 256 * j) * 4, t = e / CIN, c = e - t * CIN;
        dst[j] = ((t / 9 + 1) * 11 + t % 9 + 1) * CIN + c;
    }
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
    double bsum = 0.0;                                                  // (bias gradient: this lane's gy values, in fp64)
    const int p0 = chunk * WHT_CHUNK, p1 = min(p0 + WHT_CHUNK, n_win);
    f32x4 xr[NL];
    float av[NSTEP];
    auto fetch = [&](int p) {
        const f32x4* __restrict__ xp = (const f32x4*)(x + (int64_t)p * (WHT_T * CIN));
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int k = tid + 256 * j;
            xr[j] = k < NV4 ? xp[k] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float* __restrict__ gyp = gy + (int64_t)p * (WHT_T * WHT_C) + co;
#pragma unroll
        for (int tt = 0; tt < NSTEP; ++tt) {
            const int t = 2 * tt + kh;
            av[tt] = t < WHT_T ? gyp[(t < WHT_T ? t : 0) * WHT_C] : 0.f;
        }
    };
    if (p0 < p1) fetch(p0);
    for (int p = p0; p < p1; ++p) {
        __syncthreads();                                                // (every wave is done with the previous window in LDS)
#pragma unroll
        for (int j = 0; j < NL; ++j)
            if (tid + 256 * j < NV4) *(f32x4*)(xs + dst[j]) = xr[j];
        float a[NSTEP];
#pragma unroll
        for (int tt = 0; tt < NSTEP; ++tt) {
            a[tt] = av[tt];
            bsum += (double)a[tt];
        }
        __syncthreads();
        if (p + 1 < p1) fetch(p + 1);
        f32x16 part[NT];                                  // (one fma chain per window, added to the chunk's total on the vector ALUs)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) part[nt][r] = 0.f;
#pragma unroll
        for (int tt = 0; tt < NSTEP; ++tt) {
            const int t = 2 * tt + kh;
            const bool tv = t < WHT_T;
            const int tc = tv ? t : 0;
            const int pos = ((tc / 9 + ky) * 11 + tc % 9 + kx) * CIN;  // padded coordinates: (ty + 1 + ky - 1, tx + 1 + kx - 1)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int ci = nt * 32 + i;
                const float bv = xs[pos + (ci < CIN ? ci : 0)];
                part[nt] = mfma32(a[tt], (tv && ci < CIN) ? bv : 0.f, part[nt]);
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] += part[nt];
    }
    float* __restrict__ pw = part_w + ((int64_t)chunk * 9 + tap) * (WHT_C * CIN);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * wave + acc_row(r, lane), ci = nt * 32 + i;
            if (ci < CIN) pw[row * CIN + ci] = acc[nt][r];
        }
    const double other = __shfl_xor(bsum, 32);
    if (tap == 0 && kh == 0) part_b[chunk * WHT_C + co] = (float)(bsum + other);      // (even positions + odd positions)
}

// gw[co][ci][tap] (ci < cin_out <= cin) = sum over the chunks, in order, in fp64;  gb[co] alike
__global__ void wht_wgrad_sum_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b, int n_chunks, int cin,
                                     int cin_out, float* __restrict__ gw, float* __restrict__ gb) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_w = WHT_C * cin_out * 9;
    if (e < n_w) {
        const int tap = e % 9, ci = (e / 9) % cin_out, co = e / (9 * cin_out);
        const float* __restrict__ src = part_w + ((int64_t)tap * WHT_C + co) * cin + ci;
        double s = 0.0;
        for (int c = 0; c < n_chunks; ++c) s += (double)src[(int64_t)c * 9 * WHT_C * cin];
        gw[e] = (float)s;
    } else if (e < n_w + WHT_C) {
        const int co = e - n_w;
        double s = 0.0;
        for (int c = 0; c < n_chunks; ++c) s += (double)part_b[c * WHT_C + co];
        gb[co] = (float)s;
    }
}

// ---- closing 1x1 conv + mean over the 81 positions, backward -------------------------------------------------------------------
//   g = g_wlow[index[p]] / 81;  g_act[p][t][c] = g * w6[c] * (act[p][t][c] > 0)
//   part[chunk][c] = sum_{p, t} g * act[p][t][c]   (c < 128),   part[chunk][128] = sum_p g_wlow[index[p]]      (fp64 partials)
__global__ __launch_bounds__(128) void wht_reduce_bwd_kernel(const float* __restrict__ act, const float* __restrict__ w6,
                                                             const float* __restrict__ g_wlow, const int* __restrict__ index,
                                                             int n_win, float* __restrict__ g_act, double* __restrict__ part) {
    const int c = threadIdx.x, chunk = blockIdx.x;
    const float wc = w6[c];
    const int p0 = chunk * WHT_CHUNK, p1 = min(p0 + WHT_CHUNK, n_win);
    double sw = 0.0, sb = 0.0;
    for (int p = p0; p < p1; ++p) {
        const float gl = g_wlow[index ? index[p] : p];
        const float g = gl / (float)WHT_T;
        const float gw = g * wc;
        sb += (double)gl;
        const int64_t o = (int64_t)p * (WHT_T * WHT_C) + c;
        float s = 0.f;
        for (int t = 0; t < WHT_T; ++t) {
            const float a = act[o + t * WHT_C];
            g_act[o + t * WHT_C] = a > 0.f ? gw : 0.f;
            s += a;
        }
        sw += (double)g * (double)s;
    }
    part[(int64_t)chunk * (WHT_C + 1) + c] = sw;
    if (c == 0) part[(int64_t)chunk * (WHT_C + 1) + WHT_C] = sb;
}
__global__ void wht_reduce_sum_kernel(const double* __restrict__ part, int n_chunks, float* __restrict__ g_w6,
                                      float* __restrict__ g_b6) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > WHT_C) return;
    double s = 0.0;
    for (int k = 0; k < n_chunks; ++k) s += part[(int64_t)k * (WHT_C + 1) + c];
    if (c < WHT_C) g_w6[c] = (float)s;
    else g_b6[0] = (float)s;
}

// ---- x8 convex upsampling of the weight map at a list of pixels, backward (upsample.hip: convex_weights_at_kernel) -------------
// One thread per window (1/8-resolution cell index[j], or cell j): it walks over the points in their order and adds what each
// point whose 3x3 support holds the cell sends back -- a gather, so several points in one cell, or one point twice, need no
// atomics and always add up in the same order.
//   forward: v = (sum_k s_k * (8 * wlow[q_k])) / 8, out = v or sigmoid(v);  backward: g_wlow[q_k] += ((g_out * dsig) / 8) * (s_k * 8)
__global__ void convex_weights_at_bwd_kernel(const float* __restrict__ pts, const int* __restrict__ count, int n_max,
                                             const float* __restrict__ g_wsel, const float* __restrict__ wlow,
                                             const float* __restrict__ mask, int ld_mask, int hf, int wf, int crop_top,
                                             int crop_left, int do_sigmoid, const int* __restrict__ index, int n_win,
                                             float* __restrict__ g_wlow) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_win) return;
    const int cell = index ? index[j] : j;
    if (cell < 0 || cell >= hf * wf) return;
    const int cy = cell / wf, cx = cell - cy * wf;
    const int n = count ? min(count[0], n_max) : n_max;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) {
        const int X = (int)pts[2 * i] + crop_left, Y = (int)pts[2 * i + 1] + crop_top;
        const int hc = Y >> 3, wc = X >> 3;
        const int ky = cy - hc + 1, kx = cx - wc + 1;
        if (ky < 0 || ky > 2 || kx < 0 || kx > 2 || hc < 0 || hc >= hf || wc < 0 || wc >= wf) continue;
        const int lane = (Y & 7) * 8 + (X & 7);
        const float* m = mask + ((int64_t)hc * wf + wc) * ld_mask + lane;
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
        float g = g_wsel[i];
        if (do_sigmoid) {
            float aw = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int ny = hc + k / 3 - 1, nx = wc + k % 3 - 1;
                float vw = 0.f;
                if (ny >= 0 && ny < hf && nx >= 0 && nx < wf) vw = 8.f * wlow[(int64_t)ny * wf + nx];
                aw += (e[k] / den) * vw;
            }
            const float sg = sigmoidf_(aw / 8.f);
            g = g * (sg * (1.f - sg));
        }
        float sk = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) sk = (k == ky * 3 + kx) ? e[k] / den : sk;
        acc += (g / 8.f) * (sk * 8.f);
    }
    g_wlow[cell] = acc;
}

}  // namespace

extern "C" int woft_convex_weights_at_bwd(const float* pts, const int32_t* count, int32_t n_max, const float* g_wsel,
                                          const float* wlow, const float* mask, int32_t ld_mask, int32_t hf, int32_t wf,
                                          int32_t crop_top, int32_t crop_left, int32_t do_sigmoid, const int32_t* index,
                                          int32_t n_win, float* g_wlow, void* stream) {
    if (!pts || !g_wsel || !mask || !g_wlow || n_max <= 0 || hf <= 0 || wf <= 0 || ld_mask < 576) return WOFT_EINVAL;
    if ((int64_t)hf * wf >= (1ll << 31) || (do_sigmoid && !wlow) || crop_top < 0 || crop_left < 0) return WOFT_EINVAL;
    if (index ? (n_win <= 0 || n_win > hf * wf) : (n_win != hf * wf)) return WOFT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    (void)hipMemsetAsync(g_wlow, 0, (size_t)hf * wf * sizeof(float), s);
    hipLaunchKernelGGL(convex_weights_at_bwd_kernel, dim3((n_win + 63) / 64), dim3(64), 0, s, pts, count, n_max, g_wsel, wlow,
                       mask, ld_mask, hf, wf, crop_top, crop_left, do_sigmoid, index, n_win, g_wlow);
    return woft_launch_status();
}

extern "C" int woft_wh_reduce_bwd(const float* act, const float* w6, const float* g_wlow, const int32_t* index, int32_t n_win,
                                  float* g_act, double* ws, float* g_w6, float* g_b6, void* stream) {
    if (!act || !w6 || !g_wlow || !g_act || !ws || !g_w6 || !g_b6 || n_win <= 0 || n_win > WOFT_WH_TRAIN_MAX_WIN)
        return WOFT_EINVAL;
    const int n_chunks = (n_win + WHT_CHUNK - 1) / WHT_CHUNK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(wht_reduce_bwd_kernel, dim3(n_chunks), dim3(128), 0, s, act, w6, g_wlow, index, n_win, g_act, ws);
    hipLaunchKernelGGL(wht_reduce_sum_kernel, dim3(1), dim3(192), 0, s, (const double*)ws, n_chunks, g_w6, g_b6);
    return woft_launch_status();
}

extern "C" int woft_wh_train_conv(const float* x, int32_t cin, const float* wt, const float* bias, const float* gate,
                                  int32_t n_win, float* y, void* stream) {
    if (!x || !wt || !y || n_win <= 0 || n_win > WOFT_WH_TRAIN_MAX_WIN || (cin != 128 && cin != 8)) return WOFT_EINVAL;
    if (bias && gate) return WOFT_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(n_win < 2048 ? n_win : 2048));
    if (cin == 128)
        hipLaunchKernelGGL(wht_conv_kernel<128>, grid, dim3(256), 0, s, x, wt, bias, gate, n_win, y);
    else
        hipLaunchKernelGGL(wht_conv_kernel<8>, grid, dim3(256), 0, s, x, wt, bias, gate, n_win, y);
    return woft_launch_status();
}

extern "C" int64_t woft_wh_wgrad_ws_bytes(int32_t n_win, int32_t cin) {
    if (n_win <= 0 || n_win > WOFT_WH_TRAIN_MAX_WIN || (cin != 128 && cin != 8)) return WOFT_EINVAL;
    const int64_t n_chunks = (n_win + WHT_CHUNK - 1) / WHT_CHUNK;
    return n_chunks * (9 * WHT_C * (int64_t)cin + WHT_C) * (int64_t)sizeof(float);
}

extern "C" int woft_wh_wgrad(const float* gy, const float* x, int32_t cin, int32_t cin_out, int32_t n_win, float* ws, float* gw,
                             float* gb, void* stream) {
    if (!gy || !x || !ws || !gw || !gb || n_win <= 0 || n_win > WOFT_WH_TRAIN_MAX_WIN) return WOFT_EINVAL;
    if ((cin != 128 && cin != 8) || cin_out <= 0 || cin_out > cin) return WOFT_EINVAL;
    const int n_chunks = (n_win + WHT_CHUNK - 1) / WHT_CHUNK;
    float* part_w = ws;
    float* part_b = ws + (int64_t)n_chunks * 9 * WHT_C * cin;
    hipStream_t s = (hipStream_t)stream;
    if (cin == 128)
        hipLaunchKernelGGL(wht_wgrad_kernel<128>, dim3(9, n_chunks), dim3(256), 0, s, gy, x, n_win, part_w, part_b);
    else
        hipLaunchKernelGGL(wht_wgrad_kernel<8>, dim3(9, n_chunks), dim3(256), 0, s, gy, x, n_win, part_w, part_b);
    const int n_out = WHT_C * cin_out * 9 + WHT_C;
    hipLaunchKernelGGL(wht_wgrad_sum_kernel, dim3((n_out + 255) / 256), dim3(256), 0, s, (const float*)part_w,
                       (const float*)part_b, n_chunks, cin, cin_out, gw, gb);
    return woft_launch_status();
}
