// Training of the MaskHead (weighted_raft.py:295-309, 387-422) on the whole 1/8-resolution map: the forward layers that keep
// their activations, the data gradient, the weight gradient and the backward of the closing 1x1 conv.
// Exact fp32 throughout: the products run on v_mfma_f32_32x32x2_f32 (bit for bit a k-ordered fmaf chain) or on the vector ALUs.
// Every sum is deterministic: no floating-point atomics; the parameter gradients are written as one partial per fixed-size chunk
// of the map (a partition that does not depend on the grid) and added in chunk order in fp64.
//
// Layouts: maps NHWC, [hf * wf pixels][channel stride]; forward weights wt[tap = ky * 3 + kx][ci][co]; parameter gradients in
// the state dict's [co][ci][ky][kx].  A tile is MHT_TILE consecutive positions of one map row; it sits in LDS with a halo of one
// position on every side, and every halo position outside the map is a zero -- the x = -1 tap of a row's first pixel reads that
// zero, not the last pixel of the row before it in memory.
#include "common.h"

namespace {

constexpr int MHT_TILE = WOFT_MH_TRAIN_TILE;               // positions of a map row per tile (the M or K extent of one MFMA tile)
constexpr int MHT_CHUNK = WOFT_MH_TRAIN_CHUNK;             // tiles per partial sum of a weight gradient
constexpr int MHT_RCHUNK = WOFT_MH_REDUCE_CHUNK;           // pixels per partial sum of the closing conv's gradient
constexpr int MHT_CK = 32;                                 // input channels staged in LDS at a time
constexpr int MHT_HW = MHT_TILE + 2;                       // positions of a tile row with its halo
constexpr int MHT_MAX_C = 128, MHT_MAX_CIN = 512;

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// row of accumulator register r in a 32x32 tile (the column is lane & 31)
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// A stage in LDS: channels c0 .. c0 + 31 of a tile (row ty, columns tx0 .. tx0 + 31) and its halo, element k = (r * MHT_HW + xp)
// * 32 + c at xs[(r * MHT_HW + xp) * S + c], r = 0..2 the rows ty - 1 .. ty + 1, xp = 0..33 the columns tx0 - 1 .. tx0 + 32; zero
// outside the map.  The channels come from x0 below c_split and from x1 above it (c_split is a multiple of 32: a stage never
// straddles the two).  Thread tid of NT owns the elements tid + NT * j: it loads them into registers a stage ahead.
constexpr int MHT_TOT = 3 * MHT_HW * MHT_CK;               // elements of a stage

// ---- 3x3 conv cin -> cout over the map ---------------------------------------------------------------------------------------
//   y[p][co] = epi(sum_{tap, ci} x[p + tap][ci] * wt[tap][ci][co])
//   epi: + bias[co], ReLU (forward layer: bias != NULL) | * (gate[p][co] > 0) (data gradient: the transposed, flipped filter in
//   wt, gate = the activation the gradient flows into)
// grid (tiles of a row, rows), NW = cout / 32 waves: wave w owns output channels 32 w .. 32 w + 31 of the tile's 32 positions.  The
// input channels pass through LDS 32 at a time (channel stride 33 floats, so that the 32 positions a wave reads at one channel
// fall into 32 banks); the loads of stage s + 1 are issued before the matrix loop of stage s and land while it runs.  One fma
// chain per stage of 9 x 32 products, added to the total on the vector ALUs.
template <int NW>
__global__ __launch_bounds__(64 * NW) void mht_conv_kernel(const float* __restrict__ x0, int cs0, const float* __restrict__ x1,
                                                           int cs1, int c_split, int cin, const float* __restrict__ wt, int cout,
                                                           const float* __restrict__ bias, const float* __restrict__ gate,
                                                           int gate_cs, int hf, int wf, float* __restrict__ y, int y_cs) {
    constexpr int S = MHT_CK + 1;
    constexpr int NT = 64 * NW;                                          // threads of the block
    constexpr int NL = (MHT_TOT + NT - 1) / NT;                          // elements of a stage per thread
    __shared__ float xs[3 * MHT_HW * S];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, kh = lane >> 5;
    const int tx0 = blockIdx.x * MHT_TILE, ty = blockIdx.y;
    const int co = 32 * wave + i;
    int pix[NL];                                                         // the map pixel of this thread's elements, -1: a zero
#pragma unroll
    for (int j = 0; j < NL; ++j) {
        const int k = tid + NT * j, q = k / MHT_CK;
        const int r = q / MHT_HW, xp = q - r * MHT_HW;
        const int yy = ty + r - 1, xx = tx0 + xp - 1;
        pix[j] = (k < MHT_TOT && yy >= 0 && yy < hf && xx >= 0 && xx < wf) ? yy * wf + xx : -1;
    }
    float xr[NL];
    auto fetch = [&](int c0) {
        const float* __restrict__ src = (c0 < c_split ? x0 + c0 : x1 + (c0 - c_split)) + (tid & (MHT_CK - 1));
        const int scs = c0 < c_split ? cs0 : cs1;
#pragma unroll
        for (int j = 0; j < NL; ++j) xr[j] = pix[j] >= 0 ? src[(int64_t)pix[j] * scs] : 0.f;
    };
    fetch(0);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    constexpr int NK = MHT_CK / 2;
    const int64_t tap_stride = (int64_t)cin * cout;
    for (int c0 = 0; c0 < cin; c0 += MHT_CK) {
        // The weights of a tap are a lane's own 16 values; they are fetched one tap ahead -- tap 0's before the stage's tile is
        // loaded, tap k + 1's before the matrix loop of tap k -- and land while those run.
        const float* __restrict__ wst = wt + ((int64_t)c0 + kh) * cout + co;
        float b[NK];
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) b[kk] = wst[(2 * kk) * cout];
        __syncthreads();                                                 // (every wave is done with the previous stage in LDS)
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int k = tid + NT * j;
            if (k < MHT_TOT) xs[(k / MHT_CK) * S + (k & (MHT_CK - 1))] = xr[j];
        }
        __syncthreads();
        if (c0 + MHT_CK < cin) fetch(c0 + MHT_CK);
        f32x16 part, part2;                                              // (two chains: even and odd channel pairs)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[r] = part2[r] = 0.f;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int off = ((tap / 3) * MHT_HW + tap % 3 + i) * S + kh;   // halo coordinates: (1 + ky - 1, i + 1 + kx - 1)
            const float* __restrict__ wnext = wst + min(tap + 1, 8) * tap_stride;      // (tap 8 fetches its own again: unused)
            float bn[NK];
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) bn[kk] = wnext[(2 * kk) * cout];
#pragma unroll
            for (int kk = 0; kk < NK; kk += 2) {
                part = mfma32(xs[off + 2 * kk], b[kk], part);
                part2 = mfma32(xs[off + 2 * kk + 2], b[kk + 1], part2);
            }
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) b[kk] = bn[kk];
        }
        part += part2;
        acc += part;
    }
    const float bv = bias ? bias[co] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int xx = tx0 + acc_row(r, lane);
        if (xx >= wf) continue;
        const int64_t p = (int64_t)ty * wf + xx;
        float v = acc[r];
        if (bias) v = fmaxf(v + bv, 0.f);
        if (gate) v = gate[p * gate_cs + co] > 0.f ? v : 0.f;
        y[p * y_cs + co] = v;
    }
}

// ---- weight gradient of a 3x3 layer cin -> cout --------------------------------------------------------------------------------
//   part_w[chunk][tap][co][ci] = sum over the chunk's tiles and their positions p of gy[p][co] * x[p + tap][ci]
//   part_b[chunk][co]          = sum over the same positions of gy[p][co]                  (written by the blocks of ci tile 0)
// grid (cin / 32 tiles of ci, chunks of MHT_CHUNK tiles), cout / 32 waves.  Per tap a GEMM co x ci with K = the positions: wave w
// owns output channels 32 w .. 32 w + 31 (the M index, operand A = gy), the block's 32 input channels are the N index (operand
// B = x), and all nine taps accumulate side by side -- 9 x 16 accumulator registers per lane, one A value feeds nine MFMAs.  The K
// index runs over the positions of a tile in pairs (lane half kh takes position 2 tt + kh) and then over the chunk's tiles.
// Operand B is shared by the waves and by the taps: the tile's x sits in LDS with its zero halo (lanes differ in the channel, so a
// read is conflict free).  Operand A is private to a lane (every gy element is read by exactly one lane of the block): its 16
// values per tile are loaded into registers; positions beyond the row's end enter as zeros.
// Both are fetched one tile ahead: the loads of tile t + 1 are issued before the matrix loop of tile t and land while it runs.
template <int NW>
__global__ __launch_bounds__(64 * NW) void mht_wgrad_kernel(const float* __restrict__ gy, int gy_cs, int cout,
                                                            const float* __restrict__ x0, int cs0, const float* __restrict__ x1,
                                                            int cs1, int c_split, int cin, int hf, int wf, int tiles_x,
                                                            int n_tiles, float* __restrict__ part_w, float* __restrict__ part_b) {
    constexpr int S = MHT_CK;
    constexpr int NSTEP = MHT_TILE / 2;
    constexpr int NT = 64 * NW;                                         // threads of the block
    constexpr int TOT = MHT_TOT;                                        // floats of a tile with its halo (S = 32: xs[k])
    constexpr int NL = (TOT + NT - 1) / NT;                             // ... per thread
    __shared__ float xs[TOT];
    const int c0 = blockIdx.x * MHT_CK, chunk = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, kh = lane >> 5;
    const int co = 32 * wave + i;
    const float* __restrict__ src = c0 < c_split ? x0 + c0 : x1 + (c0 - c_split);
    const int scs = c0 < c_split ? cs0 : cs1;
    f32x16 acc[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tap][r] = 0.f;
    double bsum = 0.0;                                                  // (bias gradient: this lane's gy values, in fp64)
    const int t0 = chunk * MHT_CHUNK, t1 = min(t0 + MHT_CHUNK, n_tiles);
    float xr[NL], av[NSTEP];
    auto fetch = [&](int t) {
        const int ty = t / tiles_x, tx0 = (t - ty * tiles_x) * MHT_TILE;
#pragma unroll
        for (int j = 0; j < NL; ++j) {                                  // (element k = (r * MHT_HW + xp) * 32 + c)
            const int k = tid + NT * j;
            const int c = k & (MHT_CK - 1), q = k / MHT_CK;
            const int r = q / MHT_HW, xp = q - r * MHT_HW;
            const int yy = ty + r - 1, xx = tx0 + xp - 1;
            xr[j] = (k < TOT && yy >= 0 && yy < hf && xx >= 0 && xx < wf) ? src[((int64_t)yy * wf + xx) * scs + c] : 0.f;
        }
#pragma unroll
        for (int tt = 0; tt < NSTEP; ++tt) {
            const int xx = tx0 + 2 * tt + kh;
            av[tt] = xx < wf ? gy[((int64_t)ty * wf + xx) * gy_cs + co] : 0.f;
        }
    };
    if (t0 < t1) fetch(t0);
    for (int t = t0; t < t1; ++t) {
        __syncthreads();                                                // (every wave is done with the previous tile in LDS)
#pragma unroll
        for (int j = 0; j < NL; ++j)
            if (tid + NT * j < TOT) xs[tid + NT * j] = xr[j];
        float a[NSTEP];
#pragma unroll
        for (int tt = 0; tt < NSTEP; ++tt) {
            a[tt] = av[tt];
            bsum += (double)a[tt];
        }
        __syncthreads();
        if (t + 1 < t1) fetch(t + 1);
#pragma unroll
        for (int tt = 0; tt < NSTEP; ++tt) {
            const float* __restrict__ xb = xs + (2 * tt + kh) * S + i;   // halo coordinates of tap (ky, kx): (ky, position + kx)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) acc[tap] = mfma32(a[tt], xb[((tap / 3) * MHT_HW + tap % 3) * S], acc[tap]);
        }
    }
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        float* __restrict__ pw = part_w + ((int64_t)chunk * 9 + tap) * cout * cin + c0 + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) pw[(int64_t)(32 * wave + acc_row(r, lane)) * cin] = acc[tap][r];
    }
    const double other = __shfl_xor(bsum, 32);
    if (blockIdx.x == 0 && kh == 0) part_b[chunk * cout + co] = (float)(bsum + other);     // (even positions + odd positions)
}

// gw[co][ci][tap] = sum over the chunks, in order, in fp64;  gb[co] alike.  A thread per partial element in the partials' own
// order (consecutive threads read consecutive floats of every chunk).
__global__ void mht_wgrad_sum_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b, int n_chunks, int cin,
                                     int cout, float* __restrict__ gw, float* __restrict__ gb) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_w = 9 * cout * cin;
    if (e < n_w) {
        const int ci = e % cin, co = (e / cin) % cout, tap = e / (cin * cout);
        double s = 0.0;
        for (int c = 0; c < n_chunks; ++c) s += (double)part_w[(int64_t)c * n_w + e];
        gw[((int64_t)co * cin + ci) * 9 + tap] = (float)s;
    } else if (e < n_w + cout) {
        const int co = e - n_w;
        double s = 0.0;
        for (int c = 0; c < n_chunks; ++c) s += (double)part_b[c * cout + co];
        gb[co] = (float)s;
    }
}

// ---- closing 1x1 conv, backward ------------------------------------------------------------------------------------------------
//   g_act[p][c] = g_low[p] * w[c] * (act[p][c] > 0)
//   part[chunk][c] = sum over the chunk's pixels of g_low[p] * act[p][c]  (c < C),  part[chunk][128] = sum of g_low[p]    (fp64)
__global__ __launch_bounds__(128) void mht_reduce_bwd_kernel(const float* __restrict__ act, int act_cs, int c_n,
                                                             const float* __restrict__ w, const float* __restrict__ g_low,
                                                             int n_pix, float* __restrict__ g_act, int g_cs,
                                                             double* __restrict__ part) {
    const int c = threadIdx.x, chunk = blockIdx.x;
    const bool on = c < c_n;
    const float wc = on ? w[c] : 0.f;
    const int p0 = chunk * MHT_RCHUNK, p1 = min(p0 + MHT_RCHUNK, n_pix);
    double sw = 0.0, sb = 0.0;
    for (int p = p0; p < p1; ++p) {
        const float g = g_low[p];
        sb += (double)g;
        if (on) {
            const float a = act[(int64_t)p * act_cs + c];
            g_act[(int64_t)p * g_cs + c] = a > 0.f ? g * wc : 0.f;
            sw += (double)g * (double)a;
        }
    }
    if (on) part[(int64_t)chunk * (MHT_MAX_C + 1) + c] = sw;
    if (c == 0) part[(int64_t)chunk * (MHT_MAX_C + 1) + MHT_MAX_C] = sb;
}
__global__ void mht_reduce_sum_kernel(const double* __restrict__ part, int n_chunks, int c_n, float* __restrict__ g_w,
                                      float* __restrict__ g_b) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > MHT_MAX_C || (c >= c_n && c != MHT_MAX_C)) return;
    double s = 0.0;
    for (int k = 0; k < n_chunks; ++k) s += part[(int64_t)k * (MHT_MAX_C + 1) + c];
    if (c < MHT_MAX_C) g_w[c] = (float)s;
    else g_b[0] = (float)s;
}

bool channels_ok(int c, int c_max) { return c > 0 && c <= c_max && c % 32 == 0; }
// the two-source description of an input map: x1 NULL <=> c_split == cin
bool sources_ok(const float* x0, int cs0, const float* x1, int cs1, int c_split, int cin) {
    if (!x0 || !channels_ok(cin, MHT_MAX_CIN) || c_split <= 0 || c_split > cin || c_split % 32 != 0 || cs0 < c_split) return false;
    return x1 ? (c_split < cin && cs1 >= cin - c_split) : c_split == cin;
}
bool map_ok(int hf, int wf) { return hf > 0 && wf > 0 && hf <= 65535 && (int64_t)hf * wf < (1ll << 24); }
int64_t n_tiles_of(int hf, int wf) { return (int64_t)hf * ((wf + MHT_TILE - 1) / MHT_TILE); }

}  // namespace

extern "C" int woft_mh_train_conv(const float* x0, int32_t cs0, const float* x1, int32_t cs1, int32_t c_split, int32_t cin,
                                  const float* wt, int32_t cout, const float* bias, const float* gate, int32_t gate_cs, int32_t hf,
                                  int32_t wf, float* y, int32_t y_cs, void* stream) {
    if (!sources_ok(x0, cs0, x1, cs1, c_split, cin) || !wt || !y || !channels_ok(cout, MHT_MAX_C) || !map_ok(hf, wf))
        return WOFT_EINVAL;
    if ((bias && gate) || y_cs < cout || (gate && gate_cs < cout)) return WOFT_EINVAL;
    const dim3 grid((wf + MHT_TILE - 1) / MHT_TILE, hf);
#define MHT_CONV(NW)                                                                                                          \
    hipLaunchKernelGGL(mht_conv_kernel<NW>, grid, dim3(64 * NW), 0, (hipStream_t)stream, x0, cs0, x1, cs1, c_split, cin, wt, cout, \
                       bias, gate, gate_cs, hf, wf, y, y_cs)
    switch (cout / 32) {
        case 1: MHT_CONV(1); break;
        case 2: MHT_CONV(2); break;
        case 3: MHT_CONV(3); break;
        default: MHT_CONV(4); break;
    }
#undef MHT_CONV
    return woft_launch_status();
}

extern "C" int64_t woft_mh_wgrad_ws_bytes(int32_t hf, int32_t wf, int32_t cin, int32_t cout) {
    if (!map_ok(hf, wf) || !channels_ok(cin, MHT_MAX_CIN) || !channels_ok(cout, MHT_MAX_C)) return WOFT_EINVAL;
    const int64_t n_chunks = (n_tiles_of(hf, wf) + MHT_CHUNK - 1) / MHT_CHUNK;
    return n_chunks * (9 * (int64_t)cout * cin + cout) * (int64_t)sizeof(float);
}

extern "C" int woft_mh_wgrad(const float* gy, int32_t gy_cs, int32_t cout, const float* x0, int32_t cs0, const float* x1,
                             int32_t cs1, int32_t c_split, int32_t cin, int32_t hf, int32_t wf, float* ws, float* gw, float* gb,
                             void* stream) {
    if (!gy || !ws || !gw || !gb || !sources_ok(x0, cs0, x1, cs1, c_split, cin) || !channels_ok(cout, MHT_MAX_C) || !map_ok(hf, wf))
        return WOFT_EINVAL;
    if (gy_cs < cout) return WOFT_EINVAL;
    const int tiles_x = (wf + MHT_TILE - 1) / MHT_TILE, n_tiles = (int)n_tiles_of(hf, wf);
    const int n_chunks = (n_tiles + MHT_CHUNK - 1) / MHT_CHUNK;
    float* part_w = ws;
    float* part_b = ws + (int64_t)n_chunks * 9 * cout * cin;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cin / MHT_CK, n_chunks);
#define MHT_WGRAD(NW)                                                                                                        \
    hipLaunchKernelGGL(mht_wgrad_kernel<NW>, grid, dim3(64 * NW), 0, s, gy, gy_cs, cout, x0, cs0, x1, cs1, c_split, cin, hf, wf, \
                       tiles_x, n_tiles, part_w, part_b)
    switch (cout / 32) {
        case 1: MHT_WGRAD(1); break;
        case 2: MHT_WGRAD(2); break;
        case 3: MHT_WGRAD(3); break;
        default: MHT_WGRAD(4); break;
    }
#undef MHT_WGRAD
    const int n_out = 9 * cout * cin + cout;
    hipLaunchKernelGGL(mht_wgrad_sum_kernel, dim3((n_out + 255) / 256), dim3(256), 0, s, (const float*)part_w,
                       (const float*)part_b, n_chunks, cin, cout, gw, gb);
    return woft_launch_status();
}

extern "C" int woft_mh_reduce_bwd(const float* act, int32_t act_cs, int32_t c, const float* w, const float* g_low, int32_t n_pix,
                                  float* g_act, int32_t g_cs, double* ws, float* g_w, float* g_b, void* stream) {
    if (!act || !w || !g_low || !g_act || !ws || !g_w || !g_b || !channels_ok(c, MHT_MAX_C) || n_pix <= 0 || n_pix >= (1 << 24))
        return WOFT_EINVAL;
    if (act_cs < c || g_cs < c) return WOFT_EINVAL;
    const int n_chunks = (n_pix + MHT_RCHUNK - 1) / MHT_RCHUNK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mht_reduce_bwd_kernel, dim3(n_chunks), dim3(128), 0, s, act, act_cs, c, w, g_low, n_pix, g_act, g_cs, ws);
    hipLaunchKernelGGL(mht_reduce_sum_kernel, dim3(1), dim3(192), 0, s, (const double*)ws, n_chunks, c, g_w, g_b);
    return woft_launch_status();
}
