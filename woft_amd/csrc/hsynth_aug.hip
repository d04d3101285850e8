// Photometric augmentation of a rendered training frame: separable blur with replicate border, an affine
// colour map, stateless noise, rounding -- one launch from a float (h, w, 3) frame to its uint8 (and optionally float) version.
// Every product is followed by its add (the build passes -ffp-contract=off), the sums run in ascending tap order from 0.f.
#include <math.h>
#include "common.h"

namespace {

constexpr int TILE = 32;          // a workgroup's tile: TILE x TILE pixels, one thread per four adjacent pixels of a row

struct Blur { float tap[2 * WOFT_HSYNTH_MAX_BLUR + 1]; };
struct Colour { float m[9], o[3]; int on; };

__device__ __forceinline__ uint32_t mix32(uint32_t v) {
    v ^= v >> 16;
    v *= 0x7feb352du;
    v ^= v >> 15;
    v *= 0x846ca68bu;
    v ^= v >> 16;
    return v;
}

// z of (seed, idx): the sum of four 16-bit uniforms, centred and scaled to unit variance.  The integer part is exact.
__device__ __forceinline__ float noise_z(uint32_t seed, uint32_t idx) {
    const uint32_t a = mix32(seed ^ mix32(idx)), b = mix32(a + 0x9e3779b9u);
    const int32_t S = (int32_t)((a & 0xffffu) + (a >> 16) + (b & 0xffffu) + (b >> 16));
    return (float)(S - 131070) * (float)(1.7320508075688772 / 65536.0);
}

// Steps b and c on the three channels t[0..2] of the pixel with flat index pix (y * w + x).
__device__ __forceinline__ void colour_noise(const Colour& cm, float sigma, uint32_t seed, uint32_t pix, float* t) {
    if (cm.on) {
        float u[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = cm.o[c] + cm.m[3 * c] * t[0] + cm.m[3 * c + 1] * t[1] + cm.m[3 * c + 2] * t[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = u[c];
    }
    if (sigma != 0.f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = t[c] + sigma * noise_z(seed, pix * 3u + (uint32_t)c);
    }
}

__device__ __forceinline__ uint32_t to_byte(float v) { return (uint32_t)(uint8_t)fminf(fmaxf(rintf(v), 0.f), 255.f); }

// Four adjacent pixels v[0..11] of one row, the first at flat pixel index o0, n_ok of them inside the frame: 3 dwords / 3 float4
// when all four are there and o0 is a multiple of 4 with aligned bases (`vec`), bytes and floats otherwise -- the same values.
__device__ __forceinline__ void store4(const float* v, int64_t o0, int n_ok, int vec, uint8_t* __restrict__ out_u8,
                                       float* __restrict__ out_f32) {
    if (vec && n_ok == 4 && (o0 & 3) == 0) {
        uint32_t* o32 = reinterpret_cast<uint32_t*>(out_u8 + o0 * 3);
#pragma unroll
        for (int q = 0; q < 3; ++q)
            o32[q] = to_byte(v[4 * q]) | (to_byte(v[4 * q + 1]) << 8) | (to_byte(v[4 * q + 2]) << 16) | (to_byte(v[4 * q + 3]) << 24);
        if (out_f32 != nullptr) {
            f32x4* of = reinterpret_cast<f32x4*>(out_f32 + o0 * 3);
#pragma unroll
            for (int q = 0; q < 3; ++q) of[q] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
        }
        return;
    }
    for (int k = 0; k < 3 * n_ok; ++k) {
        out_u8[o0 * 3 + k] = (uint8_t)to_byte(v[k]);
        if (out_f32 != nullptr) out_f32[o0 * 3 + k] = v[k];
    }
}

// radius 0: no neighbourhood, no LDS.  Thread i takes pixels 4i .. 4i+3 of the flattened frame (it reads its own twelve floats
// before it writes them: in_f32 may be out_f32).
__global__ __launch_bounds__(256) void hsynth_augment_point_kernel(const float* in, int64_t n, Colour cm, float sigma, uint32_t seed,
                                                                   uint8_t* __restrict__ out_u8, float* out_f32, int vec) {
    const int64_t o0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (o0 >= n) return;
    const int n_ok = (int)(n - o0 < 4 ? n - o0 : 4);
    float v[12];
    if (vec && n_ok == 4) {
        const f32x4* p = reinterpret_cast<const f32x4*>(in + o0 * 3);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const f32x4 a = p[q];
            v[4 * q] = a.x, v[4 * q + 1] = a.y, v[4 * q + 2] = a.z, v[4 * q + 3] = a.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = k < 3 * n_ok ? in[o0 * 3 + k] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) colour_noise(cm, sigma, seed, (uint32_t)(o0 + j), v + 3 * j);
    store4(v, o0, n_ok, vec, out_u8, out_f32);
}

// radius R > 0.  A workgroup stages its TILE x TILE pixels with a halo of R (coordinates clamped to the frame: replicate border)
// in LDS, runs the horizontal pass over the tile's rows and its 2 R halo rows into LDS, and the vertical pass out of it in
// registers: thread (ty, tx) owns pixels 4 tx .. 4 tx + 3 of tile row ty, twelve consecutive floats of a row that it reads as
// three 16-byte LDS loads per tap (eight lanes cover the 32 banks once).  LDS: ((TILE + 2 R)^2 + (TILE + 2 R) TILE) * 12 bytes.
template <int R>
__global__ __launch_bounds__(256) void hsynth_augment_blur_kernel(const float* __restrict__ in, int h, int w, Blur bl, Colour cm,
                                                                  float sigma, uint32_t seed, uint8_t* __restrict__ out_u8,
                                                                  float* __restrict__ out_f32, int vec) {
    constexpr int ROWS = TILE + 2 * R, COLS3 = (TILE + 2 * R) * 3, MID3 = TILE * 3;
    __shared__ float tile[ROWS * COLS3];
    __shared__ __attribute__((aligned(16))) float mid[ROWS * MID3];
    const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE, tid = threadIdx.x;
    for (int e = tid; e < ROWS * COLS3; e += 256) {
        const int row = e / COLS3, col3 = e - row * COLS3, px = col3 / 3, c = col3 - px * 3;
        const int gx = min(max(x0 - R + px, 0), w - 1), gy = min(max(y0 - R + row, 0), h - 1);
        tile[e] = in[((int64_t)gy * w + gx) * 3 + c];
    }
    __syncthreads();
    for (int e = tid; e < ROWS * MID3; e += 256) {
        const int row = e / MID3, col3 = e - row * MID3;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i <= 2 * R; ++i) s = s + bl.tap[i] * tile[row * COLS3 + col3 + 3 * i];
        mid[e] = s;
    }
    __syncthreads();
    const int ty = tid >> 3, tx = tid & 7, x = x0 + 4 * tx, y = y0 + ty;
    if (y >= h || x >= w) return;
    float v[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = 0.f;
#pragma unroll
    for (int j = 0; j <= 2 * R; ++j) {
        const f32x4* p = reinterpret_cast<const f32x4*>(mid + (ty + j) * MID3 + 12 * tx);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const f32x4 a = p[q];
            v[4 * q] = v[4 * q] + bl.tap[j] * a.x;
            v[4 * q + 1] = v[4 * q + 1] + bl.tap[j] * a.y;
            v[4 * q + 2] = v[4 * q + 2] + bl.tap[j] * a.z;
            v[4 * q + 3] = v[4 * q + 3] + bl.tap[j] * a.w;
        }
    }
    const int64_t o0 = (int64_t)y * w + x;
    const int n_ok = w - x < 4 ? w - x : 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) colour_noise(cm, sigma, seed, (uint32_t)(o0 + j), v + 3 * j);
    store4(v, o0, n_ok, vec, out_u8, out_f32);
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <int R>
void launch_blur(const float* in, int h, int w, const Blur& bl, const Colour& cm, float sigma, uint32_t seed, uint8_t* out_u8,
                 float* out_f32, int vec, hipStream_t stream) {
    const dim3 grid((unsigned)((w + TILE - 1) / TILE), (unsigned)((h + TILE - 1) / TILE));
    hipLaunchKernelGGL(hsynth_augment_blur_kernel<R>, grid, dim3(256), 0, stream, in, h, w, bl, cm, sigma, seed, out_u8, out_f32,
                       vec);
}

}  // namespace

extern "C" int woft_hsynth_augment(const float* in_f32, int32_t h, int32_t w, const float* taps, int32_t radius,
                                   const float* colour, float noise_sigma, uint32_t seed, uint8_t* out_u8, float* out_f32,
                                   void* stream) {
    if (!in_f32 || !out_u8 || h <= 0 || w <= 0 || (int64_t)h * w >= (1ll << 31)) return WOFT_EINVAL;
    if (radius < 0 || radius > WOFT_HSYNTH_MAX_BLUR || (radius > 0 && (!taps || in_f32 == out_f32))) return WOFT_EINVAL;
    if (!(noise_sigma >= 0.f) || !isfinite(noise_sigma)) return WOFT_EINVAL;
    // (the grid's second dimension holds 65535 workgroups)
    if (radius > 0 && (h + TILE - 1) / TILE > 65535) return WOFT_EINVAL;
    Blur bl;
    for (int i = 0; i < 2 * WOFT_HSYNTH_MAX_BLUR + 1; ++i) bl.tap[i] = i <= 2 * radius && radius > 0 ? taps[i] : 0.f;
    Colour cm;
    cm.on = colour != nullptr;
    for (int i = 0; i < 9; ++i) cm.m[i] = colour ? colour[i] : (i % 4 == 0 ? 1.f : 0.f);
    for (int i = 0; i < 3; ++i) cm.o[i] = colour ? colour[9 + i] : 0.f;
    hipStream_t s = (hipStream_t)stream;
    if (radius == 0) {
        const int vec = aligned_to(in_f32, 16) && aligned_to(out_u8, 4) && aligned_to(out_f32, 16);
        const int64_t n = (int64_t)h * w;
        hipLaunchKernelGGL(hsynth_augment_point_kernel, dim3((unsigned)ceil_div64(ceil_div64(n, 4), 256)), dim3(256), 0, s, in_f32,
                           n, cm, noise_sigma, seed, out_u8, out_f32, vec);
        return woft_launch_status();
    }
    const int vec = aligned_to(out_u8, 4) && aligned_to(out_f32, 16);
    switch (radius) {
        case 1: launch_blur<1>(in_f32, h, w, bl, cm, noise_sigma, seed, out_u8, out_f32, vec, s); break;
        case 2: launch_blur<2>(in_f32, h, w, bl, cm, noise_sigma, seed, out_u8, out_f32, vec, s); break;
        case 3: launch_blur<3>(in_f32, h, w, bl, cm, noise_sigma, seed, out_u8, out_f32, vec, s); break;
        case 4: launch_blur<4>(in_f32, h, w, bl, cm, noise_sigma, seed, out_u8, out_f32, vec, s); break;
        case 5: launch_blur<5>(in_f32, h, w, bl, cm, noise_sigma, seed, out_u8, out_f32, vec, s); break;
        case 6: launch_blur<6>(in_f32, h, w, bl, cm, noise_sigma, seed, out_u8, out_f32, vec, s); break;
        default: launch_blur<7>(in_f32, h, w, bl, cm, noise_sigma, seed, out_u8, out_f32, vec, s); break;
    }
    return woft_launch_status();
}
