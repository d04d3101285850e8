// Band lookup (woft_corr_lookup_band): the volume-free lookup's samples interpolated from the correlation band that
// woft_corr_band_build stored once per flow (include/woft_hip.h: layout, m_l, hit rule) instead of recomputed by MFMA.
//
// A workgroup owns one 8 x 8 block of source pixels, as corr_lookup_otf_kernel does, and its prologue is that kernel's: the need /
// roi_* / smp_* rules and the folded flow-head gather, same operations in the same order, so coordinates and flow operands are
// bitwise the same.  Wave 0 (lane = source pixel) then derives the window origins of all levels and tests them against the band;
// the test is block-uniform.  On a hit the (2r+2) band rows that hold a pixel's window of a level -- one run of (2r+2) x 64 bytes in
// memory -- stream into LDS as 16-byte pieces, the next level's while this level's samples are interpolated with the arithmetic of
// corr_lookup_kernel (the volume-free lookup's sampling loop, cell for cell).  No MFMA, no source fragments; 130 registers and
// 54 KB of LDS: two workgroups per CU, which is what a 1080p launch (510 blocks on 256 CUs) asks for.
// woft_lookup_band_params.defer_samples: the launch stops after the hit test -- flags, counter and the gather's stores as ever, no
// sample written; the interpolation below then runs inside convc1's launch (conv_1x1_band.hip), which repeats the hit test.
#include "common.h"
#include "lookup_blocks.h"

namespace {

template <int R>
__global__ __launch_bounds__(256) void corr_lookup_band_kernel(const woft_lookup_band_params bp) {
    const woft_lookup_otf_params& p = bp.otf;
    constexpr int NPX = 64, NT = 256, MAXL = 4;
    constexpr int NW = 2 * R + 1, N2 = NW * NW, WS = NW + 1;
    constexpr int RS = WOFT_BAND_LD + 4;                 // LDS row stride (floats): 16-byte pieces stay aligned, columns i, i + 1, .. on different banks
    constexpr int PLD = WS * RS;                         // a pixel's WS band rows of one level
    constexpr int NLD = NPX * WS * 4 / NT;               // 16-byte pieces per thread and level
    static_assert(NLD * NT == NPX * WS * 4, "pieces divide among the threads");
    __shared__ __attribute__((aligned(16))) float Wl[NPX * PLD];
    __shared__ int s_ox[MAXL][NPX], s_oy[MAXL][NPX];     // window origin relative to the band's, per level
    __shared__ float s_fx[MAXL][NPX], s_fy[MAXL][NPX];

    const int tid = threadIdx.x;
    const BlockRect br = block_rect(p);
    const int tiles_x = br.nx, ntiles = br.nx * br.ny;
    int tile;
    {
        const int q = ntiles / 8, rr = ntiles % 8, xcd = blockIdx.x % 8, idx = blockIdx.x / 8;
        tile = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + idx;
    }
    const int px0 = (br.bx0 + tile % tiles_x) * 8, py0 = (br.by0 + tile / tiles_x) * 8;
    const bool sampled = (p.smp_y0 | p.smp_x0 | p.smp_h | p.smp_w) == 0 ||
                         (py0 < p.smp_y0 + p.smp_h && py0 + 8 > p.smp_y0 && px0 < p.smp_x0 + p.smp_w && px0 + 8 > p.smp_x0);
    const int y = py0 + ((tid & 63) >> 3), x = px0 + (tid & 7);       // (wave 0: this lane's source pixel)
    const bool cvalid = tid < NPX && y < p.hf && x < p.wf;
    const int64_t i = (int64_t)y * p.wf + x;
    if (p.need != nullptr) {      // nobody wants this block's samples
        const int any = cvalid ? p.need[i] : 0;
        if (!__syncthreads_or(any)) {
            if (cvalid) bp.miss[i] = 0;
            return;
        }
    }
    float cx = 0.f, cy = 0.f;
    if (cvalid) {
        cx = p.coords[i * 2];
        cy = p.coords[i * 2 + 1];
        if (p.fh_part != nullptr) {
            // the previous iteration's flow-head gather for this pixel: corr_lookup_otf_kernel's operations, in its order
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            float dx = p.fh_bias ? p.fh_bias[0] : 0.f, dy = p.fh_bias ? p.fh_bias[1] : 0.f;
            const int64_t plane = (int64_t)p.hf * p.wf * p.fh_ld;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int yy = y + ky - 1, xx = x + kx - 1;
                    f32x2 v = {0.f, 0.f};
                    if (yy >= 0 && yy < p.hf && xx >= 0 && xx < p.wf) {
                        const float* src = p.fh_part + ((int64_t)yy * p.wf + xx) * p.fh_ld + (ky * 3 + kx) * 2;
                        v = *(const f32x2*)src;
                        for (int t = 1; t < p.fh_planes; ++t) v += *(const f32x2*)(src + t * plane);
                    }
                    dx += v[0];
                    dy += v[1];
                }
            p.fh_delta[i * p.fh_ld_delta] = dx;
            p.fh_delta[i * p.fh_ld_delta + 1] = dy;
            cx += dx;
            cy += dy;
            ((float*)p.coords)[i * 2] = cx;
            ((float*)p.coords)[i * 2 + 1] = cy;
            const float fx = cx - (float)x, fy = cy - (float)y;
            if (p.fh_flow4 != nullptr) *(f32x4*)(p.fh_flow4 + i * 4) = f32x4{fx, fy, 0.f, 0.f};
            if (p.fh_flow_cat != nullptr) {
                p.fh_flow_cat[i * p.fh_ld_cat] = fx;
                p.fh_flow_cat[i * p.fh_ld_cat + 1] = fy;
            }
        }
    }
    if (!sampled) {                                      // (block-uniform, before the first barrier)
        if (cvalid) bp.miss[i] = 0;
        return;
    }
    // window origins and interpolation weights of all levels (corr_lookup_otf_kernel's), and the hit test
    int ok = 1;
    if (cvalid) {
#pragma unroll
        for (int l = 0; l < MAXL; ++l) {
            if (l < p.levels) {
                const float sc = 1.0f / (float)(1 << l);
                const float xs = cx * sc, ys = cy * sc;
                float flx = floorf(xs), fly = floorf(ys);
                s_fx[l][tid] = xs - flx;
                s_fy[l][tid] = ys - fly;
                flx = fminf(fmaxf(flx, -1.0e6f), 1.0e6f);
                fly = fminf(fmaxf(fly, -1.0e6f), 1.0e6f);
                const int m = WOFT_BAND_M(l);
                const int ox = (int)flx - (x >> l) + m, oy = (int)fly - (y >> l) + m;   // window origin - band origin
                ok &= (ox >= 0 && ox <= 2 * m && oy >= 0 && oy <= 2 * m) ? 1 : 0;
                s_ox[l][tid] = ox;
                s_oy[l][tid] = oy;
            }
        }
    }
    const int hit = __syncthreads_and(ok);               // (origins of all levels are in LDS)
    if (cvalid) bp.miss[i] = hit ? 0 : 1;
    if (!hit) {
        if (tid == 0) atomicAdd(bp.miss_count, 1);
        return;
    }
    if (bp.defer_samples != 0) return;                   // (the samples of hit blocks are woft_conv1x1_band's: conv_1x1_band.hip)
    const int rows = band_row_off(R, p.levels);
    // this thread's pieces of a level: piece k = (pixel, band row, quarter) = it / (4 WS), (it / 4) % WS, it % 4 with it = tid + k NT
    f32x4 pc[NLD];
    auto load_level = [&](int l) __attribute__((always_inline)) {
        const int roff = band_row_off(R, l);
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int it = tid + k * NT;
            const int pix = it / (4 * WS), rem = it - pix * (4 * WS);
            const int gy = py0 + (pix >> 3), gx = px0 + (pix & 7);
            pc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (gy < p.hf && gx < p.wf)
                pc[k] = *(const f32x4*)(bp.band + (((int64_t)gy * p.wf + gx) * rows + roff + s_ox[l][pix]) * WOFT_BAND_LD + rem * 4);
        }
    };
    load_level(0);
    for (int l = 0; l < p.levels; ++l) {
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int it = tid + k * NT;
            const int pix = it / (4 * WS), rem = it - pix * (4 * WS);
            *(f32x4*)(Wl + pix * PLD + (rem >> 2) * RS + (rem & 3) * 4) = pc[k];
        }
        __syncthreads();
        if (l + 1 < p.levels) load_level(l + 1);         // in flight while this level is sampled
        // ---- bilinear samples: the arithmetic of corr_lookup_kernel, one window column per item (corr_lookup_otf_kernel's loop) ----
        for (int it = tid; it < NPX * NW; it += NT) {
            const int pix = it / NW, c = it - pix * NW;
            const int gy = py0 + (pix >> 3), gx = px0 + (pix & 7);
            if (gy >= p.hf || gx >= p.wf) continue;
            const float fx = s_fx[l][pix], fy = s_fy[l][pix];
            const float* cq = Wl + pix * PLD + c * RS + s_oy[l][pix];
            float h[WS];
#pragma unroll
            for (int j = 0; j < WS; ++j) h[j] = cq[j] * (1.f - fx) + cq[RS + j] * fx;
            float* o = p.out + ((int64_t)gy * p.wf + gx) * p.ldo + l * N2 + c * NW;
#pragma unroll
            for (int j = 0; j < NW; ++j) o[j] = h[j] * (1.f - fy) + h[j + 1] * fy;
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int woft_corr_lookup_band(const woft_lookup_band_params* bp, void* stream) {
    if (!bp || !bp->band || !bp->miss || !bp->miss_count) return WOFT_EINVAL;
    const woft_lookup_otf_params& p = bp->otf;
    if (p.levels < 1 || p.levels > 4 || !p.f1 || !p.coords || !p.out || p.hf <= 0 || p.wf <= 0 || p.ablate != 0) return WOFT_EINVAL;
    if (p.terms != 1 && p.terms != 3) return WOFT_EINVAL;
    if (!((p.k == 256 && p.radius == 4) || (p.k == 128 && p.radius == 3))) return WOFT_EINVAL;     // (the band build's instances)
    for (int l = 0; l < p.levels; ++l)
        if (p.h[l] <= 0 || p.w[l] <= 0) return WOFT_EINVAL;
    const int nout = p.levels * (2 * p.radius + 1) * (2 * p.radius + 1);
    if (p.ldo < nout) return WOFT_EINVAL;
    if (p.fh_part != nullptr && (p.fh_delta == nullptr || p.fh_planes < 1 || p.fh_ld < 20 || p.fh_ld % 4 != 0 || p.fh_ld_delta < 2 ||
                                 (p.fh_flow_cat != nullptr && p.fh_ld_cat < 2) || p.need != nullptr))
        return WOFT_EINVAL;
    auto rect_bad = [&](int y0, int x0, int h, int w) {     // (all zero: not given)
        return (y0 | x0 | h | w) != 0 && (h <= 0 || w <= 0 || y0 < 0 || x0 < 0 || y0 > p.hf - h || x0 > p.wf - w);
    };
    if (rect_bad(p.roi_y0, p.roi_x0, p.roi_h, p.roi_w) || rect_bad(p.smp_y0, p.smp_x0, p.smp_h, p.smp_w)) return WOFT_EINVAL;
    const BlockRect br = block_rect(p);
    dim3 grid((unsigned)(br.nx * br.ny));
    hipStream_t s = (hipStream_t)stream;
    if (p.radius == 4) woft_launch(0, corr_lookup_band_kernel<4>, grid, dim3(256), 0, s, *bp);
    else woft_launch(0, corr_lookup_band_kernel<3>, grid, dim3(256), 0, s, *bp);
    return woft_launch_status();
}
