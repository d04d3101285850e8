// conv1x1_band_kernel (woft_conv1x1_band): the motion encoder's convc1 (324 lookup samples -> 256, update.py:89) with the band
// lookup's sampling inside its launch -- the samples of a hit block go from the band straight into the GEMM's A tiles in LDS and
// never to memory (was: 352 padded floats per pixel written by corr_lookup_band_kernel and read back by conv1x1_kernel: 2 x 45.6 MB
// and a launch boundary per refinement iteration at 1080p).
//
// A workgroup owns one 8 x 8 block of source pixels (corr_lookup_band_kernel's blocks, order and XCD mapping) x all 256 columns:
// tile row r = pixel (r / 8, r % 8) of the block.  Wave 0 reads the block's coordinates (already updated: the folded gather stays in
// the lookup launch, whose flow4 stores the partner layer reads), derives origins and fractions with the band lookup's expressions
// and repeats its hit test; the decision is block-uniform and the band is addressed only inside a pixel's own rows.
//   hit : per level, the 10 band rows of a pixel's window stream through LDS in two overlapping halves (rows 0-5 for the window
//         columns 0-4, rows 5-9 for the columns 5-8: 30 KB instead of one level's 51 KB; row 5 is fetched twice, from L2), the next
//         half's 16-byte pieces in flight in registers while this one is interpolated -- corr_lookup_band_kernel's arithmetic, cell for
//         cell -- and every sample is converted exactly as tile_1x1's store_a converts it and dropped into the A tile of its
//         32-channel chunk: a ring of four chunk tiles, since a level's 81 samples end inside a chunk (levels complete the chunks
//         0-1, 2-4, 5-6, 7-10; channels 324..351 of chunk 10 are zeros).
//   miss: the chunks are loaded from c1->in0, where the fallback lookup has just written the block's rows, as conv1x1_kernel loads them.
// After each level the completed chunks run tile_1x1's MFMAs: chunk-ascending, per k16 step lo*hi, hi*lo, hi*hi, weights streamed
// from wgt_frag NB - 1 half-chunks ahead -- the same products in the same order on the same bits, so the output equals the
// three-launch form's bit for bit.  The A ring is complete before a level's MFMAs start: no barrier inside the chunk loop; the two
// co-resident workgroups of a CU overlap one's sampling with the other's MFMAs (as in corr_lookup_otf_kernel).  conv_epilogue_t
// unchanged, on block rows.  Workgroups at or beyond `split`: the FLAT tile of the partner layer (convf1), as in conv1x1_kernel.
#include "conv_1x1_tile.h"
#include "lookup_blocks.h"

int woft_conv_check(const woft_conv_params& p);              // conv.hip: woft_conv2d's argument checks

namespace {

// tile row -> output pixel of the 8 x 8 block at (py0, px0), or -1 outside the map
struct BlockRows {
    int py0, px0, hf, wf;
    __device__ __forceinline__ int64_t operator()(int row) const {
        const int y = py0 + (row >> 3), x = px0 + (row & 7);
        return (y < hf && x < wf) ? (int64_t)y * wf + x : -1;
    }
};

template <int TERMS>
struct GeomBand {
    using G = Geom1x1<TERMS, 2>;
    static constexpr int R = 4, NW = 2 * R + 1, N2 = NW * NW, WS = NW + 1, LEVELS = 4;
    static constexpr int RING = 4;                               // chunk tiles of the A ring
    static constexpr int RS = WOFT_BAND_LD + 4;                  // LDS row stride of a band row (corr_lookup_band_kernel's)
    static constexpr int HR = 6, PLD = HR * RS;                  // band rows of the larger half; a pixel's rows of one half
    static constexpr int RING_ELEMS = RING * G::A_ELEMS;
    static constexpr int WIN_ELEMS = 64 * PLD * 2;               // the windows (floats) counted in bf16 elements
    static constexpr int SMEM_ELEMS = RING_ELEMS + WIN_ELEMS;
    static_assert(SMEM_ELEMS >= G::STAGE_ELEMS && SMEM_ELEMS >= Geom1x1<TERMS, 1>::SMEM_ELEMS, "one LDS array for every phase");
    static_assert((RING_ELEMS * 2) % 16 == 0, "the windows start 16-byte aligned");
};

template <int TERMS>
__global__ __launch_bounds__(256, 2) void conv1x1_band_kernel(const woft_conv_params pa, const woft_conv_params pb,
                                                              const woft_lookup_band_params bp, const int split) {
    using GB = GeomBand<TERMS>;
    using G = Geom1x1<TERMS, 2>;
    constexpr int NP = G::NP, TM = G::TM, TN = 2, A_PLANE = G::A_PLANE, A_ELEMS = G::A_ELEMS, WCOLS = G::WCOLS;
    constexpr int R = GB::R, NW = GB::NW, WS = GB::WS, RS = GB::RS, PLD = GB::PLD, NT = 256, NB = 4, NCHUNK = 11;
    constexpr int STEP_ELEMS = NP * 2 * 64 * 8;
    __shared__ __attribute__((aligned(16))) __bf16 smem[GB::SMEM_ELEMS];
    __shared__ int s_ox[GB::LEVELS][64], s_oy[GB::LEVELS][64];   // window origin relative to the band's, per level
    __shared__ float s_fx[GB::LEVELS][64], s_fy[GB::LEVELS][64];

    if ((int)blockIdx.x >= split) {                              // the partner layer's workgroups: conv1x1_kernel's flat tile
        int m_tile, n_tile;
        woft::tile_of_block((int)blockIdx.x - split, m_tiles_1x1(pb), pb.cout_pad / 128, m_tile, n_tile);
        tile_1x1<TERMS, 1, true, 4, 4>(pb, m_tile, n_tile, smem);
        return;
    }
    const woft_lookup_otf_params& p = bp.otf;
    __bf16* const ring = smem;
    float* const Wl = (float*)(smem + GB::RING_ELEMS);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, hh = lane >> 5;
    const int tiles_x = (p.wf + 7) / 8;
    int tile;
    {
        const int q = split / 8, rr = split % 8, xcd = blockIdx.x % 8, idx = blockIdx.x / 8;
        tile = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + idx;
    }
    const int px0 = (tile % tiles_x) * 8, py0 = (tile / tiles_x) * 8;

    // this wave's weight streams (tile_1x1's): bands wave TN + j, chunk-major, [plane][k half][64 lanes][8]
    const __bf16* wstream[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) wstream[j] = (const __bf16*)pa.wgt_frag + (int64_t)(wave * TN + j) * NCHUNK * STEP_ELEMS + lane * 8;
    bf16x8 bq[NB][TN][NP];
    auto fetch_b = [&](int step, auto slot_tag) {                          // step = 2 chunk + k half
        constexpr int slot = decltype(slot_tag)::value;
        const int s = step < 2 * NCHUNK ? step : 2 * NCHUNK - 1;          // (past the end: a harmless repeat)
        const int off = (s >> 1) * STEP_ELEMS + (s & 1) * 512;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) bq[slot][j][pl] = *(const bf16x8*)(wstream[j] + off + pl * 1024);
    };
    [&]<int... S>(std::integer_sequence<int, S...>) {
        (fetch_b(S, std::integral_constant<int, S>{}), ...);
    }(std::make_integer_sequence<int, NB - 1>{});

    // ---- window origins and interpolation weights of all levels and the hit test: corr_lookup_band_kernel's, from the stored coordinates
    int ok = 1;
    {
        const int y = py0 + (lane >> 3), x = px0 + (lane & 7);  // (wave 0: this lane's source pixel)
        const bool cvalid = tid < 64 && y < p.hf && x < p.wf;
        if (cvalid) {
            const int64_t i = (int64_t)y * p.wf + x;
            const float cx = p.coords[i * 2], cy = p.coords[i * 2 + 1];
#pragma unroll
            for (int l = 0; l < GB::LEVELS; ++l) {
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
        } else if (tid < 64) {                                   // (pixels outside the map: never read, kept tidy)
#pragma unroll
            for (int l = 0; l < GB::LEVELS; ++l) {
                s_fx[l][tid] = s_fy[l][tid] = 0.f;
                s_ox[l][tid] = s_oy[l][tid] = 0;
            }
        }
    }
    // (block-uniform; the origins of all levels are in LDS.  On a hit every valid pixel's ox lies in [0, 2 m_l]: the rows
    //  ox .. ox + 9 read below are rows of that pixel's own band, W_l = 10 + 2 m_l)
    const bool hit = __builtin_amdgcn_readfirstlane(__syncthreads_and(ok)) != 0;

    // ---- hit: a half of a level's window rows per step.  Half 0: band rows ox .. ox + 5 (window columns 0-4), half 1: ox + 5 .. ox + 9
    // (columns 5-8); piece k of a thread = (pixel, row of the half, quarter) = it / (4 NR), (it / 4) % NR, it % 4 with it = tid + k NT
    constexpr int ROWS = 16 + 14 + 12 + 12;                      // band rows per source pixel (radius 4, 4 levels: woft_hip.h)
    f32x4 pc[GB::HR];
    auto load_half = [&](auto l_tag, auto h_tag) __attribute__((always_inline)) {
        constexpr int l = decltype(l_tag)::value, half = decltype(h_tag)::value;
        constexpr int NR = half == 0 ? 6 : 5, R0 = half == 0 ? 0 : 5;
        constexpr int roff = l == 0 ? 0 : (l == 1 ? 16 : (l == 2 ? 30 : 42));
        static_assert(64 * NR * 4 == NR * NT, "NR pieces per thread");
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int it = tid + k * NT;
            const int pix = it / (4 * NR), rem = it - pix * (4 * NR);
            const int gy = py0 + (pix >> 3), gx = px0 + (pix & 7);
            pc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (gy < p.hf && gx < p.wf) {
                const int ox = s_ox[l][pix];
                pc[k] = *(const f32x4*)(bp.band + (((int64_t)gy * p.wf + gx) * ROWS + roff + ox + R0) * WOFT_BAND_LD + rem * 4);
            }
        }
    };
    auto store_half = [&](auto h_tag) __attribute__((always_inline)) {
        constexpr int half = decltype(h_tag)::value;
        constexpr int NR = half == 0 ? 6 : 5;
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int it = tid + k * NT;
            const int pix = it / (4 * NR), rem = it - pix * (4 * NR);
            *(f32x4*)(Wl + pix * PLD + (rem >> 2) * RS + (rem & 3) * 4) = pc[k];
        }
    };
    // one window column (pixel, c) -> its 9 samples -> the A tiles: corr_lookup_band_kernel's arithmetic, then store_a's conversion
    auto sample = [&](auto l_tag, int pix, int c, int lrow) __attribute__((always_inline)) {
        constexpr int l = decltype(l_tag)::value;
        const int gy = py0 + (pix >> 3), gx = px0 + (pix & 7);
        if (gy >= p.hf || gx >= p.wf) return;
        const float fx = s_fx[l][pix], fy = s_fy[l][pix];
        const float* cq = Wl + pix * PLD + lrow * RS + s_oy[l][pix];
        float h[WS];
#pragma unroll
        for (int j = 0; j < WS; ++j) h[j] = cq[j] * (1.f - fx) + cq[RS + j] * fx;
        float o[12];
#pragma unroll
        for (int j = 0; j < NW; ++j) o[j] = h[j] * (1.f - fy) + h[j + 1] * fy;
        o[9] = o[10] = o[11] = 0.f;
        const int ch0 = l * GB::N2 + c * NW;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const f32x4 val = {o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]};
            const bf16x4 hi = cvt16<TERMS>(val);
            bf16x4 lo = hi;
            if (NP == 2) lo = __builtin_convertvector(val - widen_bf16x4(hi), bf16x4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (4 * g + e >= NW) continue;
                const int ch = ch0 + 4 * g + e;
                __bf16* a = ring + ((ch >> 5) & (GB::RING - 1)) * A_ELEMS + pix * LDB + (ch & 31);
                a[0] = hi[e];
                if (NP == 2) a[A_PLANE] = lo[e];
            }
        }
    };
    // miss: chunk `chunk` from the lookup buffer, tile_1x1's load_a + store_a on block rows
    const int row = tid >> 2, v = tid & 3;
    const int64_t mrow = BlockRows{py0, px0, p.hf, p.wf}(row);
    auto fill_chunk = [&](int chunk) __attribute__((always_inline)) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 rh[2] = {zero, zero};
        if (mrow >= 0) {
            const uint32_t off = (uint32_t)mrow * (uint32_t)pa.cs0 + (uint32_t)(chunk * BK + 8 * v);
            rh[0] = *(const f32x4*)(pa.in0 + off);
            rh[1] = *(const f32x4*)(pa.in0 + off + 4);
        }
        bf16x4 hi[2], lo[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            hi[e] = cvt16<TERMS>(rh[e]);
            if (NP == 2) lo[e] = __builtin_convertvector(rh[e] - widen_bf16x4(hi[e]), bf16x4);
        }
        __bf16* As = ring + (chunk & (GB::RING - 1)) * A_ELEMS;
        *(bf16x8*)(As + row * LDB + 8 * v) = __builtin_shufflevector(hi[0], hi[1], 0, 1, 2, 3, 4, 5, 6, 7);
        if (NP == 2) *(bf16x8*)(As + A_PLANE + row * LDB + 8 * v) = __builtin_shufflevector(lo[0], lo[1], 0, 1, 2, 3, 4, 5, 6, 7);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int a_off = r32 * LDB + hh * 8;                                  // this lane's row of row tile 0, k half 0
    // chunk c from its ring tile: tile_1x1's run_chunk without the activation stream (the tile is complete) and without a barrier
    auto run_chunk = [&](auto c_tag) __attribute__((always_inline)) {
        constexpr int c = decltype(c_tag)::value;
        const __bf16* As = ring + (c & (GB::RING - 1)) * A_ELEMS;
        bf16x8 aq[2][TM][NP];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) aq[s2][i][pl] = *(const bf16x8*)(As + a_off + i * 32 * LDB + pl * A_PLANE + s2 * 16);
        [&]<int... S2>(std::integer_sequence<int, S2...>) {
            ([&] {
                constexpr int s2 = S2, slot = (2 * c + s2) % NB;
                fetch_b(2 * c + s2 + NB - 1, std::integral_constant<int, (2 * c + s2 + NB - 1) % NB>{});
                __builtin_amdgcn_sched_barrier(0);
                if (NP == 2) {
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int i = 0; i < TM; ++i) acc[i][j] = mma16<TERMS>(aq[s2][i][NP - 1], bq[slot][j][0], acc[i][j]);
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int i = 0; i < TM; ++i) acc[i][j] = mma16<TERMS>(aq[s2][i][0], bq[slot][j][NP - 1], acc[i][j]);
                }
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int i = 0; i < TM; ++i) acc[i][j] = mma16<TERMS>(aq[s2][i][0], bq[slot][j][0], acc[i][j]);
                __builtin_amdgcn_sched_barrier(0);
            }(), ...);
        }(std::make_integer_sequence<int, 2>{});
    };

    if (hit) load_half(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
    auto level = [&](auto l_tag) __attribute__((always_inline)) {
        constexpr int l = decltype(l_tag)::value;
        constexpr int c_first = l == 0 ? 0 : (l == 1 ? 2 : (l == 2 ? 5 : 7));    // chunks this level completes
        constexpr int c_last = l == 0 ? 1 : (l == 1 ? 4 : (l == 2 ? 6 : 10));
        static_assert(c_last == (l == 3 ? NCHUNK - 1 : ((l + 1) * GB::N2) / BK - 1) && c_last - c_first < GB::RING, "ring of four chunk tiles");
        if (hit) {
            store_half(std::integral_constant<int, 0>{});
            __syncthreads();                             // (also: every wave is done with the chunks of the level before)
            load_half(l_tag, std::integral_constant<int, 1>{});
            if (l == 3) {                                // channels 324 .. 351: zeros (chunk 10, elements 4 .. 31)
                __bf16* As = ring + ((NCHUNK - 1) & (GB::RING - 1)) * A_ELEMS + row * LDB;
                const bf16x4 z4 = __builtin_bit_cast(bf16x4, (uint64_t)0);
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) {
                    if (v == 0) *(bf16x4*)(As + pl * A_PLANE + 4) = z4;
                    else *(bf16x8*)(As + pl * A_PLANE + 8 * v) = __builtin_shufflevector(z4, z4, 0, 1, 2, 3, 4, 5, 6, 7);
                }
            }
            for (int it = tid; it < 64 * 5; it += NT) {
                const int pix = it / 5, c = it - pix * 5;
                sample(l_tag, pix, c, c);
            }
            __syncthreads();
            store_half(std::integral_constant<int, 1>{});
            __syncthreads();
            if constexpr (l + 1 < GB::LEVELS) load_half(std::integral_constant<int, l + 1>{}, std::integral_constant<int, 0>{});
            sample(l_tag, tid >> 2, 5 + (tid & 3), tid & 3);
        } else {
            __syncthreads();                             // (every wave is done with the chunks of the level before)
#pragma unroll
            for (int c = c_first; c <= c_last; ++c) fill_chunk(c);
        }
        __syncthreads();
        [&]<int... C>(std::integer_sequence<int, C...>) {
            (run_chunk(std::integral_constant<int, c_first + C>{}), ...);
        }(std::make_integer_sequence<int, c_last - c_first + 1>{});
    };
    level(std::integral_constant<int, 0>{});
    level(std::integral_constant<int, 1>{});
    level(std::integral_constant<int, 2>{});
    level(std::integral_constant<int, 3>{});
    __syncthreads();                                     // (the staging area overlays the ring)
    woft::conv_epilogue_t<TM, TN, G::BM, WCOLS, G::ST>(pa, acc, (float*)smem + wave * G::ST * woft::STAGE_FLOATS,
                                                        BlockRows{py0, px0, p.hf, p.wf}, 0, 0, wave, lane, tile);
}

}  // namespace

extern "C" int woft_conv1x1_band(const woft_conv_params* c1, const woft_conv_params* f1, const woft_lookup_band_params* bp,
                                 void* stream) {
    if (c1 == nullptr || bp == nullptr || bp->band == nullptr) return WOFT_EINVAL;
    const woft_lookup_otf_params& o = bp->otf;
    // the band instance: radius 4, k 256, 4 levels, whole map, every block
    if (o.radius != 4 || o.k != 256 || o.levels != 4 || (o.terms != 1 && o.terms != 3) || o.coords == nullptr || o.out == nullptr ||
        o.hf <= 0 || o.wf <= 0 || o.need != nullptr || o.ablate != 0)
        return WOFT_EINVAL;
    if ((o.roi_y0 | o.roi_x0 | o.roi_h | o.roi_w | o.smp_y0 | o.smp_x0 | o.smp_h | o.smp_w) != 0) return WOFT_EINVAL;
    for (const woft_conv_params* q : {c1, f1}) {
        if (q == nullptr) continue;
        if (woft_conv_check(*q) != WOFT_OK) return WOFT_EINVAL;
        const woft_conv_params& p = *q;
        // woft_conv2d_pair's conditions for the streamed GEMM kernel (conv_1x1.hip: woft_conv_1x1_launch), without a rectangle
        if (p.halo != 16 || p.precision < 1 || p.precision > 3 || p.precision != c1->precision) return WOFT_EINVAL;
        if (p.stride != 1 || p.ho != p.h || p.wo != p.w || p.taps_x != 1) return WOFT_EINVAL;
        if (p.wgt_frag == nullptr || p.stat_sum != nullptr || p.in_norm != 0 || p.wh0_lookup != nullptr) return WOFT_EINVAL;
        if (p.epi == WOFT_EPI_FLOWHEAD || p.epi == WOFT_EPI_WH_MEAN || p.epi == WOFT_EPI_CTX) return WOFT_EINVAL;
        if ((p.roi_y0 | p.roi_x0 | p.roi_h | p.roi_w) != 0) return WOFT_EINVAL;
        const int64_t cs_max = (p.in1 != nullptr && p.cs1 > p.cs0) ? p.cs1 : p.cs0;
        if ((int64_t)p.n_img * p.h * p.w * cs_max >= (1ll << 31)) return WOFT_EINVAL;       // 32-bit element offsets
    }
    // convc1 on the lookup buffer of bp: 324 (padded 352) -> 256, one image of hf x wf
    if (c1->flat || c1->taps_y != 1 || c1->pad_y != 0 || c1->pad_x != 0 || c1->tile_n != 256 || c1->cin_pad != 352 ||
        c1->cout_pad != 256 || c1->in1 != nullptr || c1->n_img != 1 || c1->h != o.hf || c1->w != o.wf)
        return WOFT_EINVAL;
    if (c1->in0 != o.out || c1->cs0 != o.ldo || o.ldo < 352) return WOFT_EINVAL;
    if (f1 != nullptr && (!f1->flat || f1->cin_pad != 32 || f1->tile_n != 128 || 2 * f1->pad_y + 1 != f1->taps_y ||
                          f1->cout_pad % 128 != 0))
        return WOFT_EINVAL;
    const int split = ((o.hf + 7) / 8) * ((o.wf + 7) / 8);
    const int64_t extra = f1 != nullptr ? (int64_t)m_tiles_1x1(*f1) * (f1->cout_pad / 128) : 0;
    dim3 grid((unsigned)(split + extra));
    hipStream_t s = (hipStream_t)stream;
    const woft_conv_params& pb = f1 != nullptr ? *f1 : *c1;
    switch (c1->precision) {
        case 1: woft_launch(0, conv1x1_band_kernel<3>, grid, dim3(256), 0, s, *c1, pb, *bp, split); break;
        case 2: woft_launch(0, conv1x1_band_kernel<1>, grid, dim3(256), 0, s, *c1, pb, *bp, split); break;
        default: woft_launch(0, conv1x1_band_kernel<16>, grid, dim3(256), 0, s, *c1, pb, *bp, split); break;
    }
    return woft_launch_status();
}
