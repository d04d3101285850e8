// conv1x1_kernel (woft_conv_params.halo == 16): 1x1 / stride-1 convolution = a plain GEMM out[m][n] = sum_k x[m][k] w[n][k] over
// the pixels m, for the wide 1x1 layers of the hot path -- the motion encoder's convc1 (324 lookup samples -> 256, update.py:89),
// the encoders' closing 1x1 (128 -> 256, extractor.py:166).
//
// Why a kernel of its own: the per-tap gather kernel (conv.hip: conv_mfma_bf16_kernel) runs these layers on 64 x 64 tiles -- every
// fp32 activation row is fetched and split into its bf16 terms by each of the cout / 64 column-tile workgroups, one K step ahead,
// with a workgroup barrier per step and both operand tiles through LDS (15-17 % MFMA-busy, profiles/r05_pmc_mfma_util_conv.csv).
// Here a workgroup owns 64 pixels x ALL 128 TN output columns (TN = 2: 256): the activations are read and converted ONCE per
// layer; each of the four waves owns a 32 TN-column band for all 64 rows, so its weights are nobody else's -- streamed global ->
// registers in MFMA-fragment order (the register-streamed conv kernel's packing, conv_regb_body.h) NB half-chunks ahead, no LDS,
// no barrier; the activation tile of a 32-channel chunk goes through a double-buffered LDS tile (one barrier per chunk) and is
// requested DEPTH chunks ahead in registers: a 1x1 layer has only 24 MFMAs per wave and chunk to hide a load behind, and its
// input is usually the previous launch's output on its way in from beyond L2.
//
// FLAT (round 5): the same tile loop for a "flat"-packed tiny-Cin layer (woft_conv_params.flat: the K chunk of tap row ky is the NHWC
// row itself, 32 floats from pixel ox - pad_x on; the motion encoder's convf1, 7x7 on the 2-channel flow, update.py:91) -- K chunks =
// tap rows, validity per pixel of the row -- so that convc1 and convf1, which are independent, share ONE launch (woft_conv2d_pair)
// as they did on the gather kernel.  Measured at 1/8 of 1080p (bf16x3): convc1 alone 29.7 us (gather kernel 37), the pair 39.8-42.4
// (45.5); ablations of convc1 alone (tools/regb_probe.py c1, ABL bits): no output stores -7.6 us (507 workgroups = ONE round in
// lock-step: all of them store their 33 MB at the same time), no weight stream -3.9, no activation loads -2.6, none of the three
// 17.6 us -- 11 chunks at ~1.1 us of barrier + fragment-read latency + 24 MFMAs each.  Tried and not kept: the flat tile and the
// wide tile of the same pixels in ONE workgroup (the short tile's stores under the long tile's K loop): 41.6 vs 39.8 us as two
// groups of workgroups; the shorter layer's workgroups first or last: the same; two chunks per workgroup barrier (four LDS
// sub-buffers): 32.7 vs 31.9 us, 18.0 vs 17.6 without global traffic -- the barrier is not what a chunk costs.
//
// Arithmetic: operands, products and their order as in the other split-bf16 kernels (TERMS 3: lo*hi, hi*lo, hi*hi per k16 step,
// k ascending; fp32 accumulation) -- the result equals the gather kernel's bit for bit (tests/test_kernels_gpu.py).
#include "conv_1x1_tile.h"

namespace {

// the two tile forms: 1x1 layers 256 columns per workgroup, flat layers 128

template <int TERMS>
__global__ __launch_bounds__(256, 2) void conv1x1_kernel(const woft_conv_params pa, const woft_conv_params pb, const int split) {
    // (two independent layers may share ONE launch -- woft_conv2d_pair: the workgroups [0, split) belong to the first layer, the rest
    //  to the second; split = gridDim.x for a single layer)
    __shared__ __attribute__((aligned(16))) __bf16 smem[Geom1x1<TERMS, 2>::SMEM_ELEMS];
    static_assert(Geom1x1<TERMS, 2>::SMEM_ELEMS >= Geom1x1<TERMS, 1>::SMEM_ELEMS, "one LDS array for every mode");
    const bool second_layer = (int)blockIdx.x >= split;
    const woft_conv_params p = second_layer ? pb : pa;     // (a copy: see conv_regb_kernel)
    const int bid = second_layer ? (int)blockIdx.x - split : (int)blockIdx.x;
    int m_tile, n_tile;
    woft::tile_of_block(bid, m_tiles_1x1(p), p.cout_pad / (p.flat ? 128 : 256), m_tile, n_tile);
    if (!p.flat) tile_1x1<TERMS, 2, false, 4, 4>(p, m_tile, n_tile, smem);
    else tile_1x1<TERMS, 1, true, 4, 4>(p, m_tile, n_tile, smem);
}

}  // namespace

// Called by woft_conv2d / woft_conv2d_pair for halo == 16, after their argument checks.  tile_n = 256 (the layer's columns in whole
// 256-wide tiles); flat layers: 128.
int woft_conv_1x1_launch(const woft_conv_params& a, const woft_conv_params* second, void* stream) {
    for (const woft_conv_params* q : {&a, second}) {
        if (q == nullptr) continue;
        const woft_conv_params& p = *q;
        if (p.precision < 1 || p.precision > 3 || p.precision != a.precision) return WOFT_EINVAL;
        if (p.stride != 1 || p.ho != p.h || p.wo != p.w || p.taps_x != 1) return WOFT_EINVAL;
        if (p.flat) {           // (woft_conv2d has checked cs0 in {4, 8, 16, 32} and in1 == NULL)
            if (p.cin_pad != 32 || p.tile_n != 128 || 2 * p.pad_y + 1 != p.taps_y) return WOFT_EINVAL;
        } else if (p.taps_y != 1 || p.pad_y != 0 || p.pad_x != 0 || p.tile_n != 256) {
            return WOFT_EINVAL;
        }
        if (p.wgt_frag == nullptr || p.stat_sum != nullptr || p.in_norm != 0 || p.wh0_lookup != nullptr) return WOFT_EINVAL;
        if (p.epi == WOFT_EPI_FLOWHEAD || p.epi == WOFT_EPI_WH_MEAN || p.epi == WOFT_EPI_CTX) return WOFT_EINVAL;
        if (p.cout_pad % p.tile_n != 0) return WOFT_EINVAL;
        const int64_t cs_max = (p.in1 != nullptr && p.cs1 > p.cs0) ? p.cs1 : p.cs0;
        if ((int64_t)p.n_img * p.h * p.w * cs_max >= (1ll << 31)) return WOFT_EINVAL;       // 32-bit element offsets
    }
    auto blocks = [](const woft_conv_params& q) {
        return (int64_t)m_tiles_1x1(q) * (q.cout_pad / (q.flat ? 128 : 256));
    };
    const woft_conv_params& pb = second ? *second : a;
    const int split = (int)blocks(a);
    dim3 grid((unsigned)(blocks(a) + (second ? blocks(pb) : 0)));
    hipStream_t s = (hipStream_t)stream;
    switch (a.precision) {
        case 1: woft_launch(0, conv1x1_kernel<3>, grid, dim3(256), 0, s, a, pb, split); break;
        case 2: woft_launch(0, conv1x1_kernel<1>, grid, dim3(256), 0, s, a, pb, split); break;
        default: woft_launch(0, conv1x1_kernel<16>, grid, dim3(256), 0, s, a, pb, split); break;
    }
    return woft_launch_status();
}
