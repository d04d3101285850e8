/* woft_hip.h -- C ABI of libwoft_hip.so: the MI355X (gfx950) kernels of the WOFT hot path.
 *
 * Conventions:
 *   - every entry point is extern "C", takes plain device pointers / sizes, enqueues on the
 *     hipStream_t passed as `stream` (void*), never allocates, never synchronises;
 *   - the caller owns every buffer (PyTorch caching allocator in the Python host);
 *   - return 0 on success, WOFT_EINVAL (-1) for a rejected argument, WOFT_ELAUNCH (-2) when
 *     hipGetLastError() reports a launch failure.  No C++ exceptions cross the ABI.
 *   - activations are NHWC fp32 with an explicit channel stride ("cs", floats per pixel).
 *
 * Each entry point cites the reference code it replaces (paths relative to
 * /root/reference/pytracking/).
 */
#ifndef WOFT_HIP_H
#define WOFT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WOFT_OK 0
#define WOFT_EINVAL (-1)
#define WOFT_ELAUNCH (-2)

/* ABI / build identification: returns 10000*major + 100*minor + patch. */
int woft_abi_version(void);
/* sizeof(woft_conv_params) (which = 0) / woft_lookup_params (1) / woft_lookup_otf_params (2) / woft_lookup_band_params (3) /
   woft_hsynth_occluder (4): layout check for FFI mirrors. */
int woft_sizeof(int which);
/* developer knob for the micro-benchmarks in tools/ (ablation bits of the correlation GEMM, key 2); 0 in production. */
int woft_set_tuning(int key, int value);

/* ---------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on f32-input MFMA (v_mfma_f32_32x32x2_f32), NHWC.
 * Replaces every nn.Conv2d on the path: external/RAFT/raft_core/extractor.py:10-45,127-147,
 * update.py:9-10,19-21,36-42,82-86,118-125, weighted_raft.py:336-341 -- and, used as an
 * NT GEMM, the all-pairs correlation torch.matmul of corr.py:62-69.
 * ------------------------------------------------------------------------------------- */
enum woft_epilogue {
    WOFT_EPI_LINEAR = 0,        /* y = alpha*acc + bias                                      */
    WOFT_EPI_RELU = 1,          /* relu(y)                                                   */
    WOFT_EPI_SIGMOID = 2,
    WOFT_EPI_TANH = 3,
    WOFT_EPI_RELU_RES_RELU = 4, /* relu(e0[m][n] + relu(y))   residual block, extractor.py:48-56 */
    WOFT_EPI_GRU_ZR = 5,        /* n <  split: out[m][n]   = sigmoid(y)            (z)
                                   n >= split: out1[m][n-split] = sigmoid(y) * e0[m][n-split] (r*h)
                                   update.py:47-50 */
    WOFT_EPI_GRU_Q = 6,         /* out = (1-z)*h + z*tanh(y), h = e0, z = e1   update.py:50-51 */
    WOFT_EPI_CTX = 7,           /* n < split: tanh(y) else relu(y)   weighted_raft.py:217-219   */
    WOFT_EPI_WH_MEAN = 8,       /* halo 2 (9x9 patches), one N tile: out[image] = e1[0] + mean over the 81 pixels of
                                   <e0[0..cout), relu(y)> -- the weight head's last ReLU, 1x1 conv and patch mean
                                   (weighted_raft.py:341,378-383) without writing the activation               */
    WOFT_EPI_FLOWHEAD = 9       /* halo 8 only.  FlowHead (update.py:10-17) conv2(relu(conv1(x))) with conv2 (3x3 -> 2
                                   channels) folded into conv1's epilogue: instead of relu(y) the launch writes, per
                                   pixel m, the 18 partial products s[tap * 2 + o] = <W2[o][:, tap], relu(y[m])> over
                                   the channels of column tile t to out[(t * M + m) * ldo + 0..17] (ldo >= 20; t <
                                   cout_pad / tile_n planes; M = n_img * ho * wo).  e0 = W2 as bf16 MFMA B fragments,
                                   [cout / 32 bands][2 k halves][planes hi(, lo)][64 lanes][8], lane = 32 * (k half
                                   of the half) + column j, columns j >= 18 zero.  woft_flow_head_gather finishes
                                   the 3x3 sum.                                                                */
};

typedef struct woft_conv_params {
    const float* in0;      /* source of input channels [0, c_split)                            */
    const float* in1;      /* source of input channels [c_split, cin_pad) or NULL              */
    int32_t cs0, cs1;      /* floats per pixel of in0 / in1                                    */
    int32_t c_split;       /* multiple of 32; == cin_pad when in1 is NULL                      */
    int32_t n_img, h, w;   /* input batch and spatial size                                     */
    int32_t ho, wo;        /* output spatial size                                              */
    int32_t taps_y, taps_x;/* kernel taps (flat mode: taps_x must be 1)                        */
    int32_t stride, pad_y, pad_x;
    int32_t cin_pad;       /* GEMM-K per tap, multiple of 32                                   */
    int32_t flat;          /* 1: the 32-float K chunk of a tap runs along x over 32/cs0 pixels */
    const float* wgt;      /* [cout_pad][taps_y*taps_x*cin_pad] fp32, K contiguous (precision 0) */
    const void* wgt_hi;    /* same shape, bf16: hi = bf16(w)          (precision 1, 2); fp16(w) (precision 3) */
    const void* wgt_lo;    /* same shape, bf16: lo = bf16(w - hi)     (precision 1)            */
    int32_t precision;     /* (4: see wgt_mx)  0: fp32 MFMA; 1: split-bf16 x3 (fp32-emulating); 2: bf16; 3: fp16 operands, fp32
                              accumulation (the reference's mixed_precision autocast, weighted_raft.py:204,215,233;
                              not for the 9 x 9 weight-head windows, which the reference keeps in fp32)   */
    const float* bias;     /* [cout_pad] or NULL                                               */
    float alpha;           /* scale applied to the accumulator                                 */
    int32_t cout;          /* valid output channels                                            */
    int32_t cout_pad;      /* rows of wgt, multiple of the N tile (64 or 128)                  */
    float* out;            /* out[m*ldo + co_off + col(n)]                                     */
    int64_t ldo;
    int32_t co_off;
    int32_t out_w, out_pitch; /* if out_pitch != 0: col(n) = (n / out_w)*out_pitch + n % out_w  */
    int32_t epi;           /* enum woft_epilogue                                               */
    int32_t split;         /* channel split of GRU_ZR / CTX                                    */
    const float* e0;       /* epilogue operand (residual / h), row stride lde0                 */
    const float* e1;       /* epilogue operand (z), row stride lde1                            */
    int32_t lde0, lde1;
    float* out1;           /* second output of GRU_ZR, row stride ldo1                         */
    int32_t ldo1;
    float* stat_sum;       /* optional [2*ceil(M/BM)][cout_pad] per-wave-row partial sums of y */
    float* stat_sq;        /*          ... and of y*y  (InstanceNorm statistics)               */
    int32_t tile_m, tile_n;/* block tile: 128 or 64 each (halo 16: tile_n 256; flat: 128)      */
    int32_t halo;          /* 0: gather A per tap.  Split-bf16 precisions, stride 1, 3x3/1x5/5x1 only:
                              input halo of the output tile resident in LDS for all taps; tile_m ignored:
                              1 = 8x16 px, 4 = 4x16 px, 2 = one 9x9 image per workgroup (weight-head patches;
                              ho = wo = 9).  (Larger tiles / several patches per workgroup were measured
                              1.5-3x slower: one workgroup per CU cannot hide its own latencies.)
                              7 = the encoders' first layer (extractor.py:127-129: 7x7, stride 2, pad 3) on its own kernel:
                              flat packing of an NHWC4 image (cs0 = 4, taps_y = 7, taps_x = 1, cin_pad = 32), split-bf16
                              precisions, cout_pad % 64 == 0, 8x16 output pixels x 64 channels per tile, statistics rows
                              indexed by those tiles; results bit-identical to halo = 0
                              16 = wide 1x1 / stride-1 layers (update.py:89 convc1, extractor.py:166 conv2) on the streamed
                              GEMM kernel (conv_1x1.hip): 64 pixels x tile_n = 256 columns per workgroup, the activations
                              read and converted once per layer, weights from wgt_frag (taps = 1); also stride-1 flat
                              layers (flat != 0, cin_pad = 32, taps_x = 1, pad_y = taps_y / 2; update.py:91 convf1) with
                              tile_n = 128, K chunks = tap rows; split-bf16 precisions, cout_pad % tile_n == 0, no
                              statistics / in_norm; bit-identical to halo = 0.  woft_conv2d_pair takes two such layers */
    int32_t in_norm;       /* halo != 0 only: 0 = use in0 as is; 1 / 2 = in0 holds a RAW conv output whose
                              InstanceNorm is applied while loading (extractor.py:44-47: x = (x - in_mean[c]) *
                              in_rstd[c], 2: followed by ReLU), zero padding applied after it; in1 must be NULL */
    const float* in_mean;  /* [cin] per-channel statistics of in0 (woft_inorm_finalize)          */
    const float* in_rstd;
    const float* bias_map; /* optional per-pixel bias [M][ld_bias_map] used instead of bias[] (cout % 4 == 0): the
                              contribution of input channels that do not change between launches, computed once
                              (the GRU's context features `inp`, update.py:45-60: conv(W,[h,inp,motion]) =
                              conv(W_h,m, [h,motion]) + conv(W_inp, inp))                              */
    int32_t ld_bias_map;
    const int32_t* out_index; /* WOFT_EPI_WH_MEAN only, optional: image i writes out[out_index[i]] (the weight head
                              evaluated on a subset of the source pixels)                        */
    /* Weight head only (halo == 2, 9 x 9 windows, 3 x 3 taps, cin_pad == 128, split-bf16 precisions): when
       wh0_lookup != NULL the head's FIRST conv (5 -> 128 channels, 3 x 3, zero padding, ReLU;
       weighted_raft.py:336,363-376) is evaluated inside this launch, 32 channels at a time, from the lookup
       window of the source pixel -- in0 is ignored, the 1.3 GB activation between the two layers never exists.
       Input channels of window position t: lookup[s][4 t .. 4 t + 3] and mean[s] (woft_wh_conv0's layout). */
    const float* wh0_lookup;   /* [P][wh0_ld] fp32, wh0_ld >= 324, % 4 == 0                               */
    int32_t wh0_ld;
    const float* wh0_mean;     /* [P]                                                                     */
    const void* wh0_w;         /* bf16 MFMA fragments [4 chunks][3 K steps][1 or 2 planes hi, lo][64 lanes][8]:
                                  lane L, element e = W0[32 chunk + L % 32][k = 16 step + 8 (L / 32) + e],
                                  k = (3 ky + kx) * 5 + ci, zero for k >= 45                                */
    const float* wh0_bias;     /* [128]                                                                   */
    const int32_t* wh0_index;  /* optional: window i of this launch is source pixel wh0_index[i]          */
    /* halo == 8 (8x16-pixel tiles, split-bf16 precisions, stride 1, 3x3 / 1x5 / 5x1, no in_norm): the weight operand is
       streamed global -> registers instead of through LDS; it is read from wgt_frag, the same weights in MFMA-fragment
       order: [cout_pad / 32 bands][cin_pad / 32 chunks][taps][planes: hi (, lo)][2 k halves][64 lanes][8] bf16, lane L
       element e of k half s = W[32 band + L % 32][tap][32 chunk + 8 (2 s + L / 32) + e].  tile_n 128: one wave per
       32-column band and all 128 rows; tile_n 64: 2 x 2 waves.  halo == 12: the same kernel on 4x16-pixel tiles x 128
       columns (tile_n 128, cout_pad % 128 == 0, multi-tap layers): one wave per band and all 64 rows.            */
    const void* wgt_frag;
    /* precision 4 ("f16mx8", round 4; halo 8 / 12 with 3x3 / 1x5 / 5x1 taps only): an fp32-emulating product in two matrix-pipe
       passes -- fp16(a) * fp16(w) on v_mfma_f32_32x32x16_f16 + the two cross terms (a - fp16(a)) * w and a * (w - fp16(w)) on the
       block-scaled fp8 form v_mfma_scale_f32_32x32x64_f8f6f4, one scaled MFMA per PAIR of taps (K = 2 taps x 32 channels; an odd
       last tap pairs with zero weights).  wgt_frag: the fp16 fragments (the precision-3 format).  wgt_mx: per 32-column band, 32-
       channel chunk, tap pair and term (0: w, multiplied with the activations' remainder; 1: w - fp16(w), multiplied with the
       activations): 64 lanes x 32 bytes fp8 e4m3 (lane L: column 32 band + L % 32; bytes 0-15 = channels 16 (L / 32) .. + 15 of
       the chunk at the pair's first tap, bytes 16-31 = at its second tap), then 64 x int32 whose low byte is the E8M0 scale of the
       (column, tap, chunk) block the lane half supplies (L / 32 = 0: first tap, 1: second tap; value = 2^(scale - 127)).
       Measured: 2.2-2.3 x the error of precision 1 at 1.64 x its matrix-pipe rate (tools/micro/mx_split_probe.hip). */
    const void* wgt_mx;
    /* Output rectangle (halo 8 / 12 / 16 only): the launch computes and stores only the output pixels (y, x) with
       roi_y0 <= y < roi_y0 + roi_h and roi_x0 <= x < roi_x0 + roi_w of every image -- its tile grid covers the rectangle (origin at
       (roi_y0, roi_x0): 8x16 / 4x16-pixel tiles, or 64-pixel runs along the rectangle's rows for halo 16), every other output pixel
       is left untouched.  The input is still the whole h x w map: a tile's halo reads it wherever it lies and is zero-padded at
       the true image border only, so every pixel inside the rectangle is bit-identical to the whole-map launch's.  All four zero
       = the whole map.  Otherwise 0 <= roi_y0, roi_y0 + roi_h <= ho (x alike), roi_h, roi_w > 0, no statistics; any other kernel
       (halo 0 / 1 / 2 / 4 / 7) or a rectangle outside the map: WOFT_EINVAL -- never a silent whole-map launch.  The two layers of
       woft_conv2d_pair carry a rectangle each. */
    int32_t roi_y0, roi_x0, roi_h, roi_w;
} woft_conv_params;

int woft_conv2d(const woft_conv_params* p, void* stream);
/* Two INDEPENDENT layers in one launch: both must select the same kernel instance -- same precision (split-bf16 only),
 * halo mode (0 = per-tap kernel, any tap shapes; 8 / 12 = register-streamed kernel, equal tap shape; 16 = streamed GEMM
 * kernel: a 1x1 and a flat layer, or two of a kind, each with its own tile_n), tile_m / tile_n; no InstanceNorm
 * statistics.  The first layer's workgroups are dispatched first.  Results are those of two woft_conv2d calls; what is
 * saved is one kernel boundary and the partly empty last round of workgroups of each launch (the motion encoder's
 * correlation and flow branches, update.py:91-95, are independent until `conv` joins them).  WOFT_EINVAL when the layers
 * do not share a kernel: the caller launches them one after the other. */
int woft_conv2d_pair(const woft_conv_params* a, const woft_conv_params* b, void* stream);
/* Host frame -> device (the plugin API hands track() a numpy frame per call: TRK:57-62, WOFT_demo.py:61-78).  `src` is
 * pageable host memory, `pinned` a page-locked staging buffer and `dev` the device buffer, `bytes` each.  The frame is moved in
 * n_chunks pieces: piece k is copied src -> pinned by the calling thread and its asynchronous H2D copy is enqueued on `stream`
 * at once, so the DMA of piece k runs under the host memcpy of piece k + 1 (one memcpy of the whole frame followed by one H2D
 * copy serialises the two: 0.35 ms per 1080p frame; 4 pieces: 0.18 ms; more pieces lose to the ~20 us per hipMemcpyAsync call).
 * Returns after the last piece is ENQUEUED: `pinned` may be rewritten once the stream has passed this point (the caller records an
 * event).  (Measured alternative, what the Python host now does by default: the runtime's own pageable copy, 0.13 ms.) */
int woft_upload_u8(const void* src, void* pinned, void* dev, int64_t bytes, int32_t n_chunks, void* stream);
/* fp32 array (n % 4 == 0) -> bf16 planes hi = bf16(x), lo = bf16(x - hi) (lo may be NULL): the
 * split form of a dynamic B operand (fmap2 in the correlation GEMM). */
int woft_split_bf16(const float* x, int64_t n, void* hi, void* lo, void* stream);
/* 3x3, stride 1, zero padding 1, cout in {1, 2}, cin_pad in {128, 256} (the flow head's second conv,
 * update.py:10-17: hidden -> 2), exact fp32 FMAs on the vector ALUs instead of a 97 % padded matrix-core tile.
 * in: NHWC fp32 with channel stride cs; wgt: packed fp32 rows [cout][9 * cin_pad] (k = tap * cin_pad + c, as
 * woft_conv2d's fp32 weights); out[pixel * ldo + co_off + o] = bias[o] + sum. */
int woft_conv3x3_narrow(const float* in, int32_t cs, int32_t n_img, int32_t h, int32_t w, int32_t cin_pad,
                        const float* wgt, const float* bias, int32_t cout, float* out, int64_t ldo, int32_t co_off,
                        void* stream);
/* The flow head's second conv and the coordinate update in one launch (update.py:10-17, weighted_raft.py:236-237:
 * delta = conv3x3(in) (2 channels, as woft_conv3x3_narrow, also stored to delta[pixel * ld_delta + 0..1]);
 * coords1 += delta; flow = coords1 - grid written as woft_coords_update writes it (flow4, flow_cat optional).
 * One image of h x w pixels; the same fp32 operations as the two separate calls. */
int woft_flow_head_update(const float* in, int32_t cs, int32_t h, int32_t w, int32_t cin_pad, const float* wgt,
                          const float* bias, float* delta, int64_t ld_delta, float* coords1, float* flow4,
                          float* flow_cat, int32_t ld_cat, void* stream);
/* Second half of the flow head when its first conv ran with WOFT_EPI_FLOWHEAD: delta[q][o] = bias2[o] + sum over the
 * 3x3 taps (ky, kx) and the n_planes column-tile planes of part[(plane * h * w + q + (ky-1) * w + (kx-1)) * ld +
 * (ky * 3 + kx) * 2 + o] (ld >= 20, % 4 == 0; pixels outside the image contribute nothing: zero padding, update.py:14; planes
 * first, then taps, in a fixed order);
 * then, exactly as woft_flow_head_update: delta stored, coords1 += delta, flow = coords1 - grid written to flow4 /
 * flow_cat (optional).  One image of h x w pixels. */
int woft_flow_head_gather(const float* part, int32_t n_planes, int32_t ld, int32_t h, int32_t w, const float* bias2,
                          float* delta, int64_t ld_delta, float* coords1, float* flow4, float* flow_cat, int32_t ld_cat,
                          void* stream);
/* x (n floats, n % 32 == 0) -> n/32 lines of 128 bytes, line = [bf16 hi of 32 values | bf16 lo of the same 32],
 * hi = bf16(x), lo = bf16(x - hi): the operand format of woft_corr_gemm_bf16 with terms = 3. */
int woft_split_bf16_lines(const float* x, int64_t n, void* out, void* stream);
/* All-pairs correlation (corr.py:62-69) on pre-split operands: out[i][j] = alpha * <A[i], B[j]>, i < m, j < n.
 * terms = 3 (hi*hi + hi*lo + lo*hi, fp32-emulating): a / b = woft_split_bf16_lines of fmap1 [rows_a][k] /
 * of woft_tile_rows(fmap2) [rows_b][k]; terms = 1: a / b = their plain bf16 planes (woft_split_bf16 hi), k % 64 == 0.
 * rows_a, rows_b: allocated rows, multiples of 128 (rows beyond m / n are read, their products never stored).
 * out: fp32 [m][ldo], or -- out_bf16 != 0 -- bf16 [m][ldo] (fp32 accumulators rounded to nearest even once, at the
 * store): the bf16-storage volume of the plain-bf16 operating point (2096 B per pixel and lookup). */
int woft_corr_gemm_bf16(const void* a, const void* b, int64_t m, int64_t n, int64_t rows_a, int64_t rows_b, int32_t k,
                        float alpha, void* out, int64_t ldo, int32_t terms, int32_t out_bf16, void* stream);

/* InstanceNorm (extractor.py:28-32,129-130; nn.InstanceNorm2d eps=1e-5, biased variance):
 * finalize per-channel statistics from the conv epilogue's partial sums ... */
int woft_inorm_finalize(const float* stat_sum, const float* stat_sq, int32_t n_part, int32_t ld,
                        int32_t channels, int32_t channels_pad, int64_t count, float eps,
                        float* mean, float* rstd, void* ws, void* stream);   /* mean/rstd[channels..channels_pad) := 0 */
/* ws: NULL (one workgroup does it all), or woft_inorm_ws_bytes() bytes of device scratch, ZEROED ONCE by the caller and
 * then owned by the calls on one stream (it holds the cross-workgroup partial sums and their ticket counter, which every
 * call leaves at zero); channels_pad <= 256, ld % 4 == 0. */
int64_t woft_inorm_ws_bytes(void);
/* ... and apply them.  mode 0: (x-mean)*rstd ; 1: relu(.) ; 2: relu(res' + relu(.)), where res' = res (res_mode 0), or
 * -- res being the RAW conv output of the block's shortcut, normalised here with its own statistics -- (res-res_mean)*res_rstd
 * (res_mode 1; the 1x1 downsample branch, extractor.py:40-45) or relu of that (res_mode 2; the block input). */
int woft_inorm_apply(const float* x, const float* mean, const float* rstd, const float* res,
                     const float* res_mean, const float* res_rstd, int32_t res_mode,
                     float* out, int64_t n_pix, int32_t channels, int32_t mode, void* stream);

/* uint8 BGR HWC image -> normalised RGB NHWC4 fp32 (2*x/255-1, 4th channel 0).
 * optical_flow/raft.py:113-120 + weighted_raft.py:194-195.  replicate-pads to (hp, wp) with the
 * top/left offsets (pad_top, pad_left)  (utils/utils.py:7-19 InputPadder). */
int woft_preprocess_bgr_u8(const uint8_t* img, int32_t h, int32_t w, float* out,
                           int32_t hp, int32_t wp, int32_t pad_top, int32_t pad_left, void* stream);

/* 2x2 stride-2 average pool of an NHWC feature map, floor sizes (corr.py:25-27 applied to
 * fmap2 instead of the volume: identical by linearity, as corr.py:77-81 does). */
int woft_avgpool2_nhwc(const float* in, int32_t h, int32_t w, int32_t c, float* out, void* stream);

/* The target feature pyramid of the volume-free correlation (corr.py:25-27,77-81) in ONE launch: from the level-0 map
 * in [h*w][c] fp32, the (levels - 1) pooled maps pooled[l-1] = woft_avgpool2_nhwc applied l times (floor sizes, fp32,
 * bit-identical to the chained calls) and every level's split operand split[l] -- terms = 3: woft_split_bf16_lines of
 * level l, terms = 1: woft_split_bf16's hi plane.  c % 32 == 0, 1 <= levels <= 4. */
int woft_feature_pyramid(const float* in, int32_t h, int32_t w, int32_t c, int32_t levels, float* const* pooled,
                         void* const* split, int32_t terms, void* stream);

/* Correlation lookup, corr.py:29-59 + utils/utils.py:59-73.
 * vol[l]: level l of the pyramid as [P][ht_l][wt_l][4][4] fp32: the target plane of each source pixel
 * in 4x4 tiles (64 contiguous bytes), ht = ceil(H_l/4), wt = ceil(W_l/4), zeros beyond the map.  The
 * producer is the correlation GEMM run against woft_tile_rows(fmap2_l).  coords: [P][2] (x,y) at level 0.
 * out: [P][ldo] with channel l*(2r+1)^2 + i*(2r+1) + j  <-  sample at (x/2^l + i - r, y/2^l + j - r). */
typedef struct woft_lookup_params {
    const void* vol[4];     /* fp32, or bf16 when vol_bf16 (woft_corr_gemm_bf16 with out_bf16) */
    int32_t ht[4], wt[4];   /* tiles per column / row at level l */
    int64_t plane[4];       /* elements per source pixel at level l (>= ht*wt*16) */
    int32_t levels, radius;
    const float* coords;
    int64_t n_pix;
    float* out;
    int32_t ldo;
    int32_t vol_bf16;       /* 0: fp32 volume (2896 B per pixel and call, r = 4), 1: bf16 storage (2096 B), fp32 out */
    int32_t ablate;         /* developer knob of tools/bench_lookup.py (1: no volume reads, 2: no output); 0 in production */
} woft_lookup_params;
int woft_corr_lookup(const woft_lookup_params* p, void* stream);
/* Volume-free correlation lookup (the reference's alternate_corr path: corr.py:72-100 and its alt_cuda_corr
 * extension): the same samples as woft_corr_lookup computed directly from the feature maps,
 * corr_l(p, q) = alpha * <f1[p], f2_l[q]>, f2_l = fmap2 average-pooled l times -- no P x P volume in memory.
 * f1 / f2[l]: row-major split operands in the format of woft_corr_gemm_bf16 (terms = 3: woft_split_bf16_lines,
 * terms = 1: the bf16 plane; terms = 0, exact fp32: the fp32 feature rows themselves, k % 32 == 0, products on
 * v_mfma_f32_32x32x2_f32 in the order of woft_conv2d's fp32 kernel), one row of k features per pixel; every correlation
 * value is the one that GEMM would have produced (same products, same order).  Cost grows with the spread of the flow inside each 8 x 8
 * block of source pixels (bounding box of their windows); results do not depend on it. */
typedef struct woft_lookup_otf_params {
    const void* f1;         /* [hf*wf][k] source features (split)                                  */
    const void* f2[4];      /* [h[l]*w[l]][k] target features of level l (split)                    */
    int32_t h[4], w[4];
    int32_t levels, radius, terms;
    int32_t hf, wf, k;
    float alpha;            /* 1 / sqrt(k)  (corr.py:68)                                            */
    const float* coords;    /* [hf*wf][2]                                                           */
    float* out;             /* [hf*wf][ldo], channel order of woft_corr_lookup                      */
    const int32_t* need;    /* optional [hf*wf]: source pixels whose samples are wanted (non-zero); an 8 x 8 block without
                               any is skipped (its output rows are left untouched).  NULL: every pixel                 */
    int32_t ldo;
    int32_t ablate;         /* developer knob of tools/bench_lookup_otf.py (1: no target-row stream after the first steps,
                               2: no MFMAs, 4: no window scatter, 8: no interpolation / output); 0 in production */
    /* Optional (fh_part != NULL): the previous refinement iteration's woft_flow_head_gather, folded into this launch.
       Before a workgroup reads the lookup centres of its 8 x 8 source pixels it finishes the flow head for exactly those
       pixels -- delta = fh_bias + 3x3 sum of the partial products (same operations and order as woft_flow_head_gather) --
       and writes coords += delta (coords is then read-write), fh_delta, fh_flow4 and fh_flow_cat as that call does.  No
       other workgroup reads these pixels' coordinates, and every later launch on the stream sees the updated flow.       */
    const float* fh_part;   /* [fh_planes][hf*wf][fh_ld] (fh_ld >= 20, % 4 == 0)                     */
    const float* fh_bias;   /* [2] or NULL                                                          */
    float* fh_delta;        /* [hf*wf][fh_ld_delta]                                                 */
    float* fh_flow4;        /* [hf*wf][4] or NULL                                                   */
    float* fh_flow_cat;     /* [hf*wf][fh_ld_cat] (2 values written) or NULL                        */
    int32_t fh_planes, fh_ld, fh_ld_delta, fh_ld_cat;
    /* Region-restricted launch.  roi_* (all zero: the whole map): only the 8 x 8 blocks (origins at multiples of 8) that intersect the
       pixel rectangle [roi_y0, roi_y0 + roi_h) x [roi_x0, roi_x0 + roi_w) are launched; they run whole (all their pixels inside the
       map), every other block's coordinates and output rows are left untouched.  smp_* (all zero: every launched block): of the
       launched blocks only those that intersect this second rectangle compute samples; the others stop after the folded flow-head
       gather / coordinate update (fh_part != NULL) of their pixels -- the next iteration's flow input is needed further out than its
       lookup samples.  Both rectangles must lie inside the map with positive sizes, else WOFT_EINVAL. */
    int32_t roi_y0, roi_x0, roi_h, roi_w;
    int32_t smp_y0, smp_x0, smp_h, smp_w;
} woft_lookup_otf_params;
int woft_corr_lookup_otf(const woft_lookup_otf_params* p, void* stream);
/* Correlation band: the correlations of the volume-free lookup around the identity, computed once per flow.
 * For source pixel p = (x, y) (row y * wf + x) and level l the band holds alpha * <f1[p], f2_l[q]> for the cells
 *     q = (floor(x / 2^l) - radius - m_l + bx,  floor(y / 2^l) - radius - m_l + by),   0 <= bx, by < W_l = 2 (radius + 1 + m_l),
 * i.e. every cell of every (2 radius + 2)^2 window whose centre cell floor(coords / 2^l) lies within +-m_l cells of
 * floor(p / 2^l); cells outside the level's map hold 0 (the lookup's zero padding).  m_0 = WOFT_BAND_M0 and
 * m_l = ceil(m_0 / 2^l): a centre within [-m_0, m_0) cells of p at level 0 stays within +-m_l of floor(p / 2^l) at level l
 * (floor((x + d) / 2^l) - floor(x / 2^l) lies in [-ceil(m_0 / 2^l), ceil(m_0 / 2^l)] for -m_0 <= d < m_0).
 * Layout (floats): band[(pixel * rows + row_off_l + bx) * WOFT_BAND_LD + by], row_off_l = W_0 + ... + W_(l-1), rows = the sum
 * over all levels: x-major rows of 64 bytes, entries by >= W_l are zero.  radius <= 4 (W_0 <= WOFT_BAND_LD).
 * radius 4, 4 levels: W = 16, 14, 12, 12 -> 54 rows = 3456 bytes per source pixel. */
#define WOFT_BAND_M0 3
#define WOFT_BAND_LD 16
#define WOFT_BAND_M(l) ((WOFT_BAND_M0 + (1 << (l)) - 1) >> (l))
#define WOFT_BAND_W(radius, l) (2 * ((radius) + 1 + WOFT_BAND_M(l)))
/* m[l], w[l], row_off[l] of `levels` levels (each may be NULL) -> rows per source pixel, or WOFT_EINVAL. */
int woft_corr_band_geometry(int32_t radius, int32_t levels, int32_t* m, int32_t* w, int32_t* row_off);
typedef struct woft_lookup_band_params {
    woft_lookup_otf_params otf; /* as for woft_corr_lookup_otf (terms 1 or 3; ablate = 0)                          */
    float* band;                /* [hf*wf][rows][WOFT_BAND_LD]                                                     */
    int32_t* miss;              /* [hf*wf]: 1 where the pixel's 8 x 8 block was launched and missed the band, else 0 */
    int32_t* miss_count;        /* [1]: + 1 per missed block                                                      */
    int32_t defer_samples;      /* woft_corr_lookup_band only.  Non-zero: everything as with 0 (need / roi_* / smp_* rules, folded
                                   flow-head gather with all its stores, hit test, miss flags, miss counter) except that the samples
                                   of HIT blocks are not written -- their rows of otf.out are left untouched; woft_conv1x1_band
                                   interpolates them inside convc1's launch.  Missed blocks are the fallback's as before.        */
} woft_lookup_band_params;
/* Fills the band from otf.f1 / otf.f2 (every value bit-identical to woft_corr_gemm_bf16's for that pair: the volume-free
 * lookup's chunk loop on the band's bounding boxes); reads no coordinates, ignores need / fh_* / roi_* / smp_* / out. */
int woft_corr_band_build(const woft_lookup_band_params* p, void* stream);
/* The volume-free lookup with the correlations read from the band.  Prologue (need, roi_*, smp_*, folded flow-head gather)
 * as woft_corr_lookup_otf, same operations in the same order.  An 8 x 8 block HITS when for every pixel of it inside the map
 * and every level both coordinates of floor(coords / 2^l) lie within +-m_l of floor(p / 2^l): its samples are interpolated
 * from the band (woft_corr_lookup's arithmetic) and its miss flags cleared.  Otherwise no sample is written, its flags are
 * set and *miss_count grows by one: woft_corr_lookup_otf with need = miss, fh_part = NULL and the same rectangles then
 * computes exactly the missed blocks.  Blocks skipped by need or smp_* are flagged 0. */
int woft_corr_lookup_band(const woft_lookup_band_params* p, void* stream);
/* The motion encoder's convc1 (update.py:89; 324 lookup samples -> 256, 1x1) with the band lookup's sampling inside its launch
 * (csrc/conv_1x1_band.hip): the third launch of an iteration after woft_corr_lookup_band(defer_samples = 1) and its fallback
 * woft_corr_lookup_otf(need = miss).  A workgroup owns one 8 x 8 block of source pixels (the band lookup's blocks, order and XCD
 * mapping) x all 256 columns.  It reads the block's coordinates -- already updated; nothing is gathered here -- derives window
 * origins and fractions with the band lookup's expressions and applies the hit rule itself (block-uniform; the miss flags are
 * not read, the band is never addressed outside a pixel's rows).  Hit: the levels' band rows stream through LDS and are
 * interpolated with the band lookup's arithmetic, cell for cell, into the split A tiles of the streamed GEMM kernel; the samples
 * never reach memory.  Miss: the block's rows are loaded from c1->in0, where the fallback has just written them.  Then
 * conv1x1_kernel's K loop and epilogue: 11 chunks of 32 channels (324..351 zero), ascending, same products in the same order --
 * c1->out equals woft_conv2d's on the three-launch form bit for bit.  f1 (optional): a flat layer (convf1) that shares the launch
 * as in woft_conv2d_pair, on the workgroups behind the blocks'.
 * Instance: bp->otf radius 4, k 256, 4 levels, no need / roi_* / smp_* / ablate, otf.out == c1->in0 and otf.ldo == c1->cs0;
 * c1: halo 16, 1x1, n_img 1, h x w = hf x wf, cin_pad 352, cout_pad 256, tile_n 256, no in1 / statistics / rectangle, an
 * element-wise or GRU epilogue; precision 1, 2 or 3 (the band's terms, 1 or 3, are independent of it: the band holds fp32
 * correlations); f1 as woft_conv2d_pair asks of a flat partner -- the same precision -- and no rectangle.  bp's fh_* fields are ignored.  Anything else: WOFT_EINVAL before any launch. */
int woft_conv1x1_band(const woft_conv_params* c1, const woft_conv_params* f1, const woft_lookup_band_params* bp, void* stream);
/* NHWC map [h][w][c] -> its rows in 4x4-tile order [(ceil(h/4)*ceil(w/4)*16)][c], zero rows outside
 * the map: the B operand of the correlation GEMM that yields the tiled volume layout above. */
int woft_tile_rows(const float* in, int32_t h, int32_t w, int32_t c, float* out, void* stream);

/* coords1 += delta; flow = coords1 - coords0 (weighted_raft.py:232,237).
 * delta: [P][ld_delta] (first two channels); flow4: [P][4] = (fx, fy, 0, 0);
 * flow_cat: optional, writes (fx, fy) at flow_cat[p*ld_cat + 0..1]. */
int woft_coords_update(float* coords1, const float* delta, int32_t ld_delta, int32_t wf, int64_t n_pix,
                       float* flow4, float* flow_cat, int32_t ld_cat, void* stream);
int woft_coords_init(float* coords1, int32_t hf, int32_t wf, float* flow4, float* flow_cat,
                     int32_t ld_cat, void* stream);
/* Warm start (csrc/warm.hip; weighted_raft.py:184,223-224 and raft.py: coords1 = coords1 + flow_init).
 * woft_coords_init_flow: woft_coords_init with coords1 = grid + flow_init.  flow_init: planar [2][hf][wf] fp32 (x plane, y
 * plane) in 1/8-resolution pixels of the padded image, what the reference network's forward() receives.  flow4 / flow_cat
 * (optional, woft_coords_update's layout) receive flow_init itself, bit for bit -- not (grid + flow_init) - grid.
 * -1 (before any launch) on a NULL coords1 / flow_init or hf, wf <= 0. */
int woft_coords_init_flow(float* coords1, const float* flow_init, int32_t hf, int32_t wf, float* flow4, float* flow_cat,
                          int32_t ld_cat, void* stream);
/* forward_interpolate (raft_core/utils/utils.py:28-56), the routine that carries a flow from one video frame pair to the
 * next.  flow, out: planar [2][hf][wf] fp32, distinct buffers.  Point i (row-major, at (x0, y0)) lands at
 * (x1, y1) = (x0 + dx, y0 + dy), computed in fp64, and is valid iff 0 < x1 < wf and 0 < y1 < hf (strictly).  Every grid
 * cell receives (dx, dy) of the valid point whose landing position is nearest to it: squared Euclidean distance
 * ddx*ddx + ddy*ddy in fp64 without contraction; of equally near points the one with the LOWEST index (the reference's
 * scipy griddata leaves ties unspecified).  Deviation: without any valid point the reference raises; here out is all zeros.
 * Exhaustive search (hf*wf candidates per cell), deterministic: no atomics, fixed order.
 * -1 (before any launch) on a NULL pointer, flow == out, hf, wf <= 0 or hf*wf > 2^30. */
int woft_forward_interpolate(const float* flow, int32_t hf, int32_t wf, float* out, void* stream);

/* Flow sampling, chaining and the forward-backward check (csrc/flow_chain.hip; utils/interpolation.py).  DESIGN.md section 16.
 * All planes contiguous fp32, [c][h][w]; flows [2][h][w], x plane first; grid coordinates x = column, y = row
 * (utils/misc.py: torch_get_featuremap_coords).  One point / pixel per lane, no LDS, no atomics, no workspace.  Every integer
 * index is formed from a float already clamped into the plane: no coordinate, finite or not, addresses outside it.
 * h, w <= 2^24 (so that w - 1, h - 1 are exact in fp32).
 *
 * woft_sample_bilinear: bilinear_interpolate_torch (interpolation.py:92-133) in fp32, operation for operation.
 *   x0 = floor(x), x1 = x0 + 1, both then clamped to [0, w-1] (y alike); the weights (x1-x)*(y1-y), (x1-x)*(y-y0),
 *   (x-x0)*(y1-y), (x-x0)*(y-y0) from the CLAMPED corners as floats; out[ch][i] = ((wa*a + wb*b) + wc*c) + wd*d with
 *   a = data[ch][y0][x0], b = [y1][x0], c = [y0][x1], d = [y1][x1], every product and sum rounded on its own (no FMA).
 *   So, as in the reference: a point on or beyond the last row / column, or left of / above the first, samples 0 (weights
 *   of equal corners cancel or vanish); a NaN or infinite coordinate gives NaN.  Bit-equal to the reference's CPU fp32
 *   result for finite coordinates |v| <= 1e9 (beyond int64 the reference's float -> integer conversion is unspecified).
 *   out: [c][n].  n == 0: nothing is launched.  -1 on a NULL pointer, c <= 0, n < 0, h or w <= 0 or > 2^24.
 *
 * The other two use this project's EDGE-EXACT sampler s(f, q) (the reference sampler's zeros on the last row / column would
 * be wrong in a chain): q = ((float)x + fab_x, (float)y + fab_y) in fp32; q is valid iff 0 <= qx <= w-1 and 0 <= qy <= h-1
 * (a NaN is not); x0 = floor(qx), x1 = min(x0+1, w-1), ax = qx - x0 (y alike);
 * s = (1-ay)*((1-ax)*d00 + ax*d01) + ay*((1-ax)*d10 + ax*d11) per plane.
 *
 * woft_flow_chain: chain_flow (interpolation.py:9-23, unfinished there) as its docstring says: fac = fab + s(fbc, q); an
 *   invalid q gives NaN in both planes (the fill_value of the reference's FlowInterpolator).  fac may not alias fbc.
 *   -1 on a NULL pointer, h or w <= 0 or > 2^24.
 *
 * woft_flow_fb: forward-backward consistency.  b = s(fba, q); e2 = |fab + b|^2; bound = alpha*(|fab|^2 + |b|^2) + beta;
 *   err[h][w] = sqrt(e2); ok[h][w] = 1.0f iff q is valid and e2 <= bound, else 0.0f.  An invalid q: err = +inf, ok = 0; a
 *   NaN anywhere in the compare: ok = 0.  Either of err / ok may be NULL, not both.
 *   -1 on a NULL flow, both outputs NULL, h or w <= 0 or > 2^24, alpha or beta negative, NaN or infinite. */
int woft_sample_bilinear(const float* data, int32_t c, int32_t h, int32_t w, const float* x, const float* y, int64_t n,
                         float* out, void* stream);
int woft_flow_chain(const float* fab, const float* fbc, int32_t h, int32_t w, float* fac, void* stream);
int woft_flow_fb(const float* fab, const float* fba, int32_t h, int32_t w, float alpha, float beta, float* err, float* ok,
                 void* stream);

/* Multi-delta chaining (csrc/flow_multi.hip).  DESIGN.md section 18.  One candidate chain template -> s -> t is folded into a
 * running per-pixel best; a tracker calls it once per temporal stride and keeps, per pixel, the most reliable chain.
 * All planes contiguous fp32 [h][w], flows [2][h][w], best_sel an int32 plane; h, w <= 2^24.  The sampler s(f, q), its validity
 * rule and its address rule are those of woft_flow_chain above.  One pixel per lane, no LDS, no atomics, no workspace.
 *
 * Candidate k: prev_flow / prev_cost / prev_vis = the stored result template -> s (all three NULL: s is the template itself --
 * flow 0, cost 0, vis 1, nothing is read; any other mix of NULLs is an error); step_flow = the flow s -> t (required);
 * step_wlogit = its reliability logit (NULL: the step costs the scalar unit_cost >= 0); step_mlogit = its visibility logit
 * (NULL: the step's visibility is 1).  Per template pixel p = (x, y):
 *   q    = p + prev_flow(p) in fp32                                 (p for the NULL prev)
 *   flow = prev_flow(p) + s(step_flow, q)
 *   cost = prev_cost(p) + softplus(-s(step_wlogit, q))              (the logit is interpolated, then converted;
 *                                                                    log1pf(expf(-l)), for l < 0 as -l + log1pf(expf(l)))
 *   vis  = prev_vis(p) * sigmoid(s(step_mlogit, q))
 *   valid    = q inside [0, w-1] x [0, h-1], and flow, cost, vis and both interpolated logits finite (a NaN anywhere, or an
 *              infinite logit under a tap, makes the candidate invalid)
 *   occluded = vis < vis_thr                                        (vis_thr in [0, 1])
 * The candidates are ordered by the key (occluded, cost), lexicographically.  A valid candidate replaces the running best iff
 * the best is empty (first != 0, or best_sel < 0), or the best is occluded and the candidate is not, or both have the same
 * occlusion state and cost < best_cost strictly: an equal key keeps the earlier fold.  An invalid candidate replaces nothing.
 * A replaced pixel gets flow, cost, vis and best_sel = k (k in [0, 127]).  With first != 0 the running best is not read, and
 * the pixel of an invalid candidate is written as flow NaN (both planes), cost +inf, vis 0, sel -1.  The occlusion state of
 * the running best is best_vis < vis_thr with this call's vis_thr.
 * best_* may share no byte with an input plane or with each other.
 * -1 (before any launch) on a NULL step_flow or best_*, a partly-NULL prev triple, an overlap of best_* with a plane of this
 * call, h or w <= 0 or > 2^24, k outside [0, 127], unit_cost negative or NaN, vis_thr outside [0, 1] or NaN. */
int woft_flow_chain_fold(const float* prev_flow, const float* prev_cost, const float* prev_vis, const float* step_flow,
                         const float* step_wlogit, const float* step_mlogit, int32_t h, int32_t w, float unit_cost,
                         float vis_thr, int32_t k, int32_t first, float* best_flow, float* best_cost, float* best_vis,
                         int32_t* best_sel, void* stream);

/* woft_flow_chain_fold on two rectangles, with an optional closing homography (csrc/flow_multi.hip).  DESIGN.md section 26.
 * prev_* and best_* are [th][tw] planes (flows [2][th][tw]): plane pixel (x, y) is template pixel P = (tx0 + x, ty0 + y).
 * step_* are [sh][sw] planes (step_flow [2][sh][sw]) covering the rectangle with origin (sx0, sy0) of frames s and t.  Flows are
 * displacements in frame coordinates.  Per template pixel, in the expression tree of woft_flow_chain_fold:
 *   q    = (float)P + prev_flow                                     fp32 (P itself for the NULL prev triple)
 *   u    = q - (float)(sx0, sy0)                                    fp32; exact wherever the tap is valid (Sterbenz / integers)
 *   valid iff u in [0, sw-1] x [0, sh-1]; the taps, their addresses (from clamped floats) and weights are those of u in [sh][sw]
 *   flow = prev_flow + s(step_flow, u); cost, vis, finiteness rules, key, tie rule and the `first` rule: woft_flow_chain_fold's.
 * post_H (host, 9 doubles row-major, or NULL): r = (double)P + (double)flow, den = h6 rx + h7 ry + h8; the candidate is invalid
 * unless den > 0 and the mapped point is finite; flow = (float)(H r / den - (double)P), in fp64 with one final rounding.
 * With both origins 0, th == sh, tw == sw and no post_H the bytes are woft_flow_chain_fold's.  No LDS, no atomics, no workspace;
 * no input, finite or not, produces an address outside a plane.
 * -1 (before any launch) on everything woft_flow_chain_fold rejects (the overlap rule with each plane's own size), a side <= 0,
 * a negative origin, origin + side > 2^24, a non-finite post_H, post_H[8] != 1 (the host normalises the matrix). */
int woft_flow_chain_fold_window(const float* prev_flow, const float* prev_cost, const float* prev_vis, int32_t th, int32_t tw,
                                int32_t ty0, int32_t tx0, const float* step_flow, const float* step_wlogit,
                                const float* step_mlogit, int32_t sh, int32_t sw, int32_t sy0, int32_t sx0, const double* post_H,
                                float unit_cost, float vis_thr, int32_t k, int32_t first, float* best_flow, float* best_cost,
                                float* best_vis, int32_t* best_sel, void* stream);

/* A fold result as correspondences for the planar fit (csrc/flow_multi.hip).  DESIGN.md section 19.  flow [2][gh][gw], cost, vis
 * [gh][gw] fp32 and sel [gh][gw] int32 are what woft_flow_chain_fold leaves; tmask is the frame-sized template mask of
 * woft_tc_select, uint8 [mh][mw] with gh <= mh, gw <= mw, pixel (x, y) of the grid at tmask[y * mw + x] (NULL: every pixel counts;
 * mh, mw are then not read).  Per pixel i = y * gw + x, n = gh * gw:
 *   valid  = 0 <= sel[i] <= 127 and flow_x, flow_y, cost, vis all finite       (the fold writes no sel above 127)
 *   dst[i] = (float)x + flow_x, dst[n + i] = (float)y + flow_y, one fp32 add each; NaN in both where not valid.  The [2][n]
 *            layout woft_tc_select* reads, whose bounds check drops NaN.
 *   w[i]   = expf(-cost) where valid, else 0: the product of the chain's sigmoid(reliability logit).  w may be NULL: nothing is
 *            computed or stored for it.
 *   ok[i]  = 1.0f where valid and not (vis < vis_thr), else 0.0f: the fold's occlusion rule (vis == vis_thr is not occluded), to
 *            be gated at 0.5 in the visibility slot of woft_tc_select_vis.
 *   hist   (may be NULL) int32 [WOFT_CHAIN_HIST], over the pixels whose tmask byte is non-zero: hist[s] = pixels with ok = 1 and
 *            sel = s, hist[128] = pixels that are not valid, hist[129] = valid but occluded pixels.  Zeroed by this call on the
 *            stream; blocks count in LDS and add their non-zero counters with integer atomics: deterministic.  The counters are
 *            int32: meaningful for fewer than 2^31 masked pixels.
 * One pixel per lane in the fold's geometry, no workspace, no floating-point atomics.  No input value addresses anything but
 * the range-checked sel, which indexes the LDS counters.
 * -1 (before any launch) on a NULL flow / cost / vis / sel / dst / ok, gh or gw <= 0 or > 2^24, mh < gh or mw < gw with a tmask,
 * vis_thr outside [0, 1] or NaN, an output that shares a byte with an input or with another output. */
#define WOFT_CHAIN_HIST 130
int woft_chain_tc(const float* flow, const float* cost, const float* vis, const int32_t* sel, const uint8_t* tmask, int32_t gh,
                  int32_t gw, int32_t mh, int32_t mw, float vis_thr, float* dst, float* w, float* ok, int32_t* hist, void* stream);
/* woft_chain_tc on a template rectangle (csrc/flow_multi.hip).  DESIGN.md section 26.  The [gh][gw] planes are those of
 * woft_flow_chain_fold_window: pixel (x, y) is template pixel (tx0 + x, ty0 + y) of a frame_h x frame_w frame; tmask is the
 * CROPPED mask, pixel (x, y) of the window at tmask[y * mw + x].  dst (window coordinates, (float)x + flow_x), w and hist: the
 * bytes woft_chain_tc writes for the same planes and mask.  ok is woft_chain_tc's, and additionally 0 where the landing in frame
 * coordinates X = (float)(tx0 + x) + flow_x, Y = (float)(ty0 + y) + flow_y fails the selection kernels' rule:
 * X < 0 or Y < 0 or rintf(X) >= frame_w or rintf(Y) >= frame_h.  (hist counts by woft_chain_tc's `seen`, not by this rule.)
 * -1 (before any launch) on everything woft_chain_tc rejects, a negative origin, origin + side > 2^24, frame_h or frame_w <= 0
 * or > 2^24. */
int woft_chain_tc_window(const float* flow, const float* cost, const float* vis, const int32_t* sel, const uint8_t* tmask,
                         int32_t gh, int32_t gw, int32_t mh, int32_t mw, int32_t ty0, int32_t tx0, int32_t frame_h,
                         int32_t frame_w, float vis_thr, float* dst, float* w, float* ok, int32_t* hist, void* stream);
/* woft_chain_tc for several template masks at once (csrc/flow_multi.hip).  DESIGN.md section 25.  The masks are one bit plane:
 * tbits, uint32 [mh][mw] with gh <= mh, gw <= mw, bit t of tbits[y * mw + x] set where pixel (x, y) lies in target t's mask,
 * 1 <= n_targets <= 32, masks may overlap; bits at and above n_targets are ignored.  dst, w (may be NULL) and ok do not depend on
 * a mask: they have the bytes woft_chain_tc writes.  hist: int32 [n_targets][WOFT_CHAIN_HIST], row t what woft_chain_tc writes
 * for a uint8 mask equal to bit t.  Zeroed by this call on the stream; a wave counts its lanes per (counter, target) with
 * ballots, blocks count in LDS and add their non-zero counters with integer atomics: deterministic, two calls give equal bytes.
 * Same geometry as woft_chain_tc, no workspace, no floating-point atomics; sel indexes the LDS counters after its range check.
 * -1 (before any launch) on a NULL flow / cost / vis / sel / tbits / dst / ok / hist, gh or gw <= 0 or > 2^24, mh < gh or mw < gw,
 * n_targets outside [1, 32], vis_thr outside [0, 1] or NaN, an output that shares a byte with an input or with another output. */
#define WOFT_MULTI_MAX_TARGETS 32
int woft_chain_tc_multi(const float* flow, const float* cost, const float* vis, const int32_t* sel, const uint32_t* tbits,
                        int32_t gh, int32_t gw, int32_t mh, int32_t mw, int32_t n_targets, float vis_thr, float* dst, float* w,
                        float* ok, int32_t* hist, void* stream);
/* woft_chain_tc_multi on a template rectangle (csrc/flow_multi.hip).  DESIGN.md section 28.  What woft_chain_tc_window is to
 * woft_chain_tc: the [gh][gw] planes are the rectangle with origin (tx0, ty0) of a frame_h x frame_w frame, tbits is the bit plane
 * CROPPED to the rectangle (uint32 [mh][mw], gh <= mh, gw <= mw).  dst (window coordinates), w and hist[t]: the bytes
 * woft_chain_tc_multi writes for the same planes and bit plane.  ok is additionally 0 where the landing in frame coordinates
 * X = (float)(tx0 + x) + flow_x, Y = (float)(ty0 + y) + flow_y fails X < 0 or Y < 0 or rintf(X) >= frame_w or rintf(Y) >= frame_h:
 * woft_chain_tc_window's expression, so dst, w, ok are its bytes and hist[t] its histogram for a uint8 mask equal to bit t.
 * One kernel with woft_chain_tc_multi (two instantiations), the same geometry, ballots and LDS counters.
 * -1 (before any launch) on everything woft_chain_tc_multi rejects, a negative origin, origin + side > 2^24, frame_h or frame_w <= 0
 * or > 2^24. */
int woft_chain_tc_multi_window(const float* flow, const float* cost, const float* vis, const int32_t* sel, const uint32_t* tbits,
                               int32_t gh, int32_t gw, int32_t mh, int32_t mw, int32_t n_targets, int32_t ty0, int32_t tx0,
                               int32_t frame_h, int32_t frame_w, float vis_thr, float* dst, float* w, float* ok, int32_t* hist,
                               void* stream);

/* Frame-features record (csrc/features.hip).  DESIGN.md section 20.  What the encoders produce for one image at one padded
 * geometry, P = (hp / 8) * (wp / 8) pixels, as one contiguous fp32 block: record = [P][fdim] fnet map | [P][hdim] net (after
 * tanh) | [P][cdim] inp (after relu) -- 4 * P * (fdim + hdim + cdim) bytes.  Everything else a flow reads of an image (split
 * operands, pyramid, volumes, gate biases) is derived from these.  Streaming copies, 16 bytes per lane and step, no atomics,
 * no workspace; values are moved, never recomputed: every restored float has the bits that were packed.
 * woft_features_pack: the rows of f1 (row stride ld_f1 floats), net (ld_net) and inp (ld_inp: the first cdim channels of the
 *   GRU input buffer, whose rows are wider) -> record.
 * woft_features_unpack, source role (net, xbuf and inp_c all given): record -> fmap rows (ld_fmap), net (ld_net), the first cdim
 *   channels of xbuf's rows (ld_xbuf) and the same values in inp_c (ld_inp_c), in one launch; with fmap_split also the [hi | lo]
 *   lines of the fnet map in the same pass, bit for bit what woft_split_bf16_lines makes of those P rows (needs ld_fmap ==
 *   fdim and fdim % 32 == 0).  Target role (net, xbuf, inp_c and fmap_split all NULL): the fnet map alone -> fmap (ld_fmap).
 *   Nothing outside the named maps is written: rows beyond P and channels beyond the map's count keep what they hold.
 * WOFT_EINVAL before any launch on a NULL record or map (in the source role: any of net, xbuf, inp_c missing), P < 1, a
 * channel count that is not a positive multiple of 4 (or above 4096), a row stride below the channel count or not a multiple
 * of 4, fmap_split outside the conditions above, or a record of 2^31 or more float4s. */
int woft_features_pack(const float* f1, int64_t ld_f1, const float* net, int64_t ld_net, const float* inp, int64_t ld_inp,
                       int64_t P, int32_t fdim, int32_t hdim, int32_t cdim, float* record, void* stream);
int woft_features_unpack(const float* record, int64_t P, int32_t fdim, int32_t hdim, int32_t cdim, float* fmap, int64_t ld_fmap,
                         void* fmap_split, float* net, int64_t ld_net, float* xbuf, int64_t ld_xbuf, float* inp_c,
                         int64_t ld_inp_c, void* stream);

/* Weight-head glue (weighted_raft.py:258-279, 347-384).
 * woft_colsum: total[c] = sum_q f[q][c] in fp64 (ws: [n_part][c] doubles).
 * woft_wh_pack: mean[p] = alpha * <f1[p], total>  (= mean_q vol[p,q], weighted_raft.py:358-361, in its
 *   algebraic form) and the head's input patches (weighted_raft.py:267-272, 363-376):
 *   x8[p][hp][wp][0..3] = lookup[p][(hp*nwin + wp)*4 + 0..3], x8[..][4] = mean[p], x8[..][5..7] = 0.
 * woft_wh_reduce: final 1x1 conv + mean over the patch (weighted_raft.py:341,378-383):
 *   out[p] = bias + mean_t <w, act[p][t][:]>
 * woft_wh_pack with x8 == NULL computes mean[] only.
 * woft_wh_conv0: the head's first conv + ReLU (weighted_raft.py:336; 5 -> 128 channels, 3x3, zero padding) straight
 *   from the lookup buffer and mean[] (same input definition as x8), exact fp32:
 *   out[p][hp][wp][0..127]; wt: fp32 [96][128], wt[(ky*32 + kx*8 + ci)*128 + co]; nwin in {7, 9}.
 *   index (optional): window p of the output is source pixel index[p] (n_pix = number of windows): the head
 *   evaluated on a subset of the source pixels, e.g. the tracker's template-mask region. */
int woft_colsum(const float* f, int64_t n_pix, int32_t c, double* ws, int32_t n_part, double* total, void* stream);
int woft_wh_conv0(const float* lookup, int32_t ld_lookup, const float* mean, int64_t n_pix, int32_t nwin,
                  const float* wt, const float* bias, float* out, const int32_t* index, void* stream);
int woft_wh_pack(const float* lookup, int32_t ld_lookup, const float* f1, int32_t c, const double* f2_total,
                 float alpha, int64_t n_pix, int32_t nwin, float* mean, float* x8, void* stream);
int woft_wh_reduce(const float* act, int32_t c, int32_t nwin2, const float* w, float bias,
                   int64_t n_pix, float* out, void* stream);
/* MaskHead input (external/RAFT/raft_core/weighted_raft.py:295-309; utils/utils.py:59-73): the feature map f (NHWC fp32, h x w,
 * c valid channels, channel stride cs) sampled at n_pix coordinates coords[p] = (x, y) in map pixels:
 *   out[p*ld_out + 0..c) = bilinear_sampler(f, coords[p])
 * with the reference's semantics: grid_sample(align_corners=True, padding_mode='zeros') after the normalisation
 * 2x/(w-1) - 1, 2y/(h-1) - 1 -- the normalise / un-normalise round trip is taken in the same fp32 operations; a corner outside
 * the map contributes 0 (no clamping).  Channels c..ld_out of a row are not written.  fp32 FMAs.
 * -1 (before any launch) on a NULL pointer, c % 4 != 0, cs < c, ld_out < c, cs or ld_out not a multiple of 4, f or out not
 * 16-byte aligned, h < 2 or w < 2 (the reference divides by zero there) or n_pix < 0; n_pix == 0 launches nothing. */
int woft_warp_features(const float* f, int32_t h, int32_t w, int32_t c, int32_t cs, const float* coords, int64_t n_pix,
                       float* out, int32_t ld_out, void* stream);
/* The windows of a window list that a set of full-resolution pixels needs: dyn_index[j] = index[j] if the 1/8-res pixel
 * index[j] lies in the 3x3 neighbourhood of the cell of one of the n = min(count[0], n_max) points pts[i] = (x, y) (image
 * coordinates; cell = ((y + top) >> 3, (x + left) >> 3): the support of the x8 convex upsampling, weighted_raft.py:92-103),
 * else -1.  A negative entry of woft_conv_params.wh0_index / out_index makes the weight-head launches skip that window.
 * bitmap: hf*wf int32 of scratch; n_needed (optional): receives the number of kept windows.  The tracker's fit reads the
 * weights of its Sobol-sampled correspondences only (TRK:287-312 + the subsampler), and the flow alone decides which. */
int woft_wh_needed(const float* pts, const int32_t* count, int32_t n_max, int32_t top, int32_t left, int32_t hf, int32_t wf,
                   const int32_t* index, int32_t n_win, int32_t* bitmap, int32_t* dyn_index, int32_t* n_needed, void* stream);

/* Convex upsampling of flow and weight logits + TC epilogue
 * (weighted_raft.py:92-103,285-288; optical_flow/raft.py:148-159,185-199).
 * coords1: [P][2]; wlow: [P] or NULL; mask: [P][ld_mask] channel k*64 + i*8 + j.
 * Crops to the unpadded window (crop_top, crop_left, h, w) and writes
 *   flow_up [2][h][w]            (may be NULL)
 *   dst     [2][h*w] = grid + flow (may be NULL)
 *   wout    [h*w]   = weights_up (logit, or sigmoid when do_sigmoid)  (NULL if wlow NULL) */
int woft_convex_upsample(const float* coords1, const float* wlow, const float* mask, int32_t ld_mask,
                         int32_t hf, int32_t wf, int32_t crop_top, int32_t crop_left, int32_t h, int32_t w,
                         float* flow_up, float* dst, float* wout, int32_t do_sigmoid, void* stream);
/* The weight output of woft_convex_upsample at a list of pixels only: wsel[i] = wout at pixel pts[i] = (x, y) of the
 * un-padded image, i < min(count[0], n_max) (count: device, may be NULL); same operations, same order. */
int woft_convex_weights_at(const float* pts, const int32_t* count, int32_t n_max, const float* wlow, const float* mask,
                           int32_t ld_mask, int32_t hf, int32_t wf, int32_t crop_top, int32_t crop_left,
                           int32_t do_sigmoid, float* wsel, void* stream);
/* ---- Training of the weight head (weighted_raft.py:318-384) ------------------------------------------
 * The standard head -- three 3x3 convs to 128 channels, a ReLU after each, a closing 1x1 conv, the mean over the 9x9 window --
 * on a compacted list of n_win <= WOFT_WH_TRAIN_MAX_WIN windows, forward layers that keep their activations and the backward
 * of every stage.  Exact fp32 (v_mfma_f32_32x32x2_f32 products = a k-ordered fmaf chain); every sum is deterministic: no
 * floating-point atomics, split sums are written as partials per WOFT_WH_TRAIN_CHUNK windows and added in chunk order.
 * Activations: [window][81 positions][128 channels] fp32; the first layer's input: [window][81][8], woft_wh_pack's x8 rows.
 *
 * woft_convex_weights_at_bwd: adjoint of woft_convex_weights_at with respect to wlow.  g_wsel [n_max]: the gradient of wsel
 *   (rows at and beyond min(count[0], n_max) are never read, nor are those rows of pts).  g_wlow [hf * wf] is written as zeros
 *   first; then the cell of every listed window (index [n_win]: 1/8-resolution cell ids, each at most once; NULL = every cell,
 *   n_win = hf * wf) receives the sum, in point order, of what the points whose 3x3 support holds it send back: the softmaxed
 *   mask coefficient, the 8 * ... / 8 pair and, with do_sigmoid, the sigmoid's derivative (wlow is then read; else it may be
 *   NULL).  Neighbours outside the map receive nothing (zero padding).  A gather: points that share a cell need no atomics.
 * woft_wh_reduce_bwd: adjoint of woft_wh_reduce (nwin2 = 81, c = 128) on the listed windows:
 *   g = g_wlow[index[p]] / 81 (index NULL: g_wlow[p]);  g_act[p][t][c] = g * w6[c] * (act[p][t][c] > 0);
 *   g_w6[c] = sum_{p,t} g * act[p][t][c];  g_b6[0] = sum_p g_wlow[index[p]].  ws: (n_chunks) * 129 doubles.
 * woft_wh_train_conv: one 3x3 layer cin -> 128 (cin = 128, or 8 for the first layer's x8 rows) on 9x9 windows, each window
 *   zero-padded on its own:  y[p][t][co] = sum_{tap,ci} x[p][t + tap][ci] * wt[tap][ci][co]  (wt: [9][cin][128], tap = ky*3+kx),
 *   then with bias: relu(y + bias[co]) -- a forward layer --, or with gate ([n_win][81][128]): y where gate > 0, else 0 -- the
 *   data gradient of a layer when wt holds its transposed, flipped filter and gate the activation below it.  Not both.
 * woft_wh_wgrad: parameter gradient of such a layer:  gw[co][ci][ky][kx] = sum_{p,t} gy[p][t][co] * x[p][t + tap][ci] for
 *   ci < cin_out (gw: [128][cin_out][3][3], the state dict's layout; cin_out = 5 with cin = 8), gb[co] = sum_{p,t} gy[p][t][co].
 *   ws: woft_wh_wgrad_ws_bytes(n_win, cin) bytes of partial sums.
 * All return WOFT_EINVAL before any launch on a NULL required pointer or a size outside the stated range. */
#define WOFT_WH_TRAIN_CHUNK 16
#define WOFT_WH_TRAIN_MAX_WIN (9 * 2048)
int woft_convex_weights_at_bwd(const float* pts, const int32_t* count, int32_t n_max, const float* g_wsel, const float* wlow,
                               const float* mask, int32_t ld_mask, int32_t hf, int32_t wf, int32_t crop_top,
                               int32_t crop_left, int32_t do_sigmoid, const int32_t* index, int32_t n_win, float* g_wlow,
                               void* stream);
int woft_wh_reduce_bwd(const float* act, const float* w6, const float* g_wlow, const int32_t* index, int32_t n_win,
                       float* g_act, double* ws, float* g_w6, float* g_b6, void* stream);
int woft_wh_train_conv(const float* x, int32_t cin, const float* wt, const float* bias, const float* gate, int32_t n_win,
                       float* y, void* stream);
int64_t woft_wh_wgrad_ws_bytes(int32_t n_win, int32_t cin);
int woft_wh_wgrad(const float* gy, const float* x, int32_t cin, int32_t cin_out, int32_t n_win, float* ws, float* gw,
                  float* gb, void* stream);
/* ---- Training of the MaskHead (weighted_raft.py:295-309, 387-422) ------------------------------------
 * The head is an ordinary conv stack over the whole 1/8-resolution map: 3x3 convs with zero padding at the map border, a ReLU
 * after each, a closing 1x1 conv to one logit per pixel.  Maps are NHWC fp32, [hf * wf pixels][channel stride]; channel counts
 * are multiples of 32, cout <= 128, cin <= 512.  A map may come as two sources (the first layer reads [fmap1 | warped fmap2],
 * weighted_raft.py:297-302, without a concatenated copy): channels below c_split from x0, the others from x1 (x1 NULL:
 * c_split = cin).  Exact fp32 (v_mfma_f32_32x32x2_f32 products); no floating-point atomics: the parameter gradients are written
 * as one partial per WOFT_MH_TRAIN_CHUNK tiles of WOFT_MH_TRAIN_TILE positions of a map row (per WOFT_MH_REDUCE_CHUNK pixels
 * for the closing conv) -- a partition of the map that does not depend on the grid -- and added in chunk order in fp64.
 *
 * woft_mh_train_conv: y[p][co] = sum_{tap,ci} x[p + tap][ci] * wt[tap][ci][co]  (wt: [9][cin][cout], tap = ky*3+kx; taps outside
 *   the map read zero), then with bias: relu(y + bias[co]) -- a forward layer (weighted_raft.py:411-422) --, or with gate
 *   ([pixels][gate_cs]): y where gate > 0, else 0 -- the data gradient of a layer when wt holds its transposed, flipped filter and
 *   gate the activation below it.  Not both.
 * woft_mh_wgrad: gw[co][ci][ky][kx] = sum_p gy[p][co] * x[p + tap][ci] (the state dict's layout), gb[co] = sum_p gy[p][co].
 *   ws: woft_mh_wgrad_ws_bytes(hf, wf, cin, cout) bytes of partial sums.
 * woft_mh_reduce_bwd: adjoint of the closing 1x1 conv low[p] = b + <w, act[p]>:  g_act[p][c] = g_low[p] * w[c] * (act[p][c] > 0),
 *   g_w[c] = sum_p g_low[p] * act[p][c], g_b[0] = sum_p g_low[p].  ws: ceil(n_pix / WOFT_MH_REDUCE_CHUNK) * 129 doubles.
 * All return WOFT_EINVAL before any launch on a NULL required pointer or a size outside the stated range. */
#define WOFT_MH_TRAIN_TILE 32
#define WOFT_MH_TRAIN_CHUNK 16
#define WOFT_MH_REDUCE_CHUNK 256
int woft_mh_train_conv(const float* x0, int32_t cs0, const float* x1, int32_t cs1, int32_t c_split, int32_t cin, const float* wt,
                       int32_t cout, const float* bias, const float* gate, int32_t gate_cs, int32_t hf, int32_t wf, float* y,
                       int32_t y_cs, void* stream);
int64_t woft_mh_wgrad_ws_bytes(int32_t hf, int32_t wf, int32_t cin, int32_t cout);
int woft_mh_wgrad(const float* gy, int32_t gy_cs, int32_t cout, const float* x0, int32_t cs0, const float* x1, int32_t cs1,
                  int32_t c_split, int32_t cin, int32_t hf, int32_t wf, float* ws, float* gw, float* gb, void* stream);
int woft_mh_reduce_bwd(const float* act, int32_t act_cs, int32_t c, const float* w, const float* g_low, int32_t n_pix,
                       float* g_act, int32_t g_cs, double* ws, float* g_w, float* g_b, void* stream);
/* ---- Dense adjoint of the convex upsampling (weighted_raft.py:92-103, 305-308) -------------------------
 * woft_convex_upsample_bwd: adjoint of the wout output of woft_convex_upsample with respect to wlow.  g_up [h*w]: the gradient
 *   of the cropped full-resolution map; mask, ld_mask, hf, wf, the crop window and do_sigmoid as in the forward; g_wlow [hf*wf]
 *   is written whole:
 *     g_wlow[q] = sum over the cells n and taps k = ky*3+kx with q = n + (ky-1, kx-1), over the fine positions of n inside the
 *                 crop window, of ((g_up[pixel] * dsig) / 8) * (softmax_k(mask[n])[position] * 8)
 *   dsig = 1, or with do_sigmoid v (1 - v), v the forward's sigmoid output at the pixel recomputed from wlow in the forward's
 *   order of operations (wlow is read only then; else it may be NULL).  Fine positions outside the crop window send nothing;
 *   neighbours outside the map receive nothing (zero padding); mask columns beyond 576 and rows beyond hf*wf are never read.
 *   Two launches, the mask read once: part[n][k] = the sum over the 64 positions of cell n by a fixed butterfly (ws:
 *   woft_convex_upsample_bwd_ws_bytes(hf, wf) = 9 * hf * wf floats), then g_wlow[q] = the partials addressed to q in k order.
 *   No floating-point atomics: two calls give equal bytes.  WOFT_EINVAL before any launch on a NULL required pointer,
 *   ld_mask < 576, non-positive sizes, hf * wf >= 2^28, a crop window that leaves the padded map, or do_sigmoid without wlow. */
int64_t woft_convex_upsample_bwd_ws_bytes(int32_t hf, int32_t wf);
int woft_convex_upsample_bwd(const float* g_up, const float* mask, int32_t ld_mask, const float* wlow, int32_t hf, int32_t wf,
                             int32_t crop_top, int32_t crop_left, int32_t h, int32_t w, int32_t do_sigmoid, float* ws,
                             float* g_wlow, void* stream);
/* Pre-computed flow read from the reference's cache files (utils/caching.py:53-59; raft.py:93-106) to the same
 * outputs: dst[2][h*w] = pixel grid + flow[2][h*w] (may be NULL), wout[h*w] = weights or sigmoid(weights)
 * (weights / wout may be NULL). */
int woft_flow_to_tc(const float* flow, const float* weights, int32_t h, int32_t w, float* dst, float* wout,
                    int32_t do_sigmoid, void* stream);
/* bilinear x8 upsampling, align_corners=True, times 8 (utils/utils.py:82-84), same outputs. */
int woft_upflow8(const float* coords1, const float* wlow, int32_t hf, int32_t wf,
                 int32_t crop_top, int32_t crop_left, int32_t h, int32_t w,
                 float* flow_up, float* dst, float* wout, int32_t do_sigmoid, void* stream);

/* Perspective warp, dst(x) = bilinear src(Hinv x), zeros outside
 * (tracker/YAOF_tracker_single_control.py:89-95).  hinv: 9 doubles on the HOST (by value copy).
 * img: HWC uint8 (c channels).  valid (may be NULL): uint8 1 where warp(ones) > 0. */
int woft_warp_perspective_u8(const uint8_t* img, int32_t h, int32_t w, int32_t c, const double* hinv,
                             uint8_t* out, uint8_t* valid, int32_t nearest, void* stream);

/* Search-window kernels (csrc/window.hip; tracker/WOFT_window.py: the flows of the window tracker run on a rectangle of the frame).
 * A rectangle is rows [y0, y0 + hw) x columns [x0, x0 + ww) of an h x w image and must lie inside it with hw, ww >= 1: else -1.
 *
 * woft_warp_perspective_window_u8: the rectangle of what woft_warp_perspective_u8 writes for the same arguments, into a contiguous
 * hw x ww x c `out` and hw x ww `valid` (either may be NULL, not both; nearest needs out).  Window pixel (i, j) holds exactly the
 * bytes the full-frame call gives destination pixel (x0 + i, y0 + j): one device function serves both (csrc/warp_pixel.h). */
int woft_warp_perspective_window_u8(const uint8_t* img, int32_t h, int32_t w, int32_t c, const double* hinv, int32_t y0,
                                    int32_t x0, int32_t hw, int32_t ww, uint8_t* out, uint8_t* valid, int32_t nearest,
                                    void* stream);
/* Rectangle copy: out (hw x ww x c, contiguous) = img[y0 : y0 + hw, x0 : x0 + ww, :] (h x w x c uint8, c <= 4). */
int woft_crop_u8(const uint8_t* img, int32_t h, int32_t w, int32_t c, int32_t y0, int32_t x0, int32_t hw, int32_t ww,
                 uint8_t* out, void* stream);
/* Bounding box of the non-zero pixels of a uint8 h x w mask: bbox (device) = {rmin, rmax, cmin, cmax, any} as five int32; an
 * all-zero mask gives {0, 0, 0, 0, 0} (utils/geom_utils.py:46-64, Bbox.from_mask).  One launch.
 * hinv != NULL (9 doubles on the host): the mask measured is the nearest-neighbour warp of `mask` by hinv, exactly
 * woft_warp_perspective_u8(mask, h, w, 1, hinv, warped, NULL, 1), and `warped` (h x w, may be NULL) receives it.
 * ws: woft_mask_bbox_ws_bytes() bytes of device scratch, ZEROED ONCE by the caller; every call leaves it zeroed again (calls that
 * share one ws must be ordered by their stream). */
int64_t woft_mask_bbox_ws_bytes(void);
int woft_mask_bbox(const uint8_t* mask, int32_t h, int32_t w, const double* hinv, uint8_t* warped, void* ws, int32_t* bbox,
                   void* stream);
/* woft_mask_bbox with a homography for n_targets masks at once, ONE launch whatever n_targets is.  DESIGN.md section 28.  tbits: the
 * bit plane of woft_chain_tc_multi, uint32 [h][w] (device), 1 <= n_targets <= WOFT_MULTI_MAX_TARGETS; hinv: n_targets x 9 doubles
 * on the HOST, copied by value; bbox: int32 [n_targets][5] (device).  Row t is, integer for integer, what
 * woft_mask_bbox(mask_t, h, w, hinv + 9 t, NULL, ...) writes for mask_t = (bit t of tbits): the same nearest-neighbour warp per
 * frame pixel (csrc/warp_pixel.h), integer maxima; {0, 0, 0, 0, 0} where nothing of the carried mask is set.  Bit t of `skip` set:
 * target t is not measured, its hinv is not read and its row is {0, 0, 0, 0, 0}.  Deterministic: two calls give equal bytes.
 * ws: woft_mask_bbox_multi_ws_bytes(n_targets) bytes (-1 for an n_targets outside [1, 32]) of device scratch under woft_mask_bbox's
 * contract: ZEROED ONCE by the caller, left zeroed by every call.
 * -1 (before any launch) on a NULL tbits / hinv / ws / bbox, h or w <= 0, n_targets outside [1, 32], a non-finite entry of the hinv
 * of a target that is not skipped. */
int64_t woft_mask_bbox_multi_ws_bytes(int32_t n_targets);
int woft_mask_bbox_multi(const uint32_t* tbits, int32_t h, int32_t w, int32_t n_targets, const double* hinv, uint32_t skip, void* ws,
                         int32_t* bbox, void* stream);

/* ---- Synthetic-homography training pairs (csrc/hsynth.hip) ------------------------------------------------
 * This project's own semantics for what the reference's training configs call COCOHSynth (an image, the same image through a known
 * homography, with occluders); the data set's code is not part of the reference.  An occluder is a BGRA texture and the inverse
 * homography that maps the destination frame to that texture.  The array of occluders and its hinv live on the HOST (copied by
 * value); tex is a device pointer, 4-byte aligned (one pixel is read as one dword). */
#define WOFT_HSYNTH_MAX_OCC 4
typedef struct {
    const uint8_t* tex; /* (ho, wo, 4) B, G, R, alpha */
    int32_t ho, wo;
    int32_t pad_;
    double hinv[9];
} woft_hsynth_occluder;
/* woft_hsynth_render: destination pixel (x, y) of the (h, w) frame, channel c:
 *   1. v_c = base ((hs, ws, 3) uint8) at hinv (x, y, 1): the source coordinates, fp64 de-homogenisation, bilinear taps, zero
 *      border and float operations of woft_warp_perspective_u8 before its rounding (one device function, csrc/warp_pixel.h);
 *   2. v_c = gain[c] * v_c + bias[c], a multiply and then an add (gain, bias: 3 floats on the HOST; NULL = 1 / 0);
 *   3. for k = 0 .. n_occ-1 in order, premultiplied compositing: with m the in-texture flag of a tap of occ[k].hinv (x, y, 1),
 *      A_k = bilinear(m * (alpha_tap / 255)), O_kc = bilinear((m * (alpha_tap / 255)) * colour_tap), v_c = (1 - A_k) * v_c + O_kc;
 *   4. out_u8 (h, w, 3) = (uint8) clamp(rintf(v_c), 0, 255); out_f32 (h, w, 3; may be NULL) = v_c; cover (h, w; may be NULL) =
 *      1 - prod_k (1 - A_k).
 * woft_hsynth_labels: template pixel (x, y) of the (hs, ws) base image: (px, py) = hfwd (x, y, 1) de-homogenised in fp64 with
 *   denominator d; flow (2, hs, ws) = ((float)(px - x), (float)(py - y)), written everywhere; inside = d > 0 && 0 <= px <= w-1 &&
 *   0 <= py <= h-1; T = 1 - prod_k (1 - A_k) with A_k of step 3 at occ[k].hinv (px, py, 1) (the alpha field the render composites,
 *   at the non-integer point); visible (hs, ws) = 1 iff inside && T <= lo; valid (hs, ws; uint8 0 / 1) = 0 iff inside && lo < T < hi
 *   (an occluder's soft edge, or a T that is NaN), where visible = 0 too.
 * One launch each, a thread per four adjacent pixels (dword stores when the outputs are 4- / 16-byte aligned, byte and float
 * stores otherwise: the same values); no atomics, no workspace: two calls give equal bytes.  WOFT_EINVAL before any launch on a
 * NULL required pointer (base, hinv, out_u8; hfwd, flow, visible, valid), non-positive sizes, n_occ outside
 * 0 .. WOFT_HSYNTH_MAX_OCC, n_occ > 0 with occ == NULL, an occluder with a NULL or misaligned texture or a non-positive size,
 * !(0 <= lo < hi <= 1), hs * ws or h * w at or above 2^31. */
int woft_hsynth_render(const uint8_t* base, int32_t hs, int32_t ws, const double* hinv, const float* gain, const float* bias,
                       const woft_hsynth_occluder* occ, int32_t n_occ, uint8_t* out_u8, float* out_f32, float* cover, int32_t h,
                       int32_t w, void* stream);
int woft_hsynth_labels(int32_t hs, int32_t ws, const double* hfwd, const woft_hsynth_occluder* occ, int32_t n_occ, int32_t h,
                       int32_t w, float lo, float hi, float* flow, float* visible, uint8_t* valid, void* stream);
/* woft_hsynth_render_bg: woft_hsynth_render with a background behind the warped plane.  bg: (hb, wb, 3)
 * uint8 on the device; hinv_bg: 9 doubles on the HOST, destination frame -> background image; plane: (h, w) float output, may be
 * NULL.  Destination pixel (x, y), channel c:
 *   1. v_c as in step 1 of woft_hsynth_render (the same device function: the zero border already premultiplies it);
 *   2. P = bilinear(m) of the four taps' in-image flags m with the fractional weights of the colour taps: the plane's coverage,
 *      built the way an occluder's A_k is built; P = 0 where hinv's denominator is not positive or all four taps are outside;
 *   3. g_c = bg at hinv_bg (x, y, 1): fp64 de-homogenisation, four bilinear taps with indices CLAMPED to the image (replicate
 *      border: a background has no holes), the float operations of step 1; g_c = 0 where the denominator is not positive or a
 *      coordinate is not finite;
 *   4. v_c = v_c + (1 - P) * g_c: a subtraction, a multiply and an add, in this order;
 *   5. steps 2 - 4 of woft_hsynth_render (gain / bias, occluders, rounding, cover); plane = P.
 * The launch shape, the store paths and the guarantees of woft_hsynth_render (no atomics, no workspace, equal bytes on two calls).
 * WOFT_EINVAL before any launch on bg == NULL (a caller without a background uses woft_hsynth_render), hinv_bg == NULL,
 * non-positive hb / wb, hb * wb at or above 2^31, and everything woft_hsynth_render rejects. */
int woft_hsynth_render_bg(const uint8_t* base, int32_t hs, int32_t ws, const double* hinv, const float* gain, const float* bias,
                          const woft_hsynth_occluder* occ, int32_t n_occ, const uint8_t* bg, int32_t hb, int32_t wb,
                          const double* hinv_bg, uint8_t* out_u8, float* out_f32, float* cover, float* plane, int32_t h, int32_t w,
                          void* stream);
/* woft_hsynth_augment (csrc/hsynth_aug.hip): photometric augmentation of a float frame in_f32 (h, w, 3), one
 * launch.  Pixel (x, y), channel c (memory order B, G, R); all arithmetic fp32, every product followed by its add:
 *   a. blur, separable with replicate border, 0 <= radius <= WOFT_HSYNTH_MAX_BLUR: t_c(x, y) = sum_{j=-r..r} taps[j+r] *
 *      (sum_{i=-r..r} taps[i+r] * in_c(clamp(x+i), clamp(y+j))), both sums in ascending index order starting from 0.f; taps:
 *      2 radius + 1 floats on the HOST (NULL with radius 0: t = in, no LDS touched);
 *   b. colour: u_c = o_c + M_c0 * t_0 + M_c1 * t_1 + M_c2 * t_2 in that order; colour: 12 floats on the HOST, the 3x3 M row-major
 *      and then o (NULL = identity: u = t);
 *   c. noise, skipped when noise_sigma == 0: u_c += noise_sigma * z with idx = (uint32)((y * w + x) * 3 + c),
 *      mix(v): v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16,  a = mix(seed ^ mix(idx)),
 *      b = mix(a + 0x9e3779b9), S = the sum of the four 16-bit halves of a and b, z = (float)(S - 131070) * (float)(sqrt(3) / 65536)
 *      (a sum of four uniforms, unit variance, |z| <= 3.47; a stateless function of seed, pixel and channel);
 *   d. out_f32 (h, w, 3; may be NULL) = u_c; out_u8 (h, w, 3) = (uint8) clamp(rintf(u_c), 0, 255).
 * No atomics, no workspace: two calls give equal bytes.  in_f32 may equal out_f32 only when radius == 0.  WOFT_EINVAL before any
 * launch on a NULL in_f32 / out_u8, non-positive sizes, h * w at or above 2^31, a radius outside 0 .. WOFT_HSYNTH_MAX_BLUR,
 * radius > 0 with taps == NULL or with in_f32 == out_f32, a negative or non-finite noise_sigma. */
#define WOFT_HSYNTH_MAX_BLUR 7
int woft_hsynth_augment(const float* in_f32, int32_t h, int32_t w, const float* taps, int32_t radius, const float* colour,
                        float noise_sigma, uint32_t seed, uint8_t* out_u8, float* out_f32, void* stream);

/* Photometric refinement of a homography (csrc/photo.hip; DESIGN.md section 27, this project's own semantics): inverse-compositional
 * Gauss-Newton of a template (h, w, 3) against a frame (hf, wf, 3), each uint8 or float32 (tmpl_f32 / frame_f32), on the pixels
 * Omega of the uint8 mask (h, w): mask > 0, 1 <= x <= w - 2, 1 <= y <= h - 2, (x - x0) % stride == 0 and (y - y0) % stride == 0 with
 * box = {x0, y0, x1, y1} (HOST, inclusive, inside the template: the mask's bounding box).  S = c0 + c1 + c2; template gradient by
 * central differences; normalised coordinates x~ = (x - cx) / s with cx = (x0 + x1) / 2, cy = (y0 + y1) / 2, s = max(x1 - x0,
 * y1 - y0, 1) / 2.  At a state (M = W N^-1, gain g, bias b in units of S) a pixel is valid iff q = M (x~, y~, 1) has qz > 0 and
 * u = qx / qz in [0, wf - 1), v = qy / qz in [0, hf - 1); I = the bilinear sample of S_frame, (1 - fy) ((1 - fx) s00 + fx s01) +
 * fy ((1 - fx) s10 + fx s11); e = I - g T - b; omega = weight (weights (h, w) float32 or NULL: 1) times the Huber factor
 * (huber_k > 0, in grey levels: k = 3 huber_k; huber_k < 0: none); row a = g [gx~ x~, gx~ y~, gx~, gy~ x~, gy~ y~, gy~, -x~ d,
 * -y~ d], d = gx~ x~ + gy~ y~, and with gain_bias: T, 1.  Everything fp64.
 * woft_photo_eval: out (device) = upper triangle of G = sum omega a a^T row-major (nu (nu + 1) / 2, nu = 10 with gain_bias else 8),
 *   r = sum omega a e (nu), sum weight * rho, sum weight, n_valid, at the state (W HOST 3x3 template -> frame pixels, gain, bias).
 *   Two launches: one partial per workgroup of WOFT_PHOTO_CHUNK candidates, then their sum in index order.
 * woft_photo_refine: iters + 1 (accumulate, step) launch pairs from W0 (HOST), g = 1, b = 0; the step launch records iterate k,
 *   applies the control rules of DESIGN.md section 27 (n_need = the valid-pixel threshold, eps the step in frame pixels of the
 *   box's corners below which the next iterate is the last), solves by Cholesky without a ridge and steps M <- M Delta^-1.
 *   Launches after a stop return at once.  result (device, WOFT_PHOTO_REC * (iters + 2) doubles): [0] status, [1] best iterate or
 *   -1, [2] iterates evaluated, [3..11] the best iterate's W; then per iterate k at WOFT_PHOTO_REC * (1 + k): W_k (9, h33 = 1),
 *   g_k, b_k / 3, sqrt(cost_k) / 3, n_k, step_k (NaN when no step was taken).  Only the first [2] records are written.
 * ws: woft_photo_ws_bytes(x1 - x0 + 1, y1 - y0 + 1, stride) bytes (-1 on a non-positive argument), 8-byte aligned.  No atomics:
 * two calls give equal bytes.  WOFT_EINVAL before any launch on a NULL tmpl / mask / frame / box / W / ws / out / result, h or
 * w < 3, hf or wf < 1, an image of 2^31 pixels or more, a box outside the template or empty, stride < 1, huber_k zero or NaN, a
 * non-finite W / gain / bias / eps, eps < 0, iters outside 0 .. WOFT_PHOTO_MAX_ITERS, n_need < 0. */
#define WOFT_PHOTO_NACC 68
#define WOFT_PHOTO_CHUNK 2048
#define WOFT_PHOTO_REC 16
#define WOFT_PHOTO_MAX_ITERS 64
enum woft_photo_status {
    WOFT_PHOTO_CONVERGED = 0,
    WOFT_PHOTO_MAX_ITERS_REACHED = 1,
    WOFT_PHOTO_TOO_FEW = 2,
    WOFT_PHOTO_SINGULAR = 3,
    WOFT_PHOTO_NONFINITE = 4,
    WOFT_PHOTO_SKIPPED = 5          /* (multi-target forms only: the target was not active) */
};
int64_t woft_photo_ws_bytes(int32_t box_w, int32_t box_h, int32_t stride);
int woft_photo_eval(const void* tmpl, int32_t tmpl_f32, const uint8_t* mask, int32_t h, int32_t w, const float* weights,
                    const void* frame, int32_t frame_f32, int32_t hf, int32_t wf, const int32_t* box, int32_t stride,
                    const double* W, double gain, double bias, int32_t gain_bias, double huber_k, void* ws, double* out,
                    void* stream);
int woft_photo_refine(const void* tmpl, int32_t tmpl_f32, const uint8_t* mask, int32_t h, int32_t w, const float* weights,
                      const void* frame, int32_t frame_f32, int32_t hf, int32_t wf, const int32_t* box, int32_t stride,
                      const double* W0, int32_t iters, int32_t gain_bias, double huber_k, int32_t n_need, double eps, void* ws,
                      double* result, void* stream);

/* The photometric refinement of K targets (1 .. WOFT_MULTI_MAX_TARGETS) of ONE template against ONE frame.
 * Per target the semantics, and the bytes written, are those of woft_photo_eval / woft_photo_refine on that target's mask.
 * bits: the (h, w) uint32 plane of pack_target_bits / woft_chain_tc_multi, bit t of a pixel set where it is in target t (masks may
 * overlap; the words are unsigned, target 31 is the top bit).  weights, stride, iters, gain_bias, huber_k, eps are shared.  HOST
 * arrays: boxes (K, 4) int32 {x0, y0, x1, y1} inclusive, W / W0 (K, 9), gains, biases (K; in units of S), n_need (K), active (K)
 * int32.  A target with active == 0 takes no part: its workgroups return on a uniform branch, its row of `out` is not written and
 * its result block is {WOFT_PHOTO_SKIPPED, -1, 0} with nothing else written; its box, W and n_need are still checked.  When no
 * target is active there is no launch and nothing is written.
 * woft_photo_eval_multi: the accumulate launch on the grid (P_max, K) -- P_t = ceil(nx_t ny_t / WOFT_PHOTO_CHUNK) partials of target
 *   t, P_max the largest over all K boxes; workgroup (p, t) with p >= P_t returns at once -- then one workgroup per target sums its
 *   partials in index order -> out (device, K rows of WOFT_PHOTO_NACC doubles, the first nu (nu + 1) / 2 + nu + 3 of a row written).
 * woft_photo_refine_multi: iters + 1 (accumulate on (P_max, K), step on K) launch pairs whatever K; every target carries its own
 *   state, stop, best and last iterate in its slice of the workspace and stops on its own.  result (device): K blocks of
 *   WOFT_PHOTO_REC * (iters + 2) doubles, each laid out as woft_photo_refine's.
 * ws: woft_photo_multi_ws_bytes(K, P_max) = K (P_max * WOFT_PHOTO_NACC + 18) * 8 bytes (-1 on a non-positive argument).  No atomics:
 * two calls give equal bytes.  WOFT_EINVAL before any launch on everything the single forms reject, K outside 1 ..
 * WOFT_MULTI_MAX_TARGETS, a NULL bits / boxes / W / gains / biases / n_need / active, any box outside the template or empty, any
 * non-finite W / gain / bias entry, any n_need < 0. */
int64_t woft_photo_multi_ws_bytes(int32_t n_targets, int32_t p_max);
int woft_photo_eval_multi(const void* tmpl, int32_t tmpl_f32, const uint32_t* bits, int32_t h, int32_t w, const float* weights,
                          const void* frame, int32_t frame_f32, int32_t hf, int32_t wf, int32_t n_targets, const int32_t* boxes,
                          int32_t stride, const double* W, const double* gains, const double* biases, const int32_t* active,
                          int32_t gain_bias, double huber_k, void* ws, double* out, void* stream);
int woft_photo_refine_multi(const void* tmpl, int32_t tmpl_f32, const uint32_t* bits, int32_t h, int32_t w, const float* weights,
                            const void* frame, int32_t frame_f32, int32_t hf, int32_t wf, int32_t n_targets, const int32_t* boxes,
                            int32_t stride, const double* W0, const int32_t* n_need, const int32_t* active, int32_t iters,
                            int32_t gain_bias, double huber_k, double eps, void* ws, double* result, void* stream);

/* A fold result as the weight map of the photometric refinement, and each target's visible support (csrc/photo_weights.hip;
 * DESIGN.md section 30, this project's own semantics).  cost, vis: the fp32 planes (rows, cols) woft_flow_chain_fold /
 * woft_flow_chain_fold_window leave, the rectangle with origin (ry, rx) of a template (h, w) -- (0, 0) and the planes' size for the
 * full-frame trackers (the planes may be smaller than the template), R0 for the window trackers.  On template pixels (x, y):
 *   raw(x, y) = 0 outside the rectangle; inside it, with c = cost[p], v = vis[p] at p = (y - ry) * cols + (x - rx): 0 unless c is
 *     finite and v >= vis_thr (a NaN v fails, v == vis_thr passes); where the gate passes, mode 0 (gate): 1.0f; mode 1 (soft):
 *     expf(-c) * v in fp32, and a product that is not finite or not > 0 becomes +0.
 *   map(x, y) = min of raw(x + dx, y + dy) over |dx|, |dy| <= radius (0 .. WOFT_PHOTO_WEIGHTS_MAX_RADIUS): neighbours outside the
 *     template are ignored, neighbours inside the template but outside the rectangle count as 0.
 *   support[t] = the number of template pixels with bit t of `bits` set and map > 0, t < n_targets.
 * bits: the (h, w) uint32 plane of pack_target_bits (device), n_targets 1 .. WOFT_MULTI_MAX_TARGETS; bits and support may be NULL with
 * n_targets = 0: no support is computed.  map (device, h * w floats): every entry is written.  support (device, n_targets int32).
 * One launch on 64 x 16 tiles, tile plus halo through LDS, the minimum taken separably (rows, then columns); a workgroup walks
 * several tiles of a column so that its counts leave in one flush.  Determinism: the map has one writer per pixel; the counts are
 * INTEGER sums -- one ballot and population count per target and wavefront row, integer LDS atomics per workgroup, one integer
 * global atomic per target and workgroup after a hipMemsetAsync of `support` on the stream -- so their value does not depend on
 * the order: two calls give equal bytes.  No workspace.  WOFT_EINVAL before the device is touched on a NULL cost / vis / map, a
 * side < 1, a template of 2^31 pixels or more, a rectangle that leaves the template, n_targets outside 0 .. WOFT_MULTI_MAX_TARGETS,
 * a NULL bits or support with n_targets > 0, vis_thr outside [0, 1] or NaN, mode outside {0, 1}, radius outside 0 ..
 * WOFT_PHOTO_WEIGHTS_MAX_RADIUS, or a map that shares a byte with cost, vis, bits or support. */
#define WOFT_PHOTO_WEIGHTS_MAX_RADIUS 4
int woft_photo_weights(const float* cost, const float* vis, int32_t rows, int32_t cols, int32_t ry, int32_t rx, int32_t h, int32_t w,
                       const uint32_t* bits, int32_t n_targets, float vis_thr, int32_t mode, int32_t radius, float* map,
                       int32_t* support, void* stream);

/* cv2.resize(img, None, fx, fy) with INTER_LINEAR geometry (tracker/YAOF_tracker_single_control.py:27-30,60-61,
 * `downscale_inputs`): src = (dst + 0.5) * scale - 0.5, edge clamped; scale = 1 / fx. */
int woft_resize_linear_u8(const uint8_t* img, int32_t h, int32_t w, int32_t c, uint8_t* out, int32_t ho, int32_t wo,
                          float scale_y, float scale_x, void* stream);

/* Correspondence masking + order-preserving compaction + Sobol subsampling on the device
 * (tracker/YAOF_tracker_single_control.py:287-327; configs/..._wLSq.py:31-53), outputs in woft_hfit's format.
 * The correspondences live on the flow grid gh x gw (the frame; with padding_mode 'crop' the frame cropped to a
 * multiple of 8, optical_flow/raft.py:235-247), the masks have the frame's size mh x mw (gh <= mh, gw <= mw).
 * dst: [2][gh*gw] (x plane, y plane) target coords of source pixel i = y*gw + x; w: [gh*gw] or NULL; tmask, pwmask:
 * uint8 [mh][mw]; check_dst != 0 adds the bounds test of dst against (mw, mh) and, if pwmask != NULL,
 * pwmask[rint(dy)][rint(dx)].
 * sobol_u: [n_draw] float32 1-D Sobol points (n_draw <= 1024; 0 = keep all).  ws: woft_tc_select_ws_bytes(gh*gw) bytes.
 * pa[k] = (dst_x, dst_y), pb[k] = (src_x, src_y), wout[k]; count[0] = selected (<= cap), count[1] = kept by the masks. */
int64_t woft_tc_select_ws_bytes(int64_t n);
int woft_tc_select(const float* dst, const float* w, const uint8_t* tmask, const uint8_t* pwmask, int32_t gh,
                   int32_t gw, int32_t mh, int32_t mw, int32_t check_dst, const float* sobol_u, int32_t n_draw,
                   void* ws, float* pa, float* pb, float* wout, int32_t cap, int32_t* count, void* stream);
/* The keep rule of woft_tc_select alone (`_mask_coords` / `_mask_coords_flow`, YAOF_tracker_single_control.py:287-327):
 * flags[i] = 1 where correspondence i survives, uint8 [gh*gw].  For callers that compact with their own code (the
 * tracker's generic path hands the compacted tensors to the config's subsampler / estimator callables). */
int woft_tc_flags(const float* dst, const uint8_t* tmask, const uint8_t* pwmask, int32_t gh, int32_t gw, int32_t mh,
                  int32_t mw, int32_t check_dst, uint8_t* flags, void* stream);
/* The same two with a per-source-pixel visibility probability vis: [gh*gw] float32 (this project's own rule, DESIGN.md
 * "Visibility mask in the tracker"; the reference's tracker consumes no mask).  vis_mode 1 (gate): correspondence i survives iff it
 * survives the keep rule above and vis[i] > vis_thr -- a strict fp32 compare, NaN is dropped; count[1], the Sobol draw and the
 * compaction see the gated set; weights untouched.  vis_mode 2 (weight): keep rule unchanged, wout[k] = w[i] * vis[i] (one fp32
 * multiply), vis[i] when w == NULL; woft_tc_flags_vis then equals woft_tc_flags.  vis == NULL or vis_mode 0: bit-identical to the
 * entry points above.  vis[i] is read only where tmask passes.  Same workspace, same output format. */
int woft_tc_select_vis(const float* dst, const float* w, const uint8_t* tmask, const uint8_t* pwmask, int32_t gh,
                       int32_t gw, int32_t mh, int32_t mw, int32_t check_dst, const float* sobol_u, int32_t n_draw,
                       const float* vis, int32_t vis_mode, float vis_thr, void* ws, float* pa, float* pb, float* wout,
                       int32_t cap, int32_t* count, void* stream);
int woft_tc_flags_vis(const float* dst, const uint8_t* tmask, const uint8_t* pwmask, int32_t gh, int32_t gw, int32_t mh,
                      int32_t mw, int32_t check_dst, const float* vis, int32_t vis_mode, float vis_thr, uint8_t* flags,
                      void* stream);
/* woft_tc_select_vis for n_targets template masks at once (csrc/select.hip).  DESIGN.md section 25.  tbits: the bit plane of
 * woft_chain_tc_multi, uint32 [mh][mw], 1 <= n_targets <= 32.  For every target t the keep rule of woft_tc_select_vis with
 * tmask = bit t and pwmask = NULL, then that call's order-preserving compaction and Sobol draw (float32 rint(N * u_k), sorted,
 * duplicates removed; keep-all when n_draw == 0 or n_draw >= N).  The bounds test and the visibility gate do not depend on the
 * target: dst and vis are read once per pixel.  Outputs: pa, pb [n_targets][cap][2], wout [n_targets][cap] (may be NULL),
 * count int32 [2][n_targets]: count[t] = selected (<= cap), count[n_targets + t] = kept -- two rows, so that the first is the
 * `counts` of woft_hfit_batched.  The first count[t] rows of target t's slices have the bytes the single-target call writes;
 * rows beyond are not specified.  vis, vis_mode, vis_thr and w == NULL as in woft_tc_select_vis.
 * ws: woft_tc_select_multi_ws_bytes(gh * gw, n_targets) bytes (-1 for n < 0 or n_targets outside [1, 32]): per target the
 * int32 header, per-1024 counts, offsets and rank list of the single call, then one uint32 of keep bits per pixel.
 * Three launches, no host round trip, no atomics: two calls give equal bytes.
 * WOFT_EINVAL before any launch on a NULL dst / tbits / ws / pa / pb / count, gh or gw <= 0, gh * gw above 2^31 - 1024 (ranks
 * are int32), mh < gh or mw < gw, cap <= 0,
 * n_targets outside [1, 32], n_draw outside [0, 1024] or positive with a NULL sobol_u, a vis_mode outside [0, 2], a NaN
 * vis_thr, an output (pa, pb, wout, count, ws) that shares a byte with an input or with another output. */
int64_t woft_tc_select_multi_ws_bytes(int64_t n, int32_t n_targets);
int woft_tc_select_multi(const float* dst, const float* w, const uint32_t* tbits, int32_t gh, int32_t gw, int32_t mh, int32_t mw,
                         int32_t n_targets, int32_t check_dst, const float* sobol_u, int32_t n_draw, const float* vis,
                         int32_t vis_mode, float vis_thr, void* ws, float* pa, float* pb, float* wout, int32_t cap,
                         int32_t* count, void* stream);

/* Weighted / iteratively re-weighted least-squares homography, utils/least_squares_H.py:142-210
 * (n_irls = 0) and :280-346 (n_irls = 5 -> 6 solves); reweight: 0 none, 1 L1 (:268-269),
 * 2 Huber(k) (:272-277).  pa, pb: [n][2] points (A -> B), w: [n] or NULL; n = min(count[0], n_max)
 * when count != NULL (device), else n_max.  Hout: 9 floats (row major, device).
 * status[0] (device) = 0 ok, 1 fewer than 4 points, 2 singular system.
 * ws: NULL, or woft_hfit_ws_bytes() bytes of device scratch: with it, fits of more than WOFT_HFIT_SINGLE_MAX
 * correspondences (configs without a subsampler: up to H*W) run as a streaming multi-workgroup pipeline instead of
 * in one workgroup; same arithmetic (fp32 rows, fp64 Gram matrix, fp64 Cholesky; only the summation order differs). */
#define WOFT_HFIT_SINGLE_MAX 2048
int64_t woft_hfit_ws_bytes(void);
int woft_hfit(const float* pa, const float* pb, const float* w, int32_t n_max, const int32_t* count,
              int32_t reweight, float huber_k, int32_t n_irls, void* ws, float* Hout, int32_t* status, void* stream);
/* `batch` independent fits of at most WOFT_HFIT_SINGLE_MAX correspondences each in ONE launch: workgroup b fits element b
 * with the one-workgroup code of woft_hfit (ws == NULL) -- same arithmetic, same summation order, same status codes, so
 * Hout[b] / status[b] are bit-identical to woft_hfit on element b alone.  pa, pb: [batch][n_max][2], w: [batch][n_max] or
 * NULL (all ones), counts: [batch] device int32 or NULL; element b uses n = min(counts[b], n_max) (n_max without counts) and
 * reads only the first n rows of its slice.  Hout: [batch][9], status: [batch].  reweight, huber_k and n_irls are shared by
 * the batch.  An element that fails (fewer than 4 points, singular or non-finite system) writes its own NaN Hout and status
 * and nothing else.  WOFT_EINVAL before any launch on a NULL pa / pb / Hout / status, batch < 1, batch >
 * WOFT_HFIT_BATCH_MAX (one workgroup per element in grid dimension x: larger batches are split by the caller), n_max < 1
 * and n_max > WOFT_HFIT_SINGLE_MAX (larger problems stay with woft_hfit's streaming path, one element at a time). */
#define WOFT_HFIT_BATCH_MAX 65535
int woft_hfit_batched(const float* pa, const float* pb, const float* w, int32_t batch, int32_t n_max,
                      const int32_t* counts, int32_t reweight, float huber_k, int32_t n_irls, float* Hout,
                      int32_t* status, void* stream);
/* Backward of the plain weighted fit (reweight = 0, n_irls = 0; utils/least_squares_H.py:142-210, which the reference's
 * training configs differentiate with torch autograd through torch.linalg.qr): given gH: [batch][9], the gradient of a
 * scalar with respect to the Hout of woft_hfit_batched / woft_hfit on the same pa, pb, w, counts, writes the gradients with
 * respect to the points, gpa, gpb: [batch][n_max][2], and the weights, gw: [batch][n_max].  ONE launch, workgroup b handles
 * element b alone; nothing is saved by the forward: the workgroup recomputes the Hartley statistics, the fp32 rows, the fp64
 * Gram matrix and its Cholesky factor exactly as the forward does and carries the adjoint in fp64 (one adjoint solve with
 * the same factor, then one pass over the correspondences).  No global scratch, no atomics, every sum
 * in a fixed order: deterministic, and element b gets the bits of a batch = 1 call on element b alone.  Any of gpa, gpb, gw
 * may be NULL: that gradient is neither computed nor stored and the others keep their bits; w == NULL means unit weights
 * and gw must then be NULL.  Rows at and beyond n = min(counts[b], n_max) are never read and their gradient slots are
 * written as exact zeros.  status (may be NULL): [batch], the forward's codes.  An element whose forward fails (status 1 or
 * 2) gets ZERO gradients in all of its slots -- not the NaN torch autograd would return: the forward's NaN Hout already
 * reports the failure, and one degenerate sample must not poison an optimiser step whose loss masks it out.  WOFT_EINVAL
 * before any launch on a NULL pa / pb / gH, all three outputs NULL, gw with a NULL w, batch < 1, batch >
 * WOFT_HFIT_BATCH_MAX, n_max < 1 and n_max > WOFT_HFIT_SINGLE_MAX (the streaming fit has no backward). */
int woft_hfit_batched_bwd(const float* pa, const float* pb, const float* w, int32_t batch, int32_t n_max,
                          const int32_t* counts, const float* gH, float* gpa, float* gpb, float* gw, int32_t* status,
                          void* stream);
/* ONE re-weighted solve of the same system, for arbitrary `reweighting_fn` callables (least_squares_H.py:280,323-337):
 * rew: [2n] per-row re-weights sqrt(reweighting_fn(residual)) of the previous step or NULL (= ones, first step);
 * first != 0 (re)computes the normalisation into ws; res (may be NULL): [2n] residuals A x - b of THIS step's solution
 * on the weighted, not re-weighted, system (:334) -- the host applies the user's callable to them and calls again;
 * Hout / status as woft_hfit (H of this step's solution, de-normalised). */
int woft_hfit_step(const float* pa, const float* pb, const float* w, int32_t n, const float* rew, int32_t first,
                   void* ws, float* res, float* Hout, int32_t* status, void* stream);
/* torch_proj_errors + inlier fraction (least_squares_H.py:474-489; configs/..._wLSq.py:14-21):
 * frac[0] = mean(|proj(H, A) - B| <= thr). */
int woft_inlier_frac(const float* pa, const float* pb, int32_t n_max, const int32_t* count, const float* H,
                     float thr, float* frac, void* stream);
/* `batch` inlier tests in ONE launch: workgroup b runs the code of woft_inlier_frac on element b -- pa, pb [batch][n_max][2],
 * counts [batch] device int32 or NULL (n = min(counts[b], n_max); n_max without counts), H [batch][9], frac [batch] -- so
 * frac[b] has the bits of woft_inlier_frac on element b alone (an integer count divided once).  No atomics.  WOFT_EINVAL before
 * any launch on a NULL pa / pb / H / frac, batch < 1, batch > WOFT_HFIT_BATCH_MAX, n_max < 0, a frac that shares a byte with
 * an input. */
int woft_inlier_frac_batched(const float* pa, const float* pb, int32_t batch, int32_t n_max, const int32_t* counts,
                             const float* H, float thr, float* frac, void* stream);

/* RANSAC homography, what cv2.findHomography(pa, pb, cv2.RANSAC, thr, max_iters, conf) does in
 * utils/least_squares_H.py:366-396 (find_homography_cvransac; configs/..._cvransac.py, ablation_09.py:26-30), restated in
 * csrc/ransac.hip and DESIGN.md ("RANSAC"): max_iters hypotheses from a SplitMix64 stream keyed by (seed, k, draw), cv2's sample
 * check, exact fp64 4-point models, cv2's fp32 error test err <= thr^2, cv2's sequential selection with the adaptive iteration
 * count of confidence conf; then, for n > 4 and refine != 0, woft_hfit's DLT over the inliers and 10 Levenberg-Marquardt
 * iterations.  pa, pb: [n][2] (A -> B); n = min(count[0], n_max) when count != NULL (device), else n_max.
 * ws: woft_ransac_ws_bytes(n_max, max_iters) bytes of device scratch.  Hout: 9 floats (device), h33 = 1.
 * status[0] (device) = 0 ok, 1 fewer than 4 points, 2 no model (no hypothesis with 4 or more inliers; Hout all NaN).
 * info (device, may be NULL): {inliers of the best hypothesis, its index k (-1 without a model), iterations run}.
 * inlier_mask (device, may be NULL): uint8 [n_max], 1 for the inliers of the best hypothesis, 0 elsewhere.
 * -1 (before any launch) on a NULL pointer, max_iters < 1, thr <= 0 or conf outside [0, 1]. */
int64_t woft_ransac_ws_bytes(int32_t n_max, int32_t max_iters);
int woft_ransac(const float* pa, const float* pb, int32_t n_max, const int32_t* count, int32_t max_iters, double thr,
                double conf, uint64_t seed, int32_t refine, void* ws, float* Hout, int32_t* status, int32_t* info,
                uint8_t* inlier_mask, void* stream);

/* RANSAC similarity (translation, rotation, scale; 4 degrees of freedom), what cv2.estimateAffinePartial2D(pa, pb,
 * method=cv2.RANSAC, ransacReprojThreshold=thr, maxIters=max_iters, confidence=conf) does in utils/least_squares_H.py:349-363
 * (find_homography_TRS), restated in csrc/trs.hip and DESIGN.md ("TRS"): max_iters two-point hypotheses from woft_ransac's
 * SplitMix64 stream, closed-form fp64 models, cv2's fp32 error test err <= thr^2, cv2's sequential selection with the adaptive
 * iteration count of confidence conf for two model points; then, for more than 2 inliers and refine != 0, the closed-form
 * least-squares similarity over the inliers.  Arguments, count, info and inlier_mask as woft_ransac.
 * ws: woft_trs_ws_bytes(n_max, max_iters) bytes of device scratch.  Hout: 9 floats (device), rows (a -b tx) (b a ty) (0 0 1).
 * status[0] (device) = 0 ok, 1 fewer than 2 points, 2 no model (no hypothesis with 2 or more inliers; Hout all NaN).
 * -1 (before any launch) on a NULL pointer, max_iters < 1, thr <= 0 or conf outside [0, 1]. */
int64_t woft_trs_ws_bytes(int32_t n_max, int32_t max_iters);
int woft_trs(const float* pa, const float* pb, int32_t n_max, const int32_t* count, int32_t max_iters, double thr,
             double conf, uint64_t seed, int32_t refine, void* ws, float* Hout, int32_t* status, int32_t* info,
             uint8_t* inlier_mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WOFT_HIP_H */
