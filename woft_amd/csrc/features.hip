// Frame-features record: what the encoders produce for one image -- the fnet map, the GRU state `net`
// and the context `inp` -- packed into one contiguous fp32 block [P x fdim | P x hdim | P x cdim], and restored from it into
// a plan's buffers.  Pure streaming: one float4 per lane and step, 16-byte loads and stores, no atomics, no workspace.
#include "split_lines.h"

namespace {

// One map of the copy: rows of c4 float4s, read with row stride ld_src and written with row stride ld_dst (floats); dst2
// (optional) receives the same rows a second time, split (optional; rows contiguous) their [hi | lo] lines.
struct FeatSeg {
    const float* src;
    float* dst;
    float* dst2;
    __bf16* split;
    int64_t ld_src, ld_dst, ld_dst2;
    uint32_t c4, end4;          // float4s per row; end of this map in the launch's float4 numbering
};
struct FeatArgs {
    FeatSeg seg[3];
    int n_seg;
};

__global__ __launch_bounds__(256) void features_copy_kernel(const FeatArgs a) {
    const uint32_t total = a.seg[a.n_seg - 1].end4;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        int s = 0;
        uint32_t start = 0;
        if (a.n_seg > 1 && i >= a.seg[0].end4) { s = 1; start = a.seg[0].end4; }
        if (a.n_seg > 2 && i >= a.seg[1].end4) { s = 2; start = a.seg[1].end4; }
        const FeatSeg& g = a.seg[s];
        const uint32_t j = i - start;
        const uint32_t row = j / g.c4, q = j - row * g.c4;             // row < P, q < c4: inside the map by construction
        const f32x4 v = *(const f32x4*)(g.src + (int64_t)row * g.ld_src + q * 4);
        *(f32x4*)(g.dst + (int64_t)row * g.ld_dst + q * 4) = v;
        if (g.dst2) *(f32x4*)(g.dst2 + (int64_t)row * g.ld_dst2 + q * 4) = v;
        if (g.split) split_bf16_lines_store(g.split, (int64_t)j, v);
    }
}

bool bad_dim(int64_t P, int32_t c) { return c < 4 || c % 4 != 0 || c > 4096 || P < 1; }
bool bad_ld(int64_t ld, int32_t c) { return ld < c || ld % 4 != 0; }

FeatSeg seg(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int32_t c, int64_t P, uint32_t start4) {
    FeatSeg g;
    g.src = src; g.dst = dst; g.dst2 = nullptr; g.split = nullptr;
    g.ld_src = ld_src; g.ld_dst = ld_dst; g.ld_dst2 = 0;
    g.c4 = (uint32_t)(c / 4);
    g.end4 = start4 + (uint32_t)(P * (c / 4));
    return g;
}

int launch(const FeatArgs& a, void* stream) {
    const int64_t blocks = ceil_div64(a.seg[a.n_seg - 1].end4, 256);
    hipLaunchKernelGGL(features_copy_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, a);
    return woft_launch_status();
}

}  // namespace

extern "C" int woft_features_pack(const float* f1, int64_t ld_f1, const float* net, int64_t ld_net, const float* inp,
                                  int64_t ld_inp, int64_t P, int32_t fdim, int32_t hdim, int32_t cdim, float* record,
                                  void* stream) {
    if (!f1 || !net || !inp || !record || bad_dim(P, fdim) || bad_dim(P, hdim) || bad_dim(P, cdim)) return WOFT_EINVAL;
    if (bad_ld(ld_f1, fdim) || bad_ld(ld_net, hdim) || bad_ld(ld_inp, cdim)) return WOFT_EINVAL;
    if (P * ((int64_t)fdim + hdim + cdim) / 4 >= ((int64_t)1 << 31)) return WOFT_EINVAL;
    FeatArgs a = {};
    a.n_seg = 3;
    a.seg[0] = seg(f1, ld_f1, record, fdim, fdim, P, 0);
    a.seg[1] = seg(net, ld_net, record + P * fdim, hdim, hdim, P, a.seg[0].end4);
    a.seg[2] = seg(inp, ld_inp, record + P * ((int64_t)fdim + hdim), cdim, cdim, P, a.seg[1].end4);
    return launch(a, stream);
}

extern "C" int woft_features_unpack(const float* record, int64_t P, int32_t fdim, int32_t hdim, int32_t cdim, float* fmap,
                                    int64_t ld_fmap, void* fmap_split, float* net, int64_t ld_net, float* xbuf, int64_t ld_xbuf,
                                    float* inp_c, int64_t ld_inp_c, void* stream) {
    if (!record || !fmap || bad_dim(P, fdim) || bad_dim(P, hdim) || bad_dim(P, cdim) || bad_ld(ld_fmap, fdim)) return WOFT_EINVAL;
    if (P * ((int64_t)fdim + hdim + cdim) / 4 >= ((int64_t)1 << 31)) return WOFT_EINVAL;
    const bool source = net || xbuf || inp_c;
    if (source && (!net || !xbuf || !inp_c || bad_ld(ld_net, hdim) || bad_ld(ld_xbuf, cdim) || bad_ld(ld_inp_c, cdim)))
        return WOFT_EINVAL;
    // (the split lines number the float4s of contiguous rows, whole 32-channel lines; only the source role has them)
    if (fmap_split && (!source || ld_fmap != fdim || fdim % 32 != 0)) return WOFT_EINVAL;
    FeatArgs a = {};
    a.n_seg = source ? 3 : 1;
    a.seg[0] = seg(record, fdim, fmap, ld_fmap, fdim, P, 0);
    a.seg[0].split = (__bf16*)fmap_split;
    if (source) {
        a.seg[1] = seg(record + P * fdim, hdim, net, ld_net, hdim, P, a.seg[0].end4);
        a.seg[2] = seg(record + P * ((int64_t)fdim + hdim), cdim, xbuf, ld_xbuf, cdim, P, a.seg[1].end4);
        a.seg[2].dst2 = inp_c;
        a.seg[2].ld_dst2 = ld_inp_c;
    }
    return launch(a, stream);
}
