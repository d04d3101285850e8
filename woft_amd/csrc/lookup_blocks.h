// The 8 x 8 source-pixel blocks of a lookup launch (woft_lookup_otf_params.roi_*): shared by the volume-free lookup and the
// band lookup, which must launch and skip the same blocks.
#pragma once
#include "common.h"

// 8 x 8 blocks of a launch: first block and block counts per axis
struct BlockRect {
    int by0, bx0, ny, nx;
};
__host__ __device__ __forceinline__ BlockRect block_rect(const woft_lookup_otf_params& p) {
    if ((p.roi_y0 | p.roi_x0 | p.roi_h | p.roi_w) == 0) return BlockRect{0, 0, (p.hf + 7) / 8, (p.wf + 7) / 8};
    const int by0 = p.roi_y0 / 8, bx0 = p.roi_x0 / 8;
    return BlockRect{by0, bx0, (p.roi_y0 + p.roi_h - 1) / 8 - by0 + 1, (p.roi_x0 + p.roi_w - 1) / 8 - bx0 + 1};
}

// rows of the band before level l, for a window radius R (include/woft_hip.h)
__host__ __device__ __forceinline__ int band_row_off(int R, int l) {
    int o = 0;
    for (int i = 0; i < l; ++i) o += WOFT_BAND_W(R, i);
    return o;
}
