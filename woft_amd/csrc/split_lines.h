// The [hi | lo] line format of the split-bf16 correlation operands (woft_split_bf16_lines), for every kernel that writes it.
#pragma once
#include "common.h"

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// Float4 number i of a row-major fp32 array -> its 4 hi and 4 lo values: 32 inputs make one 128-byte line [32 hi | 32 lo].
__device__ __forceinline__ void split_bf16_lines_store(__bf16* __restrict__ out, int64_t i, const f32x4 vv) {
    const bf16x4 h = __builtin_convertvector(vv, bf16x4);
    __bf16* line = out + (i >> 3) * 64 + (i & 7) * 4;
    *(bf16x4*)line = h;
    *(bf16x4*)(line + 32) = __builtin_convertvector(vv - __builtin_convertvector(h, f32x4), bf16x4);
}
