// frames_shared.h — what every kernel of the resize rules shares: a table entry and the fp32 linear rule, written once.
// frames.hip (colour, semantic, depth) and normals.hip (the normal stream) include it.
#pragma once
#include "common.h"

// One output sample of an axis: the two source indices and their coefficients — int32 (8-bit rule, sum 2048) or fp32 bits (fp32 rule)
struct Tap { int s0, s1, c0, c1; };

__device__ __forceinline__ int inside(int s, int n) { return min(max(s, 0), n - 1); }     // a table cannot send a load out of the source

__device__ __forceinline__ float linear_f32(float s00, float s01, float s10, float s11, const Tap& tx, const Tap& ty) {
    const float w0 = __int_as_float(tx.c0), w1 = __int_as_float(tx.c1), v0 = __int_as_float(ty.c0), v1 = __int_as_float(ty.c1);
    const float r0 = __fadd_rn(__fmul_rn(s00, w0), __fmul_rn(s01, w1));
    const float r1 = __fadd_rn(__fmul_rn(s10, w0), __fmul_rn(s11, w1));
    return __fadd_rn(__fmul_rn(r0, v0), __fmul_rn(r1, v1));
}

// the size checks every entry of the resize rules makes: the grid is (row segments, output rows, frames)
#define FRAMES_REQUIRE_SIZES(name)                                                                                                      \
    MUDG_REQUIRE(T > 0 && T <= 65535 && H > 0 && H <= 65535 && W > 0 && H0 > 0 && W0 > 0,                                               \
                 name ": %d frames of %d x %d to %d x %d (every size positive, at most 65535 frames and output rows)", T, H0, W0, H, W); \
    MUDG_REQUIRE((int64_t)H0 * W0 <= (1 << 28) && (int64_t)H * W <= (1 << 28), name ": a frame of more than 2^28 pixels")
