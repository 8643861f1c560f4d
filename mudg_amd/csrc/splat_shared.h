// splat_shared.h — the raster rule of DESIGN.md §12 as device functions, shared by splat.hip and lidar_depth.hip: one copy of the
// projection, the culling and the pixel cover, so that every point drawn anywhere in the project lands on the same pixels.
#pragma once
#include "common.h"

constexpr uint64_t SPLAT_EMPTY = ~0ull;
constexpr int MAX_SPRITE = 8;                          // a sprite covers at most this many pixels a side (point size <= 8)

struct SplatCam { float fx, fy, cx, cy, znear, zfar, half; };      // half = point size / 2

// The pixel columns (rows) i with lo <= i + 0.5 < hi, clipped to [0, n): the comparison is the rule's own, in fp32; floorf only
// proposes a range one pixel too wide on either side.  lo < n and hi > 0 hold on entry.
__device__ __forceinline__ void cover(float lo, float hi, int n, int& a, int& b) {
    a = max((int)floorf(lo) - 1, 0);
    b = min((int)floorf(hi) + 1, n - 1);
    while (a <= b && !(__fadd_rn((float)a, 0.5f) >= lo)) ++a;
    while (b >= a && !(__fadd_rn((float)b, 0.5f) < hi)) --b;
}

// A point through the 3 x 4 matrix m and the camera: false when it is culled (depth range, off the image, not a number); else its
// camera depth, its image position and the pixels [i0, i1] x [j0, j1] its sprite covers (never empty ranges outside the image).
__device__ __forceinline__ bool splat_project(const float* __restrict__ m, float x, float y, float z, const SplatCam& cam, int H, int W,
                                              float& zc, float& u, float& v, int& i0, int& i1, int& j0, int& j1) {
    const float xc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z)), m[3]);
    const float yc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[4], x), __fmul_rn(m[5], y)), __fmul_rn(m[6], z)), m[7]);
    zc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[8], x), __fmul_rn(m[9], y)), __fmul_rn(m[10], z)), m[11]);
    if (!(zc > cam.znear && zc < cam.zfar)) return false;
    u = __fadd_rn(__fmul_rn(cam.fx, __fdiv_rn(xc, zc)), cam.cx);
    v = __fadd_rn(__fmul_rn(cam.fy, __fdiv_rn(yc, zc)), cam.cy);
    const float ulo = __fsub_rn(u, cam.half), uhi = __fadd_rn(u, cam.half);
    const float vlo = __fsub_rn(v, cam.half), vhi = __fadd_rn(v, cam.half);
    if (!(uhi > 0.0f && ulo < (float)W && vhi > 0.0f && vlo < (float)H)) return false;          // off the image (or not a number)
    cover(ulo, uhi, W, i0, i1);
    cover(vlo, vhi, H, j0, j1);
    i1 = min(i1, i0 + MAX_SPRITE - 1);
    j1 = min(j1, j0 + MAX_SPRITE - 1);
    return true;
}

inline bool splat_args_ok(int H, int W) { return H > 0 && W > 0 && (int64_t)H * W < (1LL << 31) && H < (1 << 23) && W < (1 << 23); }
