// depth_shared.h — what the per-pixel kernels over (frames, H, W) maps share (depth.hip, normals.hip, consistency.hip): the four-pixel
// and one-pixel loads of a lane, the row of a rigid transform, the frame limits of their entries and the grid that puts the frame in
// blockIdx.y.
#pragma once
#include "common.h"

constexpr int MAX_PIXELS = 1 << 24;            // per frame: keeps every per-frame integer sum inside 64 bits and a pixel index inside an int

struct u32x3 { uint32_t x, y, z; };

template <int PX>
__device__ __forceinline__ void load_f32(const float* __restrict__ src, float (&v)[PX]) {
    if (PX == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
        for (int e = 0; e < PX; ++e) v[e] = t[e];
    } else {
        v[0] = src[0];
    }
}

template <int PX>
__device__ __forceinline__ void load_sky(const int64_t* __restrict__ labels, int64_t at, long long sky_label, bool (&sky)[PX]) {
#pragma unroll
    for (int e = 0; e < PX; ++e) sky[e] = false;
    if (!labels) return;
    if (PX == 4) {
        const u32x4 a = ld16(labels + at), b = ld16(labels + at + 2);
        const uint32_t lo = (uint32_t)sky_label, hi = (uint32_t)((unsigned long long)sky_label >> 32);
        sky[0] = a.x == lo && a.y == hi; sky[1] = a.z == lo && a.w == hi;
        sky[2] = b.x == lo && b.y == hi; sky[3] = b.z == lo && b.w == hi;
    } else {
        sky[0] = labels[at] == sky_label;
    }
}

// ((m0 x + m1 y) + m2 z) + m3, as §13's row
__device__ __forceinline__ double row4(const double* m, double x, double y, double z) {
    return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], x), __dmul_rn(m[1], y)), __dmul_rn(m[2], z)), m[3]);
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool shape_ok(int frames, int H, int W) { return frames > 0 && frames <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= MAX_PIXELS; }
inline dim3 frame_grid(int frames, int hw, int px) { return dim3((unsigned)((hw / px + 255) / 256), (unsigned)frames); }
