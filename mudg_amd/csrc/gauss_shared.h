// gauss_shared.h — what the forward (gaussians.hip) and the backward (gaussians_bwd.hip, §24) of the Gaussian splat
// renderer both need: the constants of the rule, the single rounded operations, the polynomial exponential, the camera and the argument
// checks every entry point shares.  One copy, so that the backward recomputes the forward's values bit for bit.
#pragma once
#include "splat_shared.h"

#include <cmath>

constexpr int TILE = 16;                            // pixels a side; a workgroup of 256 lanes is one tile
constexpr int BATCH = 256;                          // entries staged through LDS at a time
constexpr float MAX_RADIUS = 4096.0f;               // a footprint beyond this is dropped (keeps the integer conversion safe)
constexpr float MIN_ALPHA = 1.0f / 255.0f;
constexpr float MAX_ALPHA = 0.99f;
constexpr float MIN_POWER = -5.55f;                 // e^-5.55 < 1 / 255
constexpr float MIN_T = 1e-4f;
constexpr float BLUR = 0.3f;                        // added to the diagonal of the 2-D covariance
constexpr float LOG2E = 1.44269504f;

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float dvd(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }     // not a number -> lo

// 2^(p log2 e) for -5.6 <= p <= 0: the integer part by ldexp (exact), the fraction by a degree-5 polynomial in Horner form.
__device__ __forceinline__ float gauss_exp(float p) {
    const float t = mul(p, LOG2E);
    const float n = floorf(t);
    const float f = sub(t, n);                      // exact
    float r = 0x1.f06faep-10f;
    r = add(mul(r, f), 0x1.25429cp-7f);
    r = add(mul(r, f), 0x1.c99b9ep-5f);
    r = add(mul(r, f), 0x1.ebcf7ap-3f);
    r = add(mul(r, f), 0x1.62e526p-1f);
    r = add(mul(r, f), 1.0f);
    return ldexpf(r, (int)n);
}

struct GaussCam { float fx, fy, cx, cy, znear, zfar; };

inline bool grid_ok(int64_t lanes) { return (lanes + 255) / 256 <= 0x7fffffffLL; }
inline bool entries_ok(int64_t E) { return E >= 1 && E <= 0x7fffffffLL; }

// the image and the tile grid shared by every entry point: V NT < 2^31
inline int check_views(const char* name, int64_t n, int V, int H, int W) {
    MUDG_REQUIRE(n > 0 && V > 0, "%s: %lld Gaussians in %d views", name, (long long)n, V);
    MUDG_REQUIRE(n <= 0x7fffffffLL, "%s: %lld Gaussians (the sorted value is a 32-bit index)", name, (long long)n);
    MUDG_REQUIRE(H > 0 && W > 0 && splat_args_ok(H, W), "%s: a %d x %d image", name, H, W);
    const int64_t NT = (int64_t)((W + TILE - 1) / TILE) * ((H + TILE - 1) / TILE);
    MUDG_REQUIRE((int64_t)V * NT < (1LL << 31), "%s: %d views of %lld tiles (V NT < 2^31)", name, V, (long long)NT);
    return MUDG_OK;
}
