// rows_shared.h — the steps that several of the memory-bound row kernels must perform identically (norm.hip, the layout half of
// misc.hip, the norm / softmax / reduction kernels of train.hip), each written once: the three storage kinds of a rows matrix as
// one trait and the host's dispatch on the kind, the register pin of four rows' requests, the fixed-order fold of a 256-thread
// workgroup's four waves, the fp64 finish of a (mean, rstd) pair, and the numeric bodies of the GroupNorm / LayerNorm apply, of
// the row softmax and of the GroupNorm backward.  Everything on the device is forced inline; -ffp-contract=off is global, so the
// order of the floating-point operations below is the arithmetic.
#pragma once
#include "common.h"

namespace {     // as the kernels that use it: StreamH is part of their (mangled) names, which the traffic tool and the profiles key on

// ---- storage kinds (common.h: KIND_OPERAND / KIND_F32 / KIND_F16) ------------------------------------------------------------
struct StreamH { _Float16 v; };       // fp16 residual-stream storage (KIND_F16): a type of its own, h16 may be _Float16 too

// Eight consecutive channels of one row as fp32 (`get` / `put`), one channel (`load1` / `store1`), for operand (h16, PLANES pieces
// `ld / PLANES` apart), fp32 and fp16-stream storage; `ld` is the row stride in the caller's own integer type.  `raw` only issues
// the NR 16-byte requests and `decode` turns them into values, so a kernel can put several vectors' requests in flight before it
// touches any of them.  Stream stores saturate (f16_sat), operand stores round to PLANES pieces.
template <typename T> struct Kind;
template <> struct Kind<h16> {
    static constexpr int NR = PLANES;
    template <typename L> static __device__ __forceinline__ void get(const h16* p, L ld, float (&x)[8]) { load8_operand(p, ld / PLANES, x); }
    template <typename L> static __device__ __forceinline__ void put(h16* p, L ld, const float (&x)[8]) { store8_operand(p, ld / PLANES, x); }
    template <typename L> static __device__ __forceinline__ float load1(const h16* p, L ld) { return load1_operand(p, ld / PLANES); }
    template <typename L> static __device__ __forceinline__ void store1(h16* p, L ld, float v) { store1_operand(p, ld / PLANES, v); }
    template <typename L> static __device__ __forceinline__ void raw(const h16* p, L ld, u32x4 (&r)[NR]) {
#pragma unroll
        for (int k = 0; k < PLANES; ++k) r[k] = ld16(p + (int64_t)k * (ld / PLANES));
    }
    static __device__ __forceinline__ void decode(const u32x4 (&r)[NR], float (&x)[8]) {
#pragma unroll
        for (int k = 0; k < PLANES; ++k) {
            const h16x8 t = as_h16x8(r[k]);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = k ? x[e] + (float)t[e] : (float)t[e];
        }
    }
};
template <> struct Kind<StreamH> {
    static constexpr int NR = 1;
    template <typename L> static __device__ __forceinline__ void get(const StreamH* p, L, float (&x)[8]) { load8_f16(reinterpret_cast<const _Float16*>(p), x); }
    template <typename L> static __device__ __forceinline__ void put(StreamH* p, L, const float (&x)[8]) { store8_f16(reinterpret_cast<_Float16*>(p), x); }
    template <typename L> static __device__ __forceinline__ float load1(const StreamH* p, L) { return (float)p->v; }
    template <typename L> static __device__ __forceinline__ void store1(StreamH* p, L, float v) { p->v = f16_sat(v); }
    template <typename L> static __device__ __forceinline__ void raw(const StreamH* p, L, u32x4 (&r)[NR]) { r[0] = ld16(p); }
    static __device__ __forceinline__ void decode(const u32x4 (&r)[NR], float (&x)[8]) {
        union { u32x4 u; f16x8 h; } t; t.u = r[0];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = (float)t.h[e];
    }
};
template <> struct Kind<float> {
    static constexpr int NR = 2;
    template <typename L> static __device__ __forceinline__ void get(const float* p, L, float (&x)[8]) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { x[e] = a[e]; x[4 + e] = b[e]; }
    }
    template <typename L> static __device__ __forceinline__ void put(float* p, L, const float (&x)[8]) {
        f32x4 a, b;
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = x[e]; b[e] = x[4 + e]; }
        *reinterpret_cast<f32x4*>(p) = a;
        *reinterpret_cast<f32x4*>(p + 4) = b;
    }
    template <typename L> static __device__ __forceinline__ float load1(const float* p, L) { return *p; }
    template <typename L> static __device__ __forceinline__ void store1(float* p, L, float v) { *p = v; }
    template <typename L> static __device__ __forceinline__ void raw(const float* p, L, u32x4 (&r)[NR]) { r[0] = ld16(p); r[1] = ld16(p + 4); }
    static __device__ __forceinline__ void decode(const u32x4 (&r)[NR], float (&x)[8]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { x[e] = __uint_as_float(r[0][e]); x[4 + e] = __uint_as_float(r[1][e]); }
    }
};

// Row stride granule of a kind: with it every 8-channel vector (of every plane) of a 16-byte aligned matrix is 16-byte aligned.
inline int kind_granule(int kind) { return kind == KIND_F32 ? 4 : (kind == KIND_F16 ? 8 : 8 * PLANES); }

// Host: fn(KindTag<T>{}) with T the storage type of `kind` (2: fp16 stream, any other non-zero: fp32, 0: operand), so that a launch
// is written once:  with_kind(k, [&](auto tag) { using T = typename decltype(tag)::type; ... kernel<T> ... (const T*)X ... });
template <typename T> struct KindTag { using type = T; };
template <typename F>
inline void with_kind(int kind, F&& fn) {
    if (kind == KIND_F16) fn(KindTag<StreamH>{});
    else if (kind) fn(KindTag<float>{});
    else fn(KindTag<h16>{});
}

// ---- register pin ------------------------------------------------------------------------------------------------------------
// Every request of four rows (Kind<T>::raw) pinned in straight-line code before any value is decoded: without it the compiler sinks
// each load into the conditional block that consumes it, and the requests go out one at a time.  ONE statement per NR: a loop of
// one-operand statements changes the register allocation of the GroupNorm kernels.
__device__ __forceinline__ void pin_requests(u32x4 (&raw)[4][1]) { asm volatile("" : "+v"(raw[0][0]), "+v"(raw[1][0]), "+v"(raw[2][0]), "+v"(raw[3][0])); }
__device__ __forceinline__ void pin_requests(u32x4 (&raw)[4][2]) {
    asm volatile("" : "+v"(raw[0][0]), "+v"(raw[0][1]), "+v"(raw[1][0]), "+v"(raw[1][1]), "+v"(raw[2][0]), "+v"(raw[2][1]), "+v"(raw[3][0]), "+v"(raw[3][1]));
}
__device__ __forceinline__ void pin_requests(u32x4 (&raw)[4][3]) {
    asm volatile("" : "+v"(raw[0][0]), "+v"(raw[0][1]), "+v"(raw[0][2]), "+v"(raw[1][0]), "+v"(raw[1][1]), "+v"(raw[1][2]),
                      "+v"(raw[2][0]), "+v"(raw[2][1]), "+v"(raw[2][2]), "+v"(raw[3][0]), "+v"(raw[3][1]), "+v"(raw[3][2]));
}

// ---- fold of a 256-thread workgroup's four waves -----------------------------------------------------------------------------
// The association order is ((w0 + w1) + w2) + w3 for sums and max(max(w0, w1), max(w2, w3)) for maxima, everywhere: it is part of
// the run-to-run bit-reproducibility contract (no atomics, no order that depends on scheduling).  The scratch is the caller's LDS.
// Per-lane form: part[w][i] holds wave w's partial of item i; the caller stores, synchronises, then folds.
template <typename V, int N>
__device__ __forceinline__ V fold4(const V (&part)[4][N], int i) { return ((part[0][i] + part[1][i]) + part[2][i]) + part[3][i]; }
// Scalar form: `v` is the wave's value (after wave_sum / wave_max / wave_sum_d); ONE barrier inside, every thread gets the result.
// A caller that uses `red` again synchronises in between.
template <typename V>
__device__ __forceinline__ V block_sum4(V v, V (&red)[4]) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ float block_max4(float v, float (&red)[4]) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ---- statistics --------------------------------------------------------------------------------------------------------------
// stat = (mean, 1 / sqrt(var + eps)) from a = sum x and b = sum x^2 over `count` values, in fp64, a negative variance clamped to 0.
__device__ __forceinline__ void store_mean_rstd(double a, double b, double count, float eps, float* __restrict__ stat) {
    const double mean = a / count;
    double var = b / count - mean * mean;
    if (var < 0.0) var = 0.0;
    stat[0] = (float)mean;
    stat[1] = (float)(1.0 / sqrt(var + (double)eps));
}

// ---- numeric bodies ----------------------------------------------------------------------------------------------------------
// GroupNorm apply: y = x sc + sh (sc = rstd gamma, sh = beta - mean sc), optional SiLU.
__device__ __forceinline__ float gn_affine_act(float x, float sc, float sh, int silu) {
    float y = fmaf(x, sc, sh);
    if (silu) y = PLANES > 1 ? y / (1.0f + expf(-y))                             // split builds: IEEE division, full-precision exp
                             : y * __builtin_amdgcn_rcpf(1.0f + __expf(-y));     // 1-ulp reciprocal: the result is rounded to h16
    return y;
}
// gamma / beta of channels c .. c + 7 as two 16-byte requests each (16-byte aligned).
__device__ __forceinline__ void load_affine8(const float* __restrict__ gamma, const float* __restrict__ beta, int c, f32x4 (&g)[2], f32x4 (&b)[2]) {
    g[0] = *reinterpret_cast<const f32x4*>(gamma + c); g[1] = *reinterpret_cast<const f32x4*>(gamma + c + 4);
    b[0] = *reinterpret_cast<const f32x4*>(beta + c); b[1] = *reinterpret_cast<const f32x4*>(beta + c + 4);
}
// LayerNorm apply: (x - mean) rstd gamma + beta, of one channel and of eight.  ln_rows_kernel loops over ln_apply1 itself: handed
// its freshly decoded x by reference, the compiler no longer reuses the second pass's x - mean (32 more subtractions per lane).
__device__ __forceinline__ float ln_apply1(float x, float mean, float rstd, float g, float b) { return fmaf((x - mean) * rstd, g, b); }
__device__ __forceinline__ void ln_apply8(const float (&x)[8], float mean, float rstd, const f32x4 (&g)[2], const f32x4 (&b)[2], float (&o)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = ln_apply1(x[e], mean, rstd, g[0][e], b[0][e]); o[4 + e] = ln_apply1(x[4 + e], mean, rstd, g[1][e], b[1][e]); }
}

// Row softmax, one workgroup per row, three passes over the row (the second and third hit L2): maximum, sum of exponentials, store
// through put(c, p).  FAST: hardware exp (results rounded to 16 bits), else expf.
template <bool FAST, typename Put>
__device__ __forceinline__ void softmax_row_walk(const float* __restrict__ s, int cols, float (&red)[4], Put put) {
    const int tid = threadIdx.x;
    auto ex = [](float v) { return FAST ? __expf(v) : expf(v); };
    float mx = -INFINITY;
    for (int c = tid; c < cols; c += 256) mx = fmaxf(mx, s[c]);
    mx = block_max4(wave_max(mx), red);
    __syncthreads();
    float sum = 0.f;
    for (int c = tid; c < cols; c += 256) sum += ex(s[c] - mx);
    const float inv = 1.f / block_sum4(wave_sum(sum), red);
    for (int c = tid; c < cols; c += 256) put(c, ex(s[c] - mx) * inv);
}

// GroupNorm backward: xhat = (x - mean) rstd and dz = dy act'(xhat gamma + beta), act = SiLU or identity.
__device__ __forceinline__ float silu_grad(float z) {        // d/dz [z sigma(z)] = sigma (1 + z (1 - sigma))
    const float s = 1.0f / (1.0f + expf(-z));
    return s * (1.0f + z * (1.0f - s));
}
__device__ __forceinline__ float gn_bwd_dz(float x, float dy, float mean, float rstd, float ga, float be, int silu, float& xh) {
    xh = (x - mean) * rstd;
    return silu ? dy * silu_grad(fmaf(xh, ga, be)) : dy;
}

}  // namespace
