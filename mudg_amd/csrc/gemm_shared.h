// gemm_shared.h — what the contraction kernels of gemm.hip and pgemm.hip have in common: K-tile geometry, the buffer-descriptor
// helpers of the LDS-DMA loader, the GELU forms of the epilogues, and the kernel plan (GemmPlan) that gemm.hip makes and the launchers take.
#pragma once
#include "common.h"

constexpr int BK = 64;
constexpr int LDSLD = 64;                       // h16 elements per LDS row: unpadded, XOR-swizzled (see gemm.hip)
constexpr int VF_Y = 1, VF_R = 2;               // 16-byte access allowed on Y / R
constexpr int VF_TM = 8;                        // temporal conv: a tile is 8 pixels x 16 frames (gemm.hip, TMAP / TSHARE)
constexpr int VF_XS = 4;                        // 3x3 conv: the three dx taps of a dy share one staged activation tile (gemm.hip, XSHARE)

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// bf16x3 build, descriptor loader (FUSED): ONE K-tile stage holds both pieces of both operands (see gemm.hip).
constexpr bool fused_planes(bool fast) { return PLANES == 2 && fast; }

// Used by the 16-bit builds where the table is off and by the bf16x3 build (whose operands carry 16 significand bits: the
// polynomial's 1.5e-7 is two orders below their representation error); bf16x6 evaluates erff exactly.
__device__ __forceinline__ float gelu_fast(float x) {
    // 0.5 x (1 + erf(x / sqrt 2)) with Abramowitz-Stegun 7.1.26 for erf (|abs err| < 1.5e-7): the exact erff
    // costs about as much as the whole K loop of a K = 320 tile; the result is rounded to h16 anyway.
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __frcp_rn(fmaf(0.3275911f, z, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = 1.0f - p * t * __expf(-z * z);          // erf(|x| / sqrt 2)
    return 0.5f * x * (1.0f + copysignf(e, x));
}

// voffset of a lane whose source row / tap does not exist: at num_records, so the buffer load returns 0 into the LDS.
constexpr unsigned OOB = 0x80000000u;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const h16* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<h16*>(base), 0, (int)0x80000000u, 0x00020000);
}

// GEGLU's gate: gelu(x) = x Phi(x) with Phi linearly interpolated from a 1025-entry table over [-8, 8] held in LDS
// (|error| <= h^2/8 max|Phi''| = 7.4e-6 at h = 1/64 — below the h16 rounding of the result by two orders).
constexpr int PHI_N = 1024;
constexpr int PHI_BYTES = (PHI_N + 4) * 4;
__device__ __forceinline__ float gelu_lut(float x, const float* __restrict__ T) {
    float u = fmaf(x, 64.0f, 512.0f);
    u = __builtin_amdgcn_fmed3f(u, 0.0f, 1023.99f);
    const int i = (int)u;
    const float f = u - (float)i;
    const float a = T[i], b = T[i + 1];
    return x * fmaf(f, b - a, a);
}


// Host side.  Tile heights of wgemm.hip: the 288-row tile (wgemm_kernel, wgemm_pkernel, wq_kernel<..., 9>) and the 160-row tile
// (wq_kernel<..., 5>); what the GroupNorm partial blocks of a problem are cut to where one of them runs it.
constexpr int WBM = 288, QBM = 160;
const float* mudg_phi_table(bool split_ok = false);      // device Phi table, or nullptr (split-operand builds unless split_ok in bf16x3 / variant switch)

// What mudg_gemm runs for a problem and every parameter of that launch: chosen once, by gemm_plan (gemm.hip).
enum GemmKernel {
    GK_GENERIC,          // gemm_kernel<G128, MODE, false, false>: the generic address path
    GK_DOUBLE,           // gemm_kernel<G128, MODE, true, false>: descriptor loader, two K-tile stages
    GK_SINGLE,           // gemm_kernel<G128, MODE, true, true>: one stage, four workgroups per CU (bf16x3: the fused-piece kernel)
    GK_WIDE,             // gemm_kernel<G320 | G256, MODE, true, false> (16-bit builds)
    GK_PERSIST,          // pgemm_kernel (pgemm.hip)
    GK_W288,             // wgemm_kernel (wgemm.hip)
    GK_W288P,            // wgemm_pkernel (16-bit builds)
    GK_W288Q,            // wq_kernel<..., 9> (variant builds)
    GK_H144,             // hgeglu_kernel (16-bit builds)
    GK_W160,             // wq_kernel<..., 5> (16-bit builds)
};
struct GemmPlan {
    GemmKernel kernel;
    int vflags;          // VF_Y | VF_R | VF_TM | VF_XS
    int rows;            // height of the GroupNorm partial blocks: 288 | 160 | 128
    int ni;              // GK_WIDE: NI of the wide tile (5: 256 x 320, 4: 256 x 256)
    int wgs;             // GK_PERSIST: workgroups per CU (4 | 3: one K-tile stage, 2: two)
    int grid;            // GK_W288P: workgroups
    int rs;              // GK_W160: the residual — 0 none, 1 seeds the accumulators, 2 deferred to the epilogue
    bool pf;             // GK_H144: the prefetching K loop
    int delay;           // GK_H144: the measurement knobs of hgeglu_kernel (variant switches GEMM_H144DELAY / ABL / PRIO)
};
int mudg_pgemm_launch(const MudgGemmDesc& d, const GemmPlan& plan, hipStream_t s);       // GK_PERSIST
int mudg_wgemm_launch(const MudgGemmDesc& d, const GemmPlan& plan, hipStream_t s);       // GK_W288 ... GK_W160
