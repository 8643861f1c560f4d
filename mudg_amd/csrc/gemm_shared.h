// gemm_shared.h — what the contraction kernels of gemm.hip, pgemm.hip, wgemm.hip and sgemm.hip have in common: K-tile geometry, the GELU forms
// and the row steps of the epilogues (one site per rule), and the kernel plan (GemmPlan) that gemm.hip makes and the launchers take.
// The tile order is tile_order.h's, the LDS-DMA descriptor helpers are common.h's, the main-loop steps of the DMA-staged tiles tile_shared.h's.
#pragma once
#include "common.h"
#include <type_traits>

constexpr int BK = 64;
constexpr int LDSLD = 64;                       // h16 elements per LDS row: unpadded, XOR-swizzled (see gemm.hip)
constexpr int VF_Y = 1, VF_R = 2;               // 16-byte access allowed on Y / R
constexpr int VF_TM = 8;                        // temporal conv: a tile is 8 pixels x 16 frames (gemm.hip, TMAP / TSHARE)
constexpr int VF_XS = 4;                        // 3x3 conv: the three dx taps of a dy share one staged activation tile (gemm.hip, XSHARE)

typedef const __attribute__((address_space(1))) void* gptr_t;

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

// ---- epilogue steps: ONE site per rule, called by every epilogue of gemm.hip (wide-tile staged, 128 x 128 staged), pgemm.hip (direct) and
// wgemm.hip (w_epilogue).  A piece is a lane's W consecutive output channels of one row: W = 8, or 4 for the unpaired fragment of the
// 320-wide tiles of wgemm.hip.  Every helper decides the storage kind ONCE per piece, outside the per-value expressions: inside them the
// compiler kept a chain of scalar compares and branches per VALUE (round 6).

// The linear part of every epilogue: alpha scales the product alone — the bias (and the group bias summed into it) is added unscaled.
__device__ __forceinline__ float scale_bias(const float alpha, const float acc, const float bias) { return alpha * acc + bias; }

// GEGLU: v *= gelu(gate) — exact erf in the bf16x6 build, the Phi table when the launch brought one (phis: its copy in LDS), otherwise the
// polynomial.  Decided per piece, not per value: there the compiler kept a branch and a serialised LDS round trip per value.
template <int W>
__device__ __forceinline__ void geglu_gate(float (&v)[W], const float (&gate)[W], const bool phi, const float* __restrict__ phis) {
    if (PLANES > 2) {
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] *= gelu_erf_f(gate[j]);
    } else if (phi) {
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] *= gelu_lut(gate[j], phis);
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] *= gelu_fast(gate[j]);
    }
}

// What the store of v will hold, as fp32: GroupNorm partial sums are taken over what was stored.
template <int W>
__device__ __forceinline__ void stored_value(const float (&v)[W], const int kind, float (&t)[W]) {
    if (kind == KIND_F32) {
#pragma unroll
        for (int j = 0; j < W; ++j) t[j] = v[j];
    } else if (kind == KIND_F16) {
#pragma unroll
        for (int j = 0; j < W; ++j) t[j] = (float)f16_sat(v[j]);
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) t[j] = operand_round(v[j]);
    }
}
// One row's stored values into the running sum / sum of squares of its channels; the channels from nvalid on (none of a row outside the
// matrix: nvalid 0) add zeros.
template <int W>
__device__ __forceinline__ void stats_add(const float (&t)[W], const int nvalid, float (&gs)[W], float (&gq)[W]) {
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const float tt = (j < nvalid) ? t[j] : 0.f;
        gs[j] += tt; gq[j] = fmaf(tt, tt, gq[j]);
    }
}

// Eight consecutive values of a residual / seed of storage kind `kind` at element offset `off` of R, in 16-byte loads (ps: plane stride).
__device__ __forceinline__ void load_piece8(const void* R, const int kind, const int64_t off, const int64_t ps, float (&r)[8]) {
    if (kind == KIND_F32) {
        const float* rp = reinterpret_cast<const float*>(R) + off;
        const f32x4 a = *reinterpret_cast<const f32x4*>(rp), b = *reinterpret_cast<const f32x4*>(rp + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { r[j] = a[j]; r[4 + j] = b[j]; }
    } else if (kind == KIND_F16) {
        load8_f16(reinterpret_cast<const _Float16*>(R) + off, r);
    } else {
        load8_operand(reinterpret_cast<const h16*>(R) + off, ps, r);
    }
}
// v += the residual piece at element offset `off` of R: whole 16-byte loads when `wide`, else its first nvalid values one by one.
__device__ __forceinline__ void add_residual(float (&v)[8], const void* R, const int kind, const int64_t off, const int64_t ps, const int nvalid,
                                             const bool wide) {
    if (wide) {
        float r[8];
        load_piece8(R, kind, off, ps, r);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += r[j];
    } else if (kind == KIND_F32) {
#pragma unroll
        for (int j = 0; j < 8; ++j) if (j < nvalid) v[j] += reinterpret_cast<const float*>(R)[off + j];
    } else if (kind == KIND_F16) {
#pragma unroll
        for (int j = 0; j < 8; ++j) if (j < nvalid) v[j] += (float)reinterpret_cast<const _Float16*>(R)[off + j];
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) if (j < nvalid) v[j] += load1_operand(reinterpret_cast<const h16*>(R) + off + j, ps);
    }
}
// The same sum from a piece that is already in registers, RAW (the loads were issued earlier, to be in flight together): a — the piece's 16
// (W = 4: 8) bytes, b — the second half of an fp32 piece.  16-bit kinds: the fp16 stream or a ONE-plane operand matrix.
__device__ __forceinline__ void add_residual_raw(float (&v)[8], const u32x4 a, const u32x4 b, const int kind) {
    if (kind == KIND_F32) {
        union { u32x4 w; f32x4 f; } ta, tb; ta.w = a; tb.w = b;
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] += ta.f[j]; v[4 + j] += tb.f[j]; }
    } else if (kind == KIND_F16) {
        union { u32x4 w; f16x8 h; } t; t.w = a;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += (float)t.h[j];
    } else {
        const h16x8 t = as_h16x8(a);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += (float)t[j];
    }
}
__device__ __forceinline__ void add_residual_raw(float (&v)[4], const u32x2 a, const int kind) {
    if (kind == KIND_F16) {
        union { u32x2 w; _Float16 h[4]; } t; t.w = a;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += (float)t.h[j];
    } else {
        Pack8 t; t.u = a;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += (float)t.h[j];
    }
}

// The bits a wide store of a piece of 16-bit storage holds: the fp16 stream saturates (f16_sat), a one-plane operand matrix rounds to
// nearest even.  For the kernels that store through a buffer descriptor (sgemm.hip) instead of a pointer; store_piece's W = 4 pieces are these.
template <int W>
__device__ __forceinline__ auto f16_bits(const float (&v)[W]) {
    static_assert(W == 8 || W == 4, "a piece is 8 or 4 channels");
    union { std::conditional_t<W == 8, u32x4, u32x2> w; _Float16 h[W]; } t;
#pragma unroll
    for (int j = 0; j < W; ++j) t.h[j] = f16_sat(v[j]);
    return t.w;
}
#if MUDG_PLANES == 1
template <int W>
__device__ __forceinline__ auto operand_bits(const float (&v)[W]) {
    static_assert(W == 8 || W == 4, "a piece is 8 or 4 channels");
    union { std::conditional_t<W == 8, u32x4, u32x2> w; h16 h[W]; } t;
#pragma unroll
    for (int j = 0; j < W; ++j) t.h[j] = (h16)v[j];
    return t.w;
}
#endif

// Store a piece at element offset yoff of Y in storage kind `kind` (ps: plane stride of an operand matrix, ldy / PLANES): one 16-byte
// store per plane (fp32: two; W = 4: 8-byte stores, fp32 one 16-byte) when `wide`, else its first nvalid values one by one.
template <int W>
__device__ __forceinline__ void store_piece(void* Y, const int64_t yoff, const int kind, const int64_t ps, const float (&v)[W], const int nvalid,
                                            const bool wide) {
    static_assert(W == 8 || W == 4, "a piece is 8 or 4 channels");
    if (kind == KIND_F16) {
        _Float16* yp = reinterpret_cast<_Float16*>(Y) + yoff;
        if (wide) {
            if constexpr (W == 8) store8_f16(yp, v);
            else *reinterpret_cast<u32x2*>(yp) = f16_bits(v);
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) if (j < nvalid) yp[j] = f16_sat(v[j]);
        }
    } else if (kind == KIND_F32) {
        float* yp = reinterpret_cast<float*>(Y) + yoff;
        if (wide) {
#pragma unroll
            for (int h = 0; h < W / 4; ++h) {
                f32x4 a;
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = v[4 * h + j];
                *reinterpret_cast<f32x4*>(yp + 4 * h) = a;
            }
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) if (j < nvalid) yp[j] = v[j];
        }
    } else {
        h16* yp = reinterpret_cast<h16*>(Y) + yoff;
        if (wide) {
            if constexpr (W == 8) store8_operand(yp, ps, v);
            else {
                float r[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = v[j];
#pragma unroll
                for (int pl = 0; pl < PLANES; ++pl) {               // the pieces of store8_operand, four channels wide
                    Pack8 t;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { t.h[j] = (h16)r[j]; r[j] -= (float)t.h[j]; }
                    *reinterpret_cast<u32x2*>(yp + pl * ps) = t.u;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) if (j < nvalid) store1_operand(yp + j, ps, v[j]);
        }
    }
}

// Sub-pixel conv (MudgGemmDesc.subpixel): element offset in Y of logical row m of parity class (dy, dx) — pixel (oy, ox) of frame f of the
// low-resolution grid goes to pixel (2 oy + dy, 2 ox + dx) of the full-resolution image.
__device__ __forceinline__ int64_t subpixel_row_offset(const MudgGemmDesc& p, const int m, const int dy, const int dx) {
    const int hw = p.Hout * p.Wout;
    const int f = m / hw, r = m - f * hw;
    const int oy = r / p.Wout, ox = r - oy * p.Wout;
    return (((int64_t)(f * p.Hout + oy) * 2 + dy) * (2 * p.Wout) + 2 * ox + dx) * p.ldy;
}

// The staged epilogues' per-column constants of tile (m0, n0): sbias[0 .. BN) = bias (+ the group bias, when all rows of the tile belong to
// one group — always, for the UNet's shapes).  Returns whether the group bias is left to the store loop, row by row (a tile that straddles
// groups).  Such a tile adds bias + group bias there as ONE pre-summed constant like the staged one: a row's bits must not depend on which
// of the two paths its tile took — that changes with M, i.e. with how many clips share the launch.  The caller's barrier publishes sbias.
__device__ __forceinline__ bool stage_bias(float* sbias, const MudgGemmDesc& p, const int m0, const int n0, const int BM, const int BN, const int tid,
                                           const int NTH) {
    bool gbias_rows = p.gbias != nullptr;
    if (p.gbias && !p.geglu) {
        const int mlast = (m0 + BM <= p.M ? m0 + BM : p.M) - 1;
        const int g0 = m0 / p.rows_per_group;
        if (g0 == mlast / p.rows_per_group) {
            gbias_rows = false;
            for (int t = tid; t < BN; t += NTH) {
                float b = (p.bias && n0 + t < p.N) ? p.bias[n0 + t] : 0.f;
                if (n0 + t < p.N) b += p.gbias[(int64_t)g0 * p.N + n0 + t];
                sbias[t] = b;
            }
        }
    }
    if (gbias_rows || !p.gbias || p.geglu) {
        for (int t = tid; t < BN; t += NTH) sbias[t] = (!(gbias_rows && !p.geglu) && p.bias && n0 + t < p.N) ? p.bias[n0 + t] : 0.f;
    }
    return gbias_rows;
}
// The row-by-row form: v += (bias + group bias of row m's group), pre-summed (see stage_bias).
__device__ __forceinline__ void add_group_bias_row(float (&v)[8], const MudgGemmDesc& p, const int m, const int n, const int Nout, const int nvalid) {
    const float* gb = p.gbias + (int64_t)(m / p.rows_per_group) * Nout + n;
    const bool withb = p.bias && !p.geglu;
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j < nvalid) v[j] += withb ? p.bias[n + j] + gb[j] : gb[j];
}

#if MUDG_PLANES == 1
// The fused MX-fp8 copy of an operand-kind result (MudgGemmDesc.Y8): the values as the 16-bit store rounded them, and their largest
// magnitude; then — the block's amax gathered across its lanes at the call site, whose lane pattern is the kernel's — the block exponent
// and the piece's eight e4m3 bytes.
__device__ __forceinline__ float mx8_round(const float (&v)[8], float (&r8)[8]) {
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { r8[j] = (float)(h16)v[j]; amax = fmaxf(amax, fabsf(r8[j])); }
    return amax;
}
__device__ __forceinline__ float mx8_inv_scale(const int E) { return __uint_as_float((unsigned)(127 - E) << 23); }
__device__ __forceinline__ u32x2 mx8_pack8(const float (&r8)[8], const float inv) {
    u32x2 w8;
    w8[0] = mx_pack4_e4m3(r8[0], r8[1], r8[2], r8[3], inv);
    w8[1] = mx_pack4_e4m3(r8[4], r8[5], r8[6], r8[7], inv);
    return w8;
}
#endif


// Host side.  Tile heights of wgemm.hip: the 288-row tile (wgemm_kernel, wgemm_pkernel, wq_kernel<..., 9>) and the 160-row tile
// (wq_kernel<..., 5>); what the GroupNorm partial blocks of a problem are cut to where one of them runs it.
constexpr int WBM = 288, QBM = 160;
constexpr int SBM = 64;                                  // tile height of the stream kernel (sgemm.hip)
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
    GK_STREAM,           // sgemm_kernel (sgemm.hip; 16-bit builds)
};
struct GemmPlan {
    GemmKernel kernel;
    int vflags;          // VF_Y | VF_R | VF_TM | VF_XS
    int rows;            // height of the GroupNorm partial blocks: 288 | 160 | 128
    int ni;              // GK_WIDE: NI of the wide tile (5: 256 x 320, 4: 256 x 256)
    int wgs;             // GK_PERSIST: workgroups per CU (4 | 3: one K-tile stage, 2: two)
    int grid;            // GK_W288P, GK_STREAM: workgroups
    int rs;              // GK_W160: the residual — 0 none, 1 seeds the accumulators, 2 deferred to the epilogue
    bool pf;             // GK_H144: the prefetching K loop
    int delay;           // GK_H144: the measurement knobs of hgeglu_kernel (variant switches GEMM_H144DELAY / ABL / PRIO)
};
int mudg_pgemm_launch(const MudgGemmDesc& d, const GemmPlan& plan, hipStream_t s);       // GK_PERSIST
int mudg_wgemm_launch(const MudgGemmDesc& d, const GemmPlan& plan, hipStream_t s);       // GK_W288 ... GK_W160
int mudg_sgemm_launch(const MudgGemmDesc& d, const GemmPlan& plan, hipStream_t s);       // GK_STREAM
