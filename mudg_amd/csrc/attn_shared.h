// attn_shared.h — the steps every forward flash-attention kernel of attention.hip is built from, each written once.
//
// Conventions (see the head of attention.hip): a wave owns 32 query rows per block; scores come out TRANSPOSED, so lane
// (l31 = lane & 31, hi = lane >> 5) holds, for ITS query row, 16 of the 32 keys of a sub-tile in each f32x16, in the key
// order {0-3, 8-11, 16-19, 24-27} + 4 hi.  A key tile is 64 keys = two sub-tiles: `f32x16 s[2]`.  Probabilities are
// written as PLANES pieces (one in the 16-bit builds): `h16x8 pk[PLANES][2][2]` = [piece][sub][16-key group].
// Everything here is forced inline and takes its aggregates by reference (the padded-tile flash step is a macro: see
// FLASH_TILE).  -ffp-contract=off is global, so the order of the floating-point operations below is the arithmetic.
#pragma once
#include "common.h"
#include <type_traits>

constexpr int QB = 128;     // query rows per workgroup
constexpr int KB = 64;      // keys per tile
constexpr int ALD = 72;     // LDS row stride in h16 (64 + 8 pad -> 144 B)
constexpr int ATILE = 64 * ALD;

// ---- one key / value set of a (frame, head): set 0 = p.K / p.Vt, set 1 = p.K2 / p.Vt2 (the image tokens) ----
struct KvSet {
    const h16* Kp;          // K rows of this (frame, head): [Nk][ldk]
    const h16* Vp;          // V^T rows (head-dim index): [64][ldvt]
    int Nk, ldk, ldvt;
    int psk, psv;           // distance between the pieces of one element (split builds; common.h)
};
__device__ __forceinline__ KvSet kv_set(const MudgAttnDesc& p, int f, int h, int set) {
    KvSet kv;
    if (set == 0) {
        kv.Kp = reinterpret_cast<const h16*>(p.K) + (int64_t)(f / p.kv_div) * p.Nk * p.ldk + h * 64;
        kv.Vp = reinterpret_cast<const h16*>(p.Vt) + (int64_t)(f / p.kv_div) * p.svt + (int64_t)(h * 64) * p.ldvt;
        kv.Nk = p.Nk; kv.ldk = p.ldk; kv.ldvt = p.ldvt;
    } else {
        kv.Kp = reinterpret_cast<const h16*>(p.K2) + (int64_t)(f / p.kv_div2) * p.Nk2 * p.ldk2 + h * 64;
        kv.Vp = reinterpret_cast<const h16*>(p.Vt2) + (int64_t)(f / p.kv_div2) * p.svt2 + (int64_t)(h * 64) * p.ldvt2;
        kv.Nk = p.Nk2; kv.ldk = p.ldk2; kv.ldvt = p.ldvt2;
    }
    kv.psk = kv.ldk / PLANES; kv.psv = kv.ldvt / PLANES;
    return kv;
}

// The four 16-byte Q fragments of query row `q` (zero for a row past Nq); `piece` = column offset of the operand piece.
__device__ __forceinline__ void load_q_frags(h16x8 (&qf)[4], const h16* Qp, int q, int ldq, int piece, bool qok, int hi) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        qf[ks] = as_h16x8(qok ? ld16(Qp + (int64_t)q * ldq + piece + ks * 16 + hi * 8) : zero16());
}

// ---- register staging of key tile kt: thread (lrow = tid >> 3, kc = tid & 7) fetches 16-byte chunk kc of rows lrow and
// lrow + 32 of the K tile (row = key) and of the V^T tile (row = head-dim index, chunk = 8 keys), every piece ----
__device__ __forceinline__ void load_kv_tile(const KvSet& kv, int kt, int lrow, int kc, u32x4 (&kr)[PLANES][2], u32x4 (&vr)[PLANES][2]) {
    const int j0 = kt * KB;
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = lrow + 32 * i;
            const int j = j0 + row;                       // key index for the K tile row
            kr[pl][i] = (j < kv.Nk) ? ld16(kv.Kp + (int64_t)j * kv.ldk + pl * kv.psk + kc * 8) : zero16();
            const int jc = j0 + kc * 8;                   // first key of this V^T chunk
            u32x4 v = zero16();
            if (jc < kv.Nk) {
                v = ld16(kv.Vp + (int64_t)row * kv.ldvt + pl * kv.psv + jc);
                if (jc + 8 > kv.Nk) {                    // ragged tail: keys >= Nk must contribute exactly 0
                    h16x8 hv = as_h16x8(v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) if (jc + e >= kv.Nk) hv[e] = (h16)0.f;
                    v = as_u32x4(hv);
                }
            }
            vr[pl][i] = v;
        }
}
// ... and their plain 16-byte row copies into the padded (ALD) tiles: Kt / Vt = PLANES consecutive tiles, one per piece
__device__ __forceinline__ void stage_padded(h16* Kt, h16* Vt, int lrow, int kc, const u32x4 (&kr)[PLANES][2], const u32x4 (&vr)[PLANES][2]) {
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            st16(&Kt[pl * ATILE + (lrow + 32 * i) * ALD + kc * 8], kr[pl][i]);
            st16(&Vt[pl * ATILE + (lrow + 32 * i) * ALD + kc * 8], vr[pl][i]);
        }
}

// Ragged last tile: the scores of keys >= Nk become -inf.
__device__ __forceinline__ void mask_ragged(f32x16 (&s)[2], int kt, int Nk, int hi) {
    if (kt * KB + KB > Nk) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = kt * KB + sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (j >= Nk) s[sub][r] = -INFINITY;
            }
    }
}

// Maximum of a query row's 64 scores of a tile: in-lane over the 32 the lane holds, one exchange with the other half.
__device__ __forceinline__ float row_max32(const f32x16 (&s)[2]) {
    float mx = s[0][0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[0][r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[1][r]);
    return fmaxf(mx, __shfl_xor(mx, 32, 64));
}

// Probability e of register r of sub-tile sub -> its PLANES pieces (one plain rounding in the 16-bit builds).
__device__ __forceinline__ void put_p(h16x8 (&pk)[PLANES][2][2], int sub, int r, float e) {
    h16 piece[PLANES];
    split_operand(e, piece);
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl) pk[pl][sub][r >> 3][r & 7] = piece[pl];
}

// ---- classic online softmax of one key tile (per query row = per lane; halves exchange once) ----
// c: the scores are exponentiated in base 2 (c = scale * log2 e, or 1 when Q is prescaled).
// The running maximum only moves during the first few tiles; when no row of this wave raised it, alpha is exactly 1 and
// the 32-register rescale of O (and its exp) is skipped — bit-identical, not a threshold trick.
// The softmax was the split kernel's bottleneck (rocprofv3: twice as many VALU issue cycles as MFMA cycles per key tile): the
// exponentials run on v_exp_f32 directly (1 ulp — fp32-class, as the split products around them) instead of the library
// exp2f with its range handling, and O is rescaled only when some row's maximum actually grew (wave-uniform test).
__device__ __forceinline__ void softmax_step_classic(const f32x16 (&s)[2], float c, float& m_run, float& l_run, f32x16 (&o)[2],
                                                     h16x8 (&pk)[PLANES][2][2]) {
    const float mx = row_max32(s);
    const bool grew = !__all(mx <= m_run);
    const float m_new = grew ? fmaxf(m_run, mx) : m_run;
    const float alpha = grew ? __builtin_amdgcn_exp2f((m_run - m_new) * c) : 1.0f;
    const float mc = m_new * c;
    m_run = m_new;
    float ps = 0.f;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = __builtin_amdgcn_exp2f(fmaf(s[sub][r], c, -mc));   // explicit: contraction is off globally
            ps += e;
            put_p(pk, sub, r, e);
        }
    l_run = l_run * alpha + ps;
    if (grew) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { o[0][r] *= alpha; o[1][r] *= alpha; }
    }
}

// ---- lean softmax (prescaled Q; see attn64d_kernel): the score accumulators started at -m_ref, so s is already the base-2
// exponent: {exp, add, cvt} per score, no maximum, no rescale.  Returns whether this lane's tile sum left the accepted range.
// LEAN_LIMIT: largest per-lane tile sum of 2^(s - m_ref) accepted before the workgroup falls back to the classic loop.
// P is stored as h16: a bf16 P has fp32's exponent range (2^40 leaves room for the row sum), an IEEE-half P overflows to
// inf beyond 65504 — there the limit is 2^15, so that no single exponential can reach the h16 maximum undetected.
#ifdef MUDG_OPERAND_FP16
constexpr float LEAN_LIMIT = 32768.f;
#else
constexpr float LEAN_LIMIT = 1099511627776.f;      // 2^40
#endif
__device__ __forceinline__ bool softmax_step_lean(const f32x16 (&s)[2], float& l_run, h16x8 (&pk)[PLANES][2][2]) {
    float ps = 0.f;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = __builtin_amdgcn_exp2f(s[sub][r]);
            ps += e;
            put_p(pk, sub, r, e);
        }
    l_run += ps;
    return !(ps <= LEAN_LIMIT);             // true for inf / nan as well
}
// The lean key loop with its fallback: key_loop(std::true_type) is the lean walk and raises `overflow` in any lane whose
// step said so; then the whole workgroup redoes its block with key_loop(std::false_type), the classic online softmax.
template <bool LEAN, class KeyLoop>
__device__ __forceinline__ void lean_or_classic(const bool& overflow, KeyLoop key_loop) {
    if constexpr (LEAN) {
        key_loop(std::true_type{});
        if (__syncthreads_or(overflow ? 1 : 0)) key_loop(std::false_type{});      // cold: exact, merely slower
    } else {
        key_loop(std::false_type{});
    }
}

// ---- one flash step on a key tile staged in the padded layout (Kt / Vt = PLANES consecutive tiles, one per piece):
// scores (S^T = K Q^T for the two 32-key sub-tiles: the kept (piece, piece) products, small terms first), ragged mask,
// classic softmax step, P V (O^T += V^T P^T; contraction slots follow the key order the score MFMA left in registers: the V^T
// fragment is two 8-byte reads stitched to one).  attn_kernel, xattn_kernel and attn_split_kernel all run exactly this.
// A macro, not a function: as a forced-inline function with these eleven parameters the same text made hipcc stop
// interleaving the two sub-tiles' score MFMAs and cost attn_kernel<0> / xattn_kernel<0> 18 VGPRs and 1 us in 66 on the
// level-0 cross-attention (profiles/r10/attention_refactor_isa.md); pasted into the kernel it allocates as the hand-written
// copies did.  qf: h16x8[PLANES][4]; m_run, l_run: float lvalues; o: f32x16[2]; the other arguments are evaluated once.
#define FLASH_TILE(Kt, Vt, qf, kt, Nk, c, m_run, l_run, o, l31, hi) do {                                                  \
    const h16* const ft_K = (Kt); const h16* const ft_V = (Vt); const int ft_kt = (kt), ft_Nk = (Nk);                     \
    f32x16 ft_s[2];                                                                                                       \
    _Pragma("unroll") for (int sub = 0; sub < 2; ++sub) {                                                                 \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) ft_s[sub][r] = 0.f;                                                \
        _Pragma("unroll") for (int sg = 0; sg < NSEG; ++sg) {                                                             \
            const h16* kp = ft_K + seg_xp(sg) * ATILE + (sub * 32 + (l31)) * ALD + (hi) * 8;                              \
            _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) {                                                            \
                const h16x8 kf = *reinterpret_cast<const h16x8*>(kp + ks * 16);                                           \
                ft_s[sub] = MFMA_32x32x16(kf, (qf)[seg_wp(sg)][ks], ft_s[sub]);                                           \
            }                                                                                                             \
        }                                                                                                                 \
    }                                                                                                                     \
    mask_ragged(ft_s, ft_kt, ft_Nk, (hi));                                                                                \
    h16x8 ft_pk[PLANES][2][2];                                                                                            \
    softmax_step_classic(ft_s, (c), (m_run), (l_run), (o), ft_pk);                                                        \
    _Pragma("unroll") for (int dt = 0; dt < 2; ++dt)                                                                      \
        _Pragma("unroll") for (int sg = 0; sg < NSEG; ++sg) {                                                             \
            const h16* vp = ft_V + seg_xp(sg) * ATILE + (dt * 32 + (l31)) * ALD + 4 * (hi);                               \
            _Pragma("unroll") for (int sub = 0; sub < 2; ++sub)                                                           \
                _Pragma("unroll") for (int jj = 0; jj < 2; ++jj) {                                                        \
                    const int kk = sub * 32 + jj * 16;                                                                    \
                    const h16x4 lo = *reinterpret_cast<const h16x4*>(vp + kk);                                            \
                    const h16x4 up = *reinterpret_cast<const h16x4*>(vp + kk + 8);                                        \
                    h16x8 vf;                                                                                             \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e) { vf[e] = lo[e]; vf[4 + e] = up[e]; }                   \
                    (o)[dt] = MFMA_32x32x16(vf, ft_pk[seg_wp(sg)][sub][jj], (o)[dt]);                                     \
                }                                                                                                         \
        }                                                                                                                 \
} while (0)

// ---- epilogues of the 16-bit builds ----
// log2-sum-exp of the scaled scores of query row q: P = 2^(c s - L) (mudg_attention_bwd)
__device__ __forceinline__ void store_lse(const MudgAttnDesc& p, int f, int h, int q, bool qok, int hi, float c, float m_run, float l_tot) {
    if (p.Lse && qok && hi == 0) p.Lse[((int64_t)f * p.Nq + q) * p.heads + h] = m_run * c + __log2f(l_tot);
}
// One query row's O * inv, 16-bit: the lane holds head-dim columns dt*32 + 8g + 4*hi + {0..3}; 8-byte stores.
__device__ __forceinline__ void store_o16(const f32x16 (&o)[2], float inv, h16* orow, int hi, int accumulate) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            h16* dst = orow + dt * 32 + 8 * g + 4 * hi;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = o[dt][4 * g + j] * inv;
            if (accumulate) {
                Pack8 old; old.u = *reinterpret_cast<const u32x2*>(dst);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] += (float)old.h[j];
            }
            Pack8 nw;
#pragma unroll
            for (int j = 0; j < 4; ++j) nw.h[j] = (h16)v[j];
            *reinterpret_cast<u32x2*>(dst) = nw.u;
        }
}
// A finished key / value set of attn_kernel / xattn_kernel: returns the factor the epilogue applies to o.  TWO: the first
// set's normalised result waits in res, the second is added to it in registers (factor 1) and the sum is stored once.
template <bool TWO>
__device__ __forceinline__ float finish_set(const MudgAttnDesc& p, int set, int f, int h, int q, bool qok, int hi, float c,
                                            float m_run, float l_run, f32x16 (&o)[2], f32x16 (&res)[TWO ? 2 : 1]) {
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    float inv = 1.f / l_tot;
    if (!TWO) store_lse(p, f, h, q, qok, hi, c, m_run, l_tot);
    if (TWO) {
        if (set == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { res[0][r] = o[0][r] * inv; res[1][r] = o[1][r] * inv; }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) { o[0][r] = fmaf(o[0][r], inv, res[0][r]); o[1][r] = fmaf(o[1][r], inv, res[1][r]); }
            inv = 1.f;
        }
    }
    return inv;
}
// A finished 32-query block of the single-set kernels (attn64q_kernel, attn64d_kernel): statistics and store.
__device__ __forceinline__ void finish_block16(const MudgAttnDesc& p, int f, int h, int q, bool qok, int hi, float c,
                                               float m_run, float l_run, const f32x16 (&o)[2], h16* Op) {
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.f / l_tot;
    store_lse(p, f, h, q, qok, hi, c, m_run, l_tot);
    if (qok) store_o16(o, inv, Op + (int64_t)q * p.ldo, hi, p.accumulate);
}

// ---- LDS-DMA staging (attn64d_kernel, attn_split_dma_kernel; the layout is described at attn64d_kernel; make_rsrc, lptr_t: common.h) ----
// The involution that swaps the two middle 4-blocks of every 16 rows: LDS row `row` of a K tile holds key swap_mid4(row).
__device__ __forceinline__ int swap_mid4(int row) {
    const int i16 = row & 15;
    return (row & ~15) | (i16 & 3) | ((i16 & 8) >> 1) | ((i16 & 4) << 1);
}
// DMA geometry: wave w stages rows [16w, 16w + 16) of a tile, two 1-KiB instructions; in instruction i lane l lands in
// row 16w + 8i + (l >> 3), slot l & 7, and fetches the swizzled chunk slot ^ ((row >> 1) & 7) of K row swap_mid4(row) /
// of V^T row `row`.  vk / vv: the byte offsets inside a tile.
__device__ __forceinline__ void dma_offsets(int wave, int lane, int ldk, int ldvt, unsigned (&vk)[2], unsigned (&vv)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = 16 * wave + 8 * i + (lane >> 3), slot = lane & 7;
        const int chunk = slot ^ ((row >> 1) & 7);
        vk[i] = (unsigned)swap_mid4(row) * (unsigned)ldk * 2u + (unsigned)chunk * 16u;
        vv[i] = (unsigned)row * (unsigned)ldvt * 2u + (unsigned)chunk * 16u;
    }
}
