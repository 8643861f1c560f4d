// tile_shared.h — the main-loop steps of the DMA-staged GEMM tiles, each written once: wgemm.hip (wgemm_kernel, wgemm_pkernel,
// hgeglu_kernel, wq_kernel) and sgemm.hip (sgemm_kernel) call them.  This is geometry that must AGREE between kernels — the epilogue,
// the permuted W rows and the GroupNorm partial blocks all assume it — not arithmetic to vary per kernel.  What stays in each kernel,
// and why, is listed in DESIGN §3: every counted wait (its literals are properties of one kernel's issue order), its loop skeleton,
// the shape of its staging function.  A new tile is a new loop skeleton plus its waits on top of these.
//
// The subtile.  Operand tiles lie in LDS as 1 KiB SUBTILES of 16 rows x 32 k (one DMA piece = one 16x16x32 MFMA fragment), XOR-swizzled
// st_16x32: 16-byte chunk c of rows 8-15 sits in slot c ^ 2.  The swizzle is applied at the SOURCE of the DMA (DmaLane) and on the
// fragment read (DmaLane::frag_byte): conflict-free ds_read_b128.
#pragma once
#include "gemm_shared.h"
#include <type_traits>

namespace {

using T0 = std::integral_constant<int, 0>; using T1 = std::integral_constant<int, 1>; using T2 = std::integral_constant<int, 2>;

#define W_BARRIER()                            \
    do {                                       \
        __builtin_amdgcn_sched_barrier(0);     \
        __builtin_amdgcn_s_barrier();          \
        __builtin_amdgcn_sched_barrier(0);     \
    } while (0)

__device__ __forceinline__ f32x4 mfma16(h16x8 a, h16x8 b, f32x4 c) {
#ifdef MUDG_OPERAND_FP16
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
#else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
#endif
}

// DMA lane geometry of a subtile: lane l writes byte 16 l of it (lane-linear) and therefore fetches the element whose swizzled position
// that is — row srow, 16-byte chunk schunk.  The offsets are the lane's voffset for a source with leading dimension ld (elements).
struct DmaLane {
    int lane;             // every member is an expression of the lane number alone: written per use, it folds with what it is used in
    __device__ __forceinline__ explicit DmaLane(int l) : lane(l) {}
    __device__ __forceinline__ int sbyte() const { const int pos = lane * 16; return pos ^ (((pos >> 9) & 1) << 5); }
    __device__ __forceinline__ int srow() const { return sbyte() >> 6; }
    __device__ __forceinline__ int schunk() const { return (sbyte() >> 4) & 3; }
    __device__ __forceinline__ unsigned x_off(int ld) const { return (unsigned)(srow() * ld) * 2u + (unsigned)schunk() * 16u; }
    // W rows are fetched PERMUTED, so that the epilogue can leave the accumulators in 16-byte pieces: subtile j of a wave column
    // (j = 2 p + odd) holds in its row r = 4 q + e the channel 32 p + 8 q + 4 odd + e of the wave's 16 NREP columns — lane (pixel, q) of
    // the MFMA result then owns, over the fragment pair p, the 8 CONSECUTIVE channels 32 p + 8 q .. + 7.  The fifth fragment of the
    // 320-wide tile has no partner and keeps its rows (4 consecutive channels per lane).  Free: a row permutation of the source.
    __device__ __forceinline__ int w_row_pair() const { return 8 * (srow() >> 2) + (srow() & 3); }
    __device__ __forceinline__ unsigned w_off_pair(int ldw) const { return (unsigned)(w_row_pair() * ldw) * 2u + (unsigned)schunk() * 16u; }
    __device__ __forceinline__ unsigned w_off_single(int ldw) const { return x_off(ldw); }
    // the same three numbers in ONE register (the three-phase loop of wgemm_kernel): source row | permuted W row << 8 | chunk offset << 16
    __device__ __forceinline__ unsigned lanepk() const { return (unsigned)srow() | ((unsigned)w_row_pair() << 8) | ((unsigned)(schunk() * 16) << 16); }
    // fragment read: a 16 x 32 fragment is one subtile; lane l holds row l % 16, 16-byte k chunk l / 16
    static __device__ __forceinline__ int frag_byte(int lane) {
        const int fbyte0 = (lane & 15) * 64 + (lane >> 4) * 16;
        return fbyte0 ^ (((fbyte0 >> 9) & 1) << 5);
    }
};

// Which columns of a tile a wave column owns.  A wave's NREP fragments are NREP / 2 PAIRS (32 channels: a lane's 2 x 4 accumulator
// registers are 8 consecutive ones, a 16-byte piece of a 16-bit result row) and, on the 320-wide tile, one unpaired fragment (16
// channels, 8-byte pieces).  The pairs of all four wave columns come first, 32 channels each — so every 16-byte-per-lane store (four
// lanes = 64 contiguous bytes) starts on a 64-byte boundary of the row and the two pairs of a wave fill one 128-byte line; the four
// unpaired fragments follow at channel 256.  (A wave column as 80 CONSECUTIVE channels put the pieces of the odd wave columns across
// sector boundaries: the epilogue ran at half the store / residual-fetch rate.)  Free: which W rows a wave's fragments fetch.
template <int NREP> __device__ __forceinline__ int wave_pair_col(int wc, int pair) { return 32 * ((NREP / 2) * wc + pair); }
template <int NREP> __device__ __forceinline__ int wave_single_col(int wc) { return 32 * (NREP / 2) * 4 + 16 * wc; }
// First W row (channel) of W subtile `st` of the tile = fragment j of wave column wcol, st = NREP wcol + j; single: the unpaired fragment,
// whose lanes fetch with w_off_single (the paired ones with w_off_pair).
struct WPiece { int row0; bool single; };
template <int NREP> __device__ __forceinline__ WPiece w_frag_row0(int wcol, int j) {
    const bool single = j >= 2 * (NREP / 2);
    return {single ? wave_single_col<NREP>(wcol) : wave_pair_col<NREP>(wcol, j >> 1) + 4 * (j & 1), single};
}
template <int NREP> __device__ __forceinline__ WPiece w_piece_row0(int st) {
    const int wcol = st / NREP;
    return w_frag_row0<NREP>(wcol, st - wcol * NREP);
}

// Validity of source row m per tap (bit t): rows beyond M, taps that leave the image (MODE 1: 9 taps of a same-size 3x3 conv) or the
// clip (MODE 2: 3 temporal taps) are zero-filled by the DMA.  MODE 0: the one bit.
template <int MODE> __device__ __forceinline__ unsigned tap_mask(const MudgGemmDesc& p, int m) {
    if (m >= p.M) return 0;
    if (MODE == 0) return 1;
    unsigned mask = 0;
    if (MODE == 1) {
        const int hw = p.Hout * p.Wout;
        const int f = m / hw, r = m - f * hw;
        const int oy = r / p.Wout, ox = r - oy * p.Wout;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int iy = oy - 1 + t / 3, ix = ox - 1 + t % 3;
            if (iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win) mask |= 1u << t;
        }
    } else {
        const int fr = (m / p.HW) % p.T;
#pragma unroll
        for (int t = 0; t < 3; ++t) if (fr + t - 1 >= 0 && fr + t - 1 < p.T) mask |= 1u << t;
    }
    return mask;
}

struct KPos { int kt, tap, c; };                         // a K-tile: its index along W's K axis, its tap and first input channel
// The next K-tile, in tap-major (channels inside a tap) or slab-major (korder: taps inside a 64-channel slab) order.
template <int MODE> __device__ __forceinline__ void k_advance(const MudgGemmDesc& p, KPos& k) {
    constexpr int ntaps = MODE == 0 ? 1 : (MODE == 1 ? 9 : 3);
    k.kt += 1;
    if (MODE == 0) { k.c += BK; return; }
    const int t1 = k.tap + 1, c1 = k.c + BK;
    const bool slab = p.korder != 0;
    const bool wrap = slab ? (t1 == ntaps) : (c1 == p.Cin);
    k.tap = slab ? (wrap ? 0 : t1) : (wrap ? t1 : k.tap);
    k.c = slab ? (wrap ? c1 : k.c) : (wrap ? 0 : c1);
}

// Where the X pieces of k half ks (32 deep) of the K-tile at channel c, tap `tap` come from: the second source (channels from csplit on),
// its leading dimension, and the scalar byte offset inside a row-based descriptor (which starts at the reach of tap 0); plane: the bf16
// piece of a bf16x3 row, ld / 2 elements further.  MODE 0: the tap terms fold away.
struct XSource { bool s2; int ld, soff; };
template <int MODE> __device__ __forceinline__ XSource x_source(const MudgGemmDesc& p, int ldx2e, int c, int tap, int ks, int plane = 0) {
    const bool s2 = c >= p.csplit;
    const int cc = s2 ? c - p.csplit : c;
    const int ld = s2 ? ldx2e : p.ldx;
    int soff = (cc + ks * 32) * 2 + plane * ld;
    if (MODE == 1) { const int dy = tap / 3, dx = tap - 3 * dy; soff += (dy * p.Win + dx) * ld * 2; }
    if (MODE == 2) soff += tap * p.HW * ld * 2;
    return {s2, ld, soff};
}

// GEGLU's Phi table (gemm_shared.h) -> LDS as PAIRS: (Phi_i, Phi_{i+1} - Phi_i) for gelu_lut2, in the bf16x3 build (Phi_i, slope x node
// distance) for gelu_hermite.  Entry PHI_N exists (x = 8); its step is never used (u < 1024).  Visible after the K loop's barriers.
template <int THREADS> __device__ __forceinline__ void phi_pairs_to_lds(float* tail, const float* __restrict__ phi, int tid) {
    for (int t = tid; t <= PHI_N; t += THREADS) {
        const float a = phi[t], b = phi[t < PHI_N ? t + 1 : t];
        if constexpr (PLANES == 2) {
            const float xt = -8.0f + (float)t * (1.0f / 64.0f);
            *reinterpret_cast<f32x2*>(&tail[2 * t]) = f32x2{a, expf(-0.5f * xt * xt) * (0.3989422804014327f / 64.0f)};
        } else *reinterpret_cast<f32x2*>(&tail[2 * t]) = f32x2{a, b - a};
    }
}

// ---- the six-phase K-tile of the 288-row tile (16-bit builds): wgemm_kernel and wgemm_pkernel; the phase table is in wgemm.hip's header ----
// Fragments of one phase: the W fragments of a k half, the X fragments of a row third.
template <int NREP> struct Frag288 {
    h16x8 af[3], bf[NREP];
    // a_half / b_half: the wave's first X / W fragment in the k half to read (fragment byte included)
    __device__ __forceinline__ void read_a(const char* a_half, int third) {
#pragma unroll
        for (int i = 0; i < 3; ++i) af[i] = *reinterpret_cast<const h16x8*>(a_half + (third * 3 + i) * 1024);
    }
    __device__ __forceinline__ void read_b(const char* b_half) {
#pragma unroll
        for (int j = 0; j < NREP; ++j) bf[j] = *reinterpret_cast<const h16x8*>(b_half + j * 1024);
    }
    template <int third> __device__ __forceinline__ void mma(f32x4 (&acc)[9][NREP]) const {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);              // (register-only MFMAs may otherwise be hoisted above the wait)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < NREP; ++j)              // operands swapped: a lane ends up with 4 consecutive (permuted) channels of one pixel
                acc[third * 3 + i][j] = mfma16(bf[j], af[i], acc[third * 3 + i][j]);
    }
};
// K-tile t in ring buffer buf, whose two k halves lie KS bytes apart at a_tile / b_tile: phases p = 0..5 = (ks = p / 3, row third = p % 3), a
// phase = LOAD section | barrier | 15 MFMAs | barrier.  The kernel's own stage(where, ks, buf, part) issues this wave's pieces (part 2: W,
// part 1: X) of ks 1 of K-tile t + 1 = k1 in phases 1 and 2 and of ks 0 of K-tile t + 2 = k2 in phases 4 and 5 (n1 / n2: they exist);
// the kernel's own counted wait(more) stands at the end of phases 1 and 4 — ks 1 of tile t / ks 0 of tile t + 1 has landed, a whole phase
// before its first read.  stage and wait are the kernel's lambdas THEMSELVES, called here as the kernel would call them: wrapped in
// per-call closures (stage1(part), wait1()) the same code came out with another block layout and, in wgemm_pkernel<5, false>, two more
// registers (profiles/tile_shared/isa.txt).
template <int KS, int NREP, class Stage, class Where, class Wait>
__device__ __forceinline__ void ktile_six(Frag288<NREP>& f, f32x4 (&acc)[9][NREP], const char* a_tile, const char* b_tile, const int buf, const bool n1, const bool n2,
                                          Stage& stage, const Where& k1, const Where& k2, Wait& wait) {
    // phase 0
    f.read_b(b_tile);
    f.read_a(a_tile, 0);
    W_BARRIER();
    f.template mma<0>(acc);
    W_BARRIER();
    // phase 1
    f.read_a(a_tile, 1);
    if (n1) stage(k1, 1, buf ^ 1, 2);
    W_BARRIER();
    f.template mma<1>(acc);
    wait(n1);
    W_BARRIER();
    // phase 2
    f.read_a(a_tile, 2);
    if (n1) stage(k1, 1, buf ^ 1, 1);
    W_BARRIER();
    f.template mma<2>(acc);
    W_BARRIER();
    // phase 3
    f.read_b(b_tile + KS);
    f.read_a(a_tile + KS, 0);
    W_BARRIER();
    f.template mma<0>(acc);
    W_BARRIER();
    // phase 4
    f.read_a(a_tile + KS, 1);
    if (n2) stage(k2, 0, buf, 2);
    W_BARRIER();
    f.template mma<1>(acc);
    wait(n2);
    W_BARRIER();
    // phase 5
    f.read_a(a_tile + KS, 2);
    if (n2) stage(k2, 0, buf, 1);
    W_BARRIER();
    f.template mma<2>(acc);
    W_BARRIER();
}

}  // namespace
