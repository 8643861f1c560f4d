// sgemm.hip — the stream GEMM: Y = alpha X W^T + bias (+ residual) for K = 320 and N = 320 (or 640: two slices) in the 16-bit builds, as a
// stream of rows.
// The projections with N = K = C of level 0 (to_out of every attention, proj_in, to_q of the cross-attentions) need 60 GFLOP per launch
// — about 25 us of MFMA time — and move 378 / 566 MB: they are bound by HBM, and the one-tile kernels drain the memory pipe between their
// phases.  Here W (200 KB of 16-bit values) is RESIDENT IN REGISTERS for the whole launch and nothing but rows moves.
//
// Workgroup: persistent, one per CU, four waves (one per SIMD, 512 registers each); it owns one contiguous range of 64-row tiles and never
// talks to another workgroup.  Wave w owns 80 output columns — the two fragment pairs at 64 w (a lane's 2 x 4 accumulator registers of a
// pair are 8 consecutive channels: W's rows are fetched with the row permutation of tile_shared.h) and the unpaired fragment at 256 + 16 w —
// as 5 column blocks x 10 k steps of v_mfma_f32_16x16x32 = 200 registers of W fragments, loaded once (behind the requests for the range's
// first two tiles, so that both are in flight together).  N = 640: two such slices of W, each with half the workgroups (work numbering below).
//
// X: an LDS ring of three 64 x 320 tiles (40 KiB each), filled by LDS-DMA with the source-side XOR swizzle of tile_shared.h (a 16 x 32
// subtile of 1 KiB = one DMA piece = one fragment, conflict-free ds_read_b128); wave w stages row block w of a tile (10 pieces).  Tile
// t + 2 is requested when tile t starts: 80 KiB of X are in flight while a tile is multiplied.
// Residual: it seeds the accumulators, as in w_seed (fp16 -> fp32 is exact; the sum is ((r + x w) + bias), the 288-row tile's).  It comes
// through LDS too, 40 KiB next to the ring: every lane requests, by LDS-DMA, exactly the 16-byte pieces it will read back itself (8 for
// the fragment pairs of its four rows; 2 for the unpaired fragments, whose 8 bytes per row are one half of a 16-byte piece fetched by the
// lane itself or by its neighbour 16 lanes away), one tile ahead.  Loads to REGISTERS are kept out of the row loop: beside LDS-DMA in
// flight the compiler waits vmcnt(0) for them, which would drain the pipe once per tile.
// Stores: straight from the accumulators through a buffer descriptor, 16 bytes per lane: the pairs as they stand; the unpaired
// fragments of two row blocks after one v_permlane16_swap of the rounded bits (lane q and its neighbour q ^ 1 exchange their halves: the
// even one ends up with 8 channels of the first row block, the odd one with 8 of the second).
//
// Waits.  gfx9's vmcnt counts loads, LDS-DMA and stores in issue order, and every wave issues the SAME operations per tile whatever M
// is: 10 residual pieces (R_DMA), 10 X pieces (X_DMA), 10 stores (STORES); rows and tiles that do not exist are aimed past the
// descriptor's num_records (OOB), never branched around.  Per tile t:
//     wait | barrier | accumulators <- residual(t) | request residual(t + 1), X(t + 2) | 200 MFMAs | 10 stores
// At the wait, tile t needs X(t) (requested two tiles ago) and residual(t) (requested first thing in tile t - 1); what the wave has issued
// since residual(t) is X(t + 1) and the stores of t - 1: s_waitcnt vmcnt(X_DMA + STORES) — the store acknowledgements of the previous
// tile and the next tile's rows stay in flight across the barrier.  (First tile: only X(t0 + 1) is younger.)  The barrier publishes the
// other waves' X pieces and tells that every wave is done with tile t - 1, whose slot X(t + 2) takes.
//
// Bits.  Per output element: the accumulator seeded with the residual, k steps of 32 in ascending K with the operands in wgemm_kernel's
// order, then alpha, bias, one rounding — the 288-row tile's sum exactly, so which of the two runs a problem changes no bit
// (tests/test_gemm_stream_gpu.py).  GroupNorm partials are not produced: problems with `stats` stay on the 288-row tile.
#include "tile_shared.h"

#if MUDG_PLANES == 1
namespace {

constexpr int S_C = 320;                         // K, and the columns of a slice of W
constexpr int S_KS = S_C / 32;                   // k steps
constexpr int S_NB = 5;                          // column blocks of a wave
constexpr int S_RB = SBM / 16;                   // row blocks of a tile = waves
constexpr int S_TILE = S_RB * S_KS * 1024;       // an X tile in LDS
constexpr int S_SLOTS = 3;
constexpr int S_RPIECES = 2 * S_RB + S_RB / 2;   // residual pieces of a lane per tile
constexpr int S_RWAVE = S_RPIECES * 1024;        // a wave's residual area
constexpr int S_SMEM_X = S_SLOTS * S_TILE, S_SMEM_R = 4 * S_RWAVE;
static_assert(S_RB == 4, "wave w stages row block w");
static_assert(S_SMEM_X + S_SMEM_R <= 160 * 1024, "LDS");
// operations of a wave per tile, and the two counted waits built from them (literals: they go into the instruction)
constexpr int X_DMA = S_KS, R_DMA = S_RPIECES, STORES = 2 * S_RB + S_RB / 2;
static_assert(X_DMA == 10 && STORES == 10 && R_DMA == 10, "S_WAIT_FIRST / S_WAIT_TILE below are X_DMA and X_DMA + STORES");
#define S_WAIT_FIRST() asm volatile("s_waitcnt vmcnt(10)" ::: "memory")
#define S_WAIT_TILE() asm volatile("s_waitcnt vmcnt(20)" ::: "memory")
#define S_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
// HASR: a residual; RF16 / YF16: it / the result is the fp16 stream (else operand storage) — constants, so that no piece branches on a kind
template <bool HASR, bool RF16, bool YF16>
__global__ __launch_bounds__(256, 1) void sgemm_kernel(const MudgGemmDesc p, const int ntiles, const int nslices) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Work numbering.  N = 320 nslices: a workgroup owns ONE 320-column slice of W and a row range; the slices of a range are neighbours
    // in an XCD's share of the grid (hardware deals block b to XCD b % 8), so that they run side by side on one L2 and X leaves HBM once.
    // Ranges [t0, t1) of tiles are contiguous, the first ntiles % ranges of them one tile longer.
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int slice = idx % nslices, wg = (idx / nslices) * 8 + xcd, nwg = (int)gridDim.x / nslices;
    const int per = ntiles / nwg, rem = ntiles % nwg;
    const int t0 = wg * per + (wg < rem ? wg : rem), t1 = t0 + per + (wg < rem ? 1 : 0);
    if (t0 == t1) return;

    const int px = lane & 15, q4 = lane >> 4;
    const int n0 = S_C * slice;
    const int cpair = n0 + 64 * wave + 8 * q4;            // first channel of the lane's piece of pair 0 (pair 1: + 32)
    const int csingle = n0 + 256 + 16 * wave;             // the wave's unpaired fragment

    // ---- X pieces: subtiles with the lane geometry of tile_shared.h
    const DmaLane dl(lane);
    const h16* X = reinterpret_cast<const h16*>(p.X);
    const unsigned vx = dl.x_off(p.ldx);
    const int xrow = 16 * wave + dl.srow();               // the tile row this lane stages
    const int xsoff = 16 * wave * p.ldx * 2;
    char* const xdst = smem + wave * S_KS * 1024;
    auto issue_x = [&](const int t, const int slot) {
        const int64_t m0 = (int64_t)t * SBM;
        const bool live = t < t1 && m0 + xrow < p.M;
        const __amdgpu_buffer_rsrc_t rX = make_rsrc(X + m0 * p.ldx);
        const unsigned v = live ? vx : OOB;
        char* d = xdst + slot * S_TILE;
#pragma unroll
        for (int s = 0; s < S_KS; ++s) __builtin_amdgcn_raw_ptr_buffer_load_lds(rX, (lptr_t)(d + s * 1024), 16, (int)v, xsoff + s * 64, 0, 0);
    };
    // ---- residual pieces (16-bit storage), wave-private: piece 2 i + P = the lane's 8 channels of pair P in row 16 i + px; piece 8 + u =
    // the 16 bytes around the unpaired fragment's channels 8 (q / 2) .. + 7 in row 16 (2 u + q % 2) + px.  The same geometry addresses the
    // stores of the unpaired fragments.
    const int hrow = px + 16 * (q4 & 1), hcol = csingle + 8 * (q4 >> 1);
    char* const rdst = smem + S_SMEM_X + wave * S_RWAVE;
    const h16* R = reinterpret_cast<const h16*>(p.R);
    const unsigned vrp = HASR ? (unsigned)(px * p.ldr + cpair) * 2u : 0u, vrs = HASR ? (unsigned)(hrow * p.ldr + hcol) * 2u : 0u;
    auto issue_r = [&](const int t) {
        const int64_t m0 = (int64_t)t * SBM;
        const int64_t lim = t < t1 ? p.M : 0;
        const __amdgpu_buffer_rsrc_t rR = make_rsrc(R + m0 * p.ldr);
#pragma unroll
        for (int i = 0; i < S_RB; ++i) {
            const bool live = m0 + 16 * i + px < lim;
#pragma unroll
            for (int P = 0; P < 2; ++P)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rR, (lptr_t)(rdst + (2 * i + P) * 1024), 16, (int)(live ? vrp + 64u * P : OOB), i * 16 * p.ldr * 2, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < S_RB / 2; ++u) {
            const bool live = m0 + 32 * u + hrow < lim;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rR, (lptr_t)(rdst + (2 * S_RB + u) * 1024), 16, (int)(live ? vrs : OOB), u * 32 * p.ldr * 2, 0, 0);
        }
    };
    // the accumulators' initial value from the wave's residual area: what w_seed makes of the same bytes
    auto seed = [&](f32x4 (&acc)[S_RB][S_NB]) {
        u32x4 ra[S_RB][2];
        u32x2 rs[S_RB];
#pragma unroll
        for (int i = 0; i < S_RB; ++i) {
#pragma unroll
            for (int P = 0; P < 2; ++P) ra[i][P] = *reinterpret_cast<const u32x4*>(rdst + (2 * i + P) * 1024 + lane * 16);
            // row block i = 2 u + b was fetched by the lane of this pixel and chunk whose q is odd exactly when b is
            const int src = px + 16 * ((q4 & 2) | (i & 1));
            rs[i] = *reinterpret_cast<const u32x2*>(rdst + (2 * S_RB + (i >> 1)) * 1024 + src * 16 + (q4 & 1) * 8);
        }
#pragma unroll
        for (int i = 0; i < S_RB; ++i) {
#pragma unroll
            for (int P = 0; P < 2; ++P) {
                if constexpr (RF16) {
                    union { u32x4 w; f16x8 h; } t; t.w = ra[i][P];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[i][2 * P + (e >> 2)][e & 3] = (float)t.h[e];
                } else {
                    const h16x8 t = as_h16x8(ra[i][P]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[i][2 * P + (e >> 2)][e & 3] = (float)t[e];
                }
            }
            if constexpr (RF16) {
                union { u32x2 w; _Float16 h[4]; } t; t.w = rs[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][4][e] = (float)t.h[e];
            } else {
                Pack8 t; t.u = rs[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][4][e] = (float)t.h[e];
            }
        }
    };

    const int fbyte = DmaLane::frag_byte(lane);
    const float alpha = p.alpha;
    h16* Y = reinterpret_cast<h16*>(p.Y);
    const unsigned vyp = (unsigned)(px * p.ldy + cpair) * 2u, vys = (unsigned)(hrow * p.ldy + hcol) * 2u;

    // the first tiles are requested before W, so that both are in flight together
    if (HASR) issue_r(t0);
    issue_x(t0, 0);
    issue_x(t0 + 1, 1);

    // ---- W, once: block j = 2 P + odd of a pair holds in its fragment row r = 4 q + e the channel 32 P + 8 q + 4 odd + e (the result
    // registers of lane (pixel, q) over the pair are then 8 consecutive channels); the unpaired block keeps its rows.  A fragment: row
    // lane % 16, 16-byte k chunk lane / 16.
    h16x8 wf[S_NB][S_KS];
    {
        const h16* W = reinterpret_cast<const h16*>(p.W);
#pragma unroll
        for (int j = 0; j < S_NB; ++j) {
            const int ch = j < 4 ? n0 + 64 * wave + 32 * (j >> 1) + 8 * (px >> 2) + 4 * (j & 1) + (px & 3) : csingle + px;
            const h16* wrow = W + (int64_t)ch * p.ldw + 8 * q4;
#pragma unroll
            for (int s = 0; s < S_KS; ++s) wf[j][s] = as_h16x8(ld16(wrow + 32 * s));
        }
    }
    float bp[2][8] = {}, bs[4] = {};
    if (p.bias) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { bp[0][e] = p.bias[cpair + e]; bp[1][e] = p.bias[cpair + 32 + e]; }
#pragma unroll
        for (int e = 0; e < 4; ++e) bs[e] = p.bias[csingle + 4 * q4 + e];
    }
    // every register load has landed before the row loop (and W stays what was loaded: nothing to re-derive it from)
#pragma unroll
    for (int j = 0; j < S_NB; ++j)
#pragma unroll
        for (int s = 0; s < S_KS; ++s) asm volatile("" : "+v"(wf[j][s]));

    int slot = 0;
    for (int t = t0; t < t1; ++t) {
        if (t == t0) S_WAIT_FIRST(); else S_WAIT_TILE();
        W_BARRIER();
        f32x4 acc[S_RB][S_NB];
        if constexpr (HASR) {
            seed(acc);
            S_LGKM0();                                   // the area is read before it is requested again
            issue_r(t + 1);
        } else {
#pragma unroll
            for (int i = 0; i < S_RB; ++i)
#pragma unroll
                for (int j = 0; j < S_NB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        issue_x(t + 2, slot == 0 ? 2 : slot - 1);        // (t + 2) % 3: the slot of tile t - 1

        const char* xs = smem + slot * S_TILE + fbyte;
#pragma unroll
        for (int i = 0; i < S_RB; ++i)
#pragma unroll
            for (int s = 0; s < S_KS; ++s) {
                const h16x8 xf = *reinterpret_cast<const h16x8*>(xs + (i * S_KS + s) * 1024);
#pragma unroll
                for (int j = 0; j < S_NB; ++j) acc[i][j] = mfma16(wf[j][s], xf, acc[i][j]);      // operands as in wgemm_kernel
            }

        // ---- epilogue: alpha acc + bias, one rounding, 16-byte stores
        const int64_t m0 = (int64_t)t * SBM;
        const __amdgpu_buffer_rsrc_t rY = make_rsrc(Y + m0 * p.ldy);
#pragma unroll
        for (int i = 0; i < S_RB; ++i) {
            const bool live = m0 + 16 * i + px < p.M;
#pragma unroll
            for (int P = 0; P < 2; ++P) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = scale_bias(alpha, acc[i][2 * P + (e >> 2)][e & 3], bp[P][e]);
                const u32x4 bits = YF16 ? f16_bits(v) : operand_bits(v);
                __builtin_amdgcn_raw_buffer_store_b128(bits, rY, (int)(live ? vyp + 64u * P : OOB), i * 16 * p.ldy * 2, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < S_RB / 2; ++u) {
            u32x2 h[2];                                   // the lane's 4 channels of row blocks 2 u and 2 u + 1, rounded
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = scale_bias(alpha, acc[2 * u + b][4][e], bs[e]);
                h[b] = YF16 ? f16_bits(v) : operand_bits(v);
            }
            // rows of 16 lanes: the odd ones of h[0] change places with the even ones of h[1].  An even q then holds channels 4 q .. 4 q + 7
            // of row block 2 u (its own, then its neighbour's), an odd q channels 4 q - 4 .. 4 q + 3 of row block 2 u + 1.
            u32x4 bits;
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const auto sw = __builtin_amdgcn_permlane16_swap(h[0][d], h[1][d], false, false);
                bits[d] = sw[0]; bits[2 + d] = sw[1];
            }
            const bool live = m0 + 32 * u + hrow < p.M;
            __builtin_amdgcn_raw_buffer_store_b128(bits, rY, (int)(live ? vys : OOB), u * 32 * p.ldy * 2, 0);
        }
        slot = slot == 2 ? 0 : slot + 1;
    }
}

template <bool HASR, bool RF16, bool YF16>
int sgemm_launch(const MudgGemmDesc& d, int grid, hipStream_t s) {
    constexpr int smem = S_SMEM_X + (HASR ? S_SMEM_R : 0);
    if (const int rc = mudg_lds_opt_in<&sgemm_kernel<HASR, RF16, YF16>>(smem, "gemm")) return rc;
    const int ntiles = (d.M + SBM - 1) / SBM;
    hipLaunchKernelGGL((sgemm_kernel<HASR, RF16, YF16>), dim3(grid), dim3(256), smem, s, d, ntiles, d.N / S_C);
    return mudg_check_launch("mudg_gemm");
}

}  // namespace

int mudg_sgemm_launch(const MudgGemmDesc& d, const GemmPlan& plan, hipStream_t s) {
    if (plan.grid <= 0 || d.N % S_C != 0 || plan.grid % (8 * (d.N / S_C)) != 0 || d.out_fp32 == KIND_F32 || (d.R && d.res_fp32 == KIND_F32)) MUDG_FAIL(MUDG_EINVAL, "gemm: not a problem of the stream kernel");
    const bool yf = d.out_fp32 == KIND_F16, rf = d.res_fp32 == KIND_F16;
    if (!d.R) return yf ? sgemm_launch<false, false, true>(d, plan.grid, s) : sgemm_launch<false, false, false>(d, plan.grid, s);
    if (rf) return yf ? sgemm_launch<true, true, true>(d, plan.grid, s) : sgemm_launch<true, true, false>(d, plan.grid, s);
    return yf ? sgemm_launch<true, false, true>(d, plan.grid, s) : sgemm_launch<true, false, false>(d, plan.grid, s);
}
#else
int mudg_sgemm_launch(const MudgGemmDesc&, const GemmPlan&, hipStream_t) { MUDG_FAIL(MUDG_EINVAL, "gemm: no stream kernel in this build"); }
#endif
