// towers.hip — what the CLIP image tower needs besides mudg_gemm and mudg_layernorm (reference
// lvdm/modules/encoders/condition.py:295-372, a pre-LN ViT-H/14 of 257 tokens, 16 heads of width 80):
//   short_attention   self-attention over at most 288 tokens from the fp32 output of the fused in_proj GEMM, head width 64 or 80
//   layernorm_f32     LayerNorm with an fp32 result (ln_pre writes the residual stream)
//   clip_preprocess   blur, bicubic resize to 224 x 224, CLIP normalisation, written as the patch matrix of the 14 x 14 convolution
//
// short_attention: one workgroup of four waves per (image, head, 32 query rows).  LDS holds the query tile, ALL keys of the (image,
// head), the 32 x N scores and probabilities, and — in the region the keys leave after the score pass — ALL values: the softmax is one
// pass with the exact row maximum, nothing is rescaled.  Phases, a barrier between each:
//   1  q, k staged: fp32 from QKV, rounded once to operand storage
//   2  scores S^T = K Q^T, times c = scale log2(e), key columns >= N set to -inf                  -> S fp32 [32][NP + 4]
//   3  v staged over the keys (transposed in the 16-bit builds); softmax rows: m = max, p = 2^(s - m), l = sum p (fp32, wave
//      butterfly: a fixed order), P through operand storage                                       -> P, L
//   4  O^T = V^T P^T                                                                              -> Of fp32 [32][d]
//   5  O = Of / l, rounded once through store8_operand
// 16-bit builds: v_mfma_f32_32x32x16 with K rows / V^T rows as the A operand and Q / P as B, so that a lane owns one query (its
// column) in both products.  d = 80 is five K = 16 steps of the score product, no padding; in P V the head dim is the M axis, three
// 32-row blocks with rows 80 .. 95 zero (waves 0 .. 2 take one block each, wave 3 is idle there).  LDS rows are padded by 16 bytes
// (stride 176 B for d = 80): a 16-byte fragment read of 32 consecutive rows then spreads over all 64 banks in four-lane groups.
// Split builds: plain fp32 FMAs on the vector unit from the operand-rounded values (24 significand bits hold a bf16x2 value exactly,
// a bf16x3 value to fp32): the tower's attention is 3 % of its arithmetic and the piece products would need PLANES LDS images.
#include "common.h"

namespace {

constexpr int SA_QT = 32;            // query rows per workgroup
constexpr int SA_THREADS = 256;
constexpr int SA_NMAX = 288;

// LDS plan of one workgroup, in bytes, for NP = N rounded up to 32 keys.  Every offset is a multiple of 16.
template <int D>
struct SaPlan {
    static constexpr int DP = PLANES == 1 ? D + 8 : D + 1;          // row stride of the Q and K images (h16 | float)
    static constexpr int DV = (D + 31) / 32 * 32;                   // V^T rows of the 16-bit builds: the M axis of P V
    static constexpr int ES = PLANES == 1 ? 2 : 4;                  // bytes per staged element
    int np, ss, ps, vs;                                             // keys, S row stride (floats), P row stride, V^T row stride (h16)
    int q_off, kv_off, s_off, p_off, o_off, l_off, total;
    __host__ __device__ explicit SaPlan(int N) {
        np = (N + 31) / 32 * 32;
        ss = np + 4; ps = np + 8; vs = np + 8;
        const int kbytes = np * DP * ES;
        const int vbytes = PLANES == 1 ? DV * vs * 2 : np * D * 4;
        const int kv = (kbytes > vbytes ? kbytes : vbytes);
        q_off = 0;
        kv_off = (SA_QT * DP * ES + 15) / 16 * 16;
        s_off = kv_off + (kv + 15) / 16 * 16;
        p_off = s_off + SA_QT * ss * 4;
        o_off = p_off + (PLANES == 1 ? SA_QT * ps * 2 : 0);
        l_off = o_off + SA_QT * D * 4;
        total = l_off + SA_QT * 4;
    }
};

struct SaArgs {
    const float* QKV;
    h16* O;
    int N, heads;
    int64_t ldqkv, ldo;
    float c;                      // scale * log2(e)
};

template <int D>
__global__ __launch_bounds__(SA_THREADS) void short_attn_kernel(const SaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sa_lds[];
    typedef SaPlan<D> Plan;
    const Plan pl(a.N);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * SA_QT, h = blockIdx.y;
    const int64_t b = blockIdx.z;
    const int N = a.N, NP = pl.np, C = a.heads * D;
    const float* base = a.QKV + b * N * a.ldqkv + h * D;            // q of row n: base + n ldqkv; k: + C; v: + 2 C
    float* S = reinterpret_cast<float*>(sa_lds + pl.s_off);
    float* Of = reinterpret_cast<float*>(sa_lds + pl.o_off);
    float* L = reinterpret_cast<float*>(sa_lds + pl.l_off);
    constexpr int DP = Plan::DP;

#if MUDG_PLANES == 1
    h16* Qs = reinterpret_cast<h16*>(sa_lds + pl.q_off);
    h16* Ks = reinterpret_cast<h16*>(sa_lds + pl.kv_off);
    h16* Vt = reinterpret_cast<h16*>(sa_lds + pl.kv_off);          // after the score pass
    h16* P = reinterpret_cast<h16*>(sa_lds + pl.p_off);
    const int l31 = lane & 31, hi = lane >> 5;
    // ---- 1: q and k, rounded once
    for (int i = tid; i < SA_QT * D; i += SA_THREADS) {
        const int r = i / D, col = i - r * D, n = q0 + r;
        Qs[r * DP + col] = (h16)(n < N ? base[(int64_t)n * a.ldqkv + col] : 0.f);
    }
    for (int i = tid; i < NP * D; i += SA_THREADS) {
        const int j = i / D, col = i - j * D;
        Ks[j * DP + col] = (h16)(j < N ? base[(int64_t)j * a.ldqkv + C + col] : 0.f);
    }
    __syncthreads();
    // ---- 2: scores; the lane's query is l31, its keys of block kb are kb 32 + 8 g + 4 hi + {0 .. 3}
    {
        h16x8 qf[D / 16];
#pragma unroll
        for (int ks = 0; ks < D / 16; ++ks) qf[ks] = *reinterpret_cast<const h16x8*>(Qs + l31 * DP + ks * 16 + hi * 8);
        for (int kb = wave; kb < NP / 32; kb += 4) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const h16* kp = Ks + (kb * 32 + l31) * DP + hi * 8;
#pragma unroll
            for (int ks = 0; ks < D / 16; ++ks) acc = MFMA_32x32x16(*reinterpret_cast<const h16x8*>(kp + ks * 16), qf[ks], acc);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int j0 = kb * 32 + 8 * g + 4 * hi;
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (j0 + e < N) ? acc[4 * g + e] * a.c : -INFINITY;
                *reinterpret_cast<f32x4*>(S + l31 * pl.ss + j0) = o;
            }
        }
    }
    __syncthreads();
    // ---- 3a: v over the keys, transposed: Vt[dim][key]; dims >= D and keys >= N are zero
    for (int i = tid; i < NP * Plan::DV; i += SA_THREADS) {
        const int j = i / Plan::DV, col = i - j * Plan::DV;
        Vt[col * pl.vs + j] = (h16)((j < N && col < D) ? base[(int64_t)j * a.ldqkv + 2 * C + col] : 0.f);
    }
#else
    float* Qs = reinterpret_cast<float*>(sa_lds + pl.q_off);
    float* Ks = reinterpret_cast<float*>(sa_lds + pl.kv_off);
    float* Vs = reinterpret_cast<float*>(sa_lds + pl.kv_off);      // after the score pass
    for (int i = tid; i < SA_QT * D; i += SA_THREADS) {
        const int r = i / D, col = i - r * D, n = q0 + r;
        Qs[r * DP + col] = operand_round(n < N ? base[(int64_t)n * a.ldqkv + col] : 0.f);
    }
    for (int i = tid; i < NP * D; i += SA_THREADS) {
        const int j = i / D, col = i - j * D;
        Ks[j * DP + col] = operand_round(j < N ? base[(int64_t)j * a.ldqkv + C + col] : 0.f);
    }
    __syncthreads();
    {
        const int q = tid & 31;
        for (int j = tid >> 5; j < NP; j += SA_THREADS / 32) {
            float acc = 0.f;
#pragma unroll 8
            for (int k = 0; k < D; ++k) acc = fmaf(Qs[q * DP + k], Ks[j * DP + k], acc);
            S[q * pl.ss + j] = j < N ? acc * a.c : -INFINITY;
        }
    }
    __syncthreads();
    for (int i = tid; i < NP * D; i += SA_THREADS) {
        const int j = i / D, col = i - j * D;
        Vs[j * D + col] = operand_round(j < N ? base[(int64_t)j * a.ldqkv + 2 * C + col] : 0.f);
    }
#endif
    // ---- 3b: softmax rows, eight per wave
    for (int r = wave * (SA_QT / 4); r < (wave + 1) * (SA_QT / 4); ++r) {
        float s[(SA_NMAX + 63) / 64];
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < (SA_NMAX + 63) / 64; ++i) {
            const int j = lane + 64 * i;
            s[i] = j < NP ? S[r * pl.ss + j] : -INFINITY;
            m = fmaxf(m, s[i]);
        }
        m = wave_max(m);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < (SA_NMAX + 63) / 64; ++i) {
            const int j = lane + 64 * i;
            const float p = __builtin_amdgcn_exp2f(s[i] - m);       // 0 for a masked column
            sum += p;
            if (j < NP) {
#if MUDG_PLANES == 1
                P[r * pl.ps + j] = (h16)p;
#else
                S[r * pl.ss + j] = operand_round(p);
#endif
            }
        }
        sum = wave_sum(sum);
        if (lane == 0) L[r] = sum;
    }
    __syncthreads();
    // ---- 4: O^T = V^T P^T
#if MUDG_PLANES == 1
    if (wave < Plan::DV / 32) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const h16* vp = Vt + (wave * 32 + l31) * pl.vs + hi * 8;
        const h16* pp = P + l31 * pl.ps + hi * 8;
        for (int ks = 0; ks < NP / 16; ++ks)
            acc = MFMA_32x32x16(*reinterpret_cast<const h16x8*>(vp + ks * 16), *reinterpret_cast<const h16x8*>(pp + ks * 16), acc);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d0 = wave * 32 + 8 * g + 4 * hi;              // the lane's query is l31, its dims d0 + {0 .. 3}
            if (d0 < D) {
                f32x4 o = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
                *reinterpret_cast<f32x4*>(Of + l31 * D + d0) = o;
            }
        }
    }
#else
    {
        const int q = tid >> 3, cg = tid & 7;
        float acc[D / 8];
#pragma unroll
        for (int i = 0; i < D / 8; ++i) acc[i] = 0.f;
        for (int j = 0; j < N; ++j) {
            const float p = S[q * pl.ss + j];
#pragma unroll
            for (int i = 0; i < D / 8; ++i) acc[i] = fmaf(p, Vs[j * D + cg + 8 * i], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < D / 8; ++i) Of[q * D + cg + 8 * i] = acc[i];
    }
#endif
    __syncthreads();
    // ---- 5: normalise, round once, store
    for (int i = tid; i < SA_QT * (D / 8); i += SA_THREADS) {
        const int r = i / (D / 8), ch = i - r * (D / 8), n = q0 + r;
        if (n >= N) continue;
        const float l = L[r];
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __fdiv_rn(Of[r * D + ch * 8 + e], l);
        store8_operand(a.O + (b * N + n) * a.ldo + h * D + ch * 8, a.ldo / PLANES, v);
    }
}

int short_attn_check(const MudgShortAttnDesc* dp, const char* who) {
    MUDG_REQUIRE(dp, "%s: null descriptor", who);
    const MudgShortAttnDesc& d = *dp;
    MUDG_REQUIRE(d.d == 64 || d.d == 80, "%s: head width %d (64 or 80)", who, d.d);
    MUDG_REQUIRE(d.N >= 1 && d.N <= SA_NMAX, "%s: %d tokens (1 .. %d: every key of a head stays in LDS)", who, d.N, SA_NMAX);
    MUDG_REQUIRE(d.B >= 1 && d.B <= 65535 && d.heads >= 1 && d.heads <= 65535, "%s: B=%d heads=%d", who, d.B, d.heads);
    const int64_t C = (int64_t)d.heads * d.d;
    MUDG_REQUIRE(d.ldqkv >= 3 * C, "%s: ldqkv=%lld is less than 3 C = %lld", who, (long long)d.ldqkv, (long long)(3 * C));
    MUDG_REQUIRE(d.ldo % (8 * PLANES) == 0 && d.ldo / PLANES >= C, "%s: ldo=%lld (a multiple of %d, ldo / %d >= C = %lld)", who,
                 (long long)d.ldo, 8 * PLANES, PLANES, (long long)C);
    return MUDG_OK;
}

template <int D>
int short_attn_launch(const MudgShortAttnDesc& d, hipStream_t s) {
    const SaPlan<D> pl(d.N), most(SA_NMAX);
    const int rc = mudg_lds_opt_in<short_attn_kernel<D>>(most.total, "mudg_short_attention");
    if (rc != MUDG_OK) return rc;
    SaArgs a;
    a.QKV = d.QKV; a.O = static_cast<h16*>(d.O); a.N = d.N; a.heads = d.heads; a.ldqkv = d.ldqkv; a.ldo = d.ldo;
    a.c = d.scale * 1.4426950408889634f;
    const dim3 grid((unsigned)((d.N + SA_QT - 1) / SA_QT), (unsigned)d.heads, (unsigned)d.B);
    hipLaunchKernelGGL(short_attn_kernel<D>, grid, dim3(SA_THREADS), (size_t)pl.total, s, a);
    return mudg_check_launch("mudg_short_attention");
}

// ---------------------------------------------------------------------------------------------- LayerNorm, fp32 out
// One wave per row; the row is read three times (sum, squared deviations, apply) — ln_pre runs once per call.  The arithmetic of
// ln_kernel (norm.hip) without the operand store.
__global__ __launch_bounds__(256) void ln_f32_kernel(const float* __restrict__ X, int64_t ldx, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* __restrict__ Y, int64_t ldy, int rows, int C,
                                                     float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* x = X + row * ldx;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += x[c];
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) { const float dlt = x[c] - mean; q = fmaf(dlt, dlt, q); }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
    float* y = Y + row * ldy;
    for (int c = lane; c < C; c += 64) y[c] = fmaf((x[c] - mean) * rstd, gamma[c], beta[c]);
}

// ---------------------------------------------------------------------------------------------- CLIP preprocessing
constexpr int CLIP_SIZE = 224, CLIP_PATCH = 14, CLIP_GRID = 16, CLIP_K = 3 * CLIP_PATCH * CLIP_PATCH, CLIP_KPAD = 592;
constexpr int CLIP_MAX_TAPS = 255;

struct CubicTap { int s[4]; int c[4]; };        // four source indices, the fp32 bits of four coefficients

struct ClipArgs {
    const float* src;
    const CubicTap* yt;
    const CubicTap* xt;
    const float* gy;
    const float* gx;
    int ky, kx, H, W;
    h16* patches;
    int64_t ldp;
    float* image;
    float mean[3], std[3];
};

__device__ __forceinline__ int clip_inside(int s, int n) { return min(max(s, 0), n - 1); }
// reflect border without the edge (-1 -> 1, n -> n - 2), then clamped: no index leaves the image whatever the tap count
__device__ __forceinline__ int clip_reflect(int s, int n) {
    s = s < 0 ? -s : s;
    s = s >= n ? 2 * (n - 1) - s : s;
    return clip_inside(s, n);
}

// the blurred image at (y, x): along x first, then along y, each sum from its first tap on
__device__ __forceinline__ float clip_blurred(const ClipArgs& a, const float* __restrict__ img, int y, int x) {
    if (a.ky == 0) return img[(int64_t)y * a.W + x];
    float acc = 0.f;
    for (int iy = 0; iy < a.ky; ++iy) {
        const float* row = img + (int64_t)clip_reflect(y + iy - a.ky / 2, a.H) * a.W;
        float hsum = 0.f;
        for (int ix = 0; ix < a.kx; ++ix) {
            const float t = __fmul_rn(a.gx[ix], row[clip_reflect(x + ix - a.kx / 2, a.W)]);
            hsum = ix == 0 ? t : __fadd_rn(hsum, t);
        }
        const float t = __fmul_rn(a.gy[iy], hsum);
        acc = iy == 0 ? t : __fadd_rn(acc, t);
    }
    return acc;
}

__global__ __launch_bounds__(256) void clip_preprocess_kernel(const ClipArgs a) {
    const int dx = threadIdx.x, dy = blockIdx.x, c = blockIdx.y;
    const int64_t b = blockIdx.z;
    if (dx >= CLIP_SIZE) return;
    const CubicTap ty = a.yt[dy], tx = a.xt[dx];
    const float* img = a.src + (b * 3 + c) * a.H * a.W;
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int sy = clip_inside(ty.s[i], a.H);
        float rh = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = __fmul_rn(__int_as_float(tx.c[j]), clip_blurred(a, img, sy, clip_inside(tx.s[j], a.W)));
            rh = j == 0 ? t : __fadd_rn(rh, t);
        }
        const float t = __fmul_rn(__int_as_float(ty.c[i]), rh);
        r = i == 0 ? t : __fadd_rn(r, t);
    }
    const float v = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(r, 1.0f), 0.5f), a.mean[c]), a.std[c]);
    if (a.image) a.image[((b * 3 + c) * CLIP_SIZE + dy) * CLIP_SIZE + dx] = v;
    const int gy = dy / CLIP_PATCH, py = dy - gy * CLIP_PATCH, gx = dx / CLIP_PATCH, px = dx - gx * CLIP_PATCH;
    h16* row = a.patches + (b * (CLIP_GRID * CLIP_GRID) + CLIP_GRID * gy + gx) * a.ldp;
    const int64_t ps = a.ldp / PLANES;
    store1_operand(row + c * (CLIP_PATCH * CLIP_PATCH) + CLIP_PATCH * py + px, ps, v);
    if (c == 0 && py == 0 && px < CLIP_KPAD - CLIP_K) store1_operand(row + CLIP_K + px, ps, 0.f);       // the K padding of the patch GEMM
}

}  // namespace

extern "C" int mudg_short_attention_ok(const MudgShortAttnDesc* d) { return short_attn_check(d, "mudg_short_attention_ok") == MUDG_OK ? 1 : 0; }

extern "C" int mudg_short_attention(const MudgShortAttnDesc* dp, void* stream) {
    const int rc0 = short_attn_check(dp, "mudg_short_attention");
    if (rc0 != MUDG_OK) return rc0;
    const MudgShortAttnDesc& d = *dp;
    MUDG_REQUIRE(d.QKV && d.O, "mudg_short_attention: null pointer");
    MUDG_REQUIRE(aligned16(d.O) && (reinterpret_cast<uintptr_t>(d.QKV) & 3u) == 0, "mudg_short_attention: O is 16-byte aligned, QKV is fp32");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int slot = mudg_prof_begin(MUDG_FAM_ATTN, s);
    const int rc = d.d == 80 ? short_attn_launch<80>(d, s) : short_attn_launch<64>(d, s);
    const double items = (double)d.B * d.heads;
    mudg_prof_end(slot, s, 4.0 * items * d.N * d.N * d.d, items * d.N * d.d * (3 * 4.0 + 2.0));
    return rc;
}

extern "C" int mudg_layernorm_f32(const float* X, int64_t ldx, const float* gamma, const float* beta, float* Y, int64_t ldy, int rows,
                                  int C, float eps, void* stream) {
    MUDG_REQUIRE(X && Y && gamma && beta, "mudg_layernorm_f32: null pointer");
    MUDG_REQUIRE(rows > 0 && C > 0 && ldx >= C && ldy >= C, "mudg_layernorm_f32: rows=%d C=%d ldx=%lld ldy=%lld", rows, C, (long long)ldx,
                 (long long)ldy);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int slot = mudg_prof_begin(MUDG_FAM_LNORM, s);
    hipLaunchKernelGGL(ln_f32_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, X, ldx, gamma, beta, Y, ldy, rows, C, eps);
    const int rc = mudg_check_launch("mudg_layernorm_f32");
    mudg_prof_end(slot, s, 0.0, (double)rows * C * 8.0);
    return rc;
}

extern "C" int mudg_clip_preprocess(const float* src, int B, int H, int W, const int32_t* ytab, const int32_t* xtab, const float* gy, int ky,
                                    const float* gx, int kx, void* patches, int64_t ldp, float* image, void* stream) {
    MUDG_REQUIRE(src && ytab && xtab && patches, "mudg_clip_preprocess: null pointer");
    MUDG_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= (1 << 28), "mudg_clip_preprocess: %d images of %d x %d", B, H, W);
    MUDG_REQUIRE((ky == 0 && kx == 0) || (gy && gx && ky > 0 && kx > 0 && (ky & 1) && (kx & 1) && ky <= CLIP_MAX_TAPS && kx <= CLIP_MAX_TAPS),
                 "mudg_clip_preprocess: blur of %d x %d taps (both 0, or both odd, at most %d, with their tables)", ky, kx, CLIP_MAX_TAPS);
    MUDG_REQUIRE(aligned16(ytab) && aligned16(xtab), "mudg_clip_preprocess: the tables are 32-byte entries, 16-byte aligned");
    MUDG_REQUIRE(aligned16(patches) && ldp % (8 * PLANES) == 0 && ldp / PLANES >= CLIP_KPAD,
                 "mudg_clip_preprocess: ldp=%lld (a multiple of %d, ldp / %d >= %d), patches 16-byte aligned", (long long)ldp, 8 * PLANES, PLANES,
                 CLIP_KPAD);
    ClipArgs a = {};
    a.src = src; a.yt = reinterpret_cast<const CubicTap*>(ytab); a.xt = reinterpret_cast<const CubicTap*>(xtab); a.gy = gy; a.gx = gx;
    a.ky = ky; a.kx = kx; a.H = H; a.W = W; a.patches = static_cast<h16*>(patches); a.ldp = ldp; a.image = image;
    a.mean[0] = 0.48145466f; a.mean[1] = 0.4578275f; a.mean[2] = 0.40821073f;          // condition.py:318-319
    a.std[0] = 0.26862954f; a.std[1] = 0.26130258f; a.std[2] = 0.27577711f;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int slot = mudg_prof_begin(MUDG_FAM_MISC, s);
    hipLaunchKernelGGL(clip_preprocess_kernel, dim3(CLIP_SIZE, 3, (unsigned)B), dim3(256), 0, s, a);
    const int rc = mudg_check_launch("mudg_clip_preprocess");
    mudg_prof_end(slot, s, 0.0, (double)B * 3 * ((double)H * W * 4.0 + CLIP_SIZE * CLIP_SIZE * 2.0));
    return rc;
}
