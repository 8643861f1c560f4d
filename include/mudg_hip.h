/*
 * mudg_hip.h — C-ABI of libmudg_hip.so: the MI355X (gfx950) kernels under MuDG's
 * video-diffusion denoising path (3D-UNet + DDIM update + AutoencoderKL decode).
 *
 * The reference (heiheishuang/MuDG) has no FFI layer: its hot path is PyTorch
 * module code whose arithmetic is dispatched implicitly to ATen/cuDNN/cuBLAS.
 * Each entry point below replaces one such implicit kernel class; the reference
 * call sites it stands in for are cited as file:line (relative to the reference
 * tree).  SURVEY.md §2.1 numbers the classes K1..K16.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *     named host_*; the caller owns and allocates all buffers (outputs too);
 *   - activations are channels-last: a tensor (F, H, W, C) is a row-major
 *     matrix of F*H*W rows ("pixels"/"tokens") by C channels, bf16;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and returns immediately;
 *   - return value: 0 on success, a negative MUDG_E* code on error; nothing is
 *     thrown across the ABI and no call synchronises the device;
 *   - no hidden global state apart from the optional event profiler.
 */
#ifndef MUDG_HIP_H
#define MUDG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MUDG_OK          0
#define MUDG_EINVAL     -1   /* bad argument (shape / alignment / null pointer) */
#define MUDG_ELAUNCH    -2   /* the HIP runtime rejected a launch */
#define MUDG_EUNSUPPORTED -3 /* shape outside what the kernels implement */

/* ABI version; bumped whenever a struct below changes. */
int mudg_version(void);
/* MFMA operand type of this build: 0 = bfloat16 (libmudg_hip.so), 1 = IEEE fp16 (libmudg_hip_fp16.so),
 * 2 = split bf16 x 2 planes (libmudg_hip_x3.so: 16 significand bits, 3 MFMAs per product tile),
 * 3 = split bf16 x 3 planes (libmudg_hip_x6.so: 24 significand bits, 6 MFMAs per product tile: fp32-class).
 * Wherever this header says "bf16" for an operand buffer, the fp16 build expects fp16 in its place, and the split builds
 * expect PLANES bf16 pieces per value: piece p of element (r, c) of a rows matrix with row stride ld lives at
 * r * ld + p * (ld / PLANES) + c, value = sum of the pieces, piece 0 = bf16(value), piece 1 = bf16(value - piece 0), ...
 * (so an operand matrix of width C needs ld >= PLANES * C, and ld a multiple of 8 * PLANES).  fp32 buffers (residual
 * stream, biases, statistics) are the same in every build. */
int mudg_operand_dtype(void);
/* Text for the most recent non-zero return on this thread. */
const char* mudg_last_error(void);

/* ------------------------------------------------------------------ GEMM / conv
 * Y[m][n] = epilogue( alpha * sum_k X[m][k] * W[n][k] )          (bf16 in, fp32 accumulate)
 *
 * One MFMA kernel serves every dense contraction on the path:
 *   mode 0  plain GEMM           nn.Linear / 1x1 Conv / Conv1d k=1
 *                                (attention.py:53-57,424,447,493,519,582,602; openaimodel3d.py:168-174,187;
 *                                 ae_modules.py:31-50 q/k/v/proj_out, :181 nin_shortcut; autoencoder.py:35)
 *   mode 1  3x3 conv, pad 1      implicit GEMM over 9 taps on NHWC input, stride 1|2, optional
 *                                nearest-2x upsample fused into the read
 *                                (openaimodel3d.py:66-70,96,103,154,179,401,564; ae_modules.py:117-127,162-175,499,535)
 *   mode 2  temporal (3,1,1) conv implicit GEMM over 3 taps along T on (B,T,H,W,C)
 *                                (openaimodel3d.py:255-266)
 * W is always [N][K] row-major with K = taps*Cin ordered tap-major (the host packs it once).
 * X may be split over two sources along channels (skip-concat, openaimodel3d.py:621):
 * channels [0,csplit) come from X, [csplit,Cin) from X2.
 */
typedef struct MudgGemmDesc {
    const void* X;        /* bf16 activations */
    const void* X2;       /* second channel source or NULL */
    const void* W;        /* bf16 packed weights [N][K] */
    void*       Y;        /* bf16 (or fp32 if out_fp32) [M][ldy] */
    const float* bias;    /* fp32 [N] or NULL (packed like W's rows) */
    const float* gbias;   /* fp32 [M/rows_per_group][Nout] or NULL: per-row-group bias
                             (timestep-embedding add, openaimodel3d.py:219-228) */
    const void* R;        /* residual [M][ldr] (bf16, or fp32 if res_fp32) or NULL, added last */
    int M, N, K;
    int ldx, ldx2, ldw, ldy, ldr;   /* row strides in elements */
    int csplit;           /* channels served by X (== Cin when X2 is NULL) */
    int batch;            /* blockIdx.z count (>=1) */
    int64_t sX, sW, sY, sR;         /* per-batch strides in elements */
    int rows_per_group;   /* for gbias; 0 = unused */
    int out_fp32;         /* storage of Y: 0 = MFMA operand (bf16 ...), 1 = fp32, 2 = IEEE fp16 */
    int res_fp32;         /* storage of R, same codes.  The residual stream (block outputs, the transformers' token stream,
                             encoder skips: what later layers add onto) is kept as fp16 by the 16-bit builds' callers — the
                             reference's own stream is fp16 under torch.autocast — and as fp32 by the split-operand builds' */
    int geglu;            /* 1: W rows are packed [32 value | 32 gate] blocks and
                             Y[m][j] = v_j * gelu_erf(g_j), Nout = N/2 (attention.py:579-586) */
    int act;              /* 1: Y = gelu_erf(.) applied after bias (Perceiver FeedForward, resampler.py:27-34); 0: none */
    float alpha;
    int mode;             /* 0 | 1 | 2 */
    /* mode 1 */
    int Hin, Win, Hout, Wout, Cin, stride, upsample;
    int pad;              /* mode 1: leading zero padding rows/cols (1 = the usual pad 1; 0 = AutoencoderKL's stride-2
                             downsample, which pads (0,1,0,1): only bottom/right, ae_modules.py:104-106) */
    int korder;           /* mode 1: 0 = W's K axis is [tap][Cin]; 1 = [Cin/64][tap][64] (needs Cin % 64 == 0): the nine
                             taps of a 64-channel slab are consecutive K tiles, so the shifted re-reads of the input
                             hit L2 instead of coming back after a whole sweep over Cin.
                             mode 2: 1 = the same slab-major order [Cin/64][tap][64]; needs T = 16, HW % 8 == 0, Cin % 64 == 0, one
                             source, the 16-bit or bf16x3 builds.  A 128-row tile is then 8 pixels x 16 frames of one clip (the
                             three temporal taps of a row are rows of the same tile), and `stats` blocks are those TILES, in
                             clip order: only a clip-level GroupNorm may fold them */
    /* mode 2 */
    int T, HW;            /* mode 0: HW may carry a HINT — the rows of one frame of the matrix (0 = none): it lets the library choose a tile
                             height that divides a frame (mudg_gemm_stats_rows).  Never M decides, so a row's result does not depend on
                             the batch it travels in; with a residual R the 288-row tile (and the 160-row tile for an fp32 R) adds R first instead of last (last-bit
                             differences against the un-hinted call), without one the bits are the same */
    float* stats;         /* NULL, or fp32 [ceil(M/rows)][Nout][2], rows = mudg_gemm_stats_rows(d) (128 | 160 | 288): the epilogue also writes, per row block and output
                             channel, the sum and the sum of squares of the values it stored (as stored: after rounding to
                             bf16 when Y is bf16) — the first pass of the GroupNorm that consumes Y
                             (mudg_groupnorm_fused).  Needs batch == 1 and no GEGLU. */
    int subpixel;         /* mode 1: 1 = the sub-pixel form of "nearest-2x upsample, then 3x3 / pad 1 conv" (openaimodel3d.py:92-106,
                             ae_modules.py:77-92).  An output pixel (2 oy + py, 2 ox + px) of the upsampled image only ever sees a
                             2 x 2 neighbourhood of the LOW-resolution input, its nine taps collapsing onto four summed weights:
                             4/9 of the multiply-adds.  X is the low-resolution image (Hout x Wout == Hin x Win is the grid
                             walked, M = frames * Hin * Win); batch = 4 with entry z = 2 py + px; W holds the four [N][4 Cin]
                             matrices sW apart, K ordered [Cin/64][tap 0..3][64] with tap = 2 a + b reading input pixel
                             (oy - 1 + py + a, ox - 1 + px + b); Y is the (2 Hin x 2 Win) image, row ((f 2Hin) + 2 oy + py) 2Win
                             + 2 ox + px.  Needs what mudg_conv_subpixel_ok checks. */
    void* Y8; void* S8;   /* 16-bit builds, optional: also write the OCP MX-fp8 copy of Y (an operand-kind result of a plain or conv
                             problem, N % 32 == 0, no GEGLU) — e4m3 bytes Y8[m][ldy8] and one E8M0 scale per 32 columns S8[m][lds8],
                             bit-equal to mudg_quantize_mxfp8 of Y: the q | k projection of the long self-attention quantises its own
                             output for the fp8 score path (BASELINE config 5) instead of two more passes over it */
    int ldy8, lds8;
} MudgGemmDesc;
int mudg_gemm(const MudgGemmDesc* d, void* stream);
/* Height of the row blocks in which mudg_gemm will write `stats` for this problem: 128, or 288 where the 288 x 320-tile kernel
 * runs it (same-size 3x3 convs, temporal convs with korder 0 and plain GEMMs with N % 320 == 0 whose frames are
 * whole 288-row tiles: Hout * Wout, HW — for mode 0 the caller's hint in HW — a multiple of 288), or 160 where the 160 x 320-tile
 * kernel of the 16-bit builds does (round 6: the same problems when a frame is whole 160-row tiles but not whole 288-row ones and
 * has at least 640 rows — MDM512's 2560- and 640-pixel frames; plain GEMMs there from K = 1280).  `stats` then holds
 * fp32 [ceil(M / rows)][Nout][2], and the consumer (mudg_groupnorm_fused) is told the same height.  The answer depends on the
 * descriptor's geometry, strides and pointer alignment, never on M: a clip's results do not depend on the batch it travels in. */
int mudg_gemm_stats_rows(const MudgGemmDesc* d);
/* 1 when `d` (mode 1, subpixel = 1) can run: batch 4, stride 1, pad 1, korder 1, Cin % 64 == 0, no X2 / R / gbias / stats /
 * upsample, and offsets within reach of the buffer-descriptor loader; else the caller uses upsample = 1 with 3x3 weights. */
int mudg_conv_subpixel_ok(const MudgGemmDesc* d);
/* 1 when mudg_gemm runs `d` on the stream kernel of the 16-bit builds (plain GEMMs with K = 320 and N = 320 or 640, a 16-bit result and residual, no
 * GroupNorm partials, frames of whole 288-row tiles: the same sums as the 288 x 320-tile kernel, so no result depends on the answer).
 * Needs a current device (the kernel's grid is its CU count); 0 without one.  For tests and measurements. */
int mudg_gemm_stream_ok(const MudgGemmDesc* d);

/* ------------------------------------------------------------------ attention
 * Flash-style softmax(scale * Q K^T) V for head dim 64, never materialising the score matrix.
 *   spatial self-attention  attention.py:81-144 (attn1, 393)     Nq = Nk = H*W
 *   text / image cross-attn attention.py:89-94,128-142 (attn2)   Nk = 77 / 16; `accumulate` adds
 *                                                                 the second softmax's output
 * Q : rows (f*Nq + i), head h at columns [h*64, h*64+64), row stride ldq
 * K : rows ((f / kv_div)*Nk + j), same column convention, row stride ldk
 * Vt: V transposed per (kv batch, head): row (h*64 + d), column j, row stride ldvt,
 *     batch stride svt elements (the producing GEMM writes it in this layout)
 * O : like Q with row stride ldo
 */
typedef struct MudgAttnDesc {
    const void* Q; const void* K; const void* Vt; void* O;
    int F, heads, Nq, Nk;
    int ldq, ldk, ldvt, ldo;
    int64_t svt;
    int kv_div;          /* frames sharing one K/V batch entry (T for text context, 1 otherwise) */
    float scale;         /* dim_head**-0.5 */
    int accumulate;      /* 1: O += result */
    /* Optional second key / value set with its OWN softmax, outputs summed — the text + image cross-attention of
     * attention.py:128-142 (out = softmax(q k_text^T) v_text + softmax(q k_ip^T) v_ip) in one launch: Q is read once and
     * O written once.  K2 == NULL: single set.  Same layout conventions as K / Vt. */
    const void* K2; const void* Vt2;
    int Nk2, ldk2, ldvt2, kv_div2;
    int64_t svt2;
    /* MX-fp8 scores (BASELINE config 5; needs q_prescaled, Nk % 64 == 0, Nq >= 512): when Q8 is not NULL, Q K^T runs on
     * v_mfma_scale_f32_32x32x64_f8f6f4 — twice the bf16 MFMA rate — from OCP e4m3 copies of Q and K with one E8M0 power-of-two
     * scale per 32 consecutive head dims (mudg_quantize_mxfp8 makes both); softmax and P V stay as in the bf16 kernel
     * (P and V^T are bf16).  Q8 / K8: fp8 rows with the row -> (frame, token) and column -> (head, dim) conventions of
     * Q / K, row strides ldq8 / ldk8 BYTES; Qs / Ks: scale bytes, column 2 * head + (dim / 32), row strides ldqs / ldks. */
    const void* Q8; const void* K8; const void* Qs; const void* Ks;
    int ldq8, ldk8, ldqs, ldks;
    int q_prescaled;     /* 1: Q already carries scale * log2(e) (folded into the q-projection weights when they are packed),
                            so Q K^T is directly the base-2 exponent and `scale` is ignored.  The long self-attention kernel
                            then runs its lean softmax: the running reference maximum enters as the score accumulator's
                            initial value, one v_exp + one add per score, and the rescale of O only happens when a row sum
                            outgrows 2^40 (never on real data after the first tile). */
    float* Lse;          /* optional, fp32 [F Nq][heads]: the log2-sum-exp of the scaled scores of every (query, head) — what
                            mudg_attention_bwd needs to rebuild P without a statistics pass (single key / value set, not
                            prescaled, 16-bit builds) */
} MudgAttnDesc;
int mudg_attention(const MudgAttnDesc* d, void* stream);
/* OCP microscaling quantisation of an operand matrix (16-bit builds): every 32 consecutive columns of a row share one
 * E8M0 scale 2^(floor(log2 amax) - 8) and are stored as e4m3 (saturating): Y8[r][c] (row stride ldy bytes),
 * S[r][c / 32] (row stride lds bytes).  cols % 32 == 0. */
int mudg_quantize_mxfp8(const void* X, int ldx, int64_t rows, int cols, void* Y8, int ldy, void* S, int lds, void* stream);

/* Temporal self-attention over T <= 32 frames per pixel (attention.py:529-576 via 81-144):
 * QKV rows are ((b*T + t)*HW + p); q at columns [h*64..], k at C + h*64, v at 2C + h*64. */
int mudg_temporal_attention(const void* QKV, void* O, int B, int T, int HW, int heads,
                            int ldqkv, int ldo, float scale, void* stream);
/* The same attention with its q | k | v projection in front, in one kernel (16-bit builds; attention.py:53-55 to_q / to_k / to_v,
 * bias-free): O = attention over T of (X Wh^T), where the projected rows are rounded to the operand type exactly as mudg_gemm
 * stores them but never leave the CU.  X: operand rows [B T HW][ldx], C = 64 heads channels (the LayerNorm's output); Wh: the
 * HEAD-PACKED weight [3 C][ldw], row 192 h + 64 j + d = row 64 h + d of to_q (j = 0), to_k (1), to_v (2); O: operand rows
 * [B T HW][ldo].  Needs what the query below checks, a dry call that reads nothing: T = 16, HW % 8 == 0, head width 64
 * (C == 64 heads), row strides that are multiples of 8 and at least C, a 16-bit build (0 in the split-operand builds).  Anything
 * else takes mudg_gemm and mudg_temporal_attention.  Booked in MUDG_FAM_GEMM with flops = 2 M 3C C + 4 items T T 64 and the
 * algorithmic bytes (X, Wh and O once). */
int mudg_temporal_self_attention_ok(int T, int HW, int heads, int C, int64_t ldx, int64_t ldw, int64_t ldo);
int mudg_temporal_self_attention(const void* X, const void* Wh, void* O, int B, int T, int HW, int heads, int C, int64_t ldx,
                                 int64_t ldw, int64_t ldo, float scale, void* stream);

/* ------------------------------------------------------------------ normalisation
 * GroupNorm(32 groups) on channels-last data with optional fused SiLU / swish
 * (basics.py:76-87 GroupNormSpecific eps 1e-5; openaimodel3d.py:256-265; attention.py:420,488 eps 1e-6;
 *  ae_modules.py:10-16 eps 1e-6).  Statistics are per (sample, group) over `rows` pixels, where a
 * sample is one frame (2D norms) or one clip of T frames (the 5-D norms).  Two sources as in GEMM.
 * `ws` is fp32 scratch of at least mudg_groupnorm_ws_floats(samples, groups, rows).
 */
int64_t mudg_groupnorm_ws_floats(int samples, int groups, int rows);
int mudg_groupnorm(const void* X, const void* X2, int csplit, int ldx, int ldx2, int x_fp32,
                   const float* gamma, const float* beta, void* Y, int ldy,
                   int samples, int rows, int C, int groups, float eps, int silu,
                   float* ws, void* stream);
/* x_fp32: storage of X (and X2): 0 = operand (bf16 ...), 1 = fp32, 2 = IEEE fp16 (the residual stream of the 16-bit
 * builds); Y is always an MFMA operand (it feeds a GEMM).  Same codes in mudg_layernorm, mudg_cast_rows (src_fp32 /
 * dst_fp32) and mudg_rows_to_ncthw (src_is_fp32). */
/* Same normalisation with the statistics pass replaced by the per-(128-row block, channel) partial sums the producing
 * GEMM / conv wrote (MudgGemmDesc.stats): P1 covers X's csplit channels, P2 (NULL without X2) X2's C - csplit.
 * Needs rows % 128 == 0 (a row block never straddles two samples).  ws: fp32 scratch of 2 * samples * groups floats. */
int mudg_groupnorm_fused(const void* X, const void* X2, int csplit, int ldx, int ldx2, int x_fp32,
                         const float* gamma, const float* beta, void* Y, int ldy,
                         int samples, int rows, int C, int groups, float eps, int silu,
                         const float* P1, const float* P2, float* ws, void* stream);

/* The same with the height of the partial blocks stated per source (mudg_gemm_stats_rows of the producer: 128 | 160 | 288; `rows` must be
 * a multiple of both; mudg_groupnorm_fused = 128, 128). */
int mudg_groupnorm_fused_rows(const void* X, const void* X2, int csplit, int ldx, int ldx2, int x_fp32,
                              const float* gamma, const float* beta, void* Y, int ldy,
                              int samples, int rows, int C, int groups, float eps, int silu,
                              const float* P1, int p1_rows, const float* P2, int p2_rows, float* ws, void* stream);

/* LayerNorm over the last dim (attention.py:363-365, eps 1e-5). */
int mudg_layernorm(const void* X, int ldx, int x_fp32, const float* gamma, const float* beta,
                   void* Y, int ldy, int rows, int C, float eps, void* stream);

/* Row softmax of fp32 scores (already scaled) to bf16 probabilities
 * (ae_modules.py:64-68: the VAE's single-head d=512 attention). */
int mudg_softmax_rows(const float* S, int lds, void* P, int ldp, int rows, int cols, void* stream);

/* ------------------------------------------------------------------ embeddings / small linears
 * Sinusoidal embedding (utils_diffusion.py:8-28): out[i][:] = [cos(t_i f_j), sin(t_i f_j)], fp32.
 * freqs: device fp32 [dim/2] table exp(-ln(max_period) j / (dim/2)), built on the host as the reference does. */
int mudg_timestep_embedding(const int64_t* t, const float* freqs, float* out, int n, int dim, void* stream);
/* y[m][n] = act_out( sum_k act_in(x[m][k]) * W[n][k] + b[n] ), fp32 I/O, bf16 or fp32 weights, m <= 64
 * (time/class/fps MLPs openaimodel3d.py:377-397,569-602; ResBlock emb_layers 168-174). act: 0 none, 1 SiLU. */
int mudg_small_linear(const float* x, const void* W, int w_is_bf16, const float* b, float* y,
                      int M, int N, int K, int act_in, int act_out, int accumulate, void* stream);

/* ------------------------------------------------------------------ layout changes at the API boundary
 * (b c t h w) fp32/bf16 -> channels-last bf16 rows ((b t) h w) with channel offset/stride
 * (openaimodel3d.py:591; ddpm3d.py:1317-1319 channel concat of x and c_concat), and back (openaimodel3d.py:627). */
int mudg_ncthw_to_rows(const void* src, int src_is_fp32, void* dst, int B, int C, int T, int HW,
                       int ld, int coff, int Ttot, int t0, void* stream);
int mudg_rows_to_ncthw(const void* src, int src_is_fp32, int ld, int coff, void* dst, int dst_is_fp32,
                       int B, int C, int T, int HW, float scale, int Ttot, int t0, void* stream);
/* Ttot/t0: the (b c t h w) tensor holds Ttot frames and frames [t0, t0+T) are converted (Ttot <= 0: Ttot = T). */
/* Strided 2-D copy of bf16 rows (context token split, openaimodel3d.py:582-585) and y += alpha * x on fp32
 * vectors (summing the time / class / fps embeddings, openaimodel3d.py:576,602). */
int mudg_copy_rows(const void* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int64_t cols, void* stream);
int mudg_axpy_f32(float* y, const float* x, int64_t n, float alpha, void* stream);
/* out[b][:] = ca[b] x[b][:] + cb[b] y[b][:] on fp32 (B, n): q_sample / predict_start_from_z_and_v /
 * predict_eps_from_z_and_v (ddpm3d.py:239-251) with ca, cb gathered per sample (device fp32 [B]). */
int mudg_lincomb(float* out, const float* x, const float* y, const float* ca, const float* cb, int B, int64_t n,
                 void* stream);
/* fp32 -> bf16 cast of n contiguous elements (a fp32 stream tensor entering an MFMA GEMM as an operand).
 * 16-bit-operand builds only (a flat cast has no plane layout); mudg_cast_rows serves every build. */
int mudg_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream);
/* dst[r][c] = src[r][c] for rows x cols elements between rows matrices of any kind, any direction: operand
 * (*_fp32 = 0: h16, or PLANES pieces per value in the split builds), fp32 (1) or fp16 (2).  Row strides in elements.
 * This is how fp32 tensors (context tokens ddpm3d.py:1320-1322, skip-conv inputs) become MFMA operands and how an
 * operand matrix is read back as fp32. */
int mudg_cast_rows(const void* src, int src_fp32, int64_t lds, void* dst, int dst_fp32, int64_t ldd, int64_t rows,
                   int64_t cols, void* stream);
/* Zero the channel range [c0, c1) of a rows buffer (padding lanes of the stem input). */
int mudg_zero_channels(void* dst, int rows, int ld, int c0, int c1, void* stream);

/* ------------------------------------------------------------------ DDIM update (ddim.py:205-279)
 * One call per step on fp32 latents, n elements per sample:
 *   v  = e_u + cfg*(e_c - e_u)                      two-way guidance, or with e_m (image-only conditioning) the
 *        e_u + cfg_img*(e_m - e_u) + cfg*(e_c - e_m) three-way form of ddim_multiplecond.py:226-233;
 *   v = phi*v*std(e_c)/std(v) + (1-phi)*v            (utils_diffusion.py:147-157)
 *   e  = sqrt_ac*v + sqrt_1mac*x ;  x0 = sqrt_ac*x - sqrt_1mac*v          (v-prediction, ddpm3d.py:239-251; eps_form = 0)
 *   e  = v ;                        x0 = (x - sqrt_1mac*e) / sqrt_ac      (eps-prediction, ddim.py:227-258; eps_form = 1,
 *                                                                          sqrt_ac = sqrt(a_t), sqrt_1mac = sqrt(1 - a_t))
 *   x0 *= rescale ;  x_prev = sqrt(a_prev)*x0 + dir_coef*e + sigma*noise
 * host_coef = {cfg, phi, sqrt_ac, sqrt_1mac, rescale, sqrt_a_prev, dir_coef, sigma, cfg_img, eps_form}
 *             (HOST pointer, 10 floats).
 * ws: fp64 device scratch of mudg_ddim_ws_doubles(B) doubles. e_u may be NULL (no guidance: v = e_c);
 * noise may be NULL (eta = 0). */
int64_t mudg_ddim_ws_doubles(int B);
int mudg_ddim_step(const float* x, const float* e_c, const float* e_u, const float* e_m, const float* noise,
                   float* x_prev, float* pred_x0, int B, int64_t n, const float* host_coef,
                   double* ws, void* stream);

/* ------------------------------------------------------------------ VAE posterior (distributions.py:24-40)
 * moments (N, 2C, HW) fp32 planar: mean = [:, :C], logvar = clamp([:, C:], -30, 20);
 * out (N, C, HW) = scale * (mean + exp(0.5 logvar) * noise); noise NULL = posterior mode. */
int mudg_gaussian_sample(const float* moments, const float* noise, float* out, int N, int C, int HW, float scale,
                         void* stream);

/* ------------------------------------------------------------------ training from a data batch (ddpm3d.py:1064-1149)
 * posterior_assemble: the posterior samples of the three VAE encodes of get_batch_input in one launch, written in the layout
 *   the UNet takes.  mom_* (B*T, 2C, HW) fp32 moments of the dense / sparse colour / sparse depth frames, frame n = b*T + t;
 *   noise_* (B*T, C, HW), all three or none (NULL = posterior mode); the arithmetic of mudg_gaussian_sample, bit for bit:
 *   z (B, C, T, HW) = sample(mom_x);  c_concat (B, 2C, T, HW) = [sample(mom_sparse) | sample(mom_depth)] along the channels.
 * cond_dropout: classifier-free-guidance dropout from the device vector r (B uniform draws), thresholds p, p2 = 2p, p3 = 3p
 *   rounded to fp32 by the caller:  prompt_out (B, LD) = r < p2 ? null_prompt (LD) : cond_emb (B, LD);
 *   img_out (B, C, HW) = (1 - (r >= p)(r < p3)) * img, img read at img + b*img_bstride + c*img_cstride (floats): the key frame
 *   of a (B, C, T, HW) clip is read in place. */
int mudg_posterior_assemble(const float* mom_x, const float* mom_sparse, const float* mom_depth, const float* noise_x,
                            const float* noise_sparse, const float* noise_depth, float* z, float* c_concat, int B, int T, int C,
                            int64_t HW, float scale, void* stream);
int mudg_cond_dropout(const float* r, float p, float p2, float p3, const float* cond_emb, const float* null_prompt,
                      float* prompt_out, int B, int64_t LD, const float* img, int64_t img_bstride, int64_t img_cstride,
                      float* img_out, int C, int64_t HW, void* stream);

/* ------------------------------------------------------------------ post-processing of decoded frames
 * (virtual_render/eval_tools.py: byte / integer work, results bit-equal to the reference's)
 * frames_to_u8:     out[b][t][p][c] = (uint8) trunc((clamp(v[b][c][t][p], -1, 1) + 1) / 2 * 255)      eval_tools.py:22-27
 *                   clamp(x, -1, 1) = fminf(fmaxf(x, -1), 1): what is not a number becomes -1, byte 0; + 1, / 2, * 255 each in fp32
 * depth_from_u8:    depth[i] = ((r + g + b) / 3) / 255 over `pixels` (.., 3)-interleaved uint8 pixels   eval_tools.py:71
 * semantic_nearest: planar (3, hw) uint8 image -> label of the nearest of the 19 palette colours (Euclidean distance,
 *                   first minimum wins) and the image recoloured with the palette                       eval_tools.py:309-347 */
int mudg_frames_to_u8(const float* video, uint8_t* out, int B, int C, int T, int64_t HW, void* stream);
int mudg_depth_from_u8(const uint8_t* frames, float* depth, int64_t pixels, void* stream);
/* The frame sheet of a logged entry (utils/save_video.py:62-136): video (N, C, T, H, W) fp32, C = 1 or 3 -> out (T, N H, W, 3) uint8,
 * the samples stacked along the height (make_grid(nrow=1, padding=0)), one channel repeated to three; clamp != 0: clamp to [-1, 1]
 * first (prepare_to_log; frames_to_u8's clamp: NaN becomes -1); rescale != 0: (x + 1) / 2; then * 255 and truncation toward zero, in
 * the reference's fp32 order: byte-equal.  The byte is defined where -1 < the product < 256 (with the clamp and the rescale: for every
 * value).  An image entry (N, C, H, W) -> (N H, W, 3) is the call with T = 1. */
int mudg_log_sheet(const float* video, uint8_t* out, int N, int C, int T, int H, int W, int clamp, int rescale, void* stream);
int mudg_semantic_nearest(const uint8_t* img, uint8_t* vis, int64_t* labels, int64_t hw, void* stream);

/* ------------------------------------------------------------------ sparse conditions: point splat at virtual poses
 * (data_process/tools/generate_sparse.py:116-223 asks this of OpenGL point sprites; DESIGN.md §12 states the raster rule.)
 * A cloud is n points of 16 bytes: x, y, z fp32 and the colour in the fourth word (r | g << 8 | b << 16).
 * splat_points: every point is projected with each of `poses` matrices (mats[pose][nmat][12] fp32, the top three rows of
 *   w2c (@ transform_obj), row-major; ids == NULL: nmat = 1, else matrix ids[point] of the pose), culled unless
 *   znear < zc < zfar, and every pixel (row j, column i) with u - s/2 <= i + 0.5 < u + s/2 (likewise v, j), s = point_size,
 *   takes the unsigned 64-bit minimum of (bits(zc) << 32 | point index) in keys[pose][H][W], which the caller set to all ones
 *   before the first call (splat_resolve leaves it so).  flags: MUDG_SPLAT_NO_EARLY_REJECT issues the atomic without
 *   looking at the pixel first (measurements).  stats (or NULL): two counters, covered pixels and issued atomics, added to.
 * splat_resolve: keys -> depth (zc of the winner, 0 where nothing landed) and colour (the winner's fourth word, 0 likewise)
 *   over `pixels` = poses * H * W pixels; every key is set to all ones again.  `points` is the cloud the keys index.
 * splat_compose: mask = 13 x 13 box dilation (= three 5 x 5 ones) of all(obj rgb > 0), outside the image unset; colour and
 *   depth are the object's under the mask and the background's elsewhere (obj_* == NULL: the background); then
 *   sparse_frames[pose][c][t][y][x] = (rgb / 255 - 0.5) * 2 and sparse_depth[pose][c][t][y][x] = (clamp(depth, 0, 100) / 100 - 0.5) * 2,
 *   c = 0..2, tensors (3, T, H, W) per pose, pose_stride elements apart.  rgb_out (poses, H, W, 3) uint8, depth_out
 *   (poses, H, W) fp32 and mask_out (poses, H, W) uint8 are optional (NULL). */
#define MUDG_SPLAT_NO_EARLY_REJECT 1
int mudg_splat_points(const void* points, const int32_t* ids, int64_t n, const float* mats, int poses, int nmat,
                      uint64_t* keys, int H, int W, float fx, float fy, float cx, float cy, float znear, float zfar,
                      float point_size, int flags, uint64_t* stats, void* stream);
int mudg_splat_resolve(uint64_t* keys, const void* points, int64_t n, float* depth, uint32_t* colour, int64_t pixels, void* stream);
int mudg_splat_compose(const uint32_t* bg_colour, const float* bg_depth, const uint32_t* obj_colour, const float* obj_depth,
                       float* sparse_frames, float* sparse_depth, int64_t pose_stride, int poses, int T, int t, int H, int W,
                       uint8_t* rgb_out, float* depth_out, uint8_t* mask_out, void* stream);

/* ------------------------------------------------------------------ scene clouds from LiDAR sweeps
 * (data_process/tools/process_lidar.py:27-33, 45-82, 121-138, 229-250; fp64 in a stated order, no output depends on execution order.)
 * cloud_sweep: one launch serves `frames` frames; frame f owns rays offsets[f] .. offsets[f + 1] of rays_o / rays_d (fp32 triples) and
 *   ranges (`total` rays in all, `max_rays` the longest frame).  Device tables of 8-byte words: l2w[frames][12] doubles;
 *   cams[frames][ncam][24] = w2c[12], K[9] doubles, then int64 h, w and the byte offset of the camera's uint8 (h, w, 3) image in
 *   `images` (image_bytes long), ncam <= 8; objs[frames][nobj][16] doubles = w2l[12], the box extents[3], visible (non-zero).
 *   Per ray: p = (R o + t) + (R d) range; colour of the last camera with zc > 0 whose truncated pixel is inside its image; label -1
 *   when no camera sees p, else 1 + the first visible object k with |q.x| < bx / 2, |q.y| < by / 2, -bz / 2 + 0.25 < q.z < bz / 2,
 *   q = w2l p, else 0.  points[ray] = 16 bytes (fp32 q for an object point, p otherwise; r | g << 8 | b << 16), labels[ray] int32.
 * cloud_voxel_keys: keys[i] = (ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20), i_axis = floor(double(p) / voxel); the caller has
 *   checked |i_axis| < 2^20.
 * cloud_voxel_reduce: order[j] = index of the j-th point by key, segments[j] = rank of its voxel (0 .. voxels - 1, non-decreasing);
 *   sums[voxel][8] uint64, zero on entry, receive count, r, g, b, the three fixed-point in-voxel offsets floor((p - i v) / v * 2^32)
 *   clamped to [0, 2^32 - 1], and the key.
 * cloud_voxel_finish: points_out[voxel] = fp32(i v + v (S / (count 2^32))) per axis and (2 S_c + count) / (2 count) per channel. */
int mudg_cloud_sweep(const float* rays_o, const float* rays_d, const float* ranges, const int64_t* offsets, int frames,
                     int64_t max_rays, int64_t total, const double* l2w, const double* cams, int ncam, const double* objs,
                     int nobj, const uint8_t* images, int64_t image_bytes, void* points, int32_t* labels, void* stream);
int mudg_cloud_voxel_keys(const void* points, int64_t n, double voxel, int64_t* keys, void* stream);
int mudg_cloud_voxel_reduce(const void* points, const int64_t* order, const int64_t* segments, int64_t n, double voxel,
                            uint64_t* sums, int64_t voxels, void* stream);
int mudg_cloud_voxel_finish(const uint64_t* sums, int64_t voxels, double voxel, void* points_out, void* stream);

/* ------------------------------------------------------------------ metric depth and lifted views
 * (data_process/depthlab_tools.py:67-87, 114-136; virtual_render/eval_tools.py:137-306; integer sums and fp64 / fp32 operations in a
 * stated order: no output depends on execution order.)  frames_u8 is (frames, H, W, 3) uint8, the depth stream as frames_to_u8
 * writes it; k = r + g + b per pixel, the stream's depth is k / 765.  frames <= 65535 and H W <= 2^24 everywhere.
 * depth_align_sums: sums[frame][5] uint64, zero on entry, receive n, sum k, sum k^2, sum q and sum k q over the pixels with k > 0 and
 *   0 < lidar < 256, q = rint(lidar 2^20) (fp64, half to even), lidar (frames, H, W) fp32 metres.
 * depth_align_solve: the line lidar ~ m (k / 765) + c per frame: den = N Skk - Sk Sk, m' = (N Skq - Sk Sq) / den,
 *   c' = (Sq - m' Sk) / N, coef[frame] = (m' 765 / 2^20, c' / 2^20) fp64, fitted[frame] = 1; n < 2 or den <= 0: (100, 0) and 0.
 * depth_finish: depth[frame][H][W] fp32 = fp32(clip(m (double(k) / 765) + c, 0, 100)), 100 where labels (int64, or NULL: no sky rule)
 *   equals sky_label; vis (frames, H, W, 3) uint8 (or NULL) is the Spectral picture of depth / 100.
 * colormap_spectral: n fp32 values -> bytes (n, 3) uint8 and / or colours (n, 3) fp32 (either may be NULL): x = (x - fp32(val_min)) /
 *   fp32(val_max - val_min) unless the range is (0, 1), pos = clamp(x, 0, 1) 10, left = (int)pos, right = min(left + 1, 10),
 *   d = pos - left, colour = (1 - d) L + d R over the eleven Spectral colours (reversed: the table backwards), byte = (int)(colour 255).
 * depth_unproject: table[frame][16] doubles = the top three rows of camera-to-world, then fx, fy, cx, cy at (H, W).  Pixel (row j,
 *   column i) with depth z: xn = ((i + 0.5) - cx) / fx, yn likewise, p = c2w (xn z, yn z, z); points[frame][j][i] = 16 bytes (fp32 p,
 *   r | g << 8 | b << 16 of rgb (frames, H, W, 3) uint8), valid[frame][j][i] = 1 iff min_depth < z < max_depth and the label is not
 *   sky_label (labels NULL: no sky rule); a pixel that is not valid stores a zero point. */
int mudg_depth_align_sums(const uint8_t* frames_u8, const float* lidar, int frames, int H, int W, uint64_t* sums, void* stream);
int mudg_depth_align_solve(const uint64_t* sums, int frames, double* coef, uint8_t* fitted, void* stream);
int mudg_depth_finish(const uint8_t* frames_u8, const double* coef, const int64_t* labels, int64_t sky_label, int frames, int H,
                      int W, float* depth, uint8_t* vis, void* stream);
int mudg_colormap_spectral(const float* values, int64_t n, double val_min, double val_max, int reversed, uint8_t* bytes,
                           float* colours, void* stream);
int mudg_depth_unproject(const float* depth, const uint8_t* rgb, const int64_t* labels, int64_t sky_label, const double* table,
                         int frames, int H, int W, double min_depth, double max_depth, void* points, uint8_t* valid, void* stream);

/* ------------------------------------------------------------------ scores of generated views
 * (This project's own rules: integer sums and fp64 operations in a stated order, no output depends on execution order.)  Colour frames
 * are (frames, H, W, 3) uint8; frames <= 65535 and H W <= 2^24 everywhere; every output is zero on entry.
 * metric_sse: sse[frame] uint64 receives the sum of (a - b)^2 over all pixels and channels.
 * metric_ssim: Wang et al. 2004 over the valid region (H - 10) x (W - 10), H, W >= 11, per channel: integer window w (eleven taps that sum
 *   to 2^16, see DESIGN), the five moments Sx, Sy, Sxx, Syy, Sxy = sum_ij w_i w_j (x, y, x^2, y^2, x y) as exact integers, then in fp64
 *   mx = Sx / 2^32, vx = Sxx / 2^32 - mx mx, cxy = Sxy / 2^32 - mx my, s = ((2 mx my + C1)(2 cxy + C2)) / ((mx mx + my my + C1)(vx + vy + C2)),
 *   C1 = 6.5025, C2 = 58.5225; sums[frame] int64 receives the sum of rint(s 2^32) (half to even) over valid pixels and channels.
 * metric_depth: depth z and lidar y (frames, H, W) fp32 metres.  A pixel counts iff min_depth < y < max_depth and z is a number; z is
 *   taken into [0, 256]; e = |z - y|, r = e / y, t = max(z / y, y / z) in fp64.  sums[frame][8] int64 receive n, sum rint(e 2^20),
 *   sum rint(e e 2^20), sum rint(r 2^20), the counts of t < 1.25, 1.5625, 1.953125, and one spare that stays zero.
 *   2^-6 <= min_depth < max_depth <= 256.
 * metric_confusion: pred and gt (frames, H, W) int64; confusion[frame][gt][pred] int64 over classes <= 32; a pixel whose gt is outside
 *   [0, classes) is ignored; one whose pred is outside is counted in bad[frame] and in no cell. */
int mudg_metric_sse(const uint8_t* a_u8, const uint8_t* b_u8, int frames, int H, int W, uint64_t* sse, void* stream);
int mudg_metric_ssim(const uint8_t* a_u8, const uint8_t* b_u8, int frames, int H, int W, int64_t* sums, void* stream);
int mudg_metric_depth(const float* depth, const float* lidar, int frames, int H, int W, double min_depth, double max_depth,
                      int64_t* sums, void* stream);
int mudg_metric_confusion(const int64_t* pred, const int64_t* gt, int frames, int H, int W, int classes, int64_t* confusion,
                          int64_t* bad, void* stream);

/* ------------------------------------------------------------------ frames in: camera, depth and label frames to clips
 * (lvdm/data/waymo_data.py:55-412 and virtual_render/data_tools.py:7-215 ask this of cv2.resize on the host, per frame and stream;
 * the rules are this project's, written out in DESIGN §16, and bit-equal to tests/frames_reference.py.)
 * A table has one 16-byte entry per output sample of an axis, made on the host: int32 s0, s1 (the two source indices; nearest reads s0
 * only) and the coefficients of s0 and s1 — int32 that sum to 2048 for the 8-bit rule, fp32 bit patterns w0, w1 for the fp32 rule.
 * xtab has W entries, ytab H.  T, H <= 65535; H0 W0, H W <= 2^28.  A source index outside its axis is clamped to [0, n - 1] before it is
 * used (the coefficients stay): no table sends a load out of the source.
 * resize_u8:  src (T, H0, W0, C) uint8 -> dst (T, H, W, C), C = 1 or 3.  Linear: R = S[x0] a0 + S[x1] a1 per source row in int32,
 *   out = (((b0 (R0 >> 4)) >> 16) + ((b1 (R1 >> 4)) >> 16) + 2) >> 2                    waymo_data.py:80, 92 (INTER_LINEAR)
 *   nearest: out = S[y.s0][x.s0]                                                          waymo_data.py:86 (INTER_NEAREST)
 *   palette != 0 (linear, C = 3): src is (T, H0, W0) class ids and S is the id's colour of the 21 (an id above 20: black), looked up
 *   on the four taps                                                                      data_process/tools/semantic_tools.py:45-73
 * resize_f32: src (T, H0, W0) fp32 -> dst (T, H, W): R = S[x0] w0 + S[x1] w1, out = R0 v0 + R1 v1, every operation rounded on its own.
 * dense_stream: one stream of a clip, three fp32 planes per frame: value (channel c, frame t, row y, column x) goes to
 *   dst + slab stream_stride + (frame0 + t) frame_stride + c channel_stride + y W + x (floats).  kind colour: src (T, H0, W0, 3) uint8,
 *   the 8-bit rule, then norm[v], the caller's 256 values of (v / 255 - 0.5) * 2          waymo_data.py:103, 117
 *   semantic: src (T, H0, W0) ids, the palette form of the 8-bit rule, then norm[v]; depth: src (T, H0, W0) fp32 metres, the fp32
 *   rule, then (clamp(d, 0, 100) / 100 - 0.5) * 2 in that order, the same value in the three channels (norm may be NULL).
 *   u8_out (or NULL; NULL for depth): the resized bytes (T, H, W, 3), what resize_u8 gives. */
#define MUDG_RESIZE_LINEAR 0
#define MUDG_RESIZE_NEAREST 1
#define MUDG_STREAM_COLOUR 0
#define MUDG_STREAM_SEMANTIC 1
#define MUDG_STREAM_DEPTH 2
int mudg_resize_u8(const uint8_t* src, uint8_t* dst, int T, int H0, int W0, int C, int H, int W, int mode, int palette,
                   const int32_t* xtab, const int32_t* ytab, void* stream);
int mudg_resize_f32(const float* src, float* dst, int T, int H0, int W0, int H, int W, const int32_t* xtab, const int32_t* ytab,
                    void* stream);
int mudg_dense_stream(int kind, const void* src, int T, int H0, int W0, int H, int W, const int32_t* xtab, const int32_t* ytab,
                      const float* norm, float* dst, int64_t stream_stride, int64_t channel_stride, int64_t frame_stride, int slab,
                      int frame0, uint8_t* u8_out, void* stream);

/* ------------------------------------------------------------------ surface normals (csrc/normals.hip)
 * The fourth dense modality (lvdm/data/waymo_data.py:194-265, class_label 1000): made from depth, resized into clips, scored.  Every
 * floating-point operation is a single correctly rounded one in the stated order and every sum an integer: results are bit-equal to
 * tests/normals_reference.py and between runs.  OpenCV camera: x right, y down, z forward.
 *
 * depth_normals: depth (frames, H, W) fp32 metres, table[frame][4] doubles = fx, fy, cx, cy at (H, W).  Pixel (row j, column i) with
 *   depth z is usable iff min_depth < z < max_depth and its label is not sky_label (labels NULL: no sky rule); its point is
 *   P = (xn z, yn z, z), xn = ((i + 0.5) - cx) / fx, yn likewise, in fp64.  A neighbour counts iff it is in the frame and usable and, with
 *   max_rel_step = r >= 0, |z_nb - z| <= r z (r < 0: no such test).  dx = P(i+1) - P(i-1) when both horizontal neighbours count, the
 *   difference with P(i) when one does, else none; dy the same along j.  n = dy x dx (a surface seen from the origin has n . P < 0, a
 *   wall facing the camera (0, 0, -1); no flip), len = sqrt((nx nx + ny ny) + nz nz), normals[frame][j][i] = fp32(n / len) and
 *   valid[frame][j][i] = 1; a pixel that is not usable, lacks dx or dy, or has len 0 or not finite stores (0, 0, 0) and 0.
 *   0 <= min_depth < max_depth.
 * normal_stream: src (T, H0, W0, 3) fp32 -> three fp32 planes per frame, placed as dense_stream places them: resize_f32's rule on every
 *   channel with the same tables, no normalisation and no renormalisation to unit length (the maps are "already in [-1, 1]").
 * metric_normals: pred_u8 (frames, H, W, 3) bytes u of a generated stream, gt (frames, H, W, 3) fp32, valid (frames, H, W) bytes or NULL.
 *   p = 2 u - 255 (integers), dot = (p0 g0 + p1 g1) + p2 g2, gg = (g0 g0 + g1 g1) + g2 g2, c = dot / sqrt(double(p . p) gg) in fp64,
 *   clamped to [-1, 1].  A pixel counts iff its validity byte is nonzero, 0 < gg < inf and c is a number; it adds one to
 *   hist[frame][k] (int64, 720 bins of a quarter degree; the caller zeroes them) with cosines[k + 1] < c <= cosines[k], c = -1 in bin
 *   719.  cosines: the caller's 721 doubles cos(k / 4 degrees), descending from 1 to -1.  Integer LDS and 64-bit global atomics only. */
int mudg_depth_normals(const float* depth, const int64_t* labels, int64_t sky_label, const double* table, int frames, int H, int W,
                       double min_depth, double max_depth, double max_rel_step, float* normals, uint8_t* valid, void* stream);
int mudg_normal_stream(const float* src, int T, int H0, int W0, int H, int W, const int32_t* xtab, const int32_t* ytab, float* dst,
                       int64_t stream_stride, int64_t channel_stride, int64_t frame_stride, int slab, int frame0, void* stream);
int mudg_metric_normals(const uint8_t* pred_u8, const float* gt, const uint8_t* valid, const double* cosines, int frames, int H, int W,
                        int64_t* hist, void* stream);

/* ------------------------------------------------------------------ LiDAR depth maps and dense completion (csrc/lidar_depth.hip)
 * The reference's "six_frames_depth" (data_process/pipeline_depth.py:63-152) without Open3D, and the dense depth labels without a learned
 * model.  Results are bit-equal to tests/lidar_depth_reference.py and between runs: the depth test is a 64-bit integer minimum, every
 * other store is a plain one.
 *
 * lidar_splat_visible: the candidates are `nseg` (1 .. 8) runs of a cloud of 16-byte points, segments[2 s] the first point and
 *   segments[2 s + 1] > 0 the length of run s (host memory, read before the call returns).  Each goes through mats[nmat][12] (one pose;
 *   ids as in splat_points, read at the point's place in the cloud) and §12's projection, culling and cover at point_size.  With
 *   occluder_keys (a key image drawn by splat_points from the same candidates, or NULL: no test): home = (floor(v), floor(u)),
 *   near(q) iff q is in the image, its occluder key is not all ones and its depth < fmul(zc, rel_keep), rel_keep = fp32(1 - rel_tol);
 *   the point is hidden iff for one of the directions (0,1), (1,0), (1,1), (1,-1) some pixel home + k d and some pixel home - k' d,
 *   k, k' in 1 .. reach (<= 16), are near.  A hidden point writes nothing; every other one takes the unsigned 64-bit minimum of
 *   (bits(zc) << 32 | index_base + candidate number) in keys[H][W] over its cover.  A candidate's number is its place among the
 *   runs in the order given (a point that two runs name is two candidates).  index_base >= 0 and index_base + candidates <= 2^32:
 *   every index fits the key's low word (no key of a depth in (znear, zfar) is all ones).
 * lidar_depth_resolve: depth = the key's high word as fp32, 0 where the key is all ones; keys, and occluder_keys unless NULL, are
 *   all ones afterwards.
 * depth_complete: depth (frames, H, W) fp32 metres -> out, the same shape.  M = max_depth; a value is empty iff it is < 0.1f.
 *   1  x = M - d where d > 0.1f, else 0; a result that is empty (d within 0.1 of M or beyond, not a number) is 0
 *   2  x = max over the 13 pixels |dj| + |di| <= 2        3  x = max over 5 x 5, then x = min over 5 x 5 (outside the image: empty
 *   for the maxima, absent from the minimum)               4  empty pixels = max over 7 x 7
 *   5  (extrapolate != 0) per column, the rows above the first filled one take its value; then empty pixels = max over 31 x 31
 *   6  x = the 13th smallest of the 5 x 5, border replicated
 *   7  filled pixels = sum(w x) / sum(w) over the filled pixels of the 5 x 5 in the image, w = outer(1 4 6 4 1), exact fp64 sums,
 *      one fp64 division rounded to fp32                   8  out = M - x where filled, else 0
 *   9  labels (frames, H, W) int64 or NULL: out = M where the label is sky_label
 *   source (frames, H, W) bytes or NULL: 4 sky, else 0 where out is empty, else 1 filled after step 1, 2 after step 4, 3 later.
 *   scratch: depth_complete_scratch's bytes (-1: bad shape), 16-byte aligned: 2 round16(4 px) + round16(px), px = frames H W, round16
 *   to the next multiple of 16 (two fp32 maps and a byte map).  What it holds before the call does not matter and nothing outside
 *   those bytes is touched.  depth and out need fp32 alignment only.  1 .. 65535 frames and rows, H W <= 2^24, 0.1 < max_depth <= 65536. */
int mudg_lidar_splat_visible(const void* points, const int32_t* ids, const int64_t* segments, int nseg, const float* mats, int nmat,
                             const uint64_t* occluder_keys, uint64_t* keys, int H, int W, float fx, float fy, float cx, float cy,
                             float znear, float zfar, float point_size, int reach, float rel_keep, int64_t index_base, void* stream);
int mudg_lidar_depth_resolve(uint64_t* keys, uint64_t* occluder_keys, float* depth, int64_t pixels, void* stream);
int64_t mudg_depth_complete_scratch(int frames, int H, int W);
int mudg_depth_complete(const float* depth, const int64_t* labels, int64_t sky_label, int frames, int H, int W, float max_depth,
                        int extrapolate, float* out, uint8_t* source, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ cross-view depth consistency (csrc/consistency.hip)
 * (This project's own rule; the reference merges clouds by concatenation.)  A view is a depth map (H, W) fp32 metres with its camera;
 * 1 .. 65535 views, H W <= 2^24.  fp64 operations in a stated order and integer sums: no output depends on execution order.
 * view_flags: flags[view][H][W] bytes.  Bit 0 (usable) iff min_depth < z < max_depth and the label is not sky_label; bit 1 (dynamic) iff
 *   0 <= label < 64 and bit `label` of dynamic_mask is set.  labels (views, H, W) int64 or NULL: nothing is sky, nothing is dynamic.
 * view_consistency: src_table[view][16] doubles = the top three rows of camera-to-world, then fx, fy, cx, cy at (H, W) (depth_unproject's
 *   table); wit_table[view][16] = the top three rows of world-to-camera, then the same four; times[view] int32; witnesses[view][N]
 *   int32, N in 1 .. 64: -1 is empty, the view itself is skipped, the caller rejects anything else outside 0 .. views - 1 (the kernel
 *   ignores it).  A usable pixel's world point P is depth_unproject's, kept in fp64.  Per witness w in order, skipped when the pixel is
 *   dynamic and times differ: q = w2c_w P by rows ((m0 x + m1 y) + m2 z) + m3; no evidence unless qz > 1e-4; u = fx (qx / qz) + cx,
 *   v likewise; no evidence unless 0 <= u < W and 0 <= v < H (on doubles); over the pixels within r (0 .. 2) of ((int)v, (int)u),
 *   clipped to the image, that are usable (and not dynamic when times differ): d = qz - zw, tol = abs_tol + rel_tol qz; the witness
 *   agrees if some |d| <= tol, violates if at least one pixel counts and every one has d < -tol, else gives no evidence.
 *   agree, violate, keep [view][H][W] bytes: the witnesses with each verdict, and usable && agree >= min_agree && violate <=
 *   max_violate; a pixel that is not usable stores 0, 0, 0.  stats[view][6] uint64 (zero on entry) receives the sums of: usable,
 *   agree + violate > 0, keep, agree, violate, violate > 0. */
int mudg_view_flags(const float* depth, const int64_t* labels, int64_t sky_label, uint64_t dynamic_mask, int views, int H, int W,
                    double min_depth, double max_depth, uint8_t* flags, void* stream);
int mudg_view_consistency(const float* depth, const uint8_t* flags, const double* src_table, const double* wit_table,
                          const int32_t* times, const int32_t* witnesses, int views, int N, int H, int W, int r, int min_agree,
                          int max_violate, double rel_tol, double abs_tol, uint8_t* agree, uint8_t* violate, uint8_t* keep,
                          uint64_t* stats, void* stream);

/* ------------------------------------------------------------------ neighbour search between clouds (csrc/neighbours.hip)
 * The reference's pipeline takes radius outlier removal from open3d; the rule here is this project's own: brute force within r, found
 * through a grid.  Points are §12's packed 16 bytes.  r in (0, 64], r2 = r r, cell = r (1 + 2^-10), all doubles formed by the caller;
 * a point's cell is floor(double(p) / cell) per axis and its key cloud_voxel_keys' at voxel = cell.  ref_sorted: the n reference points
 * in ascending key order (|cell index| <= 2^20 - 2, checked by the caller); keys: their keys; order: each one's original index.
 * visit (or NULL): a permutation of 0 .. nq - 1, the order in which lanes take the queries (by cell, so that a wave's candidates share
 * cache lines); results are stored at the query's own position.  A query's candidates are the nine key intervals (ix + a, iy + b,
 * iz - 1 .. iz + 1); p is within reach iff d2 = ((dx dx + dy dy) + dz dz) <= r2 in fp64, d = double(q) - double(p).  A query with a
 * coordinate that is not finite, or with |q / cell| >= 2^20 + 1, finds nothing.
 * cloud_nearest: d2[q] = the smallest d2 within reach (+inf: none), index[q] = the lowest original index that attains it (-1: none).
 * cloud_count: counts[q] = min(points within reach, cap), cap >= 1.
 * metric_cloud: n < 2^31 such d2 values and K <= 8 squared thresholds t2 (host memory, 0 < t2[k] <= r2) -> sums[2 + K] int64 (zero on
 *   entry) receive the number of finite values, the sum over them of floor(sqrt(d2) 2^20) (d2 taken into [0, r2]), and the counts of
 *   d2 <= t2[k]. */
int mudg_cloud_nearest(const void* ref_sorted, const int64_t* keys, const int64_t* order, int64_t n, const void* queries,
                       const int64_t* visit, int64_t nq, double cell, double r2, double* d2, int64_t* index, void* stream);
int mudg_cloud_count(const void* ref_sorted, const int64_t* keys, const int64_t* order, int64_t n, const void* queries,
                     const int64_t* visit, int64_t nq, double cell, double r2, int cap, int32_t* counts, void* stream);
int mudg_metric_cloud(const double* d2, int64_t n, const double* t2_host, int K, double r2, int64_t* sums, void* stream);

/* ------------------------------------------------------------------ clouds as 3D Gaussians (csrc/gaussians.hip)
 * The forward half of a tile-binned Gaussian splat renderer.  A Gaussian is a packed point of §12, six fp32 covariance entries
 * (xx, xy, xz, yy, yz, zz) in the point's own frame, an fp32 opacity and a matrix id (clamped to 0 .. nmat - 1; ids NULL: nmat = 1).
 * A call draws V views: mats (V, nmat, 12) fp32 as in mudg_splat_points, one camera fx, fy, cx, cy, pixel centres at i + 0.5.  Tiles are
 * 16 x 16 pixels, TX = ceil(W / 16), TY = ceil(H / 16), NT = TX TY, V NT < 2^31.  Every operation is a single rounded fp32 one in the
 * order written (division and root correctly rounded); min / max return the operand that is a number.  Every entry returns MUDG_EINVAL
 * before any launch for null arguments, unaligned points, n, V, nmat, H or W <= 0, V NT >= 2^31, E outside 1 .. 2^31 - 1, more
 * workgroups than a grid holds, and znear, zfar that are not finite with 0 < znear < zfar.
 *
 * project, a lane per Gaussian, all V views:
 *   xc, yc, zc = ((m0 x + m1 y) + m2 z) + m3 per row; dropped unless znear < zc < zfar
 *   u = fx (xc / zc) + cx, v = fy (yc / zc) + cy
 *   limx = 1.3 (0.5 W / fx), tx = min(limx, max(-limx, xc / zc)) zc; likewise limy, ty
 *   j00 = fx / zc, j02 = -(fx tx) / (zc zc), j11 = fy / zc, j12 = -(fy ty) / (zc zc)
 *   T0k = j00 R0k + j02 R2k, T1k = j11 R1k + j12 R2k with R = M[:, :3];  Vrk = (Tr0 S0k + Tr1 S1k) + Tr2 S2k
 *   a = ((V00 T00 + V01 T01) + V02 T02) + 0.3, b = (V00 T10 + V01 T11) + V02 T12, c = ((V10 T10 + V11 T11) + V12 T12) + 0.3
 *   det = a c - b b, dropped unless 0 < det < inf;  A = c / det, B = -b / det, C = a / det
 *   mid = 0.5 (a + c), lam = mid + sqrt(max(0.1, mid mid - det)), rad = ceil(3 sqrt(lam)); dropped unless rad <= 4096
 *   dropped unless 1 / 255 <= opacity < inf
 *   x0 = clamp(floor((u - rad) / 16), 0, TX), x1 = clamp(floor((u + rad) / 16) + 1, 0, TX) in fp32, then converted; likewise y0, y1
 *   count = (x1 - x0)(y1 - y0), dropped if 0
 *   outputs per (view, Gaussian): uv (V, n, 2), conic (V, n, 4) = (A, B, C, opacity), depth (V, n) = zc, rect (V, n, 4) =
 *   (x0, x1, y0, y1), count (V, n); all zero where dropped.  conic and rect 16-byte aligned, uv 8-byte aligned.
 * keys, a lane per (view, Gaussian): offsets (V n) int64 = the exclusive sum of count, E its total; tile k of the rectangle in
 *   row-major order writes keys[offsets + k] = (view NT + tile) << 32 | bits(zc) and values[offsets + k] = the Gaussian's index.  A
 *   rectangle outside the tile grid, a count that is not its rectangle's or an offset outside [0, E - count] writes nothing.
 * ranges, a lane per entry of the keys sorted ascending: ranges (tiles = V NT, 2) int32 is zeroed by the call; where an entry's tile
 *   differs from its predecessor's (or it is the first) ranges[tile][0] = e, from its successor's (or it is the last) ranges[tile][1] =
 *   e + 1.  Plain stores; a tile outside 0 .. tiles - 1 is ignored.
 * blend, a workgroup of 256 lanes per (view, tile), a lane per pixel (px, py) = (i + 0.5, j + 0.5); pixels outside the image store
 *   nothing.  T = 1, Ck = 0, D = 0; the tile's entries in sorted order (staged through LDS 256 at a time; the workgroup leaves at a
 *   batch's start once every pixel is done):
 *     dx = u - px, dy = v - py, q = (A dx) dx + (C dy) dy, p = (-0.5 q) - (B dx) dy; skipped if p > 0 or p < -5.55
 *     g = E(p): t = p 1.44269504f, n = floor(t), f = t - n, Horner over f (a multiply, then an add per step) with 0x1.f06faep-10,
 *       0x1.25429cp-7, 0x1.c99b9ep-5, 0x1.ebcf7ap-3, 0x1.62e526p-1, 1; g = ldexp(poly, n)
 *     alpha = min(0.99, opacity g); skipped if alpha < 1 / 255
 *     Tn = T (1 - alpha); Tn < 1e-4: the pixel is done, the entry is not added
 *     w = alpha T, Ck += float(byte k) w, D += zc w, T = Tn
 *   rgb (V, 3, H, W) = Ck / 255, depth_out (V, H, W) = D, alpha (V, H, W) = 1 - T.  A range outside [0, E] is empty, a sorted value
 *   outside 0 .. n - 1 an entry of opacity 0.  walked (V NT) int32 or NULL: the entries each workgroup staged (tools). */
int mudg_gauss_project(const void* points, const float* cov, const float* opacity, const int32_t* ids, int64_t n, const float* mats,
                       int V, int nmat, int H, int W, float fx, float fy, float cx, float cy, float znear, float zfar, float* uv,
                       float* conic, float* depth, int32_t* rect, int32_t* count, void* stream);
int mudg_gauss_keys(const float* depth, const int32_t* rect, const int32_t* count, const int64_t* offsets, int64_t n, int V, int H,
                    int W, int64_t E, int64_t* keys, int32_t* values, void* stream);
int mudg_gauss_ranges(const int64_t* keys_sorted, int64_t E, int64_t tiles, int32_t* ranges, void* stream);
int mudg_gauss_blend(const void* points, const float* uv, const float* conic, const float* depth, const int32_t* values_sorted,
                     const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, float* rgb, float* depth_out, float* alpha,
                     int32_t* walked, void* stream);

/* ------------------------------------------------------------------ fitting Gaussians to images (csrc/gaussians_bwd.hip)
 * The training half of the renderer above: the same tiles, entries, operations and refusals; colour (n, 3) fp32 in byte units takes the
 * place of the packed colour word.  project, keys and ranges are reused as they are.
 * blend_train: mudg_gauss_blend with float(byte k) replaced by colour[g][k]; besides rgb, depth_out and alpha it stores state
 *   (V, 5, H, W) = (C0, C1, C2, D, T), the accumulators before rgb = C / 255 and alpha = 1 - T round them.
 * blend_bwd: order (E) int64 is the sort's permutation (sorted entry e was unsorted entry order[e]); partial (E, 10) fp32 is zeroed by
 *   the call.  A workgroup per (view, tile) walks the tile's entries front to back and recomputes dx, dy, p, g, alpha, Tn, w and the
 *   accumulators with the forward's operations, so the skips and the stopping entry are the forward's.  Per pixel gCk = d_rgb[k] / 255,
 *   gD = d_depth, gAT = d_alpha state[4].  For an entry the pixel blends, with Ck, D the accumulators after adding it:
 *     r0..2 = gCk w, r3 = gD w
 *     unless opacity g > 0.99 (then r4..9 = 0):
 *       own = ((gC0 c0 + gC1 c1) + gC2 c2) + gD zc, behind = ((gC0 (state0 - C0) + gC1 (state1 - C1)) + gC2 (state2 - C2)) + gD (state3 - D)
 *       dal = (T own - behind / (1 - alpha)) + gAT / (1 - alpha), r4 = dal g, dp = (dal opacity) g
 *       r5 = dp (-0.5 (dx dx)), r6 = dp (-(dx dy)), r7 = dp (-0.5 (dy dy)), r8 = dp (-(A dx + B dy)), r9 = dp (-(C dy + B dx))
 *   every other lane has r = +0.  The 256 lanes' r are added by an xor butterfly over 1, 2, 4, 8, 16, 32 inside each wave of 64 and
 *   the four waves as ((w0 + w1) + w2) + w3, and stored plainly at partial[order[e]]; an order value outside 0 .. E - 1 stores nothing.
 * project_bwd, a lane per Gaussian, views in order; a view with count 0, an offset outside [0, E - count] or zc outside the depth range
 *   adds nothing.  acc = the count partials at offsets + k added in ascending k; d_colour += acc0..2, d_opacity += acc4; the chain rule
 *   through project's steps as DESIGN §24 writes it gives d_xyz (n, 3) in the point's own frame and d_cov (n, 6), the off-diagonal
 *   entries with both symmetric halves.  A clamped tx or ty passes nothing through xc / zc; rad, the rectangle and 0.3 are constants. */
int mudg_gauss_blend_train(const float* colour, const float* uv, const float* conic, const float* depth, const int32_t* values_sorted,
                           const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, float* rgb, float* depth_out, float* alpha,
                           float* state, void* stream);
int mudg_gauss_blend_bwd(const float* colour, const float* uv, const float* conic, const float* depth, const int32_t* values_sorted,
                         const int64_t* order, const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, const float* state,
                         const float* d_rgb, const float* d_depth, const float* d_alpha, float* partial, void* stream);
int mudg_gauss_project_bwd(const void* points, const float* cov, const int32_t* ids, int64_t n, const float* mats, int V, int nmat, int H,
                           int W, float fx, float fy, float cx, float cy, float znear, float zfar, const int32_t* count,
                           const int64_t* offsets, const float* partial, int64_t E, float* d_xyz, float* d_cov, float* d_opacity,
                           float* d_colour, void* stream);

/* ------------------------------------------------------------------ view-dependent colour (csrc/gaussians_sh.hip)
 * Real spherical harmonics of degrees 1 .. L (L = degree = 1, 2 or 3; K = (L + 1)^2) on top of colour (n, 3), the direction-independent
 * term in byte units with the degree-0 constant folded in.  sh (n, K - 1, 3) fp32, row-major, 16-byte aligned, in byte units; order, signs
 * and constants are the 3DGS code's, the constants rounded once to fp32.  points, ids, mats, count: what mudg_gauss_project takes and
 * writes.  active (0 .. L) cuts the sum at Ka = (active + 1)^2.  Single rounded fp32 operations in the order DESIGN §27 writes them.
 * sh_colour, a lane per (view, Gaussian): where count[v][g] <= 0 the colour is +0 and nothing of the Gaussian is read.  Otherwise, with
 *   m = mats[v][id], c_j = -((m[j] m[3] + m[4 + j] m[7]) + m[8 + j] m[11]), w = p - c, len = sqrt((wx wx + wy wy) + wz wz), d = w / len:
 *   a = colour[g]; a += B_k(d) sh[g][k - 1] for k = 1 .. Ka - 1 in order; colours[v][g] = a < 0 ? +0 : a.  colours is (V, n, 3).  V <= 65535.
 * sh_bwd, a lane per Gaussian, views in order; partial (E, 10), count and offsets as mudg_gauss_project_bwd reads them, with its guards.
 *   Per counted view: g = columns 0 .. 2 of the partials added in ascending order from +0; the forward's d, B and a again; ge = a < 0 ?
 *   +0 : g per channel; d_colour += ge; d_sh[k - 1] += B_k ge for k < Ka; s_k = (ge0 sh0 + ge1 sh1) + ge2 sh2 for k < Ka, +0 above;
 *   gd = sum_k s_k dB_k/dd as DESIGN §27 orders its terms; dot = (dx gdx + dy gdy) + dz gdz; d_xyz_dir += (gd - d dot) / len.  d_colour
 *   (n, 3), d_sh (n, K - 1, 3) (16-byte aligned; +0 at and above Ka) and d_xyz_dir (n, 3), in the Gaussian's own frame, are written in
 *   full with plain stores.
 * blend_views, blend_train_views, blend_bwd_views: mudg_gauss_blend_train (the first without state) and mudg_gauss_blend_bwd with
 *   colours (V, n, 3), an entry of view v and Gaussian g taking colours[v][g]; everything else, refusals included, is theirs. */
int mudg_gauss_sh_colour(const void* points, const int32_t* ids, int64_t n, const float* mats, int V, int nmat, const int32_t* count,
                         const float* colour, const float* sh, int degree, int active, float* colours, void* stream);
int mudg_gauss_sh_bwd(const void* points, const int32_t* ids, int64_t n, const float* mats, int V, int nmat, const int32_t* count,
                      const int64_t* offsets, const float* partial, int64_t E, const float* colour, const float* sh, int degree, int active,
                      float* d_colour, float* d_sh, float* d_xyz_dir, void* stream);
int mudg_gauss_blend_views(const float* colours, const float* uv, const float* conic, const float* depth, const int32_t* values_sorted,
                           const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, float* rgb, float* depth_out, float* alpha,
                           void* stream);
int mudg_gauss_blend_train_views(const float* colours, const float* uv, const float* conic, const float* depth, const int32_t* values_sorted,
                                 const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, float* rgb, float* depth_out, float* alpha,
                                 float* state, void* stream);
int mudg_gauss_blend_bwd_views(const float* colours, const float* uv, const float* conic, const float* depth, const int32_t* values_sorted,
                               const int64_t* order, const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W, const float* state,
                               const float* d_rgb, const float* d_depth, const float* d_alpha, float* partial, void* stream);

/* ------------------------------------------------------------------ pose gradients (csrc/gaussians_pose.hip, gaussians_sh.hip)
 * The gradient of mats (V, nmat, 12): d_mats (V, nmat, 12) fp32, every element overwritten.  points, cov, ids, mats, the camera, count,
 * offsets, partial and E are what mudg_gauss_project_bwd (pose_bwd) and mudg_gauss_sh_bwd (sh_pose_bwd) take, with their guards and
 * refusals; V <= 65535.  stage: caller-allocated scratch of V nmat ceil(n / 256) 12 floats, cleared by the call.
 * pose_bwd, a lane per (view, Gaussian).  Where project_bwd counts the pair, with m = mats[v][id] (id clamped), p the position and dxc,
 *   dyc, dzc, dt0, dt1 project_bwd's chain quantities:
 *     g[3] = dxc, g[7] = dyc, g[11] = dzc; for k = 0, 1, 2: g[k] = dxc p[k] + dt0[k] j00, g[4 + k] = dyc p[k] + dt1[k] j11,
 *     g[8 + k] = dzc p[k] + (dt0[k] j02 + dt1[k] j12)
 * sh_pose_bwd, likewise: with dv the view's addend to mudg_gauss_sh_bwd's d_xyz_dir, for r = 0, 1, 2:
 *     g[4r + k] = dv[k] m[4r + 3], g[4r + 3] = (dv[0] m[4r] + dv[1] m[4r + 1]) + dv[2] m[4r + 2]
 * The sum over the Gaussians of one (view, matrix), the same in both: chunks of 256 consecutive Gaussians; in a chunk a lane that holds
 *   another id, is not counted or lies past n adds +0; the 256 values are added by the xor butterfly over 1 .. 32 inside each wave and the
 *   four waves as ((w0 + w1) + w2) + w3.  Then lane l of a finishing workgroup adds the sums of chunks l, l + 256, ... in ascending order
 *   from +0, and the 256 lane sums are added in the same butterfly-and-waves order.  A matrix nobody goes through gets twelve +0.  No atomics. */
int mudg_gauss_pose_bwd(const void* points, const float* cov, const int32_t* ids, int64_t n, const float* mats, int V, int nmat, int H, int W,
                        float fx, float fy, float cx, float cy, float znear, float zfar, const int32_t* count, const int64_t* offsets,
                        const float* partial, int64_t E, float* stage, float* d_mats, void* stream);
int mudg_gauss_sh_pose_bwd(const void* points, const int32_t* ids, int64_t n, const float* mats, int V, int nmat, const int32_t* count,
                           const int64_t* offsets, const float* partial, int64_t E, const float* colour, const float* sh, int degree,
                           int active, float* stage, float* d_mats_dir, void* stream);

/* ------------------------------------------------------------------ density control for the fit (csrc/gaussians_density.hip)
 * Which Gaussians a fit clones, splits and prunes, and the pass that rewrites the parameters.  fp32, single rounded operations in the
 * order written, a lane per Gaussian, plain stores, no atomics, no generator state, no transcendental.
 * accumulate: partial (E, 10), count (V, n) and offsets (V, n) are what mudg_gauss_project_bwd reads, with its guards: a view with
 *   count <= 0 or an offset outside [0, E - count] adds nothing.  Otherwise su, sv = columns 8, 9 of the count partials added in ascending
 *   k from +0; a = (0.5 W) su, b = (0.5 H) sv; grad_sum[g] += sqrt(a a + b b) (the gradient norm in [-1, 1] screen units), seen[g] += 1.
 *   The views are taken in order; grad_sum (n) fp32 and seen (n) int32 are updated in place.
 * plan: opacity (n) and scale (n, 3) = exp(log_scale) come evaluated.  smax = max(max(s0, s1), s2).  action (n) / rows (n) int32:
 *   1 / 0 (prune) if grad_sum, opacity or a scale is not a number, opacity < min_opacity or smax > max_scale; else, if grow != 0,
 *   seen > 0 and grad_sum / float(seen) >= grad_threshold: 3 / 2 (split) if smax > split_scale, 2 / 2 (clone) if not; else 0 / 1 (keep).
 * apply: start (n) int64 is the exclusive sum of rows and n_out its total.  src and dst are host arrays of 15 device pointers, read
 *   before the call returns: tensor 3 p + k is parameter p of (xyz (n, 3), colour (n, 3), log_scale (n, 3), quat (n, 4), opacity_logit (n))
 *   for k = 0, its first Adam moment for k = 1 and its second for k = 2; dst has n_out rows.  Keep copies the row and its moments to
 *   start[g]; clone writes that row and then the same row with zero moments; split writes two rows with zero moments, xyz +- d axis and
 *   log_scale - log_shrink, where k is the first index of the largest scale, axis column k of rot (n, 9) (row-major 3 x 3) and
 *   d = split_offset scale[k]; ids (n) is copied to ids_out (n_out) when both are given.  An action outside 0 .. 3 is a prune; a start
 *   outside [0, n_out - rows] stores nothing. */
int mudg_gauss_density_accumulate(const float* partial, const int32_t* count, const int64_t* offsets, int64_t n, int V, int H, int W,
                                  int64_t E, float* grad_sum, int32_t* seen, void* stream);
int mudg_gauss_density_plan(const float* grad_sum, const int32_t* seen, const float* opacity, const float* scale, int64_t n,
                            float grad_threshold, float split_scale, float min_opacity, float max_scale, int grow, int32_t* action,
                            int32_t* rows, void* stream);
int mudg_gauss_density_apply(const int32_t* action, const int64_t* start, int64_t n, int64_t n_out, const float* scale, const float* rot,
                             float split_offset, float log_shrink, const float* const* src, float* const* dst, const int32_t* ids,
                             int32_t* ids_out, void* stream);

/* The image loss of the fit (csrc/gaussians_loss.hip): (1 - l) mean|x - y| + l (1 - mean S) + depth_weight times the mean
 * of |d - dt| over the pixels with dt > 0, with l = ssim_weight.  rgb and targets (V, 3, H, W), depth and depth_targets (V, H, W) or both
 * null: fp32.  S is SSIM per pixel and channel with the 11-tap window mudg_ssim's taps / 65536, zero padding, C1 = 0.01^2, C2 = 0.03^2,
 * every operation a single rounded fp32 one in the order §26 states.  NT = ceil(W / 16) ceil(H / 16).
 * loss: maps (V, 3, 3, H, W) = dS/da, dS/db, dS/dc of every pixel (a = w*x, b = w*(x x), c = w*(x y)); partial (V, 3, NT, 4): the
 *   tile's sum |x - y|, sum S, and in channel 0 the depth sum and the depth count (an int32 in the fourth word; +0.0 and 0 elsewhere).
 * finish: adds the partials in a fixed order (fp64, the count in int64) into totals (8): the loss, mean |x - y|, mean S, the depth
 *   mean, float(max(count, 1)), the count as int32 (saturated), 0, 0.
 * bwd: upstream (1) is the gradient of the loss, on the device.  d_rgb (V, 3, H, W) = upstream ((1 - l) / N sgn(x - y) - l / N dSum S / dx),
 *   N = 3 V H W; d_depth (V, H, W), or null = upstream depth_weight / totals[4] sgn(d - dt) [dt > 0].  maps and totals are the outputs above.
 * Refused: null or unaligned pointers, exactly one of depth / depth_targets, d_depth without depth, V, H or W <= 0, V NT >= 2^31,
 * 3 V NT workgroups beyond a grid, ssim_weight outside [0, 1], a negative or non-finite depth_weight. */
int mudg_gauss_loss(const float* rgb, const float* targets, const float* depth, const float* depth_targets, int V, int H, int W, float* maps,
                    float* partial, void* stream);
int mudg_gauss_loss_finish(const float* partial, int V, int H, int W, float ssim_weight, float depth_weight, float* totals, void* stream);
int mudg_gauss_loss_bwd(const float* rgb, const float* targets, const float* maps, const float* depth, const float* depth_targets,
                        const float* totals, const float* upstream, int V, int H, int W, float ssim_weight, float depth_weight, float* d_rgb,
                        float* d_depth, void* stream);

/* ------------------------------------------------------------------ semantic Gaussians (csrc/gaussians_feat.hip)
 * Every Gaussian carries feat (n, F) fp32, row-major and unpadded, 1 <= F <= 32: class scores blended with the colours in the same walk.
 * colours: (n, 3) with colour_views = 0, (V, n, 3) with colour_views = 1, fp32 in byte units.  fp32 throughout, every operation a single
 * rounded one in the order §29 states, E(p) §23's polynomial exponential; plain stores, no atomics; a repeat run gives the same bits.
 * blend_feat: mudg_gauss_blend_train (colour_views = 1: mudg_gauss_blend_train_views) with one more line per blended entry,
 *   Fk = Fk + feat[g][k] w for k < F.  rgb, depth_out, alpha and state (V, 5, H, W; NULL for inference) are that call's bits on the same
 *   inputs; feat_out (V, F, H, W) = Fk, unrounded and undivided.  A sorted value outside 0 .. n - 1 is an entry of opacity 0 and reads
 *   no feature row.
 * blend_bwd_feat: mudg_gauss_blend_bwd's walk with the forward recomputed bit for bit.  Per pixel gF_k = d_feat[k] (d_feat (V, F, H, W)),
 *   Stot = sum_k gF_k feat_out[k], P = +0.  Per blended entry s = sum_k gF_k feat[g][k], P = P + s w, own = (§24's own) + s,
 *   behind = (§24's behind) + (Stot - P), the ten sums from own and behind as §24 computes them, and q_k = gF_k w.  Sums over k run
 *   ascending from +0.  The ten sums go to partial (E, 10) and q to partial_feat (E, F) at row order[e], reduced over the tile's pixels
 *   in §24's order; both buffers are zeroed by the call.  With d_feat = 0 partial has mudg_gauss_blend_bwd's values.
 * feat_bwd: d_feat_g (n, F): per Gaussian and channel, per view (ascending) the count[view][g] rows of partial_feat from
 *   offsets[view][g] added in ascending order from +0 (nothing where count <= 0 or the offset lies outside [0, E - count]), the views'
 *   sums added in view order from +0.
 * class_loss: x (V, F, H, W) fp32, labels (V, H, W) uint8; a pixel is labelled iff label < F.  Labelled: m = max_k x_k (fmaxf, ascending),
 *   p_k = fmaxf(x_k - m, -80), e_k = E(p_k), S = sum_k e_k, maps[k] = e_k / S - [k == label], l = L(S) - p_label with L §29's polynomial
 *   logarithm on [1, 32]; unlabelled: maps = +0, l = +0.  maps (V, F, H, W); partial (V NT, 2): each 16 x 16 tile's sum of l in the
 *   tile's fixed order and its labelled count (an int32 in the second word).
 * class_loss_finish: adds the tiles in a fixed order (fp64, the count in int64) into totals (4): sum l, the count as int32
 *   (saturated), float(max(count, 1)), and the loss weight (sum l / max(count, 1)).
 * class_loss_bwd: d_x (V, F, H, W) = ((up weight) / totals[2]) maps; up (1) is the loss's gradient, on the device.
 * Refused before any launch: what mudg_gauss_blend_train / mudg_gauss_blend_bwd / mudg_gauss_loss refuse, and F outside 1 .. 32,
 *   colour_views outside {0, 1}, null feat / feat_out / d_feat / partial_feat, E F >= 2^31, a negative or non-finite weight. */
int mudg_gauss_blend_feat(const float* colours, int colour_views, const float* feat, int F, const float* uv, const float* conic,
                          const float* depth, const int32_t* values_sorted, const int32_t* ranges, int64_t n, int64_t E, int V, int H, int W,
                          float* rgb, float* depth_out, float* alpha, float* feat_out, float* state, void* stream);
int mudg_gauss_blend_bwd_feat(const float* colours, int colour_views, const float* feat, int F, const float* uv, const float* conic,
                              const float* depth, const int32_t* values_sorted, const int64_t* order, const int32_t* ranges, int64_t n,
                              int64_t E, int V, int H, int W, const float* state, const float* feat_out, const float* d_rgb,
                              const float* d_depth, const float* d_alpha, const float* d_feat, float* partial, float* partial_feat,
                              void* stream);
int mudg_gauss_feat_bwd(const int32_t* count, const int64_t* offsets, const float* partial_feat, int64_t E, int64_t n, int V, int F,
                        float* d_feat_g, void* stream);
int mudg_gauss_class_loss(const float* x, const uint8_t* labels, int V, int F, int H, int W, float* maps, float* partial, void* stream);
int mudg_gauss_class_loss_finish(const float* partial, int V, int H, int W, float weight, float* totals, void* stream);
int mudg_gauss_class_loss_bwd(const float* maps, const float* totals, const float* up, float weight, int V, int F, int H, int W, float* d_x,
                              void* stream);

/* ------------------------------------------------------------------ the image tower (csrc/towers.hip)
 * Reference: lvdm/modules/encoders/condition.py:295-372 (FrozenOpenCLIPImageEmbedderV2): a pre-LN ViT whose GEMMs run on mudg_gemm;
 * these entries are what it needs besides.
 *
 * short_attention: softmax(scale Q K^T) V over a short sequence, every key (then every value) of one (image, head) in LDS.
 *   q, k and v are rounded once to operand storage while they are staged (the bits mudg_gemm would have stored with out_fp32 = 0);
 *   scores accumulate in fp32; one pass with the exact row maximum m: p_j = 2^(c s_j - c m), c = scale log2(e), key columns >= N
 *   masked; l = sum_j p_j in fp32; P passes through operand storage; O = (P V) / l, rounded once.  No atomics: a repeat run is
 *   bit-equal.  16-bit builds: MFMA 32x32x16 (d = 80 is five K = 16 steps, no padding of d for the scores; the value rows of P V are
 *   padded 80 -> 96); split builds: fp32 on the vector unit from the operand-rounded values. */
typedef struct MudgShortAttnDesc {
    const float* QKV;   /* fp32 rows [B N][ldqkv]: q of head h at columns [h d, h d + d), k at C + h d, v at 2 C + h d, C = heads d
                           (the fused in_proj GEMM's output with out_fp32 = 1) */
    void* O;            /* MFMA-operand rows [B N][ldo] in the build's operand layout, head h at [h d, h d + d) */
    int B, heads, N, d;
    int64_t ldqkv, ldo;
    float scale;        /* d^-0.5 */
} MudgShortAttnDesc;
/* 1 when the call below would run, reading nothing: d = 64 or 80, 1 <= N <= 288, ldqkv >= 3 C, ldo a multiple of 8 * PLANES with
 * ldo / PLANES >= C, B and heads positive (B <= 65535); else 0 with the reason as the error text.  The call itself also needs
 * non-null pointers and a 16-byte aligned O, and returns MUDG_EINVAL before any launch otherwise. */
int mudg_short_attention_ok(const MudgShortAttnDesc* d);
int mudg_short_attention(const MudgShortAttnDesc* d, void* stream);
/* LayerNorm over the last dim with an fp32 result (ln_pre: its output is the tower's residual stream): the arithmetic of
 * mudg_layernorm on fp32 rows, without the operand rounding of the store.  Row strides in elements. */
int mudg_layernorm_f32(const float* X, int64_t ldx, const float* gamma, const float* beta, float* Y, int64_t ldy, int rows, int C,
                       float eps, void* stream);
/* clip_preprocess: src (B, 3, H, W) fp32 in [-1, 1] -> the 224 x 224 CLIP input as the patch matrix of the 14 x 14 / stride 14
 *   convolution: operand rows patches[B 256][ldp], row (b, 16 gy + gx), column c 196 + 14 py + px (conv1.weight.reshape(width, 588)'s
 *   order), columns 588 .. 591 zero (ldp / PLANES >= 592); image (or NULL): the fp32 (B, 3, 224, 224) image itself.
 *   Rule: optional separable Gaussian blur (taps gx[kx] along x first, then gy[ky] along y, reflect border without the
 *   edge; ky = kx = 0: none), bicubic sample (xtab / ytab: per destination index four source indices and the fp32 bits of four
 *   coefficients, 8 int32, x taps summed first), (v + 1) * 0.5, - mean_c, / std_c.  Every operation is a single rounded fp32 one,
 *   sums run left to right from the first tap; the tables come from the host and every index is clamped before its load. */
int mudg_clip_preprocess(const float* src, int B, int H, int W, const int32_t* ytab, const int32_t* xtab, const float* gy, int ky,
                         const float* gx, int kx, void* patches, int64_t ldp, float* image, void* stream);

/* ------------------------------------------------------------------ training step
 * Reference: lvdm/models/ddpm3d.py:741-802 (p_losses), :1267-1300 (configure_optimizers -> torch.optim.AdamW),
 * main/utils_train.py:126-137 (data-parallel strategy).  The contractions of the backward pass (dX = dY W, dW = dY^T X,
 * conv / temporal-conv input gradients) run on mudg_gemm; these entries are everything else the backward pass needs.
 * Gradients and the training stream are fp32 rows matrices (row strides in elements).  Fixed-order reductions throughout. */
/* dst[c][p] = src[srcrow(p)][c] as an MFMA operand matrix [C][ldd] (ldd / PLANES >= P rounded up to 8; the tail columns are
 * zeroed): the transposed (and, for convolutions, tap-shifted) operand copies that weight-gradient GEMMs contract over.
 * mode 0: srcrow = p.  mode 1 (3x3 conv tap (dy, dx)): p = (f, oy, ox) on the Hout x Wout grid reads input pixel
 * (oy stride - pad + dy, ox stride - pad + dx) of the Hin x Win image, zero outside.  mode 2 (temporal tap dt): p = ((b T + t) HW + s)
 * reads row p + (dt - 1) HW while 0 <= t + dt - 1 < T. */
int mudg_transpose_gather(const float* src, int64_t lds, void* dst, int64_t ldd, int64_t P, int C, int mode, int Hin, int Win,
                          int Hout, int Wout, int stride, int pad, int dy, int dx, int T, int HW, int dt, int batch,
                          int64_t src_batch_stride, int64_t dst_batch_stride, void* stream);
/* batch > 1: entry z reads src + z * src_batch_stride and writes dst + z * dst_batch_stride (elements): the per-(frame, head)
 * transposes of the attention backward pass in one launch. */
/* out[g][c] = sum over the rows of group g (rows_per_group consecutive rows) of A[r][c] * (B ? B[r][c] : 1): bias gradients
 * (one group), the timestep-embedding gradient of a ResBlock (one group per clip). */
int mudg_group_colsum(const float* A, int64_t lda, const float* B, int64_t ldb, int64_t rows, int cols, int64_t rows_per_group,
                      float* out, void* stream);
/* GroupNorm (+SiLU) backward.  stat = (mean, rstd) per (sample, group) (mudg_groupnorm_stats of the same X); writes dX and
 * AB[sample][c] = (sum dz, sum dz xhat): dbeta / dgamma are its sums over the samples.  ws: mudg_groupnorm_bwd_ws_floats. */
int64_t mudg_groupnorm_bwd_ws_floats(int samples, int rows, int C, int groups);
int mudg_groupnorm_stats(const float* X, int64_t ldx, int samples, int rows, int C, int groups, float eps, float* stat, void* stream);
int mudg_groupnorm_bwd(const float* X, int64_t ldx, const float* dY, int64_t ldy, const float* gamma, const float* beta,
                       const float* stat, int samples, int rows, int C, int groups, int silu, float* dX, int64_t lddx, float* AB,
                       float* ws, const float* dres, int64_t lddres, void* stream);
/* LayerNorm backward: dX, and part[chunks][2][C] (chunks = mudg_layernorm_bwd_chunks(rows)): per chunk of rows the sums of
 * dY * xhat (row 0) and dY (row 1) — dgamma / dbeta are their sums over the chunks (mudg_group_colsum).  C <= 1280.  dres (optional,
 * rows [rows][lddres]): added to dX — the gradient of the residual branch that bypassed the norm (x + f(LN(x))). */
int64_t mudg_layernorm_bwd_chunks(int64_t rows);
int mudg_layernorm_bwd(const float* X, int64_t ldx, const float* dY, int64_t ldy, const float* gamma, float* dX, int64_t lddx,
                       float* part, int64_t rows, int C, float eps, const float* dres, int64_t lddres, void* stream);
/* Weight gradient of a linear / 3x3 conv / temporal conv layer straight from the row-major operands of the forward pass (16-bit
 * operand builds): out[slice][m][tap * C + c] = sum over the positions p of the slice of A[p][m] * B[src(p, tap)][c], with A = the
 * output gradient as operand rows [P][lda], B = the layer input as operand rows [*][ldb], src as in mudg_transpose_gather (mode 0:
 * identity, taps = 1; mode 1: 3x3 taps, tap = 3 dy + dx, taps = 9; mode 2: temporal taps, taps = 3).  M % 8 == 0, C % 64 == 0.
 * The positions are cut into `slices` ranges of `chunk` (a multiple of 64) each; the caller adds the slabs (mudg_group_colsum). */
typedef struct MudgWgradDesc {
    const void* A; const void* B; float* out;
    int64_t lda, ldb, P;
    int M, C, taps, mode;
    int Hin, Win, Hout, Wout, stride, pad, T, HW;
    int slices; int64_t chunk;
} MudgWgradDesc;
int mudg_wgrad(const MudgWgradDesc* d, void* stream);
/* One pass over fp32 rows src[P][C] (C % 4 == 0) for the three forms a layer's output gradient is needed in: dst[c][p] = src[p][c]
 * as an operand matrix [C][ldd] (columns P .. P rounded up to 8 zero; optional); rows (optional): the operand-row copy [P][ldr];
 * part (optional): fp32 [ceil(P / 64)][C], the column sums of each 64-row tile (the bias gradient is their sum). */
int mudg_transpose_cast_sum(const float* src, int64_t lds, void* dst, int64_t ldd, void* rows, int64_t ldr, float* part, int64_t P, int C,
                            void* stream);
/* GEGLU on H = [value | gate] rows [M][2 N] (attention.py:579-586): dY NULL -> out[M][N] = value * gelu(gate);
 * else out = dH [M][2 N]. */
int mudg_geglu(const float* H, int64_t ldh, const float* dY, int64_t lddy, float* out, int64_t ldo, int64_t M, int N, void* stream);
/* GEGLU followed by the feed-forward's Dropout(p) in one pass (attention.py:579-606; N % 4 == 0).  dY NULL: out [M][N] = keep(value *
 * gelu(gate)) / (1 - p) as fp32 rows and, when out16 is given, as operand rows [M][ldo16] for the next GEMM.  dY given: out = dH
 * [M][2 N].  The keep mask depends on (seed, output element index) only and is regenerated in the backward pass; p = 0: no dropout. */
int mudg_geglu_dropout(const float* H, int64_t ldh, const float* dY, int64_t lddy, float* out, int64_t ldo, void* out16, int64_t ldo16,
                       int64_t M, int N, float p, uint64_t seed, void* stream);
/* Row softmax in fp32 and its backward dS = scale * P (dP - sum_j dP_j P_j): the recomputed probabilities of the attention
 * backward pass. */
int mudg_softmax_f32(const float* S, int64_t lds, float* P, int64_t ldp, int64_t rows, int cols, void* stream);
int mudg_softmax_bwd(const float* P, int64_t ldp, const float* dP, int64_t lddp, float* dS, int64_t ldds, int64_t rows, int cols,
                     float scale, void* stream);
/* Backward of mudg_temporal_attention on fp32 Q / K / V / dO rows ((b T + t) HW + s), head h at columns [64 h, 64 h + 64). */
int mudg_temporal_attention_bwd(const float* Q, const float* K, const float* V, const float* dO, int64_t ldqkv, int64_t ldo,
                                float* dQ, float* dK, float* dV, int64_t ldg, int B, int T, int HW, int heads, float scale,
                                void* stream);
/* Backward of softmax(scale Q K^T) V, head width 64, without materialising the scores (16-bit operand builds; the forward is
 * mudg_attention, reference attention.py:81-144).  Q, dO: operand rows [F Nq][ld*]; K, V: operand rows [(F / kv_div) Nk][ld*]
 * (kv_div frames share a key / value batch: the text tokens of a clip); head h at columns [64 h, 64 h + 64).  No transposed
 * copies are needed (the kernels read K^T, Q^T, dO^T out of the row tiles with ds_read_b64_tr_b16).  L, D: fp32 [F Nq][heads]:
 * the log2-sum-exp of the scaled scores and sum_k P dP — filled by the call, or, with O given, L read (MudgAttnDesc.Lse of the
 * forward pass) and D taken from dO . O.  dQ [F Nq][ldgq], dK, dV [(F / kv_div) Nk][ldgk]: fp32, every element of the head
 * columns written once. */
typedef struct MudgAttnBwdDesc {
    const void* Q; const void* K; const void* V; const void* dO;
    const void* O;       /* optional: the forward output (operand rows, row stride ldo).  Not NULL: L holds what the forward pass
                            wrote (MudgAttnDesc.Lse) and D = sum_d dO O is taken from O — the statistics pass is skipped */
    float* L; float* D;
    float* dQ; float* dK; float* dV;
    int F, heads, Nq, Nk, kv_div;
    int ldq, ldk, ldv, lddo, ldo;
    int64_t ldgq, ldgk;
    float scale;
} MudgAttnBwdDesc;
int mudg_attention_bwd(const MudgAttnBwdDesc* d, void* stream);
/* loss[b] = mean over the n elements of sample b of (pred - target)^2; grad (optional) = w[b] * 2 (pred - target) / n — the
 * gradient of sum_b w[b] loss[b] (ddpm3d.py:766-787 folds logvar, l_simple_weight and the vlb term into w). */
int64_t mudg_mse_ws_doubles(int B);
int mudg_mse(const float* pred, const float* target, const float* w, int B, int64_t n, float* loss, float* grad, double* ws,
             void* stream);
/* Nearest-2x of channels-last fp32 rows (F, h, w, C) -> (F, 2h, 2w, C) (adjoint = 1: the sum over each 2 x 2 block, its
 * backward), and zero insertion of a stride-2 conv's output gradient onto the input grid (its input gradient is then a
 * stride-1 conv with the flipped filter). */
int mudg_upsample2x(const float* src, float* dst, int F, int h, int w, int C, int adjoint, void* stream);
int mudg_dilate2x(const float* src, float* dst, int F, int ho, int wo, int hi, int wi, int C, void* stream);
/* torch.optim.AdamW step (decoupled weight decay, bias correction with `step` >= 1), fp32, in place. */
int mudg_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
               float weight_decay, int step, void* stream);
/* The same step over many parameter tensors in ONE launch (the UNet has 1520): table = device int64 [nchunks][5] rows
 * (p, g, m, v addresses, count <= mudg_clip_chunk()) covering every parameter; bit-identical to mudg_adamw per element. */
int mudg_adamw_multi(const int64_t* table, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                     void* stream);
/* The averaged weights (lvdm/ema.py, ddpm3d.py:188-201, 398-409), same table scheme (rows of int64, count <= mudg_clip_chunk(), one
 * workgroup per row; 16-byte accesses where every address of the row is 16-byte aligned).
 * ema_multi, rows (shadow, param, count): shadow = shadow - one_minus_decay * (shadow - param), every operation rounded on its own
 *   (bit-equal to LitEma.forward on the CPU).
 * adamw_ema_multi, rows (p, g, m, v, shadow, count): mudg_adamw_multi's update and ema_multi's of the same element in one pass;
 *   p, m, v bit-identical to mudg_adamw_multi, shadow bit-identical to mudg_adamw_multi followed by mudg_ema_multi.
 * swap_multi, rows (a, b, count): a and b change places (ema_scope: one swap on entry, one on exit; no third copy). */
int mudg_adamw_ema_multi(const int64_t* table, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                         float one_minus_decay, void* stream);
int mudg_ema_multi(const int64_t* table, int nchunks, float one_minus_decay, void* stream);
int mudg_swap_multi(const int64_t* table, int nchunks, void* stream);
/* torch.nn.utils.clip_grad_norm_ over many fp32 tensors with no host round trip (the reference's trainer: gradient_clip_val 0.5,
 * norm).  table: device int64 [nchunks][2] = (address, count <= mudg_clip_chunk()) covering every gradient; partial: fp64 [nchunks]
 * scratch; out: float [2] = (total 2-norm, clip coefficient min(1, max_norm / (norm + 1e-6))); the gradients are scaled in place. */
int mudg_clip_chunk(void);
int mudg_clip_grad_norm(const int64_t* table, int nchunks, double* partial, float max_norm, float* out, void* stream);
/* Loss scaling for fp16 training (torch.amp.GradScaler semantics) with no host round trip.  record: 16 bytes of device memory,
 * 16-byte aligned: float scale, int32 growth tracker, int32 overflow flag of the current step, int32 count of steps actually taken.
 * scaled_grad_norm: the tables of mudg_clip_grad_norm over the SCALED gradients; out[0] = the 2-norm of g * inv_scale
 *   (inv_scale = float(1 / double(scale))), out[1] = min(1, max_norm / (norm + 1e-6)) or 1 when max_norm is 0 (no clipping); the
 *   record's flag is set iff any gradient is inf or NaN.  The gradients are not written.
 * unscale_multi, rows (address, count): g = g * inv_scale in place (for inspection; the optimiser does not need it).
 * adamw_scaled_multi / adamw_scaled_ema_multi: mudg_adamw_multi / mudg_adamw_ema_multi on the gradient (g * inv_scale) * stat[1]
 *   (stat: the `out` of scaled_grad_norm), bias corrections of step count + 1; flag set: parameters and moments are left alone
 *   (the EMA form still averages the unchanged parameter).
 * loss_scale_update: overflow: scale *= backoff, tracker = 0; else tracker += 1 and at growth_interval scale *= growth (if finite),
 *   tracker = 0; then count += !flag, flag = 0. */
int mudg_scaled_grad_norm(const int64_t* table, int nchunks, double* partial, float max_norm, float* out, void* record, void* stream);
int mudg_unscale_multi(const int64_t* table, int nchunks, const void* record, void* stream);
int mudg_adamw_scaled_multi(const int64_t* table, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay,
                            const void* record, const float* stat, void* stream);
int mudg_adamw_scaled_ema_multi(const int64_t* table, int nchunks, float lr, float beta1, float beta2, float eps, float weight_decay,
                                float one_minus_decay, const void* record, const float* stat, void* stream);
int mudg_loss_scale_update(void* record, float growth_factor, float backoff_factor, int growth_interval, void* stream);
/* Inverted dropout out[i] = keep(seed, i) ? x[i] / (1 - p) : 0 with a counter-based mask (the backward pass applies the same
 * call to the gradient: nothing is stored). */
int mudg_dropout(const float* x, float* out, int64_t n, float p, uint64_t seed, void* stream);
/* The same mask (element index = m C + c) on fp32 rows [M][C] (C % 4 == 0) with any row strides, optionally also writing the
 * operand rows of the result (what the conv / projection after the Dropout reads). */
int mudg_dropout_rows(const float* X, int64_t ldx, float* Y, int64_t ldy, void* Y16, int64_t ldy16, int64_t M, int C, float p, uint64_t seed,
                      void* stream);
/* out = gelu_erf(x) (dy NULL) or dy * gelu_erf'(x): the Perceiver Resampler's feed-forward activation (resampler.py:27-34). */
int mudg_gelu(const float* x, const float* dy, float* out, int64_t n, void* stream);
/* out = silu(x) (dy NULL) or dy * silu'(x). */
int mudg_silu(const float* x, const float* dy, float* out, int64_t n, void* stream);

/* ------------------------------------------------------------------ event profiler (bench.py roofline)
 * When enabled, every launch of kernel family `fam` is bracketed by hipEvents on its own stream. */
enum { MUDG_FAM_GEMM = 0, MUDG_FAM_CONV = 1, MUDG_FAM_TCONV = 2, MUDG_FAM_ATTN = 3, MUDG_FAM_TATTN = 4,
       MUDG_FAM_GNORM = 5, MUDG_FAM_LNORM = 6, MUDG_FAM_MISC = 7, MUDG_FAM_COUNT = 8 };
int mudg_prof_enable(int family_mask);       /* 0 disables and drops pending events */
/* Synchronises the recorded events and returns totals since the last reset. */
int mudg_prof_collect(int fam, double* total_ms, int64_t* launches, double* flops, double* bytes);
int mudg_prof_reset(void);

#ifdef __cplusplus
}
#endif
#endif
