"""Every forward contraction kernel behind mudg_gemm (csrc/gemm.hip, pgemm.hip, wgemm.hip) called through the C-ABI with a
hip.GemmDesc built here — strides, pointer alignment and gaps are the test's — and held to the plain fp64 definitions of
tests/gemm_reference.py, evaluated on the very operands the kernel reads (made once on the CPU).

  exact      operands, biases and residuals are small integers, alpha a power of two: every product and every partial sum is a multiple of
             one power of two below 2^24 of them, which fp32 holds exactly in any order (tests/test_gemm_reference_cpu.py asserts that for
             every case of the tables below).  torch.equal on Y, on `stats` and on Y8 / S8; a 16-bit result is the ONE rounding of the exact
             value.  In the split builds the piece planes of X and W are independent integers (not the decomposition of a value) and the
             expected result is the sum over the piece pairs csrc/common.h keeps: a dropped, doubled or swapped pair is a wrong integer.
             GELU / GEGLU join in through gates >= 8, where every documented scheme (the Phi table, the erf polynomial, erff) returns
             Phi = 1.0f: the result is the exact product.
  bounded    random operands rounded once to the operand type.  See test_*_bounded_* and test_gelu_geglu_gate_sweep for the bounds.
  refusals   every MUDG_REQUIRE of mudg_gemm that no other test triggers, and each clause of mudg_conv_subpixel_ok.

Every operand and result is a view inside a NaN-filled buffer (gap columns between the rows, guard rows around them); after each call
everything outside the view must still be NaN.  All views are in bounds.  Which kernel runs a case follows from gemm_plan (csrc/gemm.hip);
the clause a case aims at stands next to it.  The variant children of tests/test_gemm_variants_gpu.py run this file under every switch,
which is how the forced kernels (generic, single-buffer, wide, persistent at 2 / 3 / 4, W288 / W288P / W288Q / H144 / W160) meet these shapes."""
import ctypes as C
import math

import pytest
import torch

import gemm_reference as R
from backward_reference import operand_planes
from mudg_amd import hip
from sentinel_buffers import Buf

pytestmark = pytest.mark.gpu

NAN = float("nan")
F64 = torch.float64
PLANES = hip.planes()
SPLIT = PLANES > 1
OPER, F32K, F16K = R.KIND_OPERAND, R.KIND_F32, R.KIND_F16
TOL_F32 = 2e-5                     # tests/test_kernels_gpu.py: fp32 results on identical inputs differ by accumulation order only
FLIP_CAP = 0.01                    # bounded 16-bit results: share of a 32 x 64 block that may sit on the other storage neighbour


def _s():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator().manual_seed(seed)


def kind_dtype(kind):
    return {OPER: hip.operand_dtype(), F32K: torch.float32, F16K: torch.float16}[kind]


# ================================================================================================ buffers
def in_buf(pieces, gap, dev, dtype, planes=1):
    """An input [b][rows][cols]: row stride planes * (cols + gap) (gap a multiple of 8: rows stay 16-byte aligned), NaN in the gaps, and
    NaN rows after the last one for a whole tile height (a ragged tile's masked rows lie inside the allocation)."""
    b, rows, cols = pieces[0].shape
    ld = planes * (cols + gap)
    return Buf(b, rows, cols, ld, dtype, planes=planes, sb=rows * ld, tail_rows=328).put(pieces, dev)


def out_buf(batch, rows, cols, kind, pad, off, dev, sb=None):
    """A result [batch][rows][cols] of storage `kind`: row stride planes * (cols + pad) — pad 0 / 8: 16-byte rows where cols % 8 == 0;
    pad 1: rows that are not — base `off` elements past an aligned address."""
    planes = PLANES if kind == OPER else 1
    ld = planes * (cols + pad)
    return Buf(batch, rows, cols, ld, kind_dtype(kind), off=off, planes=planes, sb=rows * ld + 24 if sb is None else sb).blank(dev)


# ================================================================================================ operands
def ints(*shape, seed, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).to(torch.float32)


def asym_w(n, k, p=0):
    """W[n][k] = (n * 251 + k * (1 + 2 p)) % 7 - 3: no two rows and no two columns of a 7-neighbourhood alike."""
    nn, kk = torch.arange(n)[:, None], torch.arange(k)[None, :]
    return ((nn * 251 + kk * (1 + 2 * p) + 3 * p) % 7 - 3).to(torch.float32)


def onehot_x(rows, cin, p=0):
    """Row r is the unit vector of channel (7 r + 3 + 5 p) % cin: the output then names the row of W, the tap and the source it came from."""
    x = torch.zeros((rows, cin))
    x[torch.arange(rows), (7 * torch.arange(rows) + 3 + 5 * p) % cin] = 1.0
    return x


def position_x(coords, cin, p=0):
    """coords = (frame, y, x) (or (clip, t, s)) per row: channel c carries coordinate (c + p) % 3, folded to -3 .. 3."""
    cols = [(coords[(c + p) % 3] % 7 - 3).to(torch.float32) for c in range(3)]
    return torch.stack([cols[c % 3] for c in range(cin)], 1)


def conv_coords(frames, h, w):
    m = torch.arange(frames * h * w)
    return m // (h * w), (m % (h * w)) // w, m % w


# ================================================================================================ case tables
# Tile constants the shapes are read off (csrc/gemm_shared.h, gemm.hip, wgemm.hip): 128 x 128 one-tile kernels with BK = 64; 288-row and
# 160-row tiles 320 columns wide (GEGLU: 256); the persistent 288-row form wants K >= 2 BK and more tiles than CUs.
def G(name, M, N, K, why, **kw):
    return dict(name=name, mode=0, M=M, N=N, K=K, why=why, **kw)


GEMM_CASES = [
    # ---- the generic loader (K % 64 != 0): ragged K below, at and above one K-tile; M and N on both sides of a 128 tile
    G("m1_n4_k8", 1, 4, 8, "smallest problem: one row, half a store chunk, one 8-wide K chunk", bias=True, out=F32K),
    G("m127_n8_k56", 127, 8, 56, "one row short of a tile, K short of a K-tile", alpha=0.5, out=OPER),
    G("m128_n100_k72", 128, 100, 72, "whole tile, N not a multiple of 8 (scalar tail stores), K one chunk past a K-tile", bias=True, res=F32K, out=OPER),
    G("m129_n136_k72", 129, 136, 72, "one row and one chunk past a tile in M and N: four tiles, three of them ragged", alpha=2.0, res=OPER, out=F16K, ypad=1, yoff=1),
    G("m389_n328_k56", 389, 328, 56, "three whole row tiles and a tail, three column tiles", bias=True, gbias=97, res=F16K, out=F32K, rpad=1, roff=1),
    # ---- the descriptor loader (K % 64 == 0), one-tile kernels: single K-tile, two, three
    G("m159_n128_k64", 159, 128, 64, "single K-tile: prologue = epilogue of the K loop", bias=True, out=OPER, ypad=8),
    G("m160_n256_k128", 160, 256, 128, "two K-tiles, two column tiles", alpha=0.5, res=F16K, out=F16K),
    G("m161_n320_k192", 161, 320, 192, "three K-tiles, N = 320 without a frame hint stays on the 128 x 128 kernels", res=F32K, out=F32K, ypad=1, yoff=1, rpad=1, roff=1),
    G("m287_n100_k64", 287, 100, 64, "descriptor loader with scalar tail stores", bias=True, gbias=128, out=OPER),
    G("m288_n8_k128", 288, 8, 128, "one store chunk per row", gbias=96, res=OPER, out=OPER, rpad=8),
    G("m289_n136_k192", 289, 136, 192, "row tail of one", alpha=0.0, bias=True, out=F16K, ypad=1),
    G("m129_n128_k64_mis", 129, 128, 64, "VF_Y and VF_R both off on a shape that would take 16-byte stores", res=OPER, out=OPER, ypad=1, yoff=1, rpad=1, roff=1),
    # ---- two channel sources
    G("x2_csplit8", 130, 72, 72, "csplit 8: the second source starts in the first K chunk (generic loader)", csplit=8, bias=True, out=F32K),
    G("x2_csplit64", 130, 72, 128, "csplit 64 = one K-tile per source (descriptor loader)", csplit=64, out=OPER),
    G("x2_csplit_k_minus_8", 130, 72, 136, "csplit Cin - 8: the second source is one chunk", csplit=128, res=F32K, out=OPER),
    # ---- batch
    G("batch3_strides", 70, 72, 64, "batch with all four strides", batch=3, bias=True, res=F32K, out=OPER),
    G("batch3_shared_x_vt", 128, 100, 64, "sX = 0 with W per batch and a padded ldy: the swapped-operand V^T form (X = the projection's rows, "
      "W = a batch's tokens, Y = V^T [channels][tokens padded])", batch=3, share_x=True, out=OPER, ypad=12),
    # ---- the 288-row tile by rule: N % 320 == 0, K % 64 == 0, frame hint HW % 288 == 0
    G("w288_m1", 1, 320, 64, "288-row tile, one valid row, single K-tile", hint=288, bias=True, out=OPER),
    G("w288_m287", 287, 320, 128, "288-row tile one row short; residual seeds the accumulators", hint=288, res=F16K, out=F16K),
    G("w288_m288_gb", 288, 640, 64, "whole tile, two column tiles, group bias per tile", hint=288, gbias=288, bias=True, res=F32K, out=OPER),
    G("w288_m289", 289, 320, 192, "two tiles, the second with one row", hint=576, res=OPER, out=F32K),
    G("w288_m583_x2", 583, 320, 128, "two tiles and a tail, two sources of one K-tile each", hint=288, csplit=64, bias=True, out=OPER),
    # ---- the 160-row tile by rule: mode 0 needs K >= 1280, frames of >= 640 rows that are whole 160-row but not whole 288-row tiles
    G("w160_m161_k1280", 161, 320, 1280, "160-row tile, fp32 residual seeds", hint=640, res=F32K, out=OPER),
    G("w160_m321_defer", 321, 320, 1280, "160-row tile, 16-bit residual deferred to the epilogue", hint=640, res=F16K, bias=True, out=F16K),
    # ---- the persistent kernel by rule: plain GEMM with N >= 1280 and K >= 1280
    G("persist_n1280_k1280", 129, 1280, 1280, "pgemm_kernel: 20 tiles walked by persistent workgroups, residual seed, a group bias per row tile", res=F32K, bias=True, gbias=128, out=OPER),
    # ---- the single-buffer kernel by rule: >= 768 tiles (K <= 128: the volume is in M x N)
    G("single_768_tiles", 12288, 1024, 64, "gemm_kernel<.., SB>: 96 x 8 = 768 tiles", bias=True, out=OPER),
    # ---- GELU / GEGLU on exact terms: every gate >= 8 (bias 9 K + 8), where Phi = 1.0f in every scheme
    G("act_gate8", 130, 72, 64, "plain GELU epilogue (never persistent / tile kernels)", act=True, out=F32K),
    G("geglu_n64", 129, 64, 64, "GEGLU, one [32 | 32] block: the persistent kernel (every GEGLU on the descriptor loader)", geglu=True, out=F32K),
    G("geglu_n256_k72", 200, 256, 72, "GEGLU on the generic loader (K % 64 != 0)", geglu=True, out=OPER),
    G("geglu_n512", 289, 512, 128, "GEGLU, four column tiles of 128", geglu=True, out=OPER, ypad=8),
    G("geglu_w288_k640", 289, 256, 640, "GEGLU on the 288 x 256 tile, one-tile form (K >= 640 with a frame hint)", geglu=True, hint=288, out=OPER),
    G("geglu_w288p", 288 * 130, 512, 128, "wgemm_pkernel: 130 x 2 = 260 tiles, more than the 256 CUs, K = 2 BK", geglu=True, hint=288, out=OPER),
]


def CV(name, frames, h, w, cin, N, why, **kw):
    return dict(name=name, mode=1, frames=frames, h=h, w=w, cin=cin, N=N, why=why, **kw)


CONV_CASES = [
    # ---- degenerate and odd images, tap-major K (korder 0), generic loader (Cin % 64 != 0)
    CV("1x1", 3, 1, 1, 8, 8, "every tap but the centre is padding", bias=True, out=F32K),
    CV("1x2", 3, 1, 2, 8, 100, "H = 1: no vertical neighbour", out=OPER, make="position"),
    CV("2x1", 3, 2, 1, 16, 8, "W = 1: no horizontal neighbour", out=OPER, make="position"),
    CV("5x7_onehot", 5, 5, 7, 24, 136, "odd sizes, 175 rows: a tile spans frames; one-hot names the tap", out=F32K, make="onehot"),
    CV("3x5_three_frames_per_tile", 20, 3, 5, 8, 72, "15-row frames: a 128-row tile holds eight frames and parts of two", gbias=15, bias=True, res=F32K, out=OPER, make="position"),
    # ---- stride 2 on odd sizes, both pads
    CV("s2_p1_5x7", 4, 5, 7, 16, 72, "stride 2 / pad 1 on an odd image: last output reads the last pixel", stride=2, out=OPER, make="position"),
    CV("s2_p0_5x7", 4, 5, 7, 16, 72, "stride 2 / pad (0,1,0,1): only bottom / right zeros", stride=2, pad=0, out=F32K, make="position"),
    CV("s2_p0_8x6_k1", 3, 8, 6, 64, 136, "the AutoencoderKL downsample on the descriptor loader, slab-major K", stride=2, pad=0, korder=1, bias=True, out=OPER),
    CV("s2_p1_9x9_n320", 2, 9, 9, 64, 320, "stride 2 at N = 320: no tile kernel takes it, so the forced wide 256 x 320 tile (MUDG_GEMM_WIDE=1) does", stride=2, korder=1, bias=True, out=OPER, make="position"),
    CV("s2_p1_9x9_x2", 2, 9, 9, 72, 40, "stride 2 with two sources, csplit 8", stride=2, csplit=8, out=OPER),
    # ---- fused nearest-2x upsample (generic loader by rule)
    CV("up_2x3", 3, 2, 3, 8, 72, "upsample: four output pixels per source pixel", upsample=1, out=OPER, make="position"),
    CV("up_5x8_k1", 2, 5, 8, 64, 136, "upsample with slab-major K", upsample=1, korder=1, bias=True, out=F16K),
    # ---- same-size slab-major convs: the XSHARE halo path, Win in {1, 2, 7, 16}
    CV("xs_w1", 3, 9, 1, 64, 72, "XSHARE with W = 1", korder=1, out=OPER, make="position"),
    CV("xs_w2", 3, 5, 2, 64, 72, "XSHARE with W = 2", korder=1, bias=True, out=F32K, make="position"),
    CV("xs_w7", 3, 9, 7, 128, 136, "XSHARE with an odd W, two slabs, 189 rows", korder=1, res=F16K, out=OPER, make="onehot"),
    CV("xs_w16_x2", 2, 10, 16, 128, 264, "XSHARE with W = 16, two sources of one slab each, three column tiles", korder=1, csplit=64, gbias=160, bias=True, res=F32K, out=OPER),
    CV("k0_same_cin64", 2, 6, 7, 64, 72, "tap-major K on the descriptor loader", out=OPER, make="position"),
    CV("x2_cin_minus_8", 2, 4, 5, 72, 40, "two sources, csplit Cin - 8 (generic loader)", csplit=64, out=F32K),
    # ---- the tile kernels by rule: frames of whole 288-row / 160-row tiles, N % 320 == 0
    CV("w288_12x24", 2, 12, 24, 64, 320, "288-row tile: one frame per tile, group bias per frame, residual seed", gbias=288, bias=True, res=F16K, out=OPER, make="position"),
    CV("w288_12x24_k1", 1, 12, 24, 128, 320, "288-row tile, slab-major K, two slabs", korder=1, out=F32K),
    CV("w160_20x32", 1, 20, 32, 64, 320, "160-row tile: 640-pixel frame, fp32 residual seeds", res=F32K, out=OPER, make="position"),
    CV("w160_20x32_defer", 1, 20, 32, 64, 320, "160-row tile, 16-bit residual deferred", korder=1, res=F16K, bias=True, out=F16K),
    # ---- the single-buffer kernel by rule: same-size slab-major convs from 1024 tiles
    CV("single_1024_tiles", 4, 64, 64, 64, 1024, "gemm_kernel<.., 1, .., SB> with XSHARE: 128 x 8 = 1024 tiles", korder=1, out=OPER),
]

SUBPIXEL_CASES = [
    CV("sub_1x1", 3, 1, 1, 64, 72, "sub-pixel form on single pixels: three of four taps are padding", subpixel=1, korder=1, bias=True, out=OPER, make="position"),
    CV("sub_2x3", 3, 2, 3, 64, 136, "sub-pixel form, odd width", subpixel=1, korder=1, out=F32K, make="onehot"),
    CV("sub_5x8", 4, 5, 8, 128, 72, "sub-pixel form, 160 rows, two slabs", subpixel=1, korder=1, bias=True, out=F16K, make="position", ypad=1, yoff=1),
]


def TC(name, clips, t, hw, cin, N, why, **kw):
    return dict(name=name, mode=2, clips=clips, t=t, hw=hw, cin=cin, N=N, why=why, **kw)


TCONV_CASES = [
    TC("t1", 5, 1, 30, 8, 72, "T = 1: both outer taps are always zero; clip boundaries inside a tile", out=OPER, make="position"),
    TC("t2", 4, 2, 20, 16, 72, "T = 2: every frame is first or last", bias=True, out=F32K, make="position"),
    TC("t3_onehot", 3, 3, 15, 24, 136, "T = 3, 45-row clips: a tile spans three clips; one-hot names the tap", out=F32K, make="onehot"),
    TC("t3_n256", 3, 3, 15, 64, 256, "N = 256 on the descriptor loader: the forced wide 256 x 256 tile in mode 2", bias=True, out=OPER, make="position"),
    TC("t3_n320", 3, 3, 15, 64, 320, "N = 320 with 15-row frames: the forced wide 256 x 320 tile in mode 2", res=F32K, out=F32K),
    TC("t16_cin64", 2, 16, 5, 64, 72, "T = 16 on the descriptor loader, tap-major, 80-row clips", gbias=80, res=F32K, out=OPER, make="position"),
    TC("t17_x2", 2, 17, 4, 72, 40, "T = 17 with two sources (generic loader)", csplit=8, res=F16K, out=OPER),
    TC("k1_hw8", 2, 16, 8, 64, 72, "slab-major: one 8-pixel x 16-frame tile per clip", korder=1, gbias=128, bias=True, out=OPER, make="position"),
    TC("k1_hw24", 2, 16, 24, 64, 136, "slab-major, three tiles per clip", korder=1, res=F32K, out=F32K, make="position"),
    TC("k1_hw72", 1, 16, 72, 128, 72, "slab-major, nine tiles, two slabs", korder=1, gbias=1152, out=F16K, make="onehot"),
    TC("w288_hw288", 1, 2, 288, 64, 320, "288-row tile: one frame per tile, both frames an edge", bias=True, res=F16K, out=OPER, make="position"),
    TC("w160_hw640", 1, 2, 640, 64, 320, "160-row tile", res=F32K, out=OPER, make="position"),
]

# (case, which table) for `stats`: the block height is whatever mudg_gemm_stats_rows reports; M is not a multiple of it; every out kind
STATS_CASES = [
    G("stats_gemm_operand", 300, 136, 128, "128-row blocks, ragged last block", bias=True, out=OPER, stats=True, make="onehot"),
    G("stats_gemm_f16", 300, 72, 72, "generic loader, fp16 storage", res=F32K, out=F16K, stats=True, make="onehot"),
    G("stats_gemm_f32", 130, 100, 64, "fp32 storage, N % 8 != 0", gbias=65, out=F32K, stats=True, make="onehot"),
    # the rounding itself: y = 0.5 w + 2049 +- 5 are half-integers beyond the 11 bits of fp16 (and the 8 of bf16), three rows keep the sums
    # of squares below 2^24: partials taken BEFORE the storage rounding are a different number (16-bit operand builds; bf16x3 / bf16x6
    # operands hold these values unrounded, fp16 storage rounds them in every build)
    *([] if SPLIT else [G("stats_rounding_operand", 3, 72, 64, "stats of the rounded values, operand storage", alpha=0.5, bias_value=2049.0, out=OPER,
                           stats=True, make="onehot")]),
    G("stats_rounding_f16", 3, 136, 128, "stats of the rounded values, fp16 storage", alpha=0.5, bias_value=2049.0, out=F16K, stats=True, make="onehot"),
    G("stats_w288", 289, 320, 128, "288-row blocks", hint=288, bias=True, res=F16K, out=OPER, stats=True, make="onehot"),
    G("stats_w160", 161, 320, 1280, "160-row blocks", hint=640, out=OPER, stats=True, make="onehot"),
    CV("stats_conv", 3, 9, 7, 64, 72, "conv partials, 189 rows", korder=1, bias=True, out=OPER, stats=True, make="onehot"),
    CV("stats_conv_w288", 2, 12, 24, 64, 320, "conv on the 288-row tile", gbias=288, out=F16K, stats=True, make="onehot"),
    TC("stats_tconv", 2, 3, 25, 64, 72, "temporal conv partials, 150 rows", out=OPER, stats=True, make="onehot"),
]
FP8_CASES = [
    G("fp8_gemm", 130, 160, 128, "fused MX-fp8 copy: five scale blocks per row, ragged row tile", bias=True, out=OPER, fp8=True),
    G("fp8_gemm_k72", 70, 64, 72, "fused MX-fp8 copy on the generic loader", out=OPER, fp8=True, alpha=0.5),
    CV("fp8_conv", 2, 5, 7, 64, 96, "fused MX-fp8 copy of a conv", korder=1, out=OPER, fp8=True),
]
EXACT_CASES = GEMM_CASES + CONV_CASES + SUBPIXEL_CASES + TCONV_CASES + STATS_CASES + FP8_CASES


# ================================================================================================ geometry of a case
def geometry(c):
    """(rows of X, M, K, Cin, taps) of a case."""
    if c["mode"] == 0:
        return c["M"], c["M"], c["K"], c["K"], 1
    if c["mode"] == 1:
        if c.get("subpixel"):
            m = c["frames"] * c["h"] * c["w"]
            return m, m, 4 * c["cin"], c["cin"], 4
        ho, wo = R.conv_out_size(c["h"], c["w"], c.get("stride", 1), c.get("pad", 1), c.get("upsample", 0))
        return c["frames"] * c["h"] * c["w"], c["frames"] * ho * wo, 9 * c["cin"], c["cin"], 9
    m = c["clips"] * c["t"] * c["hw"]
    return m, m, 3 * c["cin"], c["cin"], 3


def contract_of(c):
    """The raw fp64 contraction of a case as a function of (x [1 | b][rows][Cin], w [.][N][K])."""
    if c["mode"] == 0:
        return R.contract_gemm
    if c["mode"] == 1:
        if c.get("subpixel"):
            return lambda x, w: R.contract_subpixel(x, w, frames=c["frames"], hin=c["h"], win=c["w"], cin=c["cin"])
        return lambda x, w: R.contract_conv3x3(x, w, frames=c["frames"], hin=c["h"], win=c["w"], cin=c["cin"], stride=c.get("stride", 1),
                                               pad=c.get("pad", 1), upsample=c.get("upsample", 0), korder=c.get("korder", 0))
    return lambda x, w: R.contract_tconv3(x, w, clips=c["clips"], t=c["t"], hw=c["hw"], cin=c["cin"], korder=c.get("korder", 0))


def coords_of(c):
    if c["mode"] == 1:
        return conv_coords(c["frames"], c["h"], c["w"])
    return conv_coords(c["clips"], c["t"], c["hw"])


def gate_bias(c, planes):
    """Exact GELU / GEGLU: operands are -1 .. 1 there, so |sum| <= pairs * K, and this bias lifts every gate to >= 8."""
    return float(len(R.KEPT[planes]) * c["K"] + 8)


def exact_operands(c, planes, seed):
    """Piece planes of X [bx][rows][Cin] and W [bw][N][K], bias, gbias, residual pieces: all small integers (-3 .. 3; -1 .. 1 where a
    GELU / GEGLU follows, which squares the magnitudes)."""
    rows, M, K, cin, taps = geometry(c)
    batch, N = c.get("batch", 1), c["N"]
    bx = 1 if c.get("share_x") else batch
    bw = 4 if c.get("subpixel") else batch
    make = c.get("make", "ints")
    gate = c.get("act") or c.get("geglu")
    top = 1 if gate else 3
    xs, ws = [], []
    for p in range(planes):
        if make == "onehot":
            xs.append(onehot_x(rows, cin, p)[None].repeat(bx, 1, 1))
            ws.append(torch.stack([asym_w(N, K, p + 2 * z) for z in range(bw)]))
        elif make == "position":
            xs.append(position_x(coords_of(c), cin, p)[None])
            ws.append(ints(bw, N, K, seed=seed + 11 + p))
        else:
            xs.append(ints(bx, rows, cin, seed=seed + p, lo=-top, hi=top))
            ws.append(ints(bw, N, K, seed=seed + 11 + p, lo=-top, hi=top))
    nout = N // 2 if c.get("geglu") else N
    bias = ints(N, seed=seed + 21, lo=-5, hi=5) if c.get("bias") else None
    if c.get("bias_value"):
        bias = ints(N, seed=seed + 21, lo=-5, hi=5) + c["bias_value"]
    if c.get("act"):
        bias = torch.full((N,), gate_bias(c, planes))
    if c.get("geglu"):
        bias = ints(N, seed=seed + 21, lo=-5, hi=5)
        bias[R.geglu_unpack(nout)[1]] = gate_bias(c, planes)
    gb = None
    if c.get("gbias"):
        gb = ints((M + c["gbias"] - 1) // c["gbias"], nout, seed=seed + 22, lo=-9, hi=9)
    res = None
    if c.get("res") is not None:
        rp = planes if c["res"] == OPER else 1
        mo = 4 * M if c.get("subpixel") else M
        res = [ints(batch, mo, nout, seed=seed + 31 + p, lo=-7, hi=7) for p in range(rp)]
    return xs, ws, bias, gb, res


def exact_value(c, xs, ws, bias, gb, res, planes):
    """The fp64 result the header defines for these operands: [batch][M out][Nout]."""
    s = R.split_kept(contract_of(c), xs, ws, planes)
    r = sum(t.to(F64) for t in res) if res is not None else None
    return R.epilogue(s, alpha=c.get("alpha", 1.0), bias=bias, gbias=gb, rows_per_group=c.get("gbias", 0), act=c.get("act", False),
                      geglu=c.get("geglu", False), r=r)


def exactness(c, planes, seed=1):
    """(bound / unit, unit): every product and every partial sum of the case, in ANY order, is a multiple of `unit` (a power of two) and
    at most `bound` in magnitude; bound / unit < 2^24 makes fp32 exact.  Linear cases: the worst case of the operand ranges, |sum| <=
    9 pairs K, times alpha, plus bias (5), group bias (9) and residual pieces (7 each).  GELU / GEGLU cases (operands -1 .. 1, Phi = 1):
    the result is the product v * g; worst case first, and where that is too coarse the operands' own sum_k |x_k| |w_k|, which bounds
    every partial sum of that output in any order."""
    rows, M, K, cin, taps = geometry(c)
    pairs = len(R.KEPT[planes])
    if c.get("act") or c.get("geglu"):
        s = float(pairs * K)
        worst = (s + gate_bias(c, planes)) * ((s + 5) if c.get("geglu") else 1.0)
        if worst < 2 ** 24:
            return worst, 1.0
        xs, ws, bias, gb, res = exact_operands(c, planes, seed)
        s = float(R.split_kept(contract_of(c), [x.abs() for x in xs], [w.abs() for w in ws], planes).max())
        return (s + gate_bias(c, planes)) * ((s + 5) if c.get("geglu") else 1.0), 1.0
    alpha = c.get("alpha", 1.0) or 1.0
    unit = min(alpha, 1.0)
    return R.exact_bits(3, 3, pairs * K, unit, (c.get("bias_value", 0.0) + 5 + 9 + 7 * planes) / max(alpha, 1.0)) * max(alpha, 1.0), unit


# ================================================================================================ the call
def describe(c, b, m, n):
    if c["mode"] == 0:
        return f"batch {b} row {m} col {n}"
    if c["mode"] == 1:
        if c.get("subpixel"):
            hh, ww = 2 * c["h"], 2 * c["w"]
        else:
            hh, ww = R.conv_out_size(c["h"], c["w"], c.get("stride", 1), c.get("pad", 1), c.get("upsample", 0))
        return f"frame {m // (hh * ww)} y {(m % (hh * ww)) // ww} x {m % ww} channel {n}"
    return f"clip {m // (c['t'] * c['hw'])} t {(m // c['hw']) % c['t']} pixel {m % c['hw']} channel {n}"


def assert_same(c, what, got, want):
    got, want = got.to(F64), want.to(F64)
    assert got.shape == want.shape, (c["name"], what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = torch.nonzero(~(got == want))
    lines = []
    for idx in bad[:6].tolist():
        b, m, n = (idx + [0, 0, 0])[:3] if got.dim() == 3 else (0, idx[0], idx[-1])
        lines.append(f"{describe(c, b, m, n) if got.dim() == 3 else idx}: got {float(got[tuple(idx)])} want {float(want[tuple(idx)])}")
    raise AssertionError(f"{c['name']} ({c['why']}): {what}: {bad.shape[0]} of {got.numel()} elements differ; first: " + "; ".join(lines))


class Call:
    """One mudg_gemm call: buffers placed, descriptor filled; run() launches and reads everything back."""

    def __init__(self, c, xs, ws, bias, gb, res, dev):
        rows, M, K, cin, taps = geometry(c)
        self.c, N = c, c["N"]
        batch = c.get("batch", 1)
        nout = N // 2 if c.get("geglu") else N
        mo = 4 * M if c.get("subpixel") else M
        dt = hip.operand_dtype()
        csplit = c.get("csplit")
        d = self.d = hip.GemmDesc()
        self.keep = []
        if csplit:
            x1 = in_buf([x[..., :csplit] for x in xs], 8, dev, dt, PLANES)
            x2 = in_buf([x[..., csplit:] for x in xs], 0, dev, dt, PLANES)
            d.X2, d.ldx2, d.csplit = x2.ptr, x2.ld, csplit
            self.keep.append(x2)
        else:
            x1 = in_buf(xs, c.get("xgap", 8), dev, dt, PLANES)
            d.csplit = cin
        w = in_buf(ws, c.get("wgap", 8), dev, dt, PLANES)
        self.keep += [x1, w]
        self.y = out_buf(1 if c.get("subpixel") else batch, mo, nout, c["out"], c.get("ypad", 0), c.get("yoff", 0), dev)
        d.X, d.W, d.Y = x1.ptr, w.ptr, self.y.ptr
        d.M, d.N, d.K = M, N, K
        d.ldx, d.ldw, d.ldy = x1.ld, w.ld, self.y.ld
        d.batch = 4 if c.get("subpixel") else batch
        d.sX = 0 if (c.get("share_x") or c.get("subpixel")) else x1.sb
        d.sW, d.sY = w.sb, (0 if c.get("subpixel") else self.y.sb)
        if bias is not None:
            self.bias = bias.to(dev)
            d.bias = self.bias.data_ptr()
        if gb is not None:
            self.gb = gb.to(dev).contiguous()
            d.gbias, d.rows_per_group = self.gb.data_ptr(), c["gbias"]
        if res is not None:
            rk = c["res"]
            rp = PLANES if rk == OPER else 1
            ldr = rp * (nout + c.get("rpad", 0))
            self.r = Buf(batch, mo, nout, ldr, kind_dtype(rk), off=c.get("roff", 0), planes=rp, sb=mo * ldr + 40).put(res, dev)
            d.R, d.ldr, d.sR, d.res_fp32 = self.r.ptr, ldr, self.r.sb, rk
        d.out_fp32, d.geglu, d.act, d.alpha, d.mode = c["out"], int(c.get("geglu", False)), int(c.get("act", False)), c.get("alpha", 1.0), c["mode"]
        if c["mode"] == 0:
            d.HW = c.get("hint", 0)
        elif c["mode"] == 1:
            up, sub = c.get("upsample", 0), c.get("subpixel", 0)
            ho, wo = (c["h"], c["w"]) if sub else R.conv_out_size(c["h"], c["w"], c.get("stride", 1), c.get("pad", 1), up)
            d.Hin, d.Win, d.Hout, d.Wout, d.Cin, d.stride, d.upsample = c["h"], c["w"], ho, wo, cin, c.get("stride", 1), up
            d.pad, d.korder, d.subpixel = c.get("pad", 1), c.get("korder", 0), sub
        else:
            d.Cin, d.T, d.HW, d.korder = cin, c["t"], c["hw"], c.get("korder", 0)
        self.stats = self.y8 = self.s8 = None
        if c.get("stats"):
            self.brows = hip.lib().mudg_gemm_stats_rows(C.byref(d))
            assert self.brows in (128, 160, 288), self.brows
            blocks = (M + self.brows - 1) // self.brows
            self.stats = Buf(1, blocks, 2 * nout, 2 * nout, torch.float32).blank(dev)
            d.stats = self.stats.ptr
        if c.get("fp8") and not SPLIT:
            self.y8 = Buf(1, M, nout, nout + 8, torch.uint8).blank(dev)
            self.s8 = Buf(1, M, nout // 32, nout // 32 + 3, torch.uint8).blank(dev)
            d.Y8, d.S8, d.ldy8, d.lds8 = self.y8.ptr, self.s8.ptr, self.y8.ld, self.s8.ld

    def run(self):
        hip.check(hip.lib().mudg_gemm(C.byref(self.d), _s()), f"mudg_gemm[{self.c['name']}]")
        torch.cuda.synchronize()
        return self.y.read(self.c["name"] + " Y")


def subpixel_available():
    """The sub-pixel form needs the descriptor loader (mudg_conv_subpixel_ok: "a problem the buffer-descriptor kernels accept"): the one
    variant child that switches that loader off (MUDG_GEMM_FAST=0) must refuse it, and callers then run upsample = 1."""
    import os
    return not (os.environ.get("MUDG_DEBUG_VARIANTS") == "1" and os.environ.get("MUDG_GEMM_FAST") == "0")


def refused_without_the_descriptor_loader(c, call):
    """True (after asserting the refusal) when this sub-pixel case cannot run because the descriptor loader is switched off."""
    if not c.get("subpixel") or subpixel_available():
        return False
    assert hip.lib().mudg_conv_subpixel_ok(C.byref(call.d)) == 0
    with pytest.raises(hip.MudgError):
        call.run()
    return True


def stats_exact_bits(y_stored, rows):
    """Largest sum of squares over a block of `rows` rows, in units of the square of the stored values' own granularity: below 2^24 every
    partial sum of the squares, in any order, is exact in fp32 (the plain sums are smaller still)."""
    unit = next(u for u in (1.0, 0.5, 0.25, 0.125, 2.0 ** -4, 2.0 ** -5) if bool((y_stored / u == torch.round(y_stored / u)).all()))
    return float(R.stats(y_stored, rows)[..., 1].max()) / unit ** 2


def run_exact(c, dev, seed=1):
    bits, unit = exactness(c, PLANES, seed)
    assert bits < 2 ** 24, (c["name"], bits)
    xs, ws, bias, gb, res = exact_operands(c, PLANES, seed)
    want = exact_value(c, xs, ws, bias, gb, res, PLANES)
    assert bool((want.to(torch.float32).to(F64) == want).all())            # fp32 holds the expected values exactly
    call = Call(c, xs, ws, bias, gb, res, dev)
    if refused_without_the_descriptor_loader(c, call):
        return
    if c.get("subpixel"):
        assert hip.lib().mudg_conv_subpixel_ok(C.byref(call.d)) == 1
    got = call.run()
    for p, (g, w) in enumerate(zip(got, R.store_pieces(want, c["out"], hip.operand_dtype(), PLANES))):
        assert_same(c, f"Y piece {p}", g, w)
    y_stored = R.store(want, c["out"], hip.operand_dtype(), PLANES)
    if call.stats is not None:
        st = call.stats.read(c["name"] + " stats")[0][0]
        exp = R.stats(y_stored[0], call.brows)
        assert stats_exact_bits(y_stored[0], call.brows) < 2 ** 24            # (asserted for all three block heights on the CPU as well)
        assert_same(c, f"stats ({call.brows}-row blocks)", st.reshape(exp.shape), exp.to(torch.float32))
    if call.y8 is not None:
        y8, s8 = R.mxfp8(y_stored[0])
        assert_same(c, "Y8", call.y8.read(c["name"] + " Y8")[0][0], y8)
        assert_same(c, "S8", call.s8.read(c["name"] + " S8")[0][0], s8)


_ids = lambda c: c["name"]


@pytest.mark.parametrize("c", GEMM_CASES, ids=_ids)
def test_gemm_exact(cuda, c):
    run_exact(c, cuda)


@pytest.mark.parametrize("c", CONV_CASES, ids=_ids)
def test_conv3x3_exact(cuda, c):
    run_exact(c, cuda)


@pytest.mark.parametrize("c", SUBPIXEL_CASES, ids=_ids)
def test_conv3x3_subpixel_exact(cuda, c):
    run_exact(c, cuda)


@pytest.mark.parametrize("c", TCONV_CASES, ids=_ids)
def test_tconv3_exact(cuda, c):
    """Slab-major cases (korder 1) are refused by the bf16x6 build (the header: 16-bit and bf16x3 builds): asserted as a refusal there."""
    if c.get("korder") and PLANES > 2:
        with pytest.raises(hip.MudgError):
            run_exact(c, cuda)
        return
    run_exact(c, cuda)


@pytest.mark.parametrize("c", STATS_CASES, ids=_ids)
def test_gemm_conv_tconv_stats_exact(cuda, c):
    """`stats` = sums and sums of squares of the values AS STORED.  One-hot X keeps |y| small (a few weights + biases), so that the sums
    of squares over a block stay integers below 2^24 (asserted): exact in fp32 in any order."""
    run_exact(c, cuda)


@pytest.mark.parametrize("c", FP8_CASES, ids=_ids)
def test_gemm_conv_fused_mxfp8_copy_exact(cuda, c):
    """Y8 / S8 against gemm_reference.mxfp8 of the stored Y (16-bit builds); the split builds refuse Y8 (test_gemm_refusals)."""
    run_exact(c, cuda)


@pytest.mark.parametrize("alpha", [1.0, 0.5, 2.0, 0.0])
def test_gemm_alpha_values_exact(cuda, alpha):
    """alpha in {1, 0.5, 2} and 0, which the library normalises to 1 (a zero-initialised C struct)."""
    run_exact(G(f"alpha{alpha}", 130, 72, 128, "alpha before bias", alpha=alpha, bias=True, res=F32K, out=F32K), cuda, seed=5)
    run_exact(CV(f"conv_alpha{alpha}", 2, 5, 7, 64, 72, "alpha before bias, conv", alpha=alpha, bias=True, korder=1, out=OPER), cuda, seed=6)


# ================================================================================================ bounded: random operands
def random_operands(c, seed, dt=None, planes=None):
    """X ~ N(0, 1), W ~ N(0, 0.05), rounded once to the operand type (the canonical pieces in the split builds); a residual rounded to its
    storage kind.  The linear cases carry a bias of 16 (+ N(0, 0.1) where the case has one): the sums have a deviation of 0.05 sqrt(K) <= 1.8
    and a residual one of 1, so every result lies 7 deviations away from zero and the 16-bit grid around it is coarser than 2^-8, far above
    the fp32 rounding of its terms.  Near zero, cancellation leaves an ABSOLUTE fp32 error that an ever finer 16-bit grid would resolve: the
    neighbour rule of check_16bit is a statement about one rounding, not about cancellation (signs and zeros: the exact tests).  The CPU
    file asserts the rule for plain fp32 at every shape and seed."""
    dt, planes = dt or hip.operand_dtype(), planes or PLANES
    rows, M, K, cin, taps = geometry(c)
    batch, N = c.get("batch", 1), c["N"]
    nout = N // 2 if c.get("geglu") else N
    mo = 4 * M if c.get("subpixel") else M
    x = torch.randn(batch, rows, cin, generator=gen(seed))
    w = torch.randn(4 if c.get("subpixel") else batch, N, K, generator=gen(seed + 1)) * 0.05
    xs, ws = operand_planes(x, dt, planes), operand_planes(w, dt, planes)
    gate = c.get("act") or c.get("geglu")
    bias = torch.randn(N, generator=gen(seed + 2)) * 0.1 if c.get("bias") else (None if gate else torch.zeros(N))
    if not gate:
        bias = bias + 16.0
    res = None
    if c.get("res") is not None:
        r = torch.randn(batch, mo, nout, generator=gen(seed + 3))
        rdt = {OPER: dt, F32K: torch.float32, F16K: torch.float16}[c["res"]]
        res = operand_planes(r, dt, planes) if c["res"] == OPER else [r.to(rdt).float()]
    return xs, ws, bias, res


def value_of(c, xs, ws, bias, res, dtype, kept=None):
    """The header's formula on the values the pieces add up to: contraction, alpha, bias, activation and residual all in `dtype` (fp64: the
    yardstick; fp32: what the arithmetic itself costs at that precision).  kept (2 | 3, fp64 only): the contraction a split build
    evaluates instead — the sum over the piece pairs it keeps — with everything else as the yardstick.  Returned as fp64."""
    x, w = sum(p.to(F64) for p in xs), sum(p.to(F64) for p in ws)
    r = sum(t.to(F64) for t in res) if res is not None else None
    epi = dict(act=c.get("act", False), geglu=c.get("geglu", False))
    if dtype == F64:
        s = contract_of(c)(x, w) if kept is None else R.split_kept(contract_of(c), xs, ws, kept)
        return R.epilogue(s, alpha=c.get("alpha", 1.0), bias=bias, r=r, **epi)
    y = c.get("alpha", 1.0) * (torch.matmul(x.float(), w.float().transpose(-1, -2)) if c["mode"] == 0 else _contract_f32(c, x, w))
    if bias is not None:
        y = y + bias
    if c.get("act") or c.get("geglu"):
        y = R.epilogue(y.to(F64), **epi).float()
    if r is not None:
        y = y + r.float()
    return y.to(F64)


def _contract_f32(c, x, w):
    """The conv contractions with the product in fp32: the gathers of gemm_reference are exact, so an identity weight yields the im2col
    matrix, which is then multiplied in fp32."""
    rows, M, K, cin, taps = geometry(c)
    eye = torch.eye(K, dtype=F64)[None]
    if c.get("subpixel"):
        out = torch.zeros((1, 4 * M, c["N"]), dtype=torch.float32)
        cols = contract_of(c)(x, eye.repeat(4, 1, 1))                                            # rows in output order
        for z in range(4):
            idx = R.subpixel_out_rows(c["frames"], c["h"], c["w"], z)
            out[0, idx] = cols[0, idx].float() @ w[z].float().t()
        return out
    return torch.matmul(contract_of(c)(x, eye).float(), w.float().transpose(-1, -2))


def block_sums(t, rb=32, cb=64):
    """Sums of t [b][m][n] over blocks of rb rows x cb columns; a tail shorter than a block joins the block before it, so that no block
    is a sliver in which one element is a large share."""
    b, m, n = t.shape
    ri = (torch.arange(m) // rb).clamp_max(max(m // rb - 1, 0))
    ci = (torch.arange(n) // cb).clamp_max(max(n // cb - 1, 0))
    rows = torch.zeros((b, int(ri.max()) + 1, n), dtype=F64).index_add_(1, ri, t.to(F64))
    return torch.zeros((b, rows.shape[1], int(ci.max()) + 1), dtype=F64).index_add_(2, ci, rows)


def key16(t):
    """Order-preserving integer key of 16-bit floats (sign-magnitude -> two's complement)."""
    bits = t.view(torch.int16).to(torch.int32)
    return torch.where(bits >= 0, bits, -(bits & 0x7FFF))


def flip_share(got16, want64):
    """(every element is the nearest or the other storage neighbour of the fp64 value, share of elements off the nearest one overall,
    the largest such share over the 32 x 64 blocks)."""
    near = want64.to(torch.float32).to(got16.dtype)
    direction = torch.sign(want64 - near.to(F64)).to(torch.int32)                      # where the other neighbour lies
    step = key16(got16) - key16(near)
    ok = (step == 0) | ((step == direction) & (direction != 0))
    flips = (step != 0).to(F64)
    share = block_sums(flips) / block_sums(torch.ones_like(flips))
    return ok, float(flips.mean()), float(share.max())


def check_16bit(name, got, want64):
    """got (16-bit storage) against fp64: every element on one of the two storage neighbours of the fp64 value, and per 32-row x
    64-column block at most FLIP_CAP of them off store(fp64)."""
    ok, mean, worst = flip_share(got, want64)
    rel = float((got.to(F64) - want64).norm() / want64.norm())
    print(f"[gemm {hip.operand_name()}] {name}: rel-L2 {rel:.3e}; off the nearest storage value: {mean:.5f} of all, worst 32 x 64 block {worst:.5f}, cap {FLIP_CAP}")
    bad = [(idx, float(want64[tuple(idx)]), float(got[tuple(idx)])) for idx in torch.nonzero(~ok)[:6].tolist()]
    assert bool(ok.all()), (name, "elements that are neither storage neighbour of the fp64 value: (index, fp64, got)", int((~ok).sum()), bad)
    assert worst <= FLIP_CAP, (name, worst)


def check_f32(name, got, want64, plain64):
    """The project's fp32 rule: max(2e-5, 4 x the error of the same formula in fp32 on the CPU), whole tensor and per 32 x 64 block."""
    base = float((plain64 - want64).norm() / want64.norm())
    bound = max(TOL_F32, 4.0 * base)
    d2, w2 = (got.to(F64) - want64) ** 2, want64 ** 2
    whole = float(torch.sqrt(d2.sum() / w2.sum()))
    worst = float(torch.sqrt(block_sums(d2) / block_sums(w2).clamp_min(1e-300)).max())
    print(f"[gemm {hip.operand_name()}] {name}: rel-L2 {whole:.3e}, worst 32 x 64 block {worst:.3e}, bound {bound:.3e} (cpu fp32 {base:.3e})")
    assert bool(torch.isfinite(got.float()).all()), name
    assert whole <= bound and worst <= bound, (name, whole, worst, bound)


# Four or five shapes per mode; the residual cases cover both orders of the residual add (last in the one-tile kernels; first where it
# seeds the accumulators: the 288-row tile by rule here, the 160-row tile and the persistent kernel in the variant children).
BOUNDED_CASES = [
    G("b_m129_n136_k72", 129, 136, 72, "generic loader", bias=True),
    G("b_m161_n256_k128", 161, 256, 128, "descriptor loader", res=F32K),
    G("b_m289_n320_k192_w288", 289, 320, 192, "288-row tile, residual seeds", hint=288, res=F16K, bias=True),
    G("b_m300_n328_k64_x2", 300, 328, 128, "two sources", csplit=64, alpha=0.5),
    G("b_persist_1280", 129, 1280, 1280, "persistent kernel, residual seeds", res=F32K),
    CV("b_conv_5x7", 5, 5, 7, 24, 136, "generic conv", bias=True),
    CV("b_conv_s2p0", 3, 8, 6, 64, 136, "stride 2 / pad 0", stride=2, pad=0, korder=1),
    CV("b_conv_xs_w7", 3, 9, 7, 128, 136, "XSHARE", korder=1, res=F16K),
    CV("b_conv_w288", 1, 12, 24, 64, 320, "288-row tile conv, residual seeds", res=F32K, bias=True),
    CV("b_conv_sub_5x8", 2, 5, 8, 64, 72, "sub-pixel", subpixel=1, korder=1, bias=True),
    TC("b_tconv_t3", 3, 3, 15, 24, 136, "generic temporal conv", bias=True),
    TC("b_tconv_t16", 2, 16, 5, 64, 72, "descriptor loader", res=F32K),
    TC("b_tconv_k1_hw24", 2, 16, 24, 64, 136, "slab-major", korder=1, res=F16K),
    TC("b_tconv_w288", 1, 2, 288, 64, 320, "288-row tile", res=F16K),
]
# 16-bit results: operand storage in the 16-bit builds, fp16 storage in every build — both under the neighbour + flip-cap rule.  In the
# split builds operand storage holds 16 / 24 significand bits: the fp32 rule covers it through the fp32 output of the same problem.
# bf16x3 drops the (1,1) piece pair by design (csrc/common.h): the CPU file asserts that this alone, like plain fp32, stays under a
# quarter of the cap at every shape and seed.
BOUNDED_KINDS = [OPER, F16K, F32K] if not SPLIT else [F16K, F32K]
if PLANES > 2:      # slab-major temporal convs are refused by the bf16x6 build (asserted in test_tconv3_exact)
    BOUNDED_CASES = [c for c in BOUNDED_CASES if not (c["mode"] == 2 and c.get("korder"))]


def bounded_seed(c):
    return 100 + sum(map(ord, c["name"]))


@pytest.mark.parametrize("c", BOUNDED_CASES, ids=_ids)
def test_gemm_conv_tconv_bounded_linear(cuda, c):
    xs, ws, bias, res = random_operands(c, seed=bounded_seed(c))
    want = value_of(c, xs, ws, bias, res, F64)
    plain = value_of(c, xs, ws, bias, res, torch.float32)
    for kind in BOUNDED_KINDS:
        cc = dict(c, out=kind)
        call = Call(cc, xs, ws, bias, None, res, cuda)
        if refused_without_the_descriptor_loader(cc, call):
            continue
        got = call.run()
        name = f"{c['name']} out {('operand', 'fp32', 'fp16')[kind]}"
        if kind == F32K:
            check_f32(name, got[0], want, plain)
        else:
            check_16bit(name, got[0], want)


GEGLU_BOUNDED = [
    G("bg_n64_k72", 129, 64, 72, "generic loader", geglu=True, bias=True),
    G("bg_n256_k128", 200, 256, 128, "persistent kernel", geglu=True, bias=True),
    G("bg_n512_k640_w288", 289, 512, 640, "288 x 256 tile", geglu=True, bias=True, hint=288),
    G("bg_act_n136", 129, 136, 64, "plain GELU", act=True, bias=True),
]


@pytest.mark.parametrize("c", GEGLU_BOUNDED, ids=_ids)
def test_geglu_gelu_bounded_random(cuda, c):
    """16-bit GELU / GEGLU results on random data (operand storage in the 16-bit builds, fp16 storage in every build): per 32-row block,
    rel-L2 <= 3 x the distance from fp64 of store(fp64) (as the attention file does); the split builds' fp32 output under the fp32 rule."""
    xs, ws, bias, res = random_operands(c, seed=300 + len(c["name"]))
    want = value_of(c, xs, ws, bias, res, F64)
    if SPLIT:
        got = Call(dict(c, out=F32K), xs, ws, bias, None, res, cuda).run()[0]
        # the same formula in fp32 — plus, bf16x3, the documented 1.5e-7 of its erf polynomial, far below 2e-5
        check_f32(c["name"] + " out fp32", got, want, value_of(c, xs, ws, bias, res, torch.float32))
    for kind in ((F16K,) if SPLIT else (OPER, F16K)):
        got = Call(dict(c, out=kind), xs, ws, bias, None, res, cuda).run()[0].to(F64)
        near = want.to(torch.float32).to(kind_dtype(kind)).to(F64)
        m = want.shape[1]
        mp = (m + 31) // 32 * 32
        blk = lambda t: torch.nn.functional.pad((t ** 2).sum(2), (0, mp - m)).reshape(-1, 32).sum(1)
        ref = torch.sqrt(blk(near - want) / blk(want).clamp_min(1e-300))
        err = torch.sqrt(blk(got - want) / blk(want).clamp_min(1e-300))
        worst = int((err / ref.clamp_min(1e-300)).argmax())
        print(f"[gemm {hip.operand_name()}] {c['name']} out {('operand', 'fp32', 'fp16')[kind]}: worst 32-row block rel-L2 {float(err[worst]):.3e}, "
              f"bound {3 * float(ref[worst]):.3e} (3 x storage rounding {float(ref[worst]):.3e})")
        assert bool((err <= 3.0 * ref).all()), (c["name"], kind, float(err[worst]), float(ref[worst]))


def phi_error_bound(geglu):
    """|Phi_kernel - Phi| the documented scheme allows (csrc/gemm_shared.h), before the 2 x margin.
    table (GEGLU, 16-bit builds): linear interpolation at h = 1/64: h^2 / 8 max|Phi''| = (1/64)^2 / 8 * phi(1) = 7.39e-6 (max |x phi(x)| is at
        x = 1: 0.24197), + the fp32 rounding of two table entries and of the fma (3 x 2^-24).
    polynomial (plain GELU in the 16-bit builds; everything in bf16x3, whose cubic table lookup is held to the same figure): A&S 7.1.26,
        |erf error| <= 1.5e-7, halved by Phi = (1 + erf) / 2: 0.75e-7, + fp32 evaluation (reciprocal, five fmas, __expf, 1 - p t e: 4 x 2^-24).
    erff (bf16x6): fp32 rounding only: erff to 2 ulp of a value <= 1 (2^-23, halved) + the add and the halving (2 x 2^-24)."""
    u = 2.0 ** -24
    if PLANES == 3:
        return "erff", 2.0 ** -24 + 2 * u
    if PLANES == 2 or not geglu:
        return "polynomial", 0.75e-7 + 4 * u
    return "table", (1.0 / 64) ** 2 / 8 * 0.24197072451914337 + 3 * u


def gate_sweep():
    """Two-hot X: row m selects a fine offset (m % 8) and a shift ((m // 8) % 8); gate[m][j] = fine + shift + bias_g[j] EXACTLY (every term
    has few bits: the weights fit bf16, the sums fit fp32).  bias_g[j] = -8 + j / 16, j < 256: with the fine offsets {0 .. 3} / 64 and their
    midpoints (+ 1/128) every grid point i / 64 of [-8, 8) and every midpoint appears, with the shifts 0, +-2^-10, 1/16 (-> 8 exactly; 8 -
    1/64 = 7.9375 + 3/64), -2 and 2.0625 (-> -10 and 10)."""
    fine = [a / 64 + b / 128 for b in range(2) for a in range(4)]
    shift = [0.0, 2.0 ** -10, -2.0 ** -10, 1 / 16, -2.0, 2.0625, 1.0, -1 / 64]
    return fine, shift


@pytest.mark.parametrize("geglu", [True, False], ids=["geglu", "gelu"])
def test_gelu_geglu_gate_sweep(cuda, geglu):
    """|Y - v g Phi(g)| against fp64 erfc over gates in [-10, 10] (0, +-2^-10, +-8, +-(8 - 1/64), every table node and midpoint included),
    fp32 output.  Bound per element = 2 x (|v g| * phi_error_bound + |v g Phi(g)| * 2^-23): the scheme's error in Phi, and two fp32
    roundings of the products.  The measured maximum of error / bound is printed; a kernel over the bound is a finding."""
    fine, shift = gate_sweep()
    K, nout, M = 64, 256, 64
    N = 2 * nout if geglu else nout
    x = torch.zeros((1, M, K))
    m = torch.arange(M)
    x[0, m, m % 8] = 1.0
    x[0, m, 8 + (m // 8) % 8] = 1.0
    w = torch.zeros((1, N, K))
    bias = torch.zeros(N)
    j = torch.arange(nout)
    vrow, grow = R.geglu_unpack(nout) if geglu else (None, j)
    w[0, grow, :8] = torch.tensor(fine)
    w[0, grow, 8:16] = torch.tensor(shift)
    bias[grow] = -8.0 + j.float() / 16
    if geglu:
        bias[vrow] = ((j % 5).float() - 2.0) * 0.75 + 0.25                                       # v in {-1.25, -0.5, 0.25, 1.0, 1.75}
    dt = hip.operand_dtype()
    assert torch.equal(w.to(dt).float(), w)
    xs, ws = operand_planes(x, dt, PLANES), operand_planes(w, dt, PLANES)
    c = G("sweep_geglu" if geglu else "sweep_gelu", M, N, K, "gate sweep", geglu=geglu, act=not geglu, out=F32K)
    got = Call(c, xs, ws, bias, None, None, cuda).run()[0].to(F64)
    pre = R.contract_gemm(x, w) + bias.to(F64)
    g = pre[..., grow]
    for point in (0.0, 2.0 ** -10, -2.0 ** -10, 8.0, -8.0, 8 - 1 / 64, -(8 - 1 / 64), 10.0, -10.0, 3 / 64, 3 / 64 + 1 / 128):
        assert bool((g == point).any()), point
    v = pre[..., vrow] if geglu else torch.ones_like(g)
    phi = 0.5 * torch.erfc(-g / math.sqrt(2.0))
    want = v * g * phi
    scheme, perr = phi_error_bound(geglu)
    bound = 2.0 * ((v * g).abs() * perr + want.abs() * 2.0 ** -23)
    err = (got - want).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio[(bound == 0) & (err == 0)] = 0
    at = int(ratio.argmax())
    print(f"[gemm {hip.operand_name()}] {c['name']} ({scheme}): max |error| {float(err.max()):.3e}; worst error / bound {float(ratio.max()):.3f} at gate "
          f"{float(g.reshape(-1)[at]):.6f} (|error| {float(err.reshape(-1)[at]):.3e}, bound {float(bound.reshape(-1)[at]):.3e}); rel-L2 {float((got - want).norm() / want.norm()):.3e}")
    assert bool((err <= bound).all()), (scheme, float(ratio.max()), float(g.reshape(-1)[at]))


# ================================================================================================ refusals
def _plain_desc(dev, M=64, N=64, K=64, mode=0):
    pl = PLANES
    bufs = [torch.zeros((M + 8, pl * (K + 8)), dtype=hip.operand_dtype(), device=dev), torch.zeros((N + 8, pl * (K + 8)), dtype=hip.operand_dtype(), device=dev),
            torch.zeros((4 * M + 8, pl * (N + 8)), dtype=hip.operand_dtype(), device=dev), torch.zeros((4 * M + 8, N + 8), dtype=torch.float32, device=dev)]
    d = hip.GemmDesc()
    d.X, d.W, d.Y = bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr()
    d.M, d.N, d.K, d.ldx, d.ldw, d.ldy = M, N, K, pl * (K + 8), pl * (K + 8), pl * (N + 8)
    d.csplit, d.batch, d.alpha, d.mode = K, 1, 1.0, mode
    return d, bufs


def _conv_desc(dev, **over):
    d, bufs = _plain_desc(dev, M=2 * 4 * 4, N=64, K=9 * 64, mode=1)
    d.Hin = d.Win = d.Hout = d.Wout = 4
    d.Cin, d.stride, d.pad, d.csplit = 64, 1, 1, 64
    for k, v in over.items():
        setattr(d, k, v)
    return d, bufs


def test_gemm_refusals(cuda):
    """Each MUDG_REQUIRE of mudg_gemm that no other test triggers: the call returns an error whose text (mudg_last_error, as hip.check
    raises it) names the clause, and launches nothing."""
    import re
    lib = hip.lib()

    def refused(message, d, bufs):
        with pytest.raises(hip.MudgError, match=re.escape(message)):
            hip.check(lib.mudg_gemm(C.byref(d), _s()), "mudg_gemm")

    def gemm_with(**over):
        d, bufs = _plain_desc(cuda)
        for k, v in over.items():
            setattr(d, k, v)
        return d, bufs

    refused("K=60 must be a multiple of 8", *gemm_with(K=60))
    refused("empty problem", *gemm_with(M=0))
    refused("mudg_gemm: mode 3", *gemm_with(mode=3))
    refused("must be multiples of", *gemm_with(ldx=PLANES * 72 + 4))
    refused("batch strides must be multiples of 8", *gemm_with(batch=2, sX=12))
    d, bufs = _plain_desc(cuda)
    d.X = d.X + 2
    refused("X/W must be 16-byte aligned", d, bufs)
    d, bufs = _plain_desc(cuda)
    d.W = d.W + 8
    refused("X/W must be 16-byte aligned", d, bufs)
    for csplit in (4, 0, 64):                                  # not a multiple of 8; empty first source; empty second source
        d, bufs = _plain_desc(cuda)
        d.X2, d.ldx2, d.csplit = bufs[0].data_ptr(), d.ldx, csplit
        refused(f"csplit={csplit}", d, bufs)
    d, bufs = _plain_desc(cuda)
    d.X2, d.ldx2, d.csplit = bufs[0].data_ptr() + 2, d.ldx, 32
    refused("X2 alignment", d, bufs)
    refused("geglu needs N % 64 == 0", *gemm_with(geglu=1, N=32))
    fb = torch.zeros(4096, dtype=torch.float32, device=cuda)
    refused("gbias combines with neither act nor geglu", *gemm_with(gbias=fb.data_ptr(), rows_per_group=64, act=1))
    refused("gbias combines with neither act nor geglu", *gemm_with(gbias=fb.data_ptr(), rows_per_group=64, geglu=1))
    refused("gbias needs rows_per_group", *gemm_with(gbias=fb.data_ptr(), rows_per_group=0))
    refused("gbias needs rows_per_group", *gemm_with(gbias=fb.data_ptr(), rows_per_group=64, batch=2))
    refused("stats needs batch == 1 and no GEGLU", *gemm_with(stats=fb.data_ptr(), batch=2))
    refused("stats needs batch == 1 and no GEGLU", *gemm_with(stats=fb.data_ptr(), geglu=1))
    refused("out_fp32 / res_fp32 are 0", *gemm_with(out_fp32=3))
    refused("out_fp32 / res_fp32 are 0", *gemm_with(res_fp32=-1))
    y8 = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
    fp8 = dict(Y8=y8.data_ptr(), S8=y8.data_ptr() + 32768, ldy8=64, lds8=2)
    if SPLIT:
        refused("the fused fp8 copy belongs to the 16-bit builds", *gemm_with(**fp8))
        refused(f"ldy={PLANES * 72 + 1} must be a multiple of {PLANES}", *gemm_with(ldy=PLANES * 72 + 1))
        refused(f"ldr={PLANES * 72 + 1} must be a multiple of {PLANES}", *gemm_with(R=bufs[2].data_ptr(), ldr=PLANES * 72 + 1))
        refused("split operands need ld", *gemm_with(ldx=8 * PLANES * (64 // 8 - 1)))
    else:
        # one require, one message: every clause of it broken on its own
        for over in (dict(S8=None), dict(out_fp32=1), dict(N=48), dict(ldy8=68), dict(ldy8=56), dict(lds8=1), dict(Y8=y8.data_ptr() + 4),
                     dict(geglu=1), dict(batch=2)):
            refused("Y8 needs S8", *gemm_with(**dict(fp8, **over)))
    # mode 1
    refused("conv K=512 Cin=64", *_conv_desc(cuda, K=8 * 64))
    # (K = 9 Cin is a multiple of 8 only with Cin: the Cin % 8 clause is reachable through the sub-pixel form's K = 4 Cin)
    refused("conv K=48 Cin=12", *_conv_desc(cuda, subpixel=1, batch=4, korder=1, Cin=12, K=48, csplit=12))
    refused("mudg_gemm: stride 3", *_conv_desc(cuda, stride=3))
    refused("upsample needs stride 1", *_conv_desc(cuda, upsample=1, stride=2))
    refused("conv geometry", *_conv_desc(cuda, Hout=0))
    refused("mudg_gemm: pad 2", *_conv_desc(cuda, pad=2))
    d, bufs = _plain_desc(cuda, M=32, N=64, K=9 * 72, mode=1)
    d.Hin = d.Win = d.Hout = d.Wout = 4
    d.Cin, d.stride, d.pad, d.csplit, d.korder = 72, 1, 1, 72, 1
    refused("korder=1 needs Cin % 64 == 0", d, bufs)
    refused("M not a whole number of frames", *_conv_desc(cuda, M=2 * 16 + 3))

    # mode 2
    def tconv_with(**over):
        dd, bb = _plain_desc(cuda, M=2 * 4 * 8, N=64, K=3 * 64, mode=2)
        dd.Cin, dd.T, dd.HW, dd.csplit = 64, 4, 8, 64
        for k, v in over.items():
            setattr(dd, k, v)
        return dd, bb

    refused("tconv K=128 Cin=64", *tconv_with(K=2 * 64))
    refused("tconv geometry", *tconv_with(M=2 * 4 * 8 + 8))
    refused("tconv geometry", *tconv_with(T=0))
    refused("temporal conv with korder = 1 needs T = 16", *tconv_with(korder=1))
    refused("temporal conv with korder = 1 needs T = 16", *tconv_with(korder=1, T=16, HW=4, M=64))
    # (bf16x6 refuses every slab-major temporal conv with the message before)
    refused("temporal conv with korder = 1 " + ("takes a group bias per clip" if PLANES <= 2 else "needs T = 16"),
            *tconv_with(korder=1, T=16, HW=8, M=128, gbias=fb.data_ptr(), rows_per_group=64))
    torch.cuda.synchronize()


def test_conv_subpixel_ok_contract(cuda):
    """mudg_conv_subpixel_ok: 1 for the stated form, 0 for each clause of its contract broken on its own; mudg_gemm refuses what it refuses."""
    lib = hip.lib()

    def desc(**over):
        d, bufs = _plain_desc(cuda, M=2 * 4 * 4, N=64, K=4 * 64, mode=1)
        d.Hin = d.Win = d.Hout = d.Wout = 4
        d.Cin, d.stride, d.pad, d.csplit, d.korder, d.subpixel, d.batch = 64, 1, 1, 64, 1, 1, 4
        d.sW = 64 * d.ldw
        for k, v in over.items():
            setattr(d, k, v)
        return d, bufs

    d, bufs = desc()
    assert lib.mudg_conv_subpixel_ok(C.byref(d)) == (1 if subpixel_available() else 0)
    assert lib.mudg_conv_subpixel_ok(None) == 0
    fb = torch.zeros(4096, dtype=torch.float32, device=cuda)
    broken = dict(batch=dict(batch=1), stride=dict(stride=2), pad=dict(pad=0), korder=dict(korder=0), upsample=dict(upsample=1), mode=dict(mode=0),
                  not_subpixel=dict(subpixel=0), X2=dict(X2=fb.data_ptr()), R=dict(R=fb.data_ptr()), gbias=dict(gbias=fb.data_ptr()),
                  stats=dict(stats=fb.data_ptr()), geglu=dict(geglu=1), sX=dict(sX=64), sY=dict(sY=64), Hout=dict(Hout=8), Wout=dict(Wout=2),
                  K=dict(K=9 * 64), Cin=dict(Cin=32, K=128), reach=dict(ldx=1 << 30))
    for name, over in broken.items():
        d, bufs = desc(**over)
        assert lib.mudg_conv_subpixel_ok(C.byref(d)) == 0, name
    for name in ("batch", "korder", "sX", "Hout"):
        d, bufs = desc(**broken[name])
        with pytest.raises(hip.MudgError, match="subpixel needs batch 4"):
            hip.check(lib.mudg_gemm(C.byref(d), _s()), name)
    torch.cuda.synchronize()
