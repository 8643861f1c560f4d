"""Tensor-level wrappers over the C-ABI: torch tensors are used purely as device buffers (pointer, stride,
stream); every arithmetic result on the hot path comes out of a HIP kernel in libmudg_hip.so.

Activations are "rows" matrices: 2-D bf16 tensors [pixels, channels] whose row stride may exceed the channel
count (views into wider buffers are fine as long as stride(1) == 1 and rows are 16-byte aligned).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import hip



def H16():
    """torch dtype of the 16-bit MFMA operands of the loaded library (bf16 by default, fp16 with MUDG_OPERAND=fp16)."""
    return hip.operand_dtype()


def STREAM():
    """torch dtype of the residual stream — the tensors later layers add onto (block outputs, the transformers' token
    stream, encoder skips): fp16 with bf16 operands (2 bytes per value through HBM; its 11 significand bits keep the ~150
    residual adds below the bf16 operand rounding, and the reference's own stream is fp16 under torch.autocast), fp32 in
    the accuracy-oriented modes — fp16 operands (an fp16 stream measured +35 % error per forward there: 2.0e-3 -> 2.7e-3)
    and the split-operand precision builds.  MUDG_STREAM=fp32 forces fp32."""
    import os
    if hip.operand_name() != "bf16" or os.environ.get("MUDG_STREAM", "").lower() == "fp32":
        return torch.float32
    return torch.float16


def kind(t) -> int:
    """Storage code of a rows matrix for the C-ABI (out_fp32 / res_fp32 / x_fp32 ...): 0 operand, 1 fp32, 2 fp16."""
    if t.dtype == torch.float32:
        return 1
    if t.dtype == H16():
        return 0
    if t.dtype == torch.float16:
        return 2
    raise hip.MudgError(f"no storage code for {t.dtype}")


def _out_dtype(out_fp32, out_stream):
    return torch.float32 if out_fp32 else (STREAM() if out_stream else H16())


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _rows(t: torch.Tensor, dtype=None) -> torch.Tensor:
    dtype = dtype or H16()
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype != dtype or not t.is_cuda:
        raise hip.MudgError(f"expected a cuda {dtype} rows matrix with unit channel stride, got "
                            f"{tuple(t.shape)} {t.dtype} strides {t.stride()} on {t.device}")
    return t


def empty_rows(rows: int, cols: int, dtype=None, device=None) -> torch.Tensor:
    """A rows matrix.  Operand matrices of the split-operand builds (hip.planes() > 1) are allocated planes * cols wide
    and returned as the [rows, cols] view of piece 0: piece p of a row starts stride(0) / planes elements further, which
    every column slice of the view inherits (the kernels derive the plane distance from the row stride)."""
    dtype = dtype or H16()
    planes = hip.planes() if dtype == H16() else 1
    if planes > 1:
        return torch.empty((rows, planes * cols), dtype=dtype, device=device or "cuda")[:, :cols]
    return torch.empty((rows, cols), dtype=dtype, device=device or "cuda")


def repeat_rows(t, times):
    """`times` copies of a rows matrix stacked along the rows (batch-major rows: the batch repeated).  GroupNorm partial
    sums hanging on `t` (one set per 128-row block) are repeated with it when the blocks line up."""
    if times == 1:
        return t
    rows, cols = t.shape
    out = empty_rows(times * rows, cols, t.dtype, t.device)
    src, dst = t, out
    if out._base is not None:            # an operand matrix of a split-operand build: every piece is copied
        if t._base is None or tuple(t._base.shape) != (rows, out._base.shape[1]):
            raise hip.MudgError("repeat_rows: not a whole operand matrix")
        src, dst = t._base, out._base
    for i in range(times):
        dst[i * rows:(i + 1) * rows].copy_(src)
    ws = getattr(t, GN_ATTR, None)
    brows = getattr(t, GN_ATTR + "_rows", 128)
    if ws is not None and getattr(t, GN_ATTR + "_version", -1) == _version(t) and rows % brows == 0 and not getattr(t, GN_ATTR + "_clips", 0):
        setattr(out, GN_ATTR, ws.repeat(times, 1, 1))
        setattr(out, GN_ATTR + "_version", _version(out))
        setattr(out, GN_ATTR + "_rows", brows)
    return out


# ------------------------------------------------------------------------------------------------ GEMM family
GN_ATTR = "_mudg_gn_partials"      # python attribute a producer leaves on its output: fp32 [ceil(M/rows)][N][2] partial sums per block of
                                   # `rows` rows (attribute GN_ATTR + "_rows": 128, or 288 where the 288 x 320-tile kernel ran the problem)


def _drop_stats(t):
    """A kernel is about to write into `t` through its raw pointer (torch's version counter does not see that): partial
    sums a previous producer hung on it would be stale."""
    if t is not None and getattr(t, GN_ATTR, None) is not None:
        setattr(t, GN_ATTR, None)
        setattr(t, GN_ATTR + "_clips", 0)


def _version(t):
    try:
        return t._version
    except RuntimeError:            # inference tensors do not track versions
        return 0


def _attach_stats(d, out, M, nout):
    """Ask the epilogue for GroupNorm partials of `out` (MudgGemmDesc.stats) and hang them on the tensor.  Call it on the finished
    descriptor: the height of the partial blocks depends on which kernel the library will run (mudg_gemm_stats_rows)."""
    brows = hip.lib().mudg_gemm_stats_rows(C.byref(d))
    ws = torch.empty(((M + brows - 1) // brows, nout, 2), dtype=torch.float32, device=out.device)
    d.stats = ws.data_ptr()
    setattr(out, GN_ATTR + "_rows", brows)
    setattr(out, GN_ATTR, ws)
    setattr(out, GN_ATTR + "_version", _version(out))     # a later torch in-place op on `out` invalidates the partials
    setattr(out, GN_ATTR + "_clips", 0)                   # (the tiling tag of an earlier slab-major tconv3 into the same `out=` is stale)


def gemm(x, w, *, out=None, bias=None, gbias=None, rows_per_group=0, residual=None, x2=None, geglu=False,
         out_fp32=False, alpha=1.0, batch=1, sx=0, sw=0, sy=0, sr=0, M=None, N=None, K=None, ldy=None, gelu=False,
         stats=False, out_stream=False, fp8=False, frame_rows=0):
    """out[m, n] = epilogue(alpha * sum_k x[m, k] w[n, k]); see MudgGemmDesc.  frame_rows: a hint — the rows of one frame of x
    (results never depend on it; it lets the library pick a tile height that divides a frame).  The result is an MFMA operand matrix by
    default, fp32 with out_fp32, the residual-stream dtype (STREAM()) with out_stream; `out=` decides by its dtype.
    fp8=True (16-bit builds, operand result, N % 32 == 0): returns (out, e4m3 bytes [M, N] uint8, E8M0 scales [M, N / 32] uint8) —
    the MX-fp8 copy of the result written by the same epilogue (MudgGemmDesc.Y8), bit-equal to quantize_mxfp8(out)."""
    _rows(x); _rows(w)
    if M is None:
        M = x.shape[0]
    if N is None:
        N = w.shape[0]
    if K is None:
        K = w.shape[1]
    nout = N // 2 if geglu else N
    if out is None:
        out = empty_rows(M, nout, _out_dtype(out_fp32, out_stream), x.device)
    else:
        _drop_stats(out)
    d = hip.GemmDesc()
    d.X, d.X2, d.W, d.Y = x.data_ptr(), _ptr(x2), w.data_ptr(), out.data_ptr()
    d.bias, d.gbias, d.R = _ptr(bias), _ptr(gbias), _ptr(residual)
    d.M, d.N, d.K = M, N, K
    d.ldx, d.ldw = x.stride(0), w.stride(0)
    d.ldx2 = x2.stride(0) if x2 is not None else 0
    d.ldy = ldy if ldy is not None else out.stride(0)
    d.ldr = residual.stride(0) if residual is not None else 0
    d.csplit = x.shape[1] if x2 is not None else K
    d.batch, d.sX, d.sW, d.sY, d.sR = batch, sx, sw, sy, sr
    d.rows_per_group, d.out_fp32, d.geglu, d.alpha, d.mode = rows_per_group, kind(out), int(geglu), alpha, 0
    d.res_fp32 = kind(residual) if residual is not None else 0
    d.act = int(gelu)
    d.HW = int(frame_rows)
    if fp8:
        y8 = torch.empty((M, nout), dtype=torch.uint8, device=x.device)
        s8 = torch.empty((M, nout // 32), dtype=torch.uint8, device=x.device)
        d.Y8, d.S8, d.ldy8, d.lds8 = y8.data_ptr(), s8.data_ptr(), y8.stride(0), s8.stride(0)
    if stats:
        _attach_stats(d, out, M, nout)
    hip.check(hip.lib().mudg_gemm(C.byref(d), _stream()), "mudg_gemm")
    return (out, y8, s8) if fp8 else out


def conv3x3(x, w, *, frames, hin, win, cin, stride=1, upsample=False, out=None, bias=None, gbias=None,
            rows_per_group=0, residual=None, x2=None, out_fp32=False, korder=0, pad=1, stats=False, out_stream=False):
    """3x3 / pad 1 convolution on channels-last rows; w is packed [Cout][9*cin], K axis tap-major (korder 0) or
    64-channel-slab-major (korder 1, see MudgGemmDesc.korder)."""
    _rows(x); _rows(w)
    if upsample:
        hout, wout = 2 * hin, 2 * win
    elif pad == 1:
        hout, wout = (hin - 1) // stride + 1, (win - 1) // stride + 1
    else:       # pad 0 with one trailing zero row / column: AutoencoderKL's downsample
        hout, wout = (hin + 1 - 3) // stride + 1, (win + 1 - 3) // stride + 1
    M, N = frames * hout * wout, w.shape[0]
    if out is None:
        out = empty_rows(M, N, _out_dtype(out_fp32, out_stream), x.device)
    else:
        _drop_stats(out)
    d = hip.GemmDesc()
    d.X, d.X2, d.W, d.Y = x.data_ptr(), _ptr(x2), w.data_ptr(), out.data_ptr()
    d.bias, d.gbias, d.R = _ptr(bias), _ptr(gbias), _ptr(residual)
    d.out_fp32 = kind(out)
    d.res_fp32 = kind(residual) if residual is not None else 0
    d.M, d.N, d.K = M, N, 9 * cin
    d.ldx, d.ldw, d.ldy = x.stride(0), w.stride(0), out.stride(0)
    d.ldx2 = x2.stride(0) if x2 is not None else 0
    d.ldr = residual.stride(0) if residual is not None else 0
    d.csplit = x.shape[1] if x2 is not None else cin
    d.batch, d.rows_per_group, d.alpha, d.mode = 1, rows_per_group, 1.0, 1
    d.Hin, d.Win, d.Hout, d.Wout, d.Cin, d.stride, d.upsample = hin, win, hout, wout, cin, stride, int(upsample)
    d.korder, d.pad = korder, pad
    if stats:
        _attach_stats(d, out, M, N)
    hip.check(hip.lib().mudg_gemm(C.byref(d), _stream()), "mudg_gemm[conv3x3]")
    return out


def conv3x3_up2(x, wsub, *, frames, hin, win, cin, bias=None, out_fp32=False, out_stream=False):
    """Nearest-2x upsample followed by a 3x3 / pad 1 conv in the sub-pixel form — four 2x2 convs on the low-resolution
    image, 4/9 of the multiply-adds (MudgGemmDesc.subpixel; `wsub` from packing.conv3x3_subpixel).  Returns None when the
    problem is outside what the descriptor loader accepts: the caller then runs conv3x3(upsample=True) with the 3x3 weights."""
    _rows(x); _rows(wsub)
    N = wsub.shape[0] // 4
    M = frames * hin * win
    d = hip.GemmDesc()
    d.X, d.W, d.bias = x.data_ptr(), wsub.data_ptr(), _ptr(bias)
    d.M, d.N, d.K = M, N, 4 * cin
    d.ldx, d.ldw = x.stride(0), wsub.stride(0)
    d.csplit, d.batch, d.alpha, d.mode = cin, 4, 1.0, 1
    d.sW = N * wsub.stride(0)
    d.Hin, d.Win, d.Hout, d.Wout, d.Cin, d.stride, d.upsample = hin, win, hin, win, cin, 1, 0
    d.korder, d.pad, d.subpixel = 1, 1, 1
    if not hip.lib().mudg_conv_subpixel_ok(C.byref(d)):
        return None
    out = empty_rows(4 * M, N, _out_dtype(out_fp32, out_stream), x.device)
    d.Y, d.ldy, d.out_fp32 = out.data_ptr(), out.stride(0), kind(out)
    hip.check(hip.lib().mudg_gemm(C.byref(d), _stream()), "mudg_gemm[conv3x3 subpixel]")
    return out


def tconv3_slab_ok(t, hw, cin):
    """Whether mudg_gemm accepts korder = 1 for this temporal conv (MudgGemmDesc.korder, mode 2)."""
    return hip.planes() <= 2 and t == 16 and hw % 8 == 0 and cin % 64 == 0


def tconv3_wide(t, hw, cin, cout):
    """Whether the library runs this temporal conv (plain K order, korder 0) on a tile kernel of wgemm.hip (288 x 320 or 160 x 320) — the caller then does not
    ask for the slab-major order, whose 8-pixel x 16-frame tiles belong to the 128 x 128 kernels.  A dry query: nothing is read.
    Not cached: it is one host call, and the variant builds re-read MUDG_GEMM_W288 at every call (a cached answer went stale when a
    test toggled the switch in-process).  The query assumes what the executor always passes — dense, 16-byte-aligned rows; a caller
    with other strides gets a correct result either way (ops.tconv3 asks again with the real descriptor for the GroupNorm block
    height), only possibly the slower of the two K orders."""
    d = hip.GemmDesc()
    d.X, d.W, d.Y = 256, 256, 256                     # aligned placeholders
    d.M, d.N, d.K = 16 * t * hw, cout, 3 * cin
    pl = hip.planes()
    d.ldx, d.ldw, d.ldy = pl * cin, pl * 3 * cin, pl * cout
    d.csplit, d.batch, d.alpha, d.mode = cin, 1, 1.0, 2
    d.Cin, d.T, d.HW = cin, t, hw
    return hip.lib().mudg_gemm_stats_rows(C.byref(d)) != 128       # 288 or 160: a tile kernel of wgemm.hip


def tconv3(x, w, *, clips, t, hw, cin, out=None, bias=None, residual=None, out_fp32=False, stats=False, out_stream=False, korder=0):
    """(3,1,1) temporal convolution, pad (1,0,0), on rows ordered ((b t) hw); w packed [Cout][3*cin], K axis [tap][cin] (korder 0)
    or [cin/64][tap][64] (korder 1: 16-frame clips; the kernels then tile a clip as 8 pixels x 16 frames and stage a 64-channel slab
    once for the three taps).  With korder = 1 the GroupNorm partials of `stats` are per such TILE, not per 128 consecutive rows:
    they are tagged and only a clip-level GroupNorm (samples = clips) takes them."""
    _rows(x); _rows(w)
    M, N = clips * t * hw, w.shape[0]
    if out is None:
        out = empty_rows(M, N, _out_dtype(out_fp32, out_stream), x.device)
    else:
        _drop_stats(out)
    d = hip.GemmDesc()
    d.X, d.W, d.Y = x.data_ptr(), w.data_ptr(), out.data_ptr()
    d.bias, d.R = _ptr(bias), _ptr(residual)
    d.out_fp32 = kind(out)
    d.res_fp32 = kind(residual) if residual is not None else 0
    d.M, d.N, d.K = M, N, 3 * cin
    d.ldx, d.ldw, d.ldy = x.stride(0), w.stride(0), out.stride(0)
    d.ldr = residual.stride(0) if residual is not None else 0
    d.csplit, d.batch, d.alpha, d.mode = cin, 1, 1.0, 2
    d.Cin, d.T, d.HW = cin, t, hw
    d.korder = korder
    if stats:
        _attach_stats(d, out, M, N)
        setattr(out, GN_ATTR + "_clips", clips if korder else 0)
    hip.check(hip.lib().mudg_gemm(C.byref(d), _stream()), "mudg_gemm[tconv3]")
    return out


# ------------------------------------------------------------------------------------------------ attention
def attention(q, k, vt, out, *, frames, heads, nq, nk, ldvt=None, svt=None, kv_div=1, scale=0.125, accumulate=False,
              k2=None, vt2=None, nk2=0, ldvt2=None, svt2=None, kv_div2=1, q_prescaled=False, fp8=None, lse=None):
    """vt: V^T as [kv batches * heads * 64, keys] rows (row stride = ldvt, batch stride = heads * 64 rows by default).
    k2 / vt2 / nk2: an optional second key / value set with its own softmax whose output is added (the image tokens of
    the text + image cross-attention), in the same launch.  q_prescaled: q already carries scale * log2(e) (folded into
    the packed q-projection weights); `scale` is then ignored and long self-attention runs its lean softmax.
    fp8 = (q8, qs, k8, ks) from quantize_mxfp8: Q K^T on the MX-fp8 MFMA (long self-attention, needs q_prescaled)."""
    if ldvt is None:
        ldvt = vt.stride(0)
    if svt is None:
        svt = heads * 64 * ldvt
    _drop_stats(out)
    d = hip.AttnDesc()
    d.Q, d.K, d.Vt, d.O = q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr()
    d.F, d.heads, d.Nq, d.Nk = frames, heads, nq, nk
    d.ldq, d.ldk, d.ldvt, d.ldo = q.stride(0), k.stride(0), ldvt, out.stride(0)
    d.svt, d.kv_div, d.scale, d.accumulate = svt, kv_div, scale, int(accumulate)
    d.q_prescaled = int(q_prescaled)
    if lse is not None:              # fp32 [frames * nq][heads]: the softmax statistics the training backward pass reuses
        if lse.dtype != torch.float32 or tuple(lse.shape) != (frames * nq, heads) or not lse.is_contiguous():
            raise hip.MudgError("attention: lse must be a contiguous fp32 [frames * nq][heads] tensor")
        d.Lse = lse.data_ptr()
    if fp8 is not None:
        q8, qs, k8, ks = fp8
        d.Q8, d.Qs, d.K8, d.Ks = q8.data_ptr(), qs.data_ptr(), k8.data_ptr(), ks.data_ptr()
        d.ldq8, d.ldqs, d.ldk8, d.ldks = q8.stride(0), qs.stride(0), k8.stride(0), ks.stride(0)
    if k2 is not None:
        d.K2, d.Vt2, d.Nk2, d.ldk2 = k2.data_ptr(), vt2.data_ptr(), nk2, k2.stride(0)
        d.ldvt2 = vt2.stride(0) if ldvt2 is None else ldvt2
        d.svt2 = heads * 64 * d.ldvt2 if svt2 is None else svt2
        d.kv_div2 = kv_div2
    hip.check(hip.lib().mudg_attention(C.byref(d), _stream()), "mudg_attention")
    return out


def quantize_mxfp8(x):
    """Operand rows [rows, cols] (cols % 32 == 0) -> (e4m3 bytes [rows, cols] uint8, E8M0 scales [rows, cols / 32] uint8):
    OCP microscaling, one power-of-two scale per 32 consecutive columns (mudg_quantize_mxfp8)."""
    _rows(x)
    rows, cols = x.shape
    y = torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    sc = torch.empty((rows, cols // 32), dtype=torch.uint8, device=x.device)
    hip.check(hip.lib().mudg_quantize_mxfp8(x.data_ptr(), x.stride(0), rows, cols, y.data_ptr(), y.stride(0), sc.data_ptr(),
                                            sc.stride(0), _stream()), "mudg_quantize_mxfp8")
    return y, sc


def temporal_attention(qkv, out, *, clips, t, hw, heads, scale=0.125):
    hip.check(hip.lib().mudg_temporal_attention(qkv.data_ptr(), out.data_ptr(), clips, t, hw, heads,
                                                qkv.stride(0), out.stride(0), scale, _stream()),
              "mudg_temporal_attention")
    return out


def temporal_self_attention_ok(t, hw, heads, c, ldx=None, ldw=None, ldo=None):
    """Whether mudg_temporal_self_attention runs this problem (a dry query; row strides default to dense rows)."""
    return bool(hip.lib().mudg_temporal_self_attention_ok(t, hw, heads, c, c if ldx is None else ldx, c if ldw is None else ldw,
                                                          c if ldo is None else ldo))


def temporal_self_attention(x, wh, out, *, clips, t, hw, heads, scale=0.125):
    """q | k | v projection of the normalised rows `x` and the attention over T in one launch: `wh` is the head-packed weight
    (packing.qkv_by_head), `out` receives what gemm + temporal_attention would leave in it.  16-bit builds, T = 16, hw % 8 == 0."""
    _rows(x); _rows(wh); _rows(out)
    rows, c = x.shape
    if rows != clips * t * hw or tuple(out.shape) != (rows, c) or tuple(wh.shape) != (3 * c, c):
        raise hip.MudgError(f"temporal_self_attention: x {tuple(x.shape)}, wh {tuple(wh.shape)}, out {tuple(out.shape)} are not "
                            f"[clips * t * hw = {clips * t * hw}][C], [3C][C], [clips * t * hw][C]")
    _drop_stats(out)
    hip.check(hip.lib().mudg_temporal_self_attention(x.data_ptr(), wh.data_ptr(), out.data_ptr(), clips, t, hw, heads, x.shape[1],
                                                     x.stride(0), wh.stride(0), out.stride(0), scale, _stream()),
              "mudg_temporal_self_attention")
    return out


# ------------------------------------------------------------------------------------------------ norms
def _rows_any(t):
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype not in (H16(), torch.float32, torch.float16) or not t.is_cuda:
        raise hip.MudgError(f"expected a cuda operand / fp32 / fp16 rows matrix, got {tuple(t.shape)} {t.dtype} on {t.device}")
    return t


def groupnorm(x, gamma, beta, *, samples, rows, eps, silu, groups=32, x2=None, out=None, fused=True, return_stats=False):
    """GroupNorm(+SiLU).  When every source tensor still carries the partial sums its producing GEMM / conv wrote
    (stats=True there) and a sample is a whole number of 128-row blocks, the statistics pass over x is skipped.
    return_stats: also return the (mean, rstd) per (sample, group) the kernels computed, fp32 [samples * groups][2] (the
    backward pass of the training step needs them)."""
    _rows_any(x)
    if x2 is not None and x2.dtype != x.dtype:
        raise hip.MudgError("groupnorm: both channel sources must share a dtype")
    c = x.shape[1] + (x2.shape[1] if x2 is not None else 0)
    if out is None:
        out = empty_rows(samples * rows, c, H16(), x.device)
    def partials(t):
        ws = getattr(t, GN_ATTR, None)
        tiled = getattr(t, GN_ATTR + "_clips", 0)          # partials per (8 pixels x 16 frames) tile of a clip (tconv3, korder 1)
        if tiled and tiled != samples:
            return None, 128
        ok_ = ws is not None and getattr(t, GN_ATTR + "_version", -1) == _version(t)
        return (ws if ok_ else None), getattr(t, GN_ATTR + "_rows", 128)

    p1, r1 = partials(x) if fused else (None, 128)
    p2, r2 = partials(x2) if (fused and x2 is not None) else (None, r1)
    ok = p1 is not None and rows % r1 == 0 and p1.shape[1] == x.shape[1] and p1.shape[0] * r1 >= samples * rows
    if ok and x2 is not None:
        ok = p2 is not None and rows % r2 == 0 and p2.shape[1] == x2.shape[1] and p2.shape[0] * r2 >= samples * rows
    if ok:
        ws = torch.empty(2 * samples * groups, dtype=torch.float32, device=x.device)
        hip.check(hip.lib().mudg_groupnorm_fused_rows(x.data_ptr(), _ptr(x2), x.shape[1], x.stride(0),
                                                      x2.stride(0) if x2 is not None else 0, kind(x),
                                                      gamma.data_ptr(), beta.data_ptr(),
                                                      out.data_ptr(), out.stride(0), samples, rows, c, groups, eps, int(silu),
                                                      p1.data_ptr(), r1, _ptr(p2), r2, ws.data_ptr(), _stream()), "mudg_groupnorm_fused")
        return (out, ws.reshape(samples * groups, 2)) if return_stats else out
    n = hip.lib().mudg_groupnorm_ws_floats(samples, groups, rows)
    ws = torch.empty(n, dtype=torch.float32, device=x.device)
    hip.check(hip.lib().mudg_groupnorm(x.data_ptr(), _ptr(x2), x.shape[1], x.stride(0),
                                       x2.stride(0) if x2 is not None else 0, kind(x),
                                       gamma.data_ptr(), beta.data_ptr(),
                                       out.data_ptr(), out.stride(0), samples, rows, c, groups, eps, int(silu),
                                       ws.data_ptr(), _stream()), "mudg_groupnorm")
    # the statistics sit at the tail of the scratch (behind the chunk partials): see mudg_groupnorm
    return (out, ws[-2 * samples * groups:].reshape(samples * groups, 2)) if return_stats else out


def layernorm(x, gamma, beta, *, eps=1e-5, out=None):
    _rows_any(x)
    if out is None:
        out = empty_rows(x.shape[0], x.shape[1], H16(), x.device)
    hip.check(hip.lib().mudg_layernorm(x.data_ptr(), x.stride(0), kind(x), gamma.data_ptr(),
                                       beta.data_ptr(), out.data_ptr(),
                                       out.stride(0), x.shape[0], x.shape[1], eps, _stream()), "mudg_layernorm")
    return out


def softmax_rows(s, out=None):
    if out is None:
        out = empty_rows(s.shape[0], s.shape[1], H16(), s.device)
    hip.check(hip.lib().mudg_softmax_rows(s.data_ptr(), s.stride(0), out.data_ptr(), out.stride(0), s.shape[0],
                                          s.shape[1], _stream()), "mudg_softmax_rows")
    return out


# ------------------------------------------------------------------------------------------------ small stuff
_FREQS = {}


def sinusoid_freqs(dim, max_period, device):
    """exp(-ln(max_period) * arange(dim/2) / (dim/2)) in fp32 on the HOST, op for op as utils_diffusion.py:19-22."""
    key = (dim, float(max_period), str(device))
    if key not in _FREQS:
        half = dim // 2
        f = torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
        _FREQS[key] = f.to(device)
    return _FREQS[key]


def timestep_embedding(t, dim, max_period=10000):
    t = t.to(torch.int64).contiguous()
    out = torch.empty((t.shape[0], dim), dtype=torch.float32, device=t.device)
    freqs = sinusoid_freqs(dim, max_period, t.device)
    hip.check(hip.lib().mudg_timestep_embedding(t.data_ptr(), freqs.data_ptr(), out.data_ptr(), t.shape[0], dim,
                                                _stream()), "mudg_timestep_embedding")
    return out


def small_linear(x, w, b=None, *, act_in=False, act_out=False, out=None, accumulate=False):
    """fp32 x [M, K] times w [N, K] (fp32 or bf16) plus bias, optional SiLU before / after."""
    if x.dtype != torch.float32 or not x.is_contiguous() or not w.is_contiguous():
        raise hip.MudgError("small_linear expects contiguous fp32 x and contiguous w")
    m, k = x.shape
    n = w.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().mudg_small_linear(x.data_ptr(), w.data_ptr(), int(w.dtype == H16()), _ptr(b), out.data_ptr(),
                                          m, n, k, int(act_in), int(act_out), int(accumulate), _stream()),
              "mudg_small_linear")
    return out


def ncthw_to_rows(src, dst, coff=0, t0=0, frames=None):
    """(B, C, T, H, W) fp32|bf16 -> dst rows ((b t) h w) channels [coff, coff + C); optional frame window
    [t0, t0 + frames) of the T axis."""
    b, c, t, h, w = src.shape
    src = src.contiguous()
    n = t if frames is None else frames
    hip.check(hip.lib().mudg_ncthw_to_rows(src.data_ptr(), int(src.dtype == torch.float32), dst.data_ptr(), b, c, n,
                                           h * w, dst.stride(0), coff, t, t0, _stream()), "mudg_ncthw_to_rows")
    return dst


def rows_to_ncthw(src, shape, coff=0, dtype=torch.float32, scale=1.0, out=None, t0=0, frames=None):
    """rows ((b t) h w) -> (B, C, T, H, W); with `out` given, writes frames [t0, t0 + frames) of an existing tensor."""
    b, c, t, h, w = shape
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=src.device)
    elif tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise hip.MudgError("rows_to_ncthw: `out` must be a contiguous tensor of the stated shape")
    n = t if frames is None else frames
    hip.check(hip.lib().mudg_rows_to_ncthw(src.data_ptr(), kind(src), src.stride(0), coff,
                                           out.data_ptr(), int(out.dtype == torch.float32), b, c, n, h * w, scale,
                                           t, t0, _stream()),
              "mudg_rows_to_ncthw")
    return out


def zero_channels(dst, c0, c1):
    hip.check(hip.lib().mudg_zero_channels(dst.data_ptr(), dst.shape[0], dst.stride(0), c0, c1, _stream()),
              "mudg_zero_channels")
    return dst


def cast_rows(src, dst):
    """dst[r, c] = src[r, c] between rows matrices of either kind (operand or fp32), any direction (mudg_cast_rows)."""
    if src.dim() != 2 or dst.dim() != 2 or src.shape != dst.shape or src.stride(1) != 1 or dst.stride(1) != 1:
        raise hip.MudgError(f"cast_rows: expected equal-shape rows matrices, got {tuple(src.shape)} -> {tuple(dst.shape)}")
    for t in (src, dst):
        if not t.is_cuda:
            raise hip.MudgError(f"cast_rows: expected cuda tensors, got {t.device}")
    hip.check(hip.lib().mudg_cast_rows(src.data_ptr(), kind(src), src.stride(0), dst.data_ptr(),
                                       kind(dst), dst.stride(0), src.shape[0], src.shape[1], _stream()),
              "mudg_cast_rows")
    return dst


def cast_bf16(src):
    """fp32 / stream rows matrix -> MFMA operand rows of the same shape (an operand matrix is returned as is)."""
    if src.dtype == H16():
        return src
    if src.dtype == torch.float16 and src.dim() == 2 and src.stride(1) == 1:        # fp16 stream -> bf16 operand
        return cast_rows(src, empty_rows(src.shape[0], src.shape[1], H16(), src.device))
    if src.dtype != torch.float32:
        raise hip.MudgError("cast_bf16 expects fp32 (or a 2-D stream matrix)")
    if src.dim() == 2 and src.stride(1) == 1:
        return cast_rows(src, empty_rows(src.shape[0], src.shape[1], H16(), src.device))
    if hip.planes() > 1 or not src.is_contiguous():
        raise hip.MudgError("cast_bf16: only 2-D rows matrices have an operand layout in the split-operand builds")
    out = torch.empty(src.shape, dtype=H16(), device=src.device)         # 16-bit builds: any contiguous shape, flat
    hip.check(hip.lib().mudg_cast_f32_bf16(src.data_ptr(), out.data_ptr(), src.numel(), _stream()), "mudg_cast_f32_bf16")
    return out


def to_f32(src):
    """Operand rows matrix -> fp32 copy of the same shape."""
    if src.dim() != 2:
        raise hip.MudgError("to_f32 expects a 2-D rows matrix")
    return cast_rows(src, torch.empty(src.shape, dtype=torch.float32, device=src.device))


def copy_rows(src, dst):
    """dst[r, :] = src[r, :] for bf16 2-D views with unit inner stride."""
    _rows(src); _rows(dst)
    hip.check(hip.lib().mudg_copy_rows(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), src.shape[0],
                                       src.shape[1], _stream()), "mudg_copy_rows")
    return dst


def add_(y, x, alpha=1.0):
    """y += alpha * x on contiguous fp32 tensors of equal size."""
    if y.dtype != torch.float32 or x.dtype != torch.float32 or not (y.is_contiguous() and x.is_contiguous()):
        raise hip.MudgError("add_ expects contiguous fp32 tensors")
    _drop_stats(y)
    hip.check(hip.lib().mudg_axpy_f32(y.data_ptr(), x.data_ptr(), y.numel(), alpha, _stream()), "mudg_axpy_f32")
    return y


def lincomb(x, y, ca, cb):
    """ca[b] * x[b] + cb[b] * y[b] for fp32 (B, ...) tensors and fp32 [B] device coefficient vectors."""
    for t in (x, y, ca, cb):
        if not t.is_cuda:           # the kernel would dereference host addresses
            raise hip.MudgError(f"lincomb: expected tensors on the GPU, got {t.device}")
    x, y = x.float().contiguous(), y.float().contiguous()
    ca, cb = ca.float().contiguous(), cb.float().contiguous()
    out = torch.empty_like(x)
    b = x.shape[0]
    hip.check(hip.lib().mudg_lincomb(out.data_ptr(), x.data_ptr(), y.data_ptr(), ca.data_ptr(), cb.data_ptr(), b,
                                     x.numel() // b, _stream()), "mudg_lincomb")
    return out


def gaussian_sample(moments, noise=None, scale=1.0):
    """moments (N, 2C, H, W) fp32 -> scale * (mean + std * noise) as (N, C, H, W); noise None = mode."""
    moments = moments.float().contiguous()
    n, c2, h, w = moments.shape
    out = torch.empty((n, c2 // 2, h, w), dtype=torch.float32, device=moments.device)
    if noise is not None:
        noise = noise.to(device=moments.device, dtype=torch.float32).contiguous()
    hip.check(hip.lib().mudg_gaussian_sample(moments.data_ptr(), _ptr(noise), out.data_ptr(), n, c2 // 2, h * w, scale,
                                             _stream()), "mudg_gaussian_sample")
    return out


def _dense_f32(name, t, shape=None):
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise hip.MudgError(f"{name}: expected a contiguous fp32 tensor on the GPU" + (f" of shape {tuple(shape)}" if shape else "")
                            + f", got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def posterior_assemble(mom_x, mom_sparse, mom_depth, noise, b, t, scale=1.0):
    """The three posterior samples of get_batch_input in one launch, in the UNet's layout: moments (b t, 2C, h, w) fp32 of the
    dense / sparse colour / sparse depth frames, `noise` (3, b t, C, h, w) on the device (stream order dense, sparse, depth) or
    None (posterior mode) -> z (b, C, t, h, w), c_concat (b, 2C, t, h, w) = [sparse | depth] along the channels.  The value
    arithmetic is gaussian_sample's."""
    n, c2, h, w = mom_x.shape
    c = c2 // 2
    if n != b * t:
        raise hip.MudgError(f"posterior_assemble: {n} frames are not {b} clips of {t}")
    for m in (mom_x, mom_sparse, mom_depth):
        _dense_f32("posterior_assemble: moments", m, (n, c2, h, w))
    if noise is not None:
        _dense_f32("posterior_assemble: noise", noise, (3, n, c, h, w))
    z = torch.empty((b, c, t, h, w), dtype=torch.float32, device=mom_x.device)
    cc = torch.empty((b, 2 * c, t, h, w), dtype=torch.float32, device=mom_x.device)
    nz = [None] * 3 if noise is None else [noise[i].data_ptr() for i in range(3)]
    hip.check(hip.lib().mudg_posterior_assemble(mom_x.data_ptr(), mom_sparse.data_ptr(), mom_depth.data_ptr(), *nz, z.data_ptr(),
                                                cc.data_ptr(), b, t, c, h * w, float(scale), _stream()), "mudg_posterior_assemble")
    return z, cc


def cond_dropout(r, p, cond_emb, null_prompt, clip, frame=0):
    """Conditioning dropout of get_batch_input from the device vector r (b,): prompt rows (b, L, D) <- null_prompt (1, L, D)
    where r < 2p; image (b, C, H, W) = (1 - (r >= p)(r < 3p)) * clip[:, :, frame], read in place from the (b, C, T, H, W) clip
    (which is not modified).  One launch; r never leaves the device."""
    b, ch, t, h, w = clip.shape
    _dense_f32("cond_dropout: clip", clip)
    _dense_f32("cond_dropout: r", r, (b,))
    cond_emb = _dense_f32("cond_dropout: prompt embedding", cond_emb.float().contiguous())
    null_prompt = _dense_f32("cond_dropout: null prompt", null_prompt.float().contiguous(), (1,) + tuple(cond_emb.shape[1:]))
    if cond_emb.shape[0] != b or not 0 <= frame < t:
        raise hip.MudgError(f"cond_dropout: {cond_emb.shape[0]} prompts / frame {frame} for a clip batch {tuple(clip.shape)}")
    prompt = torch.empty_like(cond_emb)
    img = torch.empty((b, ch, h, w), dtype=torch.float32, device=clip.device)
    p = float(p)
    hip.check(hip.lib().mudg_cond_dropout(r.data_ptr(), p, 2 * p, 3 * p, cond_emb.data_ptr(), null_prompt.data_ptr(), prompt.data_ptr(),
                                          b, cond_emb[0].numel(), clip.data_ptr() + 4 * frame * h * w, clip.stride(0), clip.stride(1),
                                          img.data_ptr(), ch, h * w, _stream()), "mudg_cond_dropout")
    return prompt, img


def ddim_step(x, e_c, e_u, noise, coef, e_m=None):
    """Fused DDIM update on fp32 latents (B, ...). coef = 8 to 10 host floats, see mudg_ddim_step; e_m = the
    image-only-conditioned pass of the three-way guidance (coef[8] = cfg_img); coef[9] = 1 for eps-predicting models."""
    def dense(t):      # raw pointers are handed to the kernel: insist on dense fp32 (permuted views are copied)
        return None if t is None else t.to(torch.float32).contiguous()

    x, e_c, e_u, noise, e_m = dense(x), dense(e_c), dense(e_u), dense(noise), dense(e_m)
    coef = list(coef) + [0.0] * (10 - len(coef))
    b = x.shape[0]
    n = x.numel() // b
    x_prev, pred_x0 = torch.empty_like(x), torch.empty_like(x)
    ws = torch.empty(hip.lib().mudg_ddim_ws_doubles(b), dtype=torch.float64, device=x.device)
    arr = (C.c_float * 10)(*[float(v) for v in coef])
    hip.check(hip.lib().mudg_ddim_step(x.data_ptr(), e_c.data_ptr(), _ptr(e_u), _ptr(e_m), _ptr(noise), x_prev.data_ptr(),
                                       pred_x0.data_ptr(), b, n, arr, ws.data_ptr(), _stream()), "mudg_ddim_step")
    return x_prev, pred_x0


# ------------------------------------------------------------------------------------------------ post-processing
def frames_to_uint8(video):
    """(b, c, t, h, w) float -> (b, t, h, w, c) uint8: clamp to [-1, 1], (x + 1) / 2 * 255, truncate (eval_tools.py:22-27)."""
    if video.dim() != 5 or not video.is_cuda:
        raise hip.MudgError(f"frames_to_uint8: expected a cuda (b, c, t, h, w) tensor, got {tuple(video.shape)} on {video.device}")
    v = video.to(torch.float32).contiguous()
    b, c, t, h, w = v.shape
    out = torch.empty((b, t, h, w, c), dtype=torch.uint8, device=v.device)
    hip.check(hip.lib().mudg_frames_to_u8(v.data_ptr(), out.data_ptr(), b, c, t, h * w, _stream()), "mudg_frames_to_u8")
    return out


def log_sheet(value, clamp=True, rescale=True):
    """The uint8 frame sheet of a logged entry (utils/save_video.py:62-136): a video (n, c, t, h, w) -> (t, n*h, w, 3), an image
    batch (n, c, h, w) -> (n*h, w, 3); c = 1 or 3, the samples stacked along the height, one channel repeated to three.  clamp: to
    [-1, 1] first (prepare_to_log); rescale: (x + 1) / 2; then * 255 and truncation — byte-equal to the reference's expressions."""
    if value.dim() not in (4, 5) or not value.is_cuda:
        raise hip.MudgError(f"log_sheet: expected a cuda (n, c, t, h, w) or (n, c, h, w) tensor, got {tuple(value.shape)} on {value.device}")
    v = value.detach().to(torch.float32).contiguous()
    n, c = v.shape[:2]
    t = v.shape[2] if v.dim() == 5 else 1
    h, w = v.shape[-2:]
    if c not in (1, 3):
        raise hip.MudgError(f"log_sheet: {c} channels (grayscale or rgb entries only)")
    out = torch.empty((t, n * h, w, 3), dtype=torch.uint8, device=v.device)
    hip.check(hip.lib().mudg_log_sheet(v.data_ptr(), out.data_ptr(), n, c, t, h, w, int(bool(clamp)), int(bool(rescale)), _stream()),
              "mudg_log_sheet")
    return out if v.dim() == 5 else out[0]


def depth_from_uint8(frames):
    """(..., h, w, 3) uint8 -> (..., 1, h, w) float32 in [0, 1]: channel mean / 255 (eval_tools.py:71)."""
    if frames.dtype != torch.uint8 or frames.shape[-1] != 3 or not frames.is_cuda:
        raise hip.MudgError("depth_from_uint8: expected a cuda (..., h, w, 3) uint8 tensor")
    f = frames.contiguous()
    out = torch.empty(f.shape[:-3] + (1,) + f.shape[-3:-1], dtype=torch.float32, device=f.device)
    hip.check(hip.lib().mudg_depth_from_u8(f.data_ptr(), out.data_ptr(), f.numel() // 3, _stream()), "mudg_depth_from_u8")
    return out


def semantic_nearest(img):
    """(3, h, w) uint8 -> ((3, h, w) uint8 recoloured, (h, w) int64 labels): nearest of 19 palette colours
    (eval_tools.py:309-347)."""
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[0] != 3 or not img.is_cuda:
        raise hip.MudgError("semantic_nearest: expected a cuda (3, h, w) uint8 tensor")
    x = img.contiguous()
    vis = torch.empty_like(x)
    lab = torch.empty(x.shape[1:], dtype=torch.int64, device=x.device)
    hip.check(hip.lib().mudg_semantic_nearest(x.data_ptr(), vis.data_ptr(), lab.data_ptr(), x.shape[1] * x.shape[2], _stream()),
              "mudg_semantic_nearest")
    return vis, lab


# ------------------------------------------------------------------------------------------------ sparse conditions (point splat)
def _splat_tensor(name, t, dtype, shape=None):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise hip.MudgError(f"{name}: expected a contiguous {dtype} tensor on the GPU" + (f" of shape {tuple(shape)}" if shape else "") + f", got {got}")
    return t


def splat_keys(poses, h, w, device):
    """An empty key image (poses, h, w): all ones, which is how splat_resolve leaves it."""
    return torch.full((poses, h, w), -1, dtype=torch.int64, device=device)


def splat_points(points, mats, keys, intr, point_size, *, ids=None, znear=1e-4, zfar=200.0, early_reject=True, stats=None):
    """Draw a packed cloud (n, 4) int32 — x, y, z fp32 bits and r | g << 8 | b << 16 — into keys (poses, h, w) int64 with the
    matrices mats (poses, nmat, 12) fp32 (ids (n,) int32 choose among nmat > 1) and intr = (fx, fy, cx, cy): per covered pixel the
    unsigned minimum of (bits(zc) << 32 | index).  DESIGN.md §12 states the rule.  stats: a (2,) int64 counter pair (tools)."""
    _splat_tensor("splat_points: points", points, torch.int32)
    if points.dim() != 2 or points.shape[1] != 4 or points.shape[0] == 0:
        raise hip.MudgError(f"splat_points: expected packed points (n > 0, 4), got {tuple(points.shape)}")
    _splat_tensor("splat_points: mats", mats, torch.float32)
    _splat_tensor("splat_points: keys", keys, torch.int64)
    if mats.dim() != 3 or mats.shape[2] != 12 or keys.dim() != 3 or keys.shape[0] != mats.shape[0]:
        raise hip.MudgError(f"splat_points: matrices {tuple(mats.shape)} do not go with a key image {tuple(keys.shape)}")
    n, (poses, nmat) = points.shape[0], mats.shape[:2]
    if ids is not None:
        _splat_tensor("splat_points: ids", ids, torch.int32, (n,))
    if stats is not None:
        _splat_tensor("splat_points: stats", stats, torch.int64, (2,))
    fx, fy, cx, cy = (float(v) for v in intr)
    hip.check(hip.lib().mudg_splat_points(points.data_ptr(), _ptr(ids), n, mats.data_ptr(), poses, nmat, keys.data_ptr(), keys.shape[1], keys.shape[2],
                                          fx, fy, cx, cy, float(znear), float(zfar), float(point_size), 0 if early_reject else 1,
                                          _ptr(stats), _stream()), "mudg_splat_points")
    return keys


def splat_resolve(keys, points):
    """keys (poses, h, w) -> (depth fp32, colour int32 = r | g << 8 | b << 16) of the winners, zero where nothing landed; the key image
    is empty again afterwards."""
    _splat_tensor("splat_resolve: keys", keys, torch.int64)
    _splat_tensor("splat_resolve: points", points, torch.int32)
    depth = torch.empty(keys.shape, dtype=torch.float32, device=keys.device)
    colour = torch.empty(keys.shape, dtype=torch.int32, device=keys.device)
    hip.check(hip.lib().mudg_splat_resolve(keys.data_ptr(), points.data_ptr(), points.shape[0], depth.data_ptr(), colour.data_ptr(), keys.numel(),
                                           _stream()), "mudg_splat_resolve")
    return depth, colour


def splat_compose(bg, obj, sparse_frames, sparse_depth, t, *, images=False):
    """bg / obj = (depth, colour) pairs of splat_resolve (obj None: no object layer); writes frame t of sparse_frames and sparse_depth
    (poses, 3, T, h, w) fp32.  images: also returns (rgb (poses, h, w, 3) uint8, depth (poses, h, w) fp32, mask (poses, h, w) uint8)."""
    bg_d, bg_c = bg
    poses, h, w = bg_d.shape
    _splat_tensor("splat_compose: background depth", bg_d, torch.float32)
    _splat_tensor("splat_compose: background colour", bg_c, torch.int32, (poses, h, w))
    ob_d = ob_c = None
    if obj is not None:
        ob_d = _splat_tensor("splat_compose: object depth", obj[0], torch.float32, (poses, h, w))
        ob_c = _splat_tensor("splat_compose: object colour", obj[1], torch.int32, (poses, h, w))
    _splat_tensor("splat_compose: sparse_frames", sparse_frames, torch.float32)
    _splat_tensor("splat_compose: sparse_depth", sparse_depth, torch.float32, sparse_frames.shape)
    if sparse_frames.dim() != 5 or sparse_frames.shape[0] != poses or sparse_frames.shape[1] != 3 or tuple(sparse_frames.shape[3:]) != (h, w):
        raise hip.MudgError(f"splat_compose: conditions {tuple(sparse_frames.shape)} for {poses} poses of {h} x {w}")
    T = sparse_frames.shape[2]
    rgb = depth = mask = None
    if images:
        rgb = torch.empty((poses, h, w, 3), dtype=torch.uint8, device=bg_d.device)
        depth = torch.empty((poses, h, w), dtype=torch.float32, device=bg_d.device)
        mask = torch.empty((poses, h, w), dtype=torch.uint8, device=bg_d.device)
    hip.check(hip.lib().mudg_splat_compose(bg_c.data_ptr(), bg_d.data_ptr(), _ptr(ob_c), _ptr(ob_d), sparse_frames.data_ptr(), sparse_depth.data_ptr(),
                                           3 * T * h * w, poses, T, int(t), h, w, _ptr(rgb), _ptr(depth), _ptr(mask), _stream()),
              "mudg_splat_compose")
    return (rgb, depth, mask) if images else None


# ------------------------------------------------------------------------------------------------ scene clouds from LiDAR sweeps
def cloud_sweep(rays_o, rays_d, ranges, offsets, max_rays, l2w, cams, objs, images):
    """One launch for a batch of frames: rays_o / rays_d (n, 3) and ranges (n,) fp32, concatenated over the frames;
    offsets (frames + 1,) int64 on the GPU, max_rays the longest frame; l2w (frames, 12) float64; cams (frames, ncam, 24) float64
    (w2c, K, then h, w and the image's byte offset as int64 bit patterns) or None; objs (frames, nobj, 16) float64 or None; images a
    flat uint8 buffer.  Returns packed points (n, 4) int32 and labels (n,) int32."""
    _splat_tensor("cloud_sweep: rays_o", rays_o, torch.float32)
    n = rays_o.shape[0]
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or n == 0:
        raise hip.MudgError(f"cloud_sweep: expected rays (n > 0, 3), got {tuple(rays_o.shape)}")
    _splat_tensor("cloud_sweep: rays_d", rays_d, torch.float32, (n, 3))
    _splat_tensor("cloud_sweep: ranges", ranges, torch.float32, (n,))
    _splat_tensor("cloud_sweep: offsets", offsets, torch.int64)
    frames = offsets.numel() - 1
    _splat_tensor("cloud_sweep: l2w", l2w, torch.float64, (frames, 12))
    ncam = nobj = 0
    if cams is not None:
        _splat_tensor("cloud_sweep: cams", cams, torch.float64)
        _splat_tensor("cloud_sweep: images", images, torch.uint8)
        if cams.dim() != 3 or cams.shape[0] != frames or cams.shape[2] != 24 or images.dim() != 1:
            raise hip.MudgError(f"cloud_sweep: camera table {tuple(cams.shape)} for {frames} frames, images {tuple(images.shape)}")
        ncam = cams.shape[1]
    if objs is not None:
        _splat_tensor("cloud_sweep: objs", objs, torch.float64)
        if objs.dim() != 3 or objs.shape[0] != frames or objs.shape[2] != 16:
            raise hip.MudgError(f"cloud_sweep: object table {tuple(objs.shape)} for {frames} frames")
        nobj = objs.shape[1]
    points = torch.empty((n, 4), dtype=torch.int32, device=rays_o.device)
    labels = torch.empty((n,), dtype=torch.int32, device=rays_o.device)
    hip.check(hip.lib().mudg_cloud_sweep(rays_o.data_ptr(), rays_d.data_ptr(), ranges.data_ptr(), offsets.data_ptr(), frames, int(max_rays), n,
                                         l2w.data_ptr(), _ptr(cams) if ncam else None, ncam, _ptr(objs) if nobj else None, nobj,
                                         _ptr(images) if ncam else None, images.numel() if ncam else 0, points.data_ptr(), labels.data_ptr(),
                                         _stream()), "mudg_cloud_sweep")
    return points, labels


def cloud_voxel_keys(points, voxel):
    """Packed points (n, 4) int32 -> (n,) int64 voxel keys on the absolute grid of size `voxel` (the caller has checked the range)."""
    _splat_tensor("cloud_voxel_keys: points", points, torch.int32)
    keys = torch.empty((points.shape[0],), dtype=torch.int64, device=points.device)
    hip.check(hip.lib().mudg_cloud_voxel_keys(points.data_ptr(), points.shape[0], float(voxel), keys.data_ptr(), _stream()), "mudg_cloud_voxel_keys")
    return keys


def cloud_voxel_reduce(points, order, segments, voxel, voxels):
    """Integer sums per voxel, (voxels, 8) int64: count, r, g, b, three fixed-point offsets, the key.  order / segments: (n,) int64."""
    n = points.shape[0]
    _splat_tensor("cloud_voxel_reduce: points", points, torch.int32, (n, 4))
    _splat_tensor("cloud_voxel_reduce: order", order, torch.int64, (n,))
    _splat_tensor("cloud_voxel_reduce: segments", segments, torch.int64, (n,))
    sums = torch.zeros((int(voxels), 8), dtype=torch.int64, device=points.device)
    hip.check(hip.lib().mudg_cloud_voxel_reduce(points.data_ptr(), order.data_ptr(), segments.data_ptr(), n, float(voxel), sums.data_ptr(), int(voxels),
                                                _stream()), "mudg_cloud_voxel_reduce")
    return sums


def cloud_voxel_finish(sums, voxel):
    """(voxels, 8) sums -> packed points (voxels, 4) int32: the mean position and the round-half-up mean colour of every voxel."""
    _splat_tensor("cloud_voxel_finish: sums", sums, torch.int64)
    out = torch.empty((sums.shape[0], 4), dtype=torch.int32, device=sums.device)
    hip.check(hip.lib().mudg_cloud_voxel_finish(sums.data_ptr(), sums.shape[0], float(voxel), out.data_ptr(), _stream()), "mudg_cloud_voxel_finish")
    return out


# ------------------------------------------------------------------------------------------------ neighbour search between clouds
NEIGHBOUR_MAX_RADIUS = 64.0
NEIGHBOUR_MARGIN = 1.0 + 2.0 ** -10        # cell edge / radius
CLOUD_MAX_THRESHOLDS = 8


def _neighbour_args(name, ref_sorted, keys, order, queries, visit):
    _splat_tensor(f"{name}: the sorted reference", ref_sorted, torch.int32)
    n = ref_sorted.shape[0]
    if ref_sorted.dim() != 2 or ref_sorted.shape[1] != 4 or n == 0:
        raise hip.MudgError(f"{name}: expected packed reference points (n > 0, 4), got {tuple(ref_sorted.shape)}")
    _splat_tensor(f"{name}: keys", keys, torch.int64, (n,))
    _splat_tensor(f"{name}: order", order, torch.int64, (n,))
    _splat_tensor(f"{name}: queries", queries, torch.int32)
    nq = queries.shape[0]
    if queries.dim() != 2 or queries.shape[1] != 4 or nq == 0:
        raise hip.MudgError(f"{name}: expected packed queries (nq > 0, 4), got {tuple(queries.shape)}")
    if visit is not None:
        _splat_tensor(f"{name}: visit", visit, torch.int64, (nq,))
    return n, nq


def cloud_nearest(ref_sorted, keys, order, queries, cell, r2, *, visit=None):
    """The nearest reference point within reach of every query.  ref_sorted (n, 4) int32 packed points in ascending key
    order, keys and order (n,) int64 (cloud.NeighbourGrid holds all three), queries (nq, 4) int32, visit (nq,) int64 or None: the order
    in which the lanes take the queries.  Returns (d2 (nq,) float64, +inf where nothing is within reach; index (nq,) int64, -1 there)."""
    n, nq = _neighbour_args("cloud_nearest", ref_sorted, keys, order, queries, visit)
    d2 = torch.empty((nq,), dtype=torch.float64, device=queries.device)
    index = torch.empty((nq,), dtype=torch.int64, device=queries.device)
    hip.check(hip.lib().mudg_cloud_nearest(ref_sorted.data_ptr(), keys.data_ptr(), order.data_ptr(), n, queries.data_ptr(), _ptr(visit), nq,
                                           float(cell), float(r2), d2.data_ptr(), index.data_ptr(), _stream()), "mudg_cloud_nearest")
    return d2, index


def cloud_count(ref_sorted, keys, order, queries, cell, r2, cap, *, visit=None):
    """min(reference points within reach, cap) of every query, (nq,) int32; the arguments of cloud_nearest and cap >= 1."""
    n, nq = _neighbour_args("cloud_count", ref_sorted, keys, order, queries, visit)
    counts = torch.empty((nq,), dtype=torch.int32, device=queries.device)
    hip.check(hip.lib().mudg_cloud_count(ref_sorted.data_ptr(), keys.data_ptr(), order.data_ptr(), n, queries.data_ptr(), _ptr(visit), nq,
                                         float(cell), float(r2), int(cap), counts.data_ptr(), _stream()), "mudg_cloud_count")
    return counts


def metric_cloud(d2, t2, r2):
    """d2 (n,) float64, cloud_nearest's; t2: up to eight squared thresholds (host floats, 0 < t2 <= r2) -> (2 + K,) int64: the number of
    finite values, the sum over them of floor(sqrt(d2) 2^20), the counts of d2 <= t2[k]."""
    _splat_tensor("metric_cloud: d2", d2, torch.float64)
    if d2.dim() != 1 or d2.numel() == 0:
        raise hip.MudgError(f"metric_cloud: expected (n > 0,) squared distances, got {tuple(d2.shape)}")
    t2 = [float(t) for t in t2]
    if len(t2) > CLOUD_MAX_THRESHOLDS:
        raise hip.MudgError(f"metric_cloud: {len(t2)} thresholds (at most {CLOUD_MAX_THRESHOLDS})")
    sums = torch.zeros((2 + len(t2),), dtype=torch.int64, device=d2.device)
    table = (hip.C.c_double * max(len(t2), 1))(*t2)                         # read by the call itself, before it returns
    hip.check(hip.lib().mudg_metric_cloud(d2.data_ptr(), d2.numel(), table, len(t2), float(r2), sums.data_ptr(), _stream()), "mudg_metric_cloud")
    return sums


# ------------------------------------------------------------------------------------------------ clouds as 3D Gaussians
GAUSS_TILE = 16
GAUSS_SUMS = 10                  # a partial: dcolour0..2, dzc, dopacity, dA, dB, dC, du, dv


def gauss_tiles(h, w):
    """(TX, TY) of an h x w image."""
    return (int(w) + GAUSS_TILE - 1) // GAUSS_TILE, (int(h) + GAUSS_TILE - 1) // GAUSS_TILE


def _gauss_cloud(name, points, cov, mats, ids):
    """The operands gauss_project and its backward share -> (n, V, nmat)."""
    _splat_tensor(f"{name}: points", points, torch.int32)
    if points.dim() != 2 or points.shape[1] != 4 or points.shape[0] == 0:
        raise hip.MudgError(f"{name}: expected packed points (n > 0, 4), got {tuple(points.shape)}")
    n = points.shape[0]
    _splat_tensor(f"{name}: cov", cov, torch.float32, (n, 6))
    _splat_tensor(f"{name}: mats", mats, torch.float32)
    if mats.dim() != 3 or mats.shape[2] != 12 or mats.shape[0] == 0 or mats.shape[1] == 0:
        raise hip.MudgError(f"{name}: expected matrices (V, nmat, 12), got {tuple(mats.shape)}")
    if ids is not None:
        _splat_tensor(f"{name}: ids", ids, torch.int32, (n,))
    return (n, *mats.shape[:2])


# a blend's first operand: its name, its name in the shape error, its dtype, its row width
_GAUSS_POINTS = ("points", "packed points", torch.int32, 4)
_GAUSS_COLOURS = ("colour", "colours", torch.float32, 3)


def _gauss_entries(name, first, kind, uv, conic, depth, values_sorted, ranges, hw):
    """The operands the three blends share, `first` checked as `kind` (_GAUSS_POINTS or _GAUSS_COLOURS) -> (V, n, h, w, V NT)."""
    label, plural, dtype, width = kind
    _splat_tensor(f"{name}: {label}", first, dtype)
    _splat_tensor(f"{name}: depth", depth, torch.float32)
    if first.dim() != 2 or first.shape[1] != width or depth.dim() != 2 or depth.shape[1] != first.shape[0]:
        raise hip.MudgError(f"{name}: {plural} {tuple(first.shape)} with depths {tuple(depth.shape)}")
    v, n = depth.shape
    h, w = (int(s) for s in hw)
    tx, ty = gauss_tiles(h, w)
    _splat_tensor(f"{name}: uv", uv, torch.float32, (v, n, 2))
    _splat_tensor(f"{name}: conic", conic, torch.float32, (v, n, 4))
    _splat_tensor(f"{name}: values", values_sorted, torch.int32)
    _splat_tensor(f"{name}: ranges", ranges, torch.int32, (v * tx * ty, 2))
    if values_sorted.dim() != 1 or values_sorted.numel() == 0:
        raise hip.MudgError(f"{name}: expected (E > 0,) sorted values, got {tuple(values_sorted.shape)}")
    return v, n, h, w, v * tx * ty


def _gauss_images(v, h, w, device):
    """rgb (V, 3, H, W), depth (V, H, W) and alpha (V, H, W) for a blend to fill."""
    return (torch.empty((v, 3, h, w), dtype=torch.float32, device=device), torch.empty((v, h, w), dtype=torch.float32, device=device),
            torch.empty((v, h, w), dtype=torch.float32, device=device))


def _gauss_partial(name, partial):
    _splat_tensor(f"{name}: partial", partial, torch.float32)
    if partial.dim() != 2 or partial.shape[1] != GAUSS_SUMS or partial.shape[0] == 0:
        raise hip.MudgError(f"{name}: expected partials (E > 0, {GAUSS_SUMS}), got {tuple(partial.shape)}")


def gauss_project(points, cov, opacity, mats, intr, hw, *, ids=None, znear=0.2, zfar=200.0):
    """Project packed points (n, 4) int32 with covariances (n, 6) and opacities (n,) fp32 through mats (V, nmat, 12) fp32 and intr =
    (fx, fy, cx, cy) into V views of hw.  Returns uv (V, n, 2), conic (V, n, 4) = (A, B, C, opacity), depth (V, n) fp32,
    rect (V, n, 4) = (x0, x1, y0, y1) and count (V, n) int32, all zero where a Gaussian is dropped."""
    n, v, nmat = _gauss_cloud("gauss_project", points, cov, mats, ids)
    _splat_tensor("gauss_project: opacity", opacity, torch.float32, (n,))
    h, w = (int(s) for s in hw)
    fx, fy, cx, cy = (float(s) for s in intr)
    dev = points.device
    uv = torch.empty((v, n, 2), dtype=torch.float32, device=dev)
    conic = torch.empty((v, n, 4), dtype=torch.float32, device=dev)
    depth = torch.empty((v, n), dtype=torch.float32, device=dev)
    rect = torch.empty((v, n, 4), dtype=torch.int32, device=dev)
    count = torch.empty((v, n), dtype=torch.int32, device=dev)
    hip.check(hip.lib().mudg_gauss_project(points.data_ptr(), cov.data_ptr(), opacity.data_ptr(), _ptr(ids), n, mats.data_ptr(), v, nmat, h, w,
                                           fx, fy, cx, cy, float(znear), float(zfar), uv.data_ptr(), conic.data_ptr(), depth.data_ptr(),
                                           rect.data_ptr(), count.data_ptr(), _stream()), "mudg_gauss_project")
    return uv, conic, depth, rect, count


def gauss_keys(depth, rect, count, offsets, entries, hw):
    """One (key, value) entry per tile of every rectangle: keys (E,) int64 = (view NT + tile) << 32 | bits(zc), values (E,) int32 = the
    Gaussian's index.  offsets (V, n) int64: the exclusive sum of count; entries: its total E."""
    _splat_tensor("gauss_keys: depth", depth, torch.float32)
    if depth.dim() != 2:
        raise hip.MudgError(f"gauss_keys: expected depths (V, n), got {tuple(depth.shape)}")
    v, n = depth.shape
    _splat_tensor("gauss_keys: rect", rect, torch.int32, (v, n, 4))
    _splat_tensor("gauss_keys: count", count, torch.int32, (v, n))
    _splat_tensor("gauss_keys: offsets", offsets, torch.int64, (v, n))
    e = int(entries)
    if e <= 0:
        raise hip.MudgError(f"gauss_keys: {e} entries")
    keys = torch.empty((e,), dtype=torch.int64, device=depth.device)
    values = torch.empty((e,), dtype=torch.int32, device=depth.device)
    hip.check(hip.lib().mudg_gauss_keys(depth.data_ptr(), rect.data_ptr(), count.data_ptr(), offsets.data_ptr(), n, v, int(hw[0]), int(hw[1]), e,
                                        keys.data_ptr(), values.data_ptr(), _stream()), "mudg_gauss_keys")
    return keys, values


def gauss_ranges(keys_sorted, tiles):
    """Sorted keys (E,) int64 -> (tiles, 2) int32: the [start, end) of every tile's entries, [0, 0) for an empty tile."""
    _splat_tensor("gauss_ranges: keys", keys_sorted, torch.int64)
    if keys_sorted.dim() != 1 or keys_sorted.numel() == 0:
        raise hip.MudgError(f"gauss_ranges: expected (E > 0,) keys, got {tuple(keys_sorted.shape)}")
    ranges = torch.empty((int(tiles), 2), dtype=torch.int32, device=keys_sorted.device)
    hip.check(hip.lib().mudg_gauss_ranges(keys_sorted.data_ptr(), keys_sorted.numel(), int(tiles), ranges.data_ptr(), _stream()), "mudg_gauss_ranges")
    return ranges


def gauss_blend(points, uv, conic, depth, values_sorted, ranges, hw, *, walked=None):
    """Front-to-back alpha blending of every tile's entries: rgb (V, 3, H, W) in [0, 1] on black, depth (V, H, W) alpha-weighted and
    alpha (V, H, W), fp32.  walked: a (V NT,) int32 tensor that receives the entries each workgroup staged (tools)."""
    v, n, h, w, tiles = _gauss_entries("gauss_blend", points, _GAUSS_POINTS, uv, conic, depth, values_sorted, ranges, hw)
    if walked is not None:
        _splat_tensor("gauss_blend: walked", walked, torch.int32, (tiles,))
    rgb, out_depth, alpha = _gauss_images(v, h, w, points.device)
    hip.check(hip.lib().mudg_gauss_blend(points.data_ptr(), uv.data_ptr(), conic.data_ptr(), depth.data_ptr(), values_sorted.data_ptr(),
                                         ranges.data_ptr(), n, values_sorted.numel(), v, h, w, rgb.data_ptr(), out_depth.data_ptr(),
                                         alpha.data_ptr(), _ptr(walked), _stream()), "mudg_gauss_blend")
    return rgb, out_depth, alpha


def gauss_blend_train(colour, uv, conic, depth, values_sorted, ranges, hw):
    """gauss_blend with the colour an fp32 (n, 3) tensor in byte units.  Returns rgb, depth, alpha as gauss_blend does and
    state (V, 5, H, W) fp32 = the accumulators (C0, C1, C2, D, T) of every pixel, which the backward needs unrounded."""
    v, n, h, w, _ = _gauss_entries("gauss_blend_train", colour, _GAUSS_COLOURS, uv, conic, depth, values_sorted, ranges, hw)
    rgb, out_depth, alpha = _gauss_images(v, h, w, colour.device)
    state = torch.empty((v, 5, h, w), dtype=torch.float32, device=colour.device)
    hip.check(hip.lib().mudg_gauss_blend_train(colour.data_ptr(), uv.data_ptr(), conic.data_ptr(), depth.data_ptr(), values_sorted.data_ptr(),
                                               ranges.data_ptr(), n, values_sorted.numel(), v, h, w, rgb.data_ptr(), out_depth.data_ptr(),
                                               alpha.data_ptr(), state.data_ptr(), _stream()), "mudg_gauss_blend_train")
    return rgb, out_depth, alpha, state


def gauss_blend_bwd(colour, uv, conic, depth, values_sorted, order, ranges, hw, state, d_rgb, d_depth, d_alpha):
    """The blend's backward: partial (E, 10) fp32, one row per entry at its unsorted position order[e], the sums over the tile's pixels of
    (dcolour0..2, dzc, dopacity, dA, dB, dC, du, dv) in one fixed order; zero for entries no workgroup reached."""
    v, n, h, w, _ = _gauss_entries("gauss_blend_bwd", colour, _GAUSS_COLOURS, uv, conic, depth, values_sorted, ranges, hw)
    e = values_sorted.numel()
    _splat_tensor("gauss_blend_bwd: order", order, torch.int64, (e,))
    _splat_tensor("gauss_blend_bwd: state", state, torch.float32, (v, 5, h, w))
    _splat_tensor("gauss_blend_bwd: d_rgb", d_rgb, torch.float32, (v, 3, h, w))
    _splat_tensor("gauss_blend_bwd: d_depth", d_depth, torch.float32, (v, h, w))
    _splat_tensor("gauss_blend_bwd: d_alpha", d_alpha, torch.float32, (v, h, w))
    partial = torch.empty((e, GAUSS_SUMS), dtype=torch.float32, device=colour.device)
    hip.check(hip.lib().mudg_gauss_blend_bwd(colour.data_ptr(), uv.data_ptr(), conic.data_ptr(), depth.data_ptr(), values_sorted.data_ptr(),
                                             order.data_ptr(), ranges.data_ptr(), n, e, v, h, w, state.data_ptr(), d_rgb.data_ptr(),
                                             d_depth.data_ptr(), d_alpha.data_ptr(), partial.data_ptr(), _stream()), "mudg_gauss_blend_bwd")
    return partial


def gauss_project_bwd(points, cov, mats, intr, hw, count, offsets, partial, *, ids=None, znear=0.2, zfar=200.0):
    """The projection's backward: every Gaussian's partials gathered per view in ascending order and taken through the chain rule of
    gauss_project, the views added in order.  Returns d_xyz (n, 3), d_cov (n, 6) (off-diagonal entries: both symmetric halves),
    d_opacity (n,) and d_colour (n, 3), fp32."""
    n, v, nmat = _gauss_cloud("gauss_project_bwd", points, cov, mats, ids)
    _splat_tensor("gauss_project_bwd: count", count, torch.int32, (v, n))
    _splat_tensor("gauss_project_bwd: offsets", offsets, torch.int64, (v, n))
    _gauss_partial("gauss_project_bwd", partial)
    h, w = (int(s) for s in hw)
    fx, fy, cx, cy = (float(s) for s in intr)
    dev = points.device
    d_xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    d_cov = torch.empty((n, 6), dtype=torch.float32, device=dev)
    d_opacity = torch.empty((n,), dtype=torch.float32, device=dev)
    d_colour = torch.empty((n, 3), dtype=torch.float32, device=dev)
    hip.check(hip.lib().mudg_gauss_project_bwd(points.data_ptr(), cov.data_ptr(), _ptr(ids), n, mats.data_ptr(), v, nmat, h, w, fx, fy, cx, cy,
                                               float(znear), float(zfar), count.data_ptr(), offsets.data_ptr(), partial.data_ptr(),
                                               partial.shape[0], d_xyz.data_ptr(), d_cov.data_ptr(), d_opacity.data_ptr(), d_colour.data_ptr(),
                                               _stream()), "mudg_gauss_project_bwd")
    return d_xyz, d_cov, d_opacity, d_colour


GAUSS_SH_MAX_DEGREE = 3


def gauss_sh_rows(degree):
    """K - 1 = (L + 1)^2 - 1: the coefficient rows of a Gaussian that carries harmonics of degrees 1 .. L."""
    return (int(degree) + 1) ** 2 - 1


def _gauss_sh(name, points, mats, ids, count, colour, sh, active):
    """The operands gauss_sh_colour and its backward share -> (n, V, nmat, L, active)."""
    _splat_tensor(f"{name}: points", points, torch.int32)
    if points.dim() != 2 or points.shape[1] != 4 or points.shape[0] == 0:
        raise hip.MudgError(f"{name}: expected packed points (n > 0, 4), got {tuple(points.shape)}")
    n = points.shape[0]
    _splat_tensor(f"{name}: mats", mats, torch.float32)
    if mats.dim() != 3 or mats.shape[2] != 12 or mats.shape[0] == 0 or mats.shape[1] == 0:
        raise hip.MudgError(f"{name}: expected matrices (V, nmat, 12), got {tuple(mats.shape)}")
    v, nmat = mats.shape[:2]
    if ids is not None:
        _splat_tensor(f"{name}: ids", ids, torch.int32, (n,))
    _splat_tensor(f"{name}: count", count, torch.int32, (v, n))
    _splat_tensor(f"{name}: colour", colour, torch.float32, (n, 3))
    _splat_tensor(f"{name}: sh", sh, torch.float32)
    degrees = {gauss_sh_rows(d): d for d in range(1, GAUSS_SH_MAX_DEGREE + 1)}
    if sh.dim() != 3 or sh.shape[0] != n or sh.shape[2] != 3 or sh.shape[1] not in degrees:
        raise hip.MudgError(f"{name}: expected coefficients ({n}, K - 1, 3) with K - 1 in {tuple(degrees)}, got {tuple(sh.shape)}")
    degree = degrees[sh.shape[1]]
    active = degree if active is None else int(active)
    if not 0 <= active <= degree:
        raise hip.MudgError(f"{name}: active degree {active} of {degree}")
    return n, v, nmat, degree, active


def gauss_sh_colour(points, mats, count, colour, sh, *, ids=None, active=None):
    """One colour per (view, Gaussian): colours (V, n, 3) fp32 = max(0, colour + sum B_k(d) sh[k - 1]) in byte units, d the
    unit direction from the view's camera centre to the Gaussian in the Gaussian's own frame, +0 where count (V, n) is 0.  points, mats,
    ids and count as gauss_project takes and returns them; colour (n, 3), sh (n, K - 1, 3) fp32 with K = (L + 1)^2, L = 1, 2 or 3;
    active (default L): the highest degree the sum takes."""
    n, v, nmat, degree, active = _gauss_sh("gauss_sh_colour", points, mats, ids, count, colour, sh, active)
    colours = torch.empty((v, n, 3), dtype=torch.float32, device=points.device)
    hip.check(hip.lib().mudg_gauss_sh_colour(points.data_ptr(), _ptr(ids), n, mats.data_ptr(), v, nmat, count.data_ptr(), colour.data_ptr(),
                                             sh.data_ptr(), degree, active, colours.data_ptr(), _stream()), "mudg_gauss_sh_colour")
    return colours


def gauss_sh_bwd(points, mats, count, offsets, partial, colour, sh, *, ids=None, active=None):
    """gauss_sh_colour's backward from the partials of gauss_blend_bwd_views: d_colour (n, 3), d_sh (n, K - 1, 3) (+0 above the active
    degree) and d_xyz_dir (n, 3), the gradient that reaches the position through the direction; fp32, the views added in order."""
    n, v, nmat, degree, active = _gauss_sh("gauss_sh_bwd", points, mats, ids, count, colour, sh, active)
    _splat_tensor("gauss_sh_bwd: offsets", offsets, torch.int64, (v, n))
    _gauss_partial("gauss_sh_bwd", partial)
    d_colour = torch.empty_like(colour)
    d_sh = torch.empty_like(sh)
    d_xyz = torch.empty((n, 3), dtype=torch.float32, device=points.device)
    hip.check(hip.lib().mudg_gauss_sh_bwd(points.data_ptr(), _ptr(ids), n, mats.data_ptr(), v, nmat, count.data_ptr(), offsets.data_ptr(),
                                          partial.data_ptr(), partial.shape[0], colour.data_ptr(), sh.data_ptr(), degree, active,
                                          d_colour.data_ptr(), d_sh.data_ptr(), d_xyz.data_ptr(), _stream()), "mudg_gauss_sh_bwd")
    return d_colour, d_sh, d_xyz


GAUSS_POSE_CHUNK = 256           # Gaussians a workgroup of the pose gradient reduces
GAUSS_POSE_MAX_VIEWS = 65535     # the grid's second axis


def _gauss_pose_buffers(name, n, v, nmat, device):
    """The stage buffer (V, nmat, ceil(n / 256), 12) and d_mats (V, nmat, 12) of a pose gradient; more views than a grid holds are refused."""
    if v > GAUSS_POSE_MAX_VIEWS:
        raise hip.MudgError(f"{name}: {v} views (at most {GAUSS_POSE_MAX_VIEWS} a call)")
    chunks = (n + GAUSS_POSE_CHUNK - 1) // GAUSS_POSE_CHUNK
    return (torch.empty((v, nmat, chunks, 12), dtype=torch.float32, device=device),
            torch.empty((v, nmat, 12), dtype=torch.float32, device=device))


def gauss_pose_bwd(points, cov, mats, intr, hw, count, offsets, partial, *, ids=None, znear=0.2, zfar=200.0):
    """The gradient of the matrices: d_mats (V, nmat, 12) fp32 from the operands of gauss_project_bwd, the sum over every
    Gaussian that goes through a (view, matrix) in one fixed order; +0 for a matrix nobody goes through.  Without harmonics this is the
    whole gradient; with them gauss_sh_pose_bwd's tensor is added."""
    n, v, nmat = _gauss_cloud("gauss_pose_bwd", points, cov, mats, ids)
    if ids is None and nmat != 1:
        raise hip.MudgError(f"gauss_pose_bwd: {nmat} matrices per view need ids")
    _splat_tensor("gauss_pose_bwd: count", count, torch.int32, (v, n))
    _splat_tensor("gauss_pose_bwd: offsets", offsets, torch.int64, (v, n))
    _gauss_partial("gauss_pose_bwd", partial)
    h, w = (int(s) for s in hw)
    fx, fy, cx, cy = (float(s) for s in intr)
    stage, d_mats = _gauss_pose_buffers("gauss_pose_bwd", n, v, nmat, points.device)
    hip.check(hip.lib().mudg_gauss_pose_bwd(points.data_ptr(), cov.data_ptr(), _ptr(ids), n, mats.data_ptr(), v, nmat, h, w, fx, fy, cx, cy,
                                            float(znear), float(zfar), count.data_ptr(), offsets.data_ptr(), partial.data_ptr(),
                                            partial.shape[0], stage.data_ptr(), d_mats.data_ptr(), _stream()), "mudg_gauss_pose_bwd")
    return d_mats


def gauss_sh_pose_bwd(points, mats, count, offsets, partial, colour, sh, *, ids=None, active=None):
    """What reaches the matrices through the harmonics' direction: d_mats_dir (V, nmat, 12) fp32 from the operands of
    gauss_sh_bwd, summed as gauss_pose_bwd sums."""
    n, v, nmat, degree, active = _gauss_sh("gauss_sh_pose_bwd", points, mats, ids, count, colour, sh, active)
    if ids is None and nmat != 1:
        raise hip.MudgError(f"gauss_sh_pose_bwd: {nmat} matrices per view need ids")
    _splat_tensor("gauss_sh_pose_bwd: offsets", offsets, torch.int64, (v, n))
    _gauss_partial("gauss_sh_pose_bwd", partial)
    stage, d_mats = _gauss_pose_buffers("gauss_sh_pose_bwd", n, v, nmat, points.device)
    hip.check(hip.lib().mudg_gauss_sh_pose_bwd(points.data_ptr(), _ptr(ids), n, mats.data_ptr(), v, nmat, count.data_ptr(), offsets.data_ptr(),
                                               partial.data_ptr(), partial.shape[0], colour.data_ptr(), sh.data_ptr(), degree, active,
                                               stage.data_ptr(), d_mats.data_ptr(), _stream()), "mudg_gauss_sh_pose_bwd")
    return d_mats


def _gauss_entries_views(name, colours, uv, conic, depth, values_sorted, ranges, hw):
    """_gauss_entries for colours (V, n, 3): every view's slice is an (n, 3) colour tensor."""
    _splat_tensor(f"{name}: colours", colours, torch.float32)
    _splat_tensor(f"{name}: depth", depth, torch.float32)
    if colours.dim() != 3 or depth.dim() != 2 or tuple(colours.shape) != (*depth.shape, 3) or colours.shape[0] == 0:
        raise hip.MudgError(f"{name}: colours {tuple(colours.shape)} with depths {tuple(depth.shape)}")
    return _gauss_entries(name, colours[0], _GAUSS_COLOURS, uv, conic, depth, values_sorted, ranges, hw)


def gauss_blend_views(colours, uv, conic, depth, values_sorted, ranges, hw):
    """gauss_blend with one fp32 colour per (view, Gaussian), colours (V, n, 3) in byte units: rgb, depth, alpha."""
    v, n, h, w, _ = _gauss_entries_views("gauss_blend_views", colours, uv, conic, depth, values_sorted, ranges, hw)
    rgb, out_depth, alpha = _gauss_images(v, h, w, colours.device)
    hip.check(hip.lib().mudg_gauss_blend_views(colours.data_ptr(), uv.data_ptr(), conic.data_ptr(), depth.data_ptr(), values_sorted.data_ptr(),
                                               ranges.data_ptr(), n, values_sorted.numel(), v, h, w, rgb.data_ptr(), out_depth.data_ptr(),
                                               alpha.data_ptr(), _stream()), "mudg_gauss_blend_views")
    return rgb, out_depth, alpha


def gauss_blend_train_views(colours, uv, conic, depth, values_sorted, ranges, hw):
    """gauss_blend_train with colours (V, n, 3): rgb, depth, alpha and state (V, 5, H, W)."""
    v, n, h, w, _ = _gauss_entries_views("gauss_blend_train_views", colours, uv, conic, depth, values_sorted, ranges, hw)
    rgb, out_depth, alpha = _gauss_images(v, h, w, colours.device)
    state = torch.empty((v, 5, h, w), dtype=torch.float32, device=colours.device)
    hip.check(hip.lib().mudg_gauss_blend_train_views(colours.data_ptr(), uv.data_ptr(), conic.data_ptr(), depth.data_ptr(),
                                                     values_sorted.data_ptr(), ranges.data_ptr(), n, values_sorted.numel(), v, h, w,
                                                     rgb.data_ptr(), out_depth.data_ptr(), alpha.data_ptr(), state.data_ptr(), _stream()),
              "mudg_gauss_blend_train_views")
    return rgb, out_depth, alpha, state


def gauss_blend_bwd_views(colours, uv, conic, depth, values_sorted, order, ranges, hw, state, d_rgb, d_depth, d_alpha):
    """gauss_blend_bwd with colours (V, n, 3): partial (E, 10), whose columns 0 .. 2 are the gradient of an entry's (view, Gaussian) colour."""
    v, n, h, w, _ = _gauss_entries_views("gauss_blend_bwd_views", colours, uv, conic, depth, values_sorted, ranges, hw)
    e = values_sorted.numel()
    _splat_tensor("gauss_blend_bwd_views: order", order, torch.int64, (e,))
    _splat_tensor("gauss_blend_bwd_views: state", state, torch.float32, (v, 5, h, w))
    _splat_tensor("gauss_blend_bwd_views: d_rgb", d_rgb, torch.float32, (v, 3, h, w))
    _splat_tensor("gauss_blend_bwd_views: d_depth", d_depth, torch.float32, (v, h, w))
    _splat_tensor("gauss_blend_bwd_views: d_alpha", d_alpha, torch.float32, (v, h, w))
    partial = torch.empty((e, GAUSS_SUMS), dtype=torch.float32, device=colours.device)
    hip.check(hip.lib().mudg_gauss_blend_bwd_views(colours.data_ptr(), uv.data_ptr(), conic.data_ptr(), depth.data_ptr(), values_sorted.data_ptr(),
                                                   order.data_ptr(), ranges.data_ptr(), n, e, v, h, w, state.data_ptr(), d_rgb.data_ptr(),
                                                   d_depth.data_ptr(), d_alpha.data_ptr(), partial.data_ptr(), _stream()),
              "mudg_gauss_blend_bwd_views")
    return partial


GAUSS_KEEP, GAUSS_PRUNE, GAUSS_CLONE, GAUSS_SPLIT = 0, 1, 2, 3      # the plan's action codes
GAUSS_PARAMETER_WIDTHS = (3, 3, 3, 4, 1)                            # xyz, colour, log_scale, quat, opacity_logit


def gauss_density_accumulate(partial, count, offsets, hw, grad_sum, seen):
    """Add every Gaussian's screen-space gradient norm of this backward to grad_sum (n,) fp32 and the views that counted it to seen (n,)
    int32, in place.  partial (E, 10), count (V, n) and offsets (V, n) are gauss_project_bwd's."""
    _splat_tensor("gauss_density_accumulate: count", count, torch.int32)
    if count.dim() != 2 or count.numel() == 0:
        raise hip.MudgError(f"gauss_density_accumulate: expected counts (V > 0, n > 0), got {tuple(count.shape)}")
    v, n = count.shape
    _splat_tensor("gauss_density_accumulate: offsets", offsets, torch.int64, (v, n))
    _gauss_partial("gauss_density_accumulate", partial)
    _splat_tensor("gauss_density_accumulate: grad_sum", grad_sum, torch.float32, (n,))
    _splat_tensor("gauss_density_accumulate: seen", seen, torch.int32, (n,))
    h, w = (int(s) for s in hw)
    hip.check(hip.lib().mudg_gauss_density_accumulate(partial.data_ptr(), count.data_ptr(), offsets.data_ptr(), n, v, h, w, partial.shape[0],
                                                      grad_sum.data_ptr(), seen.data_ptr(), _stream()), "mudg_gauss_density_accumulate")


def gauss_density_plan(grad_sum, seen, opacity, scale, *, grad_threshold, split_scale, min_opacity, max_scale, grow=True):
    """What becomes of every Gaussian: action (n,) int32 (GAUSS_KEEP, GAUSS_PRUNE, GAUSS_CLONE, GAUSS_SPLIT) and rows (n,)
    int32, the rows it leaves (1, 0, 2, 2).  opacity (n,) and scale (n, 3) = exp(log_scale) come evaluated."""
    _splat_tensor("gauss_density_plan: grad_sum", grad_sum, torch.float32)
    if grad_sum.dim() != 1 or grad_sum.numel() == 0:
        raise hip.MudgError(f"gauss_density_plan: expected (n > 0,) gradient sums, got {tuple(grad_sum.shape)}")
    n = grad_sum.shape[0]
    _splat_tensor("gauss_density_plan: seen", seen, torch.int32, (n,))
    _splat_tensor("gauss_density_plan: opacity", opacity, torch.float32, (n,))
    _splat_tensor("gauss_density_plan: scale", scale, torch.float32, (n, 3))
    action = torch.empty((n,), dtype=torch.int32, device=grad_sum.device)
    rows = torch.empty((n,), dtype=torch.int32, device=grad_sum.device)
    hip.check(hip.lib().mudg_gauss_density_plan(grad_sum.data_ptr(), seen.data_ptr(), opacity.data_ptr(), scale.data_ptr(), n,
                                                float(grad_threshold), float(split_scale), float(min_opacity), float(max_scale), int(bool(grow)),
                                                action.data_ptr(), rows.data_ptr(), _stream()), "mudg_gauss_density_plan")
    return action, rows


def gauss_density_apply(action, start, n_out, scale, rot, tensors, *, split_offset, log_shrink, ids=None):
    """Rewrite the fifteen tensors of a fit as the plan says.  tensors: for each of xyz (n, 3), colour (n, 3), log_scale
    (n, 3), quat (n, 4), opacity_logit (n,) the value and its two Adam moments, fifteen fp32 tensors in that order; start (n,) int64 the
    exclusive sum of the plan's rows, n_out its total; scale (n, 3) and rot (n, 9) evaluated by the caller.  Returns the fifteen tensors
    with n_out rows and ids with n_out rows (or None).  A start that is the exclusive sum of the plan's rows writes every row once."""
    _splat_tensor("gauss_density_apply: action", action, torch.int32)
    if action.dim() != 1 or action.numel() == 0:
        raise hip.MudgError(f"gauss_density_apply: expected (n > 0,) actions, got {tuple(action.shape)}")
    n, m = action.shape[0], int(n_out)
    if m <= 0:
        raise hip.MudgError(f"gauss_density_apply: {m} rows out")
    _splat_tensor("gauss_density_apply: start", start, torch.int64, (n,))
    _splat_tensor("gauss_density_apply: scale", scale, torch.float32, (n, 3))
    _splat_tensor("gauss_density_apply: rot", rot, torch.float32, (n, 9))
    tensors = list(tensors)
    if len(tensors) != 3 * len(GAUSS_PARAMETER_WIDTHS):
        raise hip.MudgError(f"gauss_density_apply: {len(tensors)} tensors (five parameters with two moments each)")
    for k, t in enumerate(tensors):
        width = GAUSS_PARAMETER_WIDTHS[k // 3]
        _splat_tensor(f"gauss_density_apply: tensor {k}", t, torch.float32, (n,) if width == 1 else (n, width))
    if ids is not None:
        _splat_tensor("gauss_density_apply: ids", ids, torch.int32, (n,))
    dev = action.device
    outs = [torch.empty((m,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev) for t in tensors]
    ids_out = None if ids is None else torch.empty((m,), dtype=torch.int32, device=dev)
    table = hip.C.c_void_p * len(tensors)                                   # read by the call itself, before it returns
    src, dst = table(*[t.data_ptr() for t in tensors]), table(*[t.data_ptr() for t in outs])
    hip.check(hip.lib().mudg_gauss_density_apply(action.data_ptr(), start.data_ptr(), n, m, scale.data_ptr(), rot.data_ptr(), float(split_offset),
                                                 float(log_shrink), src, dst, _ptr(ids), _ptr(ids_out), _stream()), "mudg_gauss_density_apply")
    return outs, ids_out


GAUSS_LOSS_COLS, GAUSS_LOSS_TOTALS = 4, 8                           # a tile's partial row; the finish buffer


def _gauss_loss_images(name, rgb, targets, depth, depth_targets):
    _splat_tensor(f"{name}: rgb", rgb, torch.float32)
    if rgb.dim() != 4 or rgb.shape[1] != 3 or rgb.numel() == 0:
        raise hip.MudgError(f"{name}: expected (V > 0, 3, H > 0, W > 0) images, got {tuple(rgb.shape)}")
    v, _, h, w = rgb.shape
    _splat_tensor(f"{name}: targets", targets, torch.float32, (v, 3, h, w))
    if (depth is None) != (depth_targets is None):
        raise hip.MudgError(f"{name}: depth and depth_targets come together or not at all")
    if depth is not None:
        _splat_tensor(f"{name}: depth", depth, torch.float32, (v, h, w))
        _splat_tensor(f"{name}: depth_targets", depth_targets, torch.float32, (v, h, w))
    tx, ty = gauss_tiles(h, w)
    return v, h, w, tx * ty


def gauss_loss(rgb, targets, depth=None, depth_targets=None):
    """The forward of the fit's image loss.  rgb and targets (V, 3, H, W), depth and depth_targets (V, H, W) or both None:
    fp32 on the GPU.  Returns maps (V, 3, 3, H, W), the derivatives of every pixel's SSIM value with respect to the three windowed moments
    of rgb, and partial (V, 3, NT, 4): each 16 x 16 tile's sum |x - y|, sum S, depth sum and depth count (int32 bits).  The window is
    SSIM_WINDOW / 65536 with zero padding on float images: not metrics.psnr_ssim's convention (uint8, valid region, integer moments)."""
    v, h, w, nt = _gauss_loss_images("gauss_loss", rgb, targets, depth, depth_targets)
    maps = torch.empty((v, 3, 3, h, w), dtype=torch.float32, device=rgb.device)
    partial = torch.empty((v, 3, nt, GAUSS_LOSS_COLS), dtype=torch.float32, device=rgb.device)
    hip.check(hip.lib().mudg_gauss_loss(rgb.data_ptr(), targets.data_ptr(), _ptr(depth), _ptr(depth_targets), v, h, w, maps.data_ptr(),
                                        partial.data_ptr(), _stream()), "mudg_gauss_loss")
    return maps, partial


def gauss_loss_finish(partial, hw, *, ssim_weight, depth_weight=0.0):
    """gauss_loss's partials (V, 3, NT, 4) of (H, W) images -> totals (8,) fp32: the loss, mean |x - y|, mean S, the depth mean,
    float(max(count, 1)), the depth count as int32 bits, 0, 0.  One workgroup, one fixed order, no host synchronisation."""
    h, w = (int(s) for s in hw)
    tx, ty = gauss_tiles(h, w)
    _splat_tensor("gauss_loss_finish: partial", partial, torch.float32)
    if partial.dim() != 4 or partial.shape[0] == 0 or tuple(partial.shape[1:]) != (3, tx * ty, GAUSS_LOSS_COLS):
        raise hip.MudgError(f"gauss_loss_finish: expected partials (V > 0, 3, {tx * ty}, {GAUSS_LOSS_COLS}) for {h} x {w}, got {tuple(partial.shape)}")
    totals = torch.empty((GAUSS_LOSS_TOTALS,), dtype=torch.float32, device=partial.device)
    hip.check(hip.lib().mudg_gauss_loss_finish(partial.data_ptr(), partial.shape[0], h, w, float(ssim_weight), float(depth_weight),
                                               totals.data_ptr(), _stream()), "mudg_gauss_loss_finish")
    return totals


def gauss_loss_bwd(rgb, targets, maps, totals, upstream, depth=None, depth_targets=None, *, ssim_weight, depth_weight=0.0, want_depth=True):
    """The backward of the fit's image loss: d_rgb (V, 3, H, W) and d_depth (V, H, W) (None without the depth pair or with
    want_depth false).  maps and totals are gauss_loss's and gauss_loss_finish's; upstream is the loss's gradient, one fp32 on the GPU,
    read by the kernel."""
    v, h, w, _ = _gauss_loss_images("gauss_loss_bwd", rgb, targets, depth, depth_targets)
    _splat_tensor("gauss_loss_bwd: maps", maps, torch.float32, (v, 3, 3, h, w))
    _splat_tensor("gauss_loss_bwd: totals", totals, torch.float32, (GAUSS_LOSS_TOTALS,))
    _splat_tensor("gauss_loss_bwd: upstream", upstream, torch.float32)
    if upstream.numel() != 1:
        raise hip.MudgError(f"gauss_loss_bwd: the upstream gradient is one number, got {tuple(upstream.shape)}")
    d_rgb = torch.empty((v, 3, h, w), dtype=torch.float32, device=rgb.device)
    d_depth = torch.empty((v, h, w), dtype=torch.float32, device=rgb.device) if depth is not None and want_depth else None
    hip.check(hip.lib().mudg_gauss_loss_bwd(rgb.data_ptr(), targets.data_ptr(), maps.data_ptr(), _ptr(depth), _ptr(depth_targets),
                                            totals.data_ptr(), upstream.data_ptr(), v, h, w, float(ssim_weight), float(depth_weight),
                                            d_rgb.data_ptr(), _ptr(d_depth), _stream()), "mudg_gauss_loss_bwd")
    return d_rgb, d_depth


GAUSS_FEAT_MAX = 32                                                 # feature values (class scores) a Gaussian may carry
GAUSS_CLASS_COLS, GAUSS_CLASS_TOTALS = 2, 4                         # a tile's partial row; the finish buffer


def _gauss_entries_feat(name, colours, feat, uv, conic, depth, values_sorted, ranges, hw):
    """The operands of the two blends with features: colours (n, 3) or (V, n, 3) and feat (n, F) -> (colour_views, F, V, n, h, w)."""
    per_view = torch.is_tensor(colours) and colours.dim() == 3
    shared = _gauss_entries_views if per_view else (lambda nm, c, *rest: _gauss_entries(nm, c, _GAUSS_COLOURS, *rest))
    v, n, h, w, _ = shared(name, colours, uv, conic, depth, values_sorted, ranges, hw)
    _splat_tensor(f"{name}: feat", feat, torch.float32)
    if feat.dim() != 2 or feat.shape[0] != n or not 1 <= feat.shape[1] <= GAUSS_FEAT_MAX:
        raise hip.MudgError(f"{name}: expected features ({n}, 1 .. {GAUSS_FEAT_MAX}), got {tuple(feat.shape)}")
    return int(per_view), feat.shape[1], v, n, h, w


def gauss_blend_feat(colours, feat, uv, conic, depth, values_sorted, ranges, hw, *, with_state=True):
    """gauss_blend_train (colours (n, 3)) or gauss_blend_train_views (colours (V, n, 3)) that also blends feat (n, F) fp32, 1 <= F <= 32
    (DESIGN.md §29).  Returns rgb, depth, alpha and state with that call's bits (state None with with_state false: inference) and
    feat_out (V, F, H, W) fp32, the raw sums of feat[g][k] w, which are their own state."""
    views, f, v, n, h, w = _gauss_entries_feat("gauss_blend_feat", colours, feat, uv, conic, depth, values_sorted, ranges, hw)
    dev = feat.device
    rgb, out_depth, alpha = _gauss_images(v, h, w, dev)
    feat_out = torch.empty((v, f, h, w), dtype=torch.float32, device=dev)
    state = torch.empty((v, 5, h, w), dtype=torch.float32, device=dev) if with_state else None
    hip.check(hip.lib().mudg_gauss_blend_feat(colours.data_ptr(), views, feat.data_ptr(), f, uv.data_ptr(), conic.data_ptr(), depth.data_ptr(),
                                              values_sorted.data_ptr(), ranges.data_ptr(), n, values_sorted.numel(), v, h, w, rgb.data_ptr(),
                                              out_depth.data_ptr(), alpha.data_ptr(), feat_out.data_ptr(), _ptr(state), _stream()),
              "mudg_gauss_blend_feat")
    return rgb, out_depth, alpha, feat_out, state


def gauss_blend_bwd_feat(colours, feat, uv, conic, depth, values_sorted, order, ranges, hw, state, feat_out, d_rgb, d_depth, d_alpha, d_feat):
    """gauss_blend_bwd (or _views) with the features' share: partial (E, 10) as that call returns it, and partial_feat (E, F) fp32, the
    sums over the tile's pixels of d_feat[k] w at the entry's unsorted position, in the same fixed order."""
    views, f, v, n, h, w = _gauss_entries_feat("gauss_blend_bwd_feat", colours, feat, uv, conic, depth, values_sorted, ranges, hw)
    e = values_sorted.numel()
    if e * f >= 2 ** 31:
        raise hip.MudgError(f"gauss_blend_bwd_feat: {e} entries of {f} features (E F < 2^31)")
    _splat_tensor("gauss_blend_bwd_feat: order", order, torch.int64, (e,))
    _splat_tensor("gauss_blend_bwd_feat: state", state, torch.float32, (v, 5, h, w))
    _splat_tensor("gauss_blend_bwd_feat: feat_out", feat_out, torch.float32, (v, f, h, w))
    _splat_tensor("gauss_blend_bwd_feat: d_rgb", d_rgb, torch.float32, (v, 3, h, w))
    _splat_tensor("gauss_blend_bwd_feat: d_depth", d_depth, torch.float32, (v, h, w))
    _splat_tensor("gauss_blend_bwd_feat: d_alpha", d_alpha, torch.float32, (v, h, w))
    _splat_tensor("gauss_blend_bwd_feat: d_feat", d_feat, torch.float32, (v, f, h, w))
    partial = torch.empty((e, GAUSS_SUMS), dtype=torch.float32, device=feat.device)
    partial_feat = torch.empty((e, f), dtype=torch.float32, device=feat.device)
    hip.check(hip.lib().mudg_gauss_blend_bwd_feat(colours.data_ptr(), views, feat.data_ptr(), f, uv.data_ptr(), conic.data_ptr(), depth.data_ptr(),
                                                  values_sorted.data_ptr(), order.data_ptr(), ranges.data_ptr(), n, e, v, h, w, state.data_ptr(),
                                                  feat_out.data_ptr(), d_rgb.data_ptr(), d_depth.data_ptr(), d_alpha.data_ptr(),
                                                  d_feat.data_ptr(), partial.data_ptr(), partial_feat.data_ptr(), _stream()),
              "mudg_gauss_blend_bwd_feat")
    return partial, partial_feat


def gauss_feat_bwd(count, offsets, partial_feat):
    """Every Gaussian's rows of partial_feat (E, F) gathered per view in ascending order, the views added in order: d_feat (n, F) fp32.
    count (V, n) int32 and offsets (V, n) int64 are gauss_project_bwd's, with its guards."""
    _splat_tensor("gauss_feat_bwd: count", count, torch.int32)
    if count.dim() != 2 or count.numel() == 0:
        raise hip.MudgError(f"gauss_feat_bwd: expected counts (V > 0, n > 0), got {tuple(count.shape)}")
    v, n = count.shape
    _splat_tensor("gauss_feat_bwd: offsets", offsets, torch.int64, (v, n))
    _splat_tensor("gauss_feat_bwd: partial_feat", partial_feat, torch.float32)
    if partial_feat.dim() != 2 or partial_feat.shape[0] == 0 or not 1 <= partial_feat.shape[1] <= GAUSS_FEAT_MAX:
        raise hip.MudgError(f"gauss_feat_bwd: expected partials (E > 0, 1 .. {GAUSS_FEAT_MAX}), got {tuple(partial_feat.shape)}")
    e, f = partial_feat.shape
    d_feat = torch.empty((n, f), dtype=torch.float32, device=count.device)
    hip.check(hip.lib().mudg_gauss_feat_bwd(count.data_ptr(), offsets.data_ptr(), partial_feat.data_ptr(), e, n, v, f, d_feat.data_ptr(),
                                            _stream()), "mudg_gauss_feat_bwd")
    return d_feat


def _gauss_scores(name, x):
    _splat_tensor(f"{name}: x", x, torch.float32)
    if x.dim() != 4 or x.numel() == 0 or not 1 <= x.shape[1] <= GAUSS_FEAT_MAX:
        raise hip.MudgError(f"{name}: expected (V > 0, 1 .. {GAUSS_FEAT_MAX}, H > 0, W > 0) scores, got {tuple(x.shape)}")
    return tuple(x.shape)


def gauss_class_loss(x, labels):
    """The forward of the class loss.  x (V, F, H, W) fp32 blended scores, labels (V, H, W) uint8; a pixel is labelled iff
    its label is below F.  Returns maps (V, F, H, W) = softmax(x) - onehot(label) (+0 where unlabelled) and partial (V NT, 2): each
    16 x 16 tile's sum of log S - p_label and its labelled count (int32 bits)."""
    v, f, h, w = _gauss_scores("gauss_class_loss", x)
    _splat_tensor("gauss_class_loss: labels", labels, torch.uint8, (v, h, w))
    tx, ty = gauss_tiles(h, w)
    maps = torch.empty((v, f, h, w), dtype=torch.float32, device=x.device)
    partial = torch.empty((v * tx * ty, GAUSS_CLASS_COLS), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().mudg_gauss_class_loss(x.data_ptr(), labels.data_ptr(), v, f, h, w, maps.data_ptr(), partial.data_ptr(), _stream()),
              "mudg_gauss_class_loss")
    return maps, partial


def gauss_class_loss_finish(partial, views, hw, *, weight=1.0):
    """gauss_class_loss's partials of `views` (H, W) images -> totals (4,) fp32: the sum of the pixels' losses, the labelled count as int32
    bits, float(max(count, 1)) and the loss weight sum / max(count, 1).  One workgroup, one fixed order, no host synchronisation."""
    h, w = (int(s) for s in hw)
    tx, ty = gauss_tiles(h, w)
    _splat_tensor("gauss_class_loss_finish: partial", partial, torch.float32, (int(views) * tx * ty, GAUSS_CLASS_COLS))
    totals = torch.empty((GAUSS_CLASS_TOTALS,), dtype=torch.float32, device=partial.device)
    hip.check(hip.lib().mudg_gauss_class_loss_finish(partial.data_ptr(), int(views), h, w, float(weight), totals.data_ptr(), _stream()),
              "mudg_gauss_class_loss_finish")
    return totals


def gauss_class_loss_bwd(maps, totals, upstream, *, weight=1.0):
    """The backward of the class loss: d_x (V, F, H, W) = ((upstream weight) / totals[2]) maps.  upstream is the loss's gradient, one
    fp32 on the GPU, read by the kernel."""
    v, f, h, w = _gauss_scores("gauss_class_loss_bwd", maps)
    _splat_tensor("gauss_class_loss_bwd: totals", totals, torch.float32, (GAUSS_CLASS_TOTALS,))
    _splat_tensor("gauss_class_loss_bwd: upstream", upstream, torch.float32)
    if upstream.numel() != 1:
        raise hip.MudgError(f"gauss_class_loss_bwd: the upstream gradient is one number, got {tuple(upstream.shape)}")
    d_x = torch.empty_like(maps)
    hip.check(hip.lib().mudg_gauss_class_loss_bwd(maps.data_ptr(), totals.data_ptr(), upstream.data_ptr(), float(weight), v, f, h, w,
                                                  d_x.data_ptr(), _stream()), "mudg_gauss_class_loss_bwd")
    return d_x


# ------------------------------------------------------------------------------------------------ metric depth and lifted views
def _depth_frames(name, frames):
    _splat_tensor(f"{name}: frames", frames, torch.uint8)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise hip.MudgError(f"{name}: expected (frames, h, w, 3) uint8 frames, got {tuple(frames.shape)}")
    return tuple(frames.shape[:3])


def depth_align_sums(frames, lidar):
    """frames (f, h, w, 3) uint8, the depth stream; lidar (f, h, w) fp32 metres -> (f, 5) int64 integer sums n, sum k, sum k^2, sum q,
    sum k q over the pixels with k = r + g + b > 0 and 0 < lidar < 256, q = rint(lidar * 2^20)."""
    f, h, w = _depth_frames("depth_align_sums", frames)
    _splat_tensor("depth_align_sums: lidar", lidar, torch.float32, (f, h, w))
    sums = torch.zeros((f, 5), dtype=torch.int64, device=frames.device)
    hip.check(hip.lib().mudg_depth_align_sums(frames.data_ptr(), lidar.data_ptr(), f, h, w, sums.data_ptr(), _stream()), "mudg_depth_align_sums")
    return sums


def depth_align_solve(sums):
    """(f, 5) sums -> (coef (f, 2) float64 = (m, c) of lidar ~ m * (k / 765) + c, fitted (f,) uint8); a frame with fewer than two counted
    pixels or no spread in k gets (100, 0) and fitted = 0.  Nothing comes to the host."""
    _splat_tensor("depth_align_solve: sums", sums, torch.int64)
    if sums.dim() != 2 or sums.shape[1] != 5 or sums.shape[0] == 0:
        raise hip.MudgError(f"depth_align_solve: expected (frames, 5) sums, got {tuple(sums.shape)}")
    coef = torch.empty((sums.shape[0], 2), dtype=torch.float64, device=sums.device)
    fitted = torch.empty((sums.shape[0],), dtype=torch.uint8, device=sums.device)
    hip.check(hip.lib().mudg_depth_align_solve(sums.data_ptr(), sums.shape[0], coef.data_ptr(), fitted.data_ptr(), _stream()), "mudg_depth_align_solve")
    return coef, fitted


def depth_finish(frames, coef, labels=None, *, sky_label=10, visualise=False):
    """frames (f, h, w, 3) uint8 and coef (f, 2) float64 -> depth (f, h, w) fp32 metres in [0, 100], 100 where labels (f, h, w) int64
    equals sky_label; with visualise also the Spectral picture of depth / 100, (f, h, w, 3) uint8.  Returns (depth, vis or None)."""
    f, h, w = _depth_frames("depth_finish", frames)
    _splat_tensor("depth_finish: coef", coef, torch.float64, (f, 2))
    if labels is not None:
        _splat_tensor("depth_finish: labels", labels, torch.int64, (f, h, w))
    depth = torch.empty((f, h, w), dtype=torch.float32, device=frames.device)
    vis = torch.empty((f, h, w, 3), dtype=torch.uint8, device=frames.device) if visualise else None
    hip.check(hip.lib().mudg_depth_finish(frames.data_ptr(), coef.data_ptr(), _ptr(labels), int(sky_label), f, h, w, depth.data_ptr(), _ptr(vis),
                                          _stream()), "mudg_depth_finish")
    return depth, vis


def colormap_spectral(values, val_min=0.0, val_max=1.0, *, reversed=False, bytes=True):
    """fp32 values of any shape -> their Spectral colours, shape + (3,): uint8 (bytes) or fp32, the reference's method_custom operation
    for operation (eval_tools.py:206-246); values are first taken from [val_min, val_max] to [0, 1] unless that range is (0, 1)."""
    _splat_tensor("colormap_spectral: values", values, torch.float32)
    if values.numel() == 0:
        raise hip.MudgError("colormap_spectral: no values")
    if not float(val_max) > float(val_min):
        raise hip.MudgError(f"colormap_spectral: invalid values range [{val_min}, {val_max}]")
    out = torch.empty(tuple(values.shape) + (3,), dtype=torch.uint8 if bytes else torch.float32, device=values.device)
    hip.check(hip.lib().mudg_colormap_spectral(values.data_ptr(), values.numel(), float(val_min), float(val_max), int(bool(reversed)),
                                               out.data_ptr() if bytes else None, None if bytes else out.data_ptr(), _stream()), "mudg_colormap_spectral")
    return out


def depth_unproject(depth, rgb, table, labels=None, *, sky_label=10, min_depth=0.0, max_depth=100.0):
    """depth (f, h, w) fp32 metres, rgb (f, h, w, 3) uint8 and table (f, 16) float64 (the top three rows of camera-to-world, then
    fx, fy, cx, cy at (h, w)) -> packed points (f * h * w, 4) int32 and valid (f * h * w,) uint8: a pixel is valid iff
    min_depth < depth < max_depth and its label is not sky_label; one that is not stores a zero point."""
    f, h, w = _depth_frames("depth_unproject", rgb)
    _splat_tensor("depth_unproject: depth", depth, torch.float32, (f, h, w))
    _splat_tensor("depth_unproject: table", table, torch.float64, (f, 16))
    if labels is not None:
        _splat_tensor("depth_unproject: labels", labels, torch.int64, (f, h, w))
    points = torch.empty((f * h * w, 4), dtype=torch.int32, device=depth.device)
    valid = torch.empty((f * h * w,), dtype=torch.uint8, device=depth.device)
    hip.check(hip.lib().mudg_depth_unproject(depth.data_ptr(), rgb.data_ptr(), _ptr(labels), int(sky_label), table.data_ptr(), f, h, w,
                                             float(min_depth), float(max_depth), points.data_ptr(), valid.data_ptr(), _stream()), "mudg_depth_unproject")
    return points, valid


# ------------------------------------------------------------------------------------------------ cross-view depth consistency
VIEW_MAX_WITNESSES = 64          # per view (csrc/consistency.hip): the verdict counts fit a byte
VIEW_MAX_RADIUS = 2
VIEW_DYNAMIC_MASK = sum(1 << c for c in range(11, 19))      # the movable classes of semantic_nearest's 19: person .. bicycle


def _view_depths(name, depth):
    _splat_tensor(f"{name}: depth", depth, torch.float32)
    if depth.dim() != 3 or depth.numel() == 0:
        raise hip.MudgError(f"{name}: expected (views, h, w) fp32 depths, got {tuple(depth.shape)}")
    return tuple(depth.shape)


def view_flags(depth, labels=None, *, sky_label=10, dynamic_mask=VIEW_DYNAMIC_MASK, min_depth=0.0, max_depth=100.0):
    """depth (v, h, w) fp32 metres and labels (v, h, w) int64 or None -> flags (v, h, w) uint8: bit 0 usable iff
    min_depth < depth < max_depth and the label is not sky_label, bit 1 dynamic iff 0 <= label < 64 and that bit of dynamic_mask is set."""
    v, h, w = _view_depths("view_flags", depth)
    if labels is not None:
        _splat_tensor("view_flags: labels", labels, torch.int64, (v, h, w))
    mask = int(dynamic_mask)
    if not 0 <= mask < 1 << 64:
        raise hip.MudgError(f"view_flags: dynamic_mask {dynamic_mask} (64 bits, one per class)")
    flags = torch.empty((v, h, w), dtype=torch.uint8, device=depth.device)
    hip.check(hip.lib().mudg_view_flags(depth.data_ptr(), _ptr(labels), int(sky_label), mask, v, h, w, float(min_depth), float(max_depth),
                                        flags.data_ptr(), _stream()), "mudg_view_flags")
    return flags


def view_witness_lists(times, witnesses, views):
    """The host side of view_consistency's argument check, which the entry point cannot make on device memory: times (views,) and
    witnesses (views, 1 .. 64) integer host arrays, every witness id -1 (empty) or 0 .. views - 1.  Returns both as contiguous int32."""
    import numpy as np
    if torch.is_tensor(times) or torch.is_tensor(witnesses):
        raise hip.MudgError("view_consistency: times and witnesses are host arrays (their ids are checked before the launch)")
    times, witnesses = np.asarray(times), np.asarray(witnesses)
    if times.shape != (views,) or witnesses.ndim != 2 or witnesses.shape[0] != views or not 1 <= witnesses.shape[1] <= VIEW_MAX_WITNESSES \
            or times.dtype.kind not in "iu" or witnesses.dtype.kind not in "iu":
        raise hip.MudgError(f"view_consistency: times {times.shape} {times.dtype} and witnesses {witnesses.shape} {witnesses.dtype} for {views} views "
                            f"(integers, (views,) and (views, 1 .. {VIEW_MAX_WITNESSES}))")
    if int(witnesses.min()) < -1 or int(witnesses.max()) >= views:
        raise hip.MudgError(f"view_consistency: witness ids in [{int(witnesses.min())}, {int(witnesses.max())}] for {views} views (-1: empty, else 0 .. {views - 1})")
    if int(times.min()) < -2 ** 31 or int(times.max()) >= 2 ** 31:
        raise hip.MudgError("view_consistency: time ids are 32-bit integers")
    return np.ascontiguousarray(times, dtype=np.int32), np.ascontiguousarray(witnesses, dtype=np.int32)


def view_consistency(depth, flags, src_table, wit_table, times, witnesses, *, r=1, min_agree=2, max_violate=0, rel_tol=0.02, abs_tol=0.2):
    """depth (v, h, w) fp32, flags (v, h, w) uint8 of view_flags, src_table and wit_table (v, 16) float64 on the GPU (camera-to-world and
    world-to-camera rows, each followed by fx, fy, cx, cy); times (v,) and witnesses (v, n) integers on the HOST (view_witness_lists checks
    them before anything is launched).  Returns (agree, violate, keep (v, h, w) uint8, stats (v, 6) int64: usable, tested, kept, sum
    agree, sum violate, pixels with a violation) by DESIGN.md §21's rule."""
    v, h, w = _view_depths("view_consistency", depth)
    _splat_tensor("view_consistency: flags", flags, torch.uint8, (v, h, w))
    _splat_tensor("view_consistency: src_table", src_table, torch.float64, (v, 16))
    _splat_tensor("view_consistency: wit_table", wit_table, torch.float64, (v, 16))
    times, witnesses = view_witness_lists(times, witnesses, v)
    if r not in range(VIEW_MAX_RADIUS + 1) or int(min_agree) < 0 or int(max_violate) < 0 or not (float(rel_tol) >= 0.0 and float(abs_tol) >= 0.0):
        raise hip.MudgError(f"view_consistency: r {r} (0 .. {VIEW_MAX_RADIUS}), min_agree {min_agree}, max_violate {max_violate}, rel_tol {rel_tol}, "
                            f"abs_tol {abs_tol} (none negative)")
    dev = depth.device
    times_d, wit_d = torch.from_numpy(times).to(dev), torch.from_numpy(witnesses).to(dev)
    agree, violate, keep = (torch.empty((v, h, w), dtype=torch.uint8, device=dev) for _ in range(3))
    stats = torch.zeros((v, 6), dtype=torch.int64, device=dev)
    hip.check(hip.lib().mudg_view_consistency(depth.data_ptr(), flags.data_ptr(), src_table.data_ptr(), wit_table.data_ptr(), times_d.data_ptr(),
                                              wit_d.data_ptr(), v, witnesses.shape[1], h, w, int(r), int(min_agree), int(max_violate), float(rel_tol),
                                              float(abs_tol), agree.data_ptr(), violate.data_ptr(), keep.data_ptr(), stats.data_ptr(), _stream()),
              "mudg_view_consistency")
    return agree, violate, keep, stats


# ------------------------------------------------------------------------------------------------ scores of generated views
SSIM_WINDOW = (67, 498, 2359, 7167, 13960, 17434, 13960, 7167, 2359, 498, 67)     # the taps sum to 2^16
SSIM_TILE = 32                   # outputs per side of one workgroup of mudg_metric_ssim


def _metric_pair(name, a, b):
    f, h, w = _depth_frames(name, a)
    _splat_tensor(f"{name}: the second stack", b, torch.uint8, (f, h, w, 3))
    return f, h, w


def metric_sse(a, b):
    """Two (f, h, w, 3) uint8 frame stacks -> (f,) int64, the sum of (a - b)^2 over all pixels and channels of every frame."""
    f, h, w = _metric_pair("metric_sse", a, b)
    sse = torch.zeros((f,), dtype=torch.int64, device=a.device)
    hip.check(hip.lib().mudg_metric_sse(a.data_ptr(), b.data_ptr(), f, h, w, sse.data_ptr(), _stream()), "mudg_metric_sse")
    return sse


def metric_ssim(a, b):
    """Two (f, h, w, 3) uint8 frame stacks, h, w >= 11 -> (f,) int64, the sum over the valid region (h - 10) x (w - 10) and the three
    channels of rint(SSIM 2^32) per pixel (integer window, exact moments, fp64 in a stated order)."""
    f, h, w = _metric_pair("metric_ssim", a, b)
    if h < len(SSIM_WINDOW) or w < len(SSIM_WINDOW):
        raise hip.MudgError(f"metric_ssim: {h} x {w} frames, the 11 x 11 window needs at least 11 x 11")
    sums = torch.zeros((f,), dtype=torch.int64, device=a.device)
    hip.check(hip.lib().mudg_metric_ssim(a.data_ptr(), b.data_ptr(), f, h, w, sums.data_ptr(), _stream()), "mudg_metric_ssim")
    return sums


def metric_depth(depth, lidar, *, min_depth=0.1, max_depth=80.0):
    """depth and lidar (f, h, w) fp32 metres -> (f, 8) int64: n, sum rint(e 2^20), sum rint(e e 2^20), sum rint(r 2^20), the counts of
    t < 1.25, 1.25^2, 1.25^3 and a zero, over the pixels with min_depth < lidar < max_depth whose depth is a number."""
    _splat_tensor("metric_depth: depth", depth, torch.float32)
    if depth.dim() != 3 or depth.numel() == 0:
        raise hip.MudgError(f"metric_depth: expected (frames, h, w) depths, got {tuple(depth.shape)}")
    f, h, w = depth.shape
    _splat_tensor("metric_depth: lidar", lidar, torch.float32, (f, h, w))
    if not (2.0 ** -6 <= float(min_depth) < float(max_depth) <= 256.0):
        raise hip.MudgError(f"metric_depth: depth range ({min_depth}, {max_depth}), expected 2^-6 <= min_depth < max_depth <= 256")
    sums = torch.zeros((f, 8), dtype=torch.int64, device=depth.device)
    hip.check(hip.lib().mudg_metric_depth(depth.data_ptr(), lidar.data_ptr(), f, h, w, float(min_depth), float(max_depth), sums.data_ptr(),
                                          _stream()), "mudg_metric_depth")
    return sums


def metric_confusion(pred, gt, classes=19):
    """pred and gt (f, h, w) int64 label maps -> (confusion (f, classes, classes) int64 indexed [gt][pred], bad (f,) int64).  A pixel
    whose gt is outside [0, classes) is ignored; one whose pred is outside is counted in bad and in no cell."""
    _splat_tensor("metric_confusion: pred", pred, torch.int64)
    if pred.dim() != 3 or pred.numel() == 0:
        raise hip.MudgError(f"metric_confusion: expected (frames, h, w) labels, got {tuple(pred.shape)}")
    f, h, w = pred.shape
    _splat_tensor("metric_confusion: gt", gt, torch.int64, (f, h, w))
    classes = int(classes)
    if not 1 <= classes <= 32:
        raise hip.MudgError(f"metric_confusion: {classes} classes, expected 1 .. 32")
    confusion = torch.zeros((f, classes, classes), dtype=torch.int64, device=pred.device)
    bad = torch.zeros((f,), dtype=torch.int64, device=pred.device)
    hip.check(hip.lib().mudg_metric_confusion(pred.data_ptr(), gt.data_ptr(), f, h, w, classes, confusion.data_ptr(), bad.data_ptr(), _stream()),
              "mudg_metric_confusion")
    return confusion, bad


# ------------------------------------------------------------------------------------------------ frames in: resize to clips
RESIZE_MODES = ("linear_u8", "linear_f32", "nearest")
STREAM_KINDS = {"color": 0, "semantic": 1, "depth": 2}           # mudg_dense_stream's kind
COEF_ONE = 2048                                                 # the 8-bit rule's coefficient pairs sum to this
_RESIZE_TABLES = {}
_NORM_TABLES = {}


def resize_table(n_src, n_dst, mode):
    """The sample table of one axis, host numpy (n_dst, 4) int32: s0, s1 and the two coefficients — int32 that sum to 2048
    (linear_u8), fp32 bit patterns 1 - f, f (linear_f32) or zeros (nearest: s1 = s0).  Everything is computed here, in float64 and fp32 as
    the rule states; a kernel computes no coordinate."""
    import numpy as np
    n_src, n_dst = int(n_src), int(n_dst)
    if n_src < 1 or n_dst < 1 or mode not in RESIZE_MODES:
        raise hip.MudgError(f"resize_table: {n_src} -> {n_dst} samples, mode {mode!r} ({' | '.join(RESIZE_MODES)})")
    d = np.arange(n_dst, dtype=np.float64)
    scale = np.float64(n_src) / np.float64(n_dst)
    table = np.zeros((n_dst, 4), dtype=np.int32)
    if mode == "nearest":
        table[:, 0] = table[:, 1] = np.minimum(np.floor(d * scale).astype(np.int64), n_src - 1)
        return table
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = f - s                                                   # fp32, exact
    s = s.astype(np.int64)
    low = s < 0
    s[low], f[low] = 0, 0
    high = s >= n_src - 1
    s[high], f[high] = n_src - 1, 0
    table[:, 0], table[:, 1] = s, np.minimum(s + 1, n_src - 1)
    one = np.float32(1)
    if mode == "linear_u8":
        k = np.float32(COEF_ONE)
        table[:, 2] = np.rint((one - f) * k).astype(np.int16)
        table[:, 3] = np.rint(f * k).astype(np.int16)
    else:
        table[:, 2] = (one - f).astype(np.float32).view(np.int32)
        table[:, 3] = f.view(np.int32)
    return table


def _resize_tables(hw_in, hw_out, mode, device):
    """The (ytab, xtab) pair on the device, uploaded once per (n_src, n_dst, mode)."""
    out = []
    for n_src, n_dst in zip(hw_in, hw_out):
        key = (int(n_src), int(n_dst), mode, device)
        if key not in _RESIZE_TABLES:
            _RESIZE_TABLES[key] = torch.from_numpy(resize_table(n_src, n_dst, mode)).to(device)
        out.append(_RESIZE_TABLES[key])
    return out


def norm_table(device):
    """(v / 255 - 0.5) * 2 for v = 0 .. 255, computed by torch on the host with the loaders' expression (waymo_data.py:117)."""
    if device not in _NORM_TABLES:
        _NORM_TABLES[device] = ((torch.arange(256, dtype=torch.uint8).float() / 255 - 0.5) * 2).to(device)
    return _NORM_TABLES[device]


def _hw_out(name, hw_out):
    h, w = (int(v) for v in hw_out)
    if h < 1 or w < 1:
        raise hip.MudgError(f"{name}: output size {h} x {w}")
    return h, w


def resize_u8(src, hw_out, mode="linear", *, palette=False):
    """(T, H0, W0, C) uint8, C = 1 or 3 -> (T, h, w, C) by the 8-bit linear rule or nearest.  palette: src is (T, H0, W0)
    class ids and the result the resized colour-mapped map (T, h, w, 3), the colours looked up on the taps."""
    _splat_tensor("resize_u8: src", src, torch.uint8)
    if mode not in ("linear", "nearest"):
        raise hip.MudgError(f"resize_u8: mode {mode!r} (linear | nearest)")
    if src.dim() != (3 if palette else 4) or src.numel() == 0 or (not palette and src.shape[3] not in (1, 3)):
        raise hip.MudgError(f"resize_u8: expected {'(frames, H, W) class ids' if palette else '(frames, H, W, 1 or 3) frames'}, got {tuple(src.shape)}")
    if palette and mode != "linear":
        raise hip.MudgError("resize_u8: the label palette goes with the linear rule")
    h, w = _hw_out("resize_u8", hw_out)
    t, h0, w0 = src.shape[:3]
    c = 3 if palette else src.shape[3]
    ytab, xtab = _resize_tables((h0, w0), (h, w), "linear_u8" if mode == "linear" else "nearest", src.device)
    out = torch.empty((t, h, w, c), dtype=torch.uint8, device=src.device)
    hip.check(hip.lib().mudg_resize_u8(src.data_ptr(), out.data_ptr(), t, h0, w0, c, h, w, 0 if mode == "linear" else 1, int(bool(palette)),
                                       xtab.data_ptr(), ytab.data_ptr(), _stream()), "mudg_resize_u8")
    return out


def resize_f32(src, hw_out):
    """(T, H0, W0) fp32 -> (T, h, w) by the fp32 linear rule: every multiply and add rounded on its own, in the rule's order."""
    _splat_tensor("resize_f32: src", src, torch.float32)
    if src.dim() != 3 or src.numel() == 0:
        raise hip.MudgError(f"resize_f32: expected (frames, H, W) maps, got {tuple(src.shape)}")
    h, w = _hw_out("resize_f32", hw_out)
    t, h0, w0 = src.shape
    ytab, xtab = _resize_tables((h0, w0), (h, w), "linear_f32", src.device)
    out = torch.empty((t, h, w), dtype=torch.float32, device=src.device)
    hip.check(hip.lib().mudg_resize_f32(src.data_ptr(), out.data_ptr(), t, h0, w0, h, w, xtab.data_ptr(), ytab.data_ptr(), _stream()), "mudg_resize_f32")
    return out


def _stream_out(name, out, device, t, h, w, slab, frame0):
    """Where a stream of t frames goes: a new (3, t, h, w) tensor, or the caller's `out` checked against stream `slab`, frames frame0 ..."""
    slab, frame0 = int(slab), int(frame0)
    if out is None:
        out = torch.empty((3, t, h, w), dtype=torch.float32, device=device)
    if not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != device or out.dim() not in (4, 5):
        raise hip.MudgError(f"{name}: out is a (3, frames, h, w) or (streams, 3, frames, h, w) fp32 tensor on the source's device")
    slabs = out.shape[0] if out.dim() == 5 else 1
    if (tuple(out.shape[-4:-2]) != (3, out.shape[-3]) or tuple(out.shape[-2:]) != (h, w) or out.stride(-1) != 1 or out.stride(-2) != w
            or not (0 <= slab < slabs and 0 <= frame0 and frame0 + t <= out.shape[-3]) or out.stride(-3) < h * w or out.stride(-4) <= 0):
        raise hip.MudgError(f"{name}: {t} frames of {h} x {w} at stream {slab}, frame {frame0} of out {tuple(out.shape)} strides {out.stride()}")
    return out, slab, frame0


def dense_stream(kind, src, hw_out, out=None, *, slab=0, frame0=0, return_u8=False):
    """One dense stream of a clip.  kind "color": src (T, H0, W0, 3) uint8; "semantic": (T, H0, W0) uint8 class ids;
    "depth": (T, H0, W0) fp32 metres.  Writes (3, T, h, w) fp32 in [-1, 1]: into a new tensor, or into `out` — (3, T', h, w), or
    (S, 3, T', h, w) at stream `slab` — at frames frame0 .. frame0 + T - 1, rows contiguous, any other strides.  return_u8 (not depth):
    also the resized bytes (T, h, w, 3), what resize_u8 gives.  Returns out, or (out, bytes)."""
    if kind not in STREAM_KINDS:
        raise hip.MudgError(f"dense_stream: kind {kind!r} ({' | '.join(STREAM_KINDS)})")
    _splat_tensor(f"dense_stream: the {kind} source", src, torch.float32 if kind == "depth" else torch.uint8)
    if src.dim() != (4 if kind == "color" else 3) or src.numel() == 0 or (kind == "color" and src.shape[3] != 3):
        raise hip.MudgError(f"dense_stream: a {kind} source is {'(frames, H, W, 3)' if kind == 'color' else '(frames, H, W)'}, got {tuple(src.shape)}")
    if return_u8 and kind == "depth":
        raise hip.MudgError("dense_stream: the depth stream has no uint8 frames")
    h, w = _hw_out("dense_stream", hw_out)
    t, h0, w0 = src.shape[:3]
    out, slab, frame0 = _stream_out("dense_stream", out, src.device, t, h, w, slab, frame0)
    ytab, xtab = _resize_tables((h0, w0), (h, w), "linear_f32" if kind == "depth" else "linear_u8", src.device)
    norm = None if kind == "depth" else norm_table(src.device)
    u8 = torch.empty((t, h, w, 3), dtype=torch.uint8, device=src.device) if return_u8 else None
    hip.check(hip.lib().mudg_dense_stream(STREAM_KINDS[kind], src.data_ptr(), t, h0, w0, h, w, xtab.data_ptr(), ytab.data_ptr(), _ptr(norm),
                                          out.data_ptr(), out.stride(0) if out.dim() == 5 else 0, out.stride(-4), out.stride(-3), slab, frame0,
                                          _ptr(u8), _stream()), "mudg_dense_stream")
    return (out, u8) if return_u8 else out


# ------------------------------------------------------------------------------------------------ surface normals
NORMAL_BINS = 720                                               # mudg_metric_normals: quarter degrees of [0, 180]
_COS_TABLES = {}


def depth_normals(depth, table, labels=None, *, sky_label=10, min_depth=0.0, max_depth=100.0, max_rel_step=None):
    """depth (f, h, w) fp32 metres and table (f, 4) float64 (fx, fy, cx, cy at (h, w)) -> camera-space unit normals (f, h, w, 3) fp32 and
    valid (f, h, w) uint8.  A pixel is usable iff min_depth < depth < max_depth and its label is not sky_label; the normal is dy x dx over
    central (or one-sided) differences of the unprojected points of usable neighbours, under max_rel_step = r also |z_nb - z| <= r z.
    What is not valid stores (0, 0, 0) and 0."""
    _splat_tensor("depth_normals: depth", depth, torch.float32)
    if depth.dim() != 3 or depth.numel() == 0:
        raise hip.MudgError(f"depth_normals: expected (frames, h, w) depths, got {tuple(depth.shape)}")
    f, h, w = depth.shape
    _splat_tensor("depth_normals: table", table, torch.float64, (f, 4))
    if labels is not None:
        _splat_tensor("depth_normals: labels", labels, torch.int64, (f, h, w))
    step = -1.0 if max_rel_step is None else float(max_rel_step)
    if max_rel_step is not None and not step >= 0.0:
        raise hip.MudgError(f"depth_normals: max_rel_step {max_rel_step} (None, or a number that is not negative)")
    normals = torch.empty((f, h, w, 3), dtype=torch.float32, device=depth.device)
    valid = torch.empty((f, h, w), dtype=torch.uint8, device=depth.device)
    hip.check(hip.lib().mudg_depth_normals(depth.data_ptr(), _ptr(labels), int(sky_label), table.data_ptr(), f, h, w, float(min_depth),
                                           float(max_depth), step, normals.data_ptr(), valid.data_ptr(), _stream()), "mudg_depth_normals")
    return normals, valid


def normal_stream(src, hw_out, out=None, *, slab=0, frame0=0):
    """(T, H0, W0, 3) fp32 normal maps -> the normal stream (3, T, h, w): the fp32 linear rule on every channel, nothing else (the maps
    are already in [-1, 1]; a NaN stays one).  out / slab / frame0 place it as dense_stream does."""
    _splat_tensor("normal_stream: the source", src, torch.float32)
    if src.dim() != 4 or src.shape[3] != 3 or src.numel() == 0:
        raise hip.MudgError(f"normal_stream: a source is (frames, H, W, 3), got {tuple(src.shape)}")
    h, w = _hw_out("normal_stream", hw_out)
    t, h0, w0 = src.shape[:3]
    out, slab, frame0 = _stream_out("normal_stream", out, src.device, t, h, w, slab, frame0)
    ytab, xtab = _resize_tables((h0, w0), (h, w), "linear_f32", src.device)
    hip.check(hip.lib().mudg_normal_stream(src.data_ptr(), t, h0, w0, h, w, xtab.data_ptr(), ytab.data_ptr(), out.data_ptr(),
                                           out.stride(0) if out.dim() == 5 else 0, out.stride(-4), out.stride(-3), slab, frame0, _stream()),
              "mudg_normal_stream")
    return out


def normal_cos_table():
    """Host, float64: T[k] = cos((k * 0.25) * (pi / 180)), k = 0 .. 720, the bin edges of mudg_metric_normals as cosines: strictly
    descending from 1 to -1."""
    import numpy as np
    table = np.cos((np.arange(NORMAL_BINS + 1, dtype=np.float64) * 0.25) * (np.pi / 180.0))
    if table[0] != 1.0 or table[-1] != -1.0 or not np.all(np.diff(table) < 0):
        raise hip.MudgError("normal_cos_table: the cosines do not descend from 1 to -1")
    return table


def metric_normals(pred, gt, valid=None):
    """pred (f, h, w, 3) uint8, gt (f, h, w, 3) fp32, valid (f, h, w) uint8 or None -> (f, 720) int64: per frame the counts of the angle
    between 2 pred - 255 and gt in quarter-degree bins, over the pixels whose validity byte is nonzero and whose gt has a finite
    positive length."""
    f, h, w = _depth_frames("metric_normals", pred)
    _splat_tensor("metric_normals: gt", gt, torch.float32, (f, h, w, 3))
    if valid is not None:
        _splat_tensor("metric_normals: valid", valid, torch.uint8, (f, h, w))
    if pred.device not in _COS_TABLES:
        _COS_TABLES[pred.device] = torch.from_numpy(normal_cos_table()).to(pred.device)
    hist = torch.zeros((f, NORMAL_BINS), dtype=torch.int64, device=pred.device)
    hip.check(hip.lib().mudg_metric_normals(pred.data_ptr(), gt.data_ptr(), _ptr(valid), _COS_TABLES[pred.device].data_ptr(), f, h, w,
                                            hist.data_ptr(), _stream()), "mudg_metric_normals")
    return hist


# ------------------------------------------------------------------------------------------------ LiDAR depth maps
LIDAR_MAX_SEGMENTS, LIDAR_MAX_REACH = 8, 16


def lidar_splat_visible(points, segments, mats, keys, intr, point_size, *, occluder_keys=None, ids=None, reach=4, rel_tol=0.05, znear=1e-4,
                        zfar=200.0, index_base=0):
    """The candidates — runs [(first point, length > 0)] (at most 8) of a packed cloud (n, 4) int32 — through mats (nmat, 12) fp32 (ids (n,)
    int32 choose among nmat > 1) and intr = (fx, fy, cx, cy) into keys (h, w) int64 by §12's rule, except the hidden ones: against
    occluder_keys (h, w) int64, drawn by splat_points from the same candidates, a point with camera depth zc is hidden iff along one of
    the four lines through its home pixel both sides hold, within `reach` pixels, a depth below fp32(zc * fp32(1 - rel_tol)).
    occluder_keys None: no test."""
    _splat_tensor("lidar_splat_visible: points", points, torch.int32)
    if points.dim() != 2 or points.shape[1] != 4 or points.shape[0] == 0:
        raise hip.MudgError(f"lidar_splat_visible: expected packed points (n > 0, 4), got {tuple(points.shape)}")
    n = points.shape[0]
    segments = [(int(a), int(b)) for a, b in segments]
    if not 1 <= len(segments) <= LIDAR_MAX_SEGMENTS or any(a < 0 or b <= 0 or a + b > n for a, b in segments):
        raise hip.MudgError(f"lidar_splat_visible: segments {segments} of a cloud of {n} points (1 .. {LIDAR_MAX_SEGMENTS} runs inside it)")
    _splat_tensor("lidar_splat_visible: mats", mats, torch.float32)
    _splat_tensor("lidar_splat_visible: keys", keys, torch.int64)
    if mats.dim() != 2 or mats.shape[1] != 12 or keys.dim() != 2:
        raise hip.MudgError(f"lidar_splat_visible: matrices {tuple(mats.shape)} and a key image {tuple(keys.shape)}, expected (nmat, 12) and (h, w)")
    if ids is not None:
        _splat_tensor("lidar_splat_visible: ids", ids, torch.int32, (n,))
    elif mats.shape[0] != 1:
        raise hip.MudgError(f"lidar_splat_visible: {mats.shape[0]} matrices need per-point ids")
    keep = 1.0
    if occluder_keys is not None:
        _splat_tensor("lidar_splat_visible: occluder keys", occluder_keys, torch.int64, keys.shape)
        if not (isinstance(reach, int) and 1 <= reach <= LIDAR_MAX_REACH) or not 0.0 <= float(rel_tol) < 1.0:
            raise hip.MudgError(f"lidar_splat_visible: reach {reach} (an integer, 1 .. {LIDAR_MAX_REACH}) and rel_tol {rel_tol} (0 <= rel_tol < 1)")
        keep = 1.0 - float(rel_tol)
    table = (C.c_int64 * (2 * len(segments)))(*[v for s in segments for v in s])
    fx, fy, cx, cy = (float(v) for v in intr)
    hip.check(hip.lib().mudg_lidar_splat_visible(points.data_ptr(), _ptr(ids), table, len(segments), mats.data_ptr(), mats.shape[0],
                                                 _ptr(occluder_keys), keys.data_ptr(), keys.shape[0], keys.shape[1], fx, fy, cx, cy, float(znear),
                                                 float(zfar), float(point_size), int(reach), keep, int(index_base), _stream()),
              "mudg_lidar_splat_visible")
    return keys


def lidar_depth_resolve(keys, depth, occluder_keys=None):
    """keys (h, w) int64 -> depth (h, w) fp32 (written in place: a frame of a larger tensor): the winner's camera depth, 0 where nothing
    landed; keys, and occluder_keys if given, are empty again afterwards."""
    _splat_tensor("lidar_depth_resolve: keys", keys, torch.int64)
    _splat_tensor("lidar_depth_resolve: depth", depth, torch.float32, keys.shape)
    if occluder_keys is not None:
        _splat_tensor("lidar_depth_resolve: occluder keys", occluder_keys, torch.int64, keys.shape)
    hip.check(hip.lib().mudg_lidar_depth_resolve(keys.data_ptr(), _ptr(occluder_keys), depth.data_ptr(), keys.numel(), _stream()),
              "mudg_lidar_depth_resolve")
    return depth


def depth_complete(depth, labels=None, *, max_depth=100.0, extrapolate=True, sky_label=10, return_source=False):
    """depth (f, h, w) fp32 metres, 0 where there is none -> the dense map (f, h, w) fp32 by the nine steps of DESIGN.md §20 (and the
    uint8 source map: 0 empty, 1 measured, 2 closed, 3 extended, 4 sky).  labels (f, h, w) int64 or None."""
    _splat_tensor("depth_complete: depth", depth, torch.float32)
    if depth.dim() != 3 or depth.numel() == 0:
        raise hip.MudgError(f"depth_complete: expected (frames, h, w) depths, got {tuple(depth.shape)}")
    f, h, w = depth.shape
    if labels is not None:
        _splat_tensor("depth_complete: labels", labels, torch.int64, (f, h, w))
    if not 0.1 < float(max_depth) <= 65536.0:
        raise hip.MudgError(f"depth_complete: max_depth {max_depth} (0.1 < max_depth <= 65536)")
    need = hip.lib().mudg_depth_complete_scratch(f, h, w)
    if need < 0:
        raise hip.MudgError(f"depth_complete: {f} frames of {h} x {w} (1 .. 65535 frames and rows, at most 2^24 pixels each)")
    scratch = torch.empty((need,), dtype=torch.uint8, device=depth.device)
    out = torch.empty_like(depth)
    source = torch.empty((f, h, w), dtype=torch.uint8, device=depth.device) if return_source else None
    hip.check(hip.lib().mudg_depth_complete(depth.data_ptr(), _ptr(labels), int(sky_label), f, h, w, float(max_depth), 1 if extrapolate else 0,
                                            out.data_ptr(), _ptr(source), scratch.data_ptr(), need, _stream()), "mudg_depth_complete")
    return (out, source) if return_source else out


# ------------------------------------------------------------------------------------------------ the CLIP image tower
CLIP_SIZE, CLIP_PATCH, CLIP_K, CLIP_KPAD = 224, 14, 588, 592
_CLIP_TABLES = {}


def clip_blur_taps(n_src, n_dst=CLIP_SIZE):
    """The Gaussian taps of one axis of the antialiasing blur, host numpy fp32 (k,): f = n_src / n_dst, sigma = max((f - 1) / 2, 0.001),
    k = int(max(4 sigma, 3)) made odd, exp(-(i - (k - 1) / 2)^2 / (2 sigma^2)) normalised to sum 1 — in float64, rounded once."""
    import numpy as np
    f = np.float64(n_src) / np.float64(n_dst)
    sigma = max((f - 1.0) / 2.0, 0.001)
    k = int(max(4.0 * sigma, 3.0))
    k += 1 - k % 2
    i = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def clip_cubic_table(n_src, n_dst=CLIP_SIZE):
    """The bicubic sample table of one axis, host numpy (n_dst, 8) int32: four source indices floor(src) - 1 .. + 2 clamped to the image and
    the fp32 bits of the four coefficients (A = -0.75), src = dst (n_src - 1) / (n_dst - 1) (align_corners) — in float64, rounded once."""
    import numpy as np
    n_src, n_dst = int(n_src), int(n_dst)
    A = -0.75
    d = np.arange(n_dst, dtype=np.float64)
    src = d * (np.float64(n_src - 1) / np.float64(n_dst - 1)) if n_dst > 1 else np.zeros(1)
    i0 = np.floor(src)
    t = src - i0
    near = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    far = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    coef = np.stack([far(t + 1.0), near(t), near(1.0 - t), far(2.0 - t)], 1).astype(np.float32)
    idx = np.clip(i0.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_src - 1)
    table = np.empty((n_dst, 8), dtype=np.int32)
    table[:, :4], table[:, 4:] = idx, coef.view(np.int32)
    return table


def _clip_tables(h, w, antialias, device):
    """(ytab, xtab, gy, gx) on the device, uploaded once per (H, W, antialias, device); gy = gx = None without the blur."""
    key = (int(h), int(w), bool(antialias), device)
    if key not in _CLIP_TABLES:
        blur = antialias and max(h, w) > CLIP_SIZE               # max(f_h, f_w) > 1
        up = lambda a: torch.from_numpy(a).to(device)
        _CLIP_TABLES[key] = (up(clip_cubic_table(h)), up(clip_cubic_table(w)), up(clip_blur_taps(h)) if blur else None,
                             up(clip_blur_taps(w)) if blur else None)
    return _CLIP_TABLES[key]


def clip_preprocess(x, *, antialias=True, patches=None, image=None, return_image=False):
    """(B, 3, H, W) fp32 in [-1, 1] -> the patch matrix of the 224 x 224 CLIP input, operand rows [B 256][592] (mudg_clip_preprocess).
    patches / image: destinations inside larger buffers (a rows view; a contiguous (B, 3, 224, 224) fp32 view); return_image: also
    return the fp32 image (tests and inspection)."""
    _splat_tensor("clip_preprocess: images", x, torch.float32)
    if x.dim() != 4 or x.shape[1] != 3 or x.numel() == 0:
        raise hip.MudgError(f"clip_preprocess: expected (B, 3, H, W) images, got {tuple(x.shape)}")
    b, _, h, w = x.shape
    if patches is None:
        patches = empty_rows(b * 256, CLIP_KPAD, None, x.device)
    _rows(patches)
    if tuple(patches.shape) != (b * 256, CLIP_KPAD):
        raise hip.MudgError(f"clip_preprocess: patches are operand rows [{b * 256}][{CLIP_KPAD}], got {tuple(patches.shape)}")
    if image is None and return_image:
        image = torch.empty((b, 3, CLIP_SIZE, CLIP_SIZE), dtype=torch.float32, device=x.device)
    if image is not None:
        _splat_tensor("clip_preprocess: image", image, torch.float32, (b, 3, CLIP_SIZE, CLIP_SIZE))
    ytab, xtab, gy, gx = _clip_tables(h, w, antialias, x.device)
    hip.check(hip.lib().mudg_clip_preprocess(x.data_ptr(), b, h, w, ytab.data_ptr(), xtab.data_ptr(), _ptr(gy), 0 if gy is None else gy.numel(),
                                             _ptr(gx), 0 if gx is None else gx.numel(), patches.data_ptr(), patches.stride(0), _ptr(image),
                                             _stream()), "mudg_clip_preprocess")
    return (patches, image) if return_image else patches


def short_attention_desc(qkv_ptr, o_ptr, *, batch, heads, n, d, ldqkv, ldo, scale=None):
    desc = hip.ShortAttnDesc()
    desc.QKV, desc.O, desc.B, desc.heads, desc.N, desc.d = qkv_ptr, o_ptr, batch, heads, n, d
    desc.ldqkv, desc.ldo, desc.scale = ldqkv, ldo, float(d) ** -0.5 if scale is None else scale
    return desc


def short_attention(qkv, out=None, *, batch, heads, n, d, scale=None):
    """Self-attention over n <= 288 tokens from the fp32 rows [batch n][>= 3 heads d] of a fused q | k | v projection
    (mudg_short_attention): operand rows [batch n][heads d].  Head width 64 or 80; anything else raises."""
    _rows(qkv, torch.float32)
    if qkv.shape[0] != batch * n:
        raise hip.MudgError(f"short_attention: qkv has {qkv.shape[0]} rows, batch {batch} x {n} tokens")
    if out is None:
        out = empty_rows(batch * n, heads * d, None, qkv.device)
    _rows(out)
    _drop_stats(out)
    if qkv.shape[1] < 3 * heads * d or out.shape[0] != batch * n or out.shape[1] < heads * d:
        raise hip.MudgError(f"short_attention: qkv {tuple(qkv.shape)} / out {tuple(out.shape)} for {heads} heads of {d}")
    desc = short_attention_desc(qkv.data_ptr(), out.data_ptr(), batch=batch, heads=heads, n=n, d=d, ldqkv=qkv.stride(0), ldo=out.stride(0),
                                scale=scale)
    hip.check(hip.lib().mudg_short_attention(C.byref(desc), _stream()), "mudg_short_attention")
    return out


def layernorm_f32(x, gamma, beta, *, eps=1e-5, out=None):
    """LayerNorm of fp32 rows with an fp32 result (mudg_layernorm_f32)."""
    _rows(x, torch.float32)
    if out is None:
        out = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    _rows(out, torch.float32)
    hip.check(hip.lib().mudg_layernorm_f32(x.data_ptr(), x.stride(0), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), out.stride(0),
                                           x.shape[0], x.shape[1], eps, _stream()), "mudg_layernorm_f32")
    return out
