"""CPU definitions of mudg_gemm (include/mudg_hip.h, "GEMM / conv"): plain torch in fp64, written from the header's text and from
nothing else — no kernel, no mudg_amd import.  tests/test_gemm_reference_cpu.py checks every definition against the textbook torch
op (F.linear, F.conv2d, F.conv3d, F.gelu) and tests/test_gemm_kernels_gpu.py holds the HIP kernels to them.

Operands are LOGICAL tensors: x [batch | 1][rows][Cin] (the two channel sources already side by side: `sources` cuts and joins them),
w [batch | 1][N][K]; a leading dimension of 1 is a batch stride of 0.  `strided` reads such a tensor out of a flat buffer with the
descriptor's base offset, row stride and batch stride, which is how the V^T form with a padded ldy is stated."""
import math

import torch

F64 = torch.float64
KIND_OPERAND, KIND_F32, KIND_F16 = 0, 1, 2
# csrc/common.h: the (X piece, W piece) products a split build adds up
KEPT = {1: ((0, 0),), 2: ((1, 0), (0, 1), (0, 0)), 3: ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))}


# ------------------------------------------------------------------------------------------------ layouts
def strided(flat, off, ld, rows, cols, batch=1, sb=0):
    """[batch][rows][cols] view of a flat buffer: element (z, r, c) at off + z sb + r ld + c."""
    return torch.as_strided(flat, (batch, rows, cols), (sb, ld, 1), off)


def sources(x, x2=None, csplit=None):
    """The channel axis the kernels see: channels [0, csplit) from x, the rest from x2."""
    if x2 is None:
        return x
    assert x.shape[-1] == csplit
    return torch.cat([x, x2], -1)


def slab_major(w_tap_major, taps, cin):
    """[N][tap][Cin] -> [N][Cin / 64][tap][64] (korder 1), both flattened to [N][taps Cin]."""
    n = w_tap_major.shape[0]
    return w_tap_major.reshape(n, taps, cin // 64, 64).permute(0, 2, 1, 3).reshape(n, taps * cin)


def _k_axis(cols, cin, korder):
    """cols [..][taps][Cin] -> the K axis [..][taps Cin] in the stated order."""
    taps = cols.shape[-2]
    lead = cols.shape[:-2]
    if korder:
        assert cin % 64 == 0
        cols = cols.reshape(*lead, taps, cin // 64, 64).transpose(-3, -2)
    return cols.reshape(*lead, taps * cin)


def _gather_rows(x, idx):
    """x [B][rows][C], idx [M] (-1 = zero) -> [B][M][C]."""
    out = x[:, idx.clamp_min(0)]
    return out * (idx >= 0).to(x.dtype)[None, :, None]


# ------------------------------------------------------------------------------------------------ epilogue pieces
def gelu_erf(g):
    """g Phi(g) with Phi = 0.5 erfc(-g / sqrt 2) (the cancellation-free form of 0.5 (1 + erf))."""
    return g * 0.5 * torch.erfc(-g / math.sqrt(2.0))


def geglu_unpack(n_out):
    """(value rows, gate rows) of the [32 value | 32 gate] packing for n_out = N / 2 outputs."""
    j = torch.arange(n_out)
    v = (j // 32) * 64 + j % 32
    return v, v + 32


def epilogue(s, *, alpha=1.0, bias=None, gbias=None, rows_per_group=0, act=False, geglu=False, r=None):
    """s [B][M][N] = the raw contraction.  alpha * s, + bias, + gbias[m // rows_per_group], act, GEGLU, + R last."""
    y = (1.0 if alpha == 0 else alpha) * s
    if bias is not None:
        y = y + bias.to(F64)
    if gbias is not None:
        m = torch.arange(y.shape[1])
        y = y + gbias.to(F64)[m // rows_per_group]
    if act:
        y = gelu_erf(y)
    if geglu:
        v, g = geglu_unpack(y.shape[-1] // 2)
        y = y[..., v] * gelu_erf(y[..., g])
    if r is not None:
        y = y + r.to(F64)
    return y


# ------------------------------------------------------------------------------------------------ the three contractions
def contract_gemm(x, w):
    """mode 0: x [Bx][M][K], w [Bw][N][K] -> [B][M][N]."""
    return torch.matmul(x.to(F64), w.to(F64).transpose(-1, -2))


def gemm(x, w, *, x2=None, csplit=None, **epi):
    return epilogue(contract_gemm(sources(x, x2, csplit), w), **epi)


def conv_out_size(hin, win, stride=1, pad=1, upsample=0):
    if upsample:
        return 2 * hin, 2 * win
    if pad == 1:
        return (hin - 1) // stride + 1, (win - 1) // stride + 1
    return (hin + 1 - 3) // stride + 1, (win + 1 - 3) // stride + 1          # pad (0, 1, 0, 1): bottom / right only


def conv_source_rows(frames, hin, win, hout, wout, stride, pad, upsample, dy, dx):
    """Input row of tap (dy, dx) for every output row, -1 outside the (possibly upsampled) image."""
    m = torch.arange(frames * hout * wout)
    f, rr = m // (hout * wout), m % (hout * wout)
    oy, ox = rr // wout, rr % wout
    uy, ux = oy * stride - pad + dy, ox * stride - pad + dx
    up = 2 if upsample else 1
    ok = (uy >= 0) & (uy < hin * up) & (ux >= 0) & (ux < win * up)
    src = (f * hin + uy // up) * win + ux // up
    return torch.where(ok, src, torch.full_like(src, -1))


def contract_conv3x3(x, w, *, frames, hin, win, cin, stride=1, pad=1, upsample=0, korder=0):
    """mode 1: x [1][frames hin win][Cin], w [1][N][9 Cin] -> [1][frames hout wout][N]; tap = 3 dy + dx."""
    hout, wout = conv_out_size(hin, win, stride, pad, upsample)
    x = x.to(F64)
    cols = torch.stack([_gather_rows(x, conv_source_rows(frames, hin, win, hout, wout, stride, pad, upsample, t // 3, t % 3))
                        for t in range(9)], -2)                                   # [1][M][9][Cin]
    return torch.matmul(_k_axis(cols, cin, korder), w.to(F64).transpose(-1, -2))


def conv3x3(x, w, *, x2=None, csplit=None, frames, hin, win, cin, stride=1, pad=1, upsample=0, korder=0, **epi):
    return epilogue(contract_conv3x3(sources(x, x2, csplit), w, frames=frames, hin=hin, win=win, cin=cin, stride=stride, pad=pad,
                                     upsample=upsample, korder=korder), **epi)


def subpixel_out_rows(frames, hin, win, z):
    """Rows of the (2 hin x 2 win) output image that batch entry z = 2 py + px writes, in the order of its low-resolution rows."""
    py, px = z // 2, z % 2
    m = torch.arange(frames * hin * win)
    f, rr = m // (hin * win), m % (hin * win)
    oy, ox = rr // win, rr % win
    return ((f * 2 * hin) + 2 * oy + py) * (2 * win) + 2 * ox + px


def contract_subpixel(x, w4, *, frames, hin, win, cin):
    """mode 1, subpixel: x [1][frames hin win][Cin], w4 [4][N][4 Cin] (K = [Cin / 64][tap 2a + b][64]) -> [1][frames 2hin 2win][N]."""
    x = x.to(F64)
    out = torch.zeros((1, frames * 4 * hin * win, w4.shape[1]), dtype=F64)
    m = torch.arange(frames * hin * win)
    f, rr = m // (hin * win), m % (hin * win)
    oy, ox = rr // win, rr % win
    for z in range(4):
        py, px = z // 2, z % 2
        taps = []
        for a in range(2):
            for b in range(2):
                iy, ix = oy - 1 + py + a, ox - 1 + px + b
                ok = (iy >= 0) & (iy < hin) & (ix >= 0) & (ix < win)
                src = (f * hin + iy) * win + ix
                taps.append(_gather_rows(x, torch.where(ok, src, torch.full_like(src, -1))))
        cols = _k_axis(torch.stack(taps, -2), cin, 1)
        out[:, subpixel_out_rows(frames, hin, win, z)] = torch.matmul(cols, w4[z].to(F64).t())
    return out


def conv3x3_subpixel(x, w4, *, frames, hin, win, cin, **epi):
    return epilogue(contract_subpixel(x, w4, frames=frames, hin=hin, win=win, cin=cin), **epi)


def tconv_source_rows(clips, t, hw, dt):
    m = torch.arange(clips * t * hw)
    tt = (m // hw) % t + dt - 1
    return torch.where((tt >= 0) & (tt < t), m + (dt - 1) * hw, torch.full_like(m, -1))


def contract_tconv3(x, w, *, clips, t, hw, cin, korder=0):
    """mode 2: rows ((b T + t) HW + s); tap dt reads frame t + dt - 1 of the same clip, zero outside it."""
    x = x.to(F64)
    cols = torch.stack([_gather_rows(x, tconv_source_rows(clips, t, hw, dt)) for dt in range(3)], -2)
    return torch.matmul(_k_axis(cols, cin, korder), w.to(F64).transpose(-1, -2))


def tconv3(x, w, *, x2=None, csplit=None, clips, t, hw, cin, korder=0, **epi):
    return epilogue(contract_tconv3(sources(x, x2, csplit), w, clips=clips, t=t, hw=hw, cin=cin, korder=korder), **epi)


# ------------------------------------------------------------------------------------------------ what is stored
def store_pieces(value, kind, op_dtype=torch.bfloat16, planes=1):
    """The numbers a result is stored as: ONE round-to-nearest-even rounding of fp64 values to fp32, to fp16 (saturating at +-65504), or
    to an operand matrix — `planes` pieces of op_dtype (backward_reference.operand_planes)."""
    v32 = value.to(torch.float32)
    if kind == KIND_F32:
        return [v32]
    if kind == KIND_F16:
        return [v32.clamp(-65504.0, 65504.0).to(torch.float16)]
    from backward_reference import operand_planes
    return operand_planes(v32, op_dtype, planes)


def store(value, kind, op_dtype=torch.bfloat16, planes=1):
    """The stored value (the sum of its pieces), as fp64."""
    return sum(p.to(F64) for p in store_pieces(value, kind, op_dtype, planes))


def stats(y_stored, rows):
    """[ceil(M / rows)][N][2]: the sum and the sum of squares of the stored values of every block of `rows` rows, per channel."""
    m, n = y_stored.shape
    blocks = (m + rows - 1) // rows
    pad = torch.zeros((blocks * rows, n), dtype=F64)
    pad[:m] = y_stored.to(F64)
    pad = pad.reshape(blocks, rows, n)
    return torch.stack([pad.sum(1), (pad * pad).sum(1)], -1)


def split_kept(contract, xpieces, wpieces, planes):
    """The contraction a split build evaluates: the sum over the piece pairs it keeps of contract(X_p, W_q)."""
    return sum(contract(xpieces[p], wpieces[q]) for p, q in KEPT[planes])


def mxfp8(y):
    """OCP MX copy of y [M][N] (N % 32 == 0): (e4m3 bytes [M][N], E8M0 bytes [M][N / 32]); one scale 2^(floor(log2 amax) - 8)
    per 32 columns (2^0 for an all-zero block), values saturating at +-448."""
    m, n = y.shape
    blocks = y.to(F64).reshape(m, n // 32, 32)
    amax = blocks.abs().amax(-1)
    floor_log2 = (torch.frexp(amax)[1] - 1).to(F64)                              # amax = m 2^e, m in [0.5, 1)
    e = torch.where(amax > 0, floor_log2 - 8, torch.zeros_like(amax)).clamp(-127, 127)
    q = (blocks / torch.pow(2.0, e)[..., None]).clamp(-448, 448).to(torch.float32).to(torch.float8_e4m3fn)
    return q.reshape(m, n).view(torch.uint8), (e + 127).to(torch.uint8)


# ------------------------------------------------------------------------------------------------ exactness
def exact_bits(operand_max, weight_max, k_terms, unit, extra=0.0):
    """The condition of the exact tests.  Every product is a multiple of `unit` (a power of two) and so is every partial sum in any
    order; all of them are bounded by k_terms * operand_max * weight_max + extra.  Returns that bound / unit, which must stay
    below 2^24 for fp32 to hold every intermediate exactly."""
    assert unit > 0 and math.log2(unit) == int(math.log2(unit))
    return (k_terms * operand_max * weight_max + extra) / unit
