"""CPU definitions of the training step's backward kernels (include/mudg_hip.h, "training step"), one plain torch function per
C-ABI entry, in the layouts the header documents.  Nothing here comes from mudg_amd: tests/test_backward_reference_cpu.py checks
every definition against torch.autograd of the textbook forward in fp64, and tests/test_backward_kernels_gpu.py holds the HIP
kernels to them.  Everything is evaluated in `dtype` — fp64 for the yardstick; the GPU tests also evaluate the same formulas in
fp32 to learn how much error the arithmetic itself (cancellation, summation) makes at that precision."""
import math

import numpy as np
import torch

F64 = torch.float64


def ceil8(n):
    return (n + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------ gathers, weight gradients
def source_rows(P, mode, geo=None, dy=0, dx=0, dt=0):
    """srcrow(p) of mudg_transpose_gather / mudg_wgrad for p < P, -1 where the tap reads outside the image / the clip.
    mode 0: p.  mode 1: p = (f, oy, ox) on the Hout x Wout grid reads pixel (oy stride - pad + dy, ox stride - pad + dx) of the
    Hin x Win image.  mode 2: p = ((b T + t) HW + s) reads row p + (dt - 1) HW while 0 <= t + dt - 1 < T."""
    p = torch.arange(P, dtype=torch.int64)
    if mode == 0:
        return p
    g = geo
    if mode == 1:
        hw = g["Hout"] * g["Wout"]
        f, r = p // hw, p % hw
        oy, ox = r // g["Wout"], r % g["Wout"]
        iy, ix = oy * g["stride"] - g["pad"] + dy, ox * g["stride"] - g["pad"] + dx
        ok = (iy >= 0) & (iy < g["Hin"]) & (ix >= 0) & (ix < g["Win"])
        return torch.where(ok, (f * g["Hin"] + iy) * g["Win"] + ix, torch.full_like(p, -1))
    t = (p // g["HW"]) % g["T"] + dt - 1
    ok = (t >= 0) & (t < g["T"])
    return torch.where(ok, p + (dt - 1) * g["HW"], torch.full_like(p, -1))


def gather(src, rows):
    """src[rows] with zero rows where rows == -1."""
    out = torch.zeros((rows.numel(), src.shape[1]), dtype=src.dtype)
    ok = rows >= 0
    out[ok] = src[rows[ok]]
    return out


def tap_offsets(mode, tap):
    return dict(dy=tap // 3, dx=tap % 3) if mode == 1 else (dict(dt=tap) if mode == 2 else {})


def wgrad(a, b, P, M, C, taps=1, mode=0, geo=None, p_range=None, dtype=F64):
    """out[m][tap C + c] = sum_p a[p][m] b[src(p, tap)][c] over the positions p (of p_range = (first, end), one slice of the
    contraction, when given): a [>= P][>= M], b [*][>= C]; tap = 3 dy + dx (mode 1) or dt (mode 2)."""
    p0, p1 = p_range or (0, P)
    at = a[p0:p1, :M].to(dtype).t().contiguous()
    bb = b[:, :C].to(dtype)
    return torch.cat([at @ gather(bb, source_rows(P, mode, geo, **tap_offsets(mode, tap))[p0:p1]) for tap in range(taps)], 1)


def transpose_gather(src, P, mode=0, geo=None, dy=0, dx=0, dt=0, dtype=F64):
    """dst[c][p] = src[srcrow(p)][c], [C][ceil8(P)], columns P .. ceil8(P) zero (the values before the operand rounding)."""
    out = torch.zeros((src.shape[1], ceil8(P)), dtype=dtype)
    out[:, :P] = gather(src.to(dtype), source_rows(P, mode, geo, dy, dx, dt)).t()
    return out


def transpose_cast_sum(src, dtype=F64):
    """(dst [C][ceil8(P)] = src^T zero-padded, rows [P][C] = src, part [ceil(P / 64)][C] = the column sums of every 64-row tile)."""
    P, C = src.shape
    s = src.to(dtype)
    tiles = (P + 63) // 64
    padded = torch.zeros((tiles * 64, C), dtype=dtype)
    padded[:P] = s
    return transpose_gather(src, P, dtype=dtype), s.clone(), padded.reshape(tiles, 64, C).sum(1)


def operand_planes(x, op_dtype, planes):
    """The 16-bit pieces an fp32 value is stored as in an operand matrix: piece 0 = the value rounded to op_dtype, piece i = what
    the pieces before it left, rounded (csrc/common.h; one piece in the 16-bit builds, 2 / 3 in bf16x3 / bf16x6)."""
    w = x.to(torch.float32).clone()
    out = []
    for _ in range(planes):
        o = w.to(op_dtype)
        w = w - o.to(torch.float32)
        out.append(o)
    return out


def group_colsum(a, b=None, rows_per_group=None, dtype=F64):
    """out[g][c] = sum over the rows_per_group rows of group g of a[r][c] (* b[r][c])."""
    rows, cols = a.shape
    rpg = rows if rows_per_group is None else rows_per_group
    v = a.to(dtype) if b is None else a.to(dtype) * b.to(dtype)
    return v.reshape(rows // rpg, rpg, cols).sum(1)


# ------------------------------------------------------------------------------------------------ attention
def attention_bwd(q, k, v, do, *, frames, heads, nq, nk, kv_div, scale, round_to=None, dtype=F64):
    """(dQ, dK, dV) of O = softmax(scale Q K^T) V per (frame, head), head width 64: q, do [frames nq][heads 64]; k, v
    [(frames / kv_div) nk][heads 64], kv_div consecutive frames sharing one key / value batch.
        P = softmax(S), dP = dO V^T, D = rowsum(P dP), dS = scale P (dP - D), dV = P^T dO, dQ = dS K, dK = dS^T Q.
    round_to (a 16-bit dtype, or (dtype, pieces) for the operand storage of a split-operand build): P and dS — and nothing else —
    pass through that type before the three products that consume them: the one deliberate loss of mudg_attention_bwd, whose MFMAs take P and dS as operands."""
    q, k, v, do = (t.to(dtype) for t in (q, k, v, do))
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    if isinstance(round_to, tuple):          # (dtype, pieces): the operand storage of a split-operand build
        rt = lambda t: sum(p.to(dtype) for p in operand_planes(t, *round_to))
    else:
        rt = (lambda t: t.to(round_to).to(dtype)) if round_to is not None else (lambda t: t)
    nqg = kv_div * nq
    for g in range(frames // kv_div):
        qs, ks = slice(g * nqg, (g + 1) * nqg), slice(g * nk, (g + 1) * nk)
        for h in range(heads):
            hs = slice(64 * h, 64 * h + 64)
            qh, kh, vh, doh = q[qs, hs], k[ks, hs], v[ks, hs], do[qs, hs]
            p = torch.softmax(scale * (qh @ kh.t()), dim=1)
            dp = doh @ vh.t()
            ds = scale * p * (dp - (p * dp).sum(1, keepdim=True))
            p, ds = rt(p), rt(ds)
            dv[ks, hs] = p.t() @ doh
            dq[qs, hs] = ds @ kh
            dk[ks, hs] = ds.t() @ qh
    return dq, dk, dv


def attention_bwd_two_sets(q, k, v, k2, v2, do, *, frames, heads, nq, nk, kv_div, nk2, kv_div2, scale, dtype=F64):
    """O = softmax(scale Q K^T) V + softmax(scale Q K2^T) V2, each set with its own softmax: (dQ, dK, dV, dK2, dV2)."""
    dq, dk, dv = attention_bwd(q, k, v, do, frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div, scale=scale, dtype=dtype)
    dq2, dk2, dv2 = attention_bwd(q, k2, v2, do, frames=frames, heads=heads, nq=nq, nk=nk2, kv_div=kv_div2, scale=scale, dtype=dtype)
    return dq + dq2, dk, dv, dk2, dv2


def temporal_attention_bwd(qkv, do, *, clips, t, hw, heads, scale, dtype=F64):
    """d[q | k | v] of self-attention over the t frames of every pixel: rows ((b t) hw), head h at columns [64 h, 64 h + 64)."""
    c = heads * 64
    x = qkv.to(dtype).reshape(clips, t, hw, 3, heads, 64).permute(3, 0, 2, 4, 1, 5)          # [3][b][s][h][t][64]
    q, k, v = x[0], x[1], x[2]
    g = do.to(dtype).reshape(clips, t, hw, heads, 64).permute(0, 2, 3, 1, 4)
    p = torch.softmax(scale * (q @ k.transpose(-1, -2)), dim=-1)
    dp = g @ v.transpose(-1, -2)
    ds = scale * p * (dp - (p * dp).sum(-1, keepdim=True))
    d = torch.stack([ds @ k, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ g])                # [3][b][s][h][t][64]
    return d.permute(1, 4, 2, 0, 3, 5).reshape(clips * t * hw, 3 * c)


# ------------------------------------------------------------------------------------------------ norms, softmax
def _silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def groupnorm_stats(x, samples, rows, groups, eps, dtype=F64):
    """[samples groups][2] = (mean, 1 / sqrt(biased variance + eps)) of every (sample, group) of rows [samples rows][C]."""
    c = x.shape[1]
    v = x[:, :c].to(dtype).reshape(samples, rows, groups, c // groups).permute(0, 2, 1, 3).reshape(samples * groups, -1)
    mean = v.mean(1)
    var = ((v - mean[:, None]) ** 2).mean(1)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], 1)


def groupnorm_bwd(x, dy, gamma, beta, stat, samples, rows, groups, silu, dres=None, dtype=F64):
    """y = act(xhat gamma + beta), xhat = (x - mean) rstd with (mean, rstd) = stat: (dX, AB [samples][C][2] = (sum_rows dz,
    sum_rows dz xhat)), dz = dy act'(z);  dX = rstd (dz gamma - m1 - xhat m2) (+ dres), m1 / m2 the group means of gamma dz and
    gamma dz xhat.  dbeta / dgamma are the sums of AB[..., 0] / AB[..., 1] over the samples."""
    c = x.shape[1]
    cpg = c // groups
    x, dy, gamma, beta, stat = (t.to(dtype) for t in (x, dy, gamma, beta, stat))
    st = stat.reshape(samples, 1, groups, 2).repeat_interleave(cpg, dim=2)                        # [s][1][C][2]
    mean, rstd = st[..., 0], st[..., 1]
    xh = (x.reshape(samples, rows, c) - mean) * rstd
    dz = dy.reshape(samples, rows, c)
    if silu:
        dz = dz * _silu_grad(xh * gamma + beta)
    ab = torch.stack([dz.sum(1), (dz * xh).sum(1)], -1)                                          # [s][C][2]
    gm = (ab * gamma[None, :, None]).reshape(samples, groups, cpg, 2).sum(2) / (rows * cpg)      # [s][groups][2]
    gm = gm.repeat_interleave(cpg, dim=1)[:, None]                                               # [s][1][C][2]
    dx = (rstd * (dz * gamma - gm[..., 0] - xh * gm[..., 1])).reshape(samples * rows, c)
    if dres is not None:
        dx = dx + dres.to(dtype)
    return dx, ab


def layernorm_bwd(x, dy, gamma, eps, dres=None, dtype=F64):
    """(dX, part [ceil(rows / 64)][2][C]): per chunk of 64 rows the sums of dy xhat (row 0) and dy (row 1)."""
    rows, c = x.shape
    x, dy, gamma = (t.to(dtype) for t in (x, dy, gamma))
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    dh = dy * gamma
    dx = rstd * (dh - dh.mean(1, keepdim=True) - xh * (dh * xh).mean(1, keepdim=True))
    if dres is not None:
        dx = dx + dres.to(dtype)
    chunks = (rows + 63) // 64
    pad = torch.zeros((chunks * 64, 2, c), dtype=dtype)
    pad[:rows, 0], pad[:rows, 1] = dy * xh, dy
    return dx, pad.reshape(chunks, 64, 2, c).sum(1)


def softmax(s, dtype=F64):
    return torch.softmax(s.to(dtype), dim=1)


def softmax_bwd(p, dp, scale, dtype=F64):
    """dS = scale P (dP - sum_j dP_j P_j)."""
    p, dp = p.to(dtype), dp.to(dtype)
    return scale * p * (dp - (p * dp).sum(1, keepdim=True))


# ------------------------------------------------------------------------------------------------ elementwise, resampling
def _gelu(g):
    return g * 0.5 * (1 + torch.erf(g / math.sqrt(2.0)))


def _gelu_grad(g):
    return 0.5 * (1 + torch.erf(g / math.sqrt(2.0))) + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


def geglu(h, dy=None, dtype=F64):
    """h = [value | gate] [M][2 N]: value gelu(gate) [M][N], or with dy its gradient dH [M][2 N]."""
    n = h.shape[1] // 2
    val, gate = h[:, :n].to(dtype), h[:, n:].to(dtype)
    if dy is None:
        return val * _gelu(gate)
    dy = dy.to(dtype)
    return torch.cat([dy * _gelu(gate), dy * val * _gelu_grad(gate)], 1)


def keep_mask(seed, count, p):
    """keep(seed, i), i < count, of mudg_dropout / mudg_dropout_rows / mudg_geglu_dropout: 24 bits of the splitmix64 finaliser of
    seed + i * 0x9E3779B97F4A7C15 against the drop probability (element index i = m C + c on rows)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(count, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return torch.from_numpy(u >= np.float32(p))


def dropout_rows(x, keep, p, dtype=F64):
    return x.to(dtype) * keep.to(dtype) / (1.0 - p)


def geglu_dropout(h, keep, p, dy=None, dtype=F64):
    """GEGLU then inverted dropout with the given keep mask [M][N]; with dy the gradient dH of both."""
    if dy is None:
        return dropout_rows(geglu(h, dtype=dtype), keep, p, dtype)
    return geglu(h, dropout_rows(dy, keep, p, dtype), dtype=dtype)


def dilate2x(dy, frames, ho, wo, hi, wi):
    """Zero insertion: (frames, ho, wo, C) rows laid onto the (frames, hi, wi, C) grid at (2 oy, 2 ox)."""
    c = dy.shape[1]
    out = torch.zeros((frames, hi, wi, c), dtype=dy.dtype)
    hh, ww = min(ho, (hi + 1) // 2), min(wo, (wi + 1) // 2)
    out[:, 0:2 * hh:2, 0:2 * ww:2] = dy.reshape(frames, ho, wo, c)[:, :hh, :ww]
    return out.reshape(frames * hi * wi, c)


def upsample2x(x, frames, h, w, adjoint=False, dtype=F64):
    """Nearest-2x of rows (frames, h, w, C) -> (frames, 2h, 2w, C); adjoint: the sum over every 2 x 2 block, (frames, 2h, 2w, C) ->
    (frames, h, w, C)."""
    c = x.shape[1]
    x = x.to(dtype)
    if adjoint:
        return x.reshape(frames, h, 2, w, 2, c).sum((2, 4)).reshape(frames * h * w, c)
    return x.reshape(frames, h, 1, w, 1, c).expand(frames, h, 2, w, 2, c).reshape(frames * 4 * h * w, c)


# ------------------------------------------------------------------------------------------------ reductions
def mse(pred, target, weights=None, dtype=F64):
    """(loss[b] = mean over the sample of (pred - target)^2, gradient of sum_b w[b] loss[b] or None)."""
    b = pred.shape[0]
    d = (pred.to(dtype) - target.to(dtype)).reshape(b, -1)
    loss = (d * d).mean(1)
    grad = None if weights is None else (weights.to(dtype)[:, None] * 2.0 * d / d.shape[1]).reshape(pred.shape)
    return loss, grad


def clip_grad_norm(tensors, max_norm, dtype=F64):
    """torch.nn.utils.clip_grad_norm_: (global 2-norm, coefficient min(1, max_norm / (norm + 1e-6)), the scaled tensors)."""
    ts = [t.to(dtype) for t in tensors]
    norm = torch.sqrt(sum((t * t).sum() for t in ts))
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return norm, coef, [t * coef for t in ts]
