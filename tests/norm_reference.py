"""CPU definitions of the entry points of csrc/norm.hip and csrc/misc.hip (include/mudg_hip.h): plain torch in fp64, no kernel code and
no mudg_amd import.  tests/test_norm_reference_cpu.py checks every definition against the textbook torch op and the formulas of lvdm/,
tests/test_norm_kernels_gpu.py holds the HIP kernels to them.

Three parts:
  definitions   groupnorm, groupnorm_from_partials, layernorm, softmax, timestep_embedding, small_linear, the two layout conversions, cast,
                gaussian_sample, lincomb, axpy, ddim_step.  What is stored comes from gemm_reference.store / store_pieces, two channel
                sources from gemm_reference.sources.
  host rules    gn_chunks, gn_stats_sweep, gn_apply (slab CS and the apply kernel), ln_kernel, rows_vec: which code a shape runs, restated
                from the text of the launchers the way shipped_path restates the attention dispatcher.
  emulations    the kernels' documented formulas in fp32 (the library is built without contraction, so CPU fp32 follows them op for
                op): one-pass statistics from per-chunk fp32 partials folded in fp64, y = fmaf(x, rstd g, b - mean rstd g), LayerNorm's
                two passes with rsqrt, the three-pass softmax.  The bounded tests take their bounds from these."""
import math

import torch

import gemm_reference as R

F64, F32 = torch.float64, torch.float32
KIND_OPERAND, KIND_F32, KIND_F16 = R.KIND_OPERAND, R.KIND_F32, R.KIND_F16
GN_UNROLL = 4


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ================================================================================================ definitions
def _silu(y):
    return y * torch.sigmoid(y)


def groupnorm(x, gamma, beta, samples, rows, groups, eps, silu, stats=None):
    """x [samples rows][C] -> (y, mean [samples][groups], rstd): biased variance over the rows x C / groups values of a (sample, group).
    `stats` = (mean, rstd) applies given statistics instead."""
    c = x.shape[1]
    cpg = c // groups
    xg = x.to(F64).reshape(samples, rows, groups, cpg)
    if stats is None:
        mean = xg.mean((1, 3))
        var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
        rstd = 1.0 / torch.sqrt(var + eps)
    else:
        mean, rstd = (t.to(F64).reshape(samples, groups) for t in stats)
    y = (xg - mean[:, None, :, None]) * rstd[:, None, :, None] * gamma.to(F64).reshape(groups, cpg) + beta.to(F64).reshape(groups, cpg)
    y = y.reshape(samples * rows, c)
    return (_silu(y) if silu else y), mean, rstd


def partial_statistics(p1, p2, samples, rows, groups, eps):
    """(mean, rstd) [samples][groups] from per-(row block, channel) sums P [samples blocks][channels][2] of the two sources (p2 may be
    None; the sources' blocks may differ in height): mean = sum / count, var = max(sum of squares / count - mean^2, 0)."""
    per = [p.to(F64).reshape(samples, -1, p.shape[1], 2).sum(1) for p in (p1, p2) if p is not None]
    ch = torch.cat(per, 1)                                                           # [samples][C][2]
    c = ch.shape[1]
    grp = ch.reshape(samples, groups, c // groups, 2).sum(2)
    count = rows * (c // groups)
    mean = grp[..., 0] / count
    var = (grp[..., 1] / count - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + eps)


def groupnorm_from_partials(p1, p2, x, gamma, beta, samples, rows, groups, eps, silu):
    mean, rstd = partial_statistics(p1, p2, samples, rows, groups, eps)
    return groupnorm(x, gamma, beta, samples, rows, groups, eps, silu, stats=(mean, rstd))


def layernorm(x, gamma, beta, eps):
    x = x.to(F64)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.to(F64) + beta.to(F64)


def softmax(s):
    s = s.to(F64)
    e = torch.exp(s - s.max(1, keepdim=True).values)
    return e / e.sum(1, keepdim=True)


def timestep_embedding(t, freqs, dim):
    """[n][dim] = [cos(a) | sin(a) | 0 if dim is odd], a = t * freqs[j] formed in fp32 (as on the device), cos / sin of it in fp64."""
    a = (t.to(F32)[:, None] * freqs.to(F32)[None, :]).to(F64)
    out = torch.zeros((t.shape[0], dim), dtype=F64)
    half = dim // 2
    out[:, :half], out[:, half:2 * half] = torch.cos(a), torch.sin(a)
    return out


def small_linear(x, w, b=None, act_in=False, act_out=False, into=None):
    """y = act_out(act_in(x) w^T + b) (+ into): x [M][K], w [N][K]; the activation is SiLU."""
    x = x.to(F64)
    y = (_silu(x) if act_in else x) @ w.to(F64).t()
    if b is not None:
        y = y + b.to(F64)
    if act_out:
        y = _silu(y)
    return y if into is None else into.to(F64) + y


def small_linear_magnitude(x, w, act_in=False):
    """sum_k |x w| per output: the scale of the fp32 accumulation error."""
    x = x.to(F64)
    return (_silu(x) if act_in else x).abs() @ w.to(F64).abs().t()


def ncthw_to_rows(src, t0, t):
    """(B, C, Ttot, H, W) -> rows ((b t) h w) x C of the frame window [t0, t0 + t)."""
    b, c = src.shape[:2]
    return src[:, :, t0:t0 + t].to(F64).permute(0, 2, 3, 4, 1).reshape(-1, c)


def rows_to_ncthw(rows, b, c, t, h, w, scale=1.0):
    """rows ((b t) h w) x C -> the (B, C, t, H, W) window, times scale."""
    return rows.to(F64).reshape(b, t, h, w, c).permute(0, 4, 1, 2, 3) * scale


def cast(value, kind, op_dtype=torch.bfloat16, planes=1):
    """What a cast stores: one rounding to fp32, to fp16 saturating at +-65504 (so +-inf too), or to the operand pieces."""
    return R.store_pieces(value, kind, op_dtype, planes)


def gaussian_sample(moments, noise, scale):
    """moments (N, 2C, H, W) -> scale (mean + exp(0.5 clamp(logvar, -30, 20)) noise); noise None = the mode."""
    m = moments.to(F64)
    c = m.shape[1] // 2
    mean, lv = m[:, :c], m[:, c:].clamp(-30.0, 20.0)
    return scale * (mean if noise is None else mean + torch.exp(0.5 * lv) * noise.to(F64))


def lincomb(x, y, ca, cb):
    shape = (-1,) + (1,) * (x.dim() - 1)
    return ca.to(F64).reshape(shape) * x.to(F64) + cb.to(F64).reshape(shape) * y.to(F64)


def axpy(y, x, alpha):
    return y.to(F64) + alpha * x.to(F64)


COEF = ("cfg", "phi", "sqrt_ac", "sqrt_1mac", "rescale", "sqrt_a_prev", "dir_coef", "sigma", "cfg_img", "eps_form")


def ddim_step(x, e_c, e_u, e_m, noise, coef):
    """One DDIM update on [B][n] latents; coef = the ten floats of mudg_ddim_step.  Returns (x_prev, pred_x0, ratio [B], mag0, mag):
    guidance e_u + cfg (e_c - e_u), or e_u + cfg_img (e_m - e_u) + cfg (e_c - e_m); phi > 0 rescales the guided prediction to the
    conditional one's UNBIASED standard deviation per sample and mixes phi : 1 - phi; eps_form picks the eps- or the v-prediction
    formulas.  mag0 / mag = the sum of the absolute values of every term that enters pred_x0 / x_prev (the guidance differences
    included): the scale of their fp32 rounding error."""
    k = dict(zip(COEF, [float(torch.tensor(v, dtype=F32)) for v in coef]))
    x, a = x.to(F64), e_c.to(F64)
    v, magv = a, a.abs()
    if e_u is not None:
        u = e_u.to(F64)
        if e_m is None:
            v, magv = u + k["cfg"] * (a - u), u.abs() + abs(k["cfg"]) * (a.abs() + u.abs())
        else:
            m = e_m.to(F64)
            v = u + k["cfg_img"] * (m - u) + k["cfg"] * (a - m)
            magv = u.abs() + abs(k["cfg_img"]) * (m.abs() + u.abs()) + abs(k["cfg"]) * (a.abs() + m.abs())
    ratio = torch.ones(x.shape[0], dtype=F64)
    if k["phi"] > 0:
        ratio = a.std(1, unbiased=True) / v.std(1, unbiased=True)
        v = k["phi"] * (v * ratio[:, None]) + (1.0 - k["phi"]) * v
        magv = (k["phi"] * ratio[:, None] + abs(1.0 - k["phi"])) * magv
    if k["eps_form"] != 0:
        e, mage = v, magv
        x0, mag0 = (x - k["sqrt_1mac"] * v) / k["sqrt_ac"], (x.abs() + abs(k["sqrt_1mac"]) * magv) / abs(k["sqrt_ac"])
    else:
        e, mage = k["sqrt_ac"] * v + k["sqrt_1mac"] * x, abs(k["sqrt_ac"]) * magv + abs(k["sqrt_1mac"]) * x.abs()
        x0, mag0 = k["sqrt_ac"] * x - k["sqrt_1mac"] * v, abs(k["sqrt_ac"]) * x.abs() + abs(k["sqrt_1mac"]) * magv
    x0, mag0 = x0 * k["rescale"], mag0 * abs(k["rescale"])
    nz = k["sigma"] * noise.to(F64) if noise is not None else torch.zeros_like(x)
    x_prev = k["sqrt_a_prev"] * x0 + k["dir_coef"] * e + nz
    mag = abs(k["sqrt_a_prev"]) * mag0 + abs(k["dir_coef"]) * mage + nz.abs()
    return x_prev, x0, ratio, mag0, mag


# ================================================================================================ host rules, restated
def gn_chunks(rows):
    """Row chunks per sample of the statistics pass (csrc/norm.hip, gn_chunks): rows / 16 below 2048 rows, rows / 64 from there, in 1 .. 1024."""
    return max(1, min(1024, rows // (64 if rows >= 2048 else 16)))


def gn_chunk_rows(rows):
    return -(-rows // gn_chunks(rows))


def gn_empty_chunks(rows):
    """Chunks that start at or past the last row."""
    n, rpc = gn_chunks(rows), gn_chunk_rows(rows)
    return sum(1 for ch in range(n) if ch * rpc >= rows)


def gn_stats_sweep(nvec):
    """Vectors per sweep: the largest divisor of nvec <= 256 whose row classes keep >= 240 of 256 lanes busy, else the busiest."""
    best, used = 1, 0
    for d in range(min(nvec, 256), 0, -1):
        if nvec % d:
            continue
        u = (256 // d) * d
        if u >= 240:
            return d
        if u > used:
            used, best = u, d
    return best


def gn_apply(c, aligned=True, reg=True):
    """(CS, kernel, rows per workgroup): the slab is the largest divisor of C that is <= 640 and a multiple of 64 (of 8 if there is none),
    from 128 up; C itself when C <= 640 or there is no such divisor.  The register kernel takes slabs of <= 256 vectors with 16-byte
    aligned gamma / beta (and MUDG_GN_REG != 0), 256 / nvec rows per pass and GN_UNROLL passes; the LDS-table kernel the rest."""
    cs = c
    if c > 640:
        best = next((d for d in range(640, 127, -64) if c % d == 0), 0) or next((d for d in range(640, 127, -8) if c % d == 0), 0)
        cs = best or c
    nvec = cs // 8
    if reg and nvec <= 256 and aligned:
        return cs, "reg", (256 // nvec) * GN_UNROLL
    return cs, "lds", max(1, 256 * GN_UNROLL // nvec)


LN_ROWS = {320: (8, 5), 512: (16, 4), 640: (16, 5), 1024: (32, 4), 1280: (32, 5)}         # C -> (LPR, NV)


def ln_kernel(c, rows_switch=True):
    """The LayerNorm kernel of a width, and the rows a workgroup takes."""
    if rows_switch and c in LN_ROWS:
        lpr, nv = LN_ROWS[c]
        return f"ln_rows<{lpr},{nv}>", 4 * (64 // lpr)
    return ("ln<3>" if c // 8 <= 192 else "ln<8>"), 4


def rows_vec(cols, lds, ldd, src_kind, dst_kind, src_off, dst_off, planes):
    """The VEC condition of mudg_cast_rows (mudg_copy_rows with both kinds = operand): cols % 8 == 0, both row strides whole 8-element
    vectors (of every plane for operand storage), both base pointers 16-byte aligned.  src_off / dst_off: elements past an aligned address."""
    esz = {KIND_OPERAND: 2, KIND_F32: 4, KIND_F16: 2}
    gran = lambda kind: 8 * planes if kind == KIND_OPERAND else 8
    return (cols % 8 == 0 and lds % gran(src_kind) == 0 and ldd % gran(dst_kind) == 0
            and (src_off * esz[src_kind]) % 16 == 0 and (dst_off * esz[dst_kind]) % 16 == 0)


# ================================================================================================ fp32 emulations
def _fma(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 numbers is exact in fp64; one extra rounding (fp64 sum, then fp32) is 2^-53."""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def gn_stats_emulated(x, samples, rows, groups, eps):
    """The one-pass formula as the statistics kernel documents it: per (sample, chunk) fp32 sums and sums of squares per channel (fmaf
    for the squares), the channels of a group added up one after the other in fp32, the chunks folded in fp64; mean = a / n,
    var = max(b / n - mean^2, 0); both statistics rounded to fp32.  The order of the rows inside a channel sum is torch's."""
    c = x.shape[1]
    cpg = c // groups
    x = x.to(F32).reshape(samples, rows, groups, cpg)
    rpc = gn_chunk_rows(rows)
    a = torch.zeros((samples, groups), dtype=F64)
    b = torch.zeros((samples, groups), dtype=F64)
    for r0 in range(0, rows, rpc):
        blk = x[:, r0:r0 + rpc]
        cs, cq = blk.sum(1, dtype=F32), (blk * blk).sum(1, dtype=F32)             # [samples][groups][cpg]
        ga, gb = torch.zeros((samples, groups), dtype=F32), torch.zeros((samples, groups), dtype=F32)
        for j in range(cpg):
            ga, gb = ga + cs[..., j], gb + cq[..., j]
        a += ga.to(F64)
        b += gb.to(F64)
    count = rows * cpg
    mean = a / count
    var = (b / count - mean * mean).clamp_min(0.0)
    return mean.to(F32), (1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=F32)))).to(F32)


def gn_apply_emulated(x, mean, rstd, gamma, beta, samples, rows, groups, silu):
    """sc = rstd * gamma, sh = beta - mean * sc, y = fmaf(x, sc, sh), SiLU as y / (1 + exp(-y)): every step one fp32 rounding."""
    c = x.shape[1]
    cpg = c // groups
    x = x.to(F32).reshape(samples, rows, groups, cpg)
    g, b = gamma.to(F32).reshape(groups, cpg), beta.to(F32).reshape(groups, cpg)
    sc = rstd.to(F32)[:, None, :, None] * g
    sh = b - mean.to(F32)[:, None, :, None] * sc
    y = _fma(x, sc.expand_as(x), sh.expand_as(x))
    if silu:
        y = y / (1.0 + torch.exp(-y))
    return y.reshape(samples * rows, c)


def layernorm_emulated(x, gamma, beta, eps):
    """mean = sum / C, q = sum of fmaf(d, d, q) with d = x - mean, rstd = rsqrt(q / C + eps), y = fmaf((x - mean) rstd, gamma, beta)."""
    x = x.to(F32)
    c = x.shape[1]
    mean = x.sum(1, keepdim=True, dtype=F32) / c
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True, dtype=F32) / c + torch.tensor(eps, dtype=F32))
    return _fma(d * rstd, gamma.to(F32).expand_as(x), beta.to(F32).expand_as(x))


def softmax_emulated(s):
    """max, sum of exp(s - max), exp(s - max) * (1 / sum): three passes in fp32."""
    s = s.to(F32)
    e = torch.exp(s - s.max(1, keepdim=True).values)
    return e * (1.0 / e.sum(1, keepdim=True, dtype=F32))


# ================================================================================================ exact GroupNorm inputs
PQ = ((1, 3), (5, 9), (7, 21))            # (p, q): var = (p^2 + q^2) / 2 = 5 | 53 | 245; + eps 11 = 16 | 64 | 256; rstd = 1/4 | 1/8 | 1/16
EXACT_EPS = 11.0
GAMMAS = (1.0, -1.0, 2.0, -2.0, 4.0, -4.0)


def exact_mean(s, g):
    """The integer mean of (sample, group): differs between neighbours in both directions."""
    return float((5 * s + 3 * g) % 13 - 6)


def exact_rstd(g):
    p, q = PQ[g % 3]
    return 1.0 / math.sqrt((p * p + q * q) / 2 + EXACT_EPS)


def exact_groupnorm_input(samples, rows, c, groups, seed):
    """x [samples rows][C] (fp32 integers): (sample, group) holds m + {+p, -p, +q, -q} in equal counts (rows * cpg % 4 == 0), placed by a
    seeded permutation over (row, channel).  mean = m, var = (p^2 + q^2) / 2, both exactly."""
    cpg = c // groups
    n = rows * cpg
    assert n % 4 == 0, "equal counts need rows * cpg % 4 == 0"
    x = torch.empty((samples, rows, groups, cpg), dtype=F32)
    g_ = gen(seed)
    for g in range(groups):
        p, q = PQ[g % 3]
        vals = torch.tensor([p, -p, q, -q], dtype=F32).repeat(n // 4)
        for s in range(samples):
            x[s, :, g, :] = (vals[torch.randperm(n, generator=g_)] + exact_mean(s, g)).reshape(rows, cpg)
    return x.reshape(samples * rows, c)


def exact_affine(c, seed):
    """gamma in {+-1, +-2, +-4}, beta an integer in -2 .. 2."""
    g_ = gen(seed)
    gamma = torch.tensor(GAMMAS)[torch.randint(0, len(GAMMAS), (c,), generator=g_)]
    beta = torch.randint(-2, 3, (c,), generator=g_).to(F32)
    return gamma, beta


def integer_split(total, n, seed, spread=40):
    """n integers that add up to `total`: total // n (+ 1 for the first total % n) plus zero-sum integer noise, shuffled."""
    q, r = divmod(int(total), n)
    g_ = gen(seed)
    noise = torch.randint(-spread, spread + 1, (n,), generator=g_)
    v = torch.full((n,), q, dtype=torch.int64) + (torch.arange(n) < r).to(torch.int64) + noise - torch.roll(noise, 1)
    return v[torch.randperm(n, generator=g_)].to(F64)


def exact_partials(samples, rows, c, csplit, groups, h1, h2, seed, clamp=False):
    """Hand-made integer partials P1 [samples rows / h1][csplit][2], P2 [samples rows / h2][C - csplit][2] (None when csplit == C)
    whose totals per (sample, group) are count m and count (m^2 + (p^2 + q^2) / 2): the statistics of exact_mean / exact_rstd, spread
    over every (block, channel) entry of the group in both sources.  clamp: every group gets a sum of squares of count (m^2 - 3), a
    negative variance, which the definition clamps to 0 (rstd = 1 / sqrt(eps))."""
    cpg = c // groups
    count = rows * cpg
    b1, b2 = rows // h1, rows // h2
    p1 = torch.zeros((samples, b1, csplit, 2), dtype=F64)
    p2 = torch.zeros((samples, b2, c - csplit, 2), dtype=F64) if csplit < c else None
    for s in range(samples):
        for g in range(groups):
            m = exact_mean(s, g)
            p, q = PQ[g % 3]
            v = -3 if clamp else (p * p + q * q) // 2
            lo, hi = g * cpg, (g + 1) * cpg
            n1 = b1 * max(0, min(hi, csplit) - lo)
            n2 = b2 * max(0, hi - max(lo, csplit))
            for j, total in enumerate((count * m, count * (m * m + v))):
                vals = integer_split(total, n1 + n2, seed + 7 * (s * groups + g) + j)
                if n1:
                    p1[s, :, lo:min(hi, csplit), j] = vals[:n1].reshape(b1, -1)
                if n2:
                    p2[s, :, max(lo, csplit) - csplit:hi - csplit, j] = vals[n1:].reshape(b2, -1)
    return p1.reshape(samples * b1, csplit, 2), (None if p2 is None else p2.reshape(samples * b2, c - csplit, 2))
