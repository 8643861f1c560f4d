"""CPU definitions of the forward attention entries (include/mudg_hip.h: mudg_attention, mudg_temporal_attention) in the layouts the
header documents, and constructors of inputs whose exact output is known without any arithmetic.  Nothing here comes from mudg_amd:
tests/test_attention_reference_cpu.py checks the definitions against torch.nn.functional.scaled_dot_product_attention in fp64 and
every constructor's condition at every shape of tests/test_attention_kernels_gpu.py, which holds the HIP kernels to them.

Exponent convention of the kernels: P = 2^(c s - lse2), c = scale log2(e), or c = 1 where Q already carries scale log2(e) (base2)."""
import math

import torch

from backward_reference import operand_planes

F64 = torch.float64
LOG2E = 1.4426950408889634
CODE = 4.0                      # the gather codes are +-CODE: exact in every operand type
LEAN_LIMIT_LOG2 = 40            # csrc/attn_shared.h LEAN_LIMIT with bf16 operands (2^15 with fp16 ones)


def through(round_to, dtype=F64):
    """round_to = None | a 16-bit dtype | (dtype, pieces): the function that passes a tensor through that operand storage."""
    if round_to is None:
        return lambda t: t
    op, planes = round_to if isinstance(round_to, tuple) else (round_to, 1)
    return lambda t: sum(p.to(dtype) for p in operand_planes(t, op, planes))


def _one_set(q, k, v, frames, heads, nq, nk, kv_div, c2, rt, dtype):
    o = torch.zeros((frames * nq, heads * 64), dtype=dtype)
    lse2 = torch.zeros((frames * nq, heads), dtype=dtype)
    for f in range(frames):
        qs, ks = slice(f * nq, (f + 1) * nq), slice((f // kv_div) * nk, (f // kv_div + 1) * nk)
        for h in range(heads):
            hs = slice(64 * h, 64 * h + 64)
            s = (q[qs, hs] @ k[ks, hs].t()) * (c2 * math.log(2.0))                 # natural-log scores
            lse = torch.logsumexp(s, dim=1)
            o[qs, hs] = rt(torch.exp(s - lse[:, None])) @ v[ks, hs]
            lse2[qs, h] = lse / math.log(2.0)
    return o, lse2


def attention(q, k, v, *, frames, heads, nq, nk, kv_div=1, scale=None, base2=False, k2=None, v2=None, nk2=0, kv_div2=1, add=None,
              round_to=None, dtype=F64):
    """(O, lse2) of O = softmax(scale Q K^T) V per (frame, head), head width 64: q [frames nq][heads 64]; k, v [(frames / kv_div) nk]
    [heads 64], kv_div consecutive frames sharing one key / value batch.  base2: softmax of 2^(Q K^T) (scale ignored).  k2 / v2: a
    second set with its own softmax (and its own kv_div2) whose output is added; add: what O is added onto (accumulate).  lse2 [frames nq][heads] = log2 sum_j 2^(c s_j) of the
    first set.  round_to: P passes through that operand storage before P V and O is rounded once — the two deliberate roundings of the
    kernels; everything else stays in `dtype`."""
    assert base2 or scale is not None
    c2 = 1.0 if base2 else scale * LOG2E
    rt = through(round_to, dtype)
    q, k, v = (t.to(dtype) for t in (q, k, v))
    o, lse2 = _one_set(q, k, v, frames, heads, nq, nk, kv_div, c2, rt, dtype)
    if k2 is not None:
        o = o + _one_set(q, k2.to(dtype), v2.to(dtype), frames, heads, nq, nk2, kv_div2, c2, rt, dtype)[0]
    if add is not None:
        o = o + add.to(dtype)
    return rt(o), lse2


def temporal_attention(qkv, *, clips, t, hw, heads, scale, round_to=None, dtype=F64):
    """Self-attention over the t frames of every pixel: qkv rows ((b t) hw) = [q | k | v], head h at columns [64 h, 64 h + 64) of each."""
    c = heads * 64
    rt = through(round_to, dtype)
    x = qkv[:, :3 * c].to(dtype).reshape(clips, t, hw, 3, heads, 64).permute(3, 0, 2, 4, 1, 5)          # [3][b][s][h][t][64]
    p = torch.softmax(scale * (x[0] @ x[1].transpose(-1, -2)), dim=-1)
    return rt((rt(p) @ x[2]).permute(0, 3, 1, 2, 4).reshape(clips * t * hw, c))


# ------------------------------------------------------------------------------------------------ the shapes of the GPU file
# (name, frames, heads, nq, nk, kv_div): the kernel each one reaches under the shipped rule is named in the GPU file, which asserts
# the rule's conditions on the numbers.  More than one head and more than one frame everywhere.
SHAPES = [
    ("few tiles, ragged keys", 4, 2, 200, 77, 2),
    ("Nk > 128, short queries", 2, 2, 333, 333, 1),
    ("Nq 511", 2, 2, 511, 256, 1),
    ("Nk 255", 2, 2, 512, 255, 1),
    ("many query tiles, ragged last", 8, 5, 128 * 51 + 40, 77, 4),
    ("long, ragged keys", 2, 2, 520, 520, 1),
    ("long, Nq 512 Nk 256", 2, 2, 512, 256, 1),
    ("long, Nq 513 Nk 320", 2, 3, 513, 320, 1),
    ("long, shared keys", 4, 2, 640, 384, 2),
    ("long, 2304 tokens", 2, 2, 2304, 2304, 1),
]
SHAPE = {s[0]: s[1:] for s in SHAPES}
# (name, frames, heads, nq, nk, kv_div, nk2, kv_div2): a second key / value set
TWO_SET_SHAPES = [
    ("text + image, few tiles", 4, 2, 150, 77, 2, 16, 1),
    ("text + ragged second set", 4, 5, 200, 77, 4, 150, 1),
    ("text + image, many query tiles", 8, 5, 128 * 51 + 40, 77, 4, 16, 1),
]
# (clips, t, hw, heads)
TEMPORAL_SHAPES = [(2, 1, 37, 5), (2, 15, 37, 1), (2, 16, 37, 5), (1, 17, 37, 5), (2, 32, 37, 1), (1, 32, 13, 5)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ constructors
def _codes(n, g):
    """n rows of +-CODE of width 64, any two of which differ in at least 12 places: the score of a row against itself is 64 CODE^2,
    against any other at most (64 - 24) CODE^2 — with CODE = 4 and scale 0.125 that is 128 nats against at most 80."""
    c = torch.where(torch.rand((n, 64), generator=g) < 0.5, -1.0, 1.0)
    for _ in range(64):
        dots = c @ c.t() - 64.0 * torch.eye(n)
        bad = (dots.max(1).values > 64 - 24).nonzero().flatten()
        if bad.numel() == 0:
            return c * CODE
        c[bad] = torch.where(torch.rand((bad.numel(), 64), generator=g) < 0.5, -1.0, 1.0)
    raise AssertionError("no code set found")


def gather_problem(frames, heads, nq, nk, kv_div, seed, first_tile=False):
    """(q, k, v, pi, want): q row i of (frame f, head h) is the code of key pi[f][h][i] of its batch, so softmax puts all weight on
    that key and O = V[pi] — bit for bit where 1 - p_target is below every rounding in sight (the CPU file asserts 2^-40) and no
    element of V is zero (asserted there too, element by element).  pi walks
    random permutations of the keys (of the first 64 keys when first_tile), so every key is some row's target — the last valid key of
    a ragged tile by construction: pi[0][0][nq - 1] = nk - 1 (63).  "Every key" is meant over the whole problem: a single (frame,
    head) with fewer rows than keys cannot name them all."""
    g = gen(seed)
    batches, span = frames // kv_div, (min(nk, 64) if first_tile else nk)
    k = torch.cat([torch.cat([_codes(nk, g) for _ in range(heads)], 1) for _ in range(batches)])            # [batches nk][heads 64]
    # V: +-(1 .. 64) / 8, 7 bits, exact in bf16 / fp16 — and never zero: the other keys leave sum_j p_j V_j, at most Nk e^-48 max|V| ~
    # 1e-16, in O; next to |V[pi]| >= 1/8 that is 2^-50 of the value and rounds away, next to a zero it would be the whole output
    v = torch.randint(1, 65, (batches * nk, heads * 64), generator=g).float() / 8.0
    v = torch.where(torch.rand(v.shape, generator=g) < 0.5, -v, v)
    pi = torch.empty((frames, heads, nq), dtype=torch.int64)
    for h in range(heads):
        walk = torch.cat([torch.randperm(span, generator=g) for _ in range((frames * nq + span - 1) // span)])[:frames * nq]
        pi[:, h] = walk.reshape(frames, nq)
    pi[0, 0, nq - 1] = span - 1
    if span > 64:
        # every 128-query block keeps a row whose target lies beyond the first 64 keys (a ragged last block may hold one row only): a
        # block without one trades its first target for that of a row in a block that has two
        for f in range(frames):
            for h in range(heads):
                far = pi[f, h] >= 64
                count = [int(far[b:b + 128].sum()) for b in range(0, nq, 128)]
                for b, n in enumerate(count):
                    if n == 0:
                        d = max(range(len(count)), key=lambda j: count[j])
                        assert count[d] >= 2
                        j = 128 * d + int(far[128 * d:min(128 * d + 128, nq - 1)].nonzero()[0])
                        i = 128 * b
                        pi[f, h, i], pi[f, h, j] = pi[f, h, j].clone(), pi[f, h, i].clone()
                        far = pi[f, h] >= 64
                        count[d] -= 1
    q = torch.empty((frames * nq, heads * 64))
    want = torch.empty((frames * nq, heads * 64))
    for f in range(frames):
        for h in range(heads):
            rows = (f // kv_div) * nk + pi[f, h]
            q[f * nq:(f + 1) * nq, 64 * h:64 * h + 64] = k[rows, 64 * h:64 * h + 64]
            want[f * nq:(f + 1) * nq, 64 * h:64 * h + 64] = v[rows, 64 * h:64 * h + 64]
    return q, k, v, pi, want


def gather_two_set_problem(frames, heads, nq, nk, kv_div, nk2, kv_div2, seed, second):
    """(q, k, v, k2, v2, pi, want, const): a gather through one set of a two-set call while the other set is uniform (its K = 0, its V
    a constant over keys), so O = V[pi] + const — second = False gathers through the first set (Nk keys, kv_div), True through the
    second (Nk2 keys, kv_div2): its last-key mask and its batch mapping get the whole-row check.  The constants are multiples of
    1/8 in [16.25, 22]: the sum with V in [-8, 8] lies in [8.25, 30], never cancels and needs at most 8 significant bits."""
    c = heads * 64
    gk, gdiv, uk, udiv = (nk2, kv_div2, nk, kv_div) if second else (nk, kv_div, nk2, kv_div2)
    q, kg, vg, pi, want = gather_problem(frames, heads, nq, gk, gdiv, seed)
    ub = frames // udiv
    vals = ((torch.arange(ub * c, dtype=torch.int64).reshape(ub, c) * 5) % 47 + 130).float() / 8.0
    const = vals.repeat_interleave(udiv * nq, 0)
    ku, vu = torch.zeros((ub * uk, c)), vals.repeat_interleave(uk, 0)
    k, v, k2, v2 = (ku, vu, kg, vg) if second else (kg, vg, ku, vu)
    return q, k, v, k2, v2, pi, want + const, const


def gather_margins(q, k, pi, *, frames, heads, nq, nk, kv_div, c2):
    """What the gather relies on, in fp64 from the operand values given (c2: log2 units per unit of q k): per row the target's score
    and the gap to the best other key (nats), 1 - p_target, and — for the lean softmax, whose reference is the row maximum over the
    first 64 keys — log2 of the largest 64-key tile sum of 2^(s - m_ref).  Each [frames nq][heads]."""
    shape = (frames * nq, heads)
    target, gap, miss, tile = (torch.zeros(shape, dtype=F64) for _ in range(4))
    q, k = q.to(F64), k.to(F64)
    for f in range(frames):
        for h in range(heads):
            rows = slice(f * nq, (f + 1) * nq)
            s2 = (q[rows, 64 * h:64 * h + 64] @ k[(f // kv_div) * nk:(f // kv_div + 1) * nk, 64 * h:64 * h + 64].t()) * c2
            st = s2.gather(1, pi[f, h][:, None])
            others = s2.scatter(1, pi[f, h][:, None], -math.inf)
            rest = torch.exp2(others - st).sum(1)                                   # sum over the other keys of p_j / p_target
            target[rows, h] = st[:, 0] * math.log(2.0)
            gap[rows, h] = (st[:, 0] - others.max(1).values) * math.log(2.0)
            miss[rows, h] = rest / (1.0 + rest)
            m_ref = s2[:, :64].max(1, keepdim=True).values
            pad = (-nk) % 64
            e = torch.cat([torch.exp2(s2 - m_ref), s2.new_zeros(nq, pad)], 1).reshape(nq, -1, 64).sum(2)
            tile[rows, h] = torch.log2(e.max(1).values)
    return target, gap, miss, tile


def uniform_values(batches, heads, second=False):
    """[batches][heads 64] of small dyadic numbers, distinct per (batch, head, channel) within a problem: multiples of 1/8 in [-6, 6];
    the second set's lie in [6.25, 12], so the sum of the two is never zero and needs at most 8 significant bits."""
    idx = torch.arange(batches * heads * 64, dtype=torch.int64).reshape(batches, heads * 64)
    return (((idx * 5) % 47 + 50) if second else ((idx * 7) % 97 - 48)).float() / 8.0


def uniform_problem(frames, heads, nq, nk, kv_div, seed, nk2=0, kv_div2=1):
    """(q, k, v, k2, v2, want, lse2): K = 0, so every key weighs 1 / Nk whatever Q is; V is constant over the keys of a batch, so
    O = that constant (+ the second set's) and lse2 = log2 Nk."""
    c = heads * 64
    q = torch.randn((frames * nq, c), generator=gen(seed))
    b1 = frames // kv_div
    v1 = uniform_values(b1, heads)
    want = v1.repeat_interleave(kv_div * nq, 0)
    k2 = v2 = None
    if nk2:
        b2 = frames // kv_div2
        vals2 = uniform_values(b2, heads, second=True)
        k2, v2 = torch.zeros((b2 * nk2, c)), vals2.repeat_interleave(nk2, 0)
        want = want + vals2.repeat_interleave(kv_div2 * nq, 0)
    return q, torch.zeros((b1 * nk, c)), v1.repeat_interleave(nk, 0), k2, v2, want, torch.full((frames * nq, heads), math.log2(nk), dtype=F64)
