"""Case tables, operand builders and fp64 references of tests/test_train_functions_gpu.py (the autograd Functions of
mudg_amd/train/functions.py, one by one).  Nothing here touches a GPU: tests/test_train_functions_cpu.py builds every exact case and
checks the condition the GPU test rests on — integer operands, integer results below 2^24 — before a GPU is involved.

A case's operands are a dict name -> fp32 CPU tensor (x, w, b bias, e group bias, r residual) plus the output gradient dy; the reference
is torch autograd of the textbook op in fp64 on those very values."""
import itertools

import torch
import torch.nn.functional as F

from test_backward_kernels_gpu import ints, rnd

MAIN, SIDE = ("x", "w", "b"), ("e", "r")

# (M rows, K, N, bias, residual); K % 8 == 0
LINEAR_CASES = [
    (1, 64, 72, True, False),              # one row, the time-embedding shape: positions = 1
    (3, 320, 136, True, False),            # a few rows, N wider than a 128 tile
    (77, 72, 64, False, False),            # K not in 64-blocks: the transposed route in every build; no bias (to_k on the context)
    (200, 96, 20, True, True),             # N % 8 != 0: dy is padded
    (1030, 128, 72, True, True),           # direct route (16-bit builds); 1030 = 16 * 64 + 6: a ragged last chunk of the column sums
    (4100, 128, 72, True, False),          # kernels.wgrad cuts the rows into 4 slices of 1088
    (4100, 96, 72, True, False),           # _splits > 1 on the transposed route
]
# (frames, h, w, stride, Cin, Cout, bias, groups of the group bias or 0, residual)
CONV_CASES = [
    (2, 5, 7, 1, 12, 24, True, 2, True),           # Cin padded to 16, transposed route
    (2, 6, 8, 2, 12, 24, True, 0, False),          # stride 2, even grid
    (3, 9, 11, 2, 64, 72, True, 3, True),          # stride 2, odd grid, direct route
    (2, 8, 8, 1, 64, 4, True, 0, False),           # Cout = 4, the UNet's out conv
    (1, 10, 12, 1, 192, 136, False, 0, False),     # an output tile of dW straddles two taps
    (4, 24, 32, 1, 64, 64, True, 2, True),         # mudg_wgrad path 1; groups of 1536 rows
    (2, 48, 64, 1, 64, 8, False, 1, False),        # one group of 6144 rows: the group_colsum chunk ladder (1024 x 6)
]
# (clips, t, hw, Cin, Cout); bias always; residual = x where Cin == Cout
TCONV_CASES = [
    (2, 5, 12, 64, 64),            # affine temporal taps, one slice
    (1, 4, 9, 24, 24),             # transposed route in every build
    (1, 1, 64, 64, 72),            # t = 1: both neighbours are padding
    (2, 8, 256, 64, 64),           # several slices
]
# the one Gaussian case of each (section B of the file's docstring)
LINEAR_GAUSS, CONV_GAUSS, TCONV_GAUSS = LINEAR_CASES[4], CONV_CASES[2], TCONV_CASES[0]

GN_CASES = [(3, 50, 64), (1, 7, 320), (2, 1030, 128)]          # (samples, rows, C), 32 groups
LN_CASES = [(77, 320), (1, 64), (130, 1280)]                   # (rows, C)
GEGLU_CASES = [(67, 324), (1, 8)]                              # (M, N): h is [M][2 N]
# (frames, heads, nq, nk, kv_div, nk2, kv_div2); nk2 = 0: one key / value set
ATTN_CASES = [(4, 2, 40, 40, 1, 0, 1), (4, 2, 200, 150, 2, 0, 1), (4, 2, 40, 77, 2, 16, 1)]
SCALE = 0.125


def int_make(*shape, seed=0, scale=1.0):
    return ints(*shape, seed=seed)


def gauss_make(*shape, seed=0, scale=1.0):
    return rnd(*shape, seed=seed, scale=scale)


def conv_out(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def linear_problem(case, make, seed=0):
    m, k, n, bias, res = case
    t = dict(x=make(m, k, seed=seed + 1), w=make(n, k, seed=seed + 2, scale=0.1))
    if bias:
        t["b"] = make(n, seed=seed + 3)
    if res:
        t["r"] = make(m, n, seed=seed + 4)
    return t, make(m, n, seed=seed + 5)


def linear_ref(x, w, b=None, r=None):
    y = F.linear(x, w, b)
    return y if r is None else y + r


def linear_apply(Fn, case, g):
    return Fn.Linear.apply(g["x"], g["w"], g.get("b"), g.get("r"))


def conv_problem(case, make, seed=0):
    frames, h, w, stride, ci, co, bias, groups, res = case
    ho, wo = conv_out(h, w, stride)
    t = dict(x=make(frames * h * w, ci, seed=seed + 1), w=make(co, ci, 3, 3, seed=seed + 2, scale=0.1))
    if bias:
        t["b"] = make(co, seed=seed + 3)
    if groups:
        t["e"] = make(groups, co, seed=seed + 4)
    if res:
        t["r"] = make(frames * ho * wo, co, seed=seed + 5)
    return t, make(frames * ho * wo, co, seed=seed + 6)


def conv_rows_per_group(case):
    frames, h, w, stride, ci, co, bias, groups, res = case
    ho, wo = conv_out(h, w, stride)
    return (frames // groups) * ho * wo if groups else 0


def conv_ref_of(case):
    frames, h, w, stride, ci, co, bias, groups, res = case

    def ref(x, w, b=None, e=None, r=None):
        y = F.conv2d(x.reshape(frames, h, case[2], ci).permute(0, 3, 1, 2), w, b, stride=stride, padding=1)
        if e is not None:
            y = y + e.repeat_interleave(frames // groups, 0)[:, :, None, None]
        y = y.permute(0, 2, 3, 1).reshape(-1, co)
        return y if r is None else y + r
    return ref


def conv_apply(Fn, case, g):
    frames, h, w, stride = case[:4]
    return Fn.Conv3x3.apply(g["x"], g["w"], g.get("b"), g.get("e"), g.get("r"), (frames, h, w, stride), conv_rows_per_group(case))


def tconv_problem(case, make, seed=0):
    """The residual is x itself where the widths allow it: the reference keeps it a separate leaf "r" of the same values, so that
    what the Function returns for the conv's input and for its residual are compared one by one."""
    clips, t, hw, ci, co = case
    ops_ = dict(x=make(clips * t * hw, ci, seed=seed + 1), w=make(co, ci, 3, 1, 1, seed=seed + 2, scale=0.1), b=make(co, seed=seed + 3))
    if ci == co:
        ops_["r"] = ops_["x"].clone()
    return ops_, make(clips * t * hw, co, seed=seed + 4)


def tconv_ref_of(case):
    clips, t, hw, ci, co = case

    def ref(x, w, b, r=None):
        y = F.conv3d(x.reshape(clips, t, hw, 1, ci).permute(0, 4, 1, 2, 3), w, b, padding=(1, 0, 0))
        y = y.permute(0, 2, 3, 4, 1).reshape(-1, co)
        return y if r is None else y + r
    return ref


def tconv_apply(Fn, case, g):
    clips, t, hw, ci, co = case
    return Fn.TConv3.apply(g["x"], g["w"], g["b"], g["x"] if ci == co else None, (clips, t, hw))


# name -> (cases, problem builder, reference of a case, how to call the Function, its class name, the operand each input position holds,
#          operands that are one tensor on the GPU side)
FAMILIES = {
    "linear": (LINEAR_CASES, linear_problem, lambda case: linear_ref, linear_apply, "Linear", ("x", "w", "b", "r"), {}),
    "conv3x3": (CONV_CASES, conv_problem, conv_ref_of, conv_apply, "Conv3x3", ("x", "w", "b", "e", "r", None, None), {}),
    "tconv3": (TCONV_CASES, tconv_problem, tconv_ref_of, tconv_apply, "TConv3", ("x", "w", "b", "r", None), {"r": "x"}),
}
EXACT_IDS = [(fam, i) for fam, spec in FAMILIES.items() for i in range(len(spec[0]))]
GAUSS = {"linear": LINEAR_GAUSS, "conv3x3": CONV_GAUSS, "tconv3": TCONV_GAUSS}


def needs_subsets(tensors, tied):
    """Every non-empty subset of the (x, w, b) present, each with the residual and the group bias requiring gradients too; then the
    residual alone and the group bias alone (an operand tied to another one follows it and is never asked for alone).  The first entry
    asks for everything."""
    main = [k for k in MAIN if k in tensors]
    side = [k for k in SIDE if k in tensors and k not in tied]
    out = [frozenset(s) | frozenset(side) for n in range(len(main), 0, -1) for s in itertools.combinations(main, n)]
    return out + [frozenset([k]) for k in side]


def reference(ref, tensors, dy, dtype=torch.float64, rt=None):
    """(y, {name: gradient}) of `ref` by torch autograd in `dtype`.  rt: x, w and dy pass through it first (the operand storage of a
    build); bias, group bias and residual stay as they are."""
    rt = rt or (lambda v: v)
    leaves = {k: (rt(v).to(dtype) if k in ("x", "w") else v.to(dtype)).clone().requires_grad_(True) for k, v in tensors.items()}
    y = ref(**leaves)
    names = list(leaves)
    grads = torch.autograd.grad(y, [leaves[k] for k in names], rt(dy).to(dtype))
    return y.detach(), dict(zip(names, grads))


def is_integer_valued(t, limit):
    t = t.double()
    return bool((t == t.round()).all()) and float(t.abs().max()) < limit if t.numel() else True


# ------------------------------------------------------------------------------------------------ textbook forms of the other Functions
def groupnorm_ref(samples, rows, c, silu, groups=32, eps=1e-5):
    def ref(x, g, b):
        y = F.group_norm(x.reshape(samples, rows, c).transpose(1, 2), groups, g, b, eps)
        return (F.silu(y) if silu else y).transpose(1, 2).reshape(-1, c)
    return ref


def attention_ref(q, k, v, frames, heads, nq, nk, kv_div, scale):
    c = q.shape[1]
    qh = q.reshape(frames, nq, heads, 64).transpose(1, 2)
    kh = k.reshape(frames // kv_div, nk, heads, 64).transpose(1, 2).repeat_interleave(kv_div, 0)
    vh = v.reshape(frames // kv_div, nk, heads, 64).transpose(1, 2).repeat_interleave(kv_div, 0)
    return (torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).transpose(1, 2).reshape(frames * nq, c)


def temporal_attention_ref(qkv, clips, t, hw, heads, scale):
    c = heads * 64
    x = qkv.reshape(clips, t, hw, 3, heads, 64).permute(3, 0, 2, 4, 1, 5)            # (3, b, s, h, t, d)
    o = torch.softmax(x[0] @ x[1].transpose(-1, -2) * scale, -1) @ x[2]
    return o.permute(0, 3, 1, 2, 4).reshape(clips * t * hw, c)
