"""CPU definitions of the image tower's pieces (include/mudg_hip.h: mudg_clip_preprocess, mudg_short_attention; mudg_amd/engine/clip.py),
written from the rules of DESIGN.md §17.  Nothing here comes from mudg_amd.

  preprocess        fp32, operation for operation: the HIP kernel is held to it with torch.equal
  short_attention   fp64 (or `dtype`), optionally with the kernel's deliberate roundings (q, k, v, P and O through operand storage)
  tower             fp64 pre-LN ViT in open_clip's layout, optionally with every MFMA operand through operand storage
"""
import math

import numpy as np
import torch

from attention_reference import LOG2E, through

F64 = torch.float64
SIZE, PATCH, GRID, K, KPAD = 224, 14, 16, 588, 592
MEAN = np.array([0.48145466, 0.4578275, 0.40821073], dtype=np.float32)          # condition.py:318-319, as torch.Tensor([...]) holds them
STD = np.array([0.26862954, 0.26130258, 0.27577711], dtype=np.float32)
CUBIC_A = -0.75


# ------------------------------------------------------------------------------------------------ preprocessing
def blur_taps(n_src, n_dst=SIZE):
    """(k,) fp32 Gaussian taps of one axis: sigma = max((n_src / n_dst - 1) / 2, 0.001), k = int(max(4 sigma, 3)) made odd."""
    f = np.float64(n_src) / np.float64(n_dst)
    sigma = max((f - 1.0) / 2.0, 0.001)
    k = int(max(4.0 * sigma, 3.0))
    if k % 2 == 0:
        k += 1
    i = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    g = np.exp(-(i ** 2) / (2.0 * sigma ** 2))
    return (g / g.sum()).astype(np.float32)


def cubic_taps(n_src, n_dst=SIZE):
    """(indices (n_dst, 4) int64 clamped to the image, coefficients (n_dst, 4) fp32) of torch's bicubic with align_corners=True."""
    src = np.arange(n_dst, dtype=np.float64) * (np.float64(n_src - 1) / np.float64(n_dst - 1)) if n_dst > 1 else np.zeros(1)
    i0 = np.floor(src)
    t = src - i0
    A = CUBIC_A

    def inner(x):           # |x| <= 1
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

    def outer(x):           # 1 < |x| < 2
        return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A

    coef = np.stack([outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t)], axis=1).astype(np.float32)
    idx = np.clip(i0.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_src - 1)
    return idx, coef


def reflect(i, n):
    """Reflect border without repeating the edge (-1 -> 1, n -> n - 2), then clamped into the image."""
    i = np.where(i < 0, -i, i)
    i = np.where(i >= n, 2 * (n - 1) - i, i)
    return np.clip(i, 0, n - 1)


def _weighted(taps, values):
    """sum_k taps[k] * values[k] in fp32, every product and every sum rounded on its own, from the first tap on."""
    acc = None
    for w, v in zip(taps, values):
        term = (w * v).astype(np.float32)
        acc = term if acc is None else (acc + term).astype(np.float32)
    return acc


def blurs(h, w, antialias=True):
    return bool(antialias) and max(h, w) > SIZE           # max(f_h, f_w) > 1


def preprocess(x, antialias=True):
    """(B, 3, H, W) fp32 in [-1, 1] -> (image (B, 3, 224, 224) fp32, patch matrix (B 256, 592) fp32 with columns 588 .. 591 zero)."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    b, c, h, w = x.shape
    assert c == 3
    if blurs(h, w, antialias):
        gx, gy = blur_taps(w), blur_taps(h)
        xs = [reflect(np.arange(w) + k - len(gx) // 2, w) for k in range(len(gx))]
        x = _weighted(gx, [x[:, :, :, s] for s in xs])                             # along x first
        ys = [reflect(np.arange(h) + k - len(gy) // 2, h) for k in range(len(gy))]
        x = _weighted(gy, [x[:, :, s, :] for s in ys])
    ix, cx = cubic_taps(w)
    iy, cy = cubic_taps(h)
    x = _weighted([cx[None, None, None, :, k] for k in range(4)], [x[:, :, :, ix[:, k]] for k in range(4)])      # (B, 3, H, 224)
    x = _weighted([cy[None, None, :, None, k] for k in range(4)], [x[:, :, iy[:, k], :] for k in range(4)])      # (B, 3, 224, 224)
    x = ((x + np.float32(1)).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    x = ((x - MEAN[None, :, None, None]).astype(np.float32) / STD[None, :, None, None]).astype(np.float32)
    return x, patches_of(x)


def patches_of(image):
    """(B, 3, 224, 224) -> (B 256, 592): row (b, 16 gy + gx), column c 196 + 14 py + px, four zero columns."""
    image = np.asarray(image)
    b = image.shape[0]
    p = image.reshape(b, 3, GRID, PATCH, GRID, PATCH).transpose(0, 2, 4, 1, 3, 5).reshape(b * GRID * GRID, K)
    return np.concatenate([p, np.zeros((p.shape[0], KPAD - K), dtype=image.dtype)], axis=1)


def preprocess_f64(x, antialias=True):
    """The same rule through torch's own operators in float64: conv2d with the Gaussian taps on a reflect-padded input, then
    interpolate(bicubic, align_corners=True), then the normalisation."""
    import torch.nn.functional as Fn
    x = torch.as_tensor(np.asarray(x), dtype=F64)
    h, w = x.shape[-2:]
    if blurs(h, w, antialias):
        gy, gx = (torch.from_numpy(blur_taps(n).astype(np.float64)) for n in (h, w))
        ry, rx = len(gy) // 2, len(gx) // 2
        x = Fn.pad(x, (rx, rx, ry, ry), mode="reflect")
        x = Fn.conv2d(x, gx.reshape(1, 1, 1, -1).repeat(3, 1, 1, 1), groups=3)
        x = Fn.conv2d(x, gy.reshape(1, 1, -1, 1).repeat(3, 1, 1, 1), groups=3)
    x = Fn.interpolate(x, size=(SIZE, SIZE), mode="bicubic", align_corners=True)
    x = (x + 1.0) / 2.0
    return (x - torch.from_numpy(MEAN.astype(np.float64))[None, :, None, None]) / torch.from_numpy(STD.astype(np.float64))[None, :, None, None]


def preprocess_bound(x, antialias=True):
    """Bound on |preprocess - preprocess_f64| computed from the tables: a chain of roundings each at most 2^-24 of a magnitude that never
    exceeds (product of the stages' sum |taps|) * max|x| (+ 1 for the normalisation), divided by the smallest std.  Roundings: per
    weighted sum of k taps, k products and k - 1 sums; the coefficient tables themselves are fp32 roundings of the float64 ones (one
    more per tap); four for the normalisation."""
    x = np.asarray(x)
    h, w = x.shape[-2:]
    stages = []
    if blurs(h, w, antialias):
        stages += [blur_taps(w)[None, :], blur_taps(h)[None, :]]
    stages += [cubic_taps(w)[1], cubic_taps(h)[1]]
    gain, roundings = 1.0, 0
    for taps in stages:
        gain *= float(np.abs(taps.astype(np.float64)).sum(axis=1).max())
        roundings += 3 * taps.shape[1] - 1
    roundings += 4
    return gain * (float(np.abs(x).max()) + 1.0) * roundings * 2.0 ** -24 / float(STD.min())


# ------------------------------------------------------------------------------------------------ attention
def short_attention(qkv, *, batch, heads, n, d, scale=None, round_to=None, dtype=F64):
    """qkv [batch n][>= 3 heads d] -> O [batch n][heads d] in fp64: q of head h at columns [h d, h d + d), k at C + h d, v at 2 C + h d.
    round_to (attention_reference.through): q, k, v rounded once; s = (q k^T) c with c = scale log2(e); m = max_j s; p = 2^(s - m);
    l = sum p (unrounded); O = through((through(p) v) / l)."""
    rt = through(round_to, dtype)
    c_all = heads * d
    scale = d ** -0.5 if scale is None else scale
    # the unrounded definition takes the exact constant; the emulation the kernel's fp32 one
    c2 = scale * LOG2E if round_to is None else float(np.float32(np.float32(scale) * np.float32(LOG2E)))
    x = rt(qkv[:, :3 * c_all].to(dtype)).reshape(batch, n, 3, heads, d).permute(2, 0, 3, 1, 4)             # [3][b][h][n][d]
    s = (x[0] @ x[1].transpose(-1, -2)) * c2
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)
    o = (rt(p) @ x[2]) / p.sum(dim=-1, keepdim=True)
    return rt(o.permute(0, 2, 1, 3).reshape(batch * n, c_all))


# ------------------------------------------------------------------------------------------------ the tower
def layer_norm(x, w, b, eps=1e-5):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def tower(params, image=None, *, patches=None, heads, round_to=None, dtype=F64):
    """The transformer's tokens (B, 257, width) in fp64 from the normalised image (B, 3, 224, 224) or its patch matrix (B 256, >= 588).
    params: open_clip's keys under `model.visual.` (conv1.weight, class_embedding, positional_embedding, ln_pre.*, transformer.resblocks.
    {i}.ln_1 / attn.in_proj_* / attn.out_proj.* / ln_2 / mlp.c_fc / mlp.c_proj).  round_to: every MFMA operand — GEMM inputs, weights,
    q, k, v, P, O — passes through that operand storage; sums, biases, norms and the residual stream stay in fp64."""
    rt = through(round_to, dtype)
    P = {k: v.to(dtype) for k, v in params.items()}
    if patches is None:
        patches = torch.from_numpy(patches_of(np.asarray(image)))
    patches = torch.as_tensor(patches)[:, :K].to(dtype)
    width = P["conv1.weight"].shape[0]
    b = patches.shape[0] // (GRID * GRID)
    d = width // heads

    def lin(x, w, bias=None):
        y = rt(x) @ rt(w).t()
        return y if bias is None else y + bias

    x = lin(patches, P["conv1.weight"].reshape(width, K)).reshape(b, GRID * GRID, width)
    x = torch.cat([P["class_embedding"].expand(b, 1, width), x], 1) + P["positional_embedding"]
    x = layer_norm(x, P["ln_pre.weight"], P["ln_pre.bias"]).reshape(b * 257, width)
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in P:
        pre = f"transformer.resblocks.{i}."
        h = layer_norm(x, P[pre + "ln_1.weight"], P[pre + "ln_1.bias"])
        qkv = lin(h, P[pre + "attn.in_proj_weight"], P[pre + "attn.in_proj_bias"])
        att = short_attention(qkv, batch=b, heads=heads, n=257, d=d, round_to=round_to, dtype=dtype)
        x = x + lin(att, P[pre + "attn.out_proj.weight"], P[pre + "attn.out_proj.bias"])
        h = layer_norm(x, P[pre + "ln_2.weight"], P[pre + "ln_2.bias"])
        hid = gelu(lin(h, P[pre + "mlp.c_fc.weight"], P[pre + "mlp.c_fc.bias"]))
        x = x + lin(hid, P[pre + "mlp.c_proj.weight"], P[pre + "mlp.c_proj.bias"])
        i += 1
    return x.reshape(b, 257, width)


def visual_shapes(width, layers, heads, mlp_ratio=4.0, embed_dim=1024, patch=PATCH, tokens=257):
    """open_clip's VisionTransformer keys (relative to `model.visual.`) and shapes."""
    mlp = int(width * mlp_ratio)
    s = {"conv1.weight": (width, 3, patch, patch), "class_embedding": (width,), "positional_embedding": (tokens, width),
         "ln_pre.weight": (width,), "ln_pre.bias": (width,), "ln_post.weight": (width,), "ln_post.bias": (width,), "proj": (width, embed_dim)}
    for i in range(layers):
        pre = f"transformer.resblocks.{i}."
        s.update({pre + "ln_1.weight": (width,), pre + "ln_1.bias": (width,), pre + "ln_2.weight": (width,), pre + "ln_2.bias": (width,),
                  pre + "attn.in_proj_weight": (3 * width, width), pre + "attn.in_proj_bias": (3 * width,),
                  pre + "attn.out_proj.weight": (width, width), pre + "attn.out_proj.bias": (width,),
                  pre + "mlp.c_fc.weight": (mlp, width), pre + "mlp.c_fc.bias": (mlp,),
                  pre + "mlp.c_proj.weight": (width, mlp), pre + "mlp.c_proj.bias": (width,)})
    return s
