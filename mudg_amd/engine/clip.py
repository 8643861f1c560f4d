"""The CLIP image tower on the gfx950 kernels (reference: lvdm/modules/encoders/condition.py:322-372, open_clip's pre-LN
VisionTransformer).

(B, 3, H, W) in [-1, 1] -> preprocessing straight into the patch matrix (csrc/towers.hip) -> patch GEMM whose fp32 residual carries
positional_embedding[1:] -> ln_pre into the fp32 residual stream -> per block
    x += out_proj(short_attention(in_proj(ln_1(x)) + in_proj_bias)) + out_proj_bias
    x += c_proj(gelu(c_fc(ln_2(x)) + b)) + b
-> (B, tokens, width) fp32, the transformer's output without ln_post and proj.  Rows are (image, token) with channels contiguous;
every GEMM operand is an MFMA operand matrix, the stream stays fp32.  Weights are packed once (engine/packing.py)."""
import torch

from .. import ops
from . import packing as pk


def _patch_weight(conv1):
    w = conv1.weight
    pk._need_cuda(w, "conv1")

    def build():
        flat = w.detach().float().reshape(w.shape[0], -1)                   # [width][c * 196 + 14 py + px]
        return pk.operand(torch.nn.functional.pad(flat, (0, ops.CLIP_KPAD - flat.shape[1])))

    return pk.cached(conv1, "wpatch", (w,), build)


def check_geometry(visual):
    """The preprocessing kernel writes 224 x 224 images as 16 x 16 patches of 14 x 14: any other tower geometry is an error."""
    w = visual.conv1.weight
    tokens = visual.positional_embedding.shape[0]
    if tuple(w.shape[1:]) != (3, ops.CLIP_PATCH, ops.CLIP_PATCH) or tokens != 257:
        raise RuntimeError(f"image tower: conv1 {tuple(w.shape)} / {tokens} tokens; the HIP path implements 224 x 224 images in 14 x 14 patches "
                           "(257 tokens)")


def block(blk, x, b, heads, n, d):
    """One residual attention block on the fp32 stream x [b n][width] (ls_1 and ls_2 are identities)."""
    attn = blk.attn
    h = ops.layernorm(x, pk.f32(blk.ln_1, "weight"), pk.f32(blk.ln_1, "bias"), eps=blk.ln_1.eps)
    w_in = pk.cached(attn, "in_proj", (attn.in_proj_weight,), lambda: pk.operand(attn.in_proj_weight.detach()))
    qkv = ops.gemm(h, w_in, bias=pk.f32(attn, "in_proj_bias"), out_fp32=True)
    att = ops.short_attention(qkv, batch=b, heads=heads, n=n, d=d)
    x = ops.gemm(att, pk.linear(attn.out_proj), bias=pk.f32(attn.out_proj, "bias"), residual=x, out_fp32=True)
    h = ops.layernorm(x, pk.f32(blk.ln_2, "weight"), pk.f32(blk.ln_2, "bias"), eps=blk.ln_2.eps)
    hid = ops.gemm(h, pk.linear(blk.mlp.c_fc), bias=pk.f32(blk.mlp.c_fc, "bias"), gelu=True)
    return ops.gemm(hid, pk.linear(blk.mlp.c_proj), bias=pk.f32(blk.mlp.c_proj, "bias"), residual=x, out_fp32=True)


@torch.no_grad()
def forward(tower, image):
    if not torch.is_tensor(image) or not image.is_cuda:
        raise RuntimeError("image tower: inputs must be on the GPU; the MI355X path has no CPU fallback")
    check_geometry(tower.model.visual)
    if image.dim() != 4 or image.shape[1] != 3:
        raise RuntimeError(f"image tower: expected (B, 3, H, W) images, got {tuple(image.shape)}")
    patches = ops.clip_preprocess(image.detach().float().contiguous(), antialias=tower.antialias)
    return forward_patches(tower, patches)


@torch.no_grad()
def forward_patches(tower, patches):
    """The tokens from the patch matrix of the normalised images, operand rows [B 256][592] (what ops.clip_preprocess writes)."""
    if not torch.is_tensor(patches) or not patches.is_cuda:
        raise RuntimeError("image tower: inputs must be on the GPU; the MI355X path has no CPU fallback")
    v = tower.model.visual
    check_geometry(v)
    if patches.dim() != 2 or patches.shape[0] % 256 or patches.shape[1] != ops.CLIP_KPAD:
        raise RuntimeError(f"image tower: the patch matrix is operand rows [B 256][{ops.CLIP_KPAD}], got {tuple(patches.shape)}")
    b, dev = patches.shape[0] // 256, patches.device
    width = v.conv1.weight.shape[0]
    heads = v.transformer.resblocks[0].attn.num_heads
    n, d = v.positional_embedding.shape[0], width // heads
    pos = v.positional_embedding
    pk._need_cuda(pos, "positional_embedding")
    # token rows before ln_pre: row 0 of an image is class_embedding + positional_embedding[0] (parameters only: packed once), rows 1 ..
    # the patch GEMM with positional_embedding[1:] as its fp32 residual, the same rows for every image (batch stride 0)
    cls = pk.cached(v, "cls_row", (v.class_embedding, pos), lambda: (v.class_embedding.detach().float() + pos.detach()[0].float()).contiguous())
    pos_rows = pk.cached(v, "pos_rows", (pos,), lambda: pos.detach()[1:].float().contiguous())
    x0 = torch.empty((b * n, width), dtype=torch.float32, device=dev)
    x0.view(b, n, width)[:, 0] = cls
    ops.gemm(patches, _patch_weight(v.conv1), out=x0[1:], residual=pos_rows, batch=b, M=n - 1, sx=(n - 1) * patches.stride(0), sy=n * width, sr=0)
    x = ops.layernorm_f32(x0, pk.f32(v.ln_pre, "weight"), pk.f32(v.ln_pre, "bias"), eps=v.ln_pre.eps)
    for blk in v.transformer.resblocks:
        x = block(blk, x, b, heads, n, d)
    return x.reshape(b, n, width)
