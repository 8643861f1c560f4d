"""The two CLIP towers MuDG's configs name, for MUDG_CONDITION_MODULE=mudg_amd.towers (lvdm/modules/encoders/condition.py resolves
`FrozenOpenCLIPImageEmbedderV2` and `FrozenOpenCLIPEmbedder` from here).

FrozenOpenCLIPImageEmbedderV2 is the image tower (reference condition.py:295-372): a module tree that carries open_clip's state-dict
keys, so that a MuDG checkpoint's `embedder.*` entries load strictly, and whose forward runs on the HIP kernels (engine/clip.py).  It
imports neither open_clip nor kornia and downloads nothing: the weights come from the checkpoint.  The key list is written from
knowledge of open_clip's VisionTransformer and CLIP classes and has not been compared with an open_clip installation.

FrozenOpenCLIPEmbedder is the text side as a TABLE: the model's prompts are two constant strings per run, so their (77, dim) rows are
looked up, never computed — the text transformer and its BPE vocabulary are not part of this package."""
from __future__ import annotations

import os
from collections import OrderedDict

import torch
import torch.nn as nn

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)          # condition.py:318-319
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
TEXT_EMBEDDINGS_ENV = "MUDG_TEXT_EMBEDDINGS"


class AbstractEncoder(nn.Module):
    def encode(self, *args, **kwargs):
        raise NotImplementedError


class _ResidualAttentionBlock(nn.Module):
    def __init__(self, width, heads, mlp_width):
        super().__init__()
        self.ln_1 = nn.LayerNorm(width)
        self.attn = nn.MultiheadAttention(width, heads)                  # in_proj_weight, in_proj_bias, out_proj.*
        self.ln_2 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(width, mlp_width)), ("gelu", nn.GELU()), ("c_proj", nn.Linear(mlp_width, width))]))


class _Transformer(nn.Module):
    def __init__(self, width, layers, heads, mlp_width):
        super().__init__()
        self.resblocks = nn.ModuleList([_ResidualAttentionBlock(width, heads, mlp_width) for _ in range(layers)])


class _VisionTransformer(nn.Module):
    def __init__(self, image_size, patch_size, width, layers, heads, mlp_ratio, output_dim):
        super().__init__()
        self.input_patchnorm = False
        self.grid_size = (image_size // patch_size, image_size // patch_size)
        self.patch_size = (patch_size, patch_size)
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn(self.grid_size[0] * self.grid_size[1] + 1, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = _Transformer(width, layers, heads, int(width * mlp_ratio))
        self.ln_post = nn.LayerNorm(width)                               # in the checkpoint, unused: the tokens leave before it
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))


class _Clip(nn.Module):
    """What the reference keeps of open_clip's CLIP after `del model.transformer`: the vision tower and, unused, the text side's
    parameters outside its transformer."""

    def __init__(self, visual, embed_dim, text_leftovers):
        super().__init__()
        self.visual = visual
        if text_leftovers:
            self.positional_embedding = nn.Parameter(torch.zeros(77, embed_dim))
            self.text_projection = nn.Parameter(torch.zeros(embed_dim, embed_dim))
            self.logit_scale = nn.Parameter(torch.zeros(()))
            self.token_embedding = nn.Embedding(49408, embed_dim)
            self.ln_final = nn.LayerNorm(embed_dim)


class FrozenOpenCLIPImageEmbedderV2(AbstractEncoder):
    """The OpenCLIP ViT-H/14 image encoder: (B, 3, H, W) in [-1, 1] -> (B, 257, 1280), the transformer's tokens."""

    def __init__(self, arch="ViT-H-14", version="laion2b_s32b_b79k", device="cuda", freeze=True, layer="pooled", antialias=True, *,
                 width=1280, layers=32, heads=16, mlp_ratio=4.0, patch_size=14, image_size=224, embed_dim=1024, text_leftovers=True):
        super().__init__()
        if width % heads:
            raise ValueError(f"image tower: width {width} is not a whole number of {heads} heads")
        self.arch, self.version = arch, version
        self.model = _Clip(_VisionTransformer(image_size, patch_size, width, layers, heads, mlp_ratio, embed_dim), embed_dim, text_leftovers)
        self.device = device
        if freeze:
            self.freeze()
        self.layer = layer
        if self.layer == "penultimate":
            raise NotImplementedError()
        self.antialias = antialias
        self.register_buffer("mean", torch.Tensor(CLIP_MEAN), persistent=False)
        self.register_buffer("std", torch.Tensor(CLIP_STD), persistent=False)

    def freeze(self):
        self.model = self.model.eval()
        for param in self.model.parameters():
            param.requires_grad = False

    def preprocess(self, x):
        """The normalised 224 x 224 image (inspection; the forward pass writes the patch matrix directly)."""
        from . import ops
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError("image tower: inputs must be on the GPU; the MI355X path has no CPU fallback")
        return ops.clip_preprocess(x.detach().float().contiguous(), antialias=self.antialias, return_image=True)[1]

    def forward(self, image, no_dropout=False):
        return self.encode_with_vision_transformer(image)

    def encode_with_vision_transformer(self, x):
        from .engine import clip
        return clip.forward(self, x)

    def encode(self, image):
        return self(image)


class FrozenOpenCLIPEmbedder(AbstractEncoder):
    """The text tower as a table: encode(list of prompts) -> (b, 77, dim) rows looked up by prompt.  The table is `embeddings` (dict
    prompt -> (77, dim) tensor) or the torch.save'd dict named by MUDG_TEXT_EMBEDDINGS; a prompt that is not in it raises.  The reference's
    other constructor arguments are accepted and ignored."""

    def __init__(self, arch="ViT-H-14", version="laion2b_s32b_b79k", device="cuda", max_length=77, freeze=True, layer="last", embeddings=None):
        super().__init__()
        self.max_length, self.layer = max_length, layer
        if embeddings is None and os.environ.get(TEXT_EMBEDDINGS_ENV):
            embeddings = torch.load(os.environ[TEXT_EMBEDDINGS_ENV], map_location="cpu", weights_only=True)
        self.prompts = []
        for i, (prompt, rows) in enumerate((embeddings or {}).items()):
            if not isinstance(prompt, str) or not torch.is_tensor(rows) or rows.dim() != 2:
                raise ValueError(f"text table: entry {prompt!r} is not prompt -> (tokens, dim) tensor")
            self.prompts.append(prompt)
            self.register_buffer(f"rows_{i}", rows.detach().clone().float(), persistent=False)      # moves with the module

    def freeze(self):
        return self

    def forward(self, text):
        text = [text] if isinstance(text, str) else list(text)
        out = []
        for prompt in text:
            if prompt not in self.prompts:
                raise KeyError(f"text table: no embedding for the prompt {prompt!r} (known: {self.prompts}); pass embeddings= or set "
                               f"{TEXT_EMBEDDINGS_ENV} to a torch.save'd dict prompt -> (77, dim) tensor — the text transformer is not built")
            out.append(getattr(self, f"rows_{self.prompts.index(prompt)}"))
        return torch.stack(out)

    def encode(self, text):
        return self(text)
