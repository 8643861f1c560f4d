"""The image tower without a GPU: the CPU definitions of tests/clip_reference.py against independent implementations (the
CLIPVisionModel fixture, torch's scaled_dot_product_attention, conv2d + interpolate in float64), the preprocessing rule's properties,
the module tree's state-dict keys, the shim, the C-ABI's rejections and the generated code's scratch use."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import clip_reference as cr
from helpers import GOLDEN, golden, rel_l2, seeded_sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (d, N) of tests/test_towers_gpu.py: one key, below and just past a 32-key boundary, the real tower, the second width
ATTN_SHAPES = [(80, 1), (80, 17), (80, 33), (80, 257), (64, 77)]
ATTN_B, ATTN_HEADS = 2, 2
# (B, H, W) of the preprocessing cases of the GPU file
PRE_SHAPES = [(2, 36, 64), (1, 320, 512), (1, 576, 1024), (1, 224, 224), (1, 100, 300)]


def attn_qkv(d, n, seed=0, gap=0):
    g = torch.Generator().manual_seed(1000 * d + n + seed)
    return torch.randn((ATTN_B * n, 3 * ATTN_HEADS * d + gap), generator=g)


def pre_image(shape):
    b, h, w = shape
    rng = np.random.default_rng(h * 4099 + w)
    return rng.uniform(-1.0, 1.0, size=(b, 3, h, w)).astype(np.float32)


def test_reference_tower_matches_the_clip_vision_model_fixture():
    g = golden("clip_tower.pt")
    sd = seeded_sd(g["param_shapes"], g["seed"], g["checksum"])
    got = cr.tower(sd, g["image"].float().numpy(), heads=g["config"]["heads"])
    err = rel_l2(got, g["tokens"])
    print(f"clip_reference.tower against the CLIPVisionModel tokens (fp32 storage): rel-L2 {err:.3e}")
    assert got.shape == g["tokens"].shape == (2, 257, 160) and err <= 1e-6


@pytest.mark.parametrize("d,n", ATTN_SHAPES)
def test_reference_short_attention_is_scaled_dot_product_attention(d, n):
    qkv = attn_qkv(d, n).double()
    got = cr.short_attention(qkv, batch=ATTN_B, heads=ATTN_HEADS, n=n, d=d)
    q, k, v = (t.reshape(ATTN_B, n, ATTN_HEADS, d).transpose(1, 2) for t in qkv.chunk(3, dim=1))
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(ATTN_B * n, ATTN_HEADS * d)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


@pytest.mark.parametrize("shape,antialias", [(s, True) for s in PRE_SHAPES] + [((1, 320, 512), False), ((1, 100, 300), False)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fp32_preprocessing_is_torchs_operators_within_the_computed_bound(shape, antialias):
    x = pre_image(shape)
    image, patches = cr.preprocess(x, antialias)
    want = cr.preprocess_f64(x, antialias)
    err = float((torch.from_numpy(image).double() - want).abs().max())
    bound = cr.preprocess_bound(x, antialias)
    print(f"preprocess {shape} antialias={antialias}: max |fp32 - fp64| {err:.3e}, bound {bound:.3e}")
    assert image.shape == (shape[0], 3, 224, 224) and image.dtype == np.float32 and err <= bound
    assert patches.shape == (shape[0] * 256, 592) and not patches[:, 588:].any()
    # row (b, 16 gy + gx), column c 196 + 14 py + px
    assert patches[(shape[0] - 1) * 256 + 16 * 3 + 5, 2 * 196 + 14 * 7 + 9] == image[shape[0] - 1, 2, 3 * 14 + 7, 5 * 14 + 9]


def test_preprocessing_properties():
    for n in (36, 64, 100, 224, 300, 320, 512, 576, 1024):
        assert abs(float(cr.blur_taps(n).astype(np.float64).sum()) - 1.0) <= 2.0 ** -22, n
        assert float(np.abs(cr.cubic_taps(n)[1].astype(np.float64).sum(1) - 1.0).max()) <= 2.0 ** -22, n
        idx = cr.cubic_taps(n)[0]
        assert idx.min() == 0 and idx.max() == n - 1
    assert (len(cr.blur_taps(576)), len(cr.blur_taps(1024))) == (3, 7) and (len(cr.blur_taps(320)), len(cr.blur_taps(512))) == (3, 3)
    assert cr.blurs(576, 1024) and cr.blurs(100, 300) and not cr.blurs(224, 224) and not cr.blurs(36, 64) and not cr.blurs(576, 1024, False)
    assert cr.reflect(np.array([-1, -2, 5, 6]), 5).tolist() == [1, 2, 3, 2]
    # 224 x 224 in: the normalisation alone, exactly
    x = pre_image((1, 224, 224))
    want = ((x + np.float32(1)) * np.float32(0.5) - cr.MEAN[None, :, None, None]) / cr.STD[None, :, None, None]
    assert want.dtype == np.float32 and np.array_equal(cr.preprocess(x)[0], want)
    # an all-zero image: (0.5 - mean_c) / std_c exactly, at a size that blurs
    zero = cr.preprocess(np.zeros((1, 3, 320, 512), dtype=np.float32))[0]
    for c in range(3):
        assert (zero[0, c] == (np.float32(0.5) - cr.MEAN[c]) / cr.STD[c]).all()


def _tower(**kw):
    from mudg_amd.towers import FrozenOpenCLIPImageEmbedderV2
    with torch.device("meta"):
        return FrozenOpenCLIPImageEmbedderV2(**kw)


def test_state_dict_keys_at_the_real_configuration():
    with open(os.path.join(GOLDEN, "clip_keys.json")) as f:
        want = json.load(f)
    tower = _tower()
    got = {k: list(v.shape) for k, v in tower.state_dict().items()}
    assert got == want, (sorted(set(got) ^ set(want))[:8])
    assert "mean" not in got and tower.mean.shape == (3,) and not any(p.requires_grad for p in tower.parameters())
    assert sum(p.numel() for p in tower.model.visual.parameters()) == 632076800          # ViT-H/14 with its 1280 x 1024 projection
    assert set(k for k in _tower(text_leftovers=False).state_dict()) == {k for k in want if k.startswith("model.visual.")}
    with pytest.raises(NotImplementedError):
        _tower(layer="penultimate")


def test_a_checkpoints_entries_load_strictly():
    from mudg_amd.towers import FrozenOpenCLIPImageEmbedderV2
    g = golden("clip_tower.pt")
    cfg = g["config"]
    tower = FrozenOpenCLIPImageEmbedderV2(width=cfg["width"], layers=cfg["layers"], heads=cfg["heads"], embed_dim=cfg["embed_dim"], text_leftovers=False)
    sd = {"model.visual." + k: v for k, v in seeded_sd(g["param_shapes"], g["seed"], g["checksum"]).items()}
    tower.load_state_dict(sd, strict=True)
    assert torch.equal(tower.model.visual.transformer.resblocks[1].attn.in_proj_weight, sd["model.visual.transformer.resblocks.1.attn.in_proj_weight"])
    with pytest.raises(RuntimeError, match="GPU"):
        tower(torch.zeros(1, 3, 32, 32))


def test_the_shim_resolves_both_towers_from_mudg_amd(monkeypatch):
    import lvdm.modules.encoders.condition as cond
    from test_host_logic import _yaml_model
    from utils.utils import instantiate_from_config
    monkeypatch.setenv("MUDG_CONDITION_MODULE", "mudg_amd.towers")
    monkeypatch.delenv("MUDG_REFERENCE", raising=False)
    monkeypatch.delenv("MUDG_TEXT_EMBEDDINGS", raising=False)
    monkeypatch.setattr(cond, "_external", None)
    params = _yaml_model("1024")["params"]
    with torch.device("meta"):
        image_tower = instantiate_from_config(params["img_cond_stage_config"])
        text_tower = instantiate_from_config(params["cond_stage_config"])
    assert type(image_tower).__module__ == "mudg_amd.towers" and type(image_tower).__name__ == "FrozenOpenCLIPImageEmbedderV2"
    assert image_tower.model.visual.positional_embedding.shape == (257, 1280) and image_tower.antialias is True
    assert type(text_tower).__module__ == "mudg_amd.towers" and type(text_tower).__name__ == "FrozenOpenCLIPEmbedder"
    monkeypatch.setattr(cond, "_external", None)


def test_the_text_table_returns_the_stored_rows_and_names_a_missing_prompt(tmp_path, monkeypatch):
    from mudg_amd.towers import FrozenOpenCLIPEmbedder
    g = torch.Generator().manual_seed(5)
    table = {"A photo a of driving scene.": torch.randn(77, 32, generator=g), "": torch.randn(77, 32, generator=g)}
    monkeypatch.delenv("MUDG_TEXT_EMBEDDINGS", raising=False)
    tower = FrozenOpenCLIPEmbedder(freeze=True, layer="penultimate", arch="x", version="y", device="cpu", max_length=77, embeddings=table)
    out = tower.encode(["", "A photo a of driving scene.", ""])
    assert out.shape == (3, 77, 32) and torch.equal(out[0], table[""]) and torch.equal(out[1], table["A photo a of driving scene."])
    assert torch.equal(tower(["A photo a of driving scene."])[0], out[1]) and not tower.state_dict()
    with pytest.raises(KeyError, match="a street"):
        tower.encode(["", "a street"])
    path = tmp_path / "text.pt"
    torch.save(table, path)
    monkeypatch.setenv("MUDG_TEXT_EMBEDDINGS", str(path))
    assert torch.equal(FrozenOpenCLIPEmbedder().encode([""])[0], table[""])
    monkeypatch.delenv("MUDG_TEXT_EMBEDDINGS")
    with pytest.raises(KeyError, match="MUDG_TEXT_EMBEDDINGS"):
        FrozenOpenCLIPEmbedder().encode([""])


def test_the_new_entries_reject_bad_arguments_without_a_gpu():
    from mudg_amd import hip, ops
    lib = hip.lib()
    for name in ("mudg_short_attention", "mudg_short_attention_ok", "mudg_clip_preprocess", "mudg_layernorm_f32"):
        assert hasattr(lib, name), name

    def desc(**kw):
        base = dict(batch=2, heads=2, n=257, d=80, ldqkv=480, ldo=160 * hip.planes())
        base.update(kw)
        return ops.short_attention_desc(256, 256, **base)

    assert lib.mudg_short_attention_ok(ctypes.byref(desc())) == 1
    assert lib.mudg_short_attention_ok(ctypes.byref(desc(d=64, n=288, ldqkv=384, ldo=128 * hip.planes()))) == 1
    for bad, word in ((dict(n=289), b"tokens"), (dict(n=0), b"tokens"), (dict(d=48), b"head width"), (dict(ldqkv=479), b"ldqkv"),
                      (dict(ldo=152 * hip.planes()), b"ldo"), (dict(ldo=160 * hip.planes() + 4), b"ldo"), (dict(batch=0), b"B=")):
        assert lib.mudg_short_attention_ok(ctypes.byref(desc(**bad))) == 0, bad
        assert lib.mudg_short_attention(ctypes.byref(desc(**bad)), None) == -1, bad
        assert word in lib.mudg_last_error(), (bad, lib.mudg_last_error())
    assert lib.mudg_short_attention(ctypes.byref(ops.short_attention_desc(None, None, batch=2, heads=2, n=257, d=80, ldqkv=480, ldo=160 * hip.planes())), None) == -1
    assert b"null" in lib.mudg_last_error()
    assert lib.mudg_short_attention(None, None) == -1 and lib.mudg_short_attention_ok(None) == 0
    assert lib.mudg_layernorm_f32(None, 8, None, None, None, 8, 1, 8, 1e-5, None) == -1 and b"null" in lib.mudg_last_error()
    assert lib.mudg_clip_preprocess(None, 1, 8, 8, None, None, None, 0, None, 0, None, 592, None, None) == -1 and b"null" in lib.mudg_last_error()
    assert lib.mudg_clip_preprocess(256, 1, 8, 8, 256, 256, None, 3, None, 3, 256, 592 * hip.planes(), None, None) == -1 and b"blur" in lib.mudg_last_error()
    assert lib.mudg_clip_preprocess(256, 1, 8, 8, 256, 256, None, 0, None, 0, 256, 584 * hip.planes(), None, None) == -1 and b"ldp" in lib.mudg_last_error()


def test_the_tower_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    from mudg_amd import build
    seen = set()
    for extra in ([], ["-DMUDG_PLANES=2"]):
        cmd = [hipcc, *build.FLAGS, *extra, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(ROOT, "mudg_amd", "csrc", "towers.hip"), "-o", str(tmp_path / "towers.o")]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stderr
        for name, scratch in re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, re.S):
            for family in ("short_attn_kernel", "clip_preprocess_kernel", "ln_f32_kernel"):
                if family in name:
                    seen.add((family, tuple(extra)))
                    assert int(scratch) == 0, (name, extra, scratch)
    assert len(seen) == 6, seen
