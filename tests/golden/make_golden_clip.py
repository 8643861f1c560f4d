"""Fixtures of the image tower: tests/golden/clip_tower.pt and tests/golden/clip_keys.json.

clip_tower.pt comes from `transformers.CLIPVisionModel` on the CPU in float64 — an implementation independent of this package and of
tests/clip_reference.py — at width 160, 2 heads of 80, 2 layers, 224 x 224 images in 14 x 14 patches (257 tokens), B = 2.  The weights are
seeded (tests/golden/seeding.py) under open_clip's key names and copied into the Hugging Face layout (q | k | v split out of in_proj);
only the normalised input image (stored as the fp16 numbers it was drawn as: exact), the tokens before post_layernorm (fp32), the
parameter shapes and the checksum are kept.

clip_keys.json is the state-dict key list (with shapes) of FrozenOpenCLIPImageEmbedderV2 at the real ViT-H/14 configuration, written
from knowledge of open_clip: it has not been compared with an open_clip installation.

    python tests/golden/make_golden_clip.py
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import clip_reference as cr          # noqa: E402  (the key / shape list, and the cross-check of its tower)

SEED = 1717
CFG = {"width": 160, "heads": 2, "layers": 2, "mlp_ratio": 4.0, "embed_dim": 64, "batch": 2}


def hf_model(sd, cfg):
    from transformers import CLIPVisionConfig, CLIPVisionModel
    w = cfg["width"]
    conf = CLIPVisionConfig(hidden_size=w, intermediate_size=int(w * cfg["mlp_ratio"]), num_hidden_layers=cfg["layers"],
                            num_attention_heads=cfg["heads"], image_size=224, patch_size=14, hidden_act="gelu", layer_norm_eps=1e-5,
                            attention_dropout=0.0, projection_dim=cfg["embed_dim"])
    conf._attn_implementation = "sdpa"          # the eager path takes its softmax in float32 whatever the model's dtype
    model = CLIPVisionModel(conf).double().eval()
    vm = getattr(model, "vision_model", model)          # newer transformers hold the tower's modules on the model itself
    with torch.no_grad():
        vm.embeddings.patch_embedding.weight.copy_(sd["conv1.weight"])
        vm.embeddings.class_embedding.copy_(sd["class_embedding"])
        vm.embeddings.position_embedding.weight.copy_(sd["positional_embedding"])
        vm.pre_layrnorm.weight.copy_(sd["ln_pre.weight"]); vm.pre_layrnorm.bias.copy_(sd["ln_pre.bias"])
        for i, layer in enumerate(vm.encoder.layers):
            pre = f"transformer.resblocks.{i}."
            wq, wk, wv = sd[pre + "attn.in_proj_weight"].chunk(3, 0)
            bq, bk, bv = sd[pre + "attn.in_proj_bias"].chunk(3, 0)
            for lin, wt, bs in ((layer.self_attn.q_proj, wq, bq), (layer.self_attn.k_proj, wk, bk), (layer.self_attn.v_proj, wv, bv),
                                (layer.self_attn.out_proj, sd[pre + "attn.out_proj.weight"], sd[pre + "attn.out_proj.bias"]),
                                (layer.mlp.fc1, sd[pre + "mlp.c_fc.weight"], sd[pre + "mlp.c_fc.bias"]),
                                (layer.mlp.fc2, sd[pre + "mlp.c_proj.weight"], sd[pre + "mlp.c_proj.bias"])):
                lin.weight.copy_(wt); lin.bias.copy_(bs)
            layer.layer_norm1.weight.copy_(sd[pre + "ln_1.weight"]); layer.layer_norm1.bias.copy_(sd[pre + "ln_1.bias"])
            layer.layer_norm2.weight.copy_(sd[pre + "ln_2.weight"]); layer.layer_norm2.bias.copy_(sd[pre + "ln_2.bias"])
    return model


def real_keys():
    keys = {"model.visual." + k: list(v) for k, v in cr.visual_shapes(1280, 32, 16, 4.0, 1024).items()}
    keys.update({"model.positional_embedding": [77, 1024], "model.text_projection": [1024, 1024], "model.logit_scale": [],
                 "model.token_embedding.weight": [49408, 1024], "model.ln_final.weight": [1024], "model.ln_final.bias": [1024]})
    return keys


def main():
    from seeding import checksum, seeded_input, seeded_state_dict
    shapes = cr.visual_shapes(CFG["width"], CFG["layers"], CFG["heads"], CFG["mlp_ratio"], CFG["embed_dim"])
    sd = seeded_state_dict(shapes, SEED)
    image = seeded_input("clip_image", (CFG["batch"], 3, 224, 224), SEED).half()         # the numbers themselves are fp16: stored exactly
    with torch.no_grad():
        tokens = hf_model({k: v.double() for k, v in sd.items()}, CFG)(pixel_values=image.double()).last_hidden_state
        mine = cr.tower(sd, image.float().numpy(), heads=CFG["heads"])
    rel = float((mine - tokens).norm() / tokens.norm())
    print(f"clip_reference.tower against CLIPVisionModel in float64: rel-L2 {rel:.3e}")
    assert rel < 1e-12, rel
    torch.save({"image": image, "tokens": tokens.float(), "param_shapes": {k: list(v) for k, v in shapes.items()}, "checksum": checksum(sd),
                "seed": SEED, "config": CFG}, os.path.join(HERE, "clip_tower.pt"))
    with open(os.path.join(HERE, "clip_keys.json"), "w") as f:
        json.dump(real_keys(), f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
