"""Training from a data batch on the GPU: LatentVisualDiffusion.get_batch_input / shared_step against what the REFERENCE's methods
gave for the same seeded batch (tests/golden/batch_input.pt, made by tests/golden/make_golden_batch.py: B = 4, the uniform draw
replaced by r = [0.02, 0.07, 0.12, 0.60] — text dropped, both dropped, image dropped, nothing dropped at uncond_prob 0.05), the
two kernels under it against their definitions, and the three-stream encode against stream-by-stream encodes.

No new bounds: the encodes are held to tests/test_pipeline_gpu.py's TOL_ENC (literal 1e-3 in bf16x3 / bf16x6), the image tokens to
that file's Resampler bound, the loss to test_latent_diffusion_forward_matches_the_reference_fixture's, the sampling arithmetic to
the 2e-6 of the existing gaussian_sample assertion."""
import pytest
import torch

from helpers import _load, golden, rel_l2, seeded_sd, seeding

from mudg_amd import hip as _hip

pytestmark = pytest.mark.gpu
MODE = _hip.operand_name()
TOL_ENC = {"bf16": 2e-2, "fp16": 3e-3, "bf16x3": 1e-3, "bf16x6": 1e-3}[MODE]                  # test_pipeline_gpu.py TOL_ENC
TOL_RESAMPLER = {"bf16": 1.5e-2, "fp16": 3e-3, "bf16x3": 1e-4, "bf16x6": 1e-5}[MODE]         # test_resampler_matches_reference
TOL_LOSS = {"bf16": 3e-2, "fp16": 5e-3, "bf16x3": 3e-4, "bf16x6": 3e-5}[MODE]                 # the training-forward fixture test
STREAMS = ("dense_frames", "sparse_frames", "sparse_depth")


def build_model(g, dev):
    from lvdm.models.ddpm3d import LatentVisualDiffusion
    from lvdm.modules.encoders.resampler import Resampler
    towers, towers_batch = _load("towers"), _load("towers_batch")
    ident = {"target": "torch.nn.Identity"}
    model = LatentVisualDiffusion(
        img_cond_stage_config=ident, image_proj_stage_config=ident, cond_stage_config=ident,
        first_stage_config={"target": "lvdm.models.autoencoder.AutoencoderKL",
                            "params": {"embed_dim": 4, "ddconfig": g["vae_ddconfig"], "lossconfig": ident}},
        unet_config={"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": g["unet_cfg"]},
        **g["diffusion_cfg"])
    model.model.diffusion_model.load_state_dict(seeded_sd(g["unet_param_shapes"], g["seed"], g["unet_checksum"]), strict=True)
    model.first_stage_model.load_state_dict(seeded_sd(g["vae_param_shapes"], g["seed"] + 1, g["vae_checksum"]), strict=True)
    d = g["driver"]
    model.image_proj_model = Resampler(**d["resampler"])
    model.image_proj_model.load_state_dict(seeded_sd(g["resampler_param_shapes"], g["seed"] + 5, g["resampler_checksum"]), strict=True)
    model.embedder = towers_batch.PerSampleImageTower(d["clip_tokens"], d["clip_dim"], d["tower_seed_img"])
    model.cond_stage_model = towers.FakeTextTower(g["unet_cfg"]["context_dim"], d["tower_seed_txt"], dev)
    return model.to(dev).eval()


def make_batch(g, dev, clips=None):
    """The batch make_golden_batch.py fed the reference, rebuilt from its seeds."""
    B, T, px = g["B"], g["unet_cfg"]["temporal_length"], g["driver"]["pixels"]
    clip = lambda name: seeding.seeded_input(name, (B, 3, T, px, px), g["input_seed"], 0.5).clamp(-1, 1).to(dev)
    batch = {"dense_frames": clip("bi_dense"), "sparse_frames": clip("bi_sparse"), "sparse_depth": clip("bi_depth"),
             "class_label": torch.tensor([0, 500, 1, 0], dtype=torch.long, device=dev)[:, None], "caption": ["a street"] * B,
             "fps": torch.full((B,), 10, dtype=torch.long, device=dev)}
    return batch


def replay_draw(model, g, dev, monkeypatch):
    monkeypatch.setattr(model, "_uncond_draw", lambda n, device: g["r"].to(device))


def test_get_batch_input_matches_the_reference_for_every_dropout_case(cuda, monkeypatch):
    towers, towers_batch = _load("towers"), _load("towers_batch")
    g = golden("batch_input.pt")
    model = build_model(g, cuda)
    batch = make_batch(g, cuda)
    d = g["driver"]
    text = towers.FakeTextTower(g["unet_cfg"]["context_dim"], d["tower_seed_txt"])
    null, prompts = text.encode([""])[0], text.encode(batch["caption"])
    # the Resampler's answer for each sample's real image and for an all-zero image, to tell the two apart below
    tokens = lambda zero: torch.stack([towers_batch.image_tokens(i, zero, d["clip_tokens"], d["clip_dim"], d["tower_seed_img"])
                                       for i in range(g["B"])]).to(cuda)
    with torch.no_grad():
        img_real, img_zero = model.image_proj_model(tokens(False)), model.image_proj_model(tokens(True))
    replay_draw(model, g, cuda, monkeypatch)
    for tag, uncond, text_dropped, image_dropped in (("dropout", True, (0, 1), (1, 2)), ("full", False, (), ())):
        want = g["outs"][tag]
        torch.manual_seed(g["cpu_seed"])
        with torch.no_grad():
            z, sparse_z, cond, fs, label = model.get_batch_input(batch, random_uncond=uncond, return_fs=True, return_class_label=True)
        cat, ctx = cond["c_concat"][0], cond["c_crossattn"][0]
        errs = {"z": rel_l2(z, want["z"]), "sparse_z": rel_l2(sparse_z, want["sparse_z"]), "c_concat": rel_l2(cat, want["c_concat"])}
        print(f"[{MODE}] get_batch_input ({tag}) rel-L2 vs the reference: " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items())
              + f"  (bound {TOL_ENC:g})")
        assert z.shape == want["z"].shape and cat.shape == want["c_concat"].shape and ctx.shape == want["c_crossattn"].shape
        assert all(v < TOL_ENC for v in errs.values()), errs
        assert sparse_z.data_ptr() == cat.data_ptr() and torch.equal(sparse_z, cat[:, :4])           # the view, not a copy
        assert torch.equal(fs.cpu(), want["fs"]) and torch.equal(label.cpu(), want["class_label"])
        for i in range(g["B"]):
            # text rows: the tower's output or the null prompt, bit for bit
            assert torch.equal(ctx[i, :77].cpu(), want["c_crossattn"][i, :77]), (tag, i)
            assert torch.equal(ctx[i, :77].cpu(), null if i in text_dropped else prompts[i]), (tag, i)
            # image rows: within the Resampler's bound of the reference, and those of the right image
            err = rel_l2(ctx[i, 77:], want["c_crossattn"][i, 77:])
            right, wrong = (img_zero, img_real) if i in image_dropped else (img_real, img_zero)
            print(f"[{MODE}]   sample {i}: image tokens rel-L2 vs the reference {err:.3e} (bound {TOL_RESAMPLER:g}); "
                  f"to the other image's tokens {rel_l2(ctx[i, 77:], wrong[i]):.3e}")
            assert err < TOL_RESAMPLER, (tag, i, err)
            assert rel_l2(ctx[i, 77:], right[i]) < TOL_RESAMPLER and rel_l2(ctx[i, 77:], wrong[i]) > 0.5, (tag, i)
    # the batch itself is not modified by the image dropout
    assert torch.equal(batch["sparse_frames"].cpu(), seeding.seeded_input("bi_sparse", tuple(batch["sparse_frames"].shape), g["input_seed"], 0.5).clamp(-1, 1))


def _noise(g, n, shape):
    torch.manual_seed(g["cpu_seed"])
    return torch.cat([torch.randn((1,) + shape) for _ in range(3 * n)], 0).reshape(3, n, *shape)


def test_posterior_assemble_is_fp32_exact_and_bit_equal_to_three_gaussian_samples(cuda):
    from mudg_amd import ops
    g = golden("batch_input.pt")
    B, T = g["B"], g["unet_cfg"]["temporal_length"]
    scale = g["diffusion_cfg"]["scale_factor"]
    moments = [g["moments"][k].to(cuda) for k in STREAMS]
    noise = _noise(g, B * T, (4, 8, 8)).to(cuda)
    z, cat = ops.posterior_assemble(*moments, noise, B, T, scale)
    want = g["outs"]["dropout"]
    e_z, e_c = rel_l2(z, want["z"]), rel_l2(cat, want["c_concat"])
    print(f"posterior_assemble on the reference's moments: z {e_z:.3e}  c_concat {e_c:.3e} (bound 2e-6)")
    assert e_z < 2e-6 and e_c < 2e-6

    def three_calls(moms, nz, b, t):
        parts = [ops.gaussian_sample(m, None if nz is None else nz[i], scale) for i, m in enumerate(moms)]
        parts = [p.reshape(b, t, *p.shape[1:]).permute(0, 2, 1, 3, 4) for p in parts]
        return parts[0].contiguous(), torch.cat(parts[1:], 1)

    z3, cat3 = three_calls(moments, noise, B, T)
    assert torch.equal(z, z3) and torch.equal(cat, cat3)
    # posterior mode (no noise), and a frame size that is no multiple of four values (the scalar form of the kernel)
    zm, catm = ops.posterior_assemble(*moments, None, B, T, scale)
    z3, cat3 = three_calls(moments, None, B, T)
    assert torch.equal(zm, z3) and torch.equal(catm, cat3)
    gen = torch.Generator().manual_seed(9)
    odd = [(torch.randn(6, 8, 3, 5, generator=gen) * 3).to(cuda) for _ in range(3)]
    nz = torch.randn(3, 6, 4, 3, 5, generator=gen).to(cuda)
    zo, cato = ops.posterior_assemble(*odd, nz, 2, 3, 0.5)
    z3, cat3 = [ops.gaussian_sample(m, nz[i], 0.5).reshape(2, 3, 4, 3, 5).permute(0, 2, 1, 3, 4) for i, m in enumerate(odd)], None
    assert torch.equal(zo, z3[0]) and torch.equal(cato, torch.cat(z3[1:], 1))
    with pytest.raises(_hip.MudgError):
        ops.posterior_assemble(*moments, noise[:, :-1].contiguous(), B, T, scale)


@pytest.mark.parametrize("shape", [(4, 77, 64, 3, 4, 16, 16), (3, 5, 7, 3, 2, 5, 3)])          # 16-byte form / scalar form
def test_cond_dropout_kernel_equals_the_reference_expressions(cuda, shape):
    from mudg_amd import ops
    b, l, dim, c, t, h, w = shape
    gen = torch.Generator().manual_seed(3)
    emb, null = torch.randn(b, l, dim, generator=gen).to(cuda), torch.randn(1, l, dim, generator=gen).to(cuda)
    clip = torch.randn(b, c, t, h, w, generator=gen).to(cuda)
    before = clip.clone()
    p = 0.05
    # every interval and its edges: r < p, p <= r < 2p, 2p <= r < 3p, r >= 3p
    for r in (torch.tensor([0.02, 0.07, 0.12, 0.60]), torch.tensor([0.05, 0.10, 0.15, 0.0]), torch.tensor([1.0, 1.0, 1.0, 1.0])):
        r = r[:b].to(cuda)
        prompt, img = ops.cond_dropout(r, p, emb, null, clip, 1)
        prompt_mask = (r < 2 * p)[:, None, None]
        input_mask = 1 - ((r >= p).float() * (r < 3 * p).float())[:, None, None, None]
        assert torch.equal(prompt, torch.where(prompt_mask, null, emb))
        assert torch.equal(img, input_mask * clip[:, :, 1])
    assert torch.equal(clip, before)


def test_three_stream_encode_is_bit_equal_to_stream_by_stream_encodes(cuda):
    from mudg_amd.engine import vae
    g = golden("batch_input.pt")
    model = build_model(g, cuda)
    batch = make_batch(g, cuda)
    flat = lambda x: x.permute(0, 2, 1, 3, 4).reshape(-1, x.shape[1], *x.shape[3:]).contiguous()
    ae = model.first_stage_model
    for clips in (g["B"], 1):                          # 16 frames per stream (whole frame batches) / 4 (a frame batch spans streams)
        streams = [batch[k][:clips] for k in STREAMS]
        joint = vae.encode_moments(ae, streams)
        for k, x, got in zip(STREAMS, streams, joint):
            alone = vae.encode_moments(ae, flat(x))
            assert got.shape == alone.shape and torch.equal(got, alone), (clips, k, rel_l2(got, alone))
            if clips == g["B"]:
                err = rel_l2(got, g["moments"][k])
                print(f"[{MODE}] moments of {k}: rel-L2 vs the reference {err:.3e} (bound {TOL_ENC:g})")
                assert err < TOL_ENC
    # 4-D streams take the same door
    joint4 = vae.encode_moments(ae, [flat(batch[k]) for k in STREAMS])
    assert all(torch.equal(a, b) for a, b in zip(joint4, vae.encode_moments(ae, [batch[k] for k in STREAMS])))


def _replay_forward(monkeypatch, g, dev):
    monkeypatch.setattr(torch, "randint", lambda *a, **k: g["t"].to(dev))
    monkeypatch.setattr(torch, "randn_like", lambda t_, **k: g["noise"].to(t_.device))


def test_shared_step_loss_matches_the_reference_and_only_the_trainable_parts_get_gradients(cuda, monkeypatch):
    g = golden("batch_input.pt")
    model = build_model(g, cuda)
    batch = make_batch(g, cuda)
    replay_draw(model, g, cuda, monkeypatch)
    _replay_forward(monkeypatch, g, cuda)

    def compare(loss, info, prefix):
        err = abs(float(loss) - float(g["loss"])) / abs(float(g["loss"]))
        print(f"[{MODE}] shared_step ({prefix}) loss {float(loss):.6f} vs the reference {float(g['loss']):.6f}: rel {err:.3e} (bound {TOL_LOSS:g})")
        assert err < TOL_LOSS
        assert set(info) == {k.replace("val/", prefix + "/") for k in g["loss_dict"]}
        for k, v in g["loss_dict"].items():
            mine = float(info[k.replace("val/", prefix + "/")])
            assert abs(mine - float(v)) < TOL_LOSS * abs(float(v)), (k, mine, float(v))

    # evaluation mode, as the reference ran it
    torch.manual_seed(g["cpu_seed"])
    compare(*_no_grad_shared_step(model, batch), "val")
    # training mode (dropout probability 0: the same function), with a graph
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    torch.manual_seed(g["cpu_seed"])
    loss, info = model.shared_step(batch, random_uncond=True)
    compare(loss.detach(), info, "train")
    loss.backward()
    proj = list(model.image_proj_model.parameters())
    assert proj and all(p.grad is not None and torch.isfinite(p.grad).all() for p in proj)
    assert sum(float(p.grad.abs().sum()) > 0 for p in proj) >= len(proj) - 1, "the Resampler sits inside the graph"
    assert all(p.grad is None for p in model.first_stage_model.parameters())
    assert all(p.grad is None for p in model.embedder.parameters()) and all(p.grad is None for p in model.cond_stage_model.parameters())
    unet = list(model.model.diffusion_model.parameters())
    assert all(p.grad is not None for p in unet if p.requires_grad)
    # training_step on a data batch is that same call
    torch.manual_seed(g["cpu_seed"])
    again = model.training_step(batch, 0)
    assert torch.equal(again.detach(), loss.detach())


def _no_grad_shared_step(model, batch):
    with torch.no_grad():
        return model.shared_step(batch, random_uncond=True)


def test_training_step_with_latents_is_the_p_losses_call_it_was(cuda, monkeypatch):
    """A batch that carries x_start takes the path training_step had before data batches existed: p_losses on the given tensors."""
    g = golden("batch_input.pt")
    model = build_model(g, cuda)
    want = g["outs"]["dropout"]
    cond = {"c_crossattn": [want["c_crossattn"].to(cuda)], "c_concat": [want["c_concat"].to(cuda)]}
    kw = dict(class_label=want["class_label"].to(cuda), fs=want["fs"].long().to(cuda))
    x, t, noise = want["z"].to(cuda), g["t"].to(cuda), g["noise"].to(cuda)
    monkeypatch.setattr(model, "shared_step", lambda *a, **k: pytest.fail("a latent batch must not go through shared_step"))
    with torch.no_grad():
        direct, _ = model.p_losses(x, cond, t, noise=noise, **kw)
        stepped = model.training_step(dict(x_start=x, cond=cond, t=t, noise=noise, **kw))
        stepped_idx = model.training_step(dict(x_start=x, cond=cond, t=t, noise=noise, **kw), 7)
    assert torch.equal(direct, stepped) and torch.equal(direct, stepped_idx)


class _DeviceImageTower(torch.nn.Module):
    def __init__(self, tokens, dim):
        super().__init__()
        self.tokens, self.dim = tokens, dim

    def forward(self, img):                      # a function of the image that never leaves the device
        return img.mean((1, 2, 3))[:, None, None].expand(img.shape[0], self.tokens, self.dim).contiguous()


class _DeviceTextTower(torch.nn.Module):
    def __init__(self, rows, null):
        super().__init__()
        self.rows, self.null = rows, null

    def encode(self, prompts):
        return self.null if len(prompts) == 1 and prompts[0] == "" else self.rows


def test_get_batch_input_never_reads_the_device_from_the_host(cuda):
    """The uniform draw, the masks and everything made from them stay on the device: under torch's synchronisation debug mode
    (an error on every blocking device-to-host or host-to-device operation) the whole method runs.  The posterior noise, drawn on
    the CPU generator as in the reference, is uploaded from page-locked memory without blocking, so no exemption is needed."""
    g = golden("batch_input.pt")
    model = build_model(g, cuda)
    batch = make_batch(g, cuda)
    d, dim = g["driver"], g["unet_cfg"]["context_dim"]
    gen = torch.Generator().manual_seed(1)
    model.embedder = _DeviceImageTower(d["clip_tokens"], d["clip_dim"])
    model.cond_stage_model = _DeviceTextTower(torch.randn(g["B"], 77, dim, generator=gen).to(cuda), torch.randn(1, 77, dim, generator=gen).to(cuda))
    with torch.no_grad():
        model.get_batch_input(batch, random_uncond=True)                 # first call: weights are packed, kernels planned
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            z, sparse_z, cond, fs, label = model.get_batch_input(batch, random_uncond=True, return_fs=True, return_class_label=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(z).all() and torch.isfinite(cond["c_crossattn"][0]).all() and torch.isfinite(cond["c_concat"][0]).all()
