"""Validating while training on the GPU: LatentVisualDiffusion.log_images against what the REFERENCE's method gave for the same seeded
batch (tests/golden/validate.pt, made by tests/golden/make_golden_validate.py), the three multi-tensor kernels behind the averaged
weights, the frame-sheet kernel, and the first place where the training side and the inference side meet in one process: a sampler
run between two optimiser steps, and weights exchanged under the sampler's feet by ema_scope.

No new bounds: `reconst` is held to tests/test_pipeline_gpu.py's TOL_DEC and `samples` to its TOL_E2E (the guided few-step
end-to-end guard of the same fixture topology); in the bf16x3 child both are the literal 1e-3.

The test prints the measured rel-L2 of every comparison before it asserts; DESIGN.md §11 says which of them have been recorded."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import golden, rel_l2, seeded_sd, seeding
from validate_common import ema_model, replay_ema, set_params

from mudg_amd import hip as _hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = _hip.operand_name()
# tests/test_pipeline_gpu.py: TOL_E2E, TOL_DEC
TOL_E2E, TOL_DEC = {"bf16": (6e-2, 2e-2), "fp16": (1e-2, 3e-3), "bf16x3": (1e-3, 1e-3), "bf16x6": (1e-3, 1e-3)}[MODE]


def build_model(g, dev, **over):
    from lvdm.models.ddpm3d import LatentVisualDiffusion
    from lvdm.modules.encoders.resampler import Resampler
    from helpers import _load
    towers, towers_batch = _load("towers"), _load("towers_batch")
    ident = {"target": "torch.nn.Identity"}
    model = LatentVisualDiffusion(
        img_cond_stage_config=ident, image_proj_stage_config=ident, cond_stage_config=ident,
        first_stage_config={"target": "lvdm.models.autoencoder.AutoencoderKL",
                            "params": {"embed_dim": 4, "ddconfig": g["vae_ddconfig"], "lossconfig": ident}},
        unet_config={"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": g["unet_cfg"]},
        **dict(g["diffusion_cfg"], **over))
    model.model.diffusion_model.load_state_dict(seeded_sd(g["unet_param_shapes"], g["seed"], g["unet_checksum"]), strict=True)
    model.first_stage_model.load_state_dict(seeded_sd(g["vae_param_shapes"], g["seed"] + 1, g["vae_checksum"]), strict=True)
    d = g["driver"]
    model.image_proj_model = Resampler(**d["resampler"])
    model.image_proj_model.load_state_dict(seeded_sd(g["resampler_param_shapes"], g["seed"] + 5, g["resampler_checksum"]), strict=True)
    model.embedder = towers_batch.PerSampleImageTower(d["clip_tokens"], d["clip_dim"], d["tower_seed_img"])
    model.cond_stage_model = towers.FakeTextTower(g["unet_cfg"]["context_dim"], d["tower_seed_txt"], dev)
    return model.to(dev).eval()


def make_batch(g, dev):
    """The batch make_golden_validate.py fed the reference (make_golden_batch.py's), rebuilt from its seeds."""
    B, T, px = g["B"], g["unet_cfg"]["temporal_length"], g["driver"]["pixels"]
    clip = lambda name: seeding.seeded_input(name, (B, 3, T, px, px), g["input_seed"], 0.5).clamp(-1, 1).to(dev)
    return {"dense_frames": clip("bi_dense"), "sparse_frames": clip("bi_sparse"), "sparse_depth": clip("bi_depth"),
            "class_label": torch.tensor([0, 500, 1, 0], dtype=torch.long, device=dev)[:, None], "caption": ["a street"] * B,
            "fps": torch.full((B,), 10, dtype=torch.long, device=dev)}


def x_T(g, dev):
    return seeding.seeded_input("validate_x_T", (1, 4, g["unet_cfg"]["temporal_length"], 8, 8), g["xt_seed"]).to(dev)


def run_log_images(model, g, dev, scale=7.5, **over):
    torch.manual_seed(g["cpu_seed"])
    return model.log_images(make_batch(g, dev), unconditional_guidance_scale=scale, x_T=x_T(g, dev), **dict(g["log_kwargs"], **over))


# ------------------------------------------------------------------------------------------------ log_images vs the reference
def test_log_images_matches_the_reference(cuda):
    """The rel-L2 of `reconst` and `samples` against the reference is printed before it is held to the bound."""
    g = golden("validate.pt")
    model = build_model(g, cuda)
    want = g["log_images"]["guided"]
    for tag, scale, samples in (("guided 7.5", 7.5, want["samples"]), ("unguided", 1.0, g["log_images"]["plain"]["samples"])):
        batch = make_batch(g, cuda)
        torch.manual_seed(g["cpu_seed"])
        log = model.log_images(batch, unconditional_guidance_scale=scale, x_T=x_T(g, cuda), **g["log_kwargs"])
        assert list(log) == ["image_condition", "reconst", "condition", "samples"]
        assert batch["dense_frames"].shape[0] == g["B"]                                   # the caller's batch is not cut
        e_rec, e_smp = rel_l2(log["reconst"], want["reconst"]), rel_l2(log["samples"], samples)
        print(f"[{MODE}] log_images ({tag}, 4 steps) rel-L2 vs the reference: reconst {e_rec:.3e} (bound {TOL_DEC:g})  "
              f"samples {e_smp:.3e} (bound {TOL_E2E:g})")
        assert torch.equal(log["image_condition"].cpu(), want["image_condition"]) and log["condition"] == want["condition"]
        assert log["reconst"].shape == want["reconst"].shape and log["samples"].shape == samples.shape
        assert e_rec < TOL_DEC, e_rec
        assert e_smp < TOL_E2E, e_smp


def test_denoise_row_is_the_grid_of_the_decoded_pred_x0_list(cuda, monkeypatch):
    g = golden("validate.pt")
    model = build_model(g, cuda)
    seen = {}
    orig = model.sample_log

    def tapped(**kw):
        out = orig(**kw)
        seen["pred_x0"] = out[1]["pred_x0"]
        return out

    monkeypatch.setattr(model, "sample_log", tapped)
    log = run_log_images(model, g, cuda, plot_denoise_rows=True)
    rows, T, px, pad = seen["pred_x0"], g["unet_cfg"]["temporal_length"], g["driver"]["pixels"], 2
    grid = log["denoise_row"]
    assert len(rows) >= 2 and grid.shape == (3, len(rows) * (px + pad) + pad, T * (px + pad) + pad)
    covered = torch.zeros_like(grid, dtype=torch.bool)
    for r, z in enumerate(rows):
        frames = model.decode_first_stage(z)                                              # (1, 3, T, px, px)
        for t in range(T):
            y0, x0 = r * (px + pad) + pad, t * (px + pad) + pad
            assert torch.equal(grid[:, y0:y0 + px, x0:x0 + px], frames[0, :, t]), (r, t)
            covered[:, y0:y0 + px, x0:x0 + px] = True
    assert torch.all(grid[~covered] == 0.0)


def test_log_images_in_the_bf16x3_build_meets_the_literal_1e_3():
    """ONE child process of this file's reference comparison with MUDG_OPERAND=bf16x3 (the operand type is fixed per process)."""
    if os.environ.get("MUDG_VALIDATE_CHILD") == "1":
        pytest.skip("already inside the bf16x3 child")
    if MODE != "bf16":
        pytest.skip("the child is started from the default operand mode only")
    env = dict(os.environ, MUDG_OPERAND="bf16x3", MUDG_VALIDATE_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_validate_gpu.py"), "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider",
                        "-k", "test_log_images_matches_the_reference"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    print("\n".join(l for l in r.stdout.splitlines() if "rel-L2" in l or "passed" in l or "failed" in l))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
    assert "[bf16x3] log_images" in r.stdout and "1 passed" in r.stdout


# ------------------------------------------------------------------------------------------------ the multi-tensor kernels
def test_ema_multi_is_bit_equal_to_the_reference(cuda):
    from lvdm.ema import LitEma
    g = golden("validate.pt")
    for tag, ema in replay_ema(g, LitEma, cuda):
        if tag == "init":
            continue
        sd = ema.state_dict()
        for key, value in g["ema"][tag].items():
            assert sd[key].is_cuda and torch.equal(sd[key].cpu(), value), (tag, key)


def _state(seed, dev, sizes=(5, 16384 * 2 + 7, 16384, 33, 4096 + 3)):
    """Parameters, gradients and shadows of sizes that are no multiples of four and that span several chunks."""
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(n, generator=gen).to(dev)) for n in sizes]
    for p in ps:
        p.grad = (torch.randn(p.numel(), generator=gen) * 0.1).to(dev)
    return ps


class _Holder(torch.nn.Module):
    def __init__(self, ps):
        super().__init__()
        self.ps = torch.nn.ParameterList(ps)


def test_fused_adamw_ema_equals_adamw_then_ema_bit_for_bit(cuda):
    from lvdm.ema import LitEma
    from mudg_amd.train import step
    runs = {}
    for fused in (False, True):
        ps = _state(3, cuda)
        extra = torch.nn.Parameter(torch.ones(9, device=cuda))            # in the optimiser, not under the average
        extra.grad = torch.full((9,), 0.5, device=cuda)
        idle = torch.nn.Parameter(torch.ones(6, device=cuda))             # under the average, never given a gradient
        holder = _Holder(ps + [idle])
        ema = LitEma(holder, decay=0.9)
        with torch.no_grad():
            for p in ps:
                p.mul_(1.25)                                              # weights != shadows
            idle.add_(1.0)
        opt = step.AdamW(ps + [extra, idle], lr=1e-2, weight_decay=0.1)
        for k in range(3):
            if fused:
                opt.step(ema=ema)
            else:
                opt.step()
                ema(holder)
        torch.cuda.synchronize()
        runs[fused] = ([p.detach().clone() for p in ps + [extra, idle]], [opt.state[p][k].clone() for p in ps + [extra] for k in ("exp_avg", "exp_avg_sq")],
                       {k: v.clone() for k, v in ema.state_dict().items()})
        assert int(ema.num_updates) == 3 and not opt.state[idle]
    for a, b in zip(runs[False][0], runs[True][0]):
        assert torch.equal(a, b)
    for a, b in zip(runs[False][1], runs[True][1]):
        assert torch.equal(a, b)
    assert all(torch.equal(v, runs[True][2][k]) for k, v in runs[False][2].items())
    assert not torch.equal(runs[True][2]["ps0"], runs[True][0][0]) and not torch.equal(runs[True][2]["ps5"], torch.ones(6, device=cuda))
    # against torch.optim.AdamW + the reference's expression on the CPU: same semantics (the kernel's rounding differs from torch's)
    ref = [torch.nn.Parameter(p.detach().cpu().clone()) for p in _state(3, "cpu")]
    shadow = [p.detach().clone() for p in ref]
    with torch.no_grad():
        for p in ref:
            p.mul_(1.25)
    for p, q in zip(ref, _state(3, "cpu")):
        p.grad = q.grad
    topt = torch.optim.AdamW(ref, lr=1e-2, weight_decay=0.1)
    for k in range(3):
        topt.step()
        omd = 1.0 - min(torch.tensor(0.9), (1 + torch.tensor(k + 1, dtype=torch.int)) / (10 + torch.tensor(k + 1, dtype=torch.int)))
        for s, p in zip(shadow, ref):
            s.sub_(omd * (s - p.detach()))
    for i, s in enumerate(shadow):
        assert torch.allclose(runs[True][2][f"ps{i}"].cpu(), s, rtol=1e-5, atol=1e-6), i


def test_swap_twice_is_the_identity_bit_for_bit(cuda):
    from lvdm.ema import LitEma
    ps = _state(4, cuda)
    holder = _Holder(ps)
    ema = LitEma(holder)
    with torch.no_grad():
        for p in ps:
            p.mul_(-0.5)
        ps[1][3] = float("nan")                                           # bits, not values
    weights = [p.detach().clone() for p in ps]
    shadows = [getattr(ema, f"ps{i}").clone() for i in range(len(ps))]
    versions = [p._version for p in ps]
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    ema.swap(holder)
    assert all(same(p, s) for p, s in zip(ps, shadows)) and all(same(getattr(ema, f"ps{i}"), w) for i, w in enumerate(weights))
    assert all(p._version > v for p, v in zip(ps, versions))
    ema.swap(holder)
    assert all(same(p, w) for p, w in zip(ps, weights)) and all(same(getattr(ema, f"ps{i}"), s) for i, s in enumerate(shadows))
    # a view that is only 4-byte aligned takes the scalar loop: same result
    flat = torch.arange(0, 41, dtype=torch.float32, device=cuda)
    odd = _Holder([torch.nn.Parameter(flat[1:38])])
    ema_odd = LitEma(odd)
    with torch.no_grad():
        odd.ps[0].neg_()
    ema_odd.swap(odd)
    assert torch.equal(odd.ps[0], torch.arange(1, 38, dtype=torch.float32, device=cuda)) and torch.equal(ema_odd.ps0, -torch.arange(1, 38, dtype=torch.float32, device=cuda))
    assert float(flat[0]) == 0.0 and torch.equal(flat[38:], torch.arange(38, 41, dtype=torch.float32, device=cuda))


def test_rows_that_are_only_4_byte_aligned_take_the_scalar_loop_in_the_ema_kernels(cuda):
    """A parameter that is a view into a flat bucket (flat[1:38]): mudg_ema_multi and mudg_adamw_ema_multi on it give the bits they
    give on an aligned copy of the same values, and the bucket's neighbours are untouched."""
    from lvdm.ema import LitEma
    from mudg_amd.train import step
    gen = torch.Generator().manual_seed(8)
    values, grads = torch.randn(37, generator=gen).to(cuda), torch.randn(37, generator=gen).to(cuda)
    out = {}
    for odd in (False, True):
        flat = torch.full((41,), 7.0, device=cuda)
        flat[1:38] = values
        p = torch.nn.Parameter(flat[1:38] if odd else values.clone())
        assert (p.data_ptr() % 16 != 0) == odd
        holder = _Holder([p])
        ema = LitEma(holder, decay=0.9)
        with torch.no_grad():
            p.mul_(1.5)
        ema(holder)                                                       # mudg_ema_multi
        after_ema = ema.ps0.clone()
        p.grad = grads.clone()
        opt = step.AdamW([p], lr=1e-2, weight_decay=0.1)
        opt.step(ema=ema)                                                 # mudg_adamw_ema_multi
        torch.cuda.synchronize()
        out[odd] = (after_ema, p.detach().clone(), ema.ps0.clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
        if odd:
            assert float(flat[0]) == 7.0 and torch.all(flat[38:] == 7.0) and torch.equal(flat[1:38], p.detach())
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)
    assert not torch.equal(out[True][0], values) and not torch.equal(out[True][1], values * 1.5)


# ------------------------------------------------------------------------------------------------ the loop
def _train_inputs(g, dev):
    gb = golden("batch_input.pt")
    want = gb["outs"]["dropout"]
    cond = {"c_crossattn": [want["c_crossattn"].to(dev)], "c_concat": [want["c_concat"].to(dev)]}
    return dict(x_start=want["z"].to(dev), cond=cond, t=gb["t"].to(dev), noise=gb["noise"].to(dev),
                class_label=want["class_label"].to(dev), fs=want["fs"].long().to(dev))


def _trainable(model):
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.learning_rate = 1e-3
    return model.configure_optimizers()


def _logged(model, g, dev):
    model.eval()
    try:
        return run_log_images(model, g, dev)
    finally:
        model.train()


def test_log_images_between_two_steps_changes_nothing_and_follows_the_weights(cuda):
    from mudg_amd.train import step
    g = golden("validate.pt")
    inp = _train_inputs(g, cuda)
    plain = build_model(g, cuda)
    opt = _trainable(plain)
    want = [step.training_step(plain, optimizer=opt, **inp)[0].clone() for _ in range(2)]
    model = build_model(g, cuda)
    opt = _trainable(model)
    log0 = _logged(model, g, cuda)
    loss1, _ = step.training_step(model, optimizer=opt, **inp)
    log1 = _logged(model, g, cuda)
    loss2, _ = step.training_step(model, optimizer=opt, **inp)
    assert torch.equal(loss1, want[0]) and torch.equal(loss2, want[1]) and not torch.equal(loss1, loss2)
    for (k, a), (_, b) in zip(plain.state_dict().items(), model.state_dict().items()):
        assert torch.equal(a, b), k
    # the sampler ran on the stepped weights: not what it gave before the step, and exactly what a fresh model with those weights gives
    assert not torch.equal(log0["samples"], log1["samples"]) and torch.equal(log0["reconst"], log1["reconst"])
    fresh = build_model(g, cuda)
    stepped = build_model(g, cuda)
    opt = _trainable(stepped)
    step.training_step(stepped, optimizer=opt, **inp)
    fresh.load_state_dict(stepped.state_dict(), strict=True)
    assert torch.equal(_logged(fresh, g, cuda)["samples"], log1["samples"])


def test_log_images_with_use_ema_samples_on_the_shadow_weights_and_gives_the_training_weights_back(cuda):
    from mudg_amd.train import step
    g = golden("validate.pt")
    inp = _train_inputs(g, cuda)
    model = build_model(g, cuda, use_ema=True)          # the shadows are the constructor's initial weights, the weights the seeded ones
    ema = model.model_ema
    opt = _trainable(model)
    step.training_step(model, optimizer=opt, ema=ema, **inp)
    assert int(ema.num_updates) == 1
    before = {k: v.clone() for k, v in model.state_dict().items()}
    log = _logged(model, g, cuda)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k                                               # weights AND shadows, bit for bit
    shadow = build_model(g, cuda)
    sd = {name: before["model_ema." + s_name] for name, s_name in ema.m_name2s_name.items()}
    assert shadow.model.load_state_dict(sd, strict=False).unexpected_keys == []
    shadow.image_proj_model.load_state_dict(model.image_proj_model.state_dict())
    got = _logged(shadow, g, cuda)
    assert torch.equal(got["samples"], log["samples"])
    weights = build_model(g, cuda)
    weights.load_state_dict({k: v for k, v in before.items() if not k.startswith("model_ema.")}, strict=True)
    assert not torch.equal(_logged(weights, g, cuda)["samples"], log["samples"])
    # validation_step: the plain entries and the *_ema entries
    out = model.validation_step(make_batch(g, cuda))
    assert {k for k in out if k.endswith("_ema")} == {k + "_ema" for k in out if not k.endswith("_ema")} and len(out) == 6
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k


# ------------------------------------------------------------------------------------------------ sheets
def test_log_sheet_is_byte_equal_to_the_reference_and_to_the_torch_expression(cuda):
    from mudg_amd import ops
    g = golden("validate.pt")
    for key, want in g["sheets"].items():
        got = ops.log_sheet(g["log_images"]["guided"][key].to(cuda))
        assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got.cpu(), want), key

    def torch_sheet(v, clamp, rescale):                                    # utils/save_video.py:133, 91-96 written out
        v = v.float() if v.dim() == 5 else v.float().unsqueeze(2)
        if clamp:
            v = torch.clamp(v, -1., 1.)
        n, c, t, h, w = v.shape
        grid = v.permute(2, 1, 0, 3, 4).reshape(t, c, n * h, w).expand(t, 3, n * h, w)
        if rescale:
            grid = (grid + 1.0) / 2.0
        return (grid * 255).to(torch.uint8).permute(0, 2, 3, 1)

    gen = torch.Generator().manual_seed(17)
    for shape in ((3, 3, 5, 7, 12), (2, 1, 3, 6, 8), (2, 3, 2, 5, 9), (4, 3, 9, 16), (3, 1, 7, 5)):     # 16-byte form / scalar form, video / image
        v = torch.randn(shape, generator=gen) * 0.8
        v.view(-1)[:4] = torch.tensor([-1.0, 1.0, 0.999999, 0.003921568])
        got = ops.log_sheet(v.to(cuda))
        want = torch_sheet(v, True, True)
        assert got.shape == (want.shape if len(shape) == 5 else want.shape[1:]) and torch.equal(got.cpu().reshape(want.shape), want), shape
        pos = v.abs().clamp(max=1.0)                                       # no rescale: values in [0, 1]
        assert torch.equal(ops.log_sheet(pos.to(cuda), clamp=False, rescale=False).cpu().reshape(want.shape), torch_sheet(pos, False, False)), shape
    with pytest.raises(_hip.MudgError):
        ops.log_sheet(torch.zeros(1, 4, 2, 8, 8, device=cuda))


def test_image_logger_writes_the_sheets_of_a_training_run(cuda, tmp_path, monkeypatch):
    """INTEGRATION.md's few lines: training_step with a data batch, then the callback; the sheets of reconst and samples are on disk."""
    import numpy as np
    import utils.save_video as save_video
    from main.callbacks import ImageLogger
    monkeypatch.setattr(save_video, "_video_writer", lambda: None)        # the .npy branch, whether or not torchvision.io imports
    from mudg_amd.train import step
    g = golden("validate.pt")
    model = build_model(g, cuda)
    model.logdir = str(tmp_path)
    opt = _trainable(model)
    logger = ImageLogger(batch_frequency=1, save_dir=str(tmp_path), to_local=True,
                         log_images_kwargs=dict(ddim_steps=4, ddim_eta=0.0, unconditional_guidance_scale=7.5, x_T=x_T(g, cuda)))
    batch = make_batch(g, cuda)
    torch.manual_seed(g["cpu_seed"])
    loss, info = step.training_step(model, batch, optimizer=opt)
    assert torch.isfinite(loss)
    torch.manual_seed(g["cpu_seed"])
    logger.on_train_batch_end(None, model, None, batch, 0)
    assert model.training
    names = sorted(os.listdir(tmp_path / "images" / "train"))
    stem = "gs0_ep0_idx0_rank0"
    assert names == sorted([f"condition-{stem}.txt"] + [f"{k}-{stem}.npy" for k in ("image_condition", "reconst", "samples")])
    for key in ("reconst", "samples"):
        sheet = np.load(tmp_path / "images" / "train" / f"{key}-{stem}.npy")
        assert sheet.dtype == np.uint8 and sheet.shape == (g["unet_cfg"]["temporal_length"], 64, 64, 3) and sheet.std() > 0
