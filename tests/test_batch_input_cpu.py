"""Host side of training from a data batch (LatentVisualDiffusion.get_batch_input / shared_step, reference ddpm3d.py:1056-1149) that
needs no GPU: the signature and the return order for the flag combinations the reference's own callers use, with stub stages in
place of the HIP ones; what a batch without data entries raises; the C-ABI of the two new kernels."""
import inspect
import os
import re

import pytest
import torch

from helpers import cfgs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, PX, L, D, NIMG = 2, 4, 16, 77, 64, 64


class _Fn(torch.nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return self.fn(x)


def _model(monkeypatch, **over):
    """The boundary class with every stage that would launch a kernel replaced: the two device methods of get_batch_input, the
    towers, the projector and the decoder.  What is left is the method's own plumbing."""
    from lvdm.models.ddpm3d import LatentVisualDiffusion
    ident = {"target": "torch.nn.Identity"}
    diff = dict(cfgs.DIFFUSION, first_stage_key="dense_frames", uncond_prob=0.05, **over)
    model = LatentVisualDiffusion(img_cond_stage_config=ident, image_proj_stage_config=ident, cond_stage_config=ident, first_stage_config=ident,
                                  unet_config={"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": cfgs.UNET_B}, **diff)
    seen = {}

    def encode_streams(x, sparse_x, sparse_depth):
        b, _, t, h, w = x.shape
        lat = lambda v, c: v.mean(1, keepdim=True).expand(b, c, t, h, w)[..., ::8, ::8].contiguous()
        return lat(x, 4), torch.cat([lat(sparse_x, 4) + 1, lat(sparse_depth, 4) + 2], 1)

    def cond_dropout(r, emb, null, sparse_x, frame):
        seen["r"] = r.clone()
        p = model.uncond_prob
        keep = 1 - ((r >= p).float() * (r < 3 * p).float())[:, None, None, None]
        return torch.where((r < 2 * p)[:, None, None], null, emb), keep * sparse_x[:, :, frame]

    monkeypatch.setattr(model, "_encode_streams", encode_streams)
    monkeypatch.setattr(model, "_cond_dropout", cond_dropout)
    monkeypatch.setattr(model, "get_learned_conditioning", lambda c: torch.full((len(c), L, D), float(len(c[0]))))
    model.embedder = _Fn(lambda img: img.flatten(1)[:, :1, None].expand(-1, NIMG, D))
    model.image_proj_model = _Fn(lambda tok: tok + 0.5)
    monkeypatch.setattr(model, "decode_first_stage", lambda z: z.mean(1, keepdim=True).expand(-1, 3, -1, -1, -1))
    return model, seen


def _batch():
    g = torch.Generator().manual_seed(5)
    clip = lambda: torch.rand(B, 3, T, PX, PX, generator=g) + 0.1
    return {"dense_frames": clip(), "sparse_frames": clip(), "sparse_depth": clip(), "class_label": torch.tensor([[500], [1]]),
            "caption": ["a street"] * B, "fps": torch.tensor([10, 12]), "frame_stride": torch.tensor([3, 4])}


def test_signature_is_the_reference_s():
    from lvdm.models.ddpm3d import LatentVisualDiffusion
    sig = inspect.signature(LatentVisualDiffusion.get_batch_input)
    assert list(sig.parameters) == ["self", "batch", "random_uncond", "return_first_stage_outputs", "return_original_cond", "return_fs",
                                    "return_cond_frame", "return_original_input", "return_sparse_input", "return_class_label", "kwargs"]
    assert all(sig.parameters[k].default is False for k in list(sig.parameters)[3:-1])
    assert sig.parameters["random_uncond"].default is inspect.Parameter.empty
    sh = inspect.signature(LatentVisualDiffusion.shared_step)
    assert list(sh.parameters) == ["self", "batch", "random_uncond", "kwargs"] and sh.parameters["random_uncond"].default is None
    assert list(inspect.signature(LatentVisualDiffusion.training_step).parameters) == ["self", "batch", "batch_idx"]
    assert callable(LatentVisualDiffusion.validation_step)


def test_return_order_for_the_flag_sets_of_shared_step_and_log_images(monkeypatch):
    model, _ = _model(monkeypatch)
    batch = _batch()
    # shared_step (ddpm3d.py:1057): return_fs + return_class_label
    out = model.get_batch_input(batch, random_uncond=False, return_fs=True, return_class_label=True)
    assert len(out) == 5
    z, sparse_z, cond, fs, label = out
    assert z.shape == (B, 4, T, 2, 2) and sparse_z.shape == z.shape and set(cond) == {"c_concat", "c_crossattn"}
    assert cond["c_concat"][0].shape == (B, 8, T, 2, 2) and torch.equal(sparse_z, cond["c_concat"][0][:, :4])
    assert cond["c_crossattn"][0].shape == (B, L + NIMG, D)
    assert torch.equal(fs, torch.tensor([10., 12.])) and fs.dtype == torch.float32                      # fps_condition_type "fps"
    assert torch.equal(label, torch.tensor([[500.], [1.]]))
    # log_images (ddpm3d.py:1200-1209)
    out = model.get_batch_input(batch, random_uncond=False, return_first_stage_outputs=True, return_original_cond=True, return_fs=True,
                                return_cond_frame=True, return_sparse_input=True, return_class_label=True)
    assert len(out) == 9
    z, sparse_z, cond, xrec, xc, fs, cond_x, sparse, label = out
    assert xrec.shape == (B, 3, T, 2, 2) and xc == batch["caption"] and torch.equal(fs, torch.tensor([10., 12.]))
    assert torch.equal(cond_x, batch["dense_frames"][:, :, :1]) and torch.equal(sparse, batch["sparse_frames"])
    assert torch.equal(label, torch.tensor([[500.], [1.]]))
    # every flag: the full order, return_original_input between the condition frame and the sparse input
    out = model.get_batch_input(batch, False, True, True, True, True, True, True, True)
    assert len(out) == 10 and torch.equal(out[7], batch["dense_frames"]) and torch.equal(out[8], batch["sparse_frames"])
    assert len(model.get_batch_input(batch, random_uncond=False)) == 3
    # fps_condition_type "fs" reads frame_stride
    model.fps_condition_type = "fs"
    assert torch.equal(model.get_batch_input(batch, random_uncond=False, return_fs=True)[3], torch.tensor([3., 4.]))


def test_dropout_draw_goes_through_one_method_and_false_means_nothing_dropped(monkeypatch):
    model, seen = _model(monkeypatch)
    batch = _batch()
    calls = []
    monkeypatch.setattr(model, "_uncond_draw", lambda n, device: calls.append((n, device)) or torch.tensor([0.02, 0.12]))
    _, _, cond = model.get_batch_input(batch, random_uncond=True)
    assert calls == [(B, batch["dense_frames"].device)] and torch.equal(seen["r"], torch.tensor([0.02, 0.12]))
    ctx = cond["c_crossattn"][0]
    # sample 0: r < p -> the null prompt (len("") = 0), its real image; sample 1: 2p <= r < 3p -> its prompt, the all-zero image
    assert torch.all(ctx[0, :L] == 0.0) and torch.all(ctx[1, :L] == float(len("a street")))
    assert torch.all(ctx[0, L:] == batch["sparse_frames"][0, 0, 0, 0, 0] + 0.5) and torch.all(ctx[1, L:] == 0.5)
    _, _, cond = model.get_batch_input(batch, random_uncond=False)
    assert len(calls) == 1 and torch.equal(seen["r"], torch.ones(B))
    ctx = cond["c_crossattn"][0]
    assert torch.all(ctx[:, :L] == float(len("a street"))) and torch.all(ctx[1, L:] == batch["sparse_frames"][1, 0, 0, 0, 0] + 0.5)
    # the draw itself: B uniforms on the batch's device
    r = type(model)._uncond_draw(model, 5, torch.device("cpu"))
    assert r.shape == (5,) and r.dtype == torch.float32 and bool(((r >= 0) & (r < 1)).all())


def test_interp_mode_and_rand_cond_frame(monkeypatch):
    model, _ = _model(monkeypatch, interp_mode=True)
    z, _, cond = model.get_batch_input(_batch(), random_uncond=False)
    cat = cond["c_concat"][0]
    assert cat.shape == z.shape and torch.equal(cat[:, :, 0], z[:, :, 0]) and torch.equal(cat[:, :, -1], z[:, :, -1])
    assert float(cat[:, :, 1:-1].abs().sum()) == 0.0
    model, _ = _model(monkeypatch, rand_cond_frame=True)
    with pytest.raises(AssertionError, match="random condition frame is not supported"):
        model.get_batch_input(_batch(), random_uncond=False)


def test_shared_step_routes_fs_sparse_x_and_label_and_a_batch_without_data_still_raises(monkeypatch):
    model, _ = _model(monkeypatch)
    batch = _batch()
    got = {}
    monkeypatch.setattr(type(model), "forward", lambda self, x, c, **kw: (got.update(x=x, c=c, kw=kw), (torch.tensor(1.5), {"val/loss": torch.tensor(1.5)}))[1])
    draws = []
    monkeypatch.setattr(model, "_uncond_draw", lambda n, device: draws.append(n) or torch.ones(n))
    loss, info = model.shared_step(batch, extra=7)                         # random_uncond None -> classifier_free_guidance (p > 0)
    assert draws == [B] and float(loss) == 1.5 and set(info) == {"val/loss"}
    kw = got["kw"]
    assert set(kw) == {"fs", "sparse_x", "class_label", "extra"} and kw["fs"].dtype == torch.int64 and torch.equal(kw["fs"], torch.tensor([10, 12]))
    assert torch.equal(kw["sparse_x"], got["c"]["c_concat"][0][:, :4]) and torch.equal(kw["class_label"], torch.tensor([[500.], [1.]]))
    model.shared_step(batch, random_uncond=False)
    assert draws == [B]
    # training_step: a data batch goes through shared_step with the model's guidance setting; validation_step returns the dictionary
    assert float(model.training_step(batch, 3)) == 1.5 and draws == [B, B]
    assert set(model.validation_step(batch)) == {"val/loss"}
    for bad in ({}, {k: v for k, v in batch.items() if k != "sparse_depth"}):
        with pytest.raises(NotImplementedError, match="data") as e:
            model.shared_step(bad)
        assert "sparse_depth" in str(e.value)
    with pytest.raises(NotImplementedError, match="data"):
        model.training_step({"cond": None})


def test_step_training_step_takes_a_data_batch(monkeypatch):
    from mudg_amd.train import step
    w = torch.nn.Parameter(torch.tensor([2.0]))

    class Model:
        classifier_free_guidance = True

        def shared_step(self, batch, random_uncond, **kw):
            assert random_uncond is True and kw == {"k": 1}
            loss = (w * batch["v"]).sum()
            return loss, {"train/loss": loss.detach()}

    opt = torch.optim.SGD([w], lr=0.1)
    loss, info = step.training_step(Model(), {"v": torch.tensor([3.0])}, optimizer=opt, k=1)
    assert float(loss) == 6.0 and set(info) == {"train/loss"} and abs(float(w.detach()) - 1.7) < 1e-6
    with pytest.raises(TypeError):
        step.training_step(Model(), {"v": torch.tensor([3.0])}, None, torch.tensor([1]), opt)


def test_new_entry_points_are_declared_and_bound():
    from mudg_amd import build, hip
    header = open(os.path.join(ROOT, "include", "mudg_hip.h")).read()
    for name, nargs in (("mudg_posterior_assemble", 14), ("mudg_cond_dropout", 16)):
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, header, re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == nargs
    assert "batch_input.hip" in build.SOURCES


def test_batch_input_kernels_use_no_scratch_and_16_byte_accesses(tmp_path):
    """tests/test_isa_rules.py-style: both kernels (16-byte and scalar forms) compile for gfx950 without private memory — the stream
    pointers are selected, not indexed, out of the by-value argument — and the 16-byte forms load and store four values at a time."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "batch_input.s"
    subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S",
                    os.path.join(ROOT, "mudg_amd", "csrc", "batch_input.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    s = out.read_text()
    md = s[s.index("amdhsa.kernels"):]
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", md, re.S):
        for family in ("posterior_assemble_kernel", "cond_dropout_kernel"):
            if family in m.group(1):
                seen[family] = seen.get(family, 0) + 1
                assert int(m.group(2)) == 0, m.groups()
    assert seen == {"posterior_assemble_kernel": 2, "cond_dropout_kernel": 2}, seen
    for name in re.findall(r"^(_Z\S*(?:posterior_assemble|cond_dropout)_kernelILi4E\S*):", s, re.M):
        body = s[s.index(name + ":"):]
        body = body[:body.index(".end_amdhsa_kernel")]
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body and "scratch_" not in body, name
