"""Host side of validating while training that needs no GPU: LitEma against the REFERENCE's shadows (tests/golden/validate.pt, made by
tests/golden/make_golden_validate.py), ema_scope, the plumbing of log_images with the sampler and every stage that would launch a
kernel replaced by recording fakes, the frame-sheet writer on CPU tensors against the reference's sheets, ImageLogger's frequency and
mode handling, and the C-ABI of the four new kernels."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from helpers import cfgs, golden
from validate_common import ema_model, replay_ema, set_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, PX, L, D, NIMG = 3, 4, 16, 77, 64, 64


# ------------------------------------------------------------------------------------------------ LitEma
def test_lit_ema_is_bit_equal_to_the_reference_on_cpu_tensors():
    from lvdm.ema import LitEma
    g = golden("validate.pt")
    for tag, ema in replay_ema(g, LitEma):
        sd = ema.state_dict()
        if tag == "init":
            assert list(sd.keys()) == g["ema"]["keys"] and ema.m_name2s_name == g["ema"]["m_name2s_name"]
            assert "frozenweight" not in sd and sd["num_updates"].dtype == torch.int32 and int(sd["num_updates"]) == 0
            continue
        want = g["ema"][tag]
        assert set(want) <= set(sd)
        for key, value in want.items():
            assert sd[key].dtype == value.dtype and torch.equal(sd[key], value), (tag, key)
    assert int(ema.num_updates) == 86


def test_lit_ema_state_dict_round_trip_and_the_reference_s_helpers():
    from lvdm.ema import LitEma
    g = golden("validate.pt")
    model = ema_model(g["ema_shapes"])
    set_params(model, 5, 0)
    ema = LitEma(model, decay=0.9)
    for k in range(3):
        set_params(model, 5, k + 1)
        ema(model)
    other = LitEma(ema_model(g["ema_shapes"]), decay=0.5)
    assert other.load_state_dict(ema.state_dict(), strict=True).missing_keys == []
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in ema.state_dict().items())
    # the loaded scalars drive the next update: both take the same fourth step
    set_params(model, 5, 9)
    ema(model)
    other(model)
    assert int(other.num_updates) == 4 and all(torch.equal(v, other.state_dict()[k]) for k, v in ema.state_dict().items())
    # use_num_upates=False: the constant decay, num_updates stays -1
    fixed = LitEma(model, decay=0.75, use_num_upates=False)
    before = {k: v.clone() for k, v in fixed.state_dict().items()}
    set_params(model, 5, 10)
    fixed(model)
    assert int(fixed.num_updates) == -1
    p, s0 = dict(model.named_parameters())["net.0.bias"], before["net0bias"]
    assert torch.equal(fixed.net0bias, s0 - torch.tensor(0.25) * (s0 - p.detach()))
    # store / copy_to / restore, and swap twice = identity
    params = [p.detach().clone() for p in model.parameters()]
    ema.store(model.parameters())
    ema.copy_to(model)
    assert torch.equal(dict(model.named_parameters())["wide.weight"], ema.wideweight)
    assert torch.equal(dict(model.named_parameters())["frozen.weight"], params[-1])
    ema.restore(model.parameters())
    assert all(torch.equal(a, b) for a, b in zip(params, model.parameters()))
    shadows = {k: v.clone() for k, v in ema.state_dict().items()}
    versions = [p._version for p in model.parameters() if p.requires_grad]
    ema.swap(model)
    assert torch.equal(dict(model.named_parameters())["net.0.weight"], shadows["net0weight"]) and torch.equal(ema.net0weight, params[0])
    assert all(p._version > v for p, v in zip((p for p in model.parameters() if p.requires_grad), versions))
    ema.swap(model)
    assert all(torch.equal(a, b) for a, b in zip(params, model.parameters()))
    assert all(torch.equal(v, ema.state_dict()[k]) for k, v in shadows.items())
    with pytest.raises(ValueError):
        LitEma(model, decay=1.5)


# ------------------------------------------------------------------------------------------------ the boundary class
class _Fn(torch.nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return self.fn(x)


def _model(monkeypatch, **over):
    """As tests/test_batch_input_cpu.py: every stage that would launch a kernel replaced; the method's own plumbing is left."""
    from lvdm.models.ddpm3d import LatentVisualDiffusion
    ident = {"target": "torch.nn.Identity"}
    diff = dict(cfgs.DIFFUSION, first_stage_key="dense_frames", uncond_prob=0.05)
    diff.update(over)
    model = LatentVisualDiffusion(img_cond_stage_config=ident, image_proj_stage_config=ident, cond_stage_config=ident, first_stage_config=ident,
                                  unet_config={"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": cfgs.UNET_B}, **diff)

    def encode_streams(x, sparse_x, sparse_depth):
        b, _, t, h, w = x.shape
        lat = lambda v, c: v.mean(1, keepdim=True).expand(b, c, t, h, w)[..., ::8, ::8].contiguous()
        return lat(x, 4), torch.cat([lat(sparse_x, 4) + 1, lat(sparse_depth, 4) + 2], 1)

    monkeypatch.setattr(model, "_encode_streams", encode_streams)
    monkeypatch.setattr(model, "_cond_dropout", lambda r, emb, null, sparse_x, frame: (emb, sparse_x[:, :, frame]))
    monkeypatch.setattr(model, "get_learned_conditioning", lambda c: torch.full((len(c), L, D), float(len(c[0]))))
    model.embedder = _Fn(lambda img: img.flatten(1)[:, :1, None].expand(-1, NIMG, D))
    model.image_proj_model = _Fn(lambda tok: tok + 0.5)
    monkeypatch.setattr(model, "decode_first_stage", lambda z: z.mean(1, keepdim=True).expand(-1, 3, -1, -1, -1) * 1.0)
    return model


def _batch():
    g = torch.Generator().manual_seed(5)
    clip = lambda: torch.rand(B, 3, T, PX, PX, generator=g) + 0.1
    return {"dense_frames": clip(), "sparse_frames": clip(), "sparse_depth": clip(), "class_label": torch.tensor([[500], [1], [0]]),
            "caption": ["a street", "a road", "a lane"], "fps": torch.tensor([10, 12, 8]), "tasks": "all"}


class _RecordingSampler:
    calls = []

    def __init__(self, model, **kw):
        self.model = model

    def sample(self, S, batch_size, shape, conditioning=None, **kw):
        type(self).calls.append(dict(S=S, batch_size=batch_size, shape=tuple(shape), cond=conditioning, kw=kw,
                                     weights=next(self.model.model.parameters()).detach().clone()))
        out = torch.full((batch_size, *shape), 0.25)
        return out, {"x_inter": [out, out], "pred_x0": [out + 1, out + 2, out + 3]}


@pytest.fixture
def sampler(monkeypatch):
    import lvdm.models.samplers.ddim as ddim
    _RecordingSampler.calls = []
    monkeypatch.setattr(ddim, "DDIMSampler", _RecordingSampler)
    return _RecordingSampler


def test_log_images_signature_keys_and_the_one_sample_cut(monkeypatch, sampler):
    from lvdm.models.ddpm3d import LatentVisualDiffusion
    sig = inspect.signature(LatentVisualDiffusion.log_images)
    assert list(sig.parameters) == ["self", "batch", "sample", "ddim_steps", "ddim_eta", "plot_denoise_rows", "unconditional_guidance_scale",
                                    "mask", "kwargs"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:-1]] == [True, 50, 1., False, 1.0, None]
    assert list(inspect.signature(LatentVisualDiffusion.sample_log).parameters) == ["self", "cond", "batch_size", "ddim", "ddim_steps", "kwargs"]
    model = _model(monkeypatch)
    batch = _batch()
    kept = {k: (v.clone() if torch.is_tensor(v) else list(v) if isinstance(v, list) else v) for k, v in batch.items()}
    x_T = torch.randn(1, 4, T, 8, 8)
    log = model.log_images(batch, ddim_steps=7, ddim_eta=0.0, unconditional_guidance_scale=1.0, split="train", x_T=x_T)
    assert list(log) == ["image_condition", "reconst", "condition", "samples"]
    # the caller's batch is whole (a stated difference to the reference, which cuts it in place)
    assert set(batch) == set(kept) and all(torch.equal(batch[k], kept[k]) if torch.is_tensor(kept[k]) else batch[k] == kept[k] for k in kept)
    assert log["image_condition"].shape == (1, 3, 1, PX, PX) and torch.equal(log["image_condition"], batch["dense_frames"][:1, :, :1])
    assert log["reconst"].shape == (1, 3, T, 2, 2) and log["condition"] == ["a street_fs=10.0"]
    assert log["samples"].shape == (1, 3, T, 8, 8) and torch.all(log["samples"] == 0.25)
    (call,) = sampler.calls
    assert call["S"] == 7 and call["batch_size"] == 1 and call["shape"] == (4, T, 8, 8)
    kw = call["kw"]
    assert kw["verbose"] is False and kw["eta"] == 0.0 and kw["unconditional_guidance_scale"] == 1.0 and kw["unconditional_conditioning"] is None
    assert kw["split"] == "train" and kw["x_T"] is x_T                                  # handed on as they came
    assert kw["x0"].shape == (1, 4, T, 2, 2) and torch.equal(kw["x0"], batch["dense_frames"][:1].mean(1, keepdim=True).expand(-1, 4, -1, -1, -1)[..., ::8, ::8])
    assert kw["fs"].dtype == torch.int64 and torch.equal(kw["fs"], torch.tensor([10])) and torch.equal(kw["class_label"], torch.tensor([[500.]]))
    assert set(call["cond"]) == {"c_concat", "c_crossattn"} and call["cond"]["c_crossattn"][0].shape == (1, L + NIMG, D)
    # sample=False: no sampler run, no samples
    assert list(model.log_images(batch, sample=False)) == ["image_condition", "reconst", "condition"] and len(sampler.calls) == 1
    # ddim_steps=None selects the ancestral sampler, which is not built
    with pytest.raises(NotImplementedError):
        model.log_images(batch, ddim_steps=None)


@pytest.mark.parametrize("uncond_type", ["empty_seq", "zero_embed"])
def test_log_images_unconditional_branch(monkeypatch, sampler, uncond_type):
    model = _model(monkeypatch, uncond_type=uncond_type)
    batch = _batch()
    log = model.log_images(batch, ddim_steps=3, unconditional_guidance_scale=7.5, plot_denoise_rows=True)
    (call,) = sampler.calls
    cond, uc = call["cond"], call["kw"]["unconditional_conditioning"]
    assert call["kw"]["unconditional_guidance_scale"] == 7.5 and call["kw"]["eta"] == 1.0
    assert set(uc) == {"c_concat", "c_crossattn"} and uc["c_concat"][0] is cond["c_concat"][0]          # shared, not copied
    ctx = uc["c_crossattn"][0]
    assert cond["c_crossattn"][0].shape == (1, L + NIMG, D)
    # empty_seq: the text tower on [""] (the fake answers len(prompt) = 0), 77 rows; zero_embed: zeros_like of the WHOLE conditional
    # context, text and image rows, as the reference writes it (ddpm3d.py:1236-1237).  Then the all-zero image through both stages.
    text_rows = L if uncond_type == "empty_seq" else L + NIMG
    assert ctx.shape == (1, text_rows + NIMG, D)
    assert torch.all(ctx[:, :text_rows] == 0.0) and torch.all(ctx[:, text_rows:] == 0.5)
    assert torch.all(cond["c_crossattn"][0][:, :L] == float(len("a street")))
    assert torch.all(cond["c_crossattn"][0][:, L:] == batch["sparse_frames"][0, 0, 0, 0, 0] + 0.5)
    # denoise_row: the three recorded pred_x0 entries decoded, one grid row each, T columns, 2 pixels of zero padding
    grid = log["denoise_row"]
    assert list(log) == ["image_condition", "reconst", "condition", "samples", "denoise_row"]
    assert grid.shape == (3, 3 * 10 + 2, T * 10 + 2)
    for row in range(3):
        for col in range(T):
            cell = grid[:, 2 + 10 * row:10 + 10 * row, 2 + 10 * col:10 + 10 * col]
            assert torch.all(cell == 0.25 + row + 1)
    mask = torch.ones_like(grid, dtype=torch.bool)
    for row in range(3):
        for col in range(T):
            mask[:, 2 + 10 * row:10 + 10 * row, 2 + 10 * col:10 + 10 * col] = False
    assert torch.all(grid[mask] == 0.0)


def test_make_grid_layout_matches_its_definition():
    from lvdm.models.ddpm3d import _make_grid
    x = torch.arange(5 * 1 * 2 * 3, dtype=torch.float32).reshape(5, 1, 2, 3) + 1
    grid = _make_grid(x, nrow=2)
    assert grid.shape == (3, 3 * 4 + 2, 2 * 5 + 2)                                   # ceil(5 / 2) rows; one channel repeated to three
    for k in range(5):
        y, xx = divmod(k, 2)
        assert torch.equal(grid[:, 2 + 4 * y:4 + 4 * y, 2 + 5 * xx:5 + 5 * xx], x[k].expand(3, 2, 3))
    assert float(grid.sum()) == 3 * float(x.sum())                                   # everything else is the zero padding
    assert torch.equal(_make_grid(x[:1], nrow=4), x[0].expand(3, 2, 3))               # a single image comes back as it is
    assert _make_grid(x.expand(5, 3, 2, 3), nrow=8, padding=0).shape == (3, 2, 15)


def test_use_ema_builds_the_average_and_ema_scope_restores_on_an_exception(monkeypatch, sampler):
    from lvdm.ema import LitEma
    model = _model(monkeypatch, use_ema=True)
    assert model.use_ema and isinstance(model.model_ema, LitEma)
    trainable = {k for k, p in model.model.named_parameters() if p.requires_grad}
    sd = model.state_dict()
    assert {"model_ema.decay", "model_ema.num_updates"} <= set(sd)
    assert {"model_ema." + k.replace(".", "") for k in trainable} == {k for k in sd if k.startswith("model_ema.")} - {"model_ema.decay", "model_ema.num_updates"}
    assert not _model(monkeypatch).use_ema and not hasattr(_model(monkeypatch), "model_ema")
    with torch.no_grad():
        for i, p in enumerate(model.model.parameters()):
            p.add_(0.01 * (i % 7 + 1))                                                # weights != shadows from here on
    before = [p.detach().clone() for p in model.model.parameters()]
    shadows = {k: v.clone() for k, v in model.model_ema.state_dict().items()}
    first = next(model.model.parameters())
    with pytest.raises(KeyError, match="inside"):
        with model.ema_scope("test"):
            assert torch.equal(first, shadows[model.model_ema.m_name2s_name[next(iter(dict(model.model.named_parameters())))]])
            raise KeyError("inside")
    assert all(torch.equal(a, b) for a, b in zip(before, model.model.parameters()))
    assert all(torch.equal(v, model.model_ema.state_dict()[k]) for k, v in shadows.items())
    # log_images samples under the scope: the sampler saw the shadow weights; afterwards the training weights are back
    model.log_images(_batch(), ddim_steps=2)
    assert torch.equal(sampler.calls[0]["weights"], shadows[model.model_ema.m_name2s_name[next(iter(dict(model.model.named_parameters())))]])
    assert all(torch.equal(a, b) for a, b in zip(before, model.model.parameters()))
    # on_train_batch_end: one update
    model.on_train_batch_end()
    assert int(model.model_ema.num_updates) == 1 and not torch.equal(model.model_ema.state_dict()["decay"] * 0 + next(iter(model.model_ema.buffers())), torch.tensor(-1.0))
    name = next(iter(dict(model.model.named_parameters())))
    s0 = shadows[model.model_ema.m_name2s_name[name]]
    omd = 1.0 - min(torch.tensor(0.9999), (1 + torch.tensor(1, dtype=torch.int)) / (10 + torch.tensor(1, dtype=torch.int)))
    assert torch.equal(getattr(model.model_ema, model.model_ema.m_name2s_name[name]), s0 - omd * (s0 - before[0]))


def test_validation_step_adds_the_ema_entries_only_with_use_ema(monkeypatch):
    seen = []

    def forward(self, x, c, **kw):
        seen.append(next(self.model.parameters()).detach().clone())
        return torch.tensor(1.5), {"val/loss": torch.tensor(1.5), "val/loss_simple": torch.tensor(0.5)}

    plain = _model(monkeypatch)
    monkeypatch.setattr(type(plain), "forward", forward)
    assert set(plain.validation_step(_batch())) == {"val/loss", "val/loss_simple"} and len(seen) == 1
    model = _model(monkeypatch, use_ema=True)
    with torch.no_grad():
        next(model.model.parameters()).add_(1.0)
    seen.clear()
    out = model.validation_step(_batch(), 0)
    assert set(out) == {"val/loss", "val/loss_simple", "val/loss_ema", "val/loss_simple_ema"}
    assert len(seen) == 2 and torch.equal(seen[0], seen[1] + 1.0) and torch.equal(next(model.model.parameters()), seen[0])


# ------------------------------------------------------------------------------------------------ sheets and the callback
def test_log_local_on_cpu_tensors_writes_the_reference_s_sheets(tmp_path, monkeypatch):
    from PIL import Image
    import utils.save_video as save_video
    from utils.save_video import log_local, prepare_to_log
    monkeypatch.setattr(save_video, "_video_writer", lambda: None)        # the .npy branch, whether or not torchvision.io imports
    g = golden("validate.pt")
    log = {k: (v.clone() if torch.is_tensor(v) else list(v)) for k, v in g["log_images"]["guided"].items()}
    log["still"] = log["reconst"][:, :, 0] * 1.7                                       # an image entry, beyond [-1, 1]
    log["gray"] = log["reconst"][:, :1, :2].repeat(2, 1, 1, 1, 1)                      # one channel, two samples
    log["latent"] = torch.zeros(1, 4, 2, 8, 8)                                         # neither grayscale nor rgb: skipped
    prepared = prepare_to_log(dict(log), max_images=8, clamp=True)
    assert prepared["samples"].shape[0] == 1 and float(prepared["still"].abs().max()) <= 1.0
    assert prepare_to_log(None) is None and log_local(None, str(tmp_path), "x") is None
    assert prepare_to_log({"a": torch.zeros(5, 3, 2, 2), "c": ["x"] * 5}, max_images=2)["a"].shape[0] == 2
    log_local(prepared, str(tmp_path), "gs0_ep0_idx0_rank0")
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(["condition-gs0_ep0_idx0_rank0.txt", "still-gs0_ep0_idx0_rank0.jpg"]
                           + [f"{k}-gs0_ep0_idx0_rank0.npy" for k in ("image_condition", "reconst", "samples", "gray")])
    assert open(tmp_path / "condition-gs0_ep0_idx0_rank0.txt").read() == "idx=0, txt=a street_fs=10.0\n"
    for key, want in g["sheets"].items():
        got = np.load(tmp_path / f"{key}-gs0_ep0_idx0_rank0.npy")
        assert got.dtype == np.uint8 and got.shape == tuple(want.shape) and np.array_equal(got, want.numpy()), key
    gray = np.load(tmp_path / "gray-gs0_ep0_idx0_rank0.npy")
    assert gray.shape == (2, 128, 64, 3) and np.array_equal(gray[:, :64], gray[:, 64:]) and np.array_equal(gray[..., 0], gray[..., 2])
    assert np.array_equal(gray[:, :64, :, 0], g["sheets"]["reconst"].numpy()[:2, :, :, 0])
    still = np.asarray(Image.open(tmp_path / "still-gs0_ep0_idx0_rank0.jpg"))
    assert still.shape == (64, 64, 3)


class _Module:
    def __init__(self, logdir="somewhere"):
        self.training, self.logdir, self.calls, self.modes = True, logdir, [], []
        self.current_epoch, self.global_step = 2, 40

    def eval(self):
        self.training = False
        self.modes.append("eval")

    def train(self):
        self.training = True
        self.modes.append("train")

    def log_images(self, batch, **kw):
        assert not self.training and not torch.is_grad_enabled()
        self.calls.append(kw)
        return {"samples": torch.zeros(9, 3, 2, 4, 4), "condition": ["c"] * 9}


def test_image_logger_frequency_modes_and_files(tmp_path, monkeypatch):
    import utils.save_video as save_video
    from main.callbacks import ImageLogger
    monkeypatch.setattr(save_video, "_video_writer", lambda: None)
    sig = inspect.signature(ImageLogger.__init__)
    assert list(sig.parameters) == ["self", "batch_frequency", "max_images", "clamp", "rescale", "save_dir", "to_local", "log_images_kwargs"]
    with pytest.raises(NotImplementedError):
        ImageLogger(batch_frequency=3, save_dir=str(tmp_path))
    logger = ImageLogger(batch_frequency=3, max_images=2, save_dir=str(tmp_path), to_local=True,
                         log_images_kwargs={"ddim_steps": 50, "unconditional_guidance_scale": 7.5})
    assert os.path.isdir(tmp_path / "images" / "train") and os.path.isdir(tmp_path / "images" / "val")
    mod = _Module()
    for idx in range(7):
        logger.on_train_batch_end(None, mod, None, {"x": 1}, idx)
    assert mod.calls == [{"split": "train", "ddim_steps": 50, "unconditional_guidance_scale": 7.5}] * 2       # batches 2 and 5
    assert mod.modes == ["eval", "train"] * 2 and mod.training
    names = sorted(os.listdir(tmp_path / "images" / "train"))
    assert [n for n in names if n.endswith(".txt")] == ["condition-gs40_ep2_idx2_rank0.txt", "condition-gs40_ep2_idx5_rank0.txt"]
    assert open(tmp_path / "images" / "train" / names[0]).read() == "idx=0, txt=c\nidx=1, txt=c\n"              # max_images
    assert len(names) == 4
    # validation: every fifth batch; a module in eval mode stays in eval mode
    mod = _Module()
    mod.training = False
    for idx in range(10):
        logger.on_validation_batch_end(None, mod, None, {"x": 1}, idx)
    assert [c["split"] for c in mod.calls] == ["val", "val"] and mod.modes == [] and len(os.listdir(tmp_path / "images" / "val")) == 4
    # switched off: frequency -1, or a module without a logdir
    mod = _Module(logdir=None)
    logger.on_train_batch_end(None, mod, None, {}, 2)
    off = ImageLogger(batch_frequency=-1, save_dir=str(tmp_path), to_local=True)
    off.on_train_batch_end(None, _Module(), None, {}, 0)
    assert mod.calls == []
    # an exception inside log_images still puts the module back into training mode
    mod = _Module()
    mod.log_images = lambda batch, **kw: (_ for _ in ()).throw(RuntimeError("boom"))
    with pytest.raises(RuntimeError, match="boom"):
        logger.on_train_batch_end(None, mod, None, {}, 2)
    assert mod.training


# ------------------------------------------------------------------------------------------------ C-ABI and the optimiser's surface
def test_new_entry_points_are_declared_and_bound():
    from mudg_amd import hip
    from mudg_amd.train import step
    header = open(os.path.join(ROOT, "include", "mudg_hip.h")).read()
    for name, nargs in (("mudg_ema_multi", 4), ("mudg_adamw_ema_multi", 10), ("mudg_swap_multi", 3), ("mudg_log_sheet", 10)):
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, header, re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == nargs
        assert hasattr(hip.lib(), name)
    lib = hip.lib()
    assert lib.mudg_ema_multi(None, 1, 0.1, None) == -1 and lib.mudg_swap_multi(None, 0, None) == -1
    assert lib.mudg_log_sheet(None, None, 1, 3, 1, 1, 1, 1, 1, None) == -1
    assert inspect.signature(step.AdamW.step).parameters["ema"].default is None
    assert inspect.signature(step.training_step).parameters["ema"].default is None


def test_multi_tensor_kernels_use_no_scratch_no_lds_and_16_byte_accesses(tmp_path):
    """Facts about the generated gfx950 code that do not depend on the compiler's scheduling: the six multi-tensor kernels and the
    sheet kernel use neither private memory nor LDS, and the multi-tensor ones address global memory (no flat_* access: the table's
    integers are typed as global pointers) with 16-byte loads and stores."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    multi = ("ema_multi_kernel", "swap_multi_kernel", "adamw_multi_kernel", "adamw_ema_multi_kernel", "adamw_scaled_multi_kernel",
             "adamw_scaled_ema_multi_kernel")
    for src, kernels in (("optim.hip", multi), ("post.hip", ("log_sheet_kernel",))):
        out = tmp_path / (src + ".s")
        subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S",
                        os.path.join(ROOT, "mudg_amd", "csrc", src), "-o", str(out)], check=True, capture_output=True, timeout=600)
        s = out.read_text()
        md = s[s.index("amdhsa.kernels"):]
        seen = set()
        for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", md, re.S):
            for family in kernels:
                if re.search(r"\d%s" % family, m.group(2)):
                    seen.add(family)
                    assert int(m.group(1)) == 0 and int(m.group(3)) == 0, m.groups()
        assert seen == set(kernels), seen
        if src != "optim.hip":
            continue
        for family in kernels:
            (name,) = set(re.findall(r"^(_Z\S*\d%s\S*):" % family, s, re.M))
            body = s[s.index(name + ":"):]
            lines = [l.strip() for l in body[:body.index(".end_amdhsa_kernel")].splitlines()]
            assert not any(l.startswith(("scratch_", "flat_", "ds_read", "ds_write")) for l in lines), family
            assert any(l.startswith("global_load_dwordx4") for l in lines) and any(l.startswith("global_store_dwordx4") for l in lines), family


def test_a_step_that_raises_leaves_the_average_alone_and_a_foreign_average_is_an_error():
    """CPU parameters make AdamW.step raise before any launch: num_updates must not have advanced.  An average built on another
    model instance shares no parameter with the optimiser: an error, not a silent plain step."""
    from lvdm.ema import LitEma
    from mudg_amd.train import step
    g = golden("validate.pt")
    model = ema_model(g["ema_shapes"])
    ema = LitEma(model, decay=0.9)
    opt = step.AdamW([p for p in model.parameters() if p.requires_grad])
    for p in model.parameters():
        if p.requires_grad:
            p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="on the GPU"):
        opt.step(ema=ema)
    assert int(ema.num_updates) == 0 and ema._scalars()[1] == 0
    other = LitEma(ema_model(g["ema_shapes"]), decay=0.9)
    with pytest.raises(RuntimeError, match="another model instance"):
        opt.step(ema=other)
    assert int(other.num_updates) == 0
    # the pairs are walked once and dropped when the average moves or is told to look again
    assert ema.pairs() is ema.pairs() and set(ema.shadow_map()) == {id(p) for p in model.parameters() if p.requires_grad}
    first = ema.pairs()
    ema.to(torch.float32)
    assert ema.pairs() is not first
