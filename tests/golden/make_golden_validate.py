#!/usr/bin/env python3
"""Capture the validate-while-training fixture from the REFERENCE implementation: LatentVisualDiffusion.log_images
(ddpm3d.py:1186-1265), LitEma (lvdm/ema.py) and the uint8 sheets log_local makes of what log_images returns
(utils/save_video.py:62-136), on the tiny model, towers and seeds of make_golden_batch.py.

Run in the build container only:   python tests/golden/make_golden_validate.py
The reference is imported exactly as make_golden.py imports it (that module is loaded for its stubs and helpers; none of its
goldens is rewritten).  Only data is stored (tests/golden/validate.pt); weights are re-derived from seeding.py on both sides.

  (a) log_images on the B = 4 batch of make_golden_batch.py with ddim_steps=4, ddim_eta=0.0, unconditional_guidance_scale=7.5,
      plot_denoise_rows=False, split="train" and a seeded x_T among the keyword arguments: the only random draws left are the
      VAE posterior noises on the CPU generator (seeded with CPU_SEED right before the call).  The reference cuts the batch to
      one sample in place, so every call gets a batch of its own.
  (b) the same with unconditional_guidance_scale=1.0; its image_condition, reconst and condition are those of (a) (same seed,
      same draws: asserted here) and are stored once.
  (c) LitEma(decay=0.9) on a seeded small parameter set (dotted names, a frozen parameter, sizes that are no multiples of four,
      one tensor longer than two kernel chunks).  Before update k the parameters are set to seeded_input(name, shape,
      EMA_SEED + k).  "run12": 12 updates from num_updates = 0 — all of them in the warm-up, (1 + n) / (10 + n) < 0.9 up to
      n = 79.  "capped": num_updates is then set to 74 and 12 more updates follow (k = 12 .. 23), which cross n = 80, where
      min() starts to return the constructor's decay.  Shadows after each run (the long tensor after the first only, to keep
      the file small), num_updates, the state_dict keys.
  (d) the uint8 sheets of (a)'s tensor entries, formed with the reference's own inline expressions (prepare_to_log's clamp,
      save_video.py:133; the sheet, :91-96): torchvision is a stub here, and make_grid(nrow=1, padding=0) of the samples of one
      frame is their concatenation along the height."""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mgb = _load("make_golden_batch")    # loads make_golden: the reference on sys.path, the no-math stubs installed
mg = mgb.mg
import torch                        # noqa: E402

cfgs, seeding = mg.cfgs, mg.seeding
CPU_SEED = 37
XT_SEED = cfgs.SEED + 13
EMA_SEED = cfgs.SEED + 17
EMA_SHAPES = {"net.0.weight": (7, 5), "net.0.bias": (7,), "net.1.blocks.proj.weight": (3, 3, 3, 3), "wide.weight": (32773,),
              "frozen.weight": (6,)}
LOG_KW = dict(ddim_steps=4, ddim_eta=0.0, plot_denoise_rows=False, split="train")


class _Leaf(torch.nn.Module):
    def __init__(self, shape, trainable=True):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(shape), requires_grad=trainable)


def ema_model():
    """The module tree whose named_parameters() are EMA_SHAPES (tests/test_validate_*.py build the same)."""
    class First(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.zeros(EMA_SHAPES["net.0.weight"]))
            self.bias = torch.nn.Parameter(torch.zeros(EMA_SHAPES["net.0.bias"]))

    class Second(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.blocks = torch.nn.ModuleDict({"proj": _Leaf(EMA_SHAPES["net.1.blocks.proj.weight"])})

    m = torch.nn.Module()
    m.net = torch.nn.Sequential(First(), Second())
    m.wide = _Leaf(EMA_SHAPES["wide.weight"])
    m.frozen = _Leaf(EMA_SHAPES["frozen.weight"], trainable=False)
    assert {k: tuple(v.shape) for k, v in m.named_parameters()} == EMA_SHAPES
    return m


def set_params(model, k):
    for name, p in model.named_parameters():
        p.data.copy_(seeding.seeded_input("ema:" + name, tuple(p.shape), EMA_SEED + k))


def golden_log_images():
    import lvdm.models.ddpm3d as ref_ddpm3d
    ref_ddpm3d.DDIMSampler = mg.CPUSampler            # the reference's sampler without its hard-coded .to('cuda')
    model, meta = mgb.build()
    T = cfgs.UNET_B_SHAPE["T"]
    x_T = seeding.seeded_input("validate_x_T", (1, 4, T, 8, 8), XT_SEED)
    runs = {}
    for tag, scale in (("guided", 7.5), ("plain", 1.0)):
        torch.manual_seed(CPU_SEED)
        log = model.log_images(mgb.make_batch(), unconditional_guidance_scale=scale, x_T=x_T.clone(), **LOG_KW)
        assert set(log) == {"image_condition", "reconst", "condition", "samples"}, set(log)
        runs[tag] = {k: (v.clone() if torch.is_tensor(v) else list(v)) for k, v in log.items()}
    a, b = runs["guided"], runs["plain"]
    assert torch.equal(a["reconst"], b["reconst"]) and torch.equal(a["image_condition"], b["image_condition"]) and a["condition"] == b["condition"]
    assert not torch.equal(a["samples"], b["samples"])
    runs["plain"] = {"samples": b["samples"]}
    return meta, runs


def golden_ema():
    from lvdm.ema import LitEma
    model = ema_model()
    set_params(model, -1)
    ema = LitEma(model, decay=0.9)
    out = {"keys": list(ema.state_dict().keys()), "m_name2s_name": dict(ema.m_name2s_name)}
    for k in range(12):
        set_params(model, k)
        ema(model)
    out["run12"] = {k: v.clone() for k, v in ema.state_dict().items()}
    ema.num_updates.fill_(74)
    for k in range(12, 24):
        set_params(model, k)
        ema(model)
    out["capped"] = {k: v.clone() for k, v in ema.state_dict().items() if k != ema.m_name2s_name["wide.weight"]}
    return out


def sheets(log):
    """save_video.py:133 then :91-96 on every tensor entry (make_grid(nrow=1, padding=0) written out, see the docstring)."""
    out = {}
    for key, value in log.items():
        if not torch.is_tensor(value):
            continue
        value = torch.clamp(value.detach().cpu().float(), -1., 1.)
        video = value.permute(2, 0, 1, 3, 4)                                         # t,n,c,h,w
        frame_grids = [torch.cat(list(framesheet), dim=1) for framesheet in video]   # [3, n*h, 1*w]
        grid = torch.stack(frame_grids, dim=0)
        grid = (grid + 1.0) / 2.0
        out[key] = (grid * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return out


def main():
    meta, runs = golden_log_images()
    path = os.path.join(HERE, "validate.pt")
    torch.save(dict(meta, B=mgb.B, cpu_seed=CPU_SEED, input_seed=mgb.INPUT_SEED, xt_seed=XT_SEED, ema_seed=EMA_SEED,
                    ema_shapes={k: list(v) for k, v in EMA_SHAPES.items()}, log_kwargs={k: v for k, v in LOG_KW.items()},
                    log_images=runs, ema=golden_ema(), sheets=sheets(runs["guided"])), path)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
