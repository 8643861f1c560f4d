"""Shared by tests/test_validate_cpu.py and tests/test_validate_gpu.py: the small parameter set of the LitEma fixture
(tests/golden/make_golden_validate.py builds the same tree for the reference) and its seeded values."""
import torch

from helpers import seeding


def ema_model(shapes):
    """A module tree whose named_parameters() are `shapes` ({dotted name: shape}, in order); names starting with 'frozen' do not
    require a gradient."""
    root = torch.nn.Module()
    for name, shape in shapes.items():
        *path, leaf = name.split(".")
        m = root
        for part in path:
            if part not in m._modules:
                m.add_module(part, torch.nn.Module())
            m = m._modules[part]
        m.register_parameter(leaf, torch.nn.Parameter(torch.zeros(tuple(shape)), requires_grad=not name.startswith("frozen")))
    assert {k: list(v.shape) for k, v in root.named_parameters()} == {k: list(v) for k, v in shapes.items()}
    assert list(dict(root.named_parameters())) == list(shapes)
    return root


def set_params(model, seed, k):
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(seeding.seeded_input("ema:" + name, tuple(p.shape), seed + k))


def replay_ema(g, ema_cls, device="cpu"):
    """The fixture's two runs on `device`: yields ('run12' | 'capped', ema) after each."""
    e = g["ema"]
    model = ema_model(g["ema_shapes"]).to(device)
    set_params(model, g["ema_seed"], -1)
    ema = ema_cls(model, decay=0.9).to(device)
    yield "init", ema
    for k in range(12):
        set_params(model, g["ema_seed"], k)
        ema(model)
    yield "run12", ema
    ema.num_updates.fill_(74)
    ema.resync()
    for k in range(12, 24):
        set_params(model, g["ema_seed"], k)
        ema(model)
    yield "capped", ema
