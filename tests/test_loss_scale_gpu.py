"""Loss scaling on the GPU (mudg_amd.train.step.LossScaler; csrc/optim.hip: mudg_scaled_grad_norm, mudg_adamw_scaled_multi,
mudg_adamw_scaled_ema_multi, mudg_loss_scale_update) against the definition in tests/scaler_reference.py and the torch sequence it
is held to on the CPU.  The file runs in the loaded build directly and once more in a child process in the fp16 build, the build the
feature is for (the operand type is fixed per process).

  norm pass       norm, coefficient and overflow flag over ragged sizes and an unaligned view; the gradients are not written
  scaled AdamW    equals the plain optimiser fed the unscaled gradients (plain / EMA, clipped / unclipped); the consumed gradient exact
  skip            an inf in one tensor leaves every parameter and moment alone; shadows, scale, tracker, counts; resume from a state_dict
  no round trip   a whole training_step under torch's synchronisation debug mode
  purpose         a Linear whose output gradient underflows the fp16 operand: zero gradients without the scaler, right ones with it
  whole step      two scaled steps of the tiny UNet against two plain ones"""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

import scaler_reference as sr
from helpers import ChildRuns, cfgs, golden, rel_l2, seeded_sd, unet_inputs
from mudg_amd import hip
from test_training_gpu import MODE, TOL, TOL_NET, check, rnd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.environ.get("MUDG_PARITY_CHILD") == "1"
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
BAD = [float("nan"), float("inf"), float("-inf")]


def record(scaler):
    """(scale, tracker, overflow flag, taken steps) read back from the device."""
    r = scaler._rec.cpu()
    return float(r.view(torch.float32)[0]), int(r[1]), int(r[2]), int(r[3])


def unaligned(values, dev):
    """`values` at an element offset of 1 inside a flat buffer: 4 bytes off every 16-byte boundary."""
    flat = torch.zeros(values.numel() + 1, device=dev)
    view = flat[1:].view(values.shape)
    view.copy_(values)
    assert view.data_ptr() % 16 == 4
    return view


# ------------------------------------------------------------------------------------------------ 1. the norm pass
NORM_SHAPES = [(1,), (3,), (5,), (300, 7), (16384,), (16385,), (40000,)]
UNALIGNED = len(NORM_SHAPES)                              # index of the gradient that sits in the flat buffer (1027 values)


def norm_problem(dev, scale):
    shapes = NORM_SHAPES + [(1027,)]
    values = [rnd(*sh, seed=40 + i) * np.float32(scale) for i, sh in enumerate(shapes)]
    params = [torch.nn.Parameter(torch.zeros(sh, device=dev)) for sh in shapes]
    for i, (p, g) in enumerate(zip(params, values)):
        p.grad = unaligned(g.to(dev), dev) if i == UNALIGNED else g.to(dev)
    return params, values


@pytest.mark.parametrize("scale", [65536.0, 3.0], ids=["scale65536", "scale3"])
def test_norm_pass_gives_the_unscaled_norm_the_coefficient_and_a_clear_flag_and_writes_no_gradient(cuda, scale):
    from mudg_amd.train import step
    params, values = norm_problem(cuda, scale)
    scaler = step.LossScaler(init_scale=scale)
    inv = sr.Scaler(init_scale=scale).inv_scale()
    want, over = sr.norm_and_overflow([v.numpy() for v in values], inv)
    assert not over
    before = [p.grad.clone() for p in params]
    for max_norm in (None, 2.0 * want, 0.5 * want, 0.5):                   # off, above the norm (untouched), below it (clipped) twice
        stat = scaler.norm_pass(params, max_norm).cpu()
        coef = sr.clip_coef(want, max_norm)
        print(f"[{MODE}] scale {scale:g} max_norm {max_norm}: norm {float(stat[0]):.9g} (definition {want:.9g}), coefficient {float(stat[1]):.9g} ({coef:.9g})")
        assert abs(float(stat[0]) - want) <= 1e-6 * want
        assert abs(float(stat[1]) - coef) <= 1e-6 * coef
        assert (float(stat[1]) == 1.0) == (max_norm is None or max_norm >= want)
        assert record(scaler) == (scale, 0, 0, 0)
    for p, b in zip(params, before):
        assert torch.equal(p.grad, b)
    assert params[UNALIGNED].grad.data_ptr() % 16 == 4


# (tensor index, element index): the first element of all, the last element of a full chunk, a 3-element tail, the unaligned tensor
PLACES = {"first": (0, 0), "chunk-end": (5, 16383), "tail3": (1, 2), "unaligned": (UNALIGNED, 513)}


@pytest.mark.parametrize("place", list(PLACES))
def test_norm_pass_raises_the_flag_for_nan_and_both_infinities_wherever_they_sit(cuda, place):
    from mudg_amd.train import step
    params, _ = norm_problem(cuda, 65536.0)
    scaler = step.LossScaler()
    ti, ei = PLACES[place]
    flat = params[ti].grad.view(-1)
    good = flat[ei].clone()
    for bad in BAD:
        flat[ei] = bad
        before = [p.grad.clone() for p in params]
        stat = scaler.norm_pass(params, 0.5).cpu()
        assert record(scaler)[2] == 1, (place, bad)
        assert not math.isfinite(float(stat[0]))
        for p, b in zip(params, before):
            assert torch.equal(p.grad.view(torch.int32), b.view(torch.int32))                  # (bit patterns: NaN != NaN)
        flat[ei] = good
        scaler.norm_pass(params, 0.5)
        assert record(scaler)[2] == 0, (place, bad)


# ------------------------------------------------------------------------------------------------ 2. / 3. the scaled optimiser
class Bag(torch.nn.Module):
    """Parameters of ragged sizes: aligned ones, one whose GRADIENT sits unaligned in a flat buffer, one that is unaligned itself."""
    SHAPES = [(5,), (300, 7), (16385,), (3,), (1027,), (515,)]
    GRAD_UNALIGNED, ALL_UNALIGNED = 4, 5

    def __init__(self, dev):
        super().__init__()
        values = [rnd(*sh, seed=60 + i).to(dev) for i, sh in enumerate(self.SHAPES)]
        values[self.ALL_UNALIGNED] = unaligned(values[self.ALL_UNALIGNED], dev)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(v) for v in values])
        assert self.ps[self.ALL_UNALIGNED].data_ptr() % 16 == 4

    def assign(self, grads, dev):
        for i, (p, g) in enumerate(zip(self.ps, grads)):
            g = g.to(dev)
            p.grad = unaligned(g, dev) if i in (self.GRAD_UNALIGNED, self.ALL_UNALIGNED) else g.clone()


def grads_of(k):
    return [rnd(*sh, seed=100 * k + i) for i, sh in enumerate(Bag.SHAPES)]


def optimiser(dev, with_ema):
    from lvdm.ema import LitEma
    from mudg_amd.train import step
    bag = Bag(dev)
    ema = LitEma(bag, decay=0.9).to(dev) if with_ema else None
    return bag, step.AdamW(list(bag.ps), **HYPER), ema


def moments(opt, bag):
    return [opt.state[p][k] for p in bag.ps for k in ("exp_avg", "exp_avg_sq")]


@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["noclip", "clip0.5"])
def test_scaled_adamw_equals_the_plain_optimiser_fed_the_unscaled_gradients(cuda, max_norm, with_ema):
    from mudg_amd.train import step
    mine, opt, ema = optimiser(cuda, with_ema)
    ref, ropt, rema = optimiser(cuda, with_ema)
    scaler = step.LossScaler()
    clip = step.GradientClipper(list(ref.ps), max_norm) if max_norm is not None else None
    for k in range(1, 4):
        g = grads_of(k)
        mine.assign([x * 65536.0 for x in g], cuda)
        ref.assign(g, cuda)
        for p, x in zip(mine.ps, g):                                        # the consumed gradient, before clipping: exact
            c = p.grad.clone()
            scaler.unscale_([c])
            assert torch.equal(c.cpu(), x)
        stat = scaler.norm_pass(list(mine.ps), max_norm)
        opt.step(ema=ema, scaler=scaler)
        scaler.update()
        rstat = clip() if clip is not None else None
        ropt.step(ema=rema)
        if rstat is not None:
            assert abs(float(stat[0]) - float(rstat[0])) <= 1e-6 * float(rstat[0]) and float(stat[1]) < 1.0
    assert record(scaler) == (65536.0, 3, 0, 3)
    for i, (p, q) in enumerate(zip(mine.ps, ref.ps)):
        check(f"parameter {i} after 3 scaled steps", p, q, 1e-6)
    for i, (a, b) in enumerate(zip(moments(opt, mine), moments(ropt, ref))):
        check(f"moment {i}", a, b, 1e-6)
    if with_ema:
        for i, ((_, s), (_, t)) in enumerate(zip(ema.pairs(), rema.pairs())):
            check(f"shadow {i}", s, t, 1e-6)
        assert int(ema.num_updates) == int(rema.num_updates) == 3


@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
def test_an_overflow_skips_the_step_on_the_device_and_the_next_one_counts_from_the_steps_taken(cuda, with_ema):
    from mudg_amd.train import step
    bag, opt, ema = optimiser(cuda, with_ema)
    scaler = step.LossScaler()
    start = [p.detach().cpu().numpy().copy() for p in bag.ps]
    scales = [65536.0, 65536.0, 32768.0]
    steps = []
    for k in range(1, 4):
        g = [(x * np.float32(scales[k - 1])).numpy() for x in grads_of(k)]
        if k == 2:
            g[1].reshape(-1)[777] = float("inf")
        steps.append(g)

    def run(k):
        bag.assign([torch.from_numpy(x) for x in steps[k - 1]], cuda)
        scaler.norm_pass(list(bag.ps), 0.5)
        opt.step(ema=ema, scaler=scaler)
        scaler.update()

    run(1)
    assert record(scaler) == (65536.0, 1, 0, 1)
    held = [t.clone() for t in list(bag.ps) + moments(opt, bag)]
    versions = [p._version for p in bag.ps]
    shadows = [s.clone() for _, s in ema.pairs()] if with_ema else []
    run(2)
    for i, (t, h) in enumerate(zip(list(bag.ps) + moments(opt, bag), held)):
        assert torch.equal(t, h), f"tensor {i} changed in a skipped step"
    assert all(p._version > v for p, v in zip(bag.ps, versions))           # bumped on a skipped step too: no decision on the flag
    assert record(scaler) == (32768.0, 0, 0, 1) and scaler.get_scale() == 32768.0 and scaler.taken_steps() == 1
    if with_ema:                                                            # LitEma.forward's update of the unchanged parameters, update 2
        n = torch.tensor(2, dtype=torch.int)
        omd = torch.tensor(float(1.0 - min(torch.tensor(0.9), (1 + n) / (10 + n))), device=cuda)
        for (p, s), s0 in zip(ema.pairs(), shadows):
            assert torch.equal(s, s0 - omd * (s0 - p))
        assert int(ema.num_updates) == 2
    run(3)
    assert record(scaler) == (32768.0, 1, 0, 2)
    assert all(opt.state[p]["step"] == 3 for p in bag.ps)                   # the host counts attempts
    sd = opt.state_dict()
    assert [sd["state"][i]["step"] for i in range(len(bag.ps))] == [2] * len(bag.ps)
    # the definition, and torch's own sequence on the CPU: step 3 ran with the bias corrections of n = 2
    want = sr.Run(start, sr.Scaler(), max_norm=0.5, **HYPER)
    skipped = [want.step(g) for g in steps]
    assert skipped == [False, True, False] and want.scaler.taken == 2
    *_, (scale, tracker, torch_p, torch_step) = sr.torch_sequence(start, steps, {}, max_norm=0.5, **HYPER)
    assert (scale, tracker, torch_step) == (32768.0, 1, 2)
    for i, p in enumerate(bag.ps):
        check(f"parameter {i} against the definition", p, torch.from_numpy(want.p[i]), 1e-6)
        check(f"parameter {i} against torch", p, torch_p[i], 1e-6)
    # resume: a fresh optimiser and scaler loaded from the state continue identically
    again, opt2, ema2 = optimiser(cuda, with_ema)
    with torch.no_grad():
        for a, p in zip(again.ps, bag.ps):
            a.copy_(p)
    if with_ema:
        ema2.load_state_dict(copy.deepcopy(ema.state_dict()))
    opt2.load_state_dict(copy.deepcopy(sd))
    scaler2 = step.LossScaler()
    scaler2.load_state_dict(scaler.state_dict())
    g4 = [x * 32768.0 for x in grads_of(4)]
    for b, o, e, s in ((bag, opt, ema, scaler), (again, opt2, ema2, scaler2)):
        b.assign(g4, cuda)
        s.norm_pass(list(b.ps), 0.5)
        o.step(ema=e, scaler=s)
        s.update()
    assert record(scaler2) == record(scaler) == (32768.0, 2, 0, 3)
    for i, (a, p) in enumerate(zip(again.ps, bag.ps)):
        assert torch.equal(a, p), f"parameter {i} after the resumed step"
    for a, b in zip(moments(opt2, again), moments(opt, bag)):
        assert torch.equal(a, b)


def test_parameters_at_different_step_counts_and_a_missing_norm_pass_are_refused(cuda):
    from mudg_amd.train import step
    bag, opt, _ = optimiser(cuda, False)
    scaler = step.LossScaler()
    bag.assign(grads_of(1), cuda)
    with pytest.raises(RuntimeError, match="norm_pass"):
        opt.step(scaler=scaler)
    for p in list(bag.ps)[1:]:
        p.grad = None
    opt.step()                                                              # the first parameter alone is now one step ahead
    bag.assign(grads_of(2), cuda)
    scaler.norm_pass(list(bag.ps))
    with pytest.raises(NotImplementedError, match="different step counts"):
        opt.step(scaler=scaler)
    bag2, opt2, _ = optimiser(cuda, False)
    bag2.assign(grads_of(1), cuda)
    scaler2 = step.LossScaler()
    scaler2.unscale_(list(bag2.ps))
    scaler2.norm_pass(list(bag2.ps))
    with pytest.raises(RuntimeError, match="already unscaled"):
        opt2.step(scaler=scaler2)


# ------------------------------------------------------------------------------------------------ the tiny model
def _tiny_model(cuda):
    from lvdm.models.ddpm3d import LatentVisualDiffusion
    g = golden("unet_b.pt")
    ident = {"target": "torch.nn.Identity"}
    model = LatentVisualDiffusion(
        img_cond_stage_config=ident, image_proj_stage_config=ident, cond_stage_config=ident, first_stage_config=ident,
        unet_config={"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": g["cfg"]}, **cfgs.DIFFUSION)
    sd = seeded_sd(g["param_shapes"], g["seed"], g["checksum"])
    model.model.diffusion_model.load_state_dict(sd, strict=True)
    model = model.to(cuda).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.learning_rate = 2e-4
    return model, g


def _inputs(g, cuda):
    shp = g["shape"]
    x, ctx = unet_inputs(g["cfg"], shp, g["seed"])
    return dict(x_start=x[:, :4].contiguous().to(cuda), cond={"c_crossattn": [ctx.to(cuda)], "c_concat": [x[:, 4:].contiguous().to(cuda)]},
                t=torch.tensor([700, 420, 100])[:shp["B"]].to(cuda), noise=rnd(shp["B"], 4, shp["T"], shp["H"], shp["W"], seed=3).to(cuda),
                class_label=torch.tensor([0, 500, 1])[:shp["B"], None].to(cuda), fs=torch.full((shp["B"],), 10).to(cuda))


# ------------------------------------------------------------------------------------------------ 4. no host round trip
def test_a_whole_scaled_training_step_never_waits_for_the_device(cuda):
    from lvdm.ema import LitEma
    from mudg_amd.train import step
    model, g = _tiny_model(cuda)
    inp = _inputs(g, cuda)
    opt = model.configure_optimizers()
    params = [p for group in opt.param_groups for p in group["params"]]
    ema = LitEma(model.model, decay=0.9999).to(cuda)
    clip, scaler = step.GradientClipper(params, 0.5), step.LossScaler()
    step.training_step(model, optimizer=opt, clipper=clip, ema=ema, scaler=scaler, **inp)          # builds the tables, packs, plans
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, info = step.training_step(model, optimizer=opt, clipper=clip, ema=ema, scaler=scaler, **inp)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert info["loss_scale"].is_cuda and info["grad_norm"].is_cuda and math.isfinite(float(loss))
    scale, tracker, flag, taken = record(scaler)
    print(f"[{MODE}] two scaled steps of the tiny UNet at 2^16: scale {scale:g}, tracker {tracker}, taken {taken}, second step ran at "
          f"{float(info['loss_scale']):g} with unscaled gradient norm {float(info['grad_norm']):.4e}")
    # (an overflow of the first steps at 2^16 is the scaler at work, not a failure: every step either counted or halved the scale)
    assert flag == 0 and 0 <= taken <= 2 and scale == 65536.0 * 0.5 ** (2 - taken) and tracker <= taken


# ------------------------------------------------------------------------------------------------ 5. what the feature is for
def test_a_linear_whose_output_gradient_underflows_the_fp16_operand_gets_its_gradients_back_under_the_scaler(cuda):
    """dy = +-2^-28 (1 + u), u in [0, 1): below half of fp16's smallest subnormal (2^-24), so the fp16 operand of the backward GEMMs is
    zero whatever the MFMA does with subnormals; times 2^16 it is a normal number.  Asserted in the fp16 build, printed in the others
    (bf16 has fp32's exponent range)."""
    from mudg_amd.train import functions as Fn
    from mudg_amd.train import step
    gen = torch.Generator().manual_seed(11)
    x0, w0 = rnd(256, 64, seed=1), rnd(64, 64, seed=2, scale=0.1)
    sign = torch.where(torch.rand((256, 64), generator=gen) < 0.5, -1.0, 1.0)
    dy = (sign * 2.0 ** -28 * (1.0 + torch.rand((256, 64), generator=gen))).float()
    want_x, want_w = dy.double() @ w0.double(), dy.double().t() @ x0.double()

    def backward(upstream, scaler):
        x, w = torch.nn.Parameter(x0.to(cuda)), torch.nn.Parameter(w0.to(cuda))
        loss = (Fn.Linear.apply(x, w, None, None) * upstream.to(cuda)).sum()
        (loss if scaler is None else scaler.scale(loss)).backward()
        return x, w

    x, w = backward(dy, None)
    zero = not bool(x.grad.any()) and not bool(w.grad.any())
    print(f"[{MODE}] Linear backward of a 2^-28 output gradient without a scaler: max |dx| {float(x.grad.abs().max()):.3e}, "
          f"max |dW| {float(w.grad.abs().max()):.3e} (fp64: {float(want_x.abs().max()):.3e}, {float(want_w.abs().max()):.3e})")
    scaler = step.LossScaler()
    x, w = backward(dy, scaler)
    scaler.norm_pass([x, w])
    flag = record(scaler)[2]
    got = [x.grad.clone(), w.grad.clone()]
    scaler.unscale_(got)
    errs = [rel_l2(got[0], want_x), rel_l2(got[1], want_w)]
    print(f"[{MODE}] with LossScaler(): rel-L2 of dx {errs[0]:.3e}, of dW {errs[1]:.3e} (bound {TOL:g}), overflow flag {flag}")
    over = step.LossScaler()
    big = dy.clone()
    big[3, 5] = 1e6                                                         # times 2^16 beyond 65504: the operand cast gives inf
    x, w = backward(big, over)
    over.norm_pass([x, w])
    print(f"[{MODE}] an output gradient of 1e6 at scale 2^16: overflow flag {record(over)[2]}")
    if MODE == "fp16":
        assert zero, "the unscaled gradients were expected to be exactly zero in the fp16 build"
        assert flag == 0 and errs[0] < TOL and errs[1] < TOL
        assert record(over)[2] == 1


# ------------------------------------------------------------------------------------------------ 6. the whole step
def test_two_scaled_steps_of_the_tiny_unet_equal_two_plain_ones(cuda):
    """A power-of-two scale commutes with every operand rounding and every fp32 sum as long as nothing leaves the normal range: the
    gradients are expected identical, the parameters then differ by the device's powf against the host's at most.  Measured: bf16 build
    all 644 tensors bit-equal (against the plain run and between two scales); fp16 build 0 of 644, 2.2e-4 rel-L2 from the plain run — the
    small elements of an output gradient are fp16 subnormals at one scale and normal numbers at the next."""
    from mudg_amd.train import step
    out = {}
    for name, scaler in (("plain", None), ("x4096", step.LossScaler(init_scale=4096.0)), ("scaled", step.LossScaler(init_scale=1024.0))):
        model, g = _tiny_model(cuda)
        inp = _inputs(g, cuda)
        opt = model.configure_optimizers()
        for _ in range(2):
            loss, info = step.training_step(model, optimizer=opt, scaler=scaler, **inp)
        out[name] = ([p.detach().clone() for p in model.model.diffusion_model.parameters()], loss)
    assert record(scaler) == (1024.0, 2, 0, 2) and float(info["loss_scale"]) == 1024.0
    num = sum(float((a.double() - b.double()).pow(2).sum()) for a, b in zip(out["scaled"][0], out["plain"][0]))
    den = sum(float(b.double().pow(2).sum()) for b in out["plain"][0])
    same = sum(bool(torch.equal(a, b)) for a, b in zip(out["scaled"][0], out["plain"][0]))
    err = math.sqrt(num / den)
    # two scales against each other: both runs keep the output gradients in the operand type's normal range, the plain run need not
    # (the fp16 build rounds the small ones as subnormals: the defect the scaler is for), so THIS is the homogeneity check there
    scales_same = sum(bool(torch.equal(a, b)) for a, b in zip(out["scaled"][0], out["x4096"][0]))
    print(f"[{MODE}] two steps at scale 1024 against two at scale 4096: {scales_same} of {len(out['plain'][0])} tensors bit-equal")
    print(f"[{MODE}] two scaled steps against two plain ones: parameters rel-L2 {err:.3e} (bound {TOL_NET:g}), {same} of {len(out['plain'][0])} "
          f"tensors bit-equal; loss {float(out['scaled'][1]):.6f} against {float(out['plain'][1]):.6f}")
    assert err < TOL_NET


# ------------------------------------------------------------------------------------------------ the fp16 build
if not CHILD and MODE != "fp16":
    @pytest.fixture(scope="module")
    def children():
        runs = ChildRuns(workers=1)
        env = dict(os.environ, MUDG_PARITY_CHILD="1", MUDG_OPERAND="fp16")
        runs.submit("fp16", [sys.executable, "-m", "pytest", "tests/test_loss_scale_gpu.py", "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider"], ROOT, env, 600)
        yield runs
        runs.shutdown()

    def test_this_file_in_the_fp16_build(cuda, children):
        rc, stdout = children.result("fp16")
        print("\n".join(l for l in stdout.splitlines() if "[fp16]" in l or "passed" in l or "failed" in l or l.startswith("[child")))
        assert rc == 0, stdout[-6000:]
