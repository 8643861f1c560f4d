"""The definition of loss scaling (tests/scaler_reference.py) against torch.amp.GradScaler("cpu") + torch.optim.AdamW + clip_grad_norm_,
and the host side of mudg_amd.train.step.LossScaler: state_dict keys in both directions, enabled=False.  No GPU."""
import math

import numpy as np
import pytest
import torch

import scaler_reference as sr

SHAPES = [(5,), (7, 3), (1,)]
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
# init_scale 4, a growth every 3 good steps by 2^70, back-off 1/2; overflows at steps 2 (NaN), 3 (+inf) and 9 (-inf):
#   step   1   2    3    4  5  6      7  8  9      10 11 12
#   scale  4   2    1    1  1  2^70   .  .  2^69   .  .  2^69 (2^139 is not an fp32 number: the growth is refused, the tracker restarts)
# the growth of step 6 is the first after the two back-offs (the tracker restarted at each of them); steps 4 to 6 run at scale 1.
SCALER = dict(init_scale=4.0, growth_factor=2.0 ** 70, backoff_factor=0.5, growth_interval=3)
OVERFLOWS = {2: float("nan"), 3: float("inf"), 9: float("-inf")}
WANT_SCALES = [4.0, 2.0, 1.0, 1.0, 1.0, 2.0 ** 70, 2.0 ** 70, 2.0 ** 70, 2.0 ** 69, 2.0 ** 69, 2.0 ** 69, 2.0 ** 69]
WANT_TRACKER = [1, 0, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0]


def script():
    """(initial parameters, per step the SCALED fp32 gradients) of the 12-step sequence; the scale of a step is known in advance
    (WANT_SCALES of the step before it), which is what the test then checks."""
    g = torch.Generator().manual_seed(5)
    params = [torch.randn(sh, generator=g).numpy() for sh in SHAPES]
    steps, scale = [], SCALER["init_scale"]
    for k in range(1, 13):
        grads = [(torch.randn(sh, generator=g) * np.float32(scale)).numpy() for sh in SHAPES]
        if k in OVERFLOWS:
            grads[k % len(SHAPES)].reshape(-1)[-1] = OVERFLOWS[k]
        steps.append(grads)
        scale = WANT_SCALES[k - 1]
    return params, steps


@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["noclip", "clip0.5"])
def test_the_definition_follows_torch_through_twelve_steps_with_three_overflows(max_norm):
    params, steps = script()
    run = sr.Run(params, sr.Scaler(**SCALER), max_norm=max_norm, **HYPER)
    taken = 0
    for k, (grads, (scale, tracker, want_p, want_step)) in enumerate(zip(steps, sr.torch_sequence(params, steps, SCALER, max_norm=max_norm, **HYPER)), 1):
        skipped = run.step(grads)
        assert skipped == (k in OVERFLOWS), k
        taken += 0 if skipped else 1
        assert (run.scaler.scale, run.scaler.tracker) == (scale, tracker) == (WANT_SCALES[k - 1], WANT_TRACKER[k - 1]), (k, run.scaler.scale, scale)
        assert run.scaler.taken == want_step == taken, (k, run.scaler.taken, want_step)
        for mine, want in zip(run.p, want_p):
            err = float(np.linalg.norm(mine - want.double().numpy()) / np.linalg.norm(want.double().numpy()))
            assert err < 1e-6, (k, err)
    assert taken == 9 and math.isinf(sr.f32(2.0 ** 69 * SCALER["growth_factor"]))


def test_norm_coefficient_and_overflow_rule():
    g = [np.array([3.0, 4.0], dtype=np.float32) * 8, np.array([12.0], dtype=np.float32) * 8]
    norm, over = sr.norm_and_overflow(g, sr.f32(1 / 8))
    assert (norm, over) == (13.0, False)
    assert sr.clip_coef(norm, None) == 1.0 and sr.clip_coef(norm, 26.0) == 1.0
    assert abs(sr.clip_coef(norm, 6.5) - 0.5) < 1e-7
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert sr.norm_and_overflow([g[0], np.array([bad], dtype=np.float32)], 0.125)[1]
    big = [np.full(1000, np.finfo(np.float32).max, dtype=np.float32)]                  # finite fp32 values never overflow the fp64 sum
    assert not sr.norm_and_overflow(big, 1.0)[1]
    assert sr.Scaler(init_scale=3.0).inv_scale() == float(np.float32(1.0 / 3.0))


def test_state_dict_keys_are_torchs_in_both_directions():
    from mudg_amd.train import step
    mine = step.LossScaler(init_scale=8.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=7)
    theirs = torch.amp.GradScaler("cpu")
    assert set(mine.state_dict()) == set(torch.amp.GradScaler("cpu", init_scale=2.0).state_dict())
    theirs.load_state_dict(mine.state_dict())
    assert theirs.state_dict() == mine.state_dict() == {"scale": 8.0, "growth_factor": 3.0, "backoff_factor": 0.25, "growth_interval": 7,
                                                        "_growth_tracker": 0}
    back = step.LossScaler()
    sd = dict(torch.amp.GradScaler("cpu", init_scale=32.0, growth_interval=11).state_dict(), _growth_tracker=5)     # as out of a checkpoint
    back.load_state_dict(sd)
    assert back.state_dict() == sd and back.get_scale() == 32.0
    with pytest.raises(RuntimeError):
        back.load_state_dict({})


def test_a_disabled_scaler_is_the_identity():
    from mudg_amd.train import step
    off = step.LossScaler(enabled=False)
    loss = torch.ones(3, requires_grad=True).sum()
    assert off.scale(loss) is loss
    p = torch.nn.Parameter(torch.ones(2))
    p.grad = torch.full((2,), 3.0)
    assert off.norm_pass([p]) is None
    off.unscale_([p])
    off.update()
    off.load_state_dict({"anything": 1})
    assert torch.equal(p.grad, torch.full((2,), 3.0))
    assert off.state_dict() == {} == torch.amp.GradScaler("cpu", enabled=False).state_dict() and off.get_scale() == 1.0
