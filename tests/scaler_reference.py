"""The definition of loss scaling that mudg_amd.train.step.LossScaler and the scaled AdamW kernels are held to, in plain Python and
float64 (numpy only where a value has to be rounded to fp32 the way the device rounds it):

  update rule     torch's _amp_update_scale_: overflow -> scale *= backoff, tracker = 0; else tracker += 1 and, at growth_interval,
                  scale *= growth unless the product leaves fp32, tracker = 0.  Then taken += not overflow.
  inv_scale       float32(1 / float64(scale))                                    (torch's unscale_)
  norm            sqrt(sum over every gradient element of float64(float32(g * inv_scale)) ** 2)
  overflow rule   the step has overflowed iff that sum is not finite
  coefficient     min(1, max_norm / (float32(norm) + 1e-6)); 1 when no clipping is asked for    (clip_grad_norm_)
  AdamW           torch.optim.AdamW on the gradient float32(float32(g * inv_scale) * coefficient), skipped as a whole on overflow, bias
                  corrections of n = taken + 1

torch_sequence() drives torch.amp.GradScaler + torch.optim.AdamW + clip_grad_norm_ on the CPU through the same steps: the CPU test
holds the definition to it, the GPU test holds the kernels to both."""
import math

import numpy as np
import torch


def f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.float32(x))


class Scaler:
    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.scale, self.tracker, self.taken = f32(init_scale), 0, 0
        self.growth, self.backoff, self.interval = f32(growth_factor), f32(backoff_factor), int(growth_interval)

    def inv_scale(self):
        return f32(1.0 / self.scale)

    def update(self, overflow):
        if overflow:
            self.scale, self.tracker = f32(self.scale * self.backoff), 0
        else:
            self.tracker += 1
            if self.tracker == self.interval:
                grown = f32(self.scale * self.growth)
                if math.isfinite(grown):
                    self.scale = grown
                self.tracker = 0
        self.taken += 0 if overflow else 1


def unscaled(g, inv):
    """float32(g * inv_scale) as a float64 array (g: the scaled fp32 gradient)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(g, dtype=np.float32) * np.float32(inv)).astype(np.float64)


def norm_and_overflow(grads, inv):
    """(norm of the unscaled gradients, whether the step has overflowed) over a list of scaled fp32 gradients."""
    with np.errstate(over="ignore", invalid="ignore"):
        total = float(sum(float(np.sum(unscaled(g, inv) ** 2)) for g in grads))
    return math.sqrt(total), not math.isfinite(total)


def clip_coef(norm, max_norm):
    if max_norm is None:
        return 1.0
    coef = f32(max_norm / f32(f32(norm) + 1e-6))
    return coef if coef < 1.0 else 1.0


def consumed(g, inv, coef):
    """The gradient the optimiser consumes: each of the two products rounded to fp32 on its own."""
    with np.errstate(over="ignore", invalid="ignore"):
        return ((np.asarray(g, dtype=np.float32) * np.float32(inv)) * np.float32(coef)).astype(np.float64)


def adamw(p, g, m, v, n, lr, betas, eps, weight_decay):
    """One torch.optim.AdamW step in float64, step count n >= 1; returns (p, m, v)."""
    b1, b2 = betas
    p = p * (1.0 - lr * weight_decay)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v) / math.sqrt(1.0 - b2 ** n) + eps
    return p - (lr / (1.0 - b1 ** n)) * (m / denom), m, v


def ema(s, p, one_minus_decay):
    return s - one_minus_decay * (s - p)


class Run:
    """Parameters, moments and the scaler of the definition, stepped with scaled fp32 gradients."""

    def __init__(self, params, scaler, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None):
        self.p = [np.asarray(p, dtype=np.float64).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.scaler, self.hyper, self.max_norm = scaler, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), max_norm
        self.norm = self.coef = None

    def step(self, grads):
        """Returns whether the step was skipped."""
        inv = self.scaler.inv_scale()
        self.norm, overflow = norm_and_overflow(grads, inv)
        self.coef = clip_coef(self.norm, self.max_norm)
        if not overflow:
            n = self.scaler.taken + 1
            for i, g in enumerate(grads):
                self.p[i], self.m[i], self.v[i] = adamw(self.p[i], consumed(g, inv, self.coef), self.m[i], self.v[i], n, **self.hyper)
        self.scaler.update(overflow)
        return overflow


def torch_sequence(params, grads_per_step, scaler_kwargs, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None):
    """torch's own loop on the CPU: for every step the scaled gradients are assigned, then unscale_ -> clip_grad_norm_ -> step ->
    update.  Yields after every step (scale, growth tracker, [parameters], state["step"] of the first parameter or 0)."""
    ps = [torch.nn.Parameter(torch.as_tensor(np.asarray(p), dtype=torch.float32).clone()) for p in params]
    opt = torch.optim.AdamW(ps, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    scaler = torch.amp.GradScaler("cpu", **scaler_kwargs)
    scaler.scale(torch.zeros(1))                               # (creates the scale and the tracker)
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = torch.as_tensor(np.asarray(g), dtype=torch.float32).clone()
        scaler.unscale_(opt)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        scaler.step(opt)
        scaler.update()
        st = opt.state[ps[0]]
        yield scaler.get_scale(), scaler._get_growth_tracker(), [p.detach().clone() for p in ps], int(st["step"]) if st else 0
