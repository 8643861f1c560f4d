#!/usr/bin/env python3
"""TEST INFRASTRUCTURE, not a test: the float64 counterpart of the fit with classes, on the CPU.  It computes the constant
R64_CLASSES that tests/test_gaussians_feat_gpu.py compares the GPU fit with.  `python tests/gaussians_feat_fit64.py`

`class_fit_problem` is gaussians_bwd_reference.fit_problem with labels: a hidden model, the problem's own scene with one of CLASSES classes
per Gaussian (the tercile of its x coordinate) as scores of HIDDEN_SCORE, is rendered in float64 by the textbook renderer; a pixel's label
is the argmax of the blended scores, 255 where alpha <= 0.5.  `class_fit64` then runs torch.optim.Adam in float64 over the textbook
renderer from the problem's start with zero scores: every iteration the mean absolute rgb difference plus CLASS_WEIGHT times
F.cross_entropy over the labelled pixels of the three views.  The ratio is the cross-entropy after ITERS steps over the cross-entropy
before the first."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gaussians_bwd_reference as gb
import gaussians_feat_reference as gf
import gaussians_reference as gr

CLASSES, HIDDEN_SCORE, CLASS_WEIGHT, ITERS, HW = 3, 4.0, 0.1, 200, (40, 56)
CLASS_RATE = 0.05                                     # mudg_amd.gaussians.CLASS_LEARNING_RATE; the GPU test asserts they agree
F = np.float32


def class_fit_problem():
    """fit_problem's (start, views, cam, targets) and labels (3, H, W) uint8."""
    start, views, cam, targets = gb.fit_problem(hw=HW)
    xyz, rgb, cov, opacity, _, _ = gr.seeded_scene(200, HW, 7)
    opacity = np.minimum(opacity, F(0.98))
    order = np.argsort(xyz[:, 0], kind="stable")
    hidden = np.zeros((len(xyz), CLASSES), F)
    hidden[order, (np.arange(len(xyz)) * CLASSES) // len(xyz)] = HIDDEN_SCORE
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=F).astype(np.float64))
    with torch.no_grad():
        _, _, alpha, feat = gf.textbook_features(t64(xyz), t64(rgb), t64(hidden), t64(cov), t64(opacity), views, cam, HW)
    return start, views, cam, targets, gf.labels_of(feat.numpy(), alpha.numpy().astype(F))


def cross_entropy64(feat, labels):
    target = torch.from_numpy(np.where(labels < CLASSES, labels.astype(np.int64), -100))
    return torch.nn.functional.cross_entropy(feat, target, ignore_index=-100)


def class_fit64(start, views, cam, targets, labels, rates, betas, eps, iters=ITERS):
    """The cross-entropy before every step and after the last: iters + 1 values."""
    params = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in start.items()}
    params["class_logits"] = torch.zeros((len(start["xyz"]), CLASSES), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([{"params": [p], "lr": float(CLASS_RATE if k == "class_logits" else rates[k])} for k, p in params.items()], betas=betas, eps=eps)
    draw = lambda: gf.textbook_features(params["xyz"], params["colour"], params["class_logits"], gb.covariance64(params["log_scale"], params["quat"]),
                                        torch.sigmoid(params["opacity_logit"]), views, cam, HW)
    history = []
    for _ in range(iters):
        opt.zero_grad()
        rgb, _, _, feat = draw()
        ce = cross_entropy64(feat, labels)
        ((rgb - targets).abs().mean() + CLASS_WEIGHT * ce).backward()
        opt.step()
        history.append(float(ce.detach()))
    with torch.no_grad():
        history.append(float(cross_entropy64(draw()[3], labels)))
    return history


if __name__ == "__main__":
    from mudg_amd import gaussians
    start, views, cam, targets, labels = class_fit_problem()
    print(f"labels: {[(int((labels == k).sum())) for k in range(CLASSES)]} pixels per class, {int((labels == 255).sum())} unlabelled of {labels.size}")
    history = class_fit64(start, views, cam, targets, labels, gaussians.LEARNING_RATES, gaussians.ADAM_BETAS, gaussians.ADAM_EPS)
    print(f"float64 fit with classes: cross-entropy {history[0]:.5f} -> {history[-1]:.5f} after {ITERS} steps, ratio R64_CLASSES = {history[-1] / history[0]:.5f}")
