#!/usr/bin/env python3
"""The image loss of the Gaussian fit (mudg_amd.gaussians.image_loss, csrc/gaussians_loss.hip) on ONE MI355X: what the three
kernels cost, what they replace and what the SSIM term adds to a fit iteration.  Measured, not asserted.

`python tools/gaussians_loss_bench.py [--points 2] [--scale 0.1] [--runs 3] [--no-fit] [--out profiles/gaussians/loss_bench.txt]`

Images: uniform random rgb and targets (V, 3, 576, 1024) with a depth pair (a third of the depth targets zero), V = 1 and V = 3.  Median
[min .. max] of `--runs` runs between device events after a warm-up of: the forward (mudg_gauss_loss), the finish, the backward, and the
whole `image_loss(...).backward()` through autograd; beside them, in the same process, the torch expression `fit` uses at ssim_weight 0
(the mean absolute difference, the masked depth term) with its backward, the same L1 + D-SSIM loss written in torch (F.conv2d with the
11 x 11 window, groups = 3) with its backward, and a device copy of as many bytes as the forward and the backward move (x, y in and
three maps out; x, y and three maps in and one gradient out: 11 N floats).

Fit: one iteration of gaussians.fit on tools/gaussians_fit_bench.py's scene (`--points` million isotropic Gaussians of `--scale` metres,
one 576 x 1024 view) with ssim_weight 0 and 0.2."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import torch.nn.functional as TF

from mudg_amd import gaussians, ops, render
from mudg_amd.synthetic import street_scene
from splat_bench import event_ms, spread

HW = (576, 1024)
SSIM_WEIGHT, DEPTH_WEIGHT = 0.2, 0.1


def fmt(s, unit="ms"):
    return f"{s['median']:.3f} {unit} [{s['min']:.3f} .. {s['max']:.3f}]"


def torch_l1(rgb, targets, depth, depth_targets):
    """The loss of gaussians.fit at ssim_weight 0, as fit writes it."""
    loss = (rgb - targets).abs().mean()
    seen = depth_targets > 0
    return loss + DEPTH_WEIGHT * ((depth - depth_targets).abs() * seen).sum() / seen.sum().clamp(min=1)


def torch_l1_dssim(rgb, targets, depth, depth_targets, window):
    """The rule of DESIGN.md §26 in torch element-wise ops and five grouped convolutions."""
    conv = lambda t: TF.conv2d(t, window, padding=5, groups=3)
    a, m = conv(rgb), conv(targets)
    s1, s2, s12 = conv(rgb * rgb) - a * a, conv(targets * targets) - m * m, conv(rgb * targets) - a * m
    s = ((2 * a * m + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((a * a + m * m + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    seen = depth_targets > 0
    return ((1 - SSIM_WEIGHT) * (rgb - targets).abs().mean() + SSIM_WEIGHT * (1 - s.mean())
            + DEPTH_WEIGHT * ((depth - depth_targets).abs() * seen).sum() / seen.sum().clamp(min=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=float, default=2.0, help="Gaussians in millions (the fit part)")
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussians", "loss_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gaussians_loss_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def timed(fn):
        fn()                                                                                    # warm-up
        torch.cuda.synchronize()
        return spread([event_ms(fn) for _ in range(args.runs)])

    say(f"gaussians_loss_bench on {torch.cuda.get_device_name(0)}: images of {HW[0]} x {HW[1]}, ssim_weight {SSIM_WEIGHT}, depth_weight "
        f"{DEPTH_WEIGHT}; median [min .. max] of {args.runs} runs")
    taps = torch.tensor(ops.SSIM_WINDOW, dtype=torch.float32, device=dev) / 65536.0
    window = torch.outer(taps, taps)[None, None].repeat(3, 1, 1, 1).contiguous()
    gen = torch.Generator(device=dev).manual_seed(3)
    for views in (1, 3):
        rgb = torch.rand((views, 3) + HW, device=dev, generator=gen)
        targets = torch.rand((views, 3) + HW, device=dev, generator=gen)
        depth = torch.rand((views,) + HW, device=dev, generator=gen) * 49 + 1
        depth_targets = (torch.rand((views,) + HW, device=dev, generator=gen) * 49 + 1) * (torch.rand((views,) + HW, device=dev, generator=gen) > 1 / 3)
        up = torch.ones(1, device=dev)
        maps, partial = ops.gauss_loss(rgb, targets, depth, depth_targets)
        totals = ops.gauss_loss_finish(partial, HW, ssim_weight=SSIM_WEIGHT, depth_weight=DEPTH_WEIGHT)
        t_fwd = timed(lambda: ops.gauss_loss(rgb, targets, depth, depth_targets))
        t_fin = timed(lambda: ops.gauss_loss_finish(partial, HW, ssim_weight=SSIM_WEIGHT, depth_weight=DEPTH_WEIGHT))
        t_bwd = timed(lambda: ops.gauss_loss_bwd(rgb, targets, maps, totals, up, depth, depth_targets, ssim_weight=SSIM_WEIGHT, depth_weight=DEPTH_WEIGHT))
        leaf, dleaf = rgb.clone().requires_grad_(True), depth.clone().requires_grad_(True)

        def through(loss_fn):
            def run():
                leaf.grad = dleaf.grad = None
                loss_fn().backward()
            return run

        t_all = timed(through(lambda: gaussians.image_loss(leaf, targets, dleaf, depth_targets, ssim_weight=SSIM_WEIGHT, depth_weight=DEPTH_WEIGHT)))
        t_l1 = timed(through(lambda: torch_l1(leaf, targets, dleaf, depth_targets)))
        t_torch = timed(through(lambda: torch_l1_dssim(leaf, targets, dleaf, depth_targets, window)))
        ours = float(gaussians.image_loss(rgb, targets, depth, depth_targets, ssim_weight=SSIM_WEIGHT, depth_weight=DEPTH_WEIGHT))
        theirs = float(torch_l1_dssim(rgb, targets, depth, depth_targets, window))
        n = rgb.numel()
        src = torch.empty(11 * n // 2, dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)
        t_copy = timed(lambda: dst.copy_(src))
        moved = 11 * n * 4
        say(f" V = {views}: N = {n} values, {partial.shape[0] * partial.shape[1] * partial.shape[2]} partials; forward {fmt(t_fwd)}; finish {fmt(t_fin)}; "
            f"backward {fmt(t_bwd)}; image_loss(...).backward() {fmt(t_all)}; torch L1 with its backward {fmt(t_l1)}; torch L1 + D-SSIM "
            f"(conv2d, groups = 3) with its backward {fmt(t_torch)}; a device copy of the {moved / 2 ** 20:.0f} MiB the two kernels move "
            f"{fmt(t_copy)} ({moved / (t_copy['median'] * 1e-3) / 1e12:.2f} TB/s; the kernels: "
            f"{moved / ((t_fwd['median'] + t_bwd['median']) * 1e-3) / 1e12:.2f} TB/s); loss {ours:.6f} against torch's {theirs:.6f}")
        del rgb, targets, depth, depth_targets, maps, partial, leaf, dleaf, src, dst
        torch.cuda.empty_cache()

    if args.no_fit:
        return
    n = int(args.points * 1e6)
    scene = street_scene(n_background=n, frames=1, seed=11, n_objects=1, object_points=100)
    cloud = render.PointCloud.from_arrays(scene["bg_xyz"], scene["bg_rgb"], dev)
    cam = render.scaled_intrinsics(scene["intr"], scene["hw_native"], HW).astype(np.float32)
    mats = torch.from_numpy(gaussians.scene_matrices(None, np.linalg.inv(scene["c2w"][:1]), 0)).to(dev)
    model = gaussians.GaussianModel.from_cloud(cloud, args.scale, 0.9)
    target = torch.rand((1, 3) + HW, device=dev, generator=gen)
    still = {k: 0.0 for k in gaussians.PARAMETERS}
    t_plain = timed(lambda: gaussians.fit(model, target, mats, cam, HW, iters=1, lr=still))
    t_ssim = timed(lambda: gaussians.fit(model, target, mats, cam, HW, iters=1, lr=still, ssim_weight=SSIM_WEIGHT))
    say(f" one whole fit iteration, {n} isotropic Gaussians of {args.scale} m, one {HW[0]} x {HW[1]} view: ssim_weight 0 {fmt(t_plain)}; "
        f"ssim_weight {SSIM_WEIGHT} {fmt(t_ssim)}")


if __name__ == "__main__":
    main()
