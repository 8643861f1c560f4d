#!/usr/bin/env python3
"""Semantic Gaussians (mudg_amd.gaussians with features, csrc/gaussians_feat.hip) on ONE MI355X: what blending, differentiating
and fitting F class scores costs beside the colour-only kernels.  Measured, not asserted; nothing is tuned, and where the time goes inside
a kernel is not claimed without a trace.

`python tools/gaussians_feat_bench.py [--points 2] [--scale 0.1] [--features 19] [--runs 3] [--no-ddim] [--out profiles/gaussians/feat_bench.txt]`

tools/gaussians_fit_bench.py's scene: street_scene's background, `--points` million isotropic Gaussians of `--scale` metres, ONE 576 x 1024
view at the street's first camera, opacity 0.9, and `--features` seeded scores per Gaussian.  Median [min .. max] of `--runs` runs between
device events after a warm-up, in one process: mudg_gauss_blend_feat beside mudg_gauss_blend_train; mudg_gauss_blend_bwd_feat beside
mudg_gauss_blend_bwd; mudg_gauss_feat_bwd; the three kernels of the class loss beside F.cross_entropy with its backward; device copies of
the bytes each must move (stated with their sizes); one whole iteration of gaussians.fit with and without the class term; one DDIM step
of the flagship workload."""
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
from splat_bench import ddim_step_ms, event_ms, spread

HW = (576, 1024)
CLASS_WEIGHT = 0.1


def fmt(s, unit="ms"):
    return f"{s['median']:.3f} {unit} [{s['min']:.3f} .. {s['max']:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=float, default=2.0, help="Gaussians in millions")
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--features", type=int, default=19)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-ddim", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussians", "feat_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gaussians_feat_bench: no GPU (a CPU run measures nothing)")
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

    def copy_of(nbytes):
        src = torch.empty(max(nbytes // 8, 1), dtype=torch.float32, device=dev)                 # half read, half written
        dst = torch.empty_like(src)
        t = timed(lambda: dst.copy_(src))
        return f"a device copy of {nbytes / 2 ** 20:.1f} MiB {fmt(t)}"

    n, F = int(args.points * 1e6), args.features
    say(f"gaussians_feat_bench on {torch.cuda.get_device_name(0)}: one {HW[0]} x {HW[1]} view of the synthetic street, {n} isotropic Gaussians "
        f"of {args.scale} m, opacity 0.9, F = {F} scores each; median [min .. max] of {args.runs} runs")
    scene = street_scene(n_background=n, frames=1, seed=11, n_objects=1, object_points=100)
    cloud = render.PointCloud.from_arrays(scene["bg_xyz"], scene["bg_rgb"], dev)
    cam = render.scaled_intrinsics(scene["intr"], scene["hw_native"], HW).astype(np.float32)
    mats = torch.from_numpy(gaussians.scene_matrices(None, np.linalg.inv(scene["c2w"][:1]), 0)).to(dev)
    model = gaussians.GaussianModel.from_cloud(cloud, args.scale, 0.9)
    gen = torch.Generator(device=dev).manual_seed(3)
    feat = torch.randn((n, F), device=dev, generator=gen)
    with torch.no_grad():
        cov, opacity, colour = model.covariance().contiguous(), model.opacity().contiguous(), model.colour.detach()
    b = gaussians._bin("gaussians_feat_bench", cloud.points, cov, opacity, mats, cam, HW, None, gaussians.ZNEAR, render.ZFAR, gaussians.MAX_ENTRIES)
    E = b.entries
    pixels = HW[0] * HW[1]
    say(f" E = {E} entries; partial is {E * 40 / 2 ** 20:.1f} MiB (E 10 4 bytes), partial_feat {E * F * 4 / 2 ** 20:.1f} MiB (E F 4 bytes), feat_out "
        f"{pixels * F * 4 / 2 ** 20:.1f} MiB, the features {n * F * 4 / 2 ** 20:.1f} MiB")
    entries = (b.uv, b.conic, b.depth, b.values)
    rgb, dimg, alpha, state = ops.gauss_blend_train(colour, *entries, b.ranges, HW)
    _, _, _, feat_out, _ = ops.gauss_blend_feat(colour, feat, *entries, b.ranges, HW)
    t_train = timed(lambda: ops.gauss_blend_train(colour, *entries, b.ranges, HW))
    t_feat = timed(lambda: ops.gauss_blend_feat(colour, feat, *entries, b.ranges, HW))
    say(f" forward: blend_train {fmt(t_train)}; blend_feat {fmt(t_feat)}; {copy_of(E * (48 + 4 * F) + (10 + F) * pixels * 4)} (every entry's 48 + 4 F "
        "bytes staged once, the images, both states)")
    up = (torch.randn_like(rgb) / rgb.numel(), torch.zeros_like(dimg), torch.zeros_like(alpha))
    d_feat = torch.randn_like(feat_out) / feat_out.numel()
    partial, partial_feat = ops.gauss_blend_bwd_feat(colour, feat, *entries, b.order, b.ranges, HW, state, feat_out, *up, d_feat)
    t_bwd = timed(lambda: ops.gauss_blend_bwd(colour, *entries, b.order, b.ranges, HW, state, *up))
    t_bwd_feat = timed(lambda: ops.gauss_blend_bwd_feat(colour, feat, *entries, b.order, b.ranges, HW, state, feat_out, *up, d_feat))
    say(f" backward: blend_bwd {fmt(t_bwd)}, {E / (t_bwd['median'] * 1e-3) / 1e9:.3f} G entries/s; blend_bwd_feat {fmt(t_bwd_feat)}, "
        f"{E / (t_bwd_feat['median'] * 1e-3) / 1e9:.3f} G entries/s; {copy_of(E * (56 + 4 * F) + 2 * E * (40 + 4 * F) + (10 + 2 * F) * pixels * 4)} "
        "(the entries and their order in, both partial buffers zeroed and then written, the states and upstream gradients in)")
    t_gather = timed(lambda: ops.gauss_feat_bwd(b.count, b.offsets, partial_feat))
    say(f" feat_bwd {fmt(t_gather)}; {copy_of(E * F * 4 + n * F * 4 + n * 12)} (partial_feat in, d_features out, count and offsets)")
    labels = torch.randint(0, F + 2, (1,) + HW, device=dev, generator=gen).to(torch.uint8)
    maps, tiles = ops.gauss_class_loss(feat_out, labels)
    totals = ops.gauss_class_loss_finish(tiles, 1, HW, weight=CLASS_WEIGHT)
    one = torch.ones(1, device=dev)
    t_loss = timed(lambda: ops.gauss_class_loss(feat_out, labels))
    t_fin = timed(lambda: ops.gauss_class_loss_finish(tiles, 1, HW, weight=CLASS_WEIGHT))
    t_lbwd = timed(lambda: ops.gauss_class_loss_bwd(maps, totals, one, weight=CLASS_WEIGHT))
    leaf = feat_out.clone().requires_grad_(True)
    target = torch.where(labels < F, labels.long(), torch.full_like(labels.long(), -100))

    def through(loss_fn):
        def run():
            leaf.grad = None
            loss_fn().backward()
        return run

    t_ours = timed(through(lambda: gaussians.class_loss(leaf, labels, weight=CLASS_WEIGHT)))
    t_torch = timed(through(lambda: CLASS_WEIGHT * TF.cross_entropy(leaf, target, ignore_index=-100)))
    ours = float(gaussians.class_loss(feat_out, labels, weight=CLASS_WEIGHT))
    theirs = float(CLASS_WEIGHT * TF.cross_entropy(feat_out, target, ignore_index=-100))
    say(f" class loss: forward {fmt(t_loss)}; finish {fmt(t_fin)}; backward {fmt(t_lbwd)}; class_loss(...).backward() {fmt(t_ours)}; "
        f"F.cross_entropy with its backward {fmt(t_torch)}; {copy_of(4 * pixels * F * 4)} (x in and maps out, maps in and d_x out); loss "
        f"{ours:.6f} against torch's {theirs:.6f}")
    del rgb, dimg, alpha, state, feat_out, partial, partial_feat, maps, leaf, d_feat, up, b, entries
    torch.cuda.empty_cache()
    rgb_target = torch.rand((1, 3) + HW, device=dev, generator=gen)
    still = {k: 0.0 for k in gaussians.PARAMETERS + ("class_logits",)}
    t_plain = timed(lambda: gaussians.fit(model, rgb_target, mats, cam, HW, iters=1, lr=still))
    t_classes = timed(lambda: gaussians.fit(model, rgb_target, mats, cam, HW, iters=1, lr=still, label_targets=labels, class_weight=CLASS_WEIGHT,
                                            classes=F))
    say(f" one whole fit iteration: colour only {fmt(t_plain)}; with the class term {fmt(t_classes)}")
    del model, cloud, cov, opacity, colour, feat, rgb_target, labels
    torch.cuda.empty_cache()
    if not args.no_ddim:
        say(f" one DDIM step of the flagship workload in this process: {fmt(ddim_step_ms(args.runs, dev))}")


if __name__ == "__main__":
    main()
