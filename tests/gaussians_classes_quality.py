#!/usr/bin/env python3
"""TEST INFRASTRUCTURE, not a test: what fitting class scores gives on the textured street of §24, on the GPU: measured,
not asserted.  `python tests/gaussians_classes_quality.py [--out profiles/gaussians/classes_quality.txt] [--iters 300]`

The street is tools/gaussians_fit_bench.py's: 30000 points on a ground plane and two walls, the colour target a smooth texture ray-cast per
pixel at 72 x 128.  The label target gives every surface a class (ground 0, the wall at x = -12 1, the wall at x = +12 2) by the same
ray-cast; where a ray leaves the street (sky) the pixel is unlabelled (255).  Every point starts grey (128) at 0.2 m and opacity 0.9 with
zero class scores, and the fit runs `--iters` iterations against three training poses (the street's camera and 2 m to either side) once
on colour alone and once with class_weight 0.1, which is not tuned; one pose is held out (1 m to one side).  Reported: mIoU and pixel
accuracy (mudg_amd.metrics.segmentation_scores) of render's label image against the ray-cast labels per pose, the share of the labelled
pixels the render leaves unlabelled (alpha <= 0.5), and PSNR of both fits per pose beside the PSNR of a repeat of the colour-only fit:
the kernels are deterministic, so the repeat shows that the run-to-run spread is zero and any difference is the class term's.  The
target is synthetic, three planes with one class each: nothing about real scenes follows from these numbers."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from gaussians_fit_bench import FIT_HW, own_image
from mudg_amd import gaussians, metrics, render
from mudg_amd.synthetic import street_scene

SEED_SCALE, CLASS_WEIGHT, CLASSES = 0.2, 0.1, 3


def own_labels(c2w, cam, hw):
    """own_image's ray-cast with the surface's class in place of its texture: ground 0, the walls 1 and 2, 255 where a ray leaves the street."""
    H, W = hw
    fx, fy, cx, cy = (float(v) for v in cam)
    j, i = np.mgrid[0:H, 0:W]
    d = np.stack([(i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, np.ones((H, W))], axis=-1).reshape(-1, 3) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    best, label = np.full(len(d), np.inf), np.full(len(d), 255, np.uint8)
    with np.errstate(all="ignore"):
        for k, (axis, value) in enumerate(((1, 1.6), (0, -12.0), (0, 12.0))):
            t = (value - o[axis]) / d[:, axis]
            p = o + t[:, None] * d
            ok = (t > 0) & (p[:, 2] > -5) & (p[:, 2] < 150) & (p[:, 1] <= 1.6 + 1e-9) & (p[:, 1] > -9) & (np.abs(p[:, 0]) <= 25)
            if axis == 1:
                ok &= np.abs(p[:, 0]) <= 12
            nearer = ok & (t < best)
            best, label = np.where(nearer, t, best), np.where(nearer, np.uint8(k), label)
    return label.reshape(H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussians", "classes_quality.txt"))
    ap.add_argument("--iters", type=int, default=300)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gaussians_classes_quality: no GPU (the fit has no CPU path)")
    dev = torch.device("cuda:0")
    s = street_scene(n_background=30000, frames=1, seed=5, n_objects=1, object_points=10)
    xyz = s["bg_xyz"]
    cam = render.scaled_intrinsics(s["intr"], s["hw_native"], FIT_HW).astype(np.float32)
    left, right = render.virtual_poses(s["c2w"][0], 2.0, with_ori_pose=False)[:2]
    held = render.virtual_poses(s["c2w"][0], 1.0, with_ori_pose=False)[0]
    poses = np.stack([s["c2w"][0], left, right, held])
    names = ["original", "2 m to one side", "2 m to the other", "1 m to one side (held out)"]
    truth = torch.from_numpy(np.stack([own_image(p, cam, FIT_HW) for p in poses])).to(dev)
    labels = torch.from_numpy(np.stack([own_labels(p, cam, FIT_HW) for p in poses])).to(dev)
    mats = torch.from_numpy(gaussians.scene_matrices(None, np.linalg.inv(poses), 0)).to(dev)
    targets = truth[:3].permute(0, 3, 1, 2).to(torch.float32).div_(255.0).contiguous()
    grey = np.full((len(xyz), 3), 128, np.uint8)
    lines = [f"gaussians_classes_quality on {torch.cuda.get_device_name(0)}: the textured street, {len(xyz)} grey Gaussians of {SEED_SCALE} m at "
             f"{FIT_HW[0]} x {FIT_HW[1]}, three training poses, {args.iters} iterations, {CLASSES} classes (ground, two walls), class_weight "
             f"{CLASS_WEIGHT}; labelled share of the pixels per pose {[round(float((l < CLASSES).float().mean()), 4) for l in labels]}.  "
             "A synthetic target: nothing about real scenes follows."]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def psnr(model):
        out = gaussians.render(model.gaussians(), mats, cam, FIT_HW)
        frames = torch.floor(out["rgb"] * 255.0 + 0.5).clamp_(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        return out, [round(float(v), 2) for v in metrics.psnr_ssim(frames, truth)["psnr"]]

    def fit(**kw):
        model = gaussians.GaussianModel.from_cloud(render.PointCloud.from_arrays(xyz, grey, dev), SEED_SCALE, 0.9)
        losses = gaussians.fit(model, targets, mats[:3].contiguous(), cam, FIT_HW, iters=args.iters, **kw)
        return model, losses

    plain, losses = fit()
    _, psnr_plain = psnr(plain)
    say(f" colour only: loss {losses[0]:.4f} -> {losses[-1]:.4f}; PSNR per pose {psnr_plain} dB")
    again, _ = fit()
    _, psnr_again = psnr(again)
    say(f" colour only, repeated: PSNR per pose {psnr_again} dB (run-to-run spread {max(abs(a - b) for a, b in zip(psnr_plain, psnr_again)):.2f} dB)")
    model, losses = fit(label_targets=labels[:3].contiguous(), class_weight=CLASS_WEIGHT, classes=CLASSES)
    out, psnr_classes = psnr(model)
    say(f" colour and classes: loss {losses[0]:.4f} -> {losses[-1]:.4f}; PSNR per pose {psnr_classes} dB (against colour only: "
        f"{[round(a - b, 2) for a, b in zip(psnr_classes, psnr_plain)]} dB)")
    terms = gaussians.class_loss.terms(out["features"][:3].contiguous(), labels[:3].contiguous())
    say(f"  the class loss on the training views after the fit: {float(terms['loss']):.4f} over {int(terms['count'])} labelled pixels "
        f"(log {CLASSES} = {np.log(CLASSES):.4f} at zero scores)")
    sc = metrics.segmentation_scores(out["labels"].to(torch.int64), labels.to(torch.int64), classes=CLASSES)
    for k, name in enumerate(names):
        labelled = labels[k] < CLASSES
        missing = float(((out["labels"][k] == 255) & labelled).sum()) / max(int(labelled.sum()), 1)
        say(f"  {name}: mIoU {float(sc['miou'][k]):.4f}, pixel accuracy {float(sc['pixel_acc'][k]):.4f}, IoU per class "
            f"{[round(float(v), 4) for v in sc['iou'][k]]}; {missing:.4f} of the labelled pixels drawn unlabelled (alpha <= 0.5), "
            f"{int(sc['bad'][k])} predictions outside the classes")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
