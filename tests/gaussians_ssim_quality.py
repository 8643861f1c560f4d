#!/usr/bin/env python3
"""TEST INFRASTRUCTURE, not a test: what the SSIM term of the fit's loss does to a fit on the textured street of §24, on
the GPU: measured, not asserted.  `python tests/gaussians_ssim_quality.py [--out profiles/gaussians/ssim_quality.txt] [--iters 300]`

The street is tools/gaussians_fit_bench.py's: 30000 points on a ground plane and two walls, the target a smooth texture ray-cast per pixel
at 72 x 128.  Every point starts grey (128) at 0.2 m and opacity 0.9, and the fit runs `--iters` iterations against three training poses
(the street's camera and 2 m to either side) once with ssim_weight 0 (the mean absolute difference alone) and once with 0.2, 3DGS's
value, which is not tuned here; one pose is held out (1 m to one side).  Reported for both: PSNR / SSIM (mudg_amd.metrics.psnr_ssim: uint8
frames, valid region, which is not the convention of the training loss) of the inference render of the exported Gaussians against the
target, per pose, and the parts of image_loss on the training views."""
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

SEED_SCALE = 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussians", "ssim_quality.txt"))
    ap.add_argument("--iters", type=int, default=300)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gaussians_ssim_quality: no GPU (the fit has no CPU path)")
    dev = torch.device("cuda:0")
    s = street_scene(n_background=30000, frames=1, seed=5, n_objects=1, object_points=10)
    xyz = s["bg_xyz"]
    cam = render.scaled_intrinsics(s["intr"], s["hw_native"], FIT_HW).astype(np.float32)
    left, right = render.virtual_poses(s["c2w"][0], 2.0, with_ori_pose=False)[:2]
    held = render.virtual_poses(s["c2w"][0], 1.0, with_ori_pose=False)[0]
    poses = np.stack([s["c2w"][0], left, right, held])
    names = ["original", "2 m to one side", "2 m to the other", "1 m to one side (held out)"]
    truth = torch.from_numpy(np.stack([own_image(p, cam, FIT_HW) for p in poses])).to(dev)
    mats = torch.from_numpy(gaussians.scene_matrices(None, np.linalg.inv(poses), 0)).to(dev)
    targets = truth[:3].permute(0, 3, 1, 2).to(torch.float32).div_(255.0).contiguous()
    grey = np.full((len(xyz), 3), 128, np.uint8)
    lines = [f"gaussians_ssim_quality on {torch.cuda.get_device_name(0)}: the textured street, {len(xyz)} grey Gaussians of {SEED_SCALE} m at "
             f"{FIT_HW[0]} x {FIT_HW[1]}, three training poses, {args.iters} iterations"]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def score(tag, model):
        out = gaussians.render(model.gaussians(), mats, cam, FIT_HW)
        frames = torch.floor(out["rgb"] * 255.0 + 0.5).clamp_(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        sc = metrics.psnr_ssim(frames, truth)
        for k, name in enumerate(names):
            say(f"  {tag}, {name}: PSNR {float(sc['psnr'][k]):.2f} dB, SSIM {float(sc['ssim'][k]):.4f}")
        terms = gaussians.image_loss.terms(out["rgb"][:3].contiguous(), targets, ssim_weight=0.2)
        say(f"  {tag}, the training views: mean |x - y| {float(terms['l1']):.5f}, mean S of the training convention {float(terms['ssim']):.5f}")

    for weight in (None, 0.0, 0.2):
        model = gaussians.GaussianModel.from_cloud(render.PointCloud.from_arrays(xyz, grey, dev), SEED_SCALE, 0.9)
        if weight is None:
            score("before", model)
            continue
        losses = gaussians.fit(model, targets, mats[:3].contiguous(), cam, FIT_HW, iters=args.iters, ssim_weight=weight)
        say(f" ssim_weight {weight}: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
        score(f"ssim_weight {weight}", model)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
