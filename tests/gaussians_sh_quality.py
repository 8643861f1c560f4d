#!/usr/bin/env python3
"""TEST INFRASTRUCTURE, not a test: what spherical harmonics do to a fit whose target depends on the direction it is seen
from, on the GPU: measured, not asserted.  `python tests/gaussians_sh_quality.py [--out profiles/gaussians/sh_quality.txt] [--iters 300]`

The street is tools/gaussians_fit_bench.py's: 30000 points on a ground plane and two walls at 72 x 128.  The target is view-dependent: the
points carry the street's texture as their colour and seeded coefficients of degrees 1 and 2 (uniform in +-`--amplitude` byte units), and
the four target frames are that textured cloud drawn by the inference renderer with the rule of §27, which tests/test_gaussians_sh_gpu.py
holds bit-equal to the numpy definition of tests/gaussians_sh_reference.py (the definition itself walks every entry in Python; at this
size it would take the better part of an hour).  The fit starts from constant-colour seeds (grey, 128) at the same positions, 0.2 m and
opacity 0.9, and runs `--iters` iterations against three training poses (the street's camera and 2 m to either side) once with
sh_degree 0 and once with 2, all degrees from the first iteration; one pose is held out (1 m to one side).  Reported for both: PSNR /
SSIM (mudg_amd.metrics.psnr_ssim) of the inference render of the exported Gaussians against the target, per pose."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from gaussians_fit_bench import FIT_HW, texture
from mudg_amd import gaussians, metrics, render
from mudg_amd.synthetic import street_scene

SEED_SCALE = 0.2
DEGREE = 2


def frames_of(g, mats, cam):
    out = gaussians.render(g, mats, cam, FIT_HW)
    return torch.floor(out["rgb"] * 255.0 + 0.5).clamp_(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussians", "sh_quality.txt"))
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--amplitude", type=float, default=60.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gaussians_sh_quality: no GPU (the fit has no CPU path)")
    dev = torch.device("cuda:0")
    s = street_scene(n_background=30000, frames=1, seed=5, n_objects=1, object_points=10)
    xyz = s["bg_xyz"]
    n = len(xyz)
    cam = render.scaled_intrinsics(s["intr"], s["hw_native"], FIT_HW).astype(np.float32)
    left, right = render.virtual_poses(s["c2w"][0], 2.0, with_ori_pose=False)[:2]
    held = render.virtual_poses(s["c2w"][0], 1.0, with_ori_pose=False)[0]
    poses = np.stack([s["c2w"][0], left, right, held])
    names = ["original", "2 m to one side", "2 m to the other", "1 m to one side (held out)"]
    mats = torch.from_numpy(gaussians.scene_matrices(None, np.linalg.inv(poses), 0)).to(dev)
    coefficients = np.random.default_rng(27).uniform(-args.amplitude, args.amplitude, (n, (DEGREE + 1) ** 2 - 1, 3)).astype(np.float32)
    textured = gaussians.Gaussians.from_cloud(render.PointCloud.from_arrays(xyz, texture(xyz), dev), SEED_SCALE, 0.9)
    textured = gaussians.Gaussians(textured.cloud, textured.cov, textured.opacity, sh=torch.from_numpy(coefficients).to(dev))
    truth = frames_of(textured, mats, cam)
    targets = truth[:3].permute(0, 3, 1, 2).to(torch.float32).div_(255.0).contiguous()
    plain = frames_of(gaussians.Gaussians(textured.cloud, textured.cov, textured.opacity), mats, cam)
    spread = float((truth.float() - plain.float()).abs().mean())                               # what the coefficients change in the frames
    grey = np.full((n, 3), 128, np.uint8)
    lines = [f"gaussians_sh_quality on {torch.cuda.get_device_name(0)}: the textured street with seeded degree-{DEGREE} coefficients of +-"
             f"{args.amplitude:g} bytes, {n} grey Gaussians of {SEED_SCALE} m at {FIT_HW[0]} x {FIT_HW[1]}, three training poses, {args.iters} "
             f"iterations; the coefficients move the target frames by {spread:.2f} bytes a value on average"]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def score(tag, model):
        sc = metrics.psnr_ssim(frames_of(model.gaussians(), mats, cam), truth)
        for k, name in enumerate(names):
            say(f"  {tag}, {name}: PSNR {float(sc['psnr'][k]):.2f} dB, SSIM {float(sc['ssim'][k]):.4f}")

    for degree in (None, 0, DEGREE):
        model = gaussians.GaussianModel.from_cloud(render.PointCloud.from_arrays(xyz, grey, dev), SEED_SCALE, 0.9)
        if degree is None:
            score("before", model)
            continue
        losses = gaussians.fit(model, targets, mats[:3].contiguous(), cam, FIT_HW, iters=args.iters, sh_degree=degree)
        say(f" sh_degree {degree}: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
        score(f"sh_degree {degree}", model)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
