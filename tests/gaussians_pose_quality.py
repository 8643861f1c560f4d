#!/usr/bin/env python3
"""TEST INFRASTRUCTURE, not a test: what camera refinement does to a fit whose training poses are off, on the GPU:
measured, not asserted.  `python tests/gaussians_pose_quality.py [--out profiles/gaussians/pose_quality.txt] [--iters 300]`

The street is tools/gaussians_fit_bench.py's: 30000 points on a ground plane and two walls at 72 x 128, textured, drawn by the inference
renderer at three training poses (the street's camera and 2 m to either side) and one held-out pose (1 m to one side).  The fit is
handed the training matrices with a seeded twist of `--angle` degrees and `--shift` metres applied on the left of each, starts from grey
seeds of 0.2 m at the points' positions, and runs `--iters` iterations once without and once with `poses=CameraPoses(3, fixed=(0,))`.
View 0 is the gauge: its matrix stays as handed over, so the Gaussians settle in its (wrong) frame.  Everything reported is in that
frame: the pose error of views 1 and 2 is that of their pose relative to view 0's (centre distance, rotation angle), and the held-out
frame is drawn at the true held-out pose carried into view 0's frame.  Reported: PSNR / SSIM (mudg_amd.metrics.psnr_ssim) of the
inference render of the exported Gaussians against the target per pose, and the residual pose error.

The target is synthetic: a cloud drawn by the renderer that is then fitted, seeds at the true positions.  Nothing about real scenes
follows from these figures, and no learning rate was tuned."""
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


def frames_of(g, mats, cam):
    out = gaussians.render(g, mats, cam, FIT_HW)
    return torch.floor(out["rgb"] * 255.0 + 0.5).clamp_(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def relative_error(w2c, w2c0, true, true0):
    """The pose of a camera relative to view 0's, estimated against true: (centre distance in metres, rotation angle in radians)."""
    e, t = w2c @ np.linalg.inv(w2c0), true @ np.linalg.inv(true0)
    centre = lambda m: -m[:3, :3].T @ m[:3, 3]
    d = e[:3, :3] @ t[:3, :3].T
    sin = 0.5 * np.linalg.norm([d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]])
    return float(np.linalg.norm(centre(e) - centre(t))), float(np.arctan2(sin, (np.trace(d) - 1.0) / 2.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussians", "pose_quality.txt"))
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--angle", type=float, default=1.0, help="degrees")
    ap.add_argument("--shift", type=float, default=0.10, help="metres")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gaussians_pose_quality: no GPU (the fit has no CPU path)")
    dev = torch.device("cuda:0")
    s = street_scene(n_background=30000, frames=1, seed=5, n_objects=1, object_points=10)
    xyz = s["bg_xyz"]
    n = len(xyz)
    cam = render.scaled_intrinsics(s["intr"], s["hw_native"], FIT_HW).astype(np.float32)
    left, right = render.virtual_poses(s["c2w"][0], 2.0, with_ori_pose=False)[:2]
    held = render.virtual_poses(s["c2w"][0], 1.0, with_ori_pose=False)[0]
    true = np.linalg.inv(np.stack([s["c2w"][0], left, right, held]))                           # world to camera, float64
    names = ["original", "2 m to one side", "2 m to the other", "1 m to one side (held out)"]
    rng = np.random.default_rng(28)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    twist = np.concatenate([unit(rng.normal(size=(3, 3))) * np.deg2rad(args.angle), unit(rng.normal(size=(3, 3))) * args.shift], axis=1)
    off = gaussians.CameraPoses(3, device="cpu")
    with torch.no_grad():
        off.twist.copy_(torch.from_numpy(twist.astype(np.float32)))
    handed = off.world_to_camera(true[:3])                                                     # what the fit is given
    held_in_gauge = true[3] @ np.linalg.inv(true[0]) @ handed[0]                               # the held-out pose in view 0's frame
    table = lambda w2c: torch.from_numpy(gaussians.scene_matrices(None, w2c, 0)).to(dev)
    textured = gaussians.Gaussians.from_cloud(render.PointCloud.from_arrays(xyz, texture(xyz), dev), SEED_SCALE, 0.9)
    truth = frames_of(textured, table(true), cam)
    targets = truth[:3].permute(0, 3, 1, 2).to(torch.float32).div_(255.0).contiguous()
    grey = np.full((n, 3), 128, np.uint8)
    lines = [f"gaussians_pose_quality on {torch.cuda.get_device_name(0)}: the textured street, {n} grey Gaussians of {SEED_SCALE} m at "
             f"{FIT_HW[0]} x {FIT_HW[1]}, three training poses each off by a seeded twist of {args.angle:g} degrees and {100 * args.shift:g} cm, "
             f"{args.iters} iterations; view 0 is the gauge.  The target is synthetic: nothing about real scenes follows"]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def report(tag, model, w2c):
        sc = metrics.psnr_ssim(frames_of(model.gaussians(), table(np.concatenate([w2c, held_in_gauge[None]])), cam), truth)
        for k, name in enumerate(names):
            say(f"  {tag}, {name}: PSNR {float(sc['psnr'][k]):.2f} dB, SSIM {float(sc['ssim'][k]):.4f}")
        for v in (1, 2):
            c, a = relative_error(w2c[v], w2c[0], true[v], true[0])
            say(f"  {tag}, view {v} relative to view 0: camera centre off by {100 * c:.2f} cm, rotation by {np.rad2deg(a):.3f} degrees")

    for with_poses in (None, False, True):
        model = gaussians.GaussianModel.from_cloud(render.PointCloud.from_arrays(xyz, grey, dev), SEED_SCALE, 0.9)
        if with_poses is None:
            report("before", model, handed)
            continue
        poses = gaussians.CameraPoses(3, fixed=(0,), device=dev) if with_poses else None
        losses = gaussians.fit(model, targets, table(handed), cam, FIT_HW, iters=args.iters, poses=poses)
        tag = "with poses" if with_poses else "without poses"
        say(f" {tag}: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
        report(tag, model, poses.world_to_camera(handed) if with_poses else handed)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
