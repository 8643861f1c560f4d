#!/usr/bin/env python3
"""TEST INFRASTRUCTURE, not a test: what the Gaussian splat rule of DESIGN.md §23 draws on the synthetic street, by the CPU definition
(tests/gaussians_reference.py; no GPU): measured, not asserted.  It lives beside the definitions because nothing in the product or its
tools may import them.  `python tests/gaussians_quality.py [--out profiles/gaussians/quality.txt] [--points 30000] [--hw 72,128]`

The cloud is mudg_amd.synthetic.street_scene's background (a ground plane and two walls, `--points` points), recoloured by a smooth
procedural texture of the surfaces so that the street has an image of its own: the same texture ray-cast per pixel against the two planes
(black where a ray leaves the street).  The cloud is drawn at the street's first camera and at the reference's two virtual poses, 2 m to
either side, as isotropic Gaussians of a few scales (opacity 1) and, for comparison, by the hard point splat of §12
(tests/splat_reference.py, point size 2.5).  Reported per pose:
  the share of pixels with alpha > 0.5 (for the point splat: the share of pixels that a point landed on);
  PSNR and SSIM (tests/metrics_reference.py) of the render, on black, against the street's own image.
The cloud is far sparser than a real one (a few points per square metre), so the scales that close its holes are far larger than a
cloud thinned at 0.1 m needs; no default scale is proposed from this."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import gaussians_reference as gr
import metrics_reference as mr
import splat_reference as sr
from mudg_amd import render
from mudg_amd.synthetic import street_scene

SCALES = (0.1, 0.2, 0.4, 0.8)
POSES = ("original", "2 m left", "2 m right")


def texture(p):
    """(n, 3) positions on the street's surfaces -> (n, 3) uint8: bands along the street, across it and up the walls."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    c = np.stack([128 + 100 * np.sin(0.8 * z), 128 + 100 * np.sin(0.9 * x + 0.7 * y), 128 + 100 * np.cos(0.35 * z + 0.5 * x)], axis=1)
    return np.clip(np.rint(c), 1, 255).astype(np.uint8)


def own_image(c2w, cam, hw):
    """The texture seen from a camera: per pixel the nearest of the ground (y = 1.6) and the walls (x = +-12) inside the street's extent."""
    H, W = hw
    fx, fy, cx, cy = (float(v) for v in cam)
    j, i = np.mgrid[0:H, 0:W]
    d = np.stack([(i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, np.ones((H, W))], axis=-1).reshape(-1, 3) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    best = np.full(len(d), np.inf)
    with np.errstate(all="ignore"):
        for axis, value in ((1, 1.6), (0, -12.0), (0, 12.0)):
            t = (value - o[axis]) / d[:, axis]
            p = o + t[:, None] * d
            ok = (t > 0) & (p[:, 2] > -5) & (p[:, 2] < 150) & (p[:, 1] <= 1.6 + 1e-9) & (p[:, 1] > -9) & (np.abs(p[:, 0]) <= 25)
            if axis == 1:
                ok &= np.abs(p[:, 0]) <= 12
            best = np.where(ok & (t < best), t, best)
    hit = np.isfinite(best)
    img = np.zeros((len(d), 3), np.uint8)
    img[hit] = texture(o + best[hit, None] * d[hit])
    return img.reshape(H, W, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussians", "quality.txt"))
    ap.add_argument("--points", type=int, default=30000)
    ap.add_argument("--hw", default="72,128")
    args = ap.parse_args()
    hw = tuple(int(v) for v in args.hw.split(","))
    t0 = time.time()
    s = street_scene(n_background=args.points, frames=1, seed=5, n_objects=1, object_points=10)
    xyz = s["bg_xyz"]
    rgb = texture(xyz.astype(np.float64))
    cam = render.scaled_intrinsics(s["intr"], s["hw_native"], hw).astype(np.float32)
    poses = np.stack(render.virtual_poses(s["c2w"][0], 2.0, with_ori_pose=True))
    mats = np.linalg.inv(poses)[:, None, :3, :].reshape(3, 1, 12).astype(np.float32)
    truth = np.stack([own_image(p, cam, hw) for p in poses])
    lines = [f"gaussians_quality: the CPU definition on the synthetic street ({len(xyz)} points on a ground plane and two walls, textured), "
             f"{hw[0]} x {hw[1]}, poses {list(POSES)}; the street's own image covers {[round(float((t.sum(axis=2) > 0).mean()), 4) for t in truth]} of the pixels"]

    def report(name, frames, cover):
        score = mr.psnr_ssim(frames, truth)
        lines.append(f" {name}: coverage {[round(float(c), 4) for c in cover]}; PSNR {[round(float(v), 2) for v in score['psnr']]} dB; "
                     f"SSIM {[round(float(v), 4) for v in score['ssim']]}")
        print(lines[-1], f"({time.time() - t0:.0f} s)", flush=True)

    hard = [sr.splat(xyz, rgb, mats[p, 0].reshape(3, 4), cam, np.float32(render.BACKGROUND_POINT_SIZE), hw[0], hw[1]) for p in range(3)]
    report("the point splat of §12 (point size 2.5, hard z-buffer)", np.stack([h[0] for h in hard]), [(h[1] > 0).mean() for h in hard])
    pts = gr.pack(xyz, rgb)
    for scale in SCALES:
        out = gr.render(pts, gr.isotropic(scale, len(xyz)), np.ones(len(xyz), np.float32), None, mats, cam, hw)
        report(f"Gaussians of {scale} m ({out['entries']} entries, longest tile {out['longest_tile']})", gr.rgb_u8(out["rgb"]),
               [(a > 0.5).mean() for a in out["alpha"]])
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
