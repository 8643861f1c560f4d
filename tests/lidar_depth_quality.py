#!/usr/bin/env python3
"""TEST INFRASTRUCTURE, not a test: what the rules of DESIGN.md §20 give on the synthetic street, by the CPU definition
(tests/lidar_depth_reference.py; no GPU): measured, not asserted.  It lives beside the definition because nothing in the product or its
tools may import that.  `python tests/lidar_depth_quality.py [--out profiles/lidar_depth/quality.txt]`

Scene: street_sweeps(frames=6, beams=64, azimuths=1325, n_objects=0, n_static=4, n_other=0, seed=0), camera_FRONT at its own 320 x 480,
frames 2 and 5, every parameter at its default.  g is the analytic depth of the world through the pixel centres.
  sparse  AbsRel = mean |d - g| / g of the LiDAR depth map over its covered pixels, without and with the occlusion filter
  dense   AbsRel of the completed map over all pixels with g < 75 m (an empty pixel counts with d = 0), beside the same score of a
          nearest-covered-pixel fill (scipy.ndimage.distance_transform_edt's indices) of the same sparse map"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import lidar_depth_cases as cases
import lidar_depth_reference as ld


def absrel(d, g, mask):
    return float(np.mean(np.abs(d[mask].astype(np.float64) - g[mask]) / g[mask]))


def nearest_fill(d):
    from scipy.ndimage import distance_transform_edt
    idx = distance_transform_edt(d == 0, return_distances=False, return_indices=True)
    return d[idx[0], idx[1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"lidar_depth_quality: the CPU definition on street_sweeps({', '.join(f'{k}={v}' for k, v in cases.LEAK_SCENE.items())}), "
             f"{cases.LEAK_CAMERA} at {cases.LEAK_HW[0]} x {cases.LEAK_HW[1]}, defaults"]
    for frame in (2, 5):
        g, off, on = cases.leak_maps(frame)
        near = np.isfinite(g) & (g < 75.0)
        lines.append(f" frame {frame}: covered {int((off > 0).sum())} pixels without the filter, {int((on > 0).sum())} with it; "
                     f"leaked {int(ld.leaked(off, g).sum())} -> {int(ld.leaked(on, g).sum())}")
        lines.append(f"  sparse AbsRel at covered pixels: {absrel(off, g, (off > 0) & np.isfinite(g)):.4f} without the filter, "
                     f"{absrel(on, g, (on > 0) & np.isfinite(g)):.4f} with it")
        for name, d in (("with the filter", on), ("without the filter", off)):
            dense = ld.complete_depth(d)[0]
            lines.append(f"  dense AbsRel over g < 75 m, {name}: completion {absrel(dense, g, near):.4f} ({int((dense[near] == 0).sum())} pixels left empty), "
                         f"nearest-pixel fill {absrel(nearest_fill(d), g, near):.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
