#!/usr/bin/env python3
"""TEST INFRASTRUCTURE, not a test: what the cross-view consistency rule of DESIGN.md §21 removes and keeps on the synthetic street, by
the CPU definition (tests/consistency_reference.py; no GPU): measured, not asserted.  It lives beside the definition because nothing in
the product or its tools may import that.  `python tests/consistency_quality.py [--out profiles/consistency/quality.txt]`

Scene: street_sweeps(frames=5, n_objects=0, n_static=4, n_other=0, seed=0) — nothing moves, so no labels are given — camera_FRONT at its
own 320 x 480, five frames at three poses (the camera and render.virtual_poses' 2 m to the left and to the right): 15 views, the default
witness lists (the other poses of the frame, then every view within two frames).  g is the analytic depth through the pixel centres,
100 m where a ray hits nothing.  The views are degraded the way a generated depth stream is:
  1  quantised to the stream's 765 levels over 100 m           2  smeared by a 3 x 3 box blur: flying pixels at every depth edge
  3  one whole view (frame 2, the left pose) multiplied by 1.10
A pixel is WRONG when its degraded depth is further than abs_tol + rel_tol g from g, and RIGHT otherwise; only usable pixels count.
Three runs: the defaults, min_agree = 1, and max_violate = 1 (one accusing witness is tolerated: what the biased view costs the others)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import consistency_reference as cr
import lidar_depth_reference as ld
from mudg_amd import depth, render
from mudg_amd.synthetic import street_sweeps

SCENE = dict(frames=5, n_objects=0, n_static=4, n_other=0, seed=0)
CAMERA, HW = "camera_FRONT", (320, 480)
BIASED = (2, 1)                                    # (frame, pose)


def views():
    scenario = street_sweeps(**SCENE)[0]
    data = scenario["observers"][CAMERA]["data"]
    order = [(f, p) for p in range(3) for f in range(SCENE["frames"])]
    c2w = np.stack([render.virtual_poses(data["c2w"][f], with_ori_pose=True)[p] for f, p in order])
    truth = []
    for (f, p), m in zip(order, c2w):
        moved = {"objects": scenario["objects"],
                 "observers": dict(scenario["observers"], **{CAMERA: {"n_frames": SCENE["frames"], "data": dict(data, c2w=np.stack([m] * SCENE["frames"]))}})}
        truth.append(np.minimum(ld.analytic_depth(moved, CAMERA, f), 100.0))
    return np.stack(truth), c2w, np.stack([data["intr"][f] for f, _ in order]), order


def degrade(g, order):
    z = np.rint(g / 100.0 * 765.0) / 765.0 * 100.0
    padded = np.pad(z, ((0, 0), (1, 1), (1, 1)), mode="edge")
    z = sum(padded[:, 1 + dj:1 + dj + z.shape[1], 1 + di:1 + di + z.shape[2]] for dj in (-1, 0, 1) for di in (-1, 0, 1)) / 9.0
    z[order.index(BIASED)] *= 1.10
    return np.minimum(z, 100.0).astype(np.float32)


def share(a, b):
    return f"{a / b:.4f} ({a} of {b})" if b else "- (0 of 0)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g, c2w, intr, order = views()
    z = degrade(g, order)
    times, poses = np.array([f for f, _ in order], dtype=np.int32), np.array([p for _, p in order], dtype=np.int32)
    source = depth.camera_table(intr, c2w, HW, HW)
    witness = depth.witness_table(c2w, source)
    lists = depth.default_witnesses(times, poses)
    biased = np.zeros(len(order), dtype=bool)
    biased[order.index(BIASED)] = True
    lines = [f"consistency_quality: the CPU definition on street_sweeps({', '.join(f'{k}={v}' for k, v in SCENE.items())}), {CAMERA} at {HW[0]} x {HW[1]}, "
             f"{SCENE['frames']} frames x 3 poses = {len(order)} views, {lists.shape[1]} witnesses at most; depths quantised to 765 levels over 100 m, "
             f"box-blurred 3 x 3, view (frame {BIASED[0]}, pose {BIASED[1]}) times 1.10"]
    for name, rule in (("defaults", dict(cr.DEFAULTS)), ("min_agree = 1", dict(cr.DEFAULTS, min_agree=1)), ("max_violate = 1", dict(cr.DEFAULTS, max_violate=1))):
        got = cr.consistency(z, None, source, witness, times, lists, **rule)
        usable = (got["flags"] & 1) == 1
        tol = rule["abs_tol"] + rule["rel_tol"] * g
        wrong = usable & (np.abs(z.astype(np.float64) - g) > tol)
        right = usable & ~wrong
        kept = got["keep"] == 1
        lines.append(f" {name}: r = {rule['r']}, min_agree = {rule['min_agree']}, max_violate = {rule['max_violate']}, rel_tol = {rule['rel_tol']}, abs_tol = {rule['abs_tol']} m")
        for what, sel in (("the 14 unbiased views", ~biased), ("the biased view", biased)):
            w, r = wrong[sel], right[sel]
            k, b, a = kept[sel], got["violate"][sel], got["agree"][sel]
            lines.append(f"  {what}: usable {int(usable[sel].sum())}, wrong {int(w.sum())}, right {int(r.sum())}")
            lines.append(f"   wrong pixels removed {share(int((w & ~k).sum()), int(w.sum()))}; of those kept, {int((w & k & (b == 0) & (a >= rule['min_agree'])).sum())} "
                         f"had enough agreeing witnesses and no violation")
            lines.append(f"   right pixels kept    {share(int((r & k).sum()), int(r.sum()))}; of those removed, {int((r & ~k & (b > 0)).sum())} by a violation, "
                         f"{int((r & ~k & (b == 0)).sum())} for too few agreeing witnesses ({int((r & ~k & (a == 0) & (b == 0)).sum())} had no verdict at all)")
        per_view, overall = cr.scores(got["stats"])
        at = order.index(BIASED)
        lines.append(f"  scores (metrics.view_consistency's): overall tested {overall['tested']:.4f}, kept {overall['kept']:.4f}, violated {overall['violated']:.4f}, "
                     f"mean agree {overall['mean_agree']:.3f}; the biased view kept {per_view[at]['kept']:.4f}, violated {per_view[at]['violated']:.4f}, "
                     f"mean agree {per_view[at]['mean_agree']:.3f}; the unbiased views kept {min(v['kept'] for n, v in enumerate(per_view) if n != at):.4f} .. "
                     f"{max(v['kept'] for n, v in enumerate(per_view) if n != at):.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
