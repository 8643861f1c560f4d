#!/usr/bin/env python3
"""TEST INFRASTRUCTURE, not a test: what the cloud scores of DESIGN.md §22 say about the consistency filter of §21, and what a radius
outlier filter removes after it, on the synthetic street, by the CPU definitions (tests/neighbours_reference.py,
tests/consistency_reference.py; no GPU): measured, not asserted.  It lives beside the definitions because nothing in the product or its
tools may import them.  `python tests/neighbours_quality.py [--out profiles/neighbours/quality.txt] [--stride 4]`

Scene, views and degradations are tests/consistency_quality.py's: 15 views of 320 x 480, depths quantised, box-blurred (flying pixels at
every depth edge), one view biased by 1.10.  The consistency rule runs on the whole views.  Every view is then lifted with numpy (the
lifting rule of §14, rounded to fp32 as a packed point is), and — the definition walks its candidate pairs in numpy — only every
`--stride`-th row and column of every view becomes a point, in the scored clouds and in the truth alike; the truth is the cloud lifted
from the undegraded depth g at the same pixels.  A point is WRONG when its pixel's degraded depth is further than abs_tol + rel_tol g
from g, and RIGHT otherwise (consistency_quality.py's split).  Reported:
  cloud_scores (pred = the cloud, truth = the undegraded cloud, the default thresholds) of the unfiltered cloud, of the cloud after the
  consistency filter at its defaults, and after the filter with max_violate = 1;
  radius_outliers on the cloud each of the two filters leaves, for a few (radius, min_neighbours): the share of its WRONG points removed
  and the share of its RIGHT points lost.
The point spacing of a strided cloud is `--stride` times a whole view's, so a radius here stands for one `--stride` times smaller on the
unstrided cloud; no default for neighbour_radius or min_neighbours is proposed from this."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import consistency_quality as cq
import consistency_reference as cr
import neighbours_reference as nr
from mudg_amd import depth

THRESHOLDS = (0.05, 0.1, 0.2, 0.5)
PAIRS = ((0.2, 1), (0.2, 2), (0.3, 2), (0.3, 4), (0.5, 4), (0.5, 8), (1.0, 8), (1.0, 16))


def lift(z, source):
    """(V, H, W) depths -> (V, H, W, 3) float32 world points."""
    return np.stack([np.stack(cr.world_points(z[v], source[v]), axis=-1) for v in range(len(z))]).astype(np.float32)


def walk(ref, queries, r):
    return nr.walk_nearest(ref, queries, r)[:2]


def describe(s):
    f = lambda a: "[" + ", ".join(f"{v:.4f}" for v in a) + "]"
    return (f"accuracy {f(s['accuracy'])}, completeness {f(s['completeness'])}, fscore {f(s['fscore'])}; found {f(s['found'])}; mean accuracy "
            f"{s['mean_accuracy']:.4f} m, mean completeness {s['mean_completeness']:.4f} m, chamfer {s['chamfer']:.4f} m")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--stride", type=int, default=4)
    args = ap.parse_args()
    t0 = time.time()
    g, c2w, intr, order = cq.views()
    z = cq.degrade(g, order)
    times, poses = np.array([f for f, _ in order], dtype=np.int32), np.array([p for _, p in order], dtype=np.int32)
    source = depth.camera_table(intr, c2w, cq.HW, cq.HW)
    witness = depth.witness_table(c2w, source)
    lists = depth.default_witnesses(times, poses)
    rule = dict(cr.DEFAULTS)
    picked = np.zeros(z.shape, dtype=bool)
    picked[:, args.stride // 2::args.stride, args.stride // 2::args.stride] = True
    usable = (cr.flags(z) & 1) == 1
    wrong = usable & (np.abs(z.astype(np.float64) - g) > rule["abs_tol"] + rule["rel_tol"] * g)
    points = lift(z, source)
    g32 = g.astype(np.float32)
    truth = lift(g32, source)[picked & ((cr.flags(g32) & 1) == 1)]
    lines = [f"neighbours_quality: the CPU definitions on consistency_quality.py's scene ({len(order)} views of {cq.HW[0]} x {cq.HW[1]}, depths quantised, "
             f"box-blurred 3 x 3, one view times 1.10); every {args.stride}th row and column of every view is a point; the truth is the cloud of "
             f"the undegraded depth, {len(truth)} points; thresholds {list(THRESHOLDS)} m"]
    keeps = {"unfiltered": usable}
    for name, kw in (("the consistency filter at its defaults", {}), ("the consistency filter with max_violate = 1", {"max_violate": 1})):
        keeps[name] = cr.consistency(z, None, source, witness, times, lists, **dict(rule, **kw))["keep"] == 1
    for name, keep in keeps.items():
        sel = picked & keep
        s = nr.cloud_scores(points[sel], truth, THRESHOLDS, search=walk)
        lines.append(f" {name}: {int(sel.sum())} points, {int((sel & wrong).sum())} of them WRONG")
        lines.append(f"  {describe(s)}")
        print("\n".join(lines[-2:]), f"({time.time() - t0:.0f} s)", flush=True)
    for name in list(keeps)[1:]:
        sel = picked & keeps[name]
        cloud, bad = points[sel], wrong[sel]
        lines.append(f" radius_outliers on the cloud that {name} leaves ({len(cloud)} points, {int(bad.sum())} WRONG, {int((~bad).sum())} RIGHT):")
        for radius, need in PAIRS:
            kept = nr.walk_counts(cloud, cloud, radius, need + 1) >= need + 1
            lines.append(f"  radius {radius} m, min_neighbours {need}: WRONG points removed {cq.share(int((bad & ~kept).sum()), int(bad.sum()))}; "
                         f"RIGHT points lost {cq.share(int((~bad & ~kept).sum()), int((~bad).sum()))}")
            print(lines[-1], f"({time.time() - t0:.0f} s)", flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
