#!/usr/bin/env python3
"""Neighbour search between clouds (csrc/neighbours.hip) on ONE MI355X.

`python tools/neighbours_bench.py [--queries 2,8,27] [--fused 8] [--runs 3] [--no-ddim] [--out profiles/neighbours/bench.txt]`

The LiDAR cloud is mudg_amd.synthetic.street_scene's background (2 M points on a ground plane and two walls), thinned at 0.1 m.  A fused
cloud is made on the device from the same surfaces — `--fused` million points (and 2 / 8 / 27 million as queries), 3 cm of noise across
the surface, 5 % of them flying points anywhere in the street's volume — the way lifted views look: dense, noisy, with isolated
points.  Median [min .. max] of `--runs` runs between device events after a warm-up:
  grid build       cloud.NeighbourGrid.build: the bounds to the host, mudg_cloud_voxel_keys, torch.sort (stable), the gather
  nearest          cloud.nearest at r = 0.5 m (metrics.cloud_scores' default radius): the queries' keys and their sort, then
                   mudg_cloud_nearest — and the kernel alone in that order, and alone in the caller's order (what the sort buys)
  counts           cloud.neighbour_counts at r = 0.2 m with cap = 5, the same three ways
  radius_outliers  cloud.radius_outliers(fused, 0.2, 4), all of it     cloud_scores   metrics.cloud_scores(fused, lidar), all of it
with queries per second, the candidates a query examines in its 27 cells (mean and maximum; the capped count stops early, so this is
its upper bound), a device-to-device copy of the bytes the rule needs at least (16 per query read, 16 or 4 written; 32 per reference
point) measured in the same process, and one DDIM step of the flagship workload alongside (tools/splat_bench.py's ddim_step_ms).
Nothing here is asserted: the file records."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from mudg_amd import cloud, metrics, ops, render
from mudg_amd.synthetic import street_scene
from splat_bench import ddim_step_ms, event_ms, spread

R_NEAREST, R_COUNT, CAP = 0.5, 0.2, 5


def fmt(s, unit="ms"):
    return f"{s['median']:.3f} {unit} [{s['min']:.3f} .. {s['max']:.3f}]"


def fused_cloud(n, dev, seed, noise=0.03, flying=0.05):
    """n points on street_scene's ground and walls with `noise` metres across the surface, a share `flying` of them anywhere."""
    g = torch.Generator(dev).manual_seed(seed)
    u = lambda lo, hi, m: torch.rand(m, device=dev, generator=g) * (hi - lo) + lo
    bump = lambda m: torch.randn(m, device=dev, generator=g) * noise
    half = n // 2
    ground = torch.stack([u(-25, 25, half), 1.6 + bump(half), u(-5, 150, half)], dim=1)
    side = torch.where(torch.rand(n - half, device=dev, generator=g) < 0.5, -12.0, 12.0)
    wall = torch.stack([side + bump(n - half), u(-9, 1.6, n - half), u(-5, 150, n - half)], dim=1)
    xyz = torch.cat([ground, wall])[torch.randperm(n, device=dev, generator=g)]                # (frame, row, column) order is no spatial order
    m = int(n * flying)
    xyz[:m] = torch.stack([u(-12, 12, m), u(-9, 1.6, m), u(-5, 150, m)], dim=1)
    rgb = torch.randint(0, 256, (n, 3), dtype=torch.uint8, device=dev, generator=g)
    return render.PointCloud.from_arrays(xyz, rgb, dev)


def candidates(grid, points):
    """Reference points in each query's 27 cells (what mudg_cloud_nearest examines), by torch.searchsorted: (mean, max)."""
    i = torch.floor(points[:, :3].view(torch.float32).double() / grid.cell).long()
    total = torch.zeros(len(points), dtype=torch.int64, device=points.device)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            row = ((i[:, 0] + a + cloud.KEY_LIMIT) << 42) | ((i[:, 1] + b + cloud.KEY_LIMIT) << 21)
            first = torch.searchsorted(grid.keys, row | (i[:, 2] - 1 + cloud.KEY_LIMIT))
            last = torch.searchsorted(grid.keys, row | (i[:, 2] + 1 + cloud.KEY_LIMIT), right=True)
            total += last - first
    return float(total.double().mean()), int(total.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", default="2,8,27", help="query counts in millions")
    ap.add_argument("--fused", type=float, default=8.0, help="the fused cloud's points in millions")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-ddim", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("neighbours_bench: no GPU (a CPU run measures nothing)")
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
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        return timed(lambda: b.copy_(a))

    def search(name, reference, queries):
        """One reference, one query set: the grid at both radii, nearest and counts each three ways."""
        q, nq, n = queries.points, len(queries), len(reference)
        say(f" {name}: {n} reference points, {nq} queries")
        for what, r, out_bytes in (("nearest", R_NEAREST, 16), ("counts", R_COUNT, 4)):
            build = timed(lambda: cloud.NeighbourGrid.build(reference, r))
            grid = cloud.NeighbourGrid.build(reference, r)
            mean, most = candidates(grid, q)
            visit = cloud._visit(grid, q)
            if what == "nearest":
                whole = lambda: cloud.nearest(grid, queries)
                kernel = lambda v: ops.cloud_nearest(grid.points, grid.keys, grid.order, q, grid.cell, grid.r2, visit=v)
                found = float(torch.isfinite(whole()[0]).double().mean())
            else:
                whole = lambda: cloud.neighbour_counts(grid, queries, CAP)
                kernel = lambda v: ops.cloud_count(grid.points, grid.keys, grid.order, q, grid.cell, grid.r2, CAP, visit=v)
                found = float((whole() >= CAP).double().mean())
            order = timed(lambda: cloud._visit(grid, q))
            all_ms, sorted_ms, plain_ms = timed(whole), timed(lambda: kernel(visit)), timed(lambda: kernel(None))
            nbytes = nq * (16 + out_bytes) + n * 32
            copy = copy_of(nbytes)
            say(f"  r = {r} m: grid build {fmt(build)}; {mean:.1f} candidates per query in its 27 cells (at most {most}); "
                f"{found:.4f} of the queries {'find a neighbour' if what == 'nearest' else f'reach the cap of {CAP}'}")
            say(f"   {what:8s} all of it {fmt(all_ms)}, {nq / (all_ms['median'] * 1e-3) / 1e6:.1f} M queries/s; the queries' keys and sort {fmt(order)}; "
                f"the kernel in cell order {fmt(sorted_ms)}, {nq / (sorted_ms['median'] * 1e-3) / 1e6:.1f} M queries/s, "
                f"{nq * mean / (sorted_ms['median'] * 1e-3) / 1e9:.2f} G candidates/s; in the caller's order {fmt(plain_ms)}; "
                f"a copy of the {nbytes / 1e6:.0f} MB the rule needs at least {fmt(copy)}")

    street = street_scene(n_background=2_000_000, frames=1, seed=0, n_objects=1, object_points=100)
    lidar = cloud.voxel_downsample(render.PointCloud.from_arrays(street["bg_xyz"], street["bg_rgb"], dev), 0.1)
    fused = fused_cloud(int(args.fused * 1e6), dev, seed=1)
    thinned = cloud.voxel_downsample(fused, 0.1)
    say(f"neighbours_bench on {torch.cuda.get_device_name(0)}: a LiDAR cloud of {len(lidar)} points (2000000 thinned at 0.1 m), a fused cloud of "
        f"{len(fused)} points ({len(thinned)} thinned at 0.1 m); nearest at r = {R_NEAREST} m, counts at r = {R_COUNT} m with cap = {CAP}; "
        f"median [min .. max] of {args.runs} runs")
    say("accuracy pass: queries against the LiDAR cloud")
    for millions in [float(v) for v in args.queries.split(",") if v]:
        queries = fused if millions == args.fused else fused_cloud(int(millions * 1e6), dev, seed=2 + int(millions))
        search(f"{millions:g} M queries", lidar, queries)
        del queries
    say("completeness pass: the LiDAR cloud's points as queries against the fused cloud")
    search("unthinned", fused, lidar)
    search("thinned at 0.1 m", thinned, lidar)
    say("filters and scores")
    for name, pc in (("the fused cloud", fused), ("the fused cloud thinned at 0.1 m", thinned)):
        ms = timed(lambda: cloud.radius_outliers(pc, R_COUNT, CAP - 1))
        kept = float(cloud.radius_outliers(pc, R_COUNT, CAP - 1).double().mean())
        say(f"  radius_outliers({name}, {R_COUNT}, {CAP - 1}) {fmt(ms)}, {len(pc) / (ms['median'] * 1e-3) / 1e6:.1f} M points/s; keeps {kept:.4f}")
        ms = timed(lambda: metrics.cloud_scores(pc, lidar))
        s = metrics.cloud_scores(pc, lidar)
        say(f"  cloud_scores({name}, lidar) {fmt(ms)}; accuracy {[round(v, 4) for v in s['accuracy'].tolist()]}, completeness "
            f"{[round(v, 4) for v in s['completeness'].tolist()]}, chamfer {float(s['chamfer']):.4f} m")
    if not args.no_ddim:
        step = ddim_step_ms(args.runs, dev)
        say(f" one DDIM step of the flagship workload in this process: {fmt(step)}")


if __name__ == "__main__":
    main()
