#!/usr/bin/env python3
"""The Gaussian splat renderer (mudg_amd/gaussians.py, csrc/gaussians.hip) on ONE MI355X.

`python tools/gaussians_bench.py [--points 2,8] [--scale 0.1] [--runs 3] [--no-ddim] [--out profiles/gaussians/bench.txt]`

The cloud is mudg_amd.synthetic.street_scene's background (a ground plane and two walls), every point an isotropic Gaussian of `--scale`
metres and opacity 1, drawn into ONE 576 x 1024 view at the street's first camera.  Per cloud size (millions of Gaussians), median
[min .. max] of `--runs` runs between device events after a warm-up:
  project       mudg_gauss_project
  keys + sort   the exclusive sum of the counts (and the .item() that reads E), mudg_gauss_keys, torch.sort (stable) and the gather of
                the values
  ranges        mudg_gauss_ranges
  blend         mudg_gauss_blend
  render        gaussians.render, all of it
with E (the (tile, Gaussian) entries), entries per tile (mean and longest) and the entries the blend's workgroups actually staged before
every pixel of their tile was opaque.  Beside them, in the same process: render_conditions (the hard point splat of §12) of the same
cloud at the same view, a device-to-device copy of the bytes the four kernels move at least (44 per Gaussian read and 40 written by the
projection, 12 per entry written and read again around the sort, 20 per pixel written), and one DDIM step of the flagship workload
(tools/splat_bench.py's ddim_step_ms).  A cloud whose E exceeds max_entries is recorded as refused.  Nothing here is asserted: the file
records."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from mudg_amd import gaussians, hip, ops, render
from mudg_amd.synthetic import street_scene
from splat_bench import ddim_step_ms, event_ms, spread

HW = (576, 1024)


def fmt(s, unit="ms"):
    return f"{s['median']:.3f} {unit} [{s['min']:.3f} .. {s['max']:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="2,8", help="Gaussians in millions")
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-ddim", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussians", "bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gaussians_bench: no GPU (a CPU run measures nothing)")
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

    say(f"gaussians_bench on {torch.cuda.get_device_name(0)}: one {HW[0]} x {HW[1]} view of the synthetic street, isotropic Gaussians of "
        f"{args.scale} m, opacity 1; median [min .. max] of {args.runs} runs")
    tx, ty = ops.gauss_tiles(*HW)
    tiles = tx * ty
    for millions in [float(v) for v in args.points.split(",") if v]:
        n = int(millions * 1e6)
        scene = street_scene(n_background=n, frames=1, seed=11, n_objects=1, object_points=100)
        cloud = render.PointCloud.from_arrays(scene["bg_xyz"], scene["bg_rgb"], dev)
        g = gaussians.Gaussians.from_cloud(cloud, args.scale)
        cam = render.scaled_intrinsics(scene["intr"], scene["hw_native"], HW).astype(np.float32)
        mats = torch.from_numpy(gaussians.scene_matrices(None, np.linalg.inv(scene["c2w"][:1]), 0)).to(dev)
        project = lambda: ops.gauss_project(cloud.points, g.cov, g.opacity, mats, cam, HW, znear=gaussians.ZNEAR, zfar=gaussians.ZFAR)
        uv, conic, depth, rect, count = project()
        entries = int(count.sum(dtype=torch.int64).item())
        say(f" {millions:g} M Gaussians: {int((count > 0).sum())} drawn, E = {entries} entries, {entries / tiles:.1f} per tile of {tiles}")
        if entries == 0 or entries > gaussians.MAX_ENTRIES:
            say(f"  refused: E is outside 1 .. max_entries = {gaussians.MAX_ENTRIES}")
            continue

        def bin_entries():
            ends = torch.cumsum(count.reshape(-1), 0, dtype=torch.int64)
            offsets = (ends - count.reshape(-1)).reshape(count.shape)
            keys, values = ops.gauss_keys(depth, rect, count, offsets, int(ends[-1].item()), HW)
            keys, order = torch.sort(keys, stable=True)
            return keys, values[order]

        keys, values = bin_entries()
        ranges = ops.gauss_ranges(keys, tiles)
        walked = torch.zeros(tiles, dtype=torch.int32, device=dev)
        ops.gauss_blend(cloud.points, uv, conic, depth, values, ranges, HW, walked=walked)
        length = (ranges[:, 1] - ranges[:, 0]).double()
        say(f"  longest tile {int(length.max())} entries, median {int(length.median())}; the blend staged {int(walked.sum())} entries "
            f"({float(walked.sum()) / entries:.3f} of E) before every pixel of its tile was opaque")
        t_project, t_bin = timed(project), timed(bin_entries)
        t_ranges = timed(lambda: ops.gauss_ranges(keys, tiles))
        t_blend = timed(lambda: ops.gauss_blend(cloud.points, uv, conic, depth, values, ranges, HW))
        t_render = timed(lambda: gaussians.render(g, mats, cam, HW))
        try:
            out = gaussians.render(g, mats, cam, HW)
            cover = float((out["alpha"] > 0.5).double().mean())
        except hip.MudgError as e:
            say(f"  render refused: {e}")
            continue
        say(f"  project {fmt(t_project)}, {n / (t_project['median'] * 1e-3) / 1e9:.2f} G Gaussians/s; keys + sort {fmt(t_bin)}, "
            f"{entries / (t_bin['median'] * 1e-3) / 1e9:.2f} G entries/s; ranges {fmt(t_ranges)}; blend {fmt(t_blend)}, "
            f"{float(walked.sum()) / (t_blend['median'] * 1e-3) / 1e9:.2f} G staged entries/s; render, all of it {fmt(t_render)}; "
            f"alpha > 0.5 on {cover:.4f} of the pixels")
        poses = scene["c2w"][:1, None]
        t_splat = timed(lambda: render.render_conditions(cloud, None, scene["intr"], scene["c2w"][:1], scene["hw_native"], HW, poses=poses))
        nbytes = n * (44 + 40) + entries * 24 + HW[0] * HW[1] * 20
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        t_copy = timed(lambda: b.copy_(a))
        del a, b
        say(f"  render_conditions (the point splat of §12) of the same cloud and view {fmt(t_splat)}; a copy of the {nbytes / 1e6:.0f} MB the four "
            f"kernels move at least {fmt(t_copy)}")
        del g, cloud, uv, conic, depth, rect, count, keys, values, ranges
        torch.cuda.empty_cache()
    if not args.no_ddim:
        say(f" one DDIM step of the flagship workload in this process: {fmt(ddim_step_ms(args.runs, dev))}")


if __name__ == "__main__":
    main()
