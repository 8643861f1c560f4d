#!/usr/bin/env python3
"""Cross-view depth consistency (csrc/consistency.hip) on ONE MI355X: 48 views — 16 frames x 3 poses (the camera and
render.virtual_poses' two) — at 576 x 1024, the default witness lists (reach 2: 14 witnesses at most) and r = 1.

`python tools/consistency_bench.py [--frames 16] [--runs 3] [--no-ddim] [--out profiles/consistency/bench.txt]`

The views are mudg_amd.synthetic.street_scene's background rendered at the three poses (render_conditions' LiDAR depth) and made dense
by depth.complete_depth; the labels are class 0, sky where nothing reached.  Median [min .. max] of `--runs` runs between device events
after a warm-up:
  flags        mudg_view_flags: per pixel 4 bytes of depth and 8 of label read, 1 written
  consistency  mudg_view_consistency: per pixel 4 bytes of depth and 1 of flags read as the source, 3 written; on top of that a usable
               pixel gathers N (2r + 1)^2 depths and as many flag bytes from its witnesses' maps — the same maps every source view reads,
               so they are counted once above and come from the caches when the kernel does well
  fuse_views   depth.fuse_views, all of it: the witness lists and tables on the host, their upload, the two kernels, mudg_depth_unproject
               (per pixel 15 read, 17 written) and the boolean selection of the kept points (16 bytes read and written per kept point)
Each with the bytes its rule needs per second, beside a device-to-device copy that moves the same number of bytes (half read, half
written) measured in the same process, and one DDIM step of the flagship workload alongside (tools/splat_bench.py's ddim_step_ms).
Nothing here is asserted: the file records."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from mudg_amd import depth, metrics, ops, render
from mudg_amd.synthetic import street_scene
from splat_bench import ddim_step_ms, event_ms, spread

HW = (576, 1024)


def fmt(s, unit="ms"):
    return f"{s['median']:.4f} {unit} [{s['min']:.4f} .. {s['max']:.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-ddim", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("consistency_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    T, (H, W) = args.frames, HW
    street = street_scene(n_background=2_000_000, frames=T, seed=0, n_objects=1, object_points=100)   # the background alone is rendered
    bg = render.PointCloud.from_arrays(street["bg_xyz"], street["bg_rgb"], dev)
    cams = np.stack([np.stack(render.virtual_poses(c, with_ori_pose=True)) for c in street["c2w"]])          # (T, 3, 4, 4)
    lidar = render.render_conditions(bg, None, street["intr"], street["c2w"], street["hw_native"], HW, poses=cams, return_images=True)["depth"]
    P = lidar.shape[0]
    V = P * T
    z = depth.complete_depth(lidar.reshape(V, H, W).contiguous())                                            # pose-major, as fuse_window_outputs stacks
    labels = torch.where(z > 0, 0, depth.SKY_LABEL).to(torch.int64)
    rgb = torch.randint(0, 256, (V, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(0))
    c2w = np.concatenate([cams[:, p] for p in range(P)])
    intr = np.broadcast_to(np.asarray(street["intr"], dtype=np.float64), (V, 3, 3))
    times, poses = np.tile(np.arange(T, dtype=np.int32), P), np.repeat(np.arange(P, dtype=np.int32), T)
    lists = depth.default_witnesses(times, poses, reach=2)
    N, r = lists.shape[1], 1
    source = depth.camera_table(intr, c2w, street["hw_native"], HW)
    tables = torch.from_numpy(np.stack([source, depth.witness_table(c2w, source)])).to(dev)
    px = V * H * W
    state = {}

    def flags():
        state["flags"] = ops.view_flags(z, labels)

    def consistency():
        state["out"] = ops.view_consistency(z, state["flags"], tables[0], tables[1], times, lists, r=r)

    def fuse():
        state["cloud"], state["result"] = depth.fuse_views(z, rgb, intr, c2w, street["hw_native"], labels, times=times, witnesses=lists, r=r)

    for fn in (flags, consistency, fuse):                                                                    # warm-up
        fn()
    torch.cuda.synchronize()
    kept = len(state["cloud"])
    scores = metrics.view_consistency(state["result"])["overall"]
    say(f"consistency_bench on {torch.cuda.get_device_name(0)}: {V} views ({T} frames x {P} poses) of {H} x {W}, {N} witnesses at most, r = {r}: "
        f"{N * (2 * r + 1) ** 2} depth and {N * (2 * r + 1) ** 2} flag gathers per usable source pixel at most; median [min .. max] of {args.runs} runs")
    say(f" usable {int(state['result']['stats'][:, 0].sum())} of {px} pixels; tested {scores['tested']:.4f}, kept {scores['kept']:.4f}, violated {scores['violated']:.4f} "
        f"of the usable ones, {scores['mean_agree']:.3f} agreeing witnesses per tested pixel; {kept} points in the fused cloud")
    stages = (("flags", flags, px * 13), ("consistency", consistency, px * 8), ("fuse_views (all of it)", fuse, px * (13 + 8 + 32) + kept * 32))
    for name, fn, nbytes in stages:
        ms = spread([event_ms(fn) for _ in range(args.runs)])
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        b.copy_(a)
        torch.cuda.synchronize()
        copy = spread([event_ms(lambda: b.copy_(a)) for _ in range(args.runs)])
        del a, b
        extra = ""
        if name == "consistency":
            usable = int(state["result"]["stats"][:, 0].sum())
            extra = f"; {usable * N * (2 * r + 1) ** 2 / (ms['median'] * 1e-3) / 1e9:.1f} G window pixels per second if every list were full"
        say(f"  {name:24s} {fmt(ms)}; {nbytes / (ms['median'] * 1e-3) / 1e12:.3f} TB/s of the {nbytes / 1e6:.1f} MB its rule needs; "
            f"a copy of the same bytes {fmt(copy)}, {nbytes / (copy['median'] * 1e-3) / 1e12:.3f} TB/s{extra}")
    if not args.no_ddim:
        step = ddim_step_ms(args.runs, dev)
        say(f" one DDIM step of the flagship workload in this process: {fmt(step)}")


if __name__ == "__main__":
    main()
