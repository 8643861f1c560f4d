#!/usr/bin/env python3
"""Metric depth and lifted views (mudg_amd/depth.py, csrc/depth.hip) on ONE MI355X, on a seeded 16-frame 576 x 1024 stream.

`python tools/depth_bench.py [--frames 16] [--runs 3] [--no-ddim] [--out profiles/r13/depth_bench.txt]`

Every time is taken between two device events after a warm-up (tools/splat_bench.py's event_ms), `--runs` times; median [min .. max].
  align      the three launches of the fit: the zeroing of the sums, mudg_depth_align_sums (7 bytes read per pixel) and
             mudg_depth_align_solve
  finish     mudg_depth_finish with the labels and the picture (11 bytes read, 7 written per pixel)
  unproject  mudg_depth_unproject with the labels (15 bytes read, 17 written per pixel)
Each with the bytes its rule needs per second beside the 6.29 TB/s a float4 copy reaches on this chip, and one DDIM step of the flagship
workload in the same process alongside (tools/splat_bench.py's ddim_step_ms)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from mudg_amd import depth, ops
from splat_bench import ddim_step_ms, event_ms, spread

COPY_TBS, HW_OUT = 6.29, (576, 1024)


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
        sys.exit("depth_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    T, (H, W) = args.frames, HW_OUT
    pixels = T * H * W
    gen = torch.Generator(device=dev).manual_seed(13)
    u8 = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    lidar = u8.sum(dim=3).float() * (90.0 / 765.0) + 3.0 + torch.randn((T, H, W), device=dev, generator=gen)
    lidar[torch.rand((T, H, W), device=dev, generator=gen) < 0.6] = 0.0                   # a rendered cloud leaves most pixels empty
    labels = torch.randint(0, 19, (T, H, W), dtype=torch.int64, device=dev, generator=gen)
    rgb = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    c2w = np.stack([np.eye(4)] * T)
    c2w[:, 0, 3] = np.arange(T) * 0.5
    table = torch.from_numpy(depth.camera_table(np.array([[2000.0, 0, 960.0], [0, 2000.0, 640.0], [0, 0, 1]]), c2w, (1280, 1920), HW_OUT)).to(dev)
    say(f"depth_bench on {torch.cuda.get_device_name(0)}: {T} frames of {H} x {W}; median [min .. max] of {args.runs} runs")

    state = {}

    def align():
        state["sums"] = ops.depth_align_sums(u8, lidar)                                    # zeroes the sums, then the sums kernel
        state["coef"], state["fitted"] = ops.depth_align_solve(state["sums"])
    stages = (("align (zero + sums + solve)", align, 7),
              ("finish (labels, picture)", lambda: ops.depth_finish(u8, state["coef"], labels, visualise=True), 18),
              ("unproject (labels)", lambda: ops.depth_unproject(state["depth"], rgb, table, labels), 32))
    total = 0.0
    for name, fn, nbytes in stages:
        fn()
        if "depth" not in state and "coef" in state:
            state["depth"] = ops.depth_finish(u8, state["coef"], labels)[0]
        torch.cuda.synchronize()
        ms = spread([event_ms(fn) for _ in range(args.runs)])
        total += ms["median"]
        say(f"  {name:30s} {fmt(ms)}; {pixels * nbytes / (ms['median'] * 1e-3) / 1e12:.3f} TB/s of {COPY_TBS} TB/s (copy), {nbytes} bytes per pixel")
    say(f"  fitted {int(state['fitted'].sum())} of {T} frames; all three stages {total:.4f} ms per {T}-frame stream")
    whole = lambda: depth.metric_depth(u8, lidar, labels, visualise=True)
    whole()
    say(f"  metric_depth (the interface, visualise=True) {fmt(spread([event_ms(whole) for _ in range(args.runs)]))}")
    if not args.no_ddim:
        step = ddim_step_ms(args.runs, dev)
        say(f"  one DDIM step of the flagship workload in this process: {fmt(step)}; the three stages are {100 * total / step['median']:.3f} % of one step")


if __name__ == "__main__":
    main()
