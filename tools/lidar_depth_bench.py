#!/usr/bin/env python3
"""LiDAR depth maps and their completion (csrc/lidar_depth.hip) on ONE MI355X: a 16-frame sequence of six-sweep windows
from mudg_amd.synthetic.street_sweeps (64 beams x 1325 azimuths), at 576 x 1024 and at 1280 x 1920.

`python tools/lidar_depth_bench.py [--frames 16] [--runs 5] [--no-ddim] [--out profiles/lidar_depth/bench.txt]`

One pass over the frames with the launches of depth.lidar_depth_maps and an event between the stages (tools/splat_bench.py's
kernel_buckets does the same for the conditions), `--runs` passes after a warm-up; median [min .. max] per 16-frame sequence.
  occluders  mudg_splat_points at size 1 into Z: 16 bytes read per candidate, 8 written per pixel of Z
  visible    mudg_lidar_splat_visible and mudg_lidar_depth_resolve: 16 bytes read per candidate, per pixel 8 read of Z, 8 written and
             8 read of the keys, 4 written of depth and 16 for leaving both key images empty
  complete   mudg_depth_complete with the source map: 4 bytes read and 5 written per pixel
Each with the bytes its rule needs per second, beside a device-to-device copy that moves the same number of bytes (half read, half
written) measured in the same process, and one DDIM step of the flagship workload alongside (tools/splat_bench.py's ddim_step_ms).
The events of the two splat stages bracket Python closures (one to three launches and the host work between them, per frame): their
times include host launch gaps, so their bytes/s say more about launch overhead than about memory rate.
Nothing here is asserted: the file records."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from mudg_amd import depth, render
from mudg_amd.synthetic import street_sweeps
from splat_bench import ddim_step_ms, event_ms, spread

SIZES = ((576, 1024), (1280, 1920))


def fmt(s, unit="ms"):
    return f"{s['median']:.4f} {unit} [{s['min']:.4f} .. {s['max']:.4f}]"


def staged_ms(passes):
    """One pass over the frames: (ms in the occluder launches, ms in the visible launches and the resolve)."""
    marks = []
    for occluders, visible in passes:
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        occluders()
        e[1].record()
        visible()
        e[2].record()
        marks.append(e)
    torch.cuda.synchronize()
    return sum(e[0].elapsed_time(e[1]) for e in marks), sum(e[1].elapsed_time(e[2]) for e in marks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-ddim", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lidar_depth_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    T = args.frames
    scenario, load_lidar, load_image = street_sweeps(frames=T, beams=64, azimuths=1325, seed=0)
    scene = render.Scene.from_scenario(scenario, load_lidar, load_image, keep_sweeps=True, device=dev)
    offsets = scene.sweeps.offsets.tolist()
    candidates = sum(offsets[max(depth.window_frames(t, T)) + 1] - offsets[min(depth.window_frames(t, T))] for t in range(T))
    if scene.objects is not None:
        candidates += sum(len(scene.objects.cloud) for t in range(T) if scene.objects.visible(t))
    say(f"lidar_depth_bench on {torch.cuda.get_device_name(0)}: {T} frames, {offsets[-1]} returns in the sweeps, {candidates} candidates over the "
        f"{T} windows; median [min .. max] of {args.runs} runs")
    total = {}
    for H, W in SIZES:
        px = T * H * W
        out, passes = depth._lidar_depth_passes(scene.sweeps, scene.objects, scene.intr, scene.c2w, scene.hw_native, (H, W))
        staged_ms(passes)                                                     # warm-up
        runs = [staged_ms(passes) for _ in range(args.runs)]
        state = {}

        def complete():
            state["dense"] = depth.complete_depth(out, return_source=True)
        complete()
        torch.cuda.synchronize()
        stages = (("occluders (size 1)", spread([r[0] for r in runs]), candidates * 16 + px * 8),
                  ("visible (reach 4) + resolve", spread([r[1] for r in runs]), candidates * 16 + px * 44),
                  ("complete (extrapolate, source)", spread([event_ms(complete) for _ in range(args.runs)]), px * 9))
        say(f" {H} x {W}: covered by returns {float((out > 0).float().mean()):.4f}, dense {float((state['dense'][0] > 0).float().mean()):.4f} of the pixels")
        total[(H, W)] = 0.0
        for name, ms, nbytes in stages:
            a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            b = torch.empty_like(a)
            b.copy_(a)
            torch.cuda.synchronize()
            copy = spread([event_ms(lambda: b.copy_(a)) for _ in range(args.runs)])
            del a, b
            total[(H, W)] += ms["median"]
            say(f"  {name:32s} {fmt(ms)}; {nbytes / (ms['median'] * 1e-3) / 1e12:.3f} TB/s of the {nbytes / 1e6:.1f} MB its rule needs; "
                f"a copy of the same bytes {fmt(copy)}, {nbytes / (copy['median'] * 1e-3) / 1e12:.3f} TB/s")
        say(f"  all three stages {total[(H, W)]:.4f} ms per {T}-frame sequence")
    if not args.no_ddim:
        step = ddim_step_ms(args.runs, dev)
        say(f" one DDIM step of the flagship workload in this process: {fmt(step)}; the three stages are "
            + ", ".join(f"{100 * v / step['median']:.2f} % ({h} x {w})" for (h, w), v in total.items()) + " of one step")


if __name__ == "__main__":
    main()
