#!/usr/bin/env python3
"""Surface normals (csrc/normals.hip) on ONE MI355X, on a seeded 16-frame 576 x 1024 stream.

`python tools/normals_bench.py [--frames 16] [--runs 5] [--no-ddim] [--out profiles/normals/bench.txt]`

Every time is taken between two device events after a warm-up (tools/splat_bench.py's event_ms), `--runs` times; median [min .. max].
  normals  mudg_depth_normals with the labels and a step limit (12 bytes read, 13 written per pixel)
  stream   mudg_normal_stream, 1280 x 1920 -> 576 x 1024 (12 bytes read per source pixel, 12 written per output pixel)
  errors   the zeroing of the counts and mudg_metric_normals with the validity bytes (16 bytes read per pixel)
Each with the bytes its rule needs per second, beside a device-to-device copy that moves the same number of bytes (half read, half
written) measured in the same process, and one DDIM step of the flagship workload alongside (tools/splat_bench.py's ddim_step_ms)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from mudg_amd import ops, render
from splat_bench import ddim_step_ms, event_ms, spread

HW_OUT, HW_SRC = (576, 1024), (1280, 1920)


def fmt(s, unit="ms"):
    return f"{s['median']:.4f} {unit} [{s['min']:.4f} .. {s['max']:.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-ddim", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("normals_bench: no GPU (a CPU run measures nothing)")
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
    gen = torch.Generator(device=dev).manual_seed(19)
    j, i = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    z = 20.0 + 8.0 * torch.sin(0.011 * i + 0.3) * torch.cos(0.017 * j) + 0.02 * torch.randn((T, H, W), device=dev, generator=gen)
    z[torch.rand((T, H, W), device=dev, generator=gen) < 0.1] = 0.0                        # holes
    labels = torch.randint(0, 19, (T, H, W), dtype=torch.int64, device=dev, generator=gen)
    cam = render.scaled_intrinsics(np.array([[2000.0, 0, 960.0], [0, 2000.0, 640.0], [0, 0, 1]]), HW_SRC, HW_OUT)
    table = torch.from_numpy(np.tile(cam, (T, 1))).to(dev)
    maps = torch.randn((T,) + HW_SRC + (3,), device=dev, generator=gen)
    maps /= maps.norm(dim=3, keepdim=True)
    pred = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    say(f"normals_bench on {torch.cuda.get_device_name(0)}: {T} frames of {H} x {W}; median [min .. max] of {args.runs} runs")

    state = {}

    def normals():
        state["normals"], state["valid"] = ops.depth_normals(z, table, labels, max_rel_step=0.05)
    out_px, src_px = T * H * W, T * HW_SRC[0] * HW_SRC[1]
    stages = (("normals (labels, step limit)", normals, out_px * 25),
              ("stream 1280 x 1920 -> 576 x 1024", lambda: ops.normal_stream(maps, HW_OUT), src_px * 12 + out_px * 12),
              ("errors (zero + counts, valid)", lambda: ops.metric_normals(pred, state["normals"], state["valid"]), out_px * 16))
    total = 0.0
    for name, fn, nbytes in stages:
        fn()
        torch.cuda.synchronize()
        ms = spread([event_ms(fn) for _ in range(args.runs)])
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        b = torch.empty_like(a)
        b.copy_(a)
        torch.cuda.synchronize()
        copy = spread([event_ms(lambda: b.copy_(a)) for _ in range(args.runs)])
        del a, b
        total += ms["median"]
        say(f"  {name:34s} {fmt(ms)}; {nbytes / (ms['median'] * 1e-3) / 1e12:.3f} TB/s of the {nbytes / 1e6:.1f} MB its rule needs; "
            f"a copy of the same bytes {fmt(copy)}, {nbytes / (copy['median'] * 1e-3) / 1e12:.3f} TB/s")
    say(f"  valid normals: {float(state['valid'].float().mean()):.4f} of the pixels; all three stages {total:.4f} ms per {T}-frame stream")
    if not args.no_ddim:
        step = ddim_step_ms(args.runs, dev)
        say(f"  one DDIM step of the flagship workload in this process: {fmt(step)}; the three stages are {100 * total / step['median']:.3f} % of one step")


if __name__ == "__main__":
    main()
