#!/usr/bin/env python3
"""The scores of generated views (mudg_amd/metrics.py, csrc/metrics.hip) on ONE MI355X, on a seeded 16-frame 576 x 1024 stream.

`python tools/metrics_bench.py [--frames 16] [--runs 3] [--no-ddim] [--out profiles/r14/metrics_bench.txt]`

Every time is taken between two device events after a warm-up (tools/splat_bench.py's event_ms), `--runs` times; median [min .. max].
Each entry point with the zeroing of its sums, and the bytes its rule needs per pixel:
  sse        mudg_metric_sse: two uint8 frames, 6 bytes read
  ssim       mudg_metric_ssim: the same 6 bytes (the aprons come from the cache)
  depth      mudg_metric_depth: two fp32 maps, 8 bytes read
  confusion  mudg_metric_confusion: two int64 label maps, 16 bytes read
beside the rate of a plain device copy of 256 MiB measured in the same process, and one DDIM step of the flagship workload in the same
process alongside (tools/splat_bench.py's ddim_step_ms)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

from mudg_amd import metrics, ops
from splat_bench import ddim_step_ms, event_ms, spread

HW_OUT = (576, 1024)


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
        sys.exit("metrics_bench: no GPU (a CPU run measures nothing)")
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
    gen = torch.Generator(device=dev).manual_seed(14)
    a = torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    b = (a.float() + 12.0 * torch.randn((T, H, W, 3), device=dev, generator=gen)).round().clamp(0, 255).to(torch.uint8)
    lidar = torch.rand((T, H, W), device=dev, generator=gen) * 79.0 + 0.5
    lidar[torch.rand((T, H, W), device=dev, generator=gen) < 0.6] = 0.0                   # a rendered cloud leaves most pixels empty
    depth = lidar * (0.6 + 1.1 * torch.rand((T, H, W), device=dev, generator=gen)) + 1.0
    gt = torch.randint(0, 19, (T, H, W), dtype=torch.int64, device=dev, generator=gen)
    pred = torch.where(torch.rand((T, H, W), device=dev, generator=gen) < 0.7, gt, torch.randint(0, 19, (T, H, W), dtype=torch.int64, device=dev, generator=gen))
    say(f"metrics_bench on {torch.cuda.get_device_name(0)}: {T} frames of {H} x {W}; median [min .. max] of {args.runs} runs")

    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    copy = spread([event_ms(lambda: dst.copy_(src)) for _ in range(args.runs)])
    copy_tbs = 2 * src.numel() / (copy["median"] * 1e-3) / 1e12
    say(f"  a plain copy of 256 MiB (read + write)  {fmt(copy)}; {copy_tbs:.3f} TB/s")
    del src, dst

    stages = (("sse", lambda: ops.metric_sse(a, b), 6), ("ssim", lambda: ops.metric_ssim(a, b), 6),
              ("depth", lambda: ops.metric_depth(depth, lidar), 8), ("confusion", lambda: ops.metric_confusion(pred, gt), 16))
    total = 0.0
    for name, fn, nbytes in stages:
        fn()
        torch.cuda.synchronize()
        ms = spread([event_ms(fn) for _ in range(args.runs)])
        total += ms["median"]
        say(f"  {name:10s} (zero + kernel)  {fmt(ms)} per stream; {pixels * nbytes / (ms['median'] * 1e-3) / 1e12:.3f} TB/s of {copy_tbs:.3f} TB/s (copy), {nbytes} bytes per pixel")
    say(f"  all four entry points {total:.4f} ms per {T}-frame stream")
    outputs = {"color": a, "depth": depth, "semantic_labels": pred}
    whole = lambda: metrics.score_window(outputs, color=b, lidar_depth=lidar, labels=gt)
    scores = whole()
    say(f"  score_window (the interface, all three truths) {fmt(spread([event_ms(whole) for _ in range(args.runs)]))}")
    say(f"  frame 0: psnr {float(scores['color_psnr'][0]):.4f} dB, ssim {float(scores['color_ssim'][0]):.4f}, mae {float(scores['depth_mae'][0]):.4f} m, "
        f"d1 {float(scores['depth_d1'][0]):.4f}, miou {float(scores['semantic_miou'][0]):.4f}")
    if not args.no_ddim:
        step = ddim_step_ms(args.runs, dev)
        say(f"  one DDIM step of the flagship workload in this process: {fmt(step)}; the four entry points are {100 * total / step['median']:.3f} % of one step")


if __name__ == "__main__":
    main()
