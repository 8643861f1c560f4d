#!/usr/bin/env python3
"""The dense streams of a clip (mudg_amd/frames.py, csrc/frames.hip) on ONE MI355X: one seeded 16-frame stream 1280 x 1920 -> 576 x 1024
and -> 320 x 512, per kind.

`python tools/frames_bench.py [--frames 16] [--runs 5] [--reps 200] [--no-ddim] [--out profiles/frames/bench.txt]`

Every time is taken between two device events (tools/splat_bench.py's event_ms) around `--reps` calls, after a warm-up of every shape,
`--runs` times; median [min .. max] per call.  The fused stream and the torch chain a user would otherwise write on the GPU
(F.interpolate(bilinear, align_corners=False), normalise, permute; for labels the palette gather first) are timed alternately in one
process; the two do not compute the same pixels, the chain stands for the work, not for the result.  Bytes are computed
here from the shapes: the source rows the vertical table touches, whole, plus the three fp32 planes written; the rate is those bytes
over the time, beside a plain device copy moving the same number of bytes (half read, half written) and one DDIM step of the flagship
workload in the same process (tools/splat_bench.py's ddim_step_ms)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import torch.nn.functional as F

from mudg_amd import frames, ops
from splat_bench import ddim_step_ms, event_ms, spread

HW_NATIVE = (1280, 1920)
SIZES = ((576, 1024), (320, 512))
SOURCE_BYTES = {"color": 3, "semantic": 1, "depth": 4}             # per source pixel


def fmt(s, unit="ms"):
    return f"{s['median']:.4f} {unit} [{s['min']:.4f} .. {s['max']:.4f}]"


def stream_bytes(kind, frames_n, hw_in, hw_out):
    """What the rule needs: every source row named by the vertical table, whole, and the three fp32 planes."""
    table = ops.resize_table(hw_in[0], hw_out[0], "linear_f32" if kind == "depth" else "linear_u8")
    rows = len(np.unique(table[:, :2]))
    return frames_n * (rows * hw_in[1] * SOURCE_BYTES[kind] + 3 * hw_out[0] * hw_out[1] * 4)


def torch_chain(kind, src, hw_out, palette):
    if kind == "depth":
        x = F.interpolate(src[:, None], size=hw_out, mode="bilinear", align_corners=False)
        x = (torch.clamp(x, 0, 100) / 100.0 - 0.5) * 2
        return x.expand(-1, 3, -1, -1).permute(1, 0, 2, 3).contiguous()
    if kind == "semantic":
        src = palette[src.long()]
    x = F.interpolate(src.permute(0, 3, 1, 2).float(), size=hw_out, mode="bilinear", align_corners=False)
    return ((x / 255 - 0.5) * 2).permute(1, 0, 2, 3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--no-ddim", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frames_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    T, (H0, W0) = args.frames, HW_NATIVE
    gen = torch.Generator(device=dev).manual_seed(16)
    sources = {"color": torch.randint(0, 256, (T, H0, W0, 3), dtype=torch.uint8, device=dev, generator=gen),
               "semantic": torch.randint(0, 21, (T, H0, W0), dtype=torch.uint8, device=dev, generator=gen),
               "depth": torch.rand((T, H0, W0), device=dev, generator=gen) * 120.0}
    palette = torch.randint(0, 256, (256, 3), dtype=torch.uint8, device=dev, generator=gen)          # the chain's gather; the values do not matter
    fused = {"color": frames.stream_from_images, "semantic": frames.stream_from_labels, "depth": frames.stream_from_depth}
    say(f"frames_bench on {torch.cuda.get_device_name(0)}: one {T}-frame stream {H0} x {W0} -> h x w; per call, median [min .. max] of "
        f"{args.runs} windows of {args.reps} calls, fused and torch windows alternating")

    def timed(fn):
        return event_ms(lambda: [fn() for _ in range(args.reps)]) / args.reps

    fused_total = {}
    for hw in SIZES:
        fused_total[hw] = 0.0
        for kind, src in sources.items():
            out = torch.empty((3, T) + hw, dtype=torch.float32, device=dev)
            nbytes = stream_bytes(kind, T, HW_NATIVE, hw)
            a, b = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            paths = {"fused": lambda: fused[kind](src, hw, out), "torch": lambda: torch_chain(kind, src, hw, palette), "copy": lambda: b.copy_(a)}
            for fn in paths.values():                                                                 # warm up every shape
                fn()
                fn()
            torch.cuda.synchronize()
            ms = {name: [] for name in paths}
            for _ in range(args.runs):
                for name, fn in paths.items():
                    ms[name].append(timed(fn))
            s = {name: spread(v) for name, v in ms.items()}
            fused_total[hw] += s["fused"]["median"]
            rate = lambda name: nbytes / (s[name]["median"] * 1e-3) / 1e12
            say(f"  {kind:8s} -> {hw[0]} x {hw[1]}: {nbytes / 1e6:.1f} MB (source rows touched + planes written)")
            say(f"      fused stream  {fmt(s['fused'])}; {rate('fused'):.3f} TB/s")
            say(f"      torch chain   {fmt(s['torch'])}; {s['torch']['median'] / s['fused']['median']:.2f} x the fused stream")
            say(f"      device copy   {fmt(s['copy'])}; {rate('copy'):.3f} TB/s for the same bytes")
            del a, b, out
        say(f"  three streams -> {hw[0]} x {hw[1]}: {fused_total[hw]:.4f} ms fused")
    if not args.no_ddim:
        del sources
        step = ddim_step_ms(3, dev)
        say(f"  one DDIM step of the flagship workload in this process: {fmt(step)}; the three fused streams at {SIZES[0][0]} x {SIZES[0][1]} are "
            f"{100 * fused_total[SIZES[0]] / step['median']:.3f} % of one step")


if __name__ == "__main__":
    main()
