#!/usr/bin/env python3
"""The CLIP image tower (mudg_amd/towers.py, engine/clip.py, csrc/towers.hip) on ONE MI355X at its real size — ViT-H/14: width 1280, 32
blocks, 16 heads of 80, 257 tokens — with random weights, from 576 x 1024 frames.

`python tools/tower_bench.py [--runs 5] [--reps 10] [--no-ddim] [--operands bf16,bf16x3] [--out profiles/towers/bench.txt]`

The operand type is fixed per process, so each library runs in a child process of this tool and its lines are gathered here.  In a
child, every time is taken between two device events (tools/splat_bench.py's event_ms) around `--reps` calls, after a warm-up of every
shape, `--runs` times; median [min .. max] per call: the preprocessing, one block on the fp32 stream, and the whole tower at B = 1, 3
and 6; then one DDIM step of the flagship workload in the same process (tools/splat_bench.py's ddim_step_ms), against which a window's
tower work — two calls at B = 3, the frames and the all-zero images — is stated.  FLOPs are counted here from the shapes."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HW = (576, 1024)
BATCHES = (1, 3, 6)
WIDTH, LAYERS, HEADS, TOKENS, MLP = 1280, 32, 16, 257, 5120


def block_flops(b):
    return b * (2.0 * TOKENS * WIDTH * (3 * WIDTH + WIDTH + 2 * MLP) + 4.0 * TOKENS * TOKENS * WIDTH)


def tower_flops(b):
    return LAYERS * block_flops(b) + b * 2.0 * 256 * 588 * WIDTH


def fmt(s, unit="ms"):
    return f"{s['median']:.4f} {unit} [{s['min']:.4f} .. {s['max']:.4f}]"


def child(args):
    import torch

    from mudg_amd import hip, ops
    from mudg_amd.engine import clip
    from mudg_amd.towers import FrozenOpenCLIPImageEmbedderV2
    from splat_bench import ddim_step_ms, event_ms, spread
    if not torch.cuda.is_available():
        sys.exit("tower_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")

    def say(line):
        print("| " + line, flush=True)

    torch.manual_seed(7)
    with torch.device(dev):
        tower = FrozenOpenCLIPImageEmbedderV2(text_leftovers=False)
    blk = tower.model.visual.transformer.resblocks[0]
    say(f"{hip.operand_name()} library on {torch.cuda.get_device_name(0)}: ViT-H/14, {LAYERS} blocks, frames {HW[0]} x {HW[1]}; per call, median "
        f"[min .. max] of {args.runs} windows of {args.reps} calls")

    def timed(fn):
        return event_ms(lambda: [fn() for _ in range(args.reps)]) / args.reps

    window = None
    with torch.no_grad():
        for b in BATCHES:
            x = torch.rand((b, 3) + HW, device=dev) * 2 - 1
            stream = torch.randn((b * TOKENS, WIDTH), device=dev)
            paths = {"preprocess": lambda: ops.clip_preprocess(x), "block": lambda: clip.block(blk, stream, b, HEADS, TOKENS, WIDTH // HEADS),
                     "tower": lambda: tower(x)}
            for fn in paths.values():
                fn()
                fn()
            torch.cuda.synchronize()
            ms = {name: [] for name in paths}
            for _ in range(args.runs):
                for name, fn in paths.items():
                    ms[name].append(timed(fn))
            s = {name: spread(v) for name, v in ms.items()}
            say(f"  B = {b}: preprocessing {fmt(s['preprocess'])}")
            say(f"         one block     {fmt(s['block'])}; {block_flops(b) / (s['block']['median'] * 1e-3) / 1e12:.1f} TFLOP/s of {block_flops(b) / 1e9:.1f} GFLOP")
            say(f"         whole tower   {fmt(s['tower'])}; {tower_flops(b) / (s['tower']['median'] * 1e-3) / 1e12:.1f} TFLOP/s of {tower_flops(b) / 1e12:.3f} TFLOP")
            if b == 3:
                window = 2.0 * s["tower"]["median"]
    if not args.no_ddim:
        del tower, blk
        torch.cuda.empty_cache()
        step = ddim_step_ms(3, dev)
        say(f"  one DDIM step of the flagship workload in this process: {fmt(step)}; a window's tower work (two calls at B = 3) is {window:.3f} ms, "
            f"{100 * window / step['median']:.2f} % of one step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-ddim", action="store_true")
    ap.add_argument("--operands", default="bf16,bf16x3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = ["tower_bench: the CLIP image tower at its real size, one child process per library"]
    for operand in args.operands.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--runs", str(args.runs), "--reps", str(args.reps)] + (["--no-ddim"] if args.no_ddim else [])
        proc = subprocess.run(cmd, env=dict(os.environ, MUDG_OPERAND=operand), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        got = [l[2:] for l in proc.stdout.splitlines() if l.startswith("| ")]
        lines += got
        print("\n".join(got), flush=True)
        if proc.returncode != 0:
            print(proc.stdout[-4000:])
            sys.exit(f"tower_bench: the {operand} child ended with {proc.returncode}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
