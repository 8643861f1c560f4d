#!/usr/bin/env python3
"""Micro-benchmarks of the kernels at the shapes the MDM1024 UNet issues (B = 1): TFLOP/s or GB/s per launch.
Run on the GPU box:  python tools/kernel_bench.py [filter]
`python tools/kernel_bench.py fused` is the table behind the rule of the fused temporal self-attention (fused_temporal below);
`MUDG_DEBUG_VARIANTS=1 python tools/kernel_bench.py stream` times the stream kernel (csrc/sgemm.hip) against the kernels it replaces."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mudg_amd import ops

dev = torch.device("cuda")
BF = torch.bfloat16


def timeit(fn, iters=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def rn(*s, dtype=BF):
    return (torch.randn(*s, device=dev) * 0.5).to(dtype)


def report(name, sec, flops=None, bytes_=None):
    msg = f"{name:58s} {sec * 1e6:9.1f} us"
    if flops:
        msg += f"  {flops / sec / 1e12:8.1f} TFLOP/s"
    if bytes_:
        msg += f"  {bytes_ / sec / 1e9:8.1f} GB/s"
    print(msg, flush=True)


def spread(fn, repeats=7, iters=10):
    """(median, min, max) seconds per call over `repeats` timings of `iters` back-to-back calls."""
    fn()
    ts = sorted(timeit(fn, iters=iters, warm=1) for _ in range(repeats))
    return ts[len(ts) // 2], ts[0], ts[-1]


# (name, clips, (level, hw, C) ...) of the temporal transformers: the one behind the input convolution (`in`: C = 512 on half the
# level-0 pixels, the shape a step profile shows) and those of the four levels.  Cond + uncond are stacked, so a step of B clips runs
# 2 B clips.  The last is the small UNet of the tests (tests/golden/unet_a.pt), whose 6-pixel level the query refuses.
def _mdm(h, w):
    return (("in", h * w // 2, 512),) + tuple((lv, (h >> lv) * (w >> lv), c) for lv, c in enumerate((320, 640, 1280, 1280)))


TEMPORAL_CONFIGS = [("MDM1024", 2, _mdm(72, 128)), ("MDM512", 2, _mdm(40, 64)), ("MDM1024 B=3", 6, _mdm(72, 128)),
                    ("test UNet", 1, ((0, 384, 64), (1, 96, 128), (2, 24, 256), (3, 6, 256)))]


def fused_temporal(T=16):
    """The fused temporal self-attention against the two launches it replaces, per level of every configuration the rule in
    engine/unet.py (_tsattn_fused) has to decide: the qkv GEMM alone, the temporal attention alone, the two alternating as a step
    issues them (`pair`: the figure the rule compares; it is not the sum of the two columns before it, which time each kernel
    back-to-back with itself), and the fused launch.  One markdown row per shape."""
    print("| config | level | rows | C | gemm us | tattn us | pair us (min..max) | fused us (min..max) | fused TFLOP/s | fused / pair |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    for name, clips, levels in TEMPORAL_CONFIGS:
        for level, hw, c in levels:
            heads, M = c // 64, clips * T * hw
            if not ops.temporal_self_attention_ok(T, hw, heads, c):
                print(f"| {name} | {level} | {M} | {c} | refused by the query |", flush=True)
                continue
            x, w = rn(M, c), rn(3 * c, c)           # timing does not depend on the row order of w: no head packing here
            out = torch.empty(M, c, device=dev, dtype=BF)
            qkv = ops.gemm(x, w, frame_rows=hw)

            def pair():
                q = ops.gemm(x, w, frame_rows=hw)
                ops.temporal_attention(q, out, clips=clips, t=T, hw=hw, heads=heads)

            g = spread(lambda: ops.gemm(x, w, frame_rows=hw))
            a = spread(lambda: ops.temporal_attention(qkv, out, clips=clips, t=T, hw=hw, heads=heads))
            p = spread(pair)
            f = spread(lambda: ops.temporal_self_attention(x, w, out, clips=clips, t=T, hw=hw, heads=heads))
            flops = 2.0 * M * 3 * c * c + 4.0 * clips * hw * heads * T * T * 64
            us = lambda s: f"{s[0] * 1e6:.1f} ({s[1] * 1e6:.1f}..{s[2] * 1e6:.1f})"
            print(f"| {name} | {level} | {M} | {c} | {g[0] * 1e6:.1f} | {a[0] * 1e6:.1f} | {us(p)} | {us(f)} | {flops / f[0] / 1e12:.0f} | "
                  f"{f[0] / p[0]:.3f} |", flush=True)
            del x, w, out, qkv
            torch.cuda.empty_cache()


def stream_projections(T=16):
    """The square projections of an MDM1024 step (two clips: cond + uncond), the stream kernel (MUDG_GEMM_STREAM=1: its rule) against the
    tile kernels (= 0), alternating in one process — the debug-variants library reads the switch at every call.  Median (min..max) of 7
    timings of 10 back-to-back launches.  Back-to-back launches of one shape find part of their operands in the 256-MiB last-level
    cache: the rule is decided inside a step (tools/shape_profile.py), this table says what a launch costs at best.  The kernel takes
    K = 320 with N = 320 or 640; the level-1 rows show what the switch leaves alone."""
    from mudg_amd import hip
    if os.environ.get("MUDG_DEBUG_VARIANTS") != "1":
        sys.exit("stream: run with MUDG_DEBUG_VARIANTS=1 (the library that reads MUDG_GEMM_STREAM)")
    F16 = torch.float16
    print("| shape (M x N x K) | flags | algorithmic MB | tiles us (min..max) | stream us (min..max) | stream TB/s | stream / tiles |")
    print("|---|---|---:|---:|---:|---:|---:|")
    shapes = [(2 * T * 9216, 320, 320, 9216), (2 * T * 2304, 640, 640, 2304), (2 * T * 9216, 640, 320, 9216)]
    for M, n, k, hw in shapes:
        for flags in ("bias, fp16 residual, fp16 out", "bias", "none"):
            if n != k and flags != "none":
                continue
            x, w = rn(M, k), rn(n, k)
            bias = torch.randn(n, device=dev) if flags != "none" else None
            res = rn(M, n, dtype=F16) if "residual" in flags else None
            out = torch.empty(M, n, device=dev, dtype=F16 if res is not None else BF)
            call = lambda: ops.gemm(x, w, out=out, bias=bias, residual=res, frame_rows=hw)
            t = {}
            for rep in range(2):                           # tiles, stream, tiles, stream: the second pair is reported
                for sw in ("0", "1"):
                    os.environ["MUDG_GEMM_STREAM"] = sw
                    t[sw] = spread(call)
            mb = (M * k + n * k + M * n * (2 if res is not None else 1)) * 2 / 1e6
            us = lambda v: f"{v[0] * 1e6:.1f} ({v[1] * 1e6:.1f}..{v[2] * 1e6:.1f})"
            print(f"| {M} x {n} x {k} | {flags} | {mb:.0f} | {us(t['0'])} | {us(t['1'])} | {mb / t['1'][0] / 1e6:.2f} | {t['1'][0] / t['0'][0]:.3f} |",
                  flush=True)
            del x, w, out, res
            torch.cuda.empty_cache()
    os.environ.pop("MUDG_GEMM_STREAM", None)


def main():
    flt = sys.argv[1] if len(sys.argv) > 1 else ""
    if flt == "fused":
        return fused_temporal()
    if flt == "stream":
        return stream_projections()
    T = 16
    levels = [(72 * 128, 320), (36 * 64, 640), (18 * 32, 1280), (9 * 16, 1280)]
    if "gemm" in flt or not flt:
        for hw, c in levels[:3]:
            M = T * hw
            for (n, k, tag) in [(c, c, "proj CxC"), (2 * c, c, "qk 2CxC"), (3 * c, c, "qkv 3CxC"), (c, 4 * c, "ff2 Cx4C")]:
                x, w = rn(M, k), rn(n, k)
                res = torch.randn(M, n, device=dev)
                report(f"gemm M={M} N={n} K={k} {tag} (+fp32 res/out)", timeit(lambda: ops.gemm(x, w, residual=res, out_fp32=True)), 2.0 * M * n * k)
                report(f"gemm M={M} N={n} K={k} {tag} (bf16 out)", timeit(lambda: ops.gemm(x, w)), 2.0 * M * n * k)
            x, w = rn(M, c), rn(8 * c, c)
            b = torch.randn(8 * c, device=dev)
            report(f"gemm M={M} N={8 * c} K={c} ff1 GEGLU", timeit(lambda: ops.gemm(x, w, bias=b, geglu=True)), 2.0 * M * 8 * c * c)
    if "conv" in flt or not flt:
        for (h, w_, cin, cout) in [(72, 128, 320, 320), (72, 128, 640, 320), (72, 128, 960, 320), (36, 64, 640, 640),
                                   (36, 64, 1280, 640), (18, 32, 1280, 1280), (18, 32, 2560, 1280), (9, 16, 2560, 1280)]:
            x, wt = rn(T * h * w_, cin), rn(cout, 9 * cin)
            for ko in (0, 1):
                report(f"conv3x3 {h}x{w_} {cin}->{cout} korder={ko}", timeit(lambda: ops.conv3x3(x, wt, frames=T, hin=h, win=w_, cin=cin, korder=ko)),
                       2.0 * T * h * w_ * cout * 9 * cin)
        for hw, c in levels:
            x, wt = rn(T * hw, c), rn(c, 3 * c)
            report(f"tconv3 hw={hw} C={c}", timeit(lambda: ops.tconv3(x, wt, clips=1, t=T, hw=hw, cin=c)), 2.0 * T * hw * c * 3 * c)
    if "attn" in flt or not flt:
        for hw, c in levels[:3]:
            heads = c // 64
            qk = rn(T * hw, 2 * c)
            vt = rn(T * c, hw)
            out = torch.empty(T * hw, c, device=dev, dtype=BF)
            report(f"attention N={hw} heads={heads} F={T}", timeit(lambda: ops.attention(qk[:, :c], qk[:, c:], vt, out, frames=T, heads=heads, nq=hw, nk=hw, ldvt=hw, svt=c * hw)),
                   4.0 * T * heads * hw * hw * 64)
            q = rn(T * hw, c); kt = rn(77, c); vtt = rn(c, 80)
            report(f"cross-attn text N={hw} heads={heads}", timeit(lambda: ops.attention(q, kt, vtt, out, frames=T, heads=heads, nq=hw, nk=77, ldvt=80, svt=c * 80, kv_div=T)),
                   4.0 * T * heads * hw * 77 * 64, bytes_=2.0 * T * hw * c * 2)
            qkv = rn(T * hw, 3 * c)
            report(f"temporal attn hw={hw} heads={heads}", timeit(lambda: ops.temporal_attention(qkv, out, clips=1, t=T, hw=hw, heads=heads)),
                   bytes_=T * hw * c * 2.0 * 4)
    if "norm" in flt or not flt:
        for hw, c in [(72 * 128, 320), (72 * 128, 960), (36 * 64, 640), (18 * 32, 1280), (9 * 16, 2560)]:
            x = torch.randn(T * hw, c, device=dev)
            g, b = torch.ones(c, device=dev), torch.zeros(c, device=dev)
            report(f"groupnorm fp32-in frame-stats hw={hw} C={c}", timeit(lambda: ops.groupnorm(x, g, b, samples=T, rows=hw, eps=1e-5, silu=True)), bytes_=T * hw * c * 10.0)
            report(f"groupnorm fp32-in clip-stats  hw={hw} C={c}", timeit(lambda: ops.groupnorm(x, g, b, samples=1, rows=T * hw, eps=1e-5, silu=True)), bytes_=T * hw * c * 10.0)
            xb = x.to(BF)
            report(f"groupnorm bf16-in clip-stats  hw={hw} C={c}", timeit(lambda: ops.groupnorm(xb, g, b, samples=1, rows=T * hw, eps=1e-5, silu=True)), bytes_=T * hw * c * 6.0)
            report(f"layernorm fp32-in rows={T * hw} C={c}", timeit(lambda: ops.layernorm(x, g, b)), bytes_=T * hw * c * 6.0)


if __name__ == "__main__":
    main()
