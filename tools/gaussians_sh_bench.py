#!/usr/bin/env python3
"""View-dependent colour of the Gaussian renderer (csrc/gaussians_sh.hip) on ONE MI355X: what the colour pass and its
backward cost beside a device copy of the bytes each must move, and what harmonics add to a fit iteration.  Measured, not asserted.

`python tools/gaussians_sh_bench.py [--points 2] [--scale 0.1] [--runs 3] [--no-ddim] [--out profiles/gaussians/sh_bench.txt]`

Scene: tools/gaussians_fit_bench.py's (street_scene's background, `--points` million isotropic Gaussians of `--scale` metres, ONE
576 x 1024 view at the street's first camera), seeded coefficients.  For L = 1, 2, 3, median [min .. max] of `--runs` runs between device
events after a warm-up of: mudg_gauss_sh_colour; mudg_gauss_sh_bwd on the partials of a real backward; a device copy of the bytes each
must move at least (colour pass: the packed points, count, colour, the coefficients in and the colours out; backward: the points, count,
offsets, colour and the coefficients in, the three gradients out; the partial rows the backward gathers are counted apart: 40 bytes a
row of which it uses 12).  Then one whole iteration of gaussians.fit with sh_degree 0 and 3, and one DDIM step of the flagship workload in
the same process."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from mudg_amd import gaussians, ops, render
from mudg_amd.synthetic import street_scene
from splat_bench import ddim_step_ms, event_ms, spread

HW = (576, 1024)


def fmt(s, unit="ms"):
    return f"{s['median']:.3f} {unit} [{s['min']:.3f} .. {s['max']:.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=float, default=2.0, help="Gaussians in millions")
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-ddim", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussians", "sh_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gaussians_sh_bench: no GPU (a CPU run measures nothing)")
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
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)
        return timed(lambda: dst.copy_(src))                                                    # nbytes / 2 read and nbytes / 2 written

    n = int(args.points * 1e6)
    scene = street_scene(n_background=n, frames=1, seed=11, n_objects=1, object_points=100)
    cloud = render.PointCloud.from_arrays(scene["bg_xyz"], scene["bg_rgb"], dev)
    cam = render.scaled_intrinsics(scene["intr"], scene["hw_native"], HW).astype(np.float32)
    mats = torch.from_numpy(gaussians.scene_matrices(None, np.linalg.inv(scene["c2w"][:1]), 0)).to(dev)
    model = gaussians.GaussianModel.from_cloud(cloud, args.scale, 0.9)
    pts = gaussians._pack_xyz(model.xyz)
    colour = model.colour.detach().contiguous()
    with torch.no_grad():
        b = gaussians._bin("gaussians_sh_bench", pts, model.covariance().contiguous(), model.opacity().contiguous(), mats, cam, HW, None,
                           gaussians.ZNEAR, gaussians.ZFAR, gaussians.MAX_ENTRIES)
    drawn = int((b.count > 0).sum())
    say(f"gaussians_sh_bench on {torch.cuda.get_device_name(0)}: {n} isotropic Gaussians of {args.scale} m, one {HW[0]} x {HW[1]} view, {drawn} "
        f"drawn, {b.entries} entries (a partial buffer of {b.entries * 40 / 2 ** 20:.0f} MiB); median [min .. max] of {args.runs} runs")
    gen = torch.Generator(device=dev).manual_seed(3)
    up = (torch.rand((1, 3) + HW, device=dev, generator=gen), torch.zeros((1,) + HW, device=dev), torch.zeros((1,) + HW, device=dev))
    for degree in (1, 2, 3):
        rows = ops.gauss_sh_rows(degree)
        sh = (torch.rand((n, rows, 3), device=dev, generator=gen) - 0.5) * 40
        colours = ops.gauss_sh_colour(pts, mats, b.count, colour, sh)
        _, _, _, state = ops.gauss_blend_train_views(colours, b.uv, b.conic, b.depth, b.values, b.ranges, HW)
        partial = ops.gauss_blend_bwd_views(colours, b.uv, b.conic, b.depth, b.values, b.order, b.ranges, HW, state, *up)
        t_fwd = timed(lambda: ops.gauss_sh_colour(pts, mats, b.count, colour, sh))
        t_bwd = timed(lambda: ops.gauss_sh_bwd(pts, mats, b.count, b.offsets, partial, colour, sh))
        fwd_bytes = n * (16 + 4 + 12 + rows * 12 + 12)
        bwd_bytes = n * (16 + 4 + 8 + 12 + rows * 12 + 12 + rows * 12 + 12)
        gathered = b.entries * 40
        c_fwd, c_bwd, c_all = copy_of(fwd_bytes), copy_of(bwd_bytes), copy_of(bwd_bytes + gathered)
        rate = lambda nbytes, t: nbytes / (t["median"] * 1e-3) / 1e12
        say(f" L = {degree}: colour pass {fmt(t_fwd)} for {fwd_bytes / 2 ** 20:.0f} MiB ({rate(fwd_bytes, t_fwd):.2f} TB/s; a device copy of as "
            f"many bytes {fmt(c_fwd)}, {rate(fwd_bytes, c_fwd):.2f} TB/s); backward {fmt(t_bwd)} for {bwd_bytes / 2 ** 20:.0f} MiB of its own "
            f"({rate(bwd_bytes, t_bwd):.2f} TB/s; a copy {fmt(c_bwd)}, {rate(bwd_bytes, c_bwd):.2f} TB/s) and the {gathered / 2 ** 20:.0f} MiB of "
            f"partial rows it walks ({rate(bwd_bytes + gathered, t_bwd):.2f} TB/s with them; a copy of both {fmt(c_all)}, "
            f"{rate(bwd_bytes + gathered, c_all):.2f} TB/s)")
        del sh, colours, state, partial
        torch.cuda.empty_cache()
    del b, pts, colour
    torch.cuda.empty_cache()
    target = torch.rand((1, 3) + HW, device=dev, generator=gen)
    still = {k: 0.0 for k in gaussians.PARAMETERS + ("sh",)}
    t_plain = timed(lambda: gaussians.fit(model, target, mats, cam, HW, iters=1, lr=still))
    lit = gaussians.GaussianModel.from_cloud(cloud, args.scale, 0.9).enable_sh(3)
    t_sh = timed(lambda: gaussians.fit(lit, target, mats, cam, HW, iters=1, lr=still, sh_degree=3))
    say(f" one whole fit iteration: sh_degree 0 {fmt(t_plain)}; sh_degree 3 {fmt(t_sh)}")
    del model, lit, cloud, target
    torch.cuda.empty_cache()
    if not args.no_ddim:
        say(f" one DDIM step of the flagship workload in this process: {fmt(ddim_step_ms(args.runs, dev))}")


if __name__ == "__main__":
    main()
