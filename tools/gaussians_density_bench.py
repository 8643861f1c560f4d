#!/usr/bin/env python3
"""Density control for the Gaussian fit (mudg_amd/gaussians.py, csrc/gaussians_density.hip) on ONE MI355X: what its three
kernels and a whole step cost beside a fit iteration.  Measured, not asserted.

`python tools/gaussians_density_bench.py [--points 2] [--scale 0.1] [--runs 3] [--no-ddim] [--out profiles/gaussians/density_bench.txt]`

tools/gaussians_fit_bench.py's scene (street_scene's background, `--points` million isotropic Gaussians of `--scale` metres, ONE
576 x 1024 view at the street's first camera), seeded at opacity 0.9.  Median [min .. max] of `--runs` runs between device events after a
warm-up of: mudg_gauss_density_accumulate on the partials of a real backward (it reads 8 of every 40 bytes of the buffer, whole cache
lines of it); mudg_gauss_density_plan; mudg_gauss_density_apply on that plan (15 tensors read and written once); a whole
densify_and_prune (with its torch expressions, the exclusive sum and its two host synchronisations); a device copy of the bytes apply
moves and of the partial buffer; one iteration of gaussians.fit without and inside the window of a DensityControl; one DDIM step of the
flagship workload in the same process.  The thresholds are chosen so that the plan holds all four actions.  The partial buffer of this
scene is smaller than the 256 MiB last-level cache, so a repeated accumulate finds it on the die; accumulate and apply are therefore
also timed with 512 MiB of other stores before every run."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussians", "density_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gaussians_density_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    flush = torch.empty((2 ** 27,), dtype=torch.float32, device=dev)                          # 512 MiB: twice the last-level cache

    def timed(fn, cold=False):
        fn()                                                                                    # warm-up
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.runs):
            if cold:                                                                            # a repeat finds nothing of its input on the die
                flush.fill_(0.0)
            runs.append(event_ms(fn))
        return spread(runs)

    n = int(args.points * 1e6)
    say(f"gaussians_density_bench on {torch.cuda.get_device_name(0)}: one {HW[0]} x {HW[1]} view of the synthetic street, {n} isotropic Gaussians "
        f"of {args.scale} m, opacity 0.9; median [min .. max] of {args.runs} runs")
    scene = street_scene(n_background=n, frames=1, seed=11, n_objects=1, object_points=100)
    cloud = render.PointCloud.from_arrays(scene["bg_xyz"], scene["bg_rgb"], dev)
    cam = render.scaled_intrinsics(scene["intr"], scene["hw_native"], HW).astype(np.float32)
    mats = torch.from_numpy(gaussians.scene_matrices(None, np.linalg.inv(scene["c2w"][:1]), 0)).to(dev)
    model = gaussians.GaussianModel.from_cloud(cloud, args.scale, 0.9)
    tx, ty = ops.gauss_tiles(*HW)
    with torch.no_grad():
        cov, opacity, colour = model.covariance().contiguous(), model.opacity().contiguous(), model.colour.detach()
        scale = torch.exp(model.log_scale.detach()).contiguous()
        rot = gaussians.rotation_from_quaternions(model.quat.detach()).reshape(n, 9).contiguous()
    pts = cloud.points
    uv, conic, depth, rect, count = ops.gauss_project(pts, cov, opacity, mats, cam, HW)
    ends = torch.cumsum(count.reshape(-1), 0, dtype=torch.int64)
    offsets = (ends - count.reshape(-1)).reshape(count.shape)
    keys, values = ops.gauss_keys(depth, rect, count, offsets, int(ends[-1].item()), HW)
    keys, order = torch.sort(keys, stable=True)
    values = values[order]
    ranges = ops.gauss_ranges(keys, tx * ty)
    rgb, dimg, alpha, state = ops.gauss_blend_train(colour, uv, conic, depth, values, ranges, HW)
    target = torch.rand((1, 3) + HW, device=dev)
    up = (torch.sign(rgb - target) / rgb.numel(), torch.zeros_like(dimg), torch.zeros_like(alpha))      # the mean absolute difference's gradient
    partial = ops.gauss_blend_bwd(colour, uv, conic, depth, values, order, ranges, HW, state, *up)
    entries = values.numel()
    del keys, values, order, ranges, rgb, dimg, alpha, state, up, uv, conic, depth, rect
    stats = gaussians.DensityStats(n, dev)
    t_acc = timed(lambda: ops.gauss_density_accumulate(partial, count, offsets, HW, stats.grad_sum, stats.seen))
    t_acc_cold = timed(lambda: ops.gauss_density_accumulate(partial, count, offsets, HW, stats.grad_sum, stats.seen), cold=True)
    stats.reset()
    ops.gauss_density_accumulate(partial, count, offsets, HW, stats.grad_sum, stats.seen)
    drawn = stats.seen > 0
    mean = (stats.grad_sum[drawn] / stats.seen[drawn]).sort()[0]
    threshold = float(mean[int(0.7 * (mean.numel() - 1))])                                    # three Gaussians in ten of those drawn grow
    with torch.no_grad():
        model.log_scale[::2] += 0.5                                                           # every other one is above split_scale
        model.opacity_logit[::10] = -9.0                                                      # one in ten is transparent
        scale = torch.exp(model.log_scale.detach()).contiguous()
        opacity = model.opacity().contiguous()
    kw = dict(grad_threshold=threshold, split_scale=1.2 * args.scale, min_opacity=0.005, max_scale=100.0)
    t_plan = timed(lambda: ops.gauss_density_plan(stats.grad_sum, stats.seen, opacity, scale, **kw))
    action, rows = ops.gauss_density_plan(stats.grad_sum, stats.seen, opacity, scale, **kw)
    ends = torch.cumsum(rows, 0, dtype=torch.int64)
    total = int(ends[-1].item())
    start = ends - rows
    kept, pruned, cloned, split = torch.bincount(action, minlength=4).tolist()
    control = gaussians.DensityControl(0, 1, 1, **kw)
    tensors = []
    for name in gaussians.PARAMETERS:
        p = getattr(model, name).detach()
        tensors += [p, torch.zeros_like(p), torch.zeros_like(p)]
    apply = lambda: ops.gauss_density_apply(action, start, total, scale, rot, tensors, split_offset=control.split_offset, log_shrink=control.log_shrink)
    t_apply, t_apply_cold = timed(apply), timed(apply, cold=True)
    moved = sum(t.numel() * 4 for t in tensors) + 3 * sum(ops.GAUSS_PARAMETER_WIDTHS) * 4 * total          # read once, written once
    src = torch.empty((moved // 8,), dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    t_copy = timed(lambda: dst.copy_(src))
    t_copy_partial = timed(lambda: torch.empty_like(partial).copy_(partial))
    say(f" E = {entries} entries, the partial buffer is {entries * 40} bytes ({entries * 40 / 2 ** 20:.1f} MiB); the plan: {kept} kept, {pruned} pruned, "
        f"{cloned} cloned, {split} split, {n} -> {total} Gaussians; apply reads and writes {moved} bytes ({moved / 2 ** 20:.1f} MiB)")
    say(f" accumulate, the buffer on the die from the run before (it is smaller than the 256 MiB last-level cache) {fmt(t_acc)}; after 512 MiB of other "
        f"stores {fmt(t_acc_cold)}, {entries * 40 / (t_acc_cold['median'] * 1e-3) / 1e9:.1f} GB/s of the partial buffer's lines; a device copy of that "
        f"buffer (read and write, repeated) {fmt(t_copy_partial)}; plan {fmt(t_plan)}; apply {fmt(t_apply)}, after 512 MiB of other stores "
        f"{fmt(t_apply_cold)}, {moved / (t_apply_cold['median'] * 1e-3) / 1e9:.1f} GB/s; a device copy of the same bytes {fmt(t_copy)}, "
        f"{moved / (t_copy['median'] * 1e-3) / 1e9:.1f} GB/s")
    del src, dst, tensors, partial
    torch.cuda.empty_cache()

    def whole():
        m = gaussians.GaussianModel(*[getattr(model, k).detach() for k in gaussians.PARAMETERS])
        st = gaussians.DensityStats(n, dev)
        st.grad_sum.copy_(stats.grad_sum)
        st.seen.copy_(stats.seen)
        return gaussians.densify_and_prune(m, st, {}, control)

    t_whole = timed(whole)
    zero = {k: 0.0 for k in gaussians.PARAMETERS}
    never = gaussians.DensityControl(0, 10, 10 ** 9, **kw)                                    # gathers in every iteration, never densifies
    t_iter = timed(lambda: gaussians.fit(model, target, mats, cam, HW, iters=1, lr=zero))
    t_iter_d = timed(lambda: gaussians.fit(model, target, mats, cam, HW, iters=1, lr=zero, density=never))
    say(f" a whole densify_and_prune (a model's clone and its statistics included) {fmt(t_whole)}; one fit iteration {fmt(t_iter)}; one fit iteration "
        f"that gathers statistics {fmt(t_iter_d)}")
    del model, cloud, pts, cov, opacity, colour, stats, target, flush
    torch.cuda.empty_cache()
    if not args.no_ddim:
        say(f" one DDIM step of the flagship workload in this process: {fmt(ddim_step_ms(args.runs, dev))}")


if __name__ == "__main__":
    main()
