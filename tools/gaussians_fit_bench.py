#!/usr/bin/env python3
"""Fitting Gaussians to images (mudg_amd/gaussians.py, csrc/gaussians_bwd.hip) on ONE MI355X: what an iteration costs and
what a fit does on the synthetic street.  Measured, not asserted.

`python tools/gaussians_fit_bench.py [--points 2] [--scale 0.1] [--runs 3] [--iters 300] [--no-ddim] [--out profiles/gaussians/fit_bench.txt]`

Cost: tools/gaussians_bench.py's scene (street_scene's background, `--points` million isotropic Gaussians of `--scale` metres, ONE
576 x 1024 view at the street's first camera), seeded at opacity 0.9.  Median [min .. max] of `--runs` runs between device events after a
warm-up of: project, keys and sort (with the .item() that reads E and mudg_gauss_ranges); the training blend; the blend's backward; the
projection's backward; the Adam launches (one per distinct learning rate: five); a whole iteration of gaussians.fit (with the set-up of the
optimiser's tables, which a longer fit pays once); beside them the inference gaussians.render and one DDIM step of the flagship workload in
the same process.  Also the bytes of the partial buffer (40 per entry).

Fit: the textured street of tests/gaussians_quality.py's construction (30000 points on a ground plane and two walls, recoloured by a
smooth texture; the target is the same texture ray-cast per pixel) at 72 x 128.  Every point starts grey (128) at 0.2 m and opacity 0.9;
`--iters` iterations against three training poses (the street's camera and 2 m to either side); one pose is held out (1 m to the left).
PSNR / SSIM (mudg_amd.metrics) of the inference render of the exported Gaussians against the target, before and after, per pose."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from mudg_amd import gaussians, metrics, ops, render
from mudg_amd.synthetic import street_scene
from mudg_amd.train import kernels as K
from splat_bench import ddim_step_ms, event_ms, spread

HW = (576, 1024)
FIT_HW = (72, 128)


def fmt(s, unit="ms"):
    return f"{s['median']:.3f} {unit} [{s['min']:.3f} .. {s['max']:.3f}]"


def texture(p):
    """(n, 3) positions on the street's surfaces -> (n, 3) uint8: bands along the street, across it and up the walls."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    c = np.stack([128 + 100 * np.sin(0.8 * z), 128 + 100 * np.sin(0.9 * x + 0.7 * y), 128 + 100 * np.cos(0.35 * z + 0.5 * x)], axis=1)
    return np.clip(np.rint(c), 1, 255).astype(np.uint8)


def own_image(c2w, cam, hw):
    """The texture seen from a camera: per pixel the nearest of the ground (y = 1.6) and the walls (x = +-12) inside the street's extent."""
    H, W = hw
    fx, fy, cx, cy = (float(v) for v in cam)
    j, i = np.mgrid[0:H, 0:W]
    d = np.stack([(i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, np.ones((H, W))], axis=-1).reshape(-1, 3) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    best = np.full(len(d), np.inf)
    with np.errstate(all="ignore"):
        for axis, value in ((1, 1.6), (0, -12.0), (0, 12.0)):
            t = (value - o[axis]) / d[:, axis]
            p = o + t[:, None] * d
            ok = (t > 0) & (p[:, 2] > -5) & (p[:, 2] < 150) & (p[:, 1] <= 1.6 + 1e-9) & (p[:, 1] > -9) & (np.abs(p[:, 0]) <= 25)
            if axis == 1:
                ok &= np.abs(p[:, 0]) <= 12
            best = np.where(ok & (t < best), t, best)
    hit = np.isfinite(best)
    img = np.zeros((len(d), 3), np.uint8)
    img[hit] = texture(o + best[hit, None] * d[hit])
    return img.reshape(H, W, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=float, default=2.0, help="Gaussians in millions (the cost part)")
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--no-ddim", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussians", "fit_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gaussians_fit_bench: no GPU (a CPU run measures nothing)")
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

    # ---------------------------------------------------------------------------------------- what an iteration costs
    n = int(args.points * 1e6)
    say(f"gaussians_fit_bench on {torch.cuda.get_device_name(0)}: one {HW[0]} x {HW[1]} view of the synthetic street, {n} isotropic Gaussians "
        f"of {args.scale} m, opacity 0.9; median [min .. max] of {args.runs} runs")
    scene = street_scene(n_background=n, frames=1, seed=11, n_objects=1, object_points=100)
    cloud = render.PointCloud.from_arrays(scene["bg_xyz"], scene["bg_rgb"], dev)
    cam = render.scaled_intrinsics(scene["intr"], scene["hw_native"], HW).astype(np.float32)
    mats = torch.from_numpy(gaussians.scene_matrices(None, np.linalg.inv(scene["c2w"][:1]), 0)).to(dev)
    model = gaussians.GaussianModel.from_cloud(cloud, args.scale, 0.9)
    tx, ty = ops.gauss_tiles(*HW)
    with torch.no_grad():
        cov, opacity, colour = model.covariance().contiguous(), model.opacity().contiguous(), model.colour.detach()
    pts = cloud.points
    box = {}

    def binning():
        uv, conic, depth, rect, count = ops.gauss_project(pts, cov, opacity, mats, cam, HW)
        ends = torch.cumsum(count.reshape(-1), 0, dtype=torch.int64)
        offsets = (ends - count.reshape(-1)).reshape(count.shape)
        keys, values = ops.gauss_keys(depth, rect, count, offsets, int(ends[-1].item()), HW)
        keys, order = torch.sort(keys, stable=True)
        box.update(uv=uv, conic=conic, depth=depth, count=count, offsets=offsets, order=order, values=values[order],
                   ranges=ops.gauss_ranges(keys, tx * ty))

    t_bin = timed(binning)
    entries = box["values"].numel()
    say(f" E = {entries} entries, {entries / (tx * ty):.1f} per tile of {tx * ty}; the partial buffer is {entries * 40} bytes ({entries * 40 / 2 ** 20:.1f} MiB)")
    forward = lambda: ops.gauss_blend_train(colour, box["uv"], box["conic"], box["depth"], box["values"], box["ranges"], HW)
    rgb, dimg, alpha, state = forward()
    up = (torch.randn_like(rgb) / rgb.numel(), torch.zeros_like(dimg), torch.zeros_like(alpha))
    backward = lambda: ops.gauss_blend_bwd(colour, box["uv"], box["conic"], box["depth"], box["values"], box["order"], box["ranges"], HW, state, *up)
    partial = backward()
    gather = lambda: ops.gauss_project_bwd(pts, cov, mats, cam, HW, box["count"], box["offsets"], partial)
    t_fwd, t_bwd, t_gather = timed(forward), timed(backward), timed(gather)
    params = list(model.parameters().values())
    tables = [K.chunk_table([(p.detach(), torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p))]) for p in params]

    def adam():
        for (table, chunks), rate in zip(tables, gaussians.LEARNING_RATES.values()):
            K.adamw_multi_(table, chunks, lr=0.0 * rate, betas=gaussians.ADAM_BETAS, eps=gaussians.ADAM_EPS, weight_decay=0.0, step=1)

    t_adam = timed(adam)
    target = torch.rand((1, 3) + HW, device=dev)
    t_iter = timed(lambda: gaussians.fit(model, target, mats, cam, HW, iters=1, lr={k: 0.0 for k in gaussians.PARAMETERS}))
    g = model.gaussians()
    t_render = timed(lambda: gaussians.render(g, mats, cam, HW))
    say(f" project, keys, sort and ranges {fmt(t_bin)}; training blend {fmt(t_fwd)}; blend backward {fmt(t_bwd)}, "
        f"{entries / (t_bwd['median'] * 1e-3) / 1e9:.3f} G entries/s; projection backward {fmt(t_gather)}; Adam, five launches {fmt(t_adam)}; "
        f"one whole fit iteration {fmt(t_iter)}; the inference render of the same Gaussians {fmt(t_render)}")
    del model, g, cloud, pts, cov, opacity, colour, box, rgb, dimg, alpha, state, up, partial, tables, params, target
    torch.cuda.empty_cache()
    if not args.no_ddim:
        say(f" one DDIM step of the flagship workload in this process: {fmt(ddim_step_ms(args.runs, dev))}")

    # ---------------------------------------------------------------------------------------- what a fit does on the textured street
    s = street_scene(n_background=30000, frames=1, seed=5, n_objects=1, object_points=10)
    xyz = s["bg_xyz"]
    cam = render.scaled_intrinsics(s["intr"], s["hw_native"], FIT_HW).astype(np.float32)
    left, right = render.virtual_poses(s["c2w"][0], 2.0, with_ori_pose=False)[:2]
    held = render.virtual_poses(s["c2w"][0], 1.0, with_ori_pose=False)[0]
    poses = np.stack([s["c2w"][0], left, right, held])
    names = ["original", "2 m to one side", "2 m to the other", "1 m to one side (held out)"]
    truth = torch.from_numpy(np.stack([own_image(p, cam, FIT_HW) for p in poses])).to(dev)
    mats = torch.from_numpy(gaussians.scene_matrices(None, np.linalg.inv(poses), 0)).to(dev)
    grey = np.full((len(xyz), 3), 128, np.uint8)
    model = gaussians.GaussianModel.from_cloud(render.PointCloud.from_arrays(xyz, grey, dev), 0.2, 0.9)

    def score(tag):
        out = gaussians.render(model.gaussians(), mats, cam, FIT_HW)
        frames = torch.floor(out["rgb"] * 255.0 + 0.5).clamp_(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        sc = metrics.psnr_ssim(frames, truth)
        for k, name in enumerate(names):
            say(f"  {tag}, {name}: PSNR {float(sc['psnr'][k]):.2f} dB, SSIM {float(sc['ssim'][k]):.4f}")

    say(f" fit on the textured street: {len(xyz)} grey Gaussians of 0.2 m at {FIT_HW[0]} x {FIT_HW[1]}, three training poses, {args.iters} iterations")
    score("before")
    targets = truth[:3].permute(0, 3, 1, 2).to(torch.float32).div_(255.0).contiguous()
    start = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start[0].record()
    losses = gaussians.fit(model, targets, mats[:3].contiguous(), cam, FIT_HW, iters=args.iters)
    start[1].record()
    torch.cuda.synchronize()
    say(f"  loss {losses[0]:.4f} -> {losses[-1]:.4f} in {start[0].elapsed_time(start[1]) / max(args.iters, 1):.2f} ms an iteration")
    score("after")


if __name__ == "__main__":
    main()
