#!/usr/bin/env python3
"""The pose gradient of the Gaussian renderer (csrc/gaussians_pose.hip, csrc/gaussians_sh.hip) on ONE MI355X: what the two
entry points cost beside mudg_gauss_project_bwd, which reads the same partial rows, and beside a device copy of the bytes each must move,
and what `poses=` adds to a fit iteration.  Measured, not asserted.

`python tools/gaussians_pose_bench.py [--points 2] [--scale 0.1] [--runs 3] [--no-ddim] [--out profiles/gaussians/pose_bench.txt]`

Scene: tools/gaussians_fit_bench.py's (street_scene's background, `--points` million isotropic Gaussians of `--scale` metres, ONE
576 x 1024 view at the street's first camera).  With nmat = 1, and with nmat = 32 where the cloud is cut into 32 runs of consecutive
Gaussians that go through 32 copies of the camera's matrix (Gaussians.from_scene lays objects out like that: a chunk of 256 holds one or
two ids), median [min .. max] of `--runs` runs between device events after a warm-up of: mudg_gauss_project_bwd; mudg_gauss_pose_bwd on
the same partials; the degree-3 mudg_gauss_sh_pose_bwd; a device copy of the bytes each must move at least (the packed points, the
covariances, count, offsets, ids and the 40-byte partial rows in; for the pose entries the stage buffer cleared, written and read; for
project_bwd its four gradients out).  Then one whole iteration of gaussians.fit without and with poses, and one DDIM step of the flagship
workload in the same process."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussians", "pose_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gaussians_pose_bench: no GPU (a CPU run measures nothing)")
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
    one = torch.from_numpy(gaussians.scene_matrices(None, np.linalg.inv(scene["c2w"][:1]), 0)).to(dev)
    model = gaussians.GaussianModel.from_cloud(cloud, args.scale, 0.9)
    pts = gaussians._pack_xyz(model.xyz)
    colour = model.colour.detach().contiguous()
    with torch.no_grad():
        cov = model.covariance().contiguous()
        b = gaussians._bin("gaussians_pose_bench", pts, cov, model.opacity().contiguous(), one, cam, HW, None, gaussians.ZNEAR, gaussians.ZFAR,
                           gaussians.MAX_ENTRIES)
    drawn = int((b.count > 0).sum())
    chunks = (n + ops.GAUSS_POSE_CHUNK - 1) // ops.GAUSS_POSE_CHUNK
    say(f"gaussians_pose_bench on {torch.cuda.get_device_name(0)}: {n} isotropic Gaussians of {args.scale} m, one {HW[0]} x {HW[1]} view, {drawn} "
        f"drawn, {b.entries} entries (a partial buffer of {b.entries * 40 / 2 ** 20:.0f} MiB), {chunks} chunks of 256; median [min .. max] of "
        f"{args.runs} runs")
    gen = torch.Generator(device=dev).manual_seed(3)
    up = (torch.rand((1, 3) + HW, device=dev, generator=gen), torch.zeros((1,) + HW, device=dev), torch.zeros((1,) + HW, device=dev))
    _, _, _, state = ops.gauss_blend_train(colour, b.uv, b.conic, b.depth, b.values, b.ranges, HW)
    partial = ops.gauss_blend_bwd(colour, b.uv, b.conic, b.depth, b.values, b.order, b.ranges, HW, state, *up)
    del state
    sh = (torch.rand((n, ops.gauss_sh_rows(3), 3), device=dev, generator=gen) - 0.5) * 40
    rate = lambda nbytes, t: nbytes / (t["median"] * 1e-3) / 1e12
    gathered = b.entries * 40
    for nmat in (1, 32):
        mats = one.repeat(1, nmat, 1).contiguous()
        ids = None if nmat == 1 else (torch.arange(n, device=dev) * nmat // n).to(torch.int32)
        per_point = 16 + 24 + 4 + 8 + (0 if ids is None else 4)
        stage = nmat * chunks * 48                                                              # cleared; read in full by the finishing kernel
        t_ref = timed(lambda: ops.gauss_project_bwd(pts, cov, mats, cam, HW, b.count, b.offsets, partial, ids=ids))
        t_pose = timed(lambda: ops.gauss_pose_bwd(pts, cov, mats, cam, HW, b.count, b.offsets, partial, ids=ids))
        t_dir = timed(lambda: ops.gauss_sh_pose_bwd(pts, mats, b.count, b.offsets, partial, colour, sh, ids=ids))
        ref_bytes = n * (per_point + 12 + 24 + 4 + 12) + gathered
        pose_bytes = n * per_point + gathered + 2 * stage + chunks * 48
        dir_bytes = n * (16 + 4 + 8 + (0 if ids is None else 4) + 12 + 180) + gathered + 2 * stage + chunks * 48
        c_ref, c_pose, c_dir = copy_of(ref_bytes), copy_of(pose_bytes), copy_of(dir_bytes)
        say(f" nmat = {nmat}: a stage buffer of {stage / 2 ** 20:.1f} MiB.  mudg_gauss_project_bwd {fmt(t_ref)} for {ref_bytes / 2 ** 20:.0f} MiB "
            f"({rate(ref_bytes, t_ref):.2f} TB/s; a copy of as many bytes {fmt(c_ref)}).  mudg_gauss_pose_bwd (clear, chunk sums, finish) "
            f"{fmt(t_pose)} for {pose_bytes / 2 ** 20:.0f} MiB ({rate(pose_bytes, t_pose):.2f} TB/s; a copy {fmt(c_pose)}): "
            f"{t_pose['median'] / t_ref['median']:.2f} of project_bwd, {t_pose['median'] / c_pose['median']:.2f} of the copy.  "
            f"mudg_gauss_sh_pose_bwd at degree 3 {fmt(t_dir)} for {dir_bytes / 2 ** 20:.0f} MiB ({rate(dir_bytes, t_dir):.2f} TB/s; a copy "
            f"{fmt(c_dir)}): {t_dir['median'] / t_ref['median']:.2f} of project_bwd, {t_dir['median'] / c_dir['median']:.2f} of the copy")
    del b, pts, colour, partial, sh, cov
    torch.cuda.empty_cache()
    target = torch.rand((1, 3) + HW, device=dev, generator=gen)
    still = {k: 0.0 for k in gaussians.PARAMETERS + ("sh", "pose")}
    t_plain = timed(lambda: gaussians.fit(model, target, one, cam, HW, iters=1, lr=still))
    poses = gaussians.CameraPoses(1, device=dev)
    t_poses = timed(lambda: gaussians.fit(model, target, one, cam, HW, iters=1, lr=still, poses=poses))
    say(f" one whole fit iteration: without poses {fmt(t_plain)}; with poses {fmt(t_poses)}")
    del model, cloud, target
    torch.cuda.empty_cache()
    if not args.no_ddim:
        say(f" one DDIM step of the flagship workload in this process: {fmt(ddim_step_ms(args.runs, dev))}")


if __name__ == "__main__":
    main()
