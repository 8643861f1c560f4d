#!/usr/bin/env python3
"""The scene-cloud builder (mudg_amd/cloud.py, csrc/cloud.hip) on ONE MI355X, on seeded synthetic scenes
(mudg_amd.synthetic.street_sweeps and street_scene).

`python tools/cloud_bench.py [--frames 198] [--distinct 18] [--beams 64] [--azimuths 2650] [--points 2,8,32] [--runs 3] [--out profiles/r12/cloud_bench.txt]`

Every time is taken between two device events after a warm-up (tools/splat_bench.py's event_ms), `--runs` times; median [min .. max].
  sweep      mudg_cloud_sweep over the whole scene, the sweeps already on the GPU, at frames_per_launch = 1, 16 and all: ms per sweep
             and per scene, and the bytes the rule needs (28 read, 20 written per return, 3 more where a camera sees it) per second
             beside the 6.29 TB/s a float4 copy reaches on this chip
  build      the whole build_scene_clouds call (host tables, uploads, compaction; the loaders answer from memory)
  thinning   voxel_downsample of a street_scene background of 2 / 8 / 32 M points at v = 0.1 and 0.3: the whole call, and its parts
             (keys kernel; torch's sort, flags and prefix sum; reduce + finish kernels)
  renderer   render_conditions, ms per frame (4 frames, 3 poses, 576 x 1024), on the cloud before and after thinning"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from mudg_amd import cloud, ops, render
from mudg_amd.synthetic import street_scene, street_sweeps
from splat_bench import event_ms, spread

COPY_TBS, HW_OUT = 6.29, (576, 1024)


def fmt(s, unit="ms"):
    return f"{s['median']:.3f} {unit} [{s['min']:.3f} .. {s['max']:.3f}]"


def bench_sweep(args, dev, say):
    scenario, load_lidar, load_image = street_sweeps(frames=args.frames, beams=args.beams, azimuths=args.azimuths, seed=11, n_objects=6, n_static=2,
                                                     front_hw=(1280, 1920), side_hw=(886, 1920))
    sweeps, images = {}, {}

    def lidar(f):                                     # the scene repeats its first --distinct sweeps and images (host time); the
        f %= args.distinct                            # poses, and so every table, are per frame
        if f not in sweeps:
            sweeps[f] = load_lidar(f)
        return sweeps[f]

    def image(c, f):
        f %= args.distinct
        if (c, f) not in images:
            images[c, f] = load_image(c, f)
        return images[c, f]
    frames = list(range(args.frames))
    candidates = cloud.moving_objects(scenario, frames)
    results = {}
    for step in (1, 16, args.frames):
        batches = [cloud._Batch(scenario, frames[s:s + step], list(range(s, min(s + step, args.frames))), cloud.CAMERAS, lidar, image, dev)
                   for s in range(0, args.frames, step)]
        run = lambda: [b.run(candidates) for b in batches]
        out = run()
        if step == 1:
            returns = sum(len(o[1]) for o in out)
            seen = sum(int((o[1] >= 0).sum()) for o in out)
            say(f"sweep: {args.frames} frames, {returns} returns ({returns / args.frames:.0f} per sweep), {seen} seen by a camera, "
                f"{len(candidates)} moving objects, 2 cameras (1280 x 1920, 886 x 1920); sweeps and images repeat after {args.distinct} frames")
            nbytes = returns * 48 + seen * 3
        ms = spread([event_ms(run) for _ in range(args.runs)])
        results[step] = ms
        say(f"  frames_per_launch = {step:3d}: {fmt(ms)} per scene, {ms['median'] / args.frames:.4f} ms per sweep, "
            f"{nbytes / (ms['median'] * 1e-3) / 1e12:.3f} TB/s of {COPY_TBS} TB/s (copy)")
        del batches, out
    whole = lambda: cloud.build_scene_clouds(scenario, lidar, image, device=dev)
    bg, objects, info = whole()
    say(f"build: build_scene_clouds (frames_per_launch = {cloud.FRAMES_PER_LAUNCH}): {fmt(spread([event_ms(whole) for _ in range(args.runs)]))}; "
        f"background {len(bg)} points, {len(info)} objects of {[len(o['point_cloud']['points']) for o in info]} points")


def thin_parts(pc, v):
    pts = pc.points
    t_keys = event_ms(lambda: ops.cloud_voxel_keys(pts, v))
    keys = ops.cloud_voxel_keys(pts, v)
    state = {}

    def plumbing():
        k, order = torch.sort(keys, stable=True)
        flags = torch.zeros_like(k)
        flags[1:] = k[1:] != k[:-1]
        state["order"], state["segments"] = order, torch.cumsum(flags, dim=0)
    t_sort = event_ms(plumbing)
    voxels = int(state["segments"][-1]) + 1
    t_reduce = event_ms(lambda: ops.cloud_voxel_finish(ops.cloud_voxel_reduce(pts, state["order"], state["segments"], v, voxels), v))
    return t_keys, t_sort, t_reduce


def bench_thinning(args, dev, say):
    for millions in args.points:
        n = int(millions * 1_000_000)
        scene = street_scene(n_background=n, frames=4, seed=11)
        bg = render.PointCloud.from_arrays(scene["bg_xyz"], scene["bg_rgb"], dev)
        objects = render.ObjectSet(scene["objects"], scene["transform_obj"], scene["visibility"], dev)
        frame = lambda pc: (lambda: render.render_conditions(pc, objects, scene["intr"], scene["c2w"], scene["hw_native"], HW_OUT))
        frame(bg)()
        before = spread([event_ms(frame(bg)) / 4 for _ in range(args.runs)])
        say(f"thinning: {millions} M points; renderer before: {fmt(before)} per frame")
        for v in (0.1, 0.3):
            thin = cloud.voxel_downsample(bg, v)
            whole = spread([event_ms(lambda: cloud.voxel_downsample(bg, v)) for _ in range(args.runs)])
            parts = [thin_parts(bg, v) for _ in range(args.runs)]
            k, s, r = (spread([p[i] for p in parts]) for i in range(3))
            frame(thin)()
            after = spread([event_ms(frame(thin)) / 4 for _ in range(args.runs)])
            say(f"  v = {v}: {len(thin)} voxels; voxel_downsample {fmt(whole)} (keys {k['median']:.3f}, sort + scan {s['median']:.3f}, reduce + finish {r['median']:.3f}); "
                f"renderer after: {fmt(after)} per frame")
        del bg, objects, scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=198)
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuths", type=int, default=2650)
    ap.add_argument("--distinct", type=int, default=18)
    ap.add_argument("--points", type=lambda s: [float(x) for x in s.split(",")], default=[2, 8, 32])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cloud_bench: no GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    say(f"cloud_bench on {torch.cuda.get_device_name(0)}: median [min .. max] of {args.runs} runs")
    bench_sweep(args, dev, say)
    bench_thinning(args, dev, say)


if __name__ == "__main__":
    main()
