#!/usr/bin/env python3
"""The sparse-condition renderer (mudg_amd/render.py, csrc/splat.hip) on ONE MI355X: a seeded synthetic street
(mudg_amd.synthetic.street_scene), 1280 x 1920 native rendered at 576 x 1024, three poses, 16 frames.

`python tools/splat_bench.py [--points 2,8,32] [--runs 3] [--no-ddim] [--no-cpu] [--out profiles/r8/splat_bench.json]`

Per cloud size (millions of background points), from `--runs` runs after a warm-up, each between two device events:
  points_ms            mudg_splat_points on the background, per frame (one launch = three poses), and the point stream's TB/s
                       (16 bytes per point, read once) beside the 6.3 TB/s a copy reaches on this chip
  object_points_ms     the same for the object layer (four boxes of 20 000 points, a matrix per object)
  resolve_compose_ms   mudg_splat_resolve of both layers + mudg_splat_compose, per frame
  frame_ms, window_ms  the whole render_conditions call over 16 frames, per frame and per window (host matrix algebra, the upload of
                       the matrices and every launch included)
  atomics              covered pixels (= atomics without the early reject) and issued atomics with it, per projected point, from the
                       kernel's own counters; and points_ms with the early reject switched off
The DDIM step of the flagship workload (bench.py's: MDM1024, CFG 7.5, 50-step schedule) is timed in the same process for scale, and
the CPU definition (tests/splat_reference.py, numpy) renders one frame of the smallest scene on the same box."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from mudg_amd import ops, render
from mudg_amd.synthetic import street_scene

HW_OUT, FRAMES, COPY_TBS = (576, 1024), 16, 6.3


def spread(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values)), "runs": [float(v) for v in values]}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_buckets(bg, objects, scene, poses, early_reject=True, stats=None):
    """One pass over the 16 frames with the launches of render_conditions, an event between the stages; ms per frame."""
    dev = bg.points.device
    T, P = poses.shape[:2]
    H, W = HW_OUT
    w2c = np.linalg.inv(poses)
    bg_mats = torch.from_numpy(np.ascontiguousarray(w2c[:, :, None, :3, :].reshape(T, P, 1, 12)).astype(np.float32)).to(dev)
    obj_mats = torch.from_numpy(np.stack([objects.matrices(w2c[t], t) for t in range(T)]).reshape(T, P, -1, 12).astype(np.float32)).to(dev)
    cam = render.scaled_intrinsics(scene["intr"], scene["hw_native"], HW_OUT).astype(np.float32)
    sparse = torch.empty((P, 3, T, H, W), dtype=torch.float32, device=dev)
    sdepth = torch.empty_like(sparse)
    keys_b, keys_o = ops.splat_keys(P, H, W, dev), ops.splat_keys(P, H, W, dev)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(T)]
    kw = dict(early_reject=early_reject, stats=stats)
    for t in range(T):
        ev[t][0].record()
        ops.splat_points(bg.points, bg_mats[t], keys_b, cam, render.BACKGROUND_POINT_SIZE, **kw)
        ev[t][1].record()
        ops.splat_points(objects.cloud.points, obj_mats[t], keys_o, cam, render.OBJECT_POINT_SIZE, ids=objects.ids, **kw)
        ev[t][2].record()
        ops.splat_compose(ops.splat_resolve(keys_b, bg.points), ops.splat_resolve(keys_o, objects.cloud.points), sparse, sdepth, t)
        ev[t][3].record()
    torch.cuda.synchronize()
    return [sum(ev[t][k].elapsed_time(ev[t][k + 1]) for t in range(T)) / T for k in range(3)]


def bench_size(millions, runs, dev):
    n = int(millions * 1_000_000)
    t0 = time.perf_counter()
    scene = street_scene(n_background=n, frames=FRAMES, seed=11)
    bg = render.PointCloud.from_arrays(scene["bg_xyz"], scene["bg_rgb"], dev)
    objects = render.ObjectSet(scene["objects"], scene["transform_obj"], scene["visibility"], dev)
    poses = np.stack([np.stack(render.virtual_poses(c, with_ori_pose=True)) for c in scene["c2w"]])
    print(f"[{millions} M] scene built and uploaded in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    whole = lambda: render.render_conditions(bg, objects, scene["intr"], scene["c2w"], scene["hw_native"], HW_OUT, poses=poses)
    whole()                                                        # warm-up: code objects, allocator
    kernel_buckets(bg, objects, scene, poses)
    buckets = [kernel_buckets(bg, objects, scene, poses) for _ in range(runs)]
    no_reject = [kernel_buckets(bg, objects, scene, poses, early_reject=False)[0] for _ in range(runs)]
    window = [event_ms(whole) for _ in range(runs)]
    counts = {}
    for tag, flag in (("with_early_reject", True), ("without_early_reject", False)):
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
        kernel_buckets(bg, objects, scene, poses, early_reject=flag, stats=stats)
        covered, issued = (int(v) for v in stats.cpu())
        projected = (n + len(objects.cloud)) * poses.shape[1] * FRAMES
        counts[tag] = {"covered_pixels": covered, "issued_atomics": issued, "atomics_per_projected_point": issued / projected,
                       "share_of_covered_pixels_that_reach_the_atomic": issued / max(covered, 1)}
    points = [b[0] for b in buckets]
    rec = {"background_points": n, "object_points": len(objects.cloud), "poses": int(poses.shape[1]), "frames": FRAMES, "hw_out": list(HW_OUT),
           "points_ms": spread(points), "object_points_ms": spread([b[1] for b in buckets]), "resolve_compose_ms": spread([b[2] for b in buckets]),
           "points_ms_without_early_reject": spread(no_reject),
           "point_stream_TBps": spread([n * 16 / (ms * 1e-3) / 1e12 for ms in points]), "copy_TBps_on_this_chip": COPY_TBS,
           "frame_ms": spread([w / FRAMES for w in window]), "window_ms": spread(window), "atomics": counts}
    return rec, scene


def ddim_step_ms(runs, dev, steps=5):
    from lvdm.models.samplers.ddim import DDIMSampler
    from mudg_amd import factory
    model = factory.build_synthetic_model("1024", dev, seed=123)
    inp = factory.synthetic_inputs(model, "1024", 1, dev, seed=123)
    sampler = DDIMSampler(model)
    sampler.make_schedule(50, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    kw = dict(unconditional_guidance_scale=7.5, unconditional_conditioning=inp["uc"], guidance_rescale=0.7, fs=inp["fs"],
              sparse_x=inp["sparse_x"], class_label=inp["class_label"], cfg_img=None, unconditional_conditioning_img_nonetext=None)
    model.model.diffusion_model.use_hip_graph = True

    def run(n, start):
        x = inp["x_T"]
        for i in range(n):
            index = (start - i) % 50
            ts = torch.full((1,), int(sampler.ddim_timesteps[index]), device=dev, dtype=torch.long)
            x, _ = sampler.p_sample_ddim(x, inp["cond"], ts, index=index, **kw)

    with torch.no_grad():
        run(3, 49)
        torch.cuda.synchronize()
        return spread([event_ms(lambda: run(steps, 46 - steps * k)) / steps for k in range(runs)])


def cpu_definition_s(scene):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import splat_reference as sr
    poses = np.stack([np.stack(render.virtual_poses(c, with_ori_pose=True)) for c in scene["c2w"][:1]])
    t0 = time.perf_counter()
    sr.render_conditions(scene["bg_xyz"], scene["bg_rgb"], scene["objects"], scene["transform_obj"], scene["visibility"], scene["intr"],
                         scene["c2w"][:1], scene["hw_native"], HW_OUT, poses)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="2,8,32")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-ddim", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r8", "splat_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("splat_bench needs the MI355X: there is nothing to time without it")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "sizes": {}}
    first = None
    for m in (float(v) for v in args.points.split(",")):
        rec, scene = bench_size(m, args.runs, dev)
        out["sizes"][f"{m:g}M"] = rec
        first = first or scene
        print(json.dumps({f"{m:g}M": {k: rec[k]["median"] for k in ("points_ms", "resolve_compose_ms", "frame_ms", "window_ms")}}), file=sys.stderr, flush=True)
        del scene
        torch.cuda.empty_cache()
    if not args.no_cpu:
        out["cpu_definition"] = {"background_points": len(first["bg_xyz"]), "frames": 1, "poses": 3, "seconds": cpu_definition_s(first)}
    if not args.no_ddim:
        out["ddim_step_ms"] = ddim_step_ms(args.runs, dev)
        if "8M" in out["sizes"]:
            out["window_8M_under_one_ddim_step"] = out["sizes"]["8M"]["window_ms"]["max"] < out["ddim_step_ms"]["min"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
