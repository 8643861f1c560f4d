"""Synthetic weights and inputs for benchmarks and smoke runs (no checkpoints or datasets are reachable offline).

Every tensor is drawn from a seeded generator ON the target device: matrices/filters N(0, 0.02^2) — including the
ones the reference zero-initialises, otherwise the UNet output is identically zero — norm scales 1 + 0.02 N,
biases / norm shifts 0.02 N.
"""
import torch


def materialize(module, device, seed=123):
    """Instantiate a module built under torch.device('meta') on `device` with synthetic parameters."""
    module.to_empty(device=device)
    fill_synthetic(module, seed)
    return module


@torch.no_grad()
def fill_synthetic(module, seed=123):
    gens = {}
    for i, (name, p) in enumerate(sorted(module.named_parameters(), key=lambda kv: kv[0])):
        g = gens.setdefault(p.device, torch.Generator(device=p.device))
        g.manual_seed(seed * 1000003 + i)
        noise = torch.empty(p.shape, dtype=torch.float32, device=p.device).normal_(0.0, 0.02, generator=g)
        if p.dim() <= 1 and name.endswith("weight"):
            noise += 1.0
        p.copy_(noise.to(p.dtype))
    return module


def rebuild_buffers(model, fresh):
    """Buffers (schedules) are deterministic functions of the config: copy them from a CPU-built twin."""
    src = dict(fresh.named_buffers())
    for name, buf in model.named_buffers():
        buf.copy_(src[name].to(buf.device))


def street_scene(n_background=2_000_000, frames=4, seed=0, n_objects=4, object_points=20_000):
    """A seeded synthetic street for the point-splat renderer (tests, tools/splat_bench.py): host arrays in the layout of the
    reference's scene files.  World = the first camera's OpenCV frame (x right, y down, z forward).  Background: a ground plane 1.6 m
    under the camera and two walls 12 m to either side, 150 m long; objects: box surfaces driving ahead, one transform per (object,
    frame); the camera moves 0.8 m per frame with a slight yaw.  Object colours avoid 0 (the merge mask is all(rgb > 0))."""
    import numpy as np
    rng = np.random.default_rng(seed)
    n_ground = n_background // 2
    n_wall = n_background - n_ground
    ground = np.stack([rng.uniform(-25, 25, n_ground), 1.6 + rng.normal(0, 0.02, n_ground), rng.uniform(-5, 150, n_ground)], axis=1)
    side = rng.choice([-1.0, 1.0], n_wall)
    wall = np.stack([side * 12 + rng.normal(0, 0.05, n_wall), rng.uniform(-9, 1.6, n_wall), rng.uniform(-5, 150, n_wall)], axis=1)
    bg_xyz = np.concatenate([ground, wall]).astype(np.float32)
    bg_rgb = rng.integers(0, 256, (n_background, 3), dtype=np.uint8)
    objects, transforms = [], []
    half = np.array([1.0, 0.8, 2.25])
    for i in range(n_objects):
        p = rng.uniform(-1, 1, (object_points, 3))
        axis = rng.integers(0, 3, object_points)
        p[np.arange(object_points), axis] = np.sign(p[np.arange(object_points), axis])          # onto a face of the box
        objects.append(((p * half).astype(np.float32), rng.integers(1, 256, (object_points, 3), dtype=np.uint8)))
        x0, z0, speed, yaw = rng.uniform(-8, 8), rng.uniform(8, 60), rng.uniform(-1.5, 1.5), rng.uniform(-0.3, 0.3)
        per_frame = []
        for f in range(frames):
            m = np.eye(4)
            a = yaw + 0.02 * f
            m[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
            m[:3, 3] = [x0, 1.6 - half[1], z0 + speed * f]
            per_frame.append(m)
        transforms.append(np.stack(per_frame))
    visibility = np.ones((n_objects, frames), dtype=np.int64)
    if n_objects > 1 and frames > 1:
        visibility[1, 1] = 0
    c2w = []
    for f in range(frames):
        m = np.eye(4)
        a = 0.01 * f
        m[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        m[:3, 3] = [0.1 * f, 0.0, 0.8 * f]
        c2w.append(m)
    intr = np.array([[2000.0, 0, 960.0], [0, 2000.0, 640.0], [0, 0, 1]])
    return {"bg_xyz": bg_xyz, "bg_rgb": bg_rgb, "objects": objects, "transform_obj": np.stack(transforms), "visibility": visibility,
            "intr": intr, "c2w": np.stack(c2w), "hw_native": (1280, 1920)}
