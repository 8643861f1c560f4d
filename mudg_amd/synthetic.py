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


def street_sweeps(frames=6, beams=32, azimuths=625, seed=0, n_objects=3, n_static=1, n_other=1, front_hw=(320, 480), side_hw=(222, 360)):
    """A seeded synthetic scenario in the layout of the reference's scenario.pt for mudg_amd.cloud (tests, tools/cloud_bench.py):
    returns (scenario, load_lidar, load_image).  World: x forward, y left, z up, the ground at z = 0 and walls at y = +-12.  A
    spinning LiDAR (beams x azimuths rays, 2 m above the ego vehicle, which drives 0.8 m per frame with a slight yaw) is cast
    against the ground, the walls and the boxes; only rays that hit within 75 m are returns, so the frames differ in length.
    n_objects Vehicle boxes drive ahead (object 1 is not tracked in frame 1), n_static more stand still and n_other more are Signs.
    camera_FRONT looks ahead, the smaller camera_SIDE_LEFT 60 degrees to the left; their images are procedural and avoid 0."""
    import numpy as np
    rng = np.random.default_rng(seed)
    total = n_objects + n_static + n_other
    scale = np.array([4.5, 2.0, 1.6])
    start = np.stack([rng.uniform(8, 40, total), rng.uniform(-8, 8, total), np.full(total, scale[2] / 2)], axis=1)
    speed = np.where(np.arange(total) < n_objects, rng.uniform(0.4, 1.5, total), 0.0)
    yaw0 = rng.uniform(-0.3, 0.3, total)

    def rot_z(a):
        return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])

    def rigid(r, t):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = r, t
        return m

    obj_tf = np.stack([np.stack([rigid(rot_z(yaw0[k] + (0.01 * f if speed[k] else 0.0)), start[k] + [speed[k] * f, 0, 0]) for f in range(frames)])
                       for k in range(total)]) if total else np.zeros((0, frames, 4, 4))
    objects = {}
    for k in range(total):
        shown = [f for f in range(frames) if not (k == 1 and f == 1 and frames > 1)]
        runs = [[shown[0]]] if shown else []
        for f in shown[1:]:
            runs[-1].append(f) if f == runs[-1][-1] + 1 else runs.append([f])
        objects[f"obj_{k}"] = {"id": k, "class_name": "Sign" if k >= n_objects + n_static else "Vehicle",
                               "segments": [{"start_frame": r[0], "n_frames": len(r), "data": {"transform": obj_tf[k, r], "scale": np.tile(scale, (len(r), 1))}}
                                            for r in runs]}
    ego = [rigid(rot_z(0.01 * f), [0.8 * f, 0.1 * f, 0.0]) for f in range(frames)]
    l2w = np.stack([e @ rigid(np.eye(3), [0.0, 0.0, 2.0]) for e in ego])
    cv = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])                 # the camera's x right, y down, z ahead in the ego frame
    mounts = {"camera_FRONT": (rigid(cv, [1.5, 0.0, 1.6]), front_hw), "camera_SIDE_LEFT": (rigid(rot_z(np.pi / 3) @ cv, [1.2, 0.5, 1.6]), side_hw)}
    observers = {"lidar_TOP": {"n_frames": frames, "data": {"l2w": l2w}}}
    for name, (mount, (h, w)) in mounts.items():
        k = np.array([[0.6 * w, 0.0, w / 2.0], [0.0, 0.6 * w, h / 2.0], [0.0, 0.0, 1.0]])
        observers[name] = {"n_frames": frames, "data": {"c2w": np.stack([e @ mount for e in ego]), "intr": np.tile(k, (frames, 1, 1)),
                                                         "hw": np.tile(np.array([h, w]), (frames, 1))}}
    scenario = {"observers": observers, "objects": objects}

    elev = np.linspace(np.radians(-17.0), np.radians(2.5), beams)
    azim = np.linspace(-np.pi, np.pi, azimuths, endpoint=False)
    el, az = (a.reshape(-1) for a in np.meshgrid(elev, azim, indexing="ij"))
    dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)

    def load_lidar(frame):
        g = np.random.default_rng([seed, 1, frame])
        o = g.normal(0.0, 0.01, dirs.shape)
        ow = o @ l2w[frame, :3, :3].T + l2w[frame, :3, 3]
        dw = dirs @ l2w[frame, :3, :3].T
        with np.errstate(all="ignore"):
            t = np.where(dw[:, 2] < 0, -ow[:, 2] / dw[:, 2], np.inf)
            for wall in (-12.0, 12.0):
                tw = (wall - ow[:, 1]) / dw[:, 1]
                t = np.minimum(t, np.where(tw > 0, tw, np.inf))
            for k in range(total):
                inv = np.linalg.inv(obj_tf[k, frame])
                ol, dl = ow @ inv[:3, :3].T + inv[:3, 3], dw @ inv[:3, :3].T
                t0, t1 = (-scale / 2 - ol) / dl, (scale / 2 - ol) / dl
                near, far = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
                t = np.minimum(t, np.where((near < far) & (near > 0), near + 0.02, np.inf))      # 2 cm under the surface
        hit = t < 75.0
        return o[hit].astype(np.float32), dirs[hit].astype(np.float32), (t[hit] + g.normal(0.0, 0.01, int(hit.sum()))).astype(np.float32)

    def load_image(camera, frame):
        h, w = mounts[camera][1]
        y, x = np.mgrid[0:h, 0:w]
        c = len(camera)
        return np.stack([1 + (x * 7 + y * 13 + frame * 17 + c) % 255, 1 + (x * 3 + y * 5 + frame * 11 + 2 * c) % 255, 1 + (x + y * 2 + frame * 29 + 3 * c) % 255],
                        axis=2).astype(np.uint8)

    return scenario, load_lidar, load_image
