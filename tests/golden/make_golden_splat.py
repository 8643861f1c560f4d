#!/usr/bin/env python3
"""Capture the host-side fixture of the sparse-condition renderer from the REFERENCE implementation: the parts of
data_process/tools/generate_sparse.py that run without OpenGL — generate_virtual_pose (:263-279), process_obj_info (:226-235) and
merge_all_obj (:238-260) — on small seeded inputs.  Its renderer itself (pyrender point sprites in an offscreen GL context) cannot run
here, so no image of it is captured; the raster rule is a definition of this project.

Run in the build container only:   python tests/golden/make_golden_splat.py
The reference is found the way make_golden_validate.py finds it (make_golden.py is loaded for that; none of its goldens is
rewritten); pyrender and plyfile are replaced by empty stand-in modules before the import.  Only data is stored
(tests/golden/splat_host.pt, a few KB).

  3 objects of 50 points (float64 coordinates, float colours in [0, 1]), 4 frames, a seeded rigid transform per (object, frame);
  object 1 is invisible in frame 1, no object is visible in frame 3 (merge_all_obj then returns its one-point sentinel);
  4 seeded camera poses, generate_virtual_pose with and without the original pose, and with a shift whose round(., 4) matters."""
import contextlib
import importlib.util
import io
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mg = _load("make_golden")           # the reference on sys.path
import numpy as np                  # noqa: E402
import torch                        # noqa: E402

sys.modules["pyrender"] = types.ModuleType("pyrender")
ply = types.ModuleType("plyfile")
ply.PlyData = ply.PlyElement = None
sys.modules["plyfile"] = ply
from data_process.tools import generate_sparse as ref      # noqa: E402  (the reference's)

SEED = 20250
OBJECTS, POINTS, FRAMES = 3, 50, 4


def rigid(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    m = np.eye(4)
    m[:3, :3] = q
    m[:3, 3] = rng.uniform(-20, 20, 3)
    return m


def main():
    rng = np.random.default_rng(SEED)
    visibility = np.ones((OBJECTS, FRAMES), dtype=np.int64)
    visibility[1, 1] = 0
    visibility[:, 3] = 0
    obj_info = []
    for i in range(OBJECTS):
        obj_info.append({"id": i, "visibility": visibility[i],
                         "transform_obj": np.stack([rigid(rng) for _ in range(FRAMES)]),
                         "point_cloud": {"points": rng.uniform(-2, 2, (POINTS, 3)), "colors": rng.uniform(0, 1, (POINTS, 3))}})
    obj_vis = ref.process_obj_info(obj_info)
    merged = []
    with contextlib.redirect_stdout(io.StringIO()):                   # merge_all_obj prints every object it takes
        for f in range(FRAMES):
            xyz, rgb = ref.merge_all_obj(obj_info, obj_vis, frame=f)
            merged.append({"xyz": torch.from_numpy(np.asarray(xyz)), "rgb": torch.from_numpy(np.asarray(rgb))})
    c2w = np.stack([rigid(rng) for _ in range(4)])
    poses = {"default": [], "with_ori": [], "shift": []}
    for c in c2w:
        poses["default"].append(torch.from_numpy(np.stack(ref.generate_virtual_pose(c.copy()))))
        poses["with_ori"].append(torch.from_numpy(np.stack(ref.generate_virtual_pose(c.copy(), with_ori_pose=True))))
        poses["shift"].append(torch.from_numpy(np.stack(ref.generate_virtual_pose(c.copy(), random_shift=1.23456789))))
    path = os.path.join(HERE, "splat_host.pt")
    torch.save({"seed": SEED,
                "points": torch.from_numpy(np.stack([o["point_cloud"]["points"] for o in obj_info])),
                "colors": torch.from_numpy(np.stack([o["point_cloud"]["colors"] for o in obj_info])),
                "transform_obj": torch.from_numpy(np.stack([o["transform_obj"] for o in obj_info])),
                "visibility": torch.from_numpy(visibility), "obj_vis": torch.from_numpy(np.asarray(obj_vis)),
                "merged": merged, "c2w": torch.from_numpy(c2w), "shift": 1.23456789,
                "poses": {k: torch.stack(v) for k, v in poses.items()}}, path)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
