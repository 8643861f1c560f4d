#!/usr/bin/env python3
"""Capture the fixtures of the LiDAR depth maps from the REFERENCE implementation: data_process/pipeline_depth.py's get_6frames_lidar
(:63-75, the six-sweep window) and load_lidar_data (:16-60, the per-frame returns with the moving objects' points removed).

Run in the build container only:   python tests/golden/make_golden_lidar.py
make_golden_cloud.py is loaded for the tiny seeded scenario, its decision margins, its temp-file layout and its stand-ins (open3d,
plyfile; the module's Image.open answers from a dict); none of its goldens is rewritten.  pipeline_depth.py also imports cv2 and
pyrender at its top and `tools.*` as a top-level package: cv2 and pyrender are replaced by empty stand-in modules and `tools` is an alias
of data_process.tools before it is executed.  Only data is stored:

  lidar_windows.json  for scenes of 1 .. 8 frames and every index, the frame of every array get_6frames_lidar concatenates: frame f's
                      list is one point whose coordinates are all f, so the result names the frames in order
  lidar_frames.pt     load_lidar_data's per-frame points (float64) and colours (uint8) on make_golden_cloud.py's scenario, with the
                      objects_info.pkl its save_object_from_pt writes — under that script's margins every decision of the definition
                      must agree"""
import contextlib
import importlib.util
import io
import json
import os
import pickle
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mgc = _load("make_golden_cloud")    # the reference on sys.path, process_lidar imported with its stand-ins
import numpy as np                  # noqa: E402
import torch                        # noqa: E402

for name in ("cv2", "pyrender"):
    sys.modules.setdefault(name, types.ModuleType(name))
import data_process.tools as ref_tools                         # noqa: E402
from data_process.tools import generate_sparse as _gs           # noqa: E402,F401  (pipeline_depth imports it through `tools`)
sys.modules["tools"] = ref_tools
sys.modules["tools.process_lidar"] = mgc.ref
sys.modules["tools.generate_sparse"] = _gs
spec = importlib.util.spec_from_file_location("ref_pipeline_depth", os.path.join(mgc.mg.REF, "data_process", "pipeline_depth.py"))
pd = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pd)


def windows():
    out = {}
    for n in range(1, 9):
        points = [np.full((1, 3), float(f)) for f in range(n)]
        colours = [np.full((1, 3), float(f)) for f in range(n)]
        rows = []
        for index in range(n):
            p, c = pd.get_6frames_lidar(index, points, colours)
            assert np.array_equal(p, c) and p.shape == (6, 3)
            rows.append([int(v) for v in p[:, 0]])
        out[str(n)] = rows
    return out


def frames():
    seed = 20260
    scenario, sweeps = mgc.draw(seed)
    while not mgc.margins_ok(scenario, sweeps):
        seed += 1
        scenario, sweeps = mgc.draw(seed)
    ref = mgc.ref
    images = {}
    ref.Image = types.SimpleNamespace(open=lambda path: images[path])
    ref.store_ply = lambda path, xyz, rgb: None
    ref.segment_obj_from_lidar.__defaults__ = (0, mgc.FRAMES - 1, 0.3)
    with tempfile.TemporaryDirectory() as path, contextlib.redirect_stdout(io.StringIO()):
        os.makedirs(os.path.join(path, "lidars", "lidar_TOP"))
        os.makedirs(os.path.join(path, "objects"))
        for f, (o, d, r) in enumerate(sweeps):
            np.savez(os.path.join(path, "lidars", "lidar_TOP", "{:08}.npz".format(f)), rays_o=o[None], rays_d=d[None], ranges=r[None])
            for name, (h, w, _) in mgc.SIZES.items():
                images[os.path.join(path, "images", name, "{:08}.jpg".format(f))] = mgc.pixel_image(name, h, w)
        pt_file = os.path.join(path, "scenario.pt")
        with open(pt_file, "wb") as fh:
            pickle.dump(scenario, fh)
        ref.save_object_from_pt(path, pt_file, 0, mgc.FRAMES - 1, voxel_size=-1)
        info_path = os.path.join(path, "objects_info.pkl")
        with open(info_path, "rb") as fh:
            obj_info = pickle.load(fh)
        points, colours = pd.load_lidar_data(path, info_path)
    assert [o["id"] for o in obj_info] == [10] and len(points) == len(colours) == mgc.FRAMES
    out = {"seed": seed, "object_ids": [o["id"] for o in obj_info], "points": [], "colours": []}
    for p, c in zip(points, colours):
        assert p.shape == c.shape and p.shape[1] == 3 and np.array_equal(c, c.astype(np.uint8))
        out["points"].append(torch.from_numpy(np.ascontiguousarray(p, dtype=np.float64)))
        out["colours"].append(torch.from_numpy(np.ascontiguousarray(c.astype(np.uint8))))
    return out


def main():
    path = os.path.join(HERE, "lidar_windows.json")
    with open(path, "w") as fh:
        json.dump(windows(), fh, indent=0, separators=(",", ":"))
        fh.write("\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    out = frames()
    path = os.path.join(HERE, "lidar_frames.pt")
    torch.save(out, path)
    print(f"seed {out['seed']}; per-frame points {[len(p) for p in out['points']]}; wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
