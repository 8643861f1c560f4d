#!/usr/bin/env python3
"""Capture the host-side fixture of the scene-cloud builder from the REFERENCE implementation: data_process/tools/process_lidar.py's
trans_local2global (:27-33), get_color_from_camera (:45-82), segment_object_pcd (:121-138), is_object_motion (:265-280),
save_object_from_pt (:141-209) and save_background_from_pt (:212-262, voxel_size = -1) on a tiny seeded scenario.

Run in the build container only:   python tests/golden/make_golden_cloud.py
The reference is found the way make_golden_splat.py finds it.  open3d and plyfile are replaced by empty stand-in modules before the
import; the module's Image.open returns an array from an in-memory dict and its store_ply captures its arguments.  The sweeps are
written as temporary .npz files and the scenario as a temporary pickle, as the reference reads them.  One default is set:
segment_obj_from_lidar walks frames 0 .. 99 whatever the scene's length (its start_f / end_f defaults), which on a 4-frame scenario
is an IndexError; its defaults become (0, 3).  Only data is stored (tests/golden/cloud_host.pt).

  4 frames, 300 rays per frame, 2 cameras of different sizes whose images encode the pixel index (so a colour names its pixel), and
  4 objects: 0 moves, is not tracked in frame 1 and keeps more than 100 points; 1 stands still; 2 is a Sign; 3 moves and keeps fewer
  than 100 points.  The reference multiplies through BLAS, so its last bits are not the rule's: the scenario is drawn again until no
  point lies within 1e-6 (pixels; metres) of a decision boundary and the motion norms are 1e-6 away from 0.5, and that is asserted
  before saving.  Under that margin every decision of the definition must agree with the reference's."""
import contextlib
import importlib.util
import io
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


mg = _load("make_golden")           # the reference on sys.path
import numpy as np                  # noqa: E402
import torch                        # noqa: E402

sys.modules["open3d"] = types.ModuleType("open3d")
ply = types.ModuleType("plyfile")
ply.PlyData = ply.PlyElement = None
sys.modules["plyfile"] = ply
from data_process.tools import process_lidar as ref      # noqa: E402  (the reference's)

sys.path.append(os.path.join(HERE, ".."))
import cloud_reference as cr        # noqa: E402  (numpy only: the margins are measured with the definition)

FRAMES, RAYS, MARGIN = 4, 300, 1e-6
SIZES = {"camera_FRONT": (24, 32, 20.0), "camera_SIDE_LEFT": (16, 24, 14.0)}       # h, w, focal length
SCALE = np.array([4.0, 2.0, 1.6])


def pixel_image(camera, h, w):
    """Pixel (y, x) holds its own index: r | g << 8 = y * w + x, b = 1 + the camera's number."""
    idx = (np.arange(h)[:, None] * w + np.arange(w)[None, :])
    return np.stack([idx & 255, idx >> 8, np.full_like(idx, 1 + list(SIZES).index(camera))], axis=2).astype(np.uint8)


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def rigid(r, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = r, t
    return m


def draw(seed):
    rng = np.random.default_rng(seed)
    ego = [rigid(rot_z(0.02 * f), [0.5 * f, 0.05 * f, 0.0]) for f in range(FRAMES)]
    l2w = np.stack([e @ rigid(rot_z(0.3), [0.2, 0.0, 2.0]) for e in ego])
    cv = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    mounts = {"camera_FRONT": rigid(cv, [1.5, 0.0, 1.6]), "camera_SIDE_LEFT": rigid(rot_z(0.9) @ cv, [1.2, 0.5, 1.6])}
    observers = {"lidar_TOP": {"n_frames": FRAMES, "data": {"l2w": l2w}}}
    for name, (h, w, f) in SIZES.items():
        observers[name] = {"n_frames": FRAMES, "data": {"c2w": np.stack([e @ mounts[name] for e in ego]),
                                                         "intr": np.tile(np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]]), (FRAMES, 1, 1)),
                                                         "hw": np.tile(np.array([h, w]), (FRAMES, 1))}}
    centre = np.array([[10.0, 2.5, 0.8], [12.0, -3.0, 0.8], [16.0, 5.0, 0.8], [18.0, -1.0, 0.8]])
    speed = [0.6, 0.0, 0.6, 0.5]
    names = ["Vehicle", "Vehicle", "Sign", "Pedestrian"]
    tf = np.stack([np.stack([rigid(rot_z(0.2 * k + (0.03 * f if speed[k] else 0.0)), centre[k] + [speed[k] * f, 0, 0]) for f in range(FRAMES)]) for k in range(4)])
    objects = {}
    for k in range(4):
        runs = [[0], [2, 3]] if k == 0 else [[0, 1, 2, 3]]
        objects[f"o{k}"] = {"id": 10 + k, "class_name": names[k],
                            "segments": [{"start_frame": r[0], "n_frames": len(r), "data": {"transform": tf[k, r], "scale": np.tile(SCALE, (len(r), 1))}} for r in runs]}
    sweeps = []
    for f in range(FRAMES):
        pts = []
        for k, n in ((0, 130), (3, 12), (1, 20), (2, 20)):                 # in and around the boxes (object coordinates, 1.2 boxes wide)
            q = rng.uniform(-0.6, 0.6, (n, 3)) * SCALE
            pts.append(q @ tf[k, f, :3, :3].T + tf[k, f, :3, 3])
        for name, (h, w, fl) in SIZES.items():                              # through pixels of either camera, the borders included
            z = rng.uniform(3, 30, 45)
            u, v = rng.uniform(-3, w + 3, 45), rng.uniform(-3, h + 3, 45)
            u[:6] = rng.uniform(-0.95, -0.05, 6)                            # x in (-1, 0): column 0
            c = np.stack([(u - w / 2) / fl * z, (v - h / 2) / fl * z, z], axis=1)
            m = observers[name]["data"]["c2w"][f]
            pts.append(c @ m[:3, :3].T + m[:3, 3])
        pts.append(rng.uniform(-30, 30, (RAYS - sum(len(p) for p in pts), 3)))          # anywhere, behind the cameras too
        p = np.concatenate(pts)
        inv = np.linalg.inv(l2w[f])
        pl = p @ inv[:3, :3].T + inv[:3, 3]
        o = rng.normal(0, 0.02, pl.shape)
        r = np.linalg.norm(pl - o, axis=1)
        sweeps.append(((o).astype(np.float32), ((pl - o) / r[:, None]).astype(np.float32), r.astype(np.float32)))
    return {"observers": observers, "objects": objects}, sweeps


def margins_ok(scenario, sweeps):
    """No decision of the rule within MARGIN of its boundary; no point in two boxes of objects of the kept classes."""
    lidar = scenario["observers"]["lidar_TOP"]
    tables = {k: cr.object_tables(o, FRAMES) for k, o in scenario["objects"].items()}
    for transform, _, visibility in tables.values():
        shown = np.flatnonzero(visibility == 1)
        if abs(np.linalg.norm(transform[shown[-1]] - transform[shown[0]]) - 0.5) < MARGIN:
            return False
    for f in range(FRAMES):
        p = cr.world_points(*sweeps[f], lidar["data"]["l2w"][f][:3])
        for name in SIZES:
            d = scenario["observers"][name]["data"]
            w2c, K = cr.w2c_of(d["c2w"][f]), d["intr"][f]
            c = p @ w2c[:, :3].T + w2c[:, 3]
            xy = (c / c[:, 2:3]) @ K.T
            if np.any(np.abs(c[:, 2]) < MARGIN) or np.any(np.abs(xy[:, :2] - np.round(xy[:, :2])) < MARGIN):
                return False
        inside = np.zeros(len(p), int)
        for k, o in scenario["objects"].items():
            transform, scale, visibility = tables[k]
            if visibility[f] != 1:
                continue
            mask, q = cr.in_box(p, cr.w2c_of(transform[f]), scale[f])
            faces = np.stack([np.abs(np.abs(q[:, 0]) - scale[f][0] / 2), np.abs(np.abs(q[:, 1]) - scale[f][1] / 2),
                              np.abs(q[:, 2] - scale[f][2] / 2), np.abs(q[:, 2] - (-scale[f][2] / 2 + 0.25))])
            if np.any(faces < MARGIN):
                return False
            inside += mask & (o["class_name"] in cr.CLASSES)
        if np.any(inside > 1):
            return False
    return True


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def u8(a):
    assert np.array_equal(a, a.astype(np.uint8))            # the colours are whole numbers
    return t(a.astype(np.uint8))


def main():
    seed = 20260
    scenario, sweeps = draw(seed)
    while not margins_ok(scenario, sweeps):
        seed += 1
        scenario, sweeps = draw(seed)
    assert margins_ok(scenario, sweeps)
    images = {}
    stored = []
    ref.Image = types.SimpleNamespace(open=lambda path: images[path])
    ref.store_ply = lambda path, xyz, rgb: stored.append((os.path.basename(path), np.array(xyz), np.array(rgb)))
    ref.segment_obj_from_lidar.__defaults__ = (0, FRAMES - 1, 0.3)
    out = {"seed": seed, "frames": [], "motion": {}}
    with tempfile.TemporaryDirectory() as path, contextlib.redirect_stdout(io.StringIO()):
        os.makedirs(os.path.join(path, "lidars", "lidar_TOP"))
        os.makedirs(os.path.join(path, "objects"))
        for f, (o, d, r) in enumerate(sweeps):
            np.savez(os.path.join(path, "lidars", "lidar_TOP", "{:08}.npz".format(f)), rays_o=o[None], rays_d=d[None], ranges=r[None])
            for name, (h, w, _) in SIZES.items():
                images[os.path.join(path, "images", name, "{:08}.jpg".format(f))] = pixel_image(name, h, w)
        pt_file = os.path.join(path, "scenario.pt")
        with open(pt_file, "wb") as fh:
            pickle.dump(scenario, fh)
        observers = scenario["observers"]
        tables = {k: cr.object_tables(o, FRAMES) for k, o in scenario["objects"].items()}
        for f, (o, d, r) in enumerate(sweeps):
            ro, rd, rr = ref.trans_local2global(o[None].copy(), d[None].copy(), r[None].copy(), observers["lidar_TOP"]["data"]["l2w"][f], offset=None)
            xyz = ro + rd * rr[:, np.newaxis]
            cls, mask = ref.get_color_from_camera(xyz, f, observers, path)
            rec = {"rays_o": t(o), "rays_d": t(d), "ranges": t(r), "o_w": t(ro), "d_w": t(rd), "xyz": t(xyz), "cls": u8(cls), "mask": t(mask), "cameras": {}, "objects": {}}
            for name in SIZES:
                c1, m1 = ref.get_color_from_camera(xyz, f, {name: observers[name]}, path)
                rec["cameras"][name] = {"cls": u8(c1), "mask": t(m1)}
            for k, (transform, scale, visibility) in tables.items():
                if visibility[f] == 1:
                    m, pl = ref.segment_object_pcd(scale[f], transform[f], xyz)
                    rec["objects"][k] = {"mask": t(np.asarray(m, dtype=bool)), "points_l": t(pl)}
            out["frames"].append(rec)
        for k, (transform, scale, visibility) in tables.items():
            out["motion"][k] = bool(ref.is_object_motion(transform, visibility))
        ref.save_object_from_pt(path, pt_file, 0, FRAMES - 1, voxel_size=-1)
        info_path = os.path.join(path, "objects_info.pkl")
        with open(info_path, "rb") as fh:
            obj_info = pickle.load(fh)
        ref.save_background_from_pt(path, pt_file, info_path, voxel_size=-1)
    assert [s[0] for s in stored] == ["10.ply", "background.ply"] and [o["id"] for o in obj_info] == [10], ([s[0] for s in stored], [o["id"] for o in obj_info])
    assert out["motion"] == {"o0": True, "o1": False, "o2": True, "o3": True}
    out["scenario"] = {"l2w": t(observers["lidar_TOP"]["data"]["l2w"]),
                       "cameras": {n: {k: t(np.asarray(v, dtype=np.float64)) for k, v in observers[n]["data"].items()} for n in SIZES},
                       "objects": {k: {"id": o["id"], "class_name": o["class_name"],
                                       "segments": [{"start_frame": s["start_frame"], "n_frames": s["n_frames"], "transform": t(s["data"]["transform"]),
                                                     "scale": t(s["data"]["scale"])} for s in o["segments"]]} for k, o in scenario["objects"].items()}}
    out["obj_info"] = [{"id": o["id"], "class_name": o["class_name"], "visibility": t(o["visibility"]), "bbox": t(o["bbox"]), "transform_obj": t(o["transform_obj"]),
                        "points": t(o["point_cloud"]["points"]), "colors": t(o["point_cloud"]["colors"]), "normals": t(o["point_cloud"]["normals"])} for o in obj_info]
    out["stored"] = [{"name": n, "xyz": t(x), "rgb": t(c)} for n, x, c in stored]
    path = os.path.join(HERE, "cloud_host.pt")
    torch.save(out, path)
    print(f"seed {seed}; object points {[len(o['points']) for o in out['obj_info']]}; background {len(stored[1][1])}; wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
