"""The scene-cloud rules on the CPU (no GPU needed): the numpy definition (tests/cloud_reference.py) and the host logic of
mudg_amd/cloud.py against what the reference's process_lidar.py computed on the tiny scenario of tests/golden/make_golden_cloud.py.
That scenario keeps every point 1e-6 away from every decision boundary, some 10^6 times what float64 rounding moves, so every mask,
pixel, colour and label must agree exactly; coordinates agree to 1e-9 relative (the reference multiplies through BLAS)."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import cloud_reference as cr
from helpers import GOLDEN

SIZES = {"camera_FRONT": (24, 32), "camera_SIDE_LEFT": (16, 24)}


def pixel_image(camera, h, w):
    idx = (np.arange(h)[:, None] * w + np.arange(w)[None, :])
    return np.stack([idx & 255, idx >> 8, np.full_like(idx, 1 + list(SIZES).index(camera))], axis=2).astype(np.uint8)


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= 1e-9 * np.maximum(np.abs(b), 1e-3)))


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(GOLDEN, "cloud_host.pt"), map_location="cpu", weights_only=True)


@pytest.fixture(scope="module")
def scene(gold):
    """The scenario in the reference's layout, and the two loaders."""
    s = gold["scenario"]
    observers = {"lidar_TOP": {"n_frames": 4, "data": {"l2w": s["l2w"].numpy()}}}
    for name, d in s["cameras"].items():
        observers[name] = {"n_frames": 4, "data": {k: v.numpy() for k, v in d.items()}}
    objects = {k: {"id": o["id"], "class_name": o["class_name"],
                   "segments": [{"start_frame": g["start_frame"], "n_frames": g["n_frames"], "data": {"transform": g["transform"].numpy(), "scale": g["scale"].numpy()}}
                                for g in o["segments"]]} for k, o in s["objects"].items()}
    load_lidar = lambda f: tuple(gold["frames"][f][k].numpy() for k in ("rays_o", "rays_d", "ranges"))
    load_image = lambda camera, f: pixel_image(camera, *SIZES[camera])
    return {"observers": observers, "objects": objects}, load_lidar, load_image


def test_world_points_and_colours_reproduce_the_reference(gold, scene):
    scenario, load_lidar, load_image = scene
    reached = {"both": 0, "none": 0, "column0": 0, "behind": 0}
    for f, rec in enumerate(gold["frames"]):
        p = cr.world_points(*load_lidar(f), scenario["observers"]["lidar_TOP"]["data"]["l2w"][f][:3])
        assert close(p, rec["xyz"].numpy())
        cams = cr.frame_cameras(scenario, f, cr.CAMERAS, load_image)
        rgb, seen = cr.colours(p, cams)
        assert np.array_equal(seen, rec["mask"].numpy()) and np.array_equal(rgb[seen], rec["cls"].numpy()[seen])
        masks = []
        for (w2c, K, image), name in zip(cams, SIZES):
            mask, ix, iy = cr.project(p, w2c, K, *image.shape[:2])
            want = rec["cameras"][name]
            assert np.array_equal(mask, want["mask"].numpy())
            col = want["cls"].numpy()[mask].astype(np.int64)                 # the reference's colour names the pixel it read
            assert np.array_equal(iy[mask] * image.shape[1] + ix[mask], col[:, 0] | (col[:, 1] << 8))
            masks.append(mask)
            c = p @ w2c[:, :3].T + w2c[:, 3]
            x = (c[:, 0] / c[:, 2]) * K[0, 0] + K[0, 2]
            reached["column0"] += int(np.sum(mask & (x < 0)))
            reached["behind"] += int(np.sum(c[:, 2] < 0))
        reached["both"] += int(np.sum(masks[0] & masks[1]))
        reached["none"] += int(np.sum(~seen))
        both = masks[0] & masks[1]
        assert np.all(rgb[both, 2] == 2)                                        # the last camera wins
    assert all(v > 0 for v in reached.values()), reached


def test_boxes_labels_and_motion_reproduce_the_reference(gold, scene):
    from mudg_amd import cloud
    scenario, load_lidar, _ = scene
    for k, obj in scenario["objects"].items():
        transform, scale, visibility = cr.object_tables(obj, 4)
        for mine, theirs in zip(cloud.object_tables(obj, 4), (transform, scale, visibility)):
            assert np.array_equal(mine, theirs)
        assert cr.is_object_motion(transform, visibility) == gold["motion"][k] == cloud.is_object_motion(transform, visibility)
        for f, rec in enumerate(gold["frames"]):
            assert (k in rec["objects"]) == (visibility[f] == 1)
            if visibility[f] == 1:
                mask, q = cr.in_box(rec["xyz"].numpy(), cr.w2c_of(transform[f]), scale[f])
                assert np.array_equal(mask, rec["objects"][k]["mask"].numpy()) and mask.any() and not mask.all()
                assert close(q, rec["objects"][k]["points_l"].numpy())
                assert np.array_equal(cr.w2c_of(transform[f]), cloud.inverse_rigid(transform[f]))
    assert gold["motion"] == {"o0": True, "o1": False, "o2": True, "o3": True}
    assert [o["id"] for o in cloud.moving_objects(scenario, [0, 1, 2, 3])] == [10, 13]        # the Sign moves too, and is not taken


def test_scene_clouds_reproduce_obj_info_and_the_background(gold, scene):
    """save_object_from_pt and save_background_from_pt: one object survives (the static one, the Sign and the one with fewer than
    100 points do not), it is invisible in frame 1, and the background is what store_ply received."""
    bg_xyz, bg_rgb, obj_info = cr.scene_clouds(*scene)
    assert len(obj_info) == len(gold["obj_info"]) == 1
    mine, theirs = obj_info[0], gold["obj_info"][0]
    assert mine["id"] == theirs["id"] == 10 and mine["class_name"] == theirs["class_name"]
    for name in ("visibility", "bbox", "transform_obj"):
        assert np.array_equal(mine[name], theirs[name].numpy()), name
    assert mine["visibility"][1] == 0
    pts = theirs["points"].numpy()
    assert 100 <= len(pts) == len(mine["point_cloud"]["points"])
    assert np.array_equal(mine["point_cloud"]["points"], pts.astype(np.float32).astype(np.float64))          # the packed format is fp32
    assert np.array_equal(mine["point_cloud"]["colors"], theirs["colors"].numpy())
    assert np.array_equal(mine["point_cloud"]["normals"], theirs["normals"].numpy())
    names = [s["name"] for s in gold["stored"]]
    assert names == ["10.ply", "background.ply"]
    assert np.array_equal(gold["stored"][0]["rgb"].numpy(), mine["point_cloud"]["colors"] * 255.0)
    want_xyz, want_rgb = gold["stored"][1]["xyz"].numpy(), gold["stored"][1]["rgb"].numpy()
    assert np.array_equal(bg_xyz, want_xyz.astype(np.float32)) and close(bg_xyz, want_xyz.astype(np.float32))
    assert np.array_equal(bg_rgb, np.round(want_rgb).astype(np.uint8)) and np.allclose(want_rgb, np.round(want_rgb), atol=1e-9, rtol=0)


def test_voxel_definition_against_a_brute_force_mean():
    rng = np.random.default_rng(7)
    xyz = np.concatenate([rng.uniform(-2, 2, (400, 3)), np.round(rng.uniform(-2, 2, (100, 3)) * 2) / 2]).astype(np.float32)    # some on faces
    rgb = rng.integers(0, 256, (500, 3), dtype=np.uint8)
    for v in (0.5, 0.3):
        got_xyz, got_rgb = cr.voxel_downsample(xyz, rgb, v)
        cells = {}
        for p, c in zip(xyz, rgb):
            idx = tuple(int(np.floor(np.float64(a) / np.float64(v))) for a in p)
            frac = tuple(min(max(int(np.floor(((np.float64(a) - i * np.float64(v)) / np.float64(v)) * 2.0 ** 32)), 0), 2 ** 32 - 1) for a, i in zip(p, idx))
            cells.setdefault(idx, []).append((frac, tuple(int(x) for x in c)))
        keys = sorted(cells)                                                   # tuple order = key order: the indices are offset alike
        assert len(keys) == len(got_xyz) and 1 < len(keys) < 500
        for k, idx in enumerate(keys):
            members = cells[idx]
            n = len(members)
            for a in range(3):
                s = sum(m[0][a] for m in members)
                want = np.float64(idx[a]) * np.float64(v) + np.float64(v) * (np.float64(s) / (np.float64(n) * 2.0 ** 32))
                assert got_xyz[k, a] == np.float32(want)
                exact = Fraction(idx[a]) * Fraction(v) + Fraction(v) * Fraction(s, n * 2 ** 32)      # the mean of the quantised points
                assert abs(Fraction(float(got_xyz[k, a])) - exact) <= Fraction(1, 2 ** 20)
                c = sum(m[1][a] for m in members)
                assert int(got_rgb[k, a]) == (2 * c + n) // (2 * n) == int(Fraction(c, n) + Fraction(1, 2))      # round half up
        assert any(min(i) < 0 for i in keys)                                   # floor, not truncation: negative voxels exist
        assert all(np.all(cr.voxel_indices(xyz[xyz[:, a] < 0], v)[:, a] < 0) for a in range(3))


def test_key_range_error():
    assert cr.voxel_keys(np.array([[(1 << 20) - 1, -(1 << 20) + 1, 0]], dtype=np.int64))[0] > 0
    with pytest.raises(ValueError):
        cr.voxel_keys(np.array([[1 << 20, 0, 0]], dtype=np.int64))
    with pytest.raises(ValueError):
        cr.voxel_keys(cr.voxel_indices(np.array([[0.0, -6e5, 0.0]], dtype=np.float32), 0.5))


def test_street_sweeps_is_deterministic_per_seed():
    from mudg_amd.synthetic import street_sweeps
    a, b, c = (street_sweeps(frames=3, beams=8, azimuths=90, seed=s) for s in (4, 4, 5))
    for f in range(3):
        for x, y in zip(a[1](f), b[1](f)):
            assert np.array_equal(x, y) and x.dtype == np.float32
        for cam in ("camera_FRONT", "camera_SIDE_LEFT"):
            assert np.array_equal(a[2](cam, f), b[2](cam, f)) and a[2](cam, f).dtype == np.uint8
            assert a[2](cam, f).shape == (*a[0]["observers"][cam]["data"]["hw"][f],  3)
    assert a[0]["observers"]["camera_FRONT"]["data"]["hw"][0].tolist() != a[0]["observers"]["camera_SIDE_LEFT"]["data"]["hw"][0].tolist()
    for k in a[0]["objects"]:
        for sa, sb in zip(a[0]["objects"][k]["segments"], b[0]["objects"][k]["segments"]):
            assert np.array_equal(sa["data"]["transform"], sb["data"]["transform"])
    assert not np.array_equal(a[0]["objects"]["obj_0"]["segments"][0]["data"]["transform"], c[0]["objects"]["obj_0"]["segments"][0]["data"]["transform"])
    assert len({len(a[1](f)[2]) for f in range(3)}) > 1 or len(a[1](0)[2]) != 8 * 90          # only hits are returns
