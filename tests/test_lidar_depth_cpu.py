"""The CPU definition of the LiDAR depth maps and the dense completion (tests/lidar_depth_reference.py) against what the
reference computes where it computes the same thing (the window and the per-frame returns, tests/golden/make_golden_lidar.py), against
scipy where the rule is a classical operator, and against the properties the rules were chosen for: a plane never hides itself, the
filter removes most of what shows through and little else, and a constant map stays constant.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import lidar_depth_cases as cases
import lidar_depth_reference as ld
from helpers import GOLDEN

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ against the reference
def test_the_window_rule_is_the_reference_s():
    from mudg_amd import depth
    with open(os.path.join(GOLDEN, "lidar_windows.json")) as fh:
        gold = json.load(fh)
    assert sorted(gold, key=int) == [str(n) for n in range(1, 9)]
    for n in range(1, 9):
        assert len(gold[str(n)]) == n
        for i in range(n):
            assert ld.window_frames(i, n) == gold[str(n)][i] == depth.window_frames(i, n), (n, i)
    assert ld.window_frames(0, 8) == [0, 0, 0, 1, 2, 3] and ld.window_frames(7, 8) == [5, 6, 7, 7, 7, 7]
    assert ld.window_frames(3, 8, (-1, 1)) == [2, 3, 4] == depth.window_frames(3, 8, (-1, 1))


def test_the_per_frame_returns_are_the_reference_s():
    """load_lidar_data on make_golden_cloud.py's scenario: the same points in the same order (the reference's float64 rounded to the
    packed format's float32) with the same colours, frame by frame; together they are the background cloud_host.pt stores."""
    SIZES = {"camera_FRONT": (24, 32), "camera_SIDE_LEFT": (16, 24)}

    def pixel_image(camera, h, w):                                              # make_golden_cloud.py's images: a pixel holds its own index
        idx = (np.arange(h)[:, None] * w + np.arange(w)[None, :])
        return np.stack([idx & 255, idx >> 8, np.full_like(idx, 1 + list(SIZES).index(camera))], axis=2).astype(np.uint8)
    gold = torch.load(os.path.join(GOLDEN, "lidar_frames.pt"), map_location="cpu", weights_only=True)
    host = torch.load(os.path.join(GOLDEN, "cloud_host.pt"), map_location="cpu", weights_only=True)
    assert gold["seed"] == host["seed"]
    s = host["scenario"]
    observers = {"lidar_TOP": {"n_frames": 4, "data": {"l2w": s["l2w"].numpy()}}}
    for name, d in s["cameras"].items():
        observers[name] = {"n_frames": 4, "data": {k: v.numpy() for k, v in d.items()}}
    objects = {k: {"id": o["id"], "class_name": o["class_name"],
                   "segments": [{"start_frame": g["start_frame"], "n_frames": g["n_frames"], "data": {"transform": g["transform"].numpy(), "scale": g["scale"].numpy()}}
                                for g in o["segments"]]} for k, o in s["objects"].items()}
    scenario = {"observers": observers, "objects": objects}
    load_lidar = lambda f: tuple(host["frames"][f][k].numpy() for k in ("rays_o", "rays_d", "ranges"))
    load_image = lambda camera, f: pixel_image(camera, *SIZES[camera])
    obj_info = ld.cr.scene_clouds(scenario, load_lidar, load_image)[2]
    assert [o["id"] for o in obj_info] == gold["object_ids"] == [10]
    mine = ld.frame_sweeps(scenario, load_lidar, load_image, obj_info)
    assert len(mine) == len(gold["points"]) == 4
    for f, (xyz, rgb) in enumerate(mine):
        want = gold["points"][f].numpy()
        assert 100 < len(want) < 300                                            # some rays are unseen, some are the object's
        assert np.array_equal(xyz, want.astype(F)), f
        assert np.array_equal(rgb, gold["colours"][f].numpy()), f
    assert np.array_equal(np.concatenate([m[0] for m in mine]), host["stored"][1]["xyz"].numpy().astype(F))


# ------------------------------------------------------------------------------------------------ the splat side of the definition
def _tiny_scene():
    from mudg_amd.synthetic import street_sweeps
    scenario, load_lidar, load_image = street_sweeps(frames=4, beams=16, azimuths=200)
    sweeps = ld.frame_sweeps(scenario, load_lidar, load_image, [])
    return scenario, sweeps


def test_without_the_filter_the_map_is_one_splat_of_the_candidates():
    """The definition's own projection (it needs the home pixel) and splat_reference's are the same arithmetic: with occlusion off the
    map is sr.splat of all candidates, and every pixel of it holds the camera depth project() gives for some candidate."""
    scenario, sweeps = _tiny_scene()
    data = scenario["observers"]["camera_FRONT"]["data"]
    for frame, n_want in ((0, 4), (3, 3), (1, 4)):                               # the window clamps: frames {0 .. 3}, {1 .. 3}, {0 .. 3}
        xyz, mats = ld.candidates([s[0] for s in sweeps], None, None, None, data["c2w"][frame], frame)
        assert len(xyz) == sum(len(sweeps[f][0]) for f in set(ld.window_frames(frame, 4))) and len(set(ld.window_frames(frame, 4))) == n_want
        cam = ld.sr.scaled_camera(data["intr"][frame], (320, 480), (37, 53))
        got = ld.lidar_depth(xyz, mats, cam, 37, 53, occlusion=False)
        want = ld.sr.splat(xyz, np.zeros((len(xyz), 3), np.uint8), mats, cam, 2.0, 37, 53)[1]
        assert np.array_equal(got, want) and (got > 0).sum() > 200
        zc, u, v, ok = ld.project(xyz, mats, cam)
        assert np.isin(got[got > 0], zc[ok]).all()
        on, hid = ld.lidar_depth(xyz, mats, cam, 37, 53, return_hidden=True)
        assert hid.any() and not hid.all() and not ((on > 0) & (got == 0)).any()


def test_a_far_plane_behind_a_near_plane_with_gaps_is_hidden_and_an_open_one_is_not():
    """A dense wall at 30 m behind a dense wall at 10 m of which every fourth column is missing: the far points seen through the gaps have
    nearer pixels on both sides of their row and go; with the near wall cut off at the image's middle the far points beyond it stay."""
    H, W, f = 40, 64, 50.0
    cam = np.array([f, f, W / 2.0, H / 2.0], F)
    j, i = np.mgrid[0:H, 0:W]
    centre = lambda z, keep: np.stack([(i[keep] + 0.5 - W / 2.0) / f * z, (j[keep] + 0.5 - H / 2.0) / f * z, np.full(int(keep.sum()), z)], axis=1).astype(F)
    far = centre(30.0, np.ones((H, W), bool))
    near = centre(10.0, i % 4 != 3)
    xyz = np.concatenate([far, near])
    depth, hid = ld.lidar_depth(xyz, cases.IDENTITY, cam, H, W, point_size=1.0, return_hidden=True)
    assert not hid[len(far):].any()
    gaps = (i % 4 == 3).reshape(-1)
    assert hid[:len(far)][gaps & (i.reshape(-1) > 3) & (i.reshape(-1) < W - 4)].all()
    assert (depth[:, 4:W - 4][:, (np.arange(4, W - 4) % 4) == 3] == 0).all() and (depth[:, ::4] == F(10.0)).all()
    half = centre(10.0, i < W // 2)
    depth, hid = ld.lidar_depth(np.concatenate([far, half]), cases.IDENTITY, cam, H, W, point_size=1.0, return_hidden=True)
    beyond = i.reshape(-1) >= W // 2                                             # nearer pixels on one side only, along every line
    assert not hid[:len(far)][beyond].any() and not hid[len(far):].any() and hid[:len(far)][((i > 0) & (i < W // 2 - 1)).reshape(-1)].all()
    assert (depth[:, W // 2:] == F(30.0)).all() and (depth[:, :W // 2] == F(10.0)).all()


def test_a_plane_never_hides_its_own_points():
    xyz = cases.plane_points()
    cam = ld.sr.scaled_camera(cases.PLANE_K, cases.PLANE_HW, cases.PLANE_HW)
    for reach in cases.REACHES:
        depth, hid = ld.lidar_depth(xyz, cases.IDENTITY, cam, *cases.PLANE_HW, reach=reach, rel_tol=cases.PLANE_REL_TOL, return_hidden=True)
        print(f"reach {reach}: {int(hid.sum())} of {len(xyz)} points hidden, {int((depth > 0).sum())} pixels covered")
        assert not hid.any(), reach
    assert (depth > 0).sum() > 0.6 * depth.size


def test_the_filter_removes_what_shows_through_and_little_else():
    cases.leak_conditions(*cases.leak_maps())


# ------------------------------------------------------------------------------------------------ the completion
def test_the_morphological_steps_are_scipy_s():
    ndi = pytest.importorskip("scipy.ndimage")
    diamond = np.array([[abs(a) + abs(b) <= 2 for b in range(-2, 3)] for a in range(-2, 3)])
    for shape, density in (((1, 40, 67), 0.05), ((1, 33, 21), 0.3), ((1, 50, 50), 0.01)):
        x1 = ld.step1(cases.sparse_map(shape, density)[0])
        assert (x1 >= 0).all() and np.isfinite(x1).all() and 0 < (x1 > 0).mean() < 0.5
        x2 = ld.step2(x1)
        assert np.array_equal(x2, ndi.grey_dilation(x1, footprint=diamond, mode="constant", cval=0.0))
        x3 = ld.step3(x2)
        dil = ndi.grey_dilation(x2, size=(5, 5), mode="constant", cval=0.0)
        assert np.array_equal(x3, ndi.grey_erosion(dil, size=(5, 5), mode="constant", cval=np.inf))
        x4 = ld.step4(x3)
        assert np.array_equal(x4, np.where(x3 < F(0.1), ndi.grey_dilation(x3, size=(7, 7), mode="constant", cval=0.0), x3))
        x5 = ld.step5(x4)
        top = x4.copy()
        for c in range(top.shape[1]):                                          # the column rule, as a loop
            rows = np.flatnonzero(top[:, c] >= F(0.1))
            if len(rows):
                top[:rows[0], c] = top[rows[0], c]
        assert np.array_equal(x5, np.where(top < F(0.1), ndi.grey_dilation(top, size=(31, 31), mode="constant", cval=0.0), top))
        x6 = ld.step6(x5)
        assert np.array_equal(x6, ndi.median_filter(x5, size=(5, 5), mode="nearest"))
        assert (x2 >= x1).all() and (x3 >= x2).all() and (x4 >= x3).all() and (x5 >= x4).all()          # nothing measured is lost on the way


def test_the_blur_is_a_normalised_binomial_over_the_filled_pixels():
    rng = np.random.default_rng(3)
    x = np.where(rng.random((20, 30)) < 0.6, rng.uniform(0.1, 99.0, (20, 30)), 0.0).astype(F)
    got = ld.step7(x)
    w1 = np.array([1.0, 4.0, 6.0, 4.0, 1.0])
    for j, i in ((0, 0), (0, 29), (19, 0), (10, 15), (3, 28)):
        num = den = 0.0
        for a in range(-2, 3):
            for b in range(-2, 3):
                if 0 <= j + a < 20 and 0 <= i + b < 30 and x[j + a, i + b] >= F(0.1):
                    num += w1[a + 2] * w1[b + 2] * float(x[j + a, i + b])
                    den += w1[a + 2] * w1[b + 2]
        assert got[j, i] == (F(num / den) if x[j, i] >= F(0.1) else x[j, i])
    assert np.array_equal(got == 0, x == 0)


def test_constant_maps_stay_constant():
    d = cases.constant_map()
    assert 0.02 < (d > 0).mean() < 0.04
    for extrapolate in (False, True):
        out, source = ld.complete_depth_frames(d, extrapolate=extrapolate)
        assert set(np.unique(out)) <= {F(0), F(12.5)} and (out == F(12.5)).mean() > 0.5
        assert np.array_equal(source == 1, d > 0) and np.array_equal(source == 0, out == 0)
    assert (out == F(12.5)).all() and set(np.unique(source)) == {1, 2, 3}


def test_step_one_empties_what_is_not_a_depth_and_the_source_map_names_the_stage():
    d = cases.sparse_map((2, 40, 67), 0.05)
    assert np.isnan(d).any() and np.isinf(d).any() and (d == F(0.1)).any() and (d > 100).any()
    x1 = ld.step1(d[0])
    with np.errstate(all="ignore"):
        valid = (d[0] > F(0.1)) & (F(100.0) - d[0] >= F(0.1))
    assert np.array_equal(x1 > 0, valid) and (x1[~valid] == 0).all() and not valid[d[0] == F(0.1)].any()
    labels = np.zeros(d.shape, np.int64)
    labels[:, :5, 10:30] = 10
    out, source = ld.complete_depth_frames(d, labels)
    assert (out[labels == 10] == F(100.0)).all() and (source[labels == 10] == 4).all()
    assert np.array_equal((source == 1)[0] & (labels[0] != 10), valid & (labels[0] != 10))
    assert ((out > 0) == (source > 0)).all() and np.isfinite(out).all() and (out >= 0).all() and (out <= F(100.0)).all()
    empty, _ = ld.complete_depth_frames(np.zeros((1, 9, 9), F))
    assert not empty.any()
