"""The scene-cloud kernels on the GPU (csrc/cloud.hip through mudg_amd/cloud.py) against the CPU definition of the rules
(tests/cloud_reference.py): torch.equal everywhere — both sides perform the same correctly rounded fp64 operations in the same order
and every sum is an integer, so there is no tolerance and no point is left out."""
import numpy as np
import pytest
import torch

import cloud_reference as cr
import splat_reference as sr

pytestmark = pytest.mark.gpu
CAMS = {"camera_FRONT": (40, 64, 48.0), "camera_SIDE_LEFT": (24, 64, 40.0)}           # h, w, focal length
COUNTS = (1000, 257, 1)
SCALE = np.array([4.0, 2.0, 1.6])


def _rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def _rigid(r, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = r, t
    return m


def _image(camera, frame, h, w):
    y, x = np.mgrid[0:h, 0:w]
    c = len(camera)
    return np.stack([(x * 7 + y * 13 + frame * 17 + c) % 256, (x * 3 + y * 5 + frame) % 256, (x + y * 2 + c) % 256], axis=2).astype(np.uint8)


@pytest.fixture(scope="module")
def sweep_case():
    """3 frames of 1000, 257 and 1 rays; two cameras of 40 x 64 and 24 x 64 looking almost the same way (many points are seen by
    both); objects 0 and 2 overlap, object 1 is not visible in frame 1 and nothing is visible in frame 2.  Frame 0's matrices hold
    only small binary fractions, and its first rays have range 0, so their camera coordinates are exact: one of them projects beyond
    int32.  The definition's outputs are computed once here and shared."""
    rng = np.random.default_rng(31)
    frames = len(COUNTS)
    ego = [_rigid(_rot_z(0.03 * f), [0.5 * f, 0.0625 * f, 0.0]) for f in range(frames)]
    l2w = np.stack([e @ _rigid(np.eye(3), [0.25, 0.0, 2.0]) for e in ego])
    cv = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    mounts = {"camera_FRONT": _rigid(cv, [1.5, 0.0, 1.5]), "camera_SIDE_LEFT": _rigid(_rot_z(0.25) @ cv, [1.25, 0.5, 1.5])}
    observers = {"lidar_TOP": {"n_frames": frames, "data": {"l2w": l2w}}}
    for name, (h, w, fl) in CAMS.items():
        observers[name] = {"data": {"c2w": np.stack([e @ mounts[name] for e in ego]), "hw": np.tile(np.array([h, w]), (frames, 1)),
                                    "intr": np.tile(np.array([[fl, 0.0, w / 2.0], [0.0, fl, h / 2.0], [0.0, 0.0, 1.0]]), (frames, 1, 1))}}
    scenario = {"observers": observers, "objects": {}}
    centre = np.array([[10.0, 1.0, 0.8], [14.0, -2.0, 0.8], [11.0, 1.5, 0.8]])
    visibility = np.array([[1, 1, 0], [1, 0, 0], [1, 1, 0]])
    objects = [{"transform_obj": np.stack([_rigid(_rot_z(0.2 * k + 0.02 * f), centre[k] + [0.5 * f, 0, 0]) for f in range(frames)]),
                "bbox": np.tile(SCALE, (frames, 1)), "visibility": visibility[k]} for k in range(3)]
    sweeps = []
    for f, n in enumerate(COUNTS):
        inv = np.linalg.inv(l2w[f])
        if n == 1:
            p = np.array([[12.0, 0.5, 0.5]])
        else:
            pts = [(rng.uniform(-0.6, 0.6, (n // 6, 3)) * SCALE) @ o["transform_obj"][f][:3, :3].T + o["transform_obj"][f][:3, 3] for o in objects]
            for name, (h, w, fl) in CAMS.items():
                z = rng.uniform(3, 30, n // 6)
                u, v = rng.uniform(-3, w + 3, n // 6), rng.uniform(-3, h + 3, n // 6)
                u[:12] = rng.uniform(-0.95, -0.05, 12)                                  # x in (-1, 0): column 0
                m = observers[name]["data"]["c2w"][f]
                pts.append(np.stack([(u - w / 2) / fl * z, (v - h / 2) / fl * z, z], axis=1) @ m[:3, :3].T + m[:3, 3])
            pts.append(rng.uniform(-30, 30, (n - sum(len(p) for p in pts), 3)))         # anywhere, behind the cameras too
            p = np.concatenate(pts)
        pl = p @ inv[:3, :3].T + inv[:3, 3]
        o = rng.normal(0, 0.02, pl.shape)
        r = np.linalg.norm(pl - o, axis=1)
        d = (pl - o) / r[:, None]
        if f == 0:                                                                      # camera_FRONT sits at x = 1.5: zc = 2^-20, xc = -64
            o[0], r[0] = np.array([1.5 + 2.0 ** -20, 64.0, 1.5]) - l2w[0][:3, 3], 0.0
        sweeps.append((o.astype(np.float32), d.astype(np.float32), r.astype(np.float32)))
    images = [[_image(name, f, h, w) for name, (h, w, _) in CAMS.items()] for f in range(frames)]
    want = []
    for f in range(frames):
        cams = [(cr.w2c_of(observers[name]["data"]["c2w"][f]), observers[name]["data"]["intr"][f], images[f][c]) for c, name in enumerate(CAMS)]
        objs = [(cr.w2c_of(o["transform_obj"][f]), o["bbox"][f], True) if o["visibility"][f] == 1 else (None, None, False) for o in objects]
        want.append(cr.sweep(*sweeps[f], l2w[f][:3], cams, objs) + (cams, objs))
    return {"scenario": scenario, "objects": objects, "sweeps": sweeps, "images": images, "l2w": l2w, "want": want}


def _run_sweep(case, frames, dev):
    from mudg_amd import cloud, ops
    table, flat = cloud.camera_table(case["scenario"], frames, cr.CAMERAS, [case["images"][f] for f in frames])
    objs = cloud.object_table(case["objects"], frames)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    counts = [len(case["sweeps"][f][2]) for f in frames]
    rays = [up(np.concatenate([case["sweeps"][f][i] for f in frames])) for i in range(3)]
    return ops.cloud_sweep(*rays, up(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)), max(counts),
                           up(np.stack([case["l2w"][f][:3].reshape(12) for f in frames])), up(table), up(objs), up(flat))


def test_sweep_scene_reaches_every_case(sweep_case):
    """The definition's view of the scene (no kernel runs here): every branch the kernel has is taken by some return."""
    reached = dict.fromkeys(("behind both", "column 0", "beyond int32", "both cameras", "two boxes", "object", "background", "unseen"), 0)
    for f, (xyz, rgb, labels, cams, objs) in enumerate(sweep_case["want"]):
        p = cr.world_points(*sweep_case["sweeps"][f], sweep_case["l2w"][f][:3])
        masks, zs = [], []
        for w2c, K, image in cams:
            mask, ix, iy = cr.project(p, w2c, K, *image.shape[:2])
            with np.errstate(all="ignore"):
                zc = cr._row4(w2c[2], p[:, 0], p[:, 1], p[:, 2])
                x = (K[0, 0] * (cr._row4(w2c[0], p[:, 0], p[:, 1], p[:, 2]) / zc) + K[0, 1] * (cr._row4(w2c[1], p[:, 0], p[:, 1], p[:, 2]) / zc)) + K[0, 2]
            reached["column 0"] += int(np.sum(mask & (x < 0) & (x > -1)))
            reached["beyond int32"] += int(np.sum((zc > 0) & (np.abs(x) >= 2.0 ** 31)))
            masks.append(mask)
            zs.append(zc)
        reached["behind both"] += int(np.sum((zs[0] < 0) & (zs[1] < 0)))
        both = masks[0] & masks[1]
        reached["both cameras"] += int(np.sum(both))
        _, ix, iy = cr.project(p, cams[1][0], cams[1][1], *cams[1][2].shape[:2])
        assert np.array_equal(rgb[both], cams[1][2][iy[both], ix[both]])             # the last camera wins
        inside = [cr.in_box(p, w2l, box)[0] & (labels >= 0) for w2l, box, visible in objs if visible]
        if len(inside) == 3:
            two = inside[0] & inside[2]
            reached["two boxes"] += int(np.sum(two))
            assert np.all(labels[two] == 1)                                     # the lower-numbered object
        reached["object"] += int(np.sum(labels > 0))
        reached["background"] += int(np.sum(labels == 0))
        reached["unseen"] += int(np.sum(labels == -1))
    assert all(v > 0 for v in reached.values()), reached
    assert not any(o[2] for o in sweep_case["want"][2][4]) and set(np.unique(sweep_case["want"][1][2])) == {-1, 0, 1, 3}


def test_sweep_is_bit_equal_to_the_definition(cuda, sweep_case):
    points, labels = _run_sweep(sweep_case, [0, 1, 2], cuda)
    torch.cuda.synchronize()
    want_points = torch.from_numpy(np.concatenate([cr.pack(w[0], w[1]) for w in sweep_case["want"]]))
    want_labels = torch.from_numpy(np.concatenate([w[2] for w in sweep_case["want"]]))
    assert points.shape == (sum(COUNTS), 4) and labels.dtype == torch.int32
    print(f"sweep: {int((points.cpu() != want_points).sum())} of {want_points.numel()} words and {int((labels.cpu() != want_labels).sum())} labels differ")
    assert torch.equal(labels.cpu(), want_labels)
    assert torch.equal(points.cpu(), want_points)
    # the same batch as three one-frame launches, and a second run
    singles = [_run_sweep(sweep_case, [f], cuda) for f in range(3)]
    assert torch.equal(torch.cat([s[0] for s in singles]), points) and torch.equal(torch.cat([s[1] for s in singles]), labels)
    again = _run_sweep(sweep_case, [0, 1, 2], cuda)
    assert torch.equal(again[0], points) and torch.equal(again[1], labels)


def _voxel_clouds():
    rng = np.random.default_rng(17)
    grid = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 3)
    faces = np.round(rng.uniform(-3, 3, (600, 3)) * 2) / 2                             # multiples of 0.5: exactly on faces at v = 0.5
    return {"one": rng.uniform(-5, 5, (1, 3)), "257": rng.uniform(-2, 2, (257, 3)), "one voxel": 7.2 + rng.uniform(0.02, 0.28, (5000, 3)),
            "distinct": (grid - 8) * 0.6 + 0.15, "negative": -rng.uniform(0, 40, (3000, 3)), "faces": faces,
            "mixed": np.concatenate([rng.normal(0, 1.5, (6000, 3)), faces])}


@pytest.mark.parametrize("v", [0.5, 0.3])
def test_voxel_thinning_is_bit_equal_and_order_free(cuda, v):
    from mudg_amd import cloud, render
    rng = np.random.default_rng(5)
    for name, xyz in _voxel_clouds().items():
        xyz = xyz.astype(np.float32)
        rgb = rng.integers(0, 256, xyz.shape, dtype=np.uint8)
        want = torch.from_numpy(cr.pack(*cr.voxel_downsample(xyz, rgb, v)))
        got = cloud.voxel_downsample(render.PointCloud.from_arrays(xyz, rgb, cuda), v)
        assert isinstance(got, render.PointCloud) and torch.equal(got.points.cpu(), want), (name, v, len(got), len(want))
        if name == "one voxel":
            assert len(want) == 1
        if name == "distinct":
            assert len(want) == 4096
        if name == "negative":
            assert np.all(cr.voxel_indices(xyz, v) < 0)
        if name == "faces" and v == 0.5:
            assert np.all(xyz / 0.5 == np.round(xyz / 0.5))
        order = rng.permutation(len(xyz))
        shuffled = cloud.voxel_downsample(render.PointCloud.from_arrays(xyz[order], rgb[order], cuda), v)
        assert torch.equal(shuffled.points, got.points), (name, v)


def test_voxel_key_range_is_checked_before_any_launch(cuda):
    from mudg_amd import cloud, hip, render
    xyz = np.array([[0.0, 0.0, 0.0], [0.0, -6e5, 1.0]], dtype=np.float32)
    pc = render.PointCloud.from_arrays(xyz, np.zeros((2, 3), np.uint8), cuda)
    with pytest.raises(hip.MudgError, match="range"):
        cloud.voxel_downsample(pc, 0.5)
    assert len(cloud.voxel_downsample(pc, 2.0)) == 2                        # 3e5 voxels from the origin: in range
    with pytest.raises(hip.MudgError):
        cloud.voxel_downsample(pc, 0.0)


@pytest.fixture(scope="module")
def street():
    from mudg_amd.synthetic import street_sweeps
    scene = street_sweeps(frames=6, seed=0)                                  # object 0 keeps fewer than 100 points: a second pass
    return scene, {v: cr.scene_clouds(*scene, voxel_size=v, object_voxel_size=-1) for v in (-1, 0.3)}


def _render_both(built, wanted, scenario, cuda):
    from mudg_amd import render
    background, objects, obj_info = built
    bg_xyz, bg_rgb, want_info = wanted
    data = scenario["observers"]["camera_FRONT"]["data"]
    hw_native, hw = tuple(int(v) for v in data["hw"][0]), (144, 256)
    got = render.render_conditions(background, objects, data["intr"], data["c2w"], hw_native, hw, return_images=True)
    poses = np.stack([np.stack(render.virtual_poses(c, with_ori_pose=True)) for c in data["c2w"]])
    clouds = [(o["point_cloud"]["points"].astype(np.float32), np.round(o["point_cloud"]["colors"] * 255.0).astype(np.uint8)) for o in want_info]
    want = sr.render_conditions(bg_xyz, bg_rgb, clouds, np.stack([o["transform_obj"] for o in want_info]), np.stack([o["visibility"] for o in want_info]),
                                data["intr"][0], data["c2w"], hw_native, hw, poses)
    assert want["bg_depth"].astype(bool).mean() > 0.05 and want["obj_depth"].any()
    for name in ("bg_rgb", "bg_depth", "obj_rgb", "obj_depth", "mask", "sparse_frames", "sparse_depth"):
        assert torch.equal(got[name].cpu(), torch.from_numpy(np.ascontiguousarray(want[name]))), name


@pytest.mark.parametrize("v", [-1, 0.3])
def test_build_scene_clouds_equals_the_definition_and_renders_alike(cuda, street, v):
    """6 frames of about 20 000 returns, 3 moving boxes (one is dropped for its point count, so the background takes a second pass),
    a static box and a Sign; then the merged renderer on the clouds."""
    from mudg_amd import cloud, render
    scene, wanted = street
    bg_xyz, bg_rgb, want_info = wanted[v]
    built = cloud.build_scene_clouds(*scene, voxel_size=v, frames_per_launch=4, device=cuda)
    background, objects, obj_info = built
    assert torch.equal(background.points.cpu(), torch.from_numpy(cr.pack(bg_xyz, bg_rgb)))
    assert len(wanted[0.3][0]) < len(wanted[-1][0]) and len(background) == len(bg_xyz)
    assert [o["id"] for o in obj_info] == [o["id"] for o in want_info] == [1, 2]
    for mine, theirs in zip(obj_info, want_info):
        assert set(mine) == set(theirs) == {"id", "class_name", "visibility", "bbox", "transform_obj", "point_cloud", "ply_path"}
        for name in ("visibility", "bbox", "transform_obj"):
            assert np.array_equal(mine[name], theirs[name]), name
        for name in ("points", "colors", "normals"):
            assert np.array_equal(mine["point_cloud"][name], theirs["point_cloud"][name]) and mine["point_cloud"][name].dtype == np.float64, name
    assert obj_info[0]["visibility"][1] == 0
    same = render.ObjectSet.from_obj_info(obj_info, cuda)
    assert torch.equal(same.cloud.points, objects.cloud.points) and torch.equal(same.ids, objects.ids)
    _render_both(built, wanted[v], scene[0], cuda)
    if v == -1:                                                               # frames_per_launch does not change a bit
        for step in (1, None):
            other = cloud.build_scene_clouds(*scene, frames_per_launch=step, device=cuda)
            assert torch.equal(other[0].points, background.points) and torch.equal(other[1].cloud.points, objects.cloud.points)
        scn = render.Scene.from_scenario(*scene, frames_per_launch=4, device=cuda)
        assert torch.equal(scn.background.points, background.points) and scn.hw_native == (320, 480) and scn.c2w.shape == (6, 4, 4)


@pytest.mark.parametrize("seed, kept", [(16, [0, 1, 2]), (3, [0])])
def test_object_thinning(cuda, seed, kept):
    """object_voxel_size = 0.1.  Seed 16: all three moving objects keep 100 points after thinning, so one pass serves objects and
    background.  Seed 3: objects 1 and 2 (128 and 112 points) fall below 100 only once thinned, and the background takes them back."""
    from mudg_amd import cloud
    from mudg_amd.synthetic import street_sweeps
    scene = street_sweeps(frames=6, seed=seed)
    bg_xyz, bg_rgb, want_info = cr.scene_clouds(*scene, voxel_size=-1, object_voxel_size=0.1)
    assert [o["id"] for o in want_info] == kept                                  # the scene is what the docstring says
    background, objects, obj_info = cloud.build_scene_clouds(*scene, object_voxel_size=0.1, device=cuda)
    assert torch.equal(background.points.cpu(), torch.from_numpy(cr.pack(bg_xyz, bg_rgb)))
    assert [o["id"] for o in obj_info] == kept
    for mine, theirs in zip(obj_info, want_info):
        assert np.array_equal(mine["point_cloud"]["points"], theirs["point_cloud"]["points"])
        assert np.array_equal(mine["point_cloud"]["colors"], theirs["point_cloud"]["colors"])
