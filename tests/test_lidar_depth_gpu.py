"""The LiDAR depth maps and the dense completion on the GPU (csrc/lidar_depth.hip through mudg_amd/ops.py, cloud.py, depth.py and
render.py) against the numpy definition of the rules (tests/lidar_depth_reference.py): torch.equal everywhere and a repeat run equal to
the first — the depth test is an integer minimum and every other operation a selection or one correctly rounded operation, so there is
no tolerance.  Then the properties the rules were chosen for, on the kernels, and the chain sweeps -> depth -> normals -> clips."""
import functools

import numpy as np
import pytest
import torch

import lidar_depth_cases as cases
import lidar_depth_reference as ld

pytestmark = pytest.mark.gpu

F = np.float32


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    differ = int((got != want).sum())
    print(f"{what}: {differ} of {want.numel()} values differ")
    assert differ == 0 and torch.equal(got, want), (what, differ)


def _sweeps(frames_xyz, dev):
    """Per-frame (n, 3) arrays (some empty) -> render.FrameSweeps with black points."""
    from mudg_amd import render
    xyz = np.concatenate([np.asarray(p, F).reshape(-1, 3) for p in frames_xyz])
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in frames_xyz])])
    return render.FrameSweeps(render._pack(xyz, np.zeros(xyz.shape, np.uint8), dev), offsets)


# ------------------------------------------------------------------------------------------------ per-frame sweeps
TINY = dict(frames=4, beams=16, azimuths=200)


@functools.lru_cache(maxsize=None)
def _tiny_definition():
    from mudg_amd.synthetic import street_sweeps
    scene = street_sweeps(**TINY)
    obj_info = ld.cr.scene_clouds(*scene)[2]
    assert [o["id"] for o in obj_info] == [2]
    return scene, obj_info, ld.frame_sweeps(*scene, obj_info)


@pytest.fixture(scope="module")
def tiny(cuda):
    from mudg_amd import cloud
    scene, want_info, want = _tiny_definition()
    background, objects, obj_info = cloud.build_scene_clouds(*scene, device=cuda)
    sweeps = cloud.frame_sweeps(*scene, obj_info, frames_per_launch=3, device=cuda)
    return scene, background, objects, obj_info, sweeps


def test_frame_sweeps_are_the_background_frame_by_frame(cuda, tiny):
    from mudg_amd import cloud, hip, render
    scene, background, objects, obj_info, sweeps = tiny
    want = _tiny_definition()[2]
    assert sweeps.frames == 4 and sweeps.offsets.tolist() == np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]).tolist()
    assert torch.equal(sweeps.points, background.points)                      # bit for bit the background of voxel_size = -1
    for f in range(4):
        _same(sweeps.frame(f), ld.cr.pack(*want[f]), f"frame {f}'s returns")
    again = cloud.frame_sweeps(*scene, obj_info, device=cuda)                 # one launch for all frames, or two: the same
    assert torch.equal(again.points, sweeps.points) and torch.equal(again.offsets, sweeps.offsets)
    scn = render.Scene.from_scenario(*scene, keep_sweeps=True, frames_per_launch=3, device=cuda)
    assert torch.equal(scn.sweeps.points, sweeps.points) and torch.equal(scn.sweeps.offsets, sweeps.offsets)
    assert torch.equal(scn.background.points, background.points)
    assert render.Scene.from_scenario(*scene, device=cuda).sweeps is None
    thinned = render.Scene.from_scenario(*scene, keep_sweeps=True, voxel_size=0.5, device=cuda)
    assert torch.equal(thinned.sweeps.points, sweeps.points) and len(thinned.background) < len(background)
    with pytest.raises(hip.MudgError, match="GPU"):
        cloud.frame_sweeps(*scene, obj_info, device="cpu")
    with pytest.raises(hip.MudgError, match="GPU"):
        render.FrameSweeps(sweeps.points.cpu(), sweeps.offsets)
    with pytest.raises(hip.MudgError, match="offsets"):
        render.FrameSweeps(sweeps.points, [0, 5])


# ------------------------------------------------------------------------------------------------ the maps
def _with_object_one(scene, obj_info, dev):
    """The surviving object and, beside it, object 1 — which the scene does not track in frame 1 — as seeded points on its box."""
    from mudg_amd import render
    rng = np.random.default_rng(11)
    transform, scale, visibility = ld.cr.object_tables(scene[0]["objects"]["obj_1"], TINY["frames"])
    assert visibility.tolist() == [1, 0, 1, 1]
    p = rng.uniform(-0.5, 0.5, (400, 3))
    axis = rng.integers(0, 3, 400)
    p[np.arange(400), axis] = np.sign(p[np.arange(400), axis]) * 0.5
    clouds = [(o["point_cloud"]["points"], o["point_cloud"]["colors"]) for o in obj_info] + [((p * scale[0]).astype(F), np.full((400, 3), 200, np.uint8))]
    tf = np.stack([np.asarray(o["transform_obj"]) for o in obj_info] + [transform])
    vis = np.stack([np.asarray(o["visibility"]) for o in obj_info] + [visibility])
    return render.ObjectSet(clouds, tf, vis, dev), clouds, tf, vis


MODES = [dict(occlusion=False), dict(), dict(reach=1, occluder_size=2.0, point_size=1.0), dict(reach=4, occluder_size=2.0),
         dict(reach=1, point_size=1.0, rel_tol=0.0)]


@pytest.mark.parametrize("hw", [(24, 32), (37, 53)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("mode", MODES, ids=["no-filter", "defaults", "reach1-occluder2-size1", "reach4-occluder2", "reach1-size1-tol0"])
def test_lidar_depth_maps_are_the_definition(cuda, tiny, hw, mode):
    from mudg_amd import depth
    scene, _, _, obj_info, sweeps = tiny
    objects, clouds, tf, vis = _with_object_one(scene, obj_info, cuda)
    data = scene[0]["observers"]["camera_FRONT"]["data"]
    native = tuple(int(v) for v in data["hw"][0])
    xyz = [w[0] for w in _tiny_definition()[2]]
    want = ld.lidar_depth_maps(xyz, clouds, tf, vis, data["intr"], data["c2w"], native, hw, **mode)          # frames 0 and 3 clamp the window
    assert all((want[t] > 0).sum() > 50 for t in range(4))
    got = depth.lidar_depth_maps(sweeps, objects, data["intr"], data["c2w"], native, hw, **mode)
    _same(got, want, f"maps {hw} {mode}")
    assert torch.equal(depth.lidar_depth_maps(sweeps, objects, data["intr"], data["c2w"], native, hw, **mode), got)
    if mode == {}:
        off = ld.lidar_depth_maps(xyz, clouds, tf, vis, data["intr"], data["c2w"], native, hw, occlusion=False)
        assert (off != want).any()                                            # the filter does something here
        none = depth.lidar_depth_maps(sweeps, None, data["intr"][0], data["c2w"][[3, 0]], native, hw, frame_ids=[3, 0], window=(-1, 1))
        _same(none, ld.lidar_depth_maps(xyz, None, None, None, data["intr"][0], data["c2w"][[3, 0]], native, hw, frame_ids=[3, 0], window=(-1, 1)),
              "two frames out of order, no objects, a three-frame window")
        invisible = ld.lidar_depth_maps(xyz, clouds[:1], tf[:1], vis[:1], data["intr"][1], data["c2w"][1:2], native, hw, frame_ids=[1])
        assert np.array_equal(invisible[0], want[1])                          # object 1 adds nothing to the frame that does not track it


def test_native_size_and_the_hand_made_cases(cuda):
    """hw_out=None is the native size.  Frame 0: a dense far plane behind a near plane with every fourth column missing, and points whose
    home pixel is one pixel outside each border; frame 1 has no points at all: an empty window."""
    from mudg_amd import depth
    H, W, f = 40, 64, 50.0
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]])
    j, i = np.mgrid[0:H, 0:W]
    centre = lambda z, keep: np.stack([(i[keep] + 0.5 - W / 2.0) / f * z, (j[keep] + 0.5 - H / 2.0) / f * z, np.full(int(keep.sum()), z)], axis=1)
    rng = np.random.default_rng(5)
    outside = []
    for u, v in ([(-0.5, y) for y in rng.uniform(0, H, 12)] + [(W + 0.5, y) for y in rng.uniform(0, H, 12)] + [(x, -0.5) for x in rng.uniform(0, W, 12)]
                 + [(x, H + 0.5) for x in rng.uniform(0, W, 12)] + [(-0.5, -0.5), (W + 0.5, H + 0.5), (-0.5, H + 0.5), (W + 0.5, -0.5)]):
        z = rng.choice([5.0, 20.0, 40.0])
        outside.append([(u - W / 2.0) / f * z, (v - H / 2.0) / f * z, z])
    frames_xyz = [np.concatenate([centre(30.0, np.ones((H, W), bool)), centre(10.0, i % 4 != 3), np.array(outside)]).astype(F), np.zeros((0, 3), F)]
    sweeps = _sweeps(frames_xyz, cuda)
    c2w = np.stack([np.eye(4), np.eye(4)])
    for mode in (dict(point_size=1.0), dict(), dict(reach=16, point_size=3.0), dict(occlusion=False)):
        want = ld.lidar_depth_maps(frames_xyz, None, None, None, K, c2w, (H, W), window=(0, 0), **mode)
        got = depth.lidar_depth_maps(sweeps, None, K, c2w, (H, W), window=(0, 0), **mode)
        _same(got, want, f"planes, borders, empty window {mode}")
        assert not want[1].any() and (want[0] > 0).mean() > 0.7
    want = ld.lidar_depth_maps(frames_xyz, None, None, None, K, c2w, (H, W), window=(0, 0), point_size=1.0)[0]
    assert (want[1:-1, 7:W - 4:4] == 0).all() and (want[1:-1, 4:W - 4:4] == F(10.0)).all()          # nothing shows through the gaps


def test_a_plane_never_hides_its_own_points(cuda):
    from mudg_amd import depth
    xyz = cases.plane_points()
    sweeps = _sweeps([xyz], cuda)
    kw = dict(window=(0, 0), rel_tol=cases.PLANE_REL_TOL)
    off = depth.lidar_depth_maps(sweeps, None, cases.PLANE_K, np.eye(4)[None], cases.PLANE_HW, occlusion=False, **kw)
    cam = ld.sr.scaled_camera(cases.PLANE_K, cases.PLANE_HW, cases.PLANE_HW)
    _same(off[0], ld.lidar_depth(xyz, cases.IDENTITY, cam, *cases.PLANE_HW, occlusion=False), "the plane without the filter")
    assert float((off > 0).float().mean()) > 0.6
    for reach in cases.REACHES:
        on = depth.lidar_depth_maps(sweeps, None, cases.PLANE_K, np.eye(4)[None], cases.PLANE_HW, reach=reach, **kw)
        assert torch.equal(on, off), reach                                    # a hidden point would change a pixel or leave it empty


def test_the_filter_removes_what_shows_through_and_little_else(cuda):
    from mudg_amd import depth, render
    scenario, load_lidar, load_image = cases.leak_scene()
    scene = render.Scene.from_scenario(scenario, load_lidar, load_image, cases.LEAK_CAMERA, keep_sweeps=True, device=cuda)
    assert scene.objects is None and scene.hw_native == cases.LEAK_HW
    g, want_off, want_on = cases.leak_maps()
    row = [cases.LEAK_FRAME]
    off = depth.lidar_depth_maps(scene.sweeps, None, scene.intr[row], scene.c2w[row], scene.hw_native, frame_ids=row, occlusion=False)
    on = depth.lidar_depth_maps(scene.sweeps, None, scene.intr[row], scene.c2w[row], scene.hw_native, frame_ids=row)
    _same(off[0], want_off, "frame 5 without the filter")
    _same(on[0], want_on, "frame 5 with the filter")
    cases.leak_conditions(g, off[0].cpu().numpy(), on[0].cpu().numpy())


# ------------------------------------------------------------------------------------------------ the completion
SHAPES = [(1, 1, 1), (2, 7, 5), (3, 40, 67), (2, 70, 100)]                    # the last: three 32 x 32 tiles down, four across
DENSITIES = [0.0, "single", 0.05, 1.0]


def _labels(shape):
    rng = np.random.default_rng(shape[1] * 31 + shape[2])
    labels = rng.integers(0, 19, shape).astype(np.int64)
    labels[:, : max(shape[1] // 4, 1), shape[2] // 3:] = 10
    return labels


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("density", DENSITIES, ids=["none", "single", "sparse", "full"])
def test_complete_depth_is_the_definition(cuda, shape, density):
    from mudg_amd import depth
    d = cases.sparse_map(shape, density)
    if d.size >= 64:
        assert np.isnan(d).any() and np.isinf(d).any() and (d == F(0.1)).any() and (d > 100).any() and (d == F(99.9)).any()
    labels = _labels(shape)
    dev_d, dev_l = _dev(d, cuda), _dev(labels, cuda)
    for extrapolate in (True, False):
        for lab, dl in ((None, None), (labels, dev_l)):
            want, want_s = ld.complete_depth_frames(d, lab, extrapolate=extrapolate)
            got, got_s = depth.complete_depth(dev_d, dl, extrapolate=extrapolate, return_source=True)
            what = f"{shape} density {density} extrapolate {extrapolate} labels {lab is not None}"
            _same(got_s, want_s, "source, " + what)
            _same(got, want, "dense depth, " + what)
            assert torch.equal(depth.complete_depth(dev_d, dl, extrapolate=extrapolate), got)
    if density == 0.05 and shape[1] >= 40:
        assert set(np.unique(want_s)) >= {0, 1, 2, 4} and set(np.unique(ld.complete_depth_frames(d)[1])) == {1, 2, 3}
        other = depth.complete_depth(dev_d, dev_l, max_depth=60.0, sky_label=3, return_source=True)          # the other parameters reach the kernel
        want_o = ld.complete_depth_frames(d, labels, max_depth=60.0, sky_label=3)
        _same(other[1], want_o[1], "source, another range and sky label")
        _same(other[0], want_o[0], "dense depth, another range and sky label")


def test_the_31_x_31_fill_across_the_seams_of_the_row_pass(cuda):
    """The row pass of the 31 x 31 maximum works in segments of 256 columns with a 15-column halo, and the column scan in blocks of 256
    lanes: a map 600 wide has three of each.  The input has near returns within 15 columns of columns 256 and 512, and the definition
    is first shown to carry them across: cutting the map at a seam changes filled pixels on the other side of it."""
    from mudg_amd import depth
    d = cases.wide_map()
    want, want_s = ld.complete_depth_frames(d)
    for seam in cases.WIDE_SEAMS:
        left, right = d.copy(), d.copy()
        left[:, :, seam:] = 0
        right[:, :, :seam] = 0
        from_left, from_right = ld.complete_depth_frames(left)[0], ld.complete_depth_frames(right)[0]
        crossed_right = (from_left[:, :, seam:seam + 15] > 0) & (want_s[:, :, seam:seam + 15] == 3) & (from_left[:, :, seam:seam + 15] == want[:, :, seam:seam + 15])
        crossed_left = (from_right[:, :, seam - 15:seam] > 0) & (want_s[:, :, seam - 15:seam] == 3) & (from_right[:, :, seam - 15:seam] == want[:, :, seam - 15:seam])
        print(f"seam {seam}: {int(crossed_right.sum())} pixels right of it filled from its left, {int(crossed_left.sum())} left of it from its right")
        assert crossed_right.sum() > 20 and crossed_left.sum() > 20, seam
    assert (want_s == 3).mean() > 0.3 and (want[0, 40:] > 0).mean() < 0.9                 # the extension does the most here; the bottom of frame 0 stays open
    got, got_s = depth.complete_depth(_dev(d, cuda), return_source=True)
    _same(got_s, want_s, "source, three segments of the row pass")
    _same(got, want, "dense depth, three segments of the row pass")
    assert torch.equal(depth.complete_depth(_dev(d, cuda)), got)
    closed = depth.complete_depth(_dev(d, cuda), extrapolate=False, return_source=True)
    want_c = ld.complete_depth_frames(d, extrapolate=False)
    _same(closed[1], want_c[1], "source, wide and closed only")
    _same(closed[0], want_c[0], "dense depth, wide and closed only")


def test_a_base_that_is_not_16_byte_aligned(cuda):
    from mudg_amd import depth
    shape = (3, 40, 67)
    d = cases.sparse_map(shape, 0.05)
    flat = torch.zeros(d.size + 8, dtype=torch.float32, device=cuda)
    assert flat.data_ptr() % 16 == 0
    view = flat[1:1 + d.size].view(shape)
    view.copy_(_dev(d, cuda))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    want, want_s = ld.complete_depth_frames(d)
    got, got_s = depth.complete_depth(view, return_source=True)
    _same(got_s, want_s, "source, unaligned depth")
    _same(got, want, "dense depth, unaligned depth")


def test_constant_maps_stay_constant(cuda):
    from mudg_amd import depth
    d = cases.constant_map()
    out, source = depth.complete_depth(_dev(d, cuda), return_source=True)
    assert bool((out == 12.5).all()) and torch.equal(source == 1, _dev(d, cuda) > 0)
    out = depth.complete_depth(_dev(d, cuda), extrapolate=False)
    assert set(out.unique().tolist()) == {0.0, 12.5}
    _same(out, ld.complete_depth_frames(d, extrapolate=False)[0], "the constant map, closed only")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(cuda, tiny):
    from mudg_amd import depth, hip, ops
    scene, _, _, obj_info, sweeps = tiny
    data = scene[0]["observers"]["camera_FRONT"]["data"]
    args = (sweeps, None, data["intr"], data["c2w"], (320, 480), (24, 32))
    for bad in (dict(reach=0), dict(reach=17), dict(reach=2.5), dict(rel_tol=-0.01), dict(rel_tol=1.0), dict(rel_tol=float("nan")),
                dict(window=(-4, 4)), dict(window=(1, 0)), dict(frame_ids=[0, 1, 2]), dict(frame_ids=[0, 1, 2, 4])):
        with pytest.raises(hip.MudgError):
            depth.lidar_depth_maps(*args, **bad)
    with pytest.raises(hip.MudgError):
        depth.lidar_depth_maps(sweeps, None, data["intr"][:3], data["c2w"], (320, 480))            # three intrinsics, four cameras
    with pytest.raises(hip.MudgError):
        depth.lidar_depth_maps(sweeps, None, data["intr"], data["c2w"][:, :3], (320, 480))
    with pytest.raises(hip.MudgError):
        depth.lidar_depth_maps(sweeps.points, None, data["intr"], data["c2w"], (320, 480))         # a tensor is not a FrameSweeps
    keys = ops.splat_keys(1, 8, 8, cuda)[0]
    mats = torch.zeros((1, 12), device=cuda)
    for bad in (dict(segments=[]), dict(segments=[(0, 1)] * 9), dict(segments=[(0, len(sweeps.points) + 1)]), dict(segments=[(0, 0)]),
                dict(occluder_keys=keys.cpu()), dict(occluder_keys=ops.splat_keys(1, 8, 9, cuda)[0]), dict(occluder_keys=keys.clone(), reach=17),
                dict(occluder_keys=keys.clone(), rel_tol=1.0)):
        kw = dict(dict(segments=[(0, 10)]), **bad)
        with pytest.raises(hip.MudgError):
            ops.lidar_splat_visible(sweeps.points, kw.pop("segments"), mats, keys, (10.0, 10.0, 4.0, 4.0), 2.0, **kw)
    assert bool((keys == -1).all())                                           # nothing was launched
    d = torch.zeros((2, 8, 8), device=cuda)
    for call in (lambda: depth.complete_depth(d.cpu()), lambda: depth.complete_depth(d[0]), lambda: depth.complete_depth(d.double()),
                 lambda: depth.complete_depth(d, torch.zeros((2, 8, 9), dtype=torch.int64, device=cuda)),
                 lambda: depth.complete_depth(d, torch.zeros((2, 8, 8), dtype=torch.int64)),
                 lambda: depth.complete_depth(d, max_depth=0.05), lambda: depth.complete_depth(d, max_depth=1e6)):
        with pytest.raises(hip.MudgError):
            call()
    assert hip.lib().mudg_depth_complete_scratch(0, 8, 8) == -1 and hip.lib().mudg_depth_complete_scratch(2, 8, 8) >= 2 * 8 * 8 * 9


# ------------------------------------------------------------------------------------------------ end to end
def test_sweeps_to_depth_labels_to_normals_to_clips(cuda):
    from mudg_amd import depth, frames, hip, ops, render
    from mudg_amd.synthetic import street_sweeps
    scenario, load_lidar, load_image = street_sweeps(frames=6)
    scene = render.Scene.from_scenario(scenario, load_lidar, load_image, keep_sweeps=True, device=cuda)
    assert scene.objects is not None and scene.sweeps.frames == 6
    native, L, hw = scene.hw_native, 4, (64, 64)
    lidar, dense, source = depth.depth_labels_from_lidar(scene, range(6))
    assert lidar.shape == dense.shape == source.shape == (6,) + native and lidar.dtype == dense.dtype == torch.float32 and source.dtype == torch.uint8
    assert torch.equal(lidar, depth.lidar_depth_maps(scene.sweeps, scene.objects, scene.intr, scene.c2w, native))
    assert torch.equal(dense, depth.complete_depth(lidar))
    covered = float((lidar > 0).float().mean())
    print(f"covered by returns {covered:.3f}, dense {float((dense > 0).float().mean()):.3f}")
    assert 0.1 < covered < 0.9 and float((dense > 0).float().mean()) > 0.8 and bool((dense[lidar > 0.1] > 0).all())
    assert bool(((source == 1) == (lidar > 0.1)).all()) and bool(((source > 0) == (dense > 0)).all())
    again = depth.depth_labels_from_lidar(scene, [4, 1], hw_out=(80, 120), reach=2, extrapolate=False)
    assert again[1].shape == (2, 80, 120) and bool((again[1] == 0).any())
    with pytest.raises(hip.MudgError, match="keep_sweeps"):
        depth.depth_labels_from_lidar(render.Scene.from_scenario(scenario, load_lidar, load_image, device=cuda), range(6))
    images = _dev(np.stack([load_image("camera_FRONT", f) for f in range(6)]), cuda)
    normals, valid = depth.normals_from_depth(dense, scene.intr, native, max_rel_step=0.05)
    assert float(valid.float().mean()) > 0.7
    sf = frames.SceneFrames(images, depth=dense, normals=normals)
    item = frames.SceneClips(scene, sf, hw, video_length=L, train_labels=("color", "depth")).__getitem__(1, label="depth")
    assert item["dense_frames"].shape == item["sparse_frames"].shape == item["sparse_depth"].shape == (3, L) + hw and item["class_label"].tolist() == [500]
    assert torch.equal(item["dense_frames"], frames.stream_from_depth(dense[1:1 + L], hw))
    item = frames.SceneClips(scene, sf, hw, video_length=L, train_labels=("color", "normal")).__getitem__(2, label="normal")
    assert item["dense_frames"].shape == (3, L) + hw and item["class_label"].tolist() == [1000]
    u8 = ops.frames_to_uint8(frames.stream_from_depth(dense, native)[None])[0]
    fit = depth.metric_depth(u8, lidar)
    assert fit["fitted"].tolist() == [1] * 6 and fit["depth"].shape == lidar.shape
