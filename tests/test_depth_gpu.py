"""Metric depth and lifted views on the GPU (csrc/depth.hip through mudg_amd/depth.py, virtual_render/eval_tools.py and
virtual_render/virtual_pose_render.py) against the CPU definition of the rules (tests/depth_reference.py): torch.equal everywhere — the
sums are integers and both sides perform the same correctly rounded operations in the same order, so there is no tolerance."""
import numpy as np
import pytest
import torch

import depth_reference as dr
from helpers import cfgs, golden

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
SIZES = [(24, 32), (23, 29)]                     # the four-pixel form; the one-pixel form with a row tail


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _streams(hw, seed, frames=3):
    """Seeded depth frames, LiDAR depths (about a third of the pixels without a return, some beyond the counted range) and labels."""
    rng = np.random.default_rng(seed)
    H, W = hw
    u8 = rng.integers(0, 256, (frames, H, W, 3), dtype=np.uint8)
    u8[0, 1, :5] = 0                                                           # black pixels: not counted
    lidar = (90.0 * dr.k_of(u8) / 765.0 + 3.0 + rng.normal(0, 1.0, (frames, H, W))).astype(F)
    lidar[rng.random((frames, H, W)) < 0.3] = 0.0
    lidar[1, 2, :4] = F([256.0, 255.99, -3.0, 2.0 ** -21])
    lidar[2] *= F(0.1)                                                         # a frame whose line leaves [0, 100] nowhere
    lidar[0] *= F(1.3)                                                         # and one whose line passes 100 m above u = 0.83
    labels = rng.integers(0, 19, (frames, H, W)).astype(np.int64)
    labels[:, :4, 3:11] = 10
    return u8, lidar, labels


@pytest.fixture(scope="module")
def cases():
    """The inputs of every size with the definition's outputs, computed once and left unchanged."""
    out = {}
    for n, hw in enumerate(SIZES):
        u8, lidar, labels = _streams(hw, 40 + n)
        out[hw] = {"u8": u8, "lidar": lidar, "labels": labels, "sky": dr.metric_depth(u8, lidar, labels), "plain": dr.metric_depth(u8, lidar)}
    return out


def _assert_metric(got, want, what, vis=True):
    pairs = [("coef", want["coef"]), ("fitted", want["fitted"]), ("depth", want["depth"])] + ([("vis", want["vis"])] if vis else [])
    for name, w in pairs:
        w, g = _t(w), got[name].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        differ = int((g != w).sum())
        print(f"{what}: {name}: {differ} of {w.numel()} values differ")
        assert torch.equal(g, w), (what, name, differ)


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("sky", [True, False])
def test_metric_depth_is_bit_equal_to_the_cpu_definition(cuda, cases, hw, sky):
    from mudg_amd import depth, ops
    c = cases[hw]
    want = c["sky" if sky else "plain"]
    u8, lidar = _t(c["u8"]).to(cuda), _t(c["lidar"]).to(cuda)
    labels = _t(c["labels"]).to(cuda) if sky else None
    sums = ops.depth_align_sums(u8, lidar)
    assert sums.dtype == torch.int64 and sums.shape == (3, 5) and sums.cpu().tolist() == [list(s) for s in want["sums"]]
    got = depth.metric_depth(u8, lidar, labels, visualise=True)
    assert set(got) == {"depth", "coef", "fitted", "vis"} and want["fitted"].tolist() == [1, 1, 1]
    _assert_metric(got, want, f"{hw} sky={sky}")
    # the fixture exercises what it is meant to: the clip at 100 m, a frame that is never clipped (before the sky rule), the sky
    assert (c["plain"]["depth"][0] == 100).any() and c["plain"]["depth"][2].max() < 100 and float(got["depth"].min()) >= 0
    assert bool((got["depth"][:, :4, 3:11] == 100).all()) == sky
    again = depth.metric_depth(u8, lidar, labels, visualise=True)             # two runs: the same bits
    for name in got:
        assert torch.equal(got[name], again[name]), name
    assert torch.equal(ops.depth_align_sums(u8, lidar), sums)
    plain = depth.metric_depth(u8, lidar, labels)
    assert set(plain) == {"depth", "coef", "fitted"} and torch.equal(plain["depth"], got["depth"])


def test_unaligned_bases_take_the_one_pixel_form_and_give_the_same_bits(cuda, cases):
    from mudg_amd import ops
    c = cases[(24, 32)]
    want = c["sky"]
    shift = lambda a, pad: torch.cat([torch.zeros(pad, dtype=_t(a).dtype), _t(a).reshape(-1)]).to(cuda)[pad:].view(a.shape)
    u8, lidar, labels = shift(c["u8"], 1), shift(c["lidar"], 1), shift(c["labels"], 1)
    assert u8.data_ptr() % 4 and lidar.data_ptr() % 16 and labels.data_ptr() % 16 and u8.is_contiguous()
    sums = ops.depth_align_sums(u8, lidar)
    assert sums.cpu().tolist() == [list(s) for s in want["sums"]]
    coef, fitted = ops.depth_align_solve(sums)
    depth, vis = ops.depth_finish(u8, coef, labels, visualise=True)
    _assert_metric({"coef": coef, "fitted": fitted, "depth": depth, "vis": vis}, want, "unaligned")


@pytest.mark.parametrize("hw", SIZES)
def test_frames_that_cannot_be_fitted_keep_the_streams_own_scale(cuda, hw):
    """A single counted pixel; every k equal; no LiDAR return at all: fitted = 0 and (m, c) = (100, 0), so depth = 100 k / 765."""
    from mudg_amd import depth
    rng = np.random.default_rng(9)
    H, W = hw
    u8 = rng.integers(1, 256, (3, H, W, 3), dtype=np.uint8)
    lidar = rng.uniform(1, 80, (3, H, W)).astype(F)
    lidar[0] = 0
    lidar[0, H - 1, W - 1] = 12.5                                              # the last pixel of the row tail
    u8[1] = (10, 20, 30)
    lidar[2] = 0
    want = dr.metric_depth(u8, lidar)
    assert [s[0] for s in want["sums"]] == [1, H * W, 0] and want["fitted"].tolist() == [0, 0, 0]
    assert np.array_equal(want["coef"], [[100.0, 0.0]] * 3)
    got = depth.metric_depth(_t(u8).to(cuda), _t(lidar).to(cuda), visualise=True)
    _assert_metric(got, want, f"unfitted {hw}")
    assert torch.equal(got["depth"][1].cpu(), torch.full((H, W), float(F(D(100.0) * (D(60) / D(765.0))))))


def test_the_sums_have_headroom_at_the_full_frame_size(cuda):
    """One 576 x 1024 frame with every k = 765 and every LiDAR depth 255.99 m: the five sums equal the Python integers."""
    from mudg_amd import ops
    H, W = 576, 1024
    u8 = torch.full((1, H, W, 3), 255, dtype=torch.uint8, device=cuda)
    lidar = torch.full((1, H, W), 255.99, dtype=torch.float32, device=cuda)
    q = int(dr.q_of(F([255.99]))[0])
    n = H * W
    want = [n, n * 765, n * 765 * 765, n * q, n * 765 * q]
    assert 2 ** 56 < want[4] < 2 ** 63
    sums = ops.depth_align_sums(u8, lidar)
    assert sums.cpu().tolist() == [want]
    assert torch.equal(ops.depth_align_sums(u8, lidar), sums)
    coef, fitted = ops.depth_align_solve(sums)                                 # no spread in k: not fitted
    assert fitted.cpu().tolist() == [0] and coef.cpu().tolist() == [[100.0, 0.0]]


def test_the_colour_map_is_bit_equal_to_the_definition_and_to_the_reference(cuda):
    from mudg_amd import ops
    from virtual_render import eval_tools
    g = golden("depth_post.pt")
    x, metres = g["cm_in"], g["vd_in"]
    lo, hi = (float(v) for v in g["vd_range"])
    for reverse, tag in ((False, "cm"), (True, "cm_r")):
        b = ops.colormap_spectral(x.to(cuda), reversed=reverse)
        f = ops.colormap_spectral(x.to(cuda), reversed=reverse, bytes=False)
        assert b.dtype == torch.uint8 and f.dtype == torch.float32 and b.shape == (3, 24, 32, 3)
        assert torch.equal(b.cpu(), g[tag + "_bytes"]) and torch.equal(f.cpu().view(torch.int32), g[tag + "_floats"].view(torch.int32)), tag
        assert torch.equal(b.cpu(), _t(dr.colormap(x.numpy(), reversed=reverse)))
        assert torch.equal(ops.colormap_spectral(x.to(cuda), reversed=reverse), b)
    ranged = ops.colormap_spectral(metres.to(cuda), lo, hi)                    # val_min / val_max other than (0, 1)
    assert torch.equal(ranged.cpu(), g["vd_bytes"]) and torch.equal(ranged.cpu(), _t(dr.colormap(metres.numpy(), lo, hi)))
    odd = ops.colormap_spectral(metres.to(cuda), 0.1, 37.3, bytes=False)       # bounds that are not fp32 numbers
    assert torch.equal(odd.cpu().view(torch.int32), _t(dr.colormap(metres.numpy(), 0.1, 37.3, bytes=False)).view(torch.int32))
    # the reference's signatures: tensors stay on the GPU, arrays come back as arrays, visualize_depth returns a list of arrays
    assert torch.equal(eval_tools.colormap(x.to(cuda), bytes=True).cpu(), g["cm_bytes"]) and eval_tools.colormap(x.to(cuda)).dtype == torch.float32
    assert np.array_equal(eval_tools.colormap(x.numpy(), cmap="Spectral_r", bytes=True), g["cm_r_bytes"].numpy())
    pictures = eval_tools.visualize_depth(metres.numpy(), val_min=lo, val_max=hi)
    assert isinstance(pictures, list) and len(pictures) == 2 and pictures[0].dtype == np.uint8 and pictures[0].shape == (24, 32, 3)
    assert np.array_equal(np.stack(pictures), g["vd_bytes"].numpy())
    assert np.array_equal(eval_tools.visualize_depth(x.numpy()[0])[0], g["vd_default"].numpy()[0])            # a single (H, W) map
    levels = torch.arange(256, dtype=torch.uint8)                              # uint8 means value / 255
    assert torch.equal(eval_tools.colormap(levels.to(cuda), bytes=True).cpu(), _t(dr.colormap((levels.float() / 255).numpy())))


def _camera(k):
    a = 0.4 + 0.3 * k
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    c2w = np.eye(4)
    c2w[:3, :3] = rz @ np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    c2w[:3, 3] = [30.0 + 7 * k, -20.0 + 3 * k, 1.5 + k]
    intr = np.array([[800.0 + 10 * k, 0, 640.0 + k], [0, 820.0 - 5 * k, 480.0 - k], [0, 0, 1]])
    return c2w, intr


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("sky", [True, False])
def test_lifted_views_are_bit_equal_to_the_cpu_definition(cuda, cases, hw, sky):
    """Three frames, each with its own pose and intrinsics; depths at and beyond both bounds."""
    from mudg_amd import depth, ops, render
    c = cases[hw]
    z = c["plain"]["depth"].copy()                                             # no 100 m on the sky pixels: the label rule itself decides
    z[0, 0, :3] = F([0.0, 100.0, 2.0 ** -30])
    rgb, labels = c["u8"], (c["labels"] if sky else None)
    c2w, intr = (np.stack(v) for v in zip(*(_camera(k) for k in range(3))))
    table = depth.camera_table(intr, c2w, (960, 1280), hw)
    assert len({tuple(r) for r in table}) == 3
    want = [dr.unproject(z[t], rgb[t], table[t], None if labels is None else labels[t]) for t in range(3)]
    want_p, want_v = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    assert 0 < want_v.sum() < want_v.size and want_v[:2].tolist() == [0, 0] and want_v[2] == (0 if sky and labels[0, 0, 2] == 10 else 1)
    dev = lambda a: None if a is None else _t(a).to(cuda)
    points, valid = ops.depth_unproject(dev(z), dev(rgb), dev(table), dev(labels))
    assert points.dtype == torch.int32 and points.shape == (3 * hw[0] * hw[1], 4) and valid.dtype == torch.uint8
    print(f"{hw} sky={sky}: {int((points.cpu() != _t(want_p)).sum())} point words and {int((valid.cpu() != _t(want_v)).sum())} flags differ")
    assert torch.equal(valid.cpu(), _t(want_v)) and torch.equal(points.cpu(), _t(want_p))
    cloud = depth.lift_views(dev(z), dev(rgb), intr, c2w, (960, 1280), dev(labels))
    assert isinstance(cloud, render.PointCloud) and len(cloud) == int(want_v.sum())
    assert torch.equal(cloud.points.cpu(), _t(want_p[want_v == 1]))
    assert torch.equal(depth.lift_views(dev(z), dev(rgb), intr, c2w, (960, 1280), dev(labels)).points, cloud.points)
    near = depth.lift_views(dev(z), dev(rgb), intr, c2w, (960, 1280), dev(labels), min_depth=20.0, max_depth=60.0)
    keep = dr.unproject(z[0], rgb[0], table[0], None if labels is None else labels[0], min_depth=20.0, max_depth=60.0)[1]
    assert 0 < len(near) < len(cloud) and torch.equal(near.points[:int(keep.sum())].cpu(), _t(want[0][0][keep == 1]))


def test_concatenated_is_the_byte_concatenation(cuda):
    from mudg_amd import render
    rng = np.random.default_rng(2)
    a = render.PointCloud.from_arrays(rng.normal(0, 10, (50, 3)), rng.integers(0, 256, (50, 3), dtype=np.uint8), cuda)
    b = render.PointCloud.from_arrays(rng.normal(0, 10, (7, 3)), rng.integers(0, 256, (7, 3), dtype=np.uint8), cuda)
    both = render.PointCloud.concatenated(a, b, a)
    assert isinstance(both, render.PointCloud) and len(both) == 107
    assert both.points.cpu().numpy().tobytes() == a.points.cpu().numpy().tobytes() + b.points.cpu().numpy().tobytes() + a.points.cpu().numpy().tobytes()
    assert torch.equal(render.PointCloud.concatenated(a).points, a.points)


def test_wrappers_check_their_arguments(cuda):
    from mudg_amd import hip, ops
    u8 = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=cuda)
    with pytest.raises(hip.MudgError, match="lidar"):
        ops.depth_align_sums(u8, torch.zeros(2, 8, 4, device=cuda))
    with pytest.raises(hip.MudgError, match="coef"):
        ops.depth_finish(u8, torch.zeros(3, 2, dtype=torch.float64, device=cuda))
    with pytest.raises(hip.MudgError, match="labels"):
        ops.depth_finish(u8, torch.zeros(2, 2, dtype=torch.float64, device=cuda), torch.zeros(2, 8, 8, dtype=torch.int32, device=cuda))
    with pytest.raises(hip.MudgError, match="range"):
        ops.colormap_spectral(torch.zeros(4, device=cuda), 1.0, 1.0)
    with pytest.raises(hip.MudgError, match="table"):
        ops.depth_unproject(torch.zeros(2, 8, 8, device=cuda), u8, torch.zeros(2, 12, dtype=torch.float64, device=cuda))


def test_a_generated_window_becomes_metric_depth_and_points_that_render_again(cuda):
    """render_windows -> synthesize_windows -> window_outputs -> lift_views -> render_conditions on the lifted cloud, on the tiny driver
    model (4 frames of 64 x 64, 2 DDIM steps).  The metric outputs are the definition's of the generated frames; the rest is shapes,
    dtypes and finiteness."""
    from mudg_amd import depth, ops, render
    from mudg_amd.synthetic import street_scene
    from test_splat_gpu import _driver_model, _upload
    from virtual_render.virtual_pose_render import render_windows, synthesize_windows, window_outputs
    small = street_scene(n_background=150_000, frames=4, seed=5, n_objects=3, object_points=3000)
    model, g = _driver_model(cuda)
    shp, px = g["shape"], g["driver"]["pixels"]
    L = shp["T"]
    assert L == 4
    bg, objects = _upload(small, cuda)
    scene = render.Scene(bg, objects, small["intr"], small["c2w"], small["hw_native"])
    dense = (torch.rand(3, 3, L, px, px, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(cuda)
    wins = list(render_windows(scene, dense, pose=1, video_length=L))
    assert len(wins) == 1
    sm = cfgs.SAMPLER
    samples = synthesize_windows(model, wins, [3, 4, L, shp["H"], shp["W"]], video_length=L, ddim_steps=2, ddim_eta=1.0,
                                 unconditional_guidance_scale=sm["cfg_scale"], fs=sm["fs"], timestep_spacing=sm["spacing"],
                                 guidance_rescale=sm["guidance_rescale"])[0]
    cams = np.stack([render.virtual_poses(c, with_ori_pose=True)[1] for c in small["c2w"]])
    cond = render.render_conditions(bg, objects, small["intr"], small["c2w"], small["hw_native"], (px, px), poses=cams[:, None], return_images=True)
    out = window_outputs(samples, cond)
    assert set(out) == {"color", "semantic_labels", "semantic", "depth", "depth_vis", "coef", "fitted"}
    for name, dtype, shape in (("color", torch.uint8, (L, px, px, 3)), ("semantic_labels", torch.int64, (L, px, px)), ("semantic", torch.uint8, (L, px, px, 3)),
                               ("depth", torch.float32, (L, px, px)), ("depth_vis", torch.uint8, (L, px, px, 3)), ("coef", torch.float64, (L, 2)),
                               ("fitted", torch.uint8, (L,))):
        assert out[name].dtype == dtype and tuple(out[name].shape) == shape and out[name].is_cuda, name
    assert torch.isfinite(out["depth"]).all() and torch.isfinite(out["coef"]).all()
    assert float(out["depth"].min()) >= 0 and float(out["depth"].max()) <= 100 and int(out["semantic_labels"].min()) >= 0 and int(out["semantic_labels"].max()) < 19
    u8 = ops.frames_to_uint8(samples[:, 0])
    assert torch.equal(out["color"], u8[0])
    want = dr.metric_depth(u8[1].cpu().numpy(), cond["depth"][0].cpu().numpy(), out["semantic_labels"].cpu().numpy())
    _assert_metric({"coef": out["coef"], "fitted": out["fitted"], "depth": out["depth"], "vis": out["depth_vis"]}, want, "window")
    # fitted wherever the rendered depth and the generated frame share two pixels with a spread in k (integers: exact)
    assert int((cond["depth"][0] > 0).flatten(1).sum(1).min()) >= 2                                          # something was rendered in every frame
    assert out["fitted"].cpu().tolist() == [int(n >= 2 and n * skk > sk * sk) for n, sk, skk, _, _ in want["sums"]], want["sums"]
    cloud = depth.lift_views(out["depth"], out["color"], small["intr"], cams, small["hw_native"], out["semantic_labels"])
    assert 0 < len(cloud) <= L * px * px and cloud.points.dtype == torch.int32 and torch.isfinite(cloud.points[:, :3].contiguous().view(torch.float32)).all()
    merged = render.PointCloud.concatenated(bg, cloud)
    assert len(merged) == len(bg) + len(cloud)
    again = render.render_conditions(cloud, None, small["intr"], small["c2w"], small["hw_native"], (px, px), poses=cams[:, None], return_images=True)
    assert again["sparse_frames"].shape == (1, 3, L, px, px) and again["sparse_frames"].dtype == torch.float32
    assert torch.isfinite(again["sparse_frames"]).all() and torch.isfinite(again["sparse_depth"]).all()
    assert bool((again["depth"] > 0).any()) and float(again["depth"].max()) < render.ZFAR                   # a lifted point lands in the view it came from
