"""The scores of generated views on the GPU (csrc/metrics.hip through mudg_amd/ops.py, mudg_amd/metrics.py and
virtual_render/eval_tools.py) against the CPU definition of the rules (tests/metrics_reference.py): torch.equal on every kernel output
and between two runs — the sums are integers and both sides perform the same correctly rounded operations in the same order, so there
is no tolerance.  The float64 scores formed from the integers are compared bit for bit too, except the PSNR (a logarithm: 1e-14)
and the mean IoU (a float64 sum in the library's order: its rounding bound)."""
import numpy as np
import pytest
import torch

import metrics_reference as mr
from helpers import cfgs

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
# one valid pixel; a small one; the one-pixel form with a row tail; the four-pixel form; one row and one column more than two of the SSIM
# kernel's 32 x 32 tiles in each direction (valid region 65 x 65: aprons cross tile boundaries)
SIZES = [(11, 11), (12, 13), (23, 29), (24, 32), (75, 75)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _pair(hw, seed, frames=3):
    """Seeded frames, different per frame: noise against a copy with noise of a strength that grows with the frame."""
    rng = np.random.default_rng(seed)
    H, W = hw
    a = rng.integers(0, 256, (frames, H, W, 3), dtype=np.uint8)
    b = np.stack([np.clip(np.rint(a[f] + rng.normal(0, 4.0 + 20.0 * f, (H, W, 3))), 0, 255).astype(np.uint8) for f in range(frames)])
    return a, b


@pytest.fixture(scope="module")
def colour_cases():
    """The inputs of every size with the definition's outputs, computed once and left unchanged."""
    out = {}
    for n, hw in enumerate(SIZES):
        a, b = _pair(hw, 60 + n)
        out[hw] = {"a": a, "b": b, "want": mr.psnr_ssim(a, b)}
    return out


def _assert_colour(got, want, what):
    assert set(got) == {"psnr", "ssim", "sse", "ssim_sum"}
    for name in ("sse", "ssim_sum", "ssim"):
        w, g = _t(want[name]), got[name].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        print(f"{what}: {name}: got {g.tolist()}, definition {w.tolist()}")
        assert torch.equal(g, w), (what, name)
    assert got["psnr"].dtype == torch.float64
    assert torch.allclose(got["psnr"].cpu(), _t(want["psnr"]), rtol=1e-14, atol=0), what


@pytest.mark.parametrize("hw", SIZES)
def test_psnr_and_ssim_are_bit_equal_to_the_cpu_definition(cuda, colour_cases, hw):
    from mudg_amd import metrics, ops
    c = colour_cases[hw]
    a, b = _t(c["a"]).to(cuda), _t(c["b"]).to(cuda)
    got = metrics.psnr_ssim(a, b)
    _assert_colour(got, c["want"], f"{hw}")
    assert len(set(c["want"]["sse"].tolist())) == 3 and len(set(c["want"]["ssim_sum"].tolist())) == 3       # F = 3, different per frame
    assert all(g.is_cuda for g in got.values())
    again = metrics.psnr_ssim(a, b)                                            # two runs: the same bits
    for name in got:
        assert torch.equal(got[name], again[name]), name
    assert torch.equal(ops.metric_sse(b, a), got["sse"]) and torch.equal(ops.metric_ssim(b, a), got["ssim_sum"])   # symmetric rules
    if hw == (75, 75):
        assert ops.SSIM_TILE == 32 and hw[0] - 10 == 2 * ops.SSIM_TILE + 1


@pytest.mark.parametrize("hw", [(24, 32), (75, 75)])
def test_unaligned_bases_take_the_one_pixel_form_and_give_the_same_bits(cuda, colour_cases, hw):
    from mudg_amd import metrics
    c = colour_cases[hw]
    shift = lambda v: torch.cat([torch.zeros(1, dtype=torch.uint8), _t(v).reshape(-1)]).to(cuda)[1:].view(v.shape)
    a, b = shift(c["a"]), shift(c["b"])
    assert a.data_ptr() % 4 and b.data_ptr() % 4 and a.is_contiguous()
    _assert_colour(metrics.psnr_ssim(a, b), c["want"], f"unaligned {hw}")


@pytest.mark.parametrize("hw", [(11, 11), (23, 29), (24, 32), (75, 75)])
def test_identical_and_constant_frames_score_their_exactly_known_values(cuda, colour_cases, hw):
    from mudg_amd import metrics
    H, W = hw
    n = 3 * (H - 10) * (W - 10)
    a = _t(colour_cases[hw]["a"]).to(cuda)
    same = metrics.psnr_ssim(a, a.clone())
    assert same["sse"].cpu().tolist() == [0] * 3 and same["ssim_sum"].cpu().tolist() == [n * 2 ** 32] * 3
    assert same["ssim"].cpu().tolist() == [1.0] * 3 and bool(torch.isinf(same["psnr"]).all()) and bool((same["psnr"] > 0).all())
    values = [(255, 0), (200, 100), (1, 2)]
    x = torch.stack([torch.full((H, W, 3), v[0], dtype=torch.uint8) for v in values]).to(cuda)
    y = torch.stack([torch.full((H, W, 3), v[1], dtype=torch.uint8) for v in values]).to(cuda)
    got = metrics.psnr_ssim(x, y)
    for f, (va, vb) in enumerate(values):
        mx, my = D(va), D(vb)
        s = ((2.0 * (mx * my) + mr.C1) * (2.0 * 0.0 + mr.C2)) / (((mx * mx + my * my) + mr.C1) * ((0.0 + 0.0) + mr.C2))
        assert int(got["ssim_sum"][f]) == n * int(np.rint(s * 2.0 ** 32)), (va, vb)
        assert int(got["sse"][f]) == 3 * H * W * (va - vb) ** 2


def test_the_colour_sums_have_headroom_at_the_full_frame_size(cuda):
    """One 576 x 1024 pair at the extremes: all 255 against all 0 (the largest squared error, the smallest SSIM of constant frames) and
    all 255 against itself (every q = 2^32)."""
    from mudg_amd import metrics
    H, W = 576, 1024
    n = 3 * (H - 10) * (W - 10)
    white = torch.full((1, H, W, 3), 255, dtype=torch.uint8, device=cuda)
    black = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=cuda)
    s = ((2.0 * (D(255) * D(0)) + mr.C1) * (2.0 * 0.0 + mr.C2)) / (((D(255) * D(255) + D(0) * D(0)) + mr.C1) * ((0.0 + 0.0) + mr.C2))
    got = metrics.psnr_ssim(white, black)
    assert got["sse"].cpu().tolist() == [3 * H * W * 65025] and got["ssim_sum"].cpu().tolist() == [n * int(np.rint(s * 2.0 ** 32))]
    assert float(got["psnr"][0]) == 0.0
    same = metrics.psnr_ssim(white, white.clone())
    assert same["sse"].cpu().tolist() == [0] and same["ssim_sum"].cpu().tolist() == [n * 2 ** 32] and n * 2 ** 32 > 2 ** 52
    assert same["ssim"].cpu().tolist() == [1.0]
    assert torch.equal(metrics.psnr_ssim(white, black)["ssim_sum"], got["ssim_sum"])


# ------------------------------------------------------------------------------------------------ depth
def _assert_depth(got, want, what):
    assert set(got) == {"n", "mae", "rmse", "abs_rel", "d1", "d2", "d3", "sums"}
    print(f"{what}: sums {got['sums'].cpu().tolist()}, definition {want['sums'].tolist()}")
    assert got["sums"].dtype == torch.int64 and torch.equal(got["sums"].cpu(), _t(want["sums"])), what
    assert torch.equal(got["n"].cpu(), _t(want["n"]))
    for name in ("mae", "rmse", "abs_rel", "d1", "d2", "d3"):
        g, w = got[name].cpu(), _t(want[name])
        assert g.dtype == torch.float64 and torch.equal(torch.isnan(g), torch.isnan(w)), (what, name)
        assert torch.equal(torch.nan_to_num(g, nan=-1.0), torch.nan_to_num(w, nan=-1.0)), (what, name, g.tolist(), w.tolist())


def test_depth_errors_of_the_small_case_are_bit_equal_to_the_cpu_definition(cuda):
    from mudg_amd import metrics
    from test_metrics_cpu import _depth_case
    z, y = _depth_case()
    want = mr.depth_errors(z[None], y[None])
    assert tuple(want["sums"][0].tolist()) == mr.depth_sums_exact(z, y)
    got = metrics.depth_errors(_t(z[None]).to(cuda), _t(y[None]).to(cuda))
    _assert_depth(got, want, "5 x 7")
    assert int(got["sums"][0, 7]) == 0 and int(got["n"][0]) == 29


@pytest.mark.parametrize("hw", [(23, 29), (24, 32)])
def test_depth_errors_are_bit_equal_to_the_cpu_definition(cuda, hw):
    """Three frames: about 15 % empty LiDAR pixels; a frame with no counted pixel (n = 0, nan scores); depths that are zero, negative,
    beyond 256 m, infinite and not numbers."""
    from mudg_amd import metrics, ops
    rng = np.random.default_rng(21)
    H, W = hw
    y = rng.uniform(0.5, 79.0, (3, H, W)).astype(F)
    z = (y * rng.uniform(0.6, 1.7, (3, H, W))).astype(F)
    y[rng.random((3, H, W)) < 0.15] = 0.0
    y[1] = 0.0                                                                 # nothing counted
    y[1, 0, :3] = F([0.05, 80.0, 90.0])
    z[0, 1, :6] = F([0.0, -3.0, 300.0, np.inf, -np.inf, np.nan])
    y[0, 1, :6] = 10.0
    want = mr.depth_errors(z, y)
    assert want["n"][1] == 0 and np.isnan(want["mae"][1]) and np.isnan(want["d1"][1]) and 0.8 * H * W < want["n"][0] < 0.9 * H * W
    zt, yt = _t(z).to(cuda), _t(y).to(cuda)
    got = metrics.depth_errors(zt, yt)
    _assert_depth(got, want, f"{hw}")
    assert torch.equal(ops.metric_depth(zt, yt), got["sums"])                  # two runs: the same bits
    shift = lambda v: torch.cat([torch.zeros(1), _t(v).reshape(-1)]).to(cuda)[1:].view(v.shape)
    zs, ys = shift(z), shift(y)                                                # unaligned: the one-pixel form
    assert zs.data_ptr() % 16 and ys.data_ptr() % 16
    assert torch.equal(ops.metric_depth(zs, ys), got["sums"])
    narrow = metrics.depth_errors(zt, yt, min_depth=5.0, max_depth=40.0)       # another range
    _assert_depth(narrow, mr.depth_errors(z, y, 5.0, 40.0), f"{hw} (5, 40)")


def test_lidar_depths_just_inside_and_just_outside_both_bounds(cuda):
    from mudg_amd import ops
    up, down = lambda v: np.nextafter(F(v), F(np.inf)), lambda v: np.nextafter(F(v), F(-np.inf))
    for lo, hi in ((0.1, 80.0), (2.0 ** -6, 256.0), (0.5, 64.0)):
        below_lo, above_lo = (down(lo), F(lo)) if float(F(lo)) > lo else (F(lo), up(lo))                     # fp32 numbers around the double bound
        below_hi, above_hi = (F(hi), up(hi)) if float(F(hi)) < hi else (down(hi), F(hi))
        y = np.zeros((1, 2, 16), F)
        y[0, 0, :4] = [below_lo, above_lo, below_hi, above_hi]
        z = np.full((1, 2, 16), 1.0, F)
        want = mr.depth_errors(z, y, lo, hi)
        assert want["n"][0] == 2                                                                             # above_lo and below_hi
        got = ops.metric_depth(_t(z).to(cuda), _t(y).to(cuda), min_depth=lo, max_depth=hi)
        assert torch.equal(got.cpu(), _t(want["sums"])), (lo, hi)


def test_the_depth_sums_have_headroom_at_the_full_frame_size(cuda):
    """One 576 x 1024 frame with e at its maximum: the widest range the entry takes, every LiDAR depth the fp32 number above 2^-6 and
    every depth 256 m and beyond — e just below 256, e e just below 2^16, r just below 2^14."""
    from mudg_amd import ops
    H, W = 576, 1024
    y0 = np.nextafter(F(2.0 ** -6), F(1))
    z = torch.full((1, H, W), 1000.0, dtype=torch.float32, device=cuda)        # taken to 256
    y = torch.full((1, H, W), float(y0), dtype=torch.float32, device=cuda)
    one = mr.depth_sums(np.full((1, 1), 1000.0, F), np.full((1, 1), y0, F), 2.0 ** -6, 256.0)
    assert one[0] == 1 and one[2] > 2 ** 35 and one[3] > 2 ** 33 and one[4:7] == (0, 0, 0)
    got = ops.metric_depth(z, y, min_depth=2.0 ** -6, max_depth=256.0)
    assert got.cpu().tolist() == [[H * W * v for v in one]]
    assert torch.equal(ops.metric_depth(z, y, min_depth=2.0 ** -6, max_depth=256.0), got)
    exact = ops.metric_depth(y.clone(), y, min_depth=2.0 ** -6, max_depth=256.0)
    assert exact.cpu().tolist() == [[H * W, 0, 0, 0, H * W, H * W, H * W, 0]]


# ------------------------------------------------------------------------------------------------ labels
def _assert_labels(got, want, what):
    assert set(got) == {"confusion", "iou", "miou", "pixel_acc", "bad"}
    assert got["confusion"].dtype == torch.int64 and torch.equal(got["confusion"].cpu(), _t(want["confusion"])), what
    assert got["bad"].dtype == torch.int64 and torch.equal(got["bad"].cpu(), _t(want["bad"])), what
    for name in ("iou", "pixel_acc"):                                         # one division of exactly known integers each
        g, w = got[name].cpu(), _t(want[name])
        assert g.dtype == torch.float64 and g.shape == w.shape and torch.equal(torch.isnan(g), torch.isnan(w)), (what, name)
        assert torch.equal(torch.nan_to_num(g, nan=-1.0), torch.nan_to_num(w, nan=-1.0)), (what, name)
    # miou is a float64 sum of up to 32 values in [0, 1] in the order the library chooses: on either side at most 31 additions, each
    # rounding by at most 2^-53 of a partial sum below 32, and one division
    g, w = got["miou"].cpu(), _t(want["miou"])
    assert g.dtype == torch.float64 and g.shape == w.shape and float((g - w).abs().max()) <= 2 * (31 * 32 + 1) * 2.0 ** -53, (what, g.tolist(), w.tolist())


@pytest.mark.parametrize("classes", [19, 3])
@pytest.mark.parametrize("hw", [(23, 29), (70, 64)])                         # one workgroup; 4480 pixels: two workgroups per frame
def test_the_confusion_matrix_is_equal_to_the_cpu_definition(cuda, classes, hw):
    from mudg_amd import metrics
    rng = np.random.default_rng(31)
    H, W = hw
    gt = rng.integers(0, classes, (3, H, W)).astype(np.int64)
    pred = np.where(rng.random((3, H, W)) < 0.7, gt, rng.integers(0, classes, (3, H, W))).astype(np.int64)
    gt[0, :2, :5], gt[1, 3, 3], gt[2, 0, 0] = 255, -1, classes                 # ignored ground truth
    pred[0, 0, 0] = classes                                                    # under an ignored pixel: not counted at all
    pred[1, 5, :4] = [classes, -1, 2 ** 40, -(2 ** 40)]                        # out of range: bad, in no cell
    gt[1, 5, :4] = 1
    want = mr.segmentation_scores(pred, gt, classes)
    assert want["bad"].tolist() == [0, 4, 0] and int(want["confusion"][1].sum()) == H * W - 1 - 4
    got = metrics.segmentation_scores(_t(pred).to(cuda), _t(gt).to(cuda), classes=classes)
    _assert_labels(got, want, f"{hw} C={classes}")
    again = metrics.segmentation_scores(_t(pred).to(cuda), _t(gt).to(cuda), classes=classes)
    for name in ("confusion", "bad", "miou"):
        assert torch.equal(got[name], again[name]), name
    perfect = metrics.segmentation_scores(_t(gt.clip(0, classes - 1)).to(cuda), _t(gt).to(cuda), classes=classes)
    assert perfect["miou"].cpu().tolist() == [1.0] * 3 and perfect["pixel_acc"].cpu().tolist() == [1.0] * 3


def test_a_full_frame_of_a_single_class_puts_every_count_in_one_cell(cuda):
    from mudg_amd import metrics
    H, W = 576, 1024
    labels = torch.full((1, H, W), 7, dtype=torch.int64, device=cuda)
    got = metrics.segmentation_scores(labels, labels.clone())
    want = torch.zeros((1, 19, 19), dtype=torch.int64)
    want[0, 7, 7] = H * W
    assert torch.equal(got["confusion"].cpu(), want) and got["bad"].cpu().tolist() == [0]
    assert got["miou"].cpu().tolist() == [1.0] and bool(torch.isnan(got["iou"][0, 0])) and float(got["iou"][0, 7]) == 1.0
    wrong = metrics.segmentation_scores(torch.full_like(labels, 8), labels)
    assert int(wrong["confusion"][0, 7, 8]) == H * W and wrong["miou"].cpu().tolist() == [0.0]


# ------------------------------------------------------------------------------------------------ the interface
def test_wrappers_reject_what_the_rules_do_not_cover(cuda):
    from mudg_amd import hip, metrics, ops
    u8 = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=cuda)
    f32 = torch.zeros(2, 16, 16, device=cuda)
    i64 = torch.zeros(2, 16, 16, dtype=torch.int64, device=cuda)
    for call in (lambda: metrics.psnr_ssim(u8[:, :10], u8[:, :10]), lambda: metrics.psnr_ssim(u8[:, :, :10].contiguous(), u8[:, :, :10].contiguous()),
                 lambda: ops.metric_ssim(u8[:, :10].contiguous(), u8[:, :10].contiguous())):
        with pytest.raises(hip.MudgError, match="11 x 11"):                    # H < 11, W < 11
            call()
    for call in (lambda: metrics.psnr_ssim(u8, u8[:1]), lambda: metrics.psnr_ssim(u8, torch.zeros(2, 16, 12, 3, dtype=torch.uint8, device=cuda)),
                 lambda: metrics.depth_errors(f32, f32[:, :8]), lambda: metrics.segmentation_scores(i64, i64[:1]),
                 lambda: metrics.psnr_ssim(u8, u8.float()), lambda: metrics.depth_errors(f32, f32.double()), lambda: metrics.segmentation_scores(i64, i64.int()),
                 lambda: ops.metric_sse(u8, u8[:1]), lambda: metrics.psnr_ssim(f32, f32)):
        with pytest.raises(hip.MudgError, match="on the GPU"):                 # mismatched shapes and types
            call()
    for call in (lambda: metrics.psnr_ssim(u8.cpu(), u8), lambda: metrics.psnr_ssim(u8, u8.cpu()), lambda: metrics.depth_errors(f32, f32.cpu()),
                 lambda: metrics.segmentation_scores(i64.cpu(), i64), lambda: metrics.score_window({"color": u8.cpu()}, color=u8)):
        with pytest.raises(hip.MudgError, match="on the GPU"):                 # CPU tensors
            call()
    for lo, hi in ((2.0 ** -7, 80.0), (0.0, 80.0), (0.1, 256.5), (80.0, 0.1), (float("nan"), 80.0)):
        with pytest.raises(hip.MudgError, match="depth range"):
            metrics.depth_errors(f32, f32, min_depth=lo, max_depth=hi)
    assert hip.lib().mudg_metric_depth(f32.data_ptr(), f32.data_ptr(), 2, 16, 16, 2.0 ** -7, 80.0, i64.data_ptr(), None) == -1   # the entry itself
    assert hip.lib().mudg_metric_depth(f32.data_ptr(), f32.data_ptr(), 2, 16, 16, 0.1, 257.0, i64.data_ptr(), None) == -1
    assert hip.lib().mudg_metric_ssim(u8.data_ptr(), u8.data_ptr(), 2, 10, 16, i64.data_ptr(), None) == -1
    for classes in (0, 33):
        with pytest.raises(hip.MudgError, match="classes"):
            metrics.segmentation_scores(i64, i64, classes=classes)


def test_a_generated_window_is_scored_against_its_own_truths(cuda):
    """render_windows -> synthesize_windows -> window_outputs -> score_window on the tiny driver model (4 frames of 64 x 64, 2 DDIM steps),
    with the rendered colour, the rendered LiDAR depth and the window's own labels as truths.  Every integer equals the definition's;
    labels against themselves give miou = 1 and colour against itself ssim = 1, exactly."""
    from mudg_amd import render
    from mudg_amd.synthetic import street_scene
    from test_splat_gpu import _driver_model, _upload
    from virtual_render import eval_tools
    from virtual_render.virtual_pose_render import render_windows, synthesize_windows, window_outputs
    small = street_scene(n_background=150_000, frames=4, seed=5, n_objects=3, object_points=3000)
    model, g = _driver_model(cuda)
    shp, px = g["shape"], g["driver"]["pixels"]
    L = shp["T"]
    bg, objects = _upload(small, cuda)
    scene = render.Scene(bg, objects, small["intr"], small["c2w"], small["hw_native"])
    dense = (torch.rand(3, 3, L, px, px, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(cuda)
    wins = list(render_windows(scene, dense, pose=1, video_length=L))
    sm = cfgs.SAMPLER
    samples = synthesize_windows(model, wins, [3, 4, L, shp["H"], shp["W"]], video_length=L, ddim_steps=2, ddim_eta=1.0,
                                 unconditional_guidance_scale=sm["cfg_scale"], fs=sm["fs"], timestep_spacing=sm["spacing"],
                                 guidance_rescale=sm["guidance_rescale"])[0]
    cams = np.stack([render.virtual_poses(c, with_ori_pose=True)[1] for c in small["c2w"]])
    cond = render.render_conditions(bg, objects, small["intr"], small["c2w"], small["hw_native"], (px, px), poses=cams[:, None], return_images=True)
    out = window_outputs(samples, cond)
    colour, lidar, labels = cond["rgb"][0], cond["depth"][0], out["semantic_labels"]
    assert colour.dtype == torch.uint8 and tuple(colour.shape) == (L, px, px, 3)
    scores = eval_tools.score_window(out, color=colour, lidar_depth=lidar, labels=labels)
    colour_keys = {"color_" + k for k in ("psnr", "ssim", "sse", "ssim_sum")}
    depth_keys = {"depth_" + k for k in ("n", "mae", "rmse", "abs_rel", "d1", "d2", "d3", "sums")}
    label_keys = {"semantic_" + k for k in ("confusion", "iou", "miou", "pixel_acc", "bad")}
    assert set(scores) == colour_keys | depth_keys | label_keys and all(v.is_cuda for v in scores.values())
    assert set(eval_tools.score_window(out, lidar_depth=lidar)) == depth_keys and eval_tools.score_window(out) == {}       # an absent truth adds no key
    strip = lambda prefix: {k[len(prefix):]: v for k, v in scores.items() if k.startswith(prefix)}
    _assert_colour(strip("color_"), mr.psnr_ssim(out["color"].cpu().numpy(), colour.cpu().numpy()), "window colour")
    _assert_depth(strip("depth_"), mr.depth_errors(out["depth"].cpu().numpy(), lidar.cpu().numpy()), "window depth")
    _assert_labels(strip("semantic_"), mr.segmentation_scores(labels.cpu().numpy(), labels.cpu().numpy()), "window labels")
    assert int(scores["depth_n"].min()) > 0 and bool(torch.isfinite(scores["depth_mae"]).all())
    assert scores["semantic_miou"].cpu().tolist() == [1.0] * L and scores["semantic_bad"].cpu().tolist() == [0] * L
    own = eval_tools.score_window(out, color=out["color"].clone())
    assert own["color_ssim"].cpu().tolist() == [1.0] * L and bool(torch.isinf(own["color_psnr"]).all())
