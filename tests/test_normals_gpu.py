"""The surface-normal kernels on the GPU (csrc/normals.hip through mudg_amd/ops.py, depth.py, frames.py and metrics.py) against the numpy
definition of the rules (tests/normals_reference.py): torch.equal everywhere and a repeat run equal to the first — both sides do the same
individually rounded operations in the same order and the same integer counts, so there is no tolerance.  Then the layers above: the
stream written into slabs, rendered LiDAR depth -> normals -> SceneFrames -> SceneClips -> shared_step, and the round trip through the
8-bit frames into the scores."""
import functools
import math

import numpy as np
import pytest
import torch

import normals_reference as nr

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    differ = int(((got != want) & ~(torch.isnan(got) & torch.isnan(want))).sum()) if got.is_floating_point() else int((got != want).sum())
    print(f"{what}: {differ} of {want.numel()} values differ")
    assert differ == 0, (what, differ)
    if not got.is_floating_point() or not bool(torch.isnan(want).any()):
        assert torch.equal(got, want), what


def _cams(intr, hw_native, hw):
    """fx, fy, cx, cy at the map's size: the intrinsics scaled by the ratio of the sizes, float64."""
    (h0, w0), (h, w) = hw_native, hw
    return [(k[0, 0] * w / w0, k[1, 1] * h / h0, k[0, 2] * w / w0, k[1, 2] * h / h0) for k in np.asarray(intr, dtype=D)]


# ------------------------------------------------------------------------------------------------ normals from depth
HW_NATIVE = (96, 128)
INTR = np.array([[[110.0, 0, 63.2], [0, 108.0, 47.9], [0, 0, 1]], [[95.5, 0, 66.0], [0, 99.25, 45.1], [0, 0, 1]], [[110.0, 0, 63.2], [0, 108.0, 47.9], [0, 0, 1]]])


@functools.lru_cache(maxsize=None)
def _depth_inputs(hw):
    """Three frames with their own intrinsics: a smooth surface with a step, holes of every kind, a sky region; the last has no usable pixel."""
    H, W = hw
    rng = np.random.default_rng(H * 1009 + W)
    j, i = np.mgrid[0:H, 0:W]
    z = np.stack([12.0 + 3.0 * np.sin(0.31 * i + f) * np.cos(0.23 * j) + 0.05 * i + rng.normal(scale=0.01, size=hw) for f in range(3)])
    z[0, :, W // 2:] += 25.0                                                 # a depth edge
    z = z.astype(F)
    flat = z[:2].reshape(-1)
    bad = rng.choice(flat.size, size=flat.size // 12, replace=False)
    flat[bad] = rng.choice(np.array([0.0, -3.0, 100.0, 150.0, np.inf, np.nan], dtype=F), size=bad.size)
    z[2] = rng.choice(np.array([0.0, 100.0, np.nan], dtype=F), size=hw)
    labels = rng.integers(0, 19, size=(3,) + hw).astype(np.int64)
    labels[:, : H // 4, W // 3:] = 10                                        # sky
    return z, labels


@pytest.mark.parametrize("hw", [(24, 32), (23, 29)], ids=["four-pixel", "one-pixel"])
@pytest.mark.parametrize("step", [None, 0.05], ids=["free", "step-limit"])
@pytest.mark.parametrize("sky", [False, True], ids=["no-labels", "labels"])
def test_normals_from_depth_are_the_definition(cuda, hw, step, sky):
    from mudg_amd import depth
    z, labels = _depth_inputs(hw)
    assert np.isnan(z).any() and np.isinf(z).any() and (z == 0).any() and (z > 100).any() and (labels == 10).any()
    want_n, want_v = nr.depth_normals_frames(z, _cams(INTR, HW_NATIVE, hw), labels if sky else None, max_rel_step=step)
    assert 0.3 < want_v[:2].mean() < 0.95 and not want_v[2].any()
    dev_z, dev_l = _dev(z, cuda), _dev(labels, cuda) if sky else None
    n, v = depth.normals_from_depth(dev_z, INTR, HW_NATIVE, dev_l, max_rel_step=step)
    _same(v, want_v, f"validity {hw} step {step} sky {sky}")
    _same(n, want_n, f"normals {hw} step {step} sky {sky}")
    n2, v2 = depth.normals_from_depth(dev_z, INTR, HW_NATIVE, dev_l, max_rel_step=step)
    assert torch.equal(n2, n) and torch.equal(v2, v)
    if step is None and not sky:                                             # the other parameters reach the kernel
        other = depth.normals_from_depth(dev_z, INTR, HW_NATIVE, _dev(labels, cuda), sky_label=3, min_depth=5.0, max_depth=14.0)
        want = nr.depth_normals_frames(z, _cams(INTR, HW_NATIVE, hw), labels, sky_label=3, min_depth=5.0, max_depth=14.0)
        _same(other[1], want[1], "validity, another range and sky label")
        _same(other[0], want[0], "normals, another range and sky label")
        assert not np.array_equal(want[1], want_v)


def test_a_depth_base_that_is_not_16_byte_aligned_takes_the_one_pixel_form(cuda):
    from mudg_amd import depth
    hw = (24, 32)
    z, labels = _depth_inputs(hw)
    flat = torch.zeros(z.size + 8, dtype=torch.float32, device=cuda)
    assert flat.data_ptr() % 16 == 0
    view = flat[1:1 + z.size].view(z.shape)
    view.copy_(_dev(z, cuda))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    want_n, want_v = nr.depth_normals_frames(z, _cams(INTR, HW_NATIVE, hw), labels)
    n, v = depth.normals_from_depth(view, INTR, HW_NATIVE, _dev(labels, cuda))
    _same(v, want_v, "validity, unaligned depth")
    _same(n, want_n, "normals, unaligned depth")


@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (5, 1)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_frames_of_one_row_or_column_are_wholly_invalid(cuda, hw):
    from mudg_amd import depth
    n, v = depth.normals_from_depth(torch.full((2,) + hw, 4.0, device=cuda), INTR[0], hw)
    assert n.shape == (2,) + hw + (3,) and v.shape == (2,) + hw and not bool(v.any()) and not bool(n.any())


# ------------------------------------------------------------------------------------------------ the normal stream
SIZES = [((7, 9), (3, 5)), ((5, 6), (11, 13)), ((37, 53), (16, 29)), ((20, 600), (9, 320)), ((4, 1100), (3, 1030))]
IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SIZES]
T = 2


@functools.lru_cache(maxsize=None)
def _maps(hw_in, hw_out):
    rng = np.random.default_rng(hw_in[0] * 10007 + hw_in[1])
    v = rng.normal(size=(T,) + hw_in + (3,))
    v = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)
    row, column = nr._taps(hw_in[0], hw_out[0])[hw_out[0] // 2][0], nr._taps(hw_in[1], hw_out[1])[hw_out[1] // 2][0]
    v[1, row, column, 2] = np.nan                                            # on a tap of the middle output pixel; it stays one, in its channel
    v[0, 0, 0] = 0                                                           # a pixel that was not valid
    return v


@functools.lru_cache(maxsize=None)
def _stream(hw_in, hw_out):
    return nr.normal_stream(_maps(hw_in, hw_out), hw_out)


@pytest.mark.parametrize("hw_in,hw_out", SIZES, ids=IDS)
def test_the_normal_stream_is_the_definition(cuda, hw_in, hw_out):
    from mudg_amd import frames
    src = _maps(hw_in, hw_out)
    assert not np.array_equal(src[0, 1:], src[1, 1:])
    want = _stream(hw_in, hw_out)
    assert np.isnan(want[2, 1]).any() and not np.isnan(want[:2]).any() and not np.isnan(want[2, 0]).any()
    dev = _dev(src, cuda)
    got = frames.stream_from_normals(dev, hw_out)
    _same(got, want, f"normal stream {hw_in}->{hw_out}")
    again = frames.stream_from_normals(dev, hw_out)
    assert torch.equal(torch.nan_to_num(again, nan=7.0), torch.nan_to_num(got, nan=7.0))
    same_size = frames.stream_from_normals(dev, hw_in)                       # equal sizes: the input, apart from what a NaN tap touches
    keep = ~torch.isnan(same_size)
    assert torch.equal(same_size[keep], dev.permute(3, 0, 1, 2)[keep]) and int((~keep).sum()) <= 4


@pytest.mark.parametrize("hw_in,hw_out", [((20, 600), (9, 320)), ((37, 53), (16, 29))], ids=["wide", "tail"])
def test_the_normal_stream_written_into_a_slab_changes_nothing_else(cuda, hw_in, hw_out):
    """Stream 1, frames 3 .. 4 of a sentinel-filled (3, 3, 8, h, w) tensor."""
    from mudg_amd import frames
    maps = np.nan_to_num(_maps(hw_in, hw_out), nan=0.25)                             # NaN is the sentinel here
    want = torch.from_numpy(nr.normal_stream(maps, hw_out))
    out = torch.full((3, 3, 8) + hw_out, float("nan"), device=cuda)
    assert frames.stream_from_normals(_dev(maps, cuda), hw_out, out, slab=1, frame0=3) is out
    got = out.cpu()
    assert torch.equal(got[1, :, 3:5], want)
    got[1, :, 3:5] = float("nan")
    assert bool(torch.isnan(got).all()), "values outside stream 1, frames 3 .. 4 were written"


# ------------------------------------------------------------------------------------------------ angular errors
@functools.lru_cache(maxsize=None)
def _error_inputs(hw):
    """Three frames: predictions near the truth and far from it, truths of any length with zero and non-finite vectors; the last frame's
    truth is all zeros, so nothing of it is counted."""
    rng = np.random.default_rng(hw[0] * 31 + hw[1])
    pred = rng.integers(0, 256, size=(3,) + hw + (3,), dtype=np.uint8)
    gt = (rng.normal(size=(3,) + hw + (3,)) * rng.uniform(0.2, 3.0, size=(3,) + hw + (1,))).astype(F)
    gt[0] = ((2.0 * pred[0] - 255) / 255 + rng.normal(scale=0.08, size=hw + (3,))).astype(F)
    gt[1, 0, :6] = np.array([[0, 0, 0], [np.inf, 0, 0], [np.nan, 1, 0], [0, -np.inf, 1], [3e38, 3e38, 3e38], [1e-30, 0, 0]], dtype=F)
    gt[2] = 0
    valid = (rng.integers(0, 4, size=(3,) + hw) > 0).astype(np.uint8) * rng.integers(1, 256, size=(3,) + hw).astype(np.uint8)
    return pred, gt, valid


def _check_scores(got, hists, what):
    for key in ("n", "mean", "median", "a11", "a22", "a30"):
        want = np.array([nr.scores(h)[key] for h in hists])
        _same(got[key], want.astype(np.int64 if key == "n" else D), f"{what}: {key}")


@pytest.mark.parametrize("hw", [(24, 32), (23, 29)], ids=["four-pixel", "one-pixel"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "valid"])
def test_normal_errors_are_the_definition(cuda, hw, masked):
    from mudg_amd import metrics
    pred, gt, valid = _error_inputs(hw)
    hists = [nr.normal_hist(pred[f], gt[f], valid[f] if masked else None) for f in range(3)]
    assert hists[0].sum() > 0 and hists[0][:60].sum() > hists[0][60:].sum() and hists[1].sum() > 0 and hists[2].sum() == 0
    args = (_dev(pred, cuda), _dev(gt, cuda), _dev(valid, cuda) if masked else None)
    got = metrics.normal_errors(*args)
    _same(got["hist"], np.stack(hists), f"histogram {hw} masked {masked}")
    _check_scores(got, hists, f"scores {hw} masked {masked}")
    assert bool(torch.isnan(got["mean"][2])) and bool(torch.isnan(got["a11"][2])) and int(got["n"][2]) == 0
    again = metrics.normal_errors(*args)
    assert torch.equal(again["hist"], got["hist"])


def test_a_whole_frame_in_one_bin(cuda):
    """576 x 1024 pixels with the same prediction and the same truth: every count of a frame lands on one LDS word and one global word."""
    from mudg_amd import metrics
    H, W = 576, 1024
    pixel_u, pixel_g = np.array([[255, 128, 100]], np.uint8), np.array([[0.9, 0.1, -0.3]], F)
    one = nr.normal_hist(pixel_u, pixel_g)
    k = int(np.flatnonzero(one)[0])
    assert one.sum() == 1 and 0 < k < 719
    pred = torch.from_numpy(pixel_u).to(cuda).expand(1, H, W, 3).contiguous()
    gt = torch.from_numpy(pixel_g).to(cuda).expand(1, H, W, 3).contiguous()
    got = metrics.normal_errors(pred, gt)
    _same(got["hist"], (one * (H * W))[None], "one bin")
    _check_scores(got, [one * (H * W)], "one bin")
    assert float(got["median"][0]) == (k + 0.5) * 0.25 and float(got["mean"][0]) == (k + 0.5) * 0.25


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def small():
    from mudg_amd.synthetic import street_scene
    return street_scene(n_background=150_000, frames=6, seed=5, n_objects=3, object_points=3000)


def _scene(street, dev):
    from mudg_amd import render
    bg = render.PointCloud.from_arrays(street["bg_xyz"], street["bg_rgb"], dev)
    objects = render.ObjectSet(street["objects"], street["transform_obj"], street["visibility"], dev)
    return render.Scene(bg, objects, street["intr"], street["c2w"], street["hw_native"])


def _frames_with_normals(street, scene, dev, hw):
    """Random camera frames and labels of size hw, and the normals of the LiDAR depth rendered at the original poses at that size."""
    from mudg_amd import depth, frames, render
    n = len(street["c2w"])
    rng = np.random.default_rng(21)
    images = _dev(rng.integers(0, 256, size=(n,) + hw + (3,), dtype=np.uint8), dev)
    labels = _dev(rng.integers(0, 21, size=(n,) + hw, dtype=np.uint8), dev)
    cond = render.render_conditions(scene.background, scene.objects, street["intr"], street["c2w"], street["hw_native"], hw,
                                    poses=np.asarray(street["c2w"])[:, None], return_images=True)
    lidar = cond["depth"][0].contiguous()
    assert lidar.shape == (n,) + hw and float((lidar > 0).float().mean()) > 0.2
    normals, valid = depth.normals_from_depth(lidar, street["intr"], street["hw_native"], max_rel_step=0.05)
    return frames.SceneFrames(images, labels=labels, normals=normals), lidar, normals, valid


def test_rendered_depth_to_normals_to_scene_clips(cuda, small):
    from mudg_amd import frames, hip
    scene = _scene(small, cuda)
    hw_src, hw, L = (90, 134), (64, 64), 4
    sf, lidar, normals, valid = _frames_with_normals(small, scene, cuda, hw_src)
    cams = _cams(np.broadcast_to(np.asarray(small["intr"], dtype=D), (6, 3, 3)), small["hw_native"], hw_src)
    want_n, want_v = nr.depth_normals_frames(lidar.cpu().numpy(), cams, max_rel_step=0.05)
    _same(valid, want_v, "validity of the rendered depth's normals")
    _same(normals, want_n, "normals of the rendered depth")
    assert int(valid.sum()) > 0 and torch.equal(sf.source("normal"), normals)
    clips = frames.SceneClips(scene, sf, hw, video_length=L, train_labels=("color", "semantic", "normal"), generator=np.random.default_rng(0))
    item = clips.__getitem__(1, label="normal")
    assert item["class_label"].tolist() == [1000] and item["class_label"].device == cuda and item["class_label"].dtype == torch.long
    assert item["dense_frames"].shape == (3, L, 64, 64) and torch.equal(item["dense_frames"], frames.stream_from_normals(normals[1:1 + L], hw))
    _same(item["dense_frames"], nr.normal_stream(normals[1:1 + L].cpu().numpy(), hw), "the item's dense frames")
    colour = clips.__getitem__(1, label="color")
    assert torch.equal(item["sparse_frames"][:, 0], colour["dense_frames"][:, 0])        # the colour stream's frame 0, whatever the label
    assert torch.equal(item["sparse_frames"], colour["sparse_frames"]) and torch.equal(item["sparse_depth"], colour["sparse_depth"])
    drawn = {int(clips[0]["class_label"]) for _ in range(12)}
    assert drawn == {0, 1, 1000}
    with pytest.raises(hip.MudgError, match="depth"):                        # the other triple's stream is not in these frames
        clips.__getitem__(0, label="depth")
    with pytest.raises(hip.MudgError, match="train_labels"):
        frames.SceneClips(scene, sf, hw, video_length=L, train_labels=("color", "semantic", "normal", "depth"))
    with pytest.raises(hip.MudgError, match="train_labels"):
        frames.SceneClips(scene, sf, hw, video_length=L, train_labels=("color", "depth", "normal"))


def test_a_normal_item_and_a_colour_item_go_through_shared_step(cuda):
    """Two items of the size and model tests/test_batch_input_gpu.py uses -> collate -> shared_step: a finite loss."""
    from helpers import golden
    from mudg_amd import frames
    from mudg_amd.synthetic import street_scene
    from test_batch_input_gpu import build_model
    g = golden("batch_input.pt")
    L, px = g["unet_cfg"]["temporal_length"], g["driver"]["pixels"]
    model = build_model(g, cuda)
    street = street_scene(n_background=50_000, frames=L + 1, seed=7, n_objects=2, object_points=1000)
    scene = _scene(street, cuda)
    sf = _frames_with_normals(street, scene, cuda, (70, 100))[0]
    clips = frames.SceneClips(scene, sf, (px, px), video_length=L, train_labels=("color", "semantic", "normal"), generator=np.random.default_rng(1))
    batch = clips.collate([clips.__getitem__(0, label="normal"), clips.__getitem__(1, label="color")])
    assert batch["dense_frames"].shape == (2, 3, L, px, px) and batch["class_label"].tolist() == [[1000], [0]]
    with torch.no_grad():
        loss, info = model.shared_step(batch, random_uncond=True)
    assert loss.dim() == 0 and bool(torch.isfinite(loss)), float(loss)


def test_the_round_trip_through_8_bit_frames_stays_inside_the_rounding_rule(cuda):
    """normals -> stream at equal size -> frames_to_uint8 -> normal_errors against the same normals.  frames_to_uint8 truncates
    g = (x + 1) / 2 * 255, so u = floor(g) (its three fp32 roundings move g by less than 3 * 2^-24 * 255 < 1e-4 and can move u by one
    only where g is that close to an integer) and the decoded p = 2 u - 255 differs from 255 x by at most a whole step of 2, plus 2e-4,
    per channel: |p - 255 n| <= sqrt(3) (2 + 2e-4), and the angle between p and n is at most asin of that over |255 n| — the fp32
    components of a unit normal leave |n| >= 1 - 2^-22.  Derived from the rule, not from what the kernels give."""
    from mudg_amd import depth, frames, metrics, ops
    hw = (24, 32)
    z, _ = _depth_inputs(hw)
    normals, valid = depth.normals_from_depth(_dev(z, cuda), INTR, HW_NATIVE)
    stream = frames.stream_from_normals(normals, hw)
    assert torch.equal(stream, normals.permute(3, 0, 1, 2))                  # nothing here is NaN: the input itself
    u8 = ops.frames_to_uint8(stream[None])[0]
    assert u8.shape == normals.shape and u8.dtype == torch.uint8
    got = metrics.normal_errors(u8, normals, valid)
    assert torch.equal(got["n"], valid.sum((1, 2)).long()) and int(got["n"][0]) > 300
    assert torch.equal(metrics.normal_errors(u8, normals)["hist"], got["hist"])          # what is not valid is (0, 0, 0): never counted
    limit = math.degrees(math.asin(math.sqrt(3.0) * (2.0 + 2e-4) / (255.0 * (1.0 - 2.0 ** -22))))
    last = int(limit / 0.25)                                                 # the bin that holds the limit
    print(f"round trip: the rule allows {limit:.4f} degrees (bin {last}); counts per bin {got['hist'][:, :last + 2].sum(0).tolist()}")
    assert 0.5 < limit < 1.0 and int(got["hist"][:, last + 1:].sum()) == 0
    _same(got["hist"], np.stack([nr.normal_hist(u8[f].cpu().numpy(), normals[f].cpu().numpy(), valid[f].cpu().numpy()) for f in range(3)]), "round trip")
