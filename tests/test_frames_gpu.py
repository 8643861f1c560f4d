"""The frame kernels on the GPU (csrc/frames.hip through mudg_amd/ops.py and mudg_amd/frames.py) against the numpy definition of the
rules (tests/frames_reference.py): torch.equal everywhere and a repeat run equal to the first — both sides do the same integer operations
and the same individually rounded fp32 operations in the same order, so there is no tolerance.  Then the layers above: streams written
into slabs of larger tensors, the palette tied to the one the post-processing holds, dense_streams -> render_windows, SceneClips ->
shared_step."""
import functools

import numpy as np
import pytest
import torch

import frames_reference as fr

pytestmark = pytest.mark.gpu

# the smallest sizes at which each path can go wrong; T = 2, the frames differ
SIZES = [((7, 9), (3, 5)),            # non-integer shrink, right / bottom clamp
         ((5, 6), (11, 13)),          # enlargement: left / top clamp, s < 0
         ((8, 12), (4, 6)),           # exact halving
         ((6, 10), (6, 10)),          # identity
         ((1, 1), (3, 2)), ((2, 3), (1, 1)),      # degenerate
         ((37, 53), (16, 29)),        # odd everything, the bounds-checked path only
         ((9, 130), (5, 67)),         # several lanes per row, with a tail
         ((20, 600), (9, 320)),       # the 16-byte store path at the 1.875 ratio of 1920 -> 1024, two waves per row
         ((4, 1100), (3, 1030))]      # three workgroups per row (512 pixels each), the last one partly filled, with a tail
IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SIZES]
T = 2


@functools.lru_cache(maxsize=None)
def _inputs(hw_in):
    rng = np.random.default_rng(hw_in[0] * 10007 + hw_in[1])
    images = rng.integers(0, 256, size=(T,) + hw_in + (3,), dtype=np.uint8)
    ids = rng.integers(0, 21, size=(T,) + hw_in, dtype=np.uint8)
    ids.reshape(-1)[:: 5] = rng.choice(np.array([0, 20, 21, 255], dtype=np.uint8), size=ids.reshape(-1)[:: 5].shape)
    depth = rng.uniform(-20.0, 160.0, size=(T,) + hw_in).astype(np.float32)          # negatives and values above 100
    depth.reshape(-1)[:: 7] = 0.0
    return images, ids, depth


@functools.lru_cache(maxsize=None)
def _streams(hw_in, hw_out):
    images, ids, depth = _inputs(hw_in)
    return {"color": fr.colour_stream(images, hw_out), "semantic": fr.semantic_stream(ids, hw_out), "depth": (fr.depth_stream(depth, hw_out), None)}


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    differ = int((got != want).sum())
    print(f"{what}: {differ} of {want.numel()} values differ")
    assert torch.equal(got, want), (what, differ)


@pytest.mark.parametrize("hw_in,hw_out", SIZES, ids=IDS)
def test_resize_u8_is_the_definition(cuda, hw_in, hw_out):
    from mudg_amd import ops
    images, ids, _ = _inputs(hw_in)
    for c in (3, 1):
        src = images[..., :c]
        dev = _dev(src, cuda)
        for mode, rule in (("linear", fr.resize_u8_linear), ("nearest", fr.resize_u8_nearest)):
            got = ops.resize_u8(dev, hw_out, mode)
            _same(got, rule(src, hw_out), f"resize_u8 {mode} C={c} {hw_in}->{hw_out}")
            assert torch.equal(ops.resize_u8(dev, hw_out, mode), got)
    got = ops.resize_u8(_dev(ids, cuda), hw_out, palette=True)
    _same(got, fr.resize_u8_linear(fr.colourise(ids), hw_out), f"resize_u8 palette {hw_in}->{hw_out}")


@pytest.mark.parametrize("hw_in,hw_out", SIZES, ids=IDS)
def test_resize_f32_is_the_definition(cuda, hw_in, hw_out):
    from mudg_amd import ops
    depth = _inputs(hw_in)[2]
    big = _inputs((37, 53))[2]
    assert (big == 0).any() and (big < 0).any() and (big > 100).any()
    dev = _dev(depth, cuda)
    got = ops.resize_f32(dev, hw_out)
    _same(got, fr.resize_f32_linear(depth, hw_out), f"resize_f32 {hw_in}->{hw_out}")
    assert torch.equal(ops.resize_f32(dev, hw_out), got)


@pytest.mark.parametrize("hw_in,hw_out", SIZES, ids=IDS)
def test_the_three_streams_are_the_definition(cuda, hw_in, hw_out):
    from mudg_amd import frames, ops
    images, ids, depth = _inputs(hw_in)
    assert set(range(21)) | {21, 255} <= set(np.unique(_inputs((37, 53))[1]).tolist())
    want = _streams(hw_in, hw_out)
    dev_images, dev_ids = _dev(images, cuda), _dev(ids, cuda)
    for name, fn, src in (("color", frames.stream_from_images, dev_images), ("semantic", frames.stream_from_labels, dev_ids)):
        got, u8 = fn(src, hw_out, return_u8=True)
        _same(got, want[name][0], f"{name} stream {hw_in}->{hw_out}")
        _same(u8, want[name][1], f"{name} stream's uint8 frames {hw_in}->{hw_out}")
        assert torch.equal(u8, ops.resize_u8(src, hw_out, palette=name == "semantic"))
        assert torch.equal(fn(src, hw_out), got)                                                         # without the bytes, and again
    got = frames.stream_from_depth(_dev(depth, cuda), hw_out)
    _same(got, want["depth"][0], f"depth stream {hw_in}->{hw_out}")
    assert torch.equal(frames.stream_from_depth(_dev(depth, cuda), hw_out), got)
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


@pytest.mark.parametrize("hw_in,hw_out", [((20, 600), (9, 320)), ((37, 53), (16, 29))], ids=["wide", "tail"])
@pytest.mark.parametrize("kind", ["color", "semantic", "depth"])
def test_a_stream_written_into_a_slab_changes_nothing_else(cuda, kind, hw_in, hw_out):
    """Stream 1, frames 3 .. 4 of a sentinel-filled (3, 3, 8, h, w) tensor."""
    from mudg_amd import ops
    src = _dev(_inputs(hw_in)[("color", "semantic", "depth").index(kind)], cuda)
    want = torch.from_numpy(_streams(hw_in, hw_out)[kind][0])
    out = torch.full((3, 3, 8) + hw_out, float("nan"), device=cuda)
    assert ops.dense_stream(kind, src, hw_out, out, slab=1, frame0=3) is out
    got = out.cpu()
    assert torch.equal(got[1, :, 3:5], want)
    got[1, :, 3:5] = float("nan")
    assert bool(torch.isnan(got).all()), "values outside stream 1, frames 3 .. 4 were written"


@pytest.mark.parametrize("kind", ["color", "semantic", "depth"])
def test_a_destination_that_is_not_16_byte_aligned_takes_the_tail_path(cuda, kind):
    """W % 4 == 0, but the base is one float past a 16-byte boundary: the same values, one store per value, nothing outside the view."""
    from mudg_amd import ops
    hw_in, hw_out = (20, 600), (9, 320)
    h, w = hw_out
    src = _dev(_inputs(hw_in)[("color", "semantic", "depth").index(kind)], cuda)
    want = torch.from_numpy(_streams(hw_in, hw_out)[kind][0])
    frame, channel = h * w + 3, T * (h * w + 3) + 5                           # strides that are no multiple of 4 either
    flat = torch.full((256 + 1 + 3 * channel + 64,), float("nan"), device=cuda)
    assert flat.data_ptr() % 16 == 0
    view = torch.as_strided(flat, (3, T, h, w), (channel, frame, w, 1), 257)
    assert view.data_ptr() % 16 == 4
    ops.dense_stream(kind, src, hw_out, view)
    host = flat.cpu()
    got = torch.as_strided(host, (3, T, h, w), (channel, frame, w, 1), 257)
    assert torch.equal(got, want)
    got.fill_(float("nan"))
    assert bool(torch.isnan(host).all()), "values outside the view were written"


def test_offsets_past_2_to_the_31_bytes_in_the_source_and_the_destination(cuda):
    """A resident scene is gigabytes per stream: 11000 colour frames of 64 x 1024 are 2.16 GB of source, and the destination's strides put
    the last frames of channel 2 beyond 2^31 bytes as well.  The first and the last two frames against the definition."""
    from mudg_amd import ops
    frames_n, hw_in, hw_out, fs = 11000, (64, 1024), (3, 5), 17000
    src = torch.randint(0, 256, (frames_n,) + hw_in + (3,), dtype=torch.uint8, device=cuda, generator=torch.Generator(device=cuda).manual_seed(31))
    assert src.numel() > 2 ** 31
    flat = torch.empty(3 * frames_n * fs, dtype=torch.float32, device=cuda)
    out = torch.as_strided(flat, (3, frames_n) + hw_out, (frames_n * fs, fs, hw_out[1], 1))
    assert (out[2, -1].data_ptr() - flat.data_ptr()) > 2 ** 31
    ops.dense_stream("color", src, hw_out, out)
    ends = [0, 1, frames_n - 2, frames_n - 1]
    want = fr.colour_stream(src[ends].cpu().numpy(), hw_out)[0]
    _same(out[:, ends], want, "colour stream, frames at both ends of 2.16 GB")


def test_the_palette_is_the_one_the_post_processing_holds(cuda):
    """labels 0 .. 18 at equal sizes -> semantic stream -> frames_to_uint8 -> semantic_nearest gives the labels back."""
    from mudg_amd import frames, ops
    labels = torch.from_numpy(np.random.default_rng(8).integers(0, 19, size=(2, 24, 40), dtype=np.uint8)).to(cuda)
    labels[0, 0, :19] = torch.arange(19, dtype=torch.uint8, device=cuda)
    stream = frames.stream_from_labels(labels, (24, 40))
    u8 = ops.frames_to_uint8(stream[None])[0]                                # (t, h, w, 3)
    for t in range(2):
        _, back = ops.semantic_nearest(u8[t].permute(2, 0, 1))
        assert torch.equal(back, labels[t].long())


@pytest.fixture(scope="module")
def small():
    from mudg_amd.synthetic import street_scene
    return street_scene(n_background=150_000, frames=6, seed=5, n_objects=3, object_points=3000)


def _scene(small, dev):
    from mudg_amd import render
    bg = render.PointCloud.from_arrays(small["bg_xyz"], small["bg_rgb"], dev)
    objects = render.ObjectSet(small["objects"], small["transform_obj"], small["visibility"], dev)
    return render.Scene(bg, objects, small["intr"], small["c2w"], small["hw_native"])


def _scene_frames(dev, n=6, hw=(90, 134)):
    from mudg_amd import frames
    rng = np.random.default_rng(21)
    images = {f: rng.integers(0, 256, size=hw + (3,), dtype=np.uint8) for f in range(n)}
    depth = {f: rng.uniform(0.0, 120.0, size=hw).astype(np.float32) for f in range(n)}
    labels = {f: rng.integers(0, 21, size=hw, dtype=np.uint8) for f in range(n)}
    sf = frames.SceneFrames.from_loader(lambda cam, f: images[f], "camera_FRONT", range(n), load_depth=lambda cam, f: depth[f],
                                        load_labels=lambda cam, f: labels[f], device=dev)
    assert len(sf) == n and sf.images.is_cuda and sf.images.shape == (n,) + hw + (3,) and sf.depth.dtype == torch.float32
    assert np.array_equal(sf.images[3].cpu().numpy(), images[3]) and np.array_equal(sf.labels[n - 1].cpu().numpy(), labels[n - 1])
    return sf


def test_dense_streams_feed_render_windows(cuda, small):
    from mudg_amd import frames
    from virtual_render.virtual_pose_render import render_windows
    scene, sf, hw, L = _scene(small, cuda), _scene_frames(cuda), (64, 64), 4
    dense = frames.dense_streams(sf.images, sf.depth, sf.labels, hw)
    assert dense.shape == (3, 3, 6, 64, 64) and dense.dtype == torch.float32 and dense.is_cuda
    assert torch.equal(dense[0], frames.stream_from_images(sf.images, hw)) and torch.equal(dense[1], frames.stream_from_depth(sf.depth, hw))
    assert torch.equal(dense[2], frames.stream_from_labels(sf.labels, hw))
    only_colour = frames.dense_streams(sf.images, None, None, hw)
    assert all(torch.equal(only_colour[s], dense[0]) for s in range(3))
    wins = list(render_windows(scene, dense, pose=1, video_length=L))
    assert len(wins) == 2
    for k, win in enumerate(wins):
        assert win["sparse"].shape == (3, 3, L, 64, 64) and win["sparse_depth"].shape == (3, 3, L, 64, 64)
        assert torch.equal(win["dense"], dense[:, :, 2 * k:2 * k + L]) and win["class_label"].tolist() == [[0], [500], [1]]
        assert torch.equal(win["sparse"][:, :, 0], dense[:, :, 2 * k])                  # sparse frame 0 is dense frame 0, per stream


def test_scene_clips_items(cuda, small):
    from mudg_amd import frames, hip, render
    scene, sf, hw, L = _scene(small, cuda), _scene_frames(cuda), (64, 64), 4
    clips = frames.SceneClips(scene, sf, hw, video_length=L, generator=np.random.default_rng(0))
    assert len(clips) == 3
    colour = frames.stream_from_images(sf.images, hw)
    whole = {"color": colour, "semantic": frames.stream_from_labels(sf.labels, hw), "depth": frames.stream_from_depth(sf.depth, hw)}
    for index, label, code in ((0, "color", 0), (1, "semantic", 1), (2, "depth", 500)):
        item = clips.__getitem__(index, label=label)
        assert set(item) == {"dense_frames", "sparse_frames", "sparse_depth", "caption", "fps", "class_label"}
        for key in ("dense_frames", "sparse_frames", "sparse_depth"):
            assert item[key].shape == (3, L, 64, 64) and item[key].dtype == torch.float32 and item[key].device == cuda, key
        assert item["caption"] == "A photo a of driving scene." and item["fps"] == 10
        assert item["class_label"].tolist() == [code] and item["class_label"].device == cuda and item["class_label"].dtype == torch.long
        sel = slice(index, index + L)
        assert torch.equal(item["dense_frames"], whole[label][:, sel])
        cond = render.render_conditions(scene.background, scene.objects, np.asarray(small["intr"]), small["c2w"][sel], small["hw_native"], hw,
                                        poses=small["c2w"][sel, None], frame_ids=range(index, index + L))
        assert torch.equal(item["sparse_frames"][:, 0], colour[:, index])                # the colour stream's frame 0, whatever the label
        assert torch.equal(item["sparse_frames"][:, 1:], cond["sparse_frames"][0, :, 1:])
        assert torch.equal(item["sparse_depth"], cond["sparse_depth"][0])
        assert float((item["sparse_depth"] > -1).float().mean()) > 0.2                    # something was drawn
    drawn = {int(clips[0]["class_label"]) for _ in range(12)}
    assert drawn == {0, 1, 500}
    with pytest.raises(hip.MudgError, match="normal"):
        clips.__getitem__(0, label="normal")
    with pytest.raises(hip.MudgError, match="normal"):
        frames.SceneClips(scene, sf, hw, video_length=L, train_labels=("color", "normal"))
    with pytest.raises(hip.MudgError, match="no depth"):
        frames.SceneClips(scene, frames.SceneFrames(sf.images), hw, video_length=L).__getitem__(0, label="depth")


def test_collated_scene_clips_go_through_shared_step(cuda):
    """Two items of the size and model tests/test_batch_input_gpu.py uses -> collate -> shared_step: a finite loss."""
    from helpers import golden
    from mudg_amd import frames
    from mudg_amd.synthetic import street_scene
    from test_batch_input_gpu import build_model
    g = golden("batch_input.pt")
    L, px = g["unet_cfg"]["temporal_length"], g["driver"]["pixels"]
    model = build_model(g, cuda)
    scene = _scene(street_scene(n_background=50_000, frames=L + 1, seed=7, n_objects=2, object_points=1000), cuda)
    clips = frames.SceneClips(scene, _scene_frames(cuda, n=L + 1, hw=(70, 100)), (px, px), video_length=L, generator=np.random.default_rng(1))
    batch = clips.collate([clips.__getitem__(0, label="depth"), clips.__getitem__(1, label="semantic")])
    assert batch["dense_frames"].shape == (2, 3, L, px, px) and batch["class_label"].tolist() == [[500], [1]]
    assert batch["fps"].tolist() == [10, 10] and batch["fps"].device == cuda and batch["caption"] == [frames.CAPTION] * 2
    with torch.no_grad():
        loss, info = model.shared_step(batch, random_uncond=True)
    assert loss.dim() == 0 and bool(torch.isfinite(loss)), float(loss)
