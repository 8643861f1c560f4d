"""The sparse-condition renderer on the GPU (csrc/splat.hip through mudg_amd/render.py) against the CPU definition of the raster rule
(tests/splat_reference.py): torch.equal everywhere — both sides perform the same correctly rounded fp32 operations and the depth test is
an order-free integer minimum, so there is no tolerance and no pixel is left out."""
import numpy as np
import pytest
import torch

import splat_reference as sr
from helpers import cfgs, golden, seeded_sd

pytestmark = pytest.mark.gpu
NAMES = ("bg_rgb", "bg_depth", "obj_rgb", "obj_depth", "mask", "rgb", "depth", "sparse_frames", "sparse_depth")


def _upload(scene, dev):
    from mudg_amd import render
    bg = render.PointCloud.from_arrays(scene["bg_xyz"], scene["bg_rgb"], dev)
    objects = render.ObjectSet(scene["objects"], scene["transform_obj"], scene["visibility"], dev)
    return bg, objects


def _poses(scene):
    from mudg_amd import render
    return np.stack([np.stack(render.virtual_poses(c, with_ori_pose=True)) for c in scene["c2w"]])


def _reference(scene, hw_out, poses=None, frame_ids=None, frames=slice(None)):
    poses = _poses(scene) if poses is None else poses
    return sr.render_conditions(scene["bg_xyz"], scene["bg_rgb"], scene["objects"], scene["transform_obj"], scene["visibility"],
                                scene["intr"], scene["c2w"][frames], scene["hw_native"], hw_out, poses[frames], frame_ids)


def _assert_equal(got, want, what):
    for name in NAMES:
        w = torch.from_numpy(np.ascontiguousarray(want[name]))
        g = got[name].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        differ = int((g != w).sum())
        print(f"{what}: {name}: {differ} of {w.numel()} values differ")
        assert torch.equal(g, w), (what, name, differ)


@pytest.fixture(scope="module")
def street():
    from mudg_amd.synthetic import street_scene
    return street_scene(n_background=2_000_000, frames=4, seed=11)


@pytest.fixture(scope="module")
def small():
    from mudg_amd.synthetic import street_scene
    return street_scene(n_background=150_000, frames=6, seed=5, n_objects=3, object_points=3000)


@pytest.mark.parametrize("hw_out", [(576, 1024), (320, 512)])
def test_street_scene_is_bit_equal_to_the_cpu_definition(cuda, street, hw_out):
    """2 M background points and four moving boxes, 1280 x 1920 native, three poses (the camera and 2 m to either side), four
    frames: both layers, the mask, the merged images and both condition tensors."""
    from mudg_amd import render
    bg, objects = _upload(street, cuda)
    assert len(bg) == 2_000_000 and street["visibility"][1, 1] == 0
    got = render.render_conditions(bg, objects, street["intr"], street["c2w"], street["hw_native"], hw_out, return_images=True)
    torch.cuda.synchronize()
    assert got["sparse_frames"].shape == (3, 3, 4, *hw_out) and got["rgb"].shape == (3, 4, *hw_out, 3)
    want = _reference(street, hw_out)
    # the scene exercises what it is meant to: both layers visible in every pose, the mask neither empty nor everything
    assert all(want["bg_depth"][p, t].astype(bool).mean() > 0.2 for p in range(3) for t in range(4))
    assert all(0 < want["mask"][p, t].mean() < 0.5 for p in range(3) for t in range(4))
    _assert_equal(got, want, f"street {hw_out}")
    # the default poses are the reference's: the original camera, then generate_virtual_pose
    again = render.render_conditions(bg, objects, street["intr"], street["c2w"], street["hw_native"], hw_out, poses=_poses(street))
    assert torch.equal(again["sparse_frames"], got["sparse_frames"]) and torch.equal(again["sparse_depth"], got["sparse_depth"])


def test_runs_are_identical_and_one_launch_of_three_poses_equals_three_of_one(cuda, small):
    from mudg_amd import render
    bg, objects = _upload(small, cuda)
    hw = (144, 256)
    args = (bg, objects, small["intr"], small["c2w"], small["hw_native"], hw)
    a = render.render_conditions(*args, return_images=True)
    b = render.render_conditions(*args, return_images=True)
    for name in NAMES:
        assert torch.equal(a[name], b[name]), name
    poses = _poses(small)
    for p in range(3):
        one = render.render_conditions(*args, poses=poses[:, p:p + 1], return_images=True)
        for name in NAMES:
            assert torch.equal(one[name][0], a[name][p]), (p, name)
    # without the early reject: the same image (the load in front of the atomic only ever skips what would lose)
    c = render.render_conditions(*args, return_images=True, early_reject=False)
    for name in NAMES:
        assert torch.equal(a[name], c[name]), name
    _assert_equal(a, _reference(small, hw), "small scene")


def test_equal_depth_goes_to_the_lower_index(cuda, small):
    """Every point twice, the copy in another colour: the image is the one of the cloud alone, whichever arrives first."""
    from mudg_amd import render
    hw = (144, 256)
    other = (255 - small["bg_rgb"]).astype(np.uint8)
    single = render.PointCloud.from_arrays(small["bg_xyz"], small["bg_rgb"], cuda)
    double = render.PointCloud.from_arrays(np.concatenate([small["bg_xyz"], small["bg_xyz"]]), np.concatenate([small["bg_rgb"], other]), cuda)
    flipped = render.PointCloud.from_arrays(np.concatenate([small["bg_xyz"], small["bg_xyz"]]), np.concatenate([other, small["bg_rgb"]]), cuda)
    args = (None, small["intr"], small["c2w"][:2], small["hw_native"], hw)
    a = render.render_conditions(single, *args, return_images=True)
    b = render.render_conditions(double, *args, return_images=True)
    c = render.render_conditions(flipped, *args, return_images=True)
    assert torch.equal(a["rgb"], b["rgb"]) and torch.equal(a["depth"], b["depth"]) and torch.equal(a["sparse_frames"], b["sparse_frames"])
    assert torch.equal(a["depth"], c["depth"]) and not torch.equal(a["rgb"], c["rgb"])
    hit = a["depth"] > 0
    assert torch.equal(c["rgb"][hit], 255 - a["rgb"][hit])


def test_all_culled_and_no_visible_object(cuda, small):
    from mudg_amd import render
    hw = (144, 256)
    bg, objects = _upload(small, cuda)
    front = small["bg_xyz"][:, 2] > 1.0                                                   # a cloud wholly in front of the first camera
    cloud = render.PointCloud.from_arrays(small["bg_xyz"][front], small["bg_rgb"][front], cuda)
    about = np.diag([-1.0, 1.0, -1.0, 1.0])                                               # the camera turned round: every zc < 0
    out = render.render_conditions(cloud, None, small["intr"], about[None], small["hw_native"], hw, poses=about[None, None], return_images=True)
    assert not out["rgb"].any() and not out["depth"].any() and not out["mask"].any()
    assert torch.all(out["sparse_frames"] == -1.0) and torch.all(out["sparse_depth"] == -1.0)
    # no visible object: the background (the reference draws its one-point sentinel, which is black)
    hidden = render.ObjectSet(small["objects"], small["transform_obj"], np.zeros_like(small["visibility"]), cuda)
    args = (small["intr"], small["c2w"][:2], small["hw_native"], hw)
    a = render.render_conditions(bg, hidden, *args, return_images=True)
    b = render.render_conditions(bg, None, *args, return_images=True)
    for name in NAMES:
        assert torch.equal(a[name], b[name]), name
    assert not a["mask"].any() and torch.equal(a["rgb"], a["bg_rgb"]) and a["depth"].any()
    # and with objects shown the image differs
    c = render.render_conditions(bg, objects, *args, return_images=True)
    assert c["mask"].any() and not torch.equal(c["rgb"], a["rgb"])


def test_kernel_wrappers_check_their_arguments(cuda):
    from mudg_amd import hip, ops
    pts = torch.zeros(8, 4, dtype=torch.int32, device=cuda)
    keys = ops.splat_keys(2, 8, 8, cuda)
    mats = torch.zeros(2, 1, 12, device=cuda)
    with pytest.raises(hip.MudgError, match="point size"):
        ops.splat_points(pts, mats, keys, (1, 1, 0, 0), 9.0)
    with pytest.raises(hip.MudgError, match="per-point ids"):
        ops.splat_points(pts, torch.zeros(2, 3, 12, device=cuda), keys, (1, 1, 0, 0), 2.5)
    with pytest.raises(hip.MudgError, match="do not go with"):
        ops.splat_points(pts, torch.zeros(3, 1, 12, device=cuda), keys, (1, 1, 0, 0), 2.5)
    ops.splat_points(pts, mats, keys, (1, 1, 0, 0), 2.5)                                  # zero matrices: zc = 0, nothing drawn
    depth, colour = ops.splat_resolve(keys, pts)
    assert not depth.any() and not colour.any() and torch.all(keys == -1)


def _driver_model(dev):
    from helpers import _load
    from lvdm.models.ddpm3d import LatentVisualDiffusion
    from lvdm.modules.encoders.resampler import Resampler
    towers = _load("towers")
    g = golden("driver.pt")
    d = g["driver"]
    ident = {"target": "torch.nn.Identity"}
    model = LatentVisualDiffusion(
        img_cond_stage_config=ident, image_proj_stage_config=ident, cond_stage_config=ident,
        first_stage_config={"target": "lvdm.models.autoencoder.AutoencoderKL",
                            "params": {"embed_dim": 4, "ddconfig": g["vae_ddconfig"], "lossconfig": ident}},
        unet_config={"target": "lvdm.modules.networks.openaimodel3d.UNetModel", "params": g["unet_cfg"]},
        **g["diffusion_cfg"])
    model.model.diffusion_model.load_state_dict(seeded_sd(g["unet_param_shapes"], g["seed"], g["unet_checksum"]), strict=True)
    model.first_stage_model.load_state_dict(seeded_sd(g["vae_param_shapes"], g["seed"] + 1, g["vae_checksum"]), strict=True)
    model = model.to(dev).eval()
    model.image_proj_model = Resampler(**d["resampler"])
    model.image_proj_model.load_state_dict(seeded_sd(g["resampler_param_shapes"], g["seed"] + 5, g["resampler_checksum"]), strict=True)
    model.image_proj_model = model.image_proj_model.to(dev).eval()
    model.embedder = towers.FakeImageTower(d["clip_tokens"], d["clip_dim"], d["tower_seed_img"])
    model.cond_stage_model = towers.FakeTextTower(g["unet_cfg"]["context_dim"], d["tower_seed_txt"], dev)
    return model, g


def test_render_windows_feeds_synthesize_windows(cuda, small):
    """A cloud and a pose in, generated clips out: two overlapping windows of the tiny driver model (4 frames of 64 x 64); the window
    dicts are the ones assembled by hand from the CPU definition."""
    from mudg_amd import render
    from virtual_render.virtual_pose_render import render_windows, synthesize_windows
    model, g = _driver_model(cuda)
    shp, px = g["shape"], g["driver"]["pixels"]
    L = shp["T"]
    assert L == 4 and len(small["c2w"]) == 6
    bg, objects = _upload(small, cuda)
    scene = render.Scene(bg, objects, small["intr"], small["c2w"], small["hw_native"])
    gen = torch.Generator().manual_seed(3)
    dense = (torch.rand(3, 3, 6, px, px, generator=gen) * 2 - 1).to(cuda)
    wins = list(render_windows(scene, dense, pose=1, video_length=L))
    assert len(wins) == 2
    cams = np.stack([render.virtual_poses(c, with_ori_pose=True)[1] for c in small["c2w"]])
    assert np.array_equal(cams, np.stack([render.virtual_poses(c)[0] for c in small["c2w"]]))           # the reference's move_id 1
    for k, win in enumerate(wins):
        sel = slice(2 * k, 2 * k + L)
        want = _reference(small, (px, px), poses=cams[:, None], frame_ids=range(2 * k, 2 * k + L), frames=sel)
        sparse = torch.from_numpy(want["sparse_frames"]).repeat(3, 1, 1, 1, 1)
        sparse[:, :, 0] = dense[:, :, 2 * k].cpu()
        assert set(win) == {"sparse", "dense", "sparse_depth", "class_label"}
        assert win["sparse"].shape == (3, 3, L, px, px) and torch.equal(win["sparse"].cpu(), sparse)
        assert torch.equal(win["sparse_depth"].cpu(), torch.from_numpy(want["sparse_depth"]).repeat(3, 1, 1, 1, 1))
        assert torch.equal(win["dense"], dense[:, :, sel]) and win["class_label"].tolist() == [[0], [500], [1]]
        assert float((win["sparse_depth"] > -1).float().mean()) > 0.2                                   # something was drawn
    sm = cfgs.SAMPLER
    outs = synthesize_windows(model, wins, [3, 4, L, shp["H"], shp["W"]], video_length=L, ddim_steps=2, ddim_eta=1.0,
                              unconditional_guidance_scale=sm["cfg_scale"], fs=sm["fs"], timestep_spacing=sm["spacing"],
                              guidance_rescale=sm["guidance_rescale"])
    torch.cuda.synchronize()
    assert len(outs) == 2
    for out in outs:
        assert out.shape == (3, 1, 3, L, px, px) and torch.isfinite(out).all() and float(out.abs().max()) <= 1.0
    # a (4, 4) camera-from-virtual-camera matrix is the same pose
    left = np.eye(4)
    left[0, 3] = -2.0
    first = next(iter(render_windows(scene, dense, pose=left, video_length=L)))
    assert torch.equal(first["sparse"], wins[0]["sparse"]) and torch.equal(first["sparse_depth"], wins[0]["sparse_depth"])
