#!/usr/bin/env python3
"""Capture the fixture of the metric-depth rules from the REFERENCE implementation: virtual_render/eval_tools.py's colormap (:137-261)
and visualize_depth (:264-306), data_process/depthlab_tools.py's align_depth (:114-136), and the two inline expressions of its
process_sky (:80-83, which reads files around them).

Run in the build container only:   python tests/golden/make_golden_depth.py
The reference is found the way make_golden_splat.py finds it (make_golden.py is loaded for that; none of its goldens is rewritten), and
eval_tools.py is loaded the way golden_postprocess loads it.  depthlab_tools.py imports diffusers, transformers, cv2, tqdm and modules of
the DepthLab checkout at its top: all of them are replaced by empty stand-in modules before it is executed; align_depth itself is numpy.
Only tensors are stored (tests/golden/depth_post.pt).

  colour map   a seeded (3, 24, 32) fp32 batch holding 0, 1, values outside [0, 1], every j / 10 and the fp32 neighbours of each j / 10
               on either side: bytes and floats of "Spectral", the floats' bytes of "Spectral_r" (forced through method_custom, which
               is the only branch this project reproduces), visualize_depth with the default range and with (val_min, val_max) = (2, 50)
  alignment    two 24 x 32 frames of seeded uint8 triples (a few of them black), LiDAR depths = 80 u + 2 + noise in fp32 with about
               15 % of the pixels zero; u is the reference's own expression for the relative depth (eval_tools.py:72)
  sky          a seeded depth map with values below 0 and above 100 and a float class image with a block of class 10"""
import importlib.util
import os
import sys
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

SEED = 20270
H, W = 24, 32


def stand_in(name, *attrs):
    """An empty module under `name` (and under every parent that is not there yet) with the given attributes set to None."""
    parts = name.split(".")
    for n in range(1, len(parts) + 1):
        key = ".".join(parts[:n])
        if n == len(parts) or key not in sys.modules:
            sys.modules[key] = types.ModuleType(key)
        if n > 1:
            setattr(sys.modules[".".join(parts[:n - 1])], parts[n - 1], sys.modules[key])
    for a in attrs:
        setattr(sys.modules[name], a, None)


def load_reference(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(mg.REF, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def main():
    tvio = types.ModuleType("torchvision.io")                               # as golden_postprocess does
    sys.modules["torchvision"].io = tvio
    sys.modules["torchvision.io"] = tvio
    import PIL.Image                                                          # noqa: F401  (eval_tools.py uses PIL.Image after a bare `import PIL`)
    et = load_reference(("virtual_render", "eval_tools.py"), "ref_eval_tools")
    stand_in("tqdm.auto", "tqdm")
    stand_in("diffusers", "DDIMScheduler", "AutoencoderKL")
    stand_in("transformers", "CLIPTextModel", "CLIPTokenizer", "CLIPVisionModelWithProjection")
    stand_in("src.models.unet_2d_condition", "UNet2DConditionModel")
    stand_in("src.models.unet_2d_condition_main", "UNet2DConditionModel_main")
    stand_in("src.models.projection", "My_proj")
    stand_in("inference.depthlab_pipeline", "DepthLabPipeline")
    stand_in("utils.seed_all", "seed_all")
    stand_in("utils.image_util", "get_filled_for_latents")
    dt = load_reference(("data_process", "depthlab_tools.py"), "ref_depthlab_tools")

    rng = np.random.default_rng(SEED)
    out = {}

    # ---- the colour map
    x = rng.uniform(-0.2, 1.2, (3, H, W)).astype(np.float32)
    tenths = (np.arange(11, dtype=np.float32) / np.float32(10))
    special = np.concatenate([tenths, np.nextafter(tenths, np.float32(-1)), np.nextafter(tenths, np.float32(2)),
                              np.float32([0.0, 1.0, -0.5, 1.5, -0.0, 1e-30, 0.99999994])])
    x.reshape(-1)[:len(special)] = special
    x[1].reshape(-1)[:11] = np.float32([j / 10 for j in range(11)])         # the doubles j / 10 rounded, should they differ
    xt = torch.from_numpy(x)
    out["cm_in"] = xt.clone()
    out["cm_bytes"] = et.colormap(xt, cmap="Spectral", bytes=True)
    out["cm_floats"] = et.colormap(xt, cmap="Spectral", bytes=False)
    out["cm_r_bytes"] = et.colormap(xt, cmap="Spectral_r", bytes=True, _force_method="custom")
    out["cm_r_floats"] = et.colormap(xt, cmap="Spectral_r", bytes=False, _force_method="custom")
    out["vd_default"] = t(np.stack([np.array(im) for im in et.visualize_depth(x)]))
    metres = rng.uniform(0.0, 55.0, (2, H, W)).astype(np.float32)
    metres[0, 0, :4] = np.float32([2.0, 50.0, 1.0, 26.0])
    out["vd_in"] = t(metres)
    out["vd_range"] = torch.tensor([2.0, 50.0], dtype=torch.float64)
    out["vd_bytes"] = t(np.stack([np.array(im) for im in et.visualize_depth(metres, val_min=2.0, val_max=50.0)]))
    assert out["cm_bytes"].dtype == torch.uint8 and out["cm_floats"].dtype == torch.float32 and torch.equal(out["vd_default"], out["cm_bytes"])

    # ---- the alignment
    frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    frames[0, 3, 5:9] = 0                                                    # black: not in the fit
    grid = torch.from_numpy(frames)
    u = torch.stack([torch.mean(grid[i].permute(2, 0, 1).float(), dim=0, keepdim=True) / 255 for i in range(2)])   # eval_tools.py:72, (2, 1, h, w)
    lidar = (80.0 * u[:, 0].numpy().astype(np.float64) + 2.0 + rng.normal(0.0, 0.5, (2, H, W)))
    lidar = np.maximum(lidar, 0.1).astype(np.float32)
    lidar[rng.random((2, H, W)) < 0.15] = 0.0
    aligned = np.stack([dt.align_depth(lidar[i].copy(), u[i].numpy().copy()) for i in range(2)])
    assert aligned.dtype == np.float64 and aligned.shape == (2, H, W)
    out.update({"align_frames": grid.clone(), "align_u": u.clone(), "align_lidar": t(lidar), "aligned": t(aligned)})

    # ---- the sky: process_sky's expressions (depthlab_tools.py:80-83)
    depth = rng.uniform(-20.0, 140.0, (H, W)).astype(np.float32)
    semantic = rng.integers(0, 19, (H, W)).astype(np.float32)              # read_semantic_pfm returns the class image as floats
    semantic[:6, 10:20] = 10.0
    out["sky_in"], out["sky_semantic"] = t(depth.copy()), t(semantic)
    mask = semantic == 10  # sky mask
    depth[mask] = 100
    depth = np.clip(depth, 0, 100)
    out["sky_out"] = t(depth)
    out["sky_vis"] = t(np.array(et.visualize_depth(depth / 100)[0]))

    assert all(torch.is_tensor(v) for v in out.values())
    path = os.path.join(HERE, "depth_post.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
