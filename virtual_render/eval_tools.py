"""Tensor-level part of MuDG's result post-processing (reference: virtual_render/eval_tools.py) on the MI355X path: what
`save_virtual_{color,depth,semantic}_results` compute before they hand pixels to the PNG / NPY writers.  The writers and the mp4
export are host I/O outside the path.  The depth colour map is not: for "Spectral" the reference's `colormap` takes its torch-only
`method_custom` branch (eleven table colours and a linear blend, no matplotlib), and that rule runs here as a kernel.

  frames_to_uint8     eval_tools.py:22-27, 59-63, 109-113   clamp, (x + 1) / 2 * 255, truncate, (b c t h w) -> (b t h w c)
  depth_prediction    eval_tools.py:71                       channel mean of the uint8 frame / 255  -> (1, h, w) in [0, 1]
  visualize_semantic  eval_tools.py:309-347                  nearest of the 19 class colours; same signature and return
  colormap            eval_tools.py:137-261                  "Spectral" / "Spectral_r", the reference's method_custom; same signature
  visualize_depth     eval_tools.py:264-306                  same signature; (H, W, 3) uint8 arrays where the reference returns PIL images
  aligned_depth       data_process/depthlab_tools.py:67-87, 114-136   the depth stream in metres: fitted to the LiDAR depth, sky at 100 m
  score_window        (none: the reference only saves files)          PSNR / SSIM, depth errors and class IoU of a window
"""
import numpy as np
import torch

from mudg_amd import depth as _depth
from mudg_amd import metrics as _metrics
from mudg_amd import ops

_COLOR_MAPS = ("Spectral", "Spectral_r")


def frames_to_uint8(video):
    """(b, c, t, h, w) samples -> (b, t, h, w, c) uint8 like `grid` in the reference's save functions."""
    return ops.frames_to_uint8(video)


def depth_prediction(grid_frame):
    """(h, w, 3) uint8 frame of the depth stream -> (1, h, w) fp32 depth in [0, 1] (`result_pred`, eval_tools.py:71)."""
    return ops.depth_from_uint8(grid_frame)


def visualize_semantic(semantic, return_pt=False):
    """(3, H, W) uint8 -> (recoloured (H, W, 3) [or (3, H, W) tensor with return_pt], labels (H, W)) as eval_tools.py:309-347:
    numpy arrays by default, torch tensors with return_pt=True."""
    if not torch.is_tensor(semantic):
        semantic = torch.as_tensor(semantic)
    vis, lab = ops.semantic_nearest(semantic.to(torch.uint8).cuda() if not semantic.is_cuda else semantic.to(torch.uint8))
    if return_pt:
        return vis, lab
    return vis.permute(1, 2, 0).cpu().numpy(), lab.cpu().numpy()


def colormap(image, cmap="Spectral", bytes=False):
    """Values in [0, 1] (a torch tensor or a numpy array of any shape; uint8 means value / 255) -> their colours, shape + (3,): fp32, or
    uint8 with bytes=True, as the reference's `colormap` returns them for "Spectral" (its method_custom, bit for bit).  A numpy array
    comes back as a numpy array, a tensor stays where the kernel wrote it (on the GPU).  Only "Spectral" and "Spectral_r" exist here:
    every other map of the reference goes through matplotlib, which is not part of this path."""
    if not (torch.is_tensor(image) or isinstance(image, np.ndarray)):
        raise ValueError("Argument must be a numpy array or torch tensor.")
    if cmap not in _COLOR_MAPS:
        raise ValueError(f"Unexpected color map {cmap!r}: only {' and '.join(repr(c) for c in _COLOR_MAPS)} are supported")
    values = torch.as_tensor(image)
    if values.dtype == torch.uint8:                                          # image.float() / 255: 256 values, divided once on the host
        values = (torch.arange(256, dtype=torch.uint8).float() / 255).cuda()[values.cuda().long()]
    out = ops.colormap_spectral(values.float().cuda().contiguous(), reversed=cmap.endswith("_r"), bytes=bytes)
    return out.cpu().numpy() if isinstance(image, np.ndarray) else out


def visualize_depth(depth, val_min=0.0, val_max=1.0, color_map="Spectral"):
    """Depth maps ((H, W) or (N, H, W), a numpy array, a tensor or a list of either) -> a list of (H, W, 3) uint8 numpy arrays, the
    Spectral pictures of (depth - val_min) / (val_max - val_min).  The reference returns PIL images of the same bytes; PIL is host
    I/O and stays with the caller (PIL.Image.fromarray takes the arrays as they are)."""
    if depth is None or isinstance(depth, list) and any(o is None for o in depth):
        raise ValueError("Input depth is `None`")
    if color_map not in _COLOR_MAPS:
        raise ValueError(f"Unexpected color map {color_map!r}: only {' and '.join(repr(c) for c in _COLOR_MAPS)} are supported")
    if val_max <= val_min:
        raise ValueError(f"Invalid values range: [{val_min}, {val_max}].")
    if not isinstance(depth, list) and depth.ndim == 2:
        depth = depth[None, ...]
    out = []
    for img in depth:
        values = torch.as_tensor(img).float().cuda().contiguous()
        out.append(ops.colormap_spectral(values, val_min, val_max, reversed=color_map.endswith("_r")).cpu().numpy())
    return out


def aligned_depth(grid_frames, lidar_depth, labels=None):
    """(T, H, W, 3) uint8 frames of the depth stream and the LiDAR depth (T, H, W) fp32 metres at the same pose -> (T, H, W) fp32
    metres: align_depth's least-squares line per frame, then process_sky's 100 m on class 10 and its clip to [0, 100]
    (mudg_amd.depth.metric_depth, which also returns the line and whether a frame could be fitted)."""
    return _depth.metric_depth(grid_frames, lidar_depth, labels)["depth"]


def score_window(outputs, *, color=None, lidar_depth=None, labels=None, **options):
    """window_outputs' dict and whichever ground truths there are -> "color_psnr", "color_ssim", "depth_mae", ..., "semantic_miou", ... as
    small tensors on the GPU (mudg_amd.metrics.score_window)."""
    return _metrics.score_window(outputs, color=color, lidar_depth=lidar_depth, labels=labels, **options)
