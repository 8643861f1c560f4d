"""Metric depth from the generated depth stream, and generated views lifted to points: the way back from "clips" to "scene".

The reference turns a relative depth map into metres with a host least-squares fit against the LiDAR depth (align_depth,
data_process/depthlab_tools.py:114-136), sets the sky to 100 m and clips (process_sky, :67-87), draws the result with the Spectral colour
map (virtual_render/eval_tools.py:137-306) and puts a second cloud beside the LiDAR one (data_process/tools/merge_points.py:77-90).
Here the generated frames, the class labels and the LiDAR depth rendered at the same virtual pose are already on the GPU, and
csrc/depth.hip does the rest: integer sums per frame, a one-lane solve, one pass that writes metres and the picture, and one pass that
lifts every pixel to a packed world-space point.  DESIGN.md §14 states the rules and every deviation.  Nothing comes to the host on the
way, and there is no CPU fallback: tensors that are not on the GPU are an error.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip, ops, render

SKY_LABEL = 10                   # depthlab_tools.py:80
MAX_DEPTH = 100.0                # depthlab_tools.py:81-83; the dataset normalises by the same 100 m (lvdm/data/waymo_data.py:328)


def _on_gpu(name, what, t, dtype, shape=None):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)):
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise hip.MudgError(f"{name}: {what} is a {dtype} tensor on the GPU" + (f" of shape {tuple(shape)}" if shape else "") + f" (there is no CPU path), got {got}")
    return t.contiguous()


def metric_depth(depth_frames_u8, lidar_depth, labels=None, *, sky_label=SKY_LABEL, visualise=False):
    """One stream's depth in metres.  depth_frames_u8: (T, H, W, 3) uint8, the depth stream as ops.frames_to_uint8 returns it;
    lidar_depth: (T, H, W) fp32 metres at the same pose, 0 where no return landed (render_conditions(..., return_images=True)["depth"]);
    labels: (T, H, W) int64 classes of ops.semantic_nearest or None (no sky rule).

    Returns {"depth": (T, H, W) fp32 metres in [0, 100], "coef": (T, 2) float64 (m, c) of lidar ~ m * relative + c per frame,
    "fitted": (T,) uint8 — 0 where a frame had fewer than two usable pixels or no spread, and (m, c) = (100, 0)}, with visualise also
    "vis": (T, H, W, 3) uint8, the Spectral picture of depth / 100."""
    frames = _on_gpu("metric_depth", "the depth stream", depth_frames_u8, torch.uint8)
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise hip.MudgError(f"metric_depth: expected (T, H, W, 3) frames, got {tuple(frames.shape)}")
    shape = tuple(frames.shape[:3])
    lidar = _on_gpu("metric_depth", "the LiDAR depth", lidar_depth, torch.float32, shape)
    if labels is not None:
        labels = _on_gpu("metric_depth", "the label image", labels, torch.int64, shape)
    coef, fitted = ops.depth_align_solve(ops.depth_align_sums(frames, lidar))
    depth, vis = ops.depth_finish(frames, coef, labels, sky_label=sky_label, visualise=visualise)
    out = {"depth": depth, "coef": coef, "fitted": fitted}
    if visualise:
        out["vis"] = vis
    return out


def camera_table(intr, c2w, hw_native, hw_out):
    """Host, float64: (T, 16) — the top three rows of every frame's camera-to-world matrix, then render.scaled_intrinsics."""
    c2w = np.asarray(c2w, dtype=np.float64)
    if c2w.ndim != 3 or c2w.shape[1:] != (4, 4):
        raise hip.MudgError(f"lift_views: cameras {c2w.shape}, expected (T, 4, 4)")
    intr = np.broadcast_to(np.asarray(intr, dtype=np.float64), (c2w.shape[0], 3, 3))
    return np.stack([np.concatenate([c2w[t, :3].reshape(12), render.scaled_intrinsics(intr[t], hw_native, hw_out)]) for t in range(c2w.shape[0])])


def normals_from_depth(depth, intr, hw_native, labels=None, *, sky_label=SKY_LABEL, min_depth=0.0, max_depth=MAX_DEPTH, max_rel_step=None):
    """Camera-space surface normals of depth maps (OpenCV camera: x right, y down, z forward).  depth: (F, H, W) fp32
    metres (metric_depth's, or a dense depth map); intr: (3, 3) or (F, 3, 3) at hw_native; labels: (F, H, W) int64 or None.  A pixel is
    usable iff min_depth < depth < max_depth and it is not sky; the normal is dy x dx over central differences of the unprojected points,
    one-sided where only one neighbour is usable — and, with max_rel_step = r, only where |z_nb - z| <= r z, so that a depth edge takes
    the side that lies on the surface.  A surface seen from the camera has n . P < 0 (a wall facing it: (0, 0, -1)); no flip is applied.
    Returns (normals (F, H, W, 3) fp32 of unit length, valid (F, H, W) uint8); a pixel that is not valid holds (0, 0, 0)."""
    depth = _on_gpu("normals_from_depth", "the depth", depth, torch.float32)
    if depth.dim() != 3:
        raise hip.MudgError(f"normals_from_depth: expected (F, H, W) depths, got {tuple(depth.shape)}")
    if labels is not None:
        labels = _on_gpu("normals_from_depth", "the label image", labels, torch.int64, depth.shape)
    intr = np.asarray(intr, dtype=np.float64)
    if intr.shape not in ((3, 3), (depth.shape[0], 3, 3)):
        raise hip.MudgError(f"normals_from_depth: intrinsics {intr.shape} for {depth.shape[0]} frames, expected (3, 3) or (F, 3, 3)")
    intr = np.broadcast_to(intr, (depth.shape[0], 3, 3))
    table = np.stack([render.scaled_intrinsics(k, hw_native, depth.shape[1:]) for k in intr])
    return ops.depth_normals(depth, torch.from_numpy(table).to(depth.device), labels, sky_label=sky_label, min_depth=min_depth,
                             max_depth=max_depth, max_rel_step=max_rel_step)


def lift_views(depth, rgb, intr, c2w, hw_native, labels=None, *, min_depth=0.0, max_depth=MAX_DEPTH, sky_label=SKY_LABEL):
    """Generated views as coloured world-space points in the renderer's packed format.  depth: (T, H, W) fp32 metres; rgb: (T, H, W, 3)
    uint8; intr: (3, 3) or (T, 3, 3) at hw_native; c2w: (T, 4, 4), the poses the views were generated at (OpenCV convention);
    labels: (T, H, W) int64 or None.  A pixel becomes a point iff min_depth < depth < max_depth and it is not sky — with the defaults
    the sky's 100 m is out.  Returns a render.PointCloud in (frame, row, column) order."""
    rgb = _on_gpu("lift_views", "the colour stream", rgb, torch.uint8)
    if rgb.dim() != 4 or rgb.shape[3] != 3:
        raise hip.MudgError(f"lift_views: expected (T, H, W, 3) colours, got {tuple(rgb.shape)}")
    shape = tuple(rgb.shape[:3])
    depth = _on_gpu("lift_views", "the depth", depth, torch.float32, shape)
    if labels is not None:
        labels = _on_gpu("lift_views", "the label image", labels, torch.int64, shape)
    table = camera_table(intr, c2w, hw_native, shape[1:])
    if table.shape[0] != shape[0]:
        raise hip.MudgError(f"lift_views: {table.shape[0]} cameras for {shape[0]} frames")
    points, valid = ops.depth_unproject(depth, rgb, torch.from_numpy(table).to(rgb.device), labels, sky_label=sky_label, min_depth=min_depth,
                                        max_depth=max_depth)
    return render.PointCloud(points[valid.bool()])                           # stable: (frame, row, column) order
