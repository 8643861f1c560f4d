"""Scores of generated views against the truths that are already on the GPU: PSNR and SSIM for colour, depth errors against the rendered
LiDAR depth, class IoU for the semantic stream, angular errors for the normal stream — and, against no truth at all, how far the views
of a window agree with one another (view_consistency).  A fused cloud is scored against the scene's LiDAR cloud by
cloud_scores: accuracy, completeness and F-score at distance thresholds and the mean nearest-neighbour distances.

The reference has no scoring code (its eval_tools.py writes files, its validation_step logs the loss); its paper reports these
numbers.  The rules here are this project's own and DESIGN.md §15 states them: every kernel of csrc/metrics.hip reduces a frame to a
few integers that do not depend on the order of execution, and the scores are formed from those integers in float64 on the device.
Results are small device tensors, nothing synchronises, and there is no CPU fallback: tensors that are not on the GPU are an error.
"""
from __future__ import annotations

import torch

from . import hip, ops
from .depth import _on_gpu

MIN_DEPTH, MAX_DEPTH = 0.1, 80.0          # the range of LiDAR depths that depth errors are taken over
CLASSES = 19                              # ops.semantic_nearest's classes
_D = torch.float64


def _frames(name, a, b):
    a = _on_gpu(name, "the first frame stack", a, torch.uint8)
    if a.dim() != 4 or a.shape[3] != 3:
        raise hip.MudgError(f"{name}: expected (F, H, W, 3) frames, got {tuple(a.shape)}")
    return a, _on_gpu(name, "the second frame stack", b, torch.uint8, a.shape)


def psnr_ssim(a_u8, b_u8):
    """Two (F, H, W, 3) uint8 frame stacks (ops.frames_to_uint8's, window_outputs' "color"), H, W >= 11.  Returns {"psnr": (F,) float64 =
    10 log10(255^2 3 H W / sse), inf where the frames are equal; "ssim": (F,) float64, the mean over the valid region and the channels;
    "sse", "ssim_sum": (F,) int64, the integers both come from}."""
    a, b = _frames("psnr_ssim", a_u8, b_u8)
    f, h, w = a.shape[:3]
    if h < 11 or w < 11:
        raise hip.MudgError(f"psnr_ssim: {h} x {w} frames, SSIM's 11 x 11 window needs at least 11 x 11")
    sse, ssim_sum = ops.metric_sse(a, b), ops.metric_ssim(a, b)
    const = lambda v: torch.full((), float(v), dtype=_D, device=a.device)    # a device tensor: dividing by a Python number multiplies by its reciprocal
    psnr = 10.0 * torch.log10(const(255.0 ** 2 * 3 * h * w) / sse.to(_D))
    ssim = ssim_sum.to(_D) / const(2.0 ** 32 * (3 * (h - 10) * (w - 10)))
    return {"psnr": psnr, "ssim": ssim, "sse": sse, "ssim_sum": ssim_sum}


def depth_errors(depth, lidar_depth, *, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH):
    """depth: (F, H, W) fp32 metres (metric_depth's, window_outputs' "depth"); lidar_depth: (F, H, W) fp32 metres, 0 where no return
    landed.  Over the pixels with min_depth < lidar < max_depth whose depth is a number, per frame in float64: {"n" (int64), "mae",
    "rmse", "abs_rel", "d1", "d2", "d3" (the shares with max(z / y, y / z) < 1.25, 1.25^2, 1.25^3), "sums": (F, 8) int64}; a frame without
    such a pixel scores nan."""
    depth = _on_gpu("depth_errors", "the depth", depth, torch.float32)
    if depth.dim() != 3:
        raise hip.MudgError(f"depth_errors: expected (F, H, W) depths, got {tuple(depth.shape)}")
    lidar = _on_gpu("depth_errors", "the LiDAR depth", lidar_depth, torch.float32, depth.shape)
    sums = ops.metric_depth(depth, lidar, min_depth=min_depth, max_depth=max_depth)
    s = sums.to(_D)
    n = s[:, 0]                                                              # 0 / 0 = nan: a frame with nothing counted
    return {"n": sums[:, 0], "mae": s[:, 1] / (2.0 ** 20 * n), "rmse": torch.sqrt(s[:, 2] / (2.0 ** 20 * n)), "abs_rel": s[:, 3] / (2.0 ** 20 * n),
            "d1": s[:, 4] / n, "d2": s[:, 5] / n, "d3": s[:, 6] / n, "sums": sums}


def segmentation_scores(pred_labels, gt_labels, *, classes=CLASSES):
    """Two (F, H, W) int64 label maps in ops.semantic_nearest's format.  Returns {"confusion": (F, classes, classes) int64, [gt][pred];
    "iou": (F, classes) float64, nan for a class in neither map; "miou": (F,) the mean over the defined classes; "pixel_acc": (F,);
    "bad": (F,) int64, predictions outside [0, classes), which are in no cell}.  Ground truth outside [0, classes) (255, -1) is ignored."""
    pred = _on_gpu("segmentation_scores", "the predicted labels", pred_labels, torch.int64)
    if pred.dim() != 3:
        raise hip.MudgError(f"segmentation_scores: expected (F, H, W) labels, got {tuple(pred.shape)}")
    gt = _on_gpu("segmentation_scores", "the ground-truth labels", gt_labels, torch.int64, pred.shape)
    confusion, bad = ops.metric_confusion(pred, gt, classes)
    c = confusion.to(_D)
    diag = torch.diagonal(c, dim1=1, dim2=2)
    iou = diag / (c.sum(2) + c.sum(1) - diag)                                # 0 / 0 = nan: the class is in neither map
    defined = ~torch.isnan(iou)
    miou = torch.where(defined, iou, torch.zeros_like(iou)).sum(1) / defined.sum(1).to(_D)
    return {"confusion": confusion, "iou": iou, "miou": miou, "pixel_acc": diag.sum(1) / (c.sum((1, 2)) + bad.to(_D)), "bad": bad}


def normal_errors(pred_u8, gt_normals, valid=None):
    """pred_u8: (F, H, W, 3) uint8, a generated normal stream as ops.frames_to_uint8 returns it; gt_normals: (F, H, W, 3) fp32
    (normals_from_depth's, or loaded maps); valid: (F, H, W) uint8 or None.  The angle between 2 u - 255 and the truth, binned per frame
    into quarter degrees by its cosine, over the pixels whose validity byte is nonzero and whose truth has a finite
    positive length.  Per frame: {"n" (int64), "mean" (over bin centres: within 0.125 degrees of the mean angle), "median" (the centre of
    the bin that holds the lower median), "a11", "a22", "a30" (the shares below 11.25, 22.5 and 30 degrees, which are bin edges: exact),
    "hist": (F, 720) int64}, degrees in float64; a frame with nothing counted scores nan."""
    pred = _on_gpu("normal_errors", "the normal stream", pred_u8, torch.uint8)
    if pred.dim() != 4 or pred.shape[3] != 3:
        raise hip.MudgError(f"normal_errors: expected (F, H, W, 3) frames, got {tuple(pred.shape)}")
    gt = _on_gpu("normal_errors", "the true normals", gt_normals, torch.float32, pred.shape)
    if valid is not None:
        valid = _on_gpu("normal_errors", "the validity bytes", valid, torch.uint8, pred.shape[:3])
    hist = ops.metric_normals(pred, gt, valid)
    below = hist.cumsum(1)                                                   # integers: the pixels of bins 0 .. k
    counted = below[:, -1]
    n = counted.to(_D)                                                       # 0 / 0 = nan: a frame with nothing counted
    odd = 2 * torch.arange(ops.NORMAL_BINS, device=hist.device) + 1         # bin k's centre is (2 k + 1) / 8 degrees
    middle = (2 * below >= counted[:, None]).to(torch.uint8).argmax(1)      # the first bin at which half the pixels are reached
    nan = torch.full_like(n, float("nan"))
    return {"n": counted, "mean": (hist * odd).sum(1).to(_D) / (8.0 * n), "median": torch.where(counted > 0, (2 * middle + 1).to(_D) / 8.0, nan),
            "a11": below[:, 44].to(_D) / n, "a22": below[:, 89].to(_D) / n, "a30": below[:, 119].to(_D) / n, "hist": hist}


def view_consistency(result):
    """result: depth.consistent_views' dict (or its "stats", (V, 6) int64).  The one score of a generated window that needs no truth
    (DESIGN.md §21), from the integer counts, as Python floats: {"tested": the share of each view's usable pixels that some witness gave
    a verdict on, "kept": the share kept, "violated": the share a witness saw through, "mean_agree": agreeing witnesses per tested
    pixel — each a list of V floats — and "overall": the same four over all views}; nan where nothing was usable (or tested).  Brings
    V x 6 integers to the host."""
    stats = result["stats"] if isinstance(result, dict) else result
    stats = _on_gpu("view_consistency", "the statistics", stats, torch.int64)
    if stats.dim() != 2 or stats.shape[1] != 6:
        raise hip.MudgError(f"view_consistency: expected (V, 6) statistics, got {tuple(stats.shape)}")
    rows = stats.cpu().tolist()
    share = lambda a, b: a / b if b else float("nan")
    one = lambda s: {"tested": share(s[1], s[0]), "kept": share(s[2], s[0]), "violated": share(s[5], s[0]), "mean_agree": share(s[3], s[1])}
    views = [one(s) for s in rows]
    scores = {k: [v[k] for v in views] for k in ("tested", "kept", "violated", "mean_agree")}
    scores["overall"] = one([sum(s[k] for s in rows) for k in range(6)])
    return scores


def cloud_scores(pred, truth, thresholds=(0.05, 0.1, 0.2, 0.5)):
    """Two render.PointClouds — a reconstruction (depth.fuse_views') and a truth (cloud.build_scene_clouds' background) — and up to
    eight ascending distance thresholds in metres, each in (0, 64].  Every point looks for its nearest neighbour in the
    other cloud within max(thresholds): pred in truth for accuracy, truth in pred for completeness.  Returns {"accuracy", "completeness":
    (K,) float64, the shares of all points with a neighbour within each threshold; "fscore": 2 a c / (a + c), nan at 0 / 0; "found":
    (2,) the shares with a neighbour within the radius at all; "mean_accuracy", "mean_completeness": the mean distance in metres over
    the found points (on a 2^-20 grid, rounded down; nan when nothing is found); "chamfer": their sum; "sums": (2, 2 + K) int64, the
    integers everything comes from}."""
    from . import cloud, render
    if not isinstance(pred, render.PointCloud) or not isinstance(truth, render.PointCloud):
        raise hip.MudgError("cloud_scores: expected two render.PointClouds (on the GPU; there is no CPU path)")
    try:
        th = [float(t) for t in thresholds]
    except (TypeError, ValueError):
        raise hip.MudgError(f"cloud_scores: thresholds {thresholds!r}") from None
    if not 1 <= len(th) <= ops.CLOUD_MAX_THRESHOLDS or not all(0.0 < t <= ops.NEIGHBOUR_MAX_RADIUS for t in th) or any(b <= a for a, b in zip(th, th[1:])):
        raise hip.MudgError(f"cloud_scores: thresholds {thresholds!r} (1 .. {ops.CLOUD_MAX_THRESHOLDS} ascending distances in (0, {ops.NEIGHBOUR_MAX_RADIUS:g}])")
    if len(pred) == 0 or len(truth) == 0:
        raise hip.MudgError(f"cloud_scores: clouds of {len(pred)} and {len(truth)} points")
    radius, t2 = th[-1], [t * t for t in th]
    rows = []
    for queries, reference in ((pred, truth), (truth, pred)):
        grid = cloud.NeighbourGrid.build(reference, radius)
        rows.append(ops.metric_cloud(cloud.nearest(grid, queries)[0], t2, grid.r2))
    sums = torch.stack(rows)
    s = sums.to(_D)
    const = lambda v: torch.full((), float(v), dtype=_D, device=sums.device)
    total = torch.stack([const(len(pred)), const(len(truth))])
    share = s[:, 2:] / total[:, None]
    a, c = share[0], share[1]
    mean = s[:, 1] / (const(2.0 ** 20) * s[:, 0])                            # 0 / 0 = nan: nothing found
    return {"accuracy": a, "completeness": c, "fscore": (2.0 * a * c) / (a + c), "found": s[:, 0] / total, "mean_accuracy": mean[0],
            "mean_completeness": mean[1], "chamfer": mean[0] + mean[1], "sums": sums}


def score_window(outputs, *, color=None, lidar_depth=None, labels=None, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, classes=CLASSES):
    """outputs: the dict virtual_render.virtual_pose_render.window_outputs returns; color: (T, H, W, 3) uint8, the camera frames;
    lidar_depth: (T, H, W) fp32 metres at the window's pose; labels: (T, H, W) int64.  Returns the union of psnr_ssim, depth_errors and
    segmentation_scores for the truths that were given, keyed "color_*", "depth_*" and "semantic_*"; an absent truth adds no key."""
    scores = {}
    if color is not None:
        scores.update({"color_" + k: v for k, v in psnr_ssim(outputs["color"], color).items()})
    if lidar_depth is not None:
        scores.update({"depth_" + k: v for k, v in depth_errors(outputs["depth"], lidar_depth, min_depth=min_depth, max_depth=max_depth).items()})
    if labels is not None:
        scores.update({"semantic_" + k: v for k, v in segmentation_scores(outputs["semantic_labels"], labels, classes=classes).items()})
    return scores
