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


def window_frames(frame, n_frames, window=(-2, 3)):
    """The sweeps pooled for a frame (get_6frames_lidar, data_process/pipeline_depth.py:63-67, restated): frame + window[0] ..
    frame + window[1], each replaced by the frame itself when it falls outside [0, n_frames)."""
    return [f if 0 <= f < n_frames else frame for f in range(frame + window[0], frame + window[1] + 1)]


def lidar_depth_maps(sweeps, objects, intr, c2w, hw_native, hw_out=None, *, frame_ids=None, window=(-2, 3), point_size=2.0, occlusion=True,
                     reach=4, rel_tol=0.05, occluder_size=1.0, znear=render.ZNEAR, zfar=render.ZFAR):
    """The reference's "six_frames_depth" (data_process/pipeline_depth.py:63-152).  sweeps: a render.FrameSweeps
    (cloud.frame_sweeps); objects: a render.ObjectSet or None; intr (3, 3) or (T, 3, 3) at hw_native; c2w (T, 4, 4), the camera in the
    T frames asked for; frame_ids: their numbers in the sweeps and the objects' tables (default 0 .. T-1); hw_out: None for native.

    A frame's candidates are the sweeps of window_frames (a frame that occurs twice counts once: the result cannot differ) and the
    points of the objects visible at the frame.  They are projected, culled and drawn by §12's rule at point_size, except those the
    occlusion test hides: all candidates are first drawn at occluder_size into a buffer Z, and a point with camera depth zc and home
    pixel (floor(v), floor(u)) is hidden iff along one of the four lines through the home pixel (row, column, both diagonals) there is
    on BOTH sides, within `reach` pixels, a pixel whose Z depth is below zc (1 - rel_tol).  This image-space rule stands in for the
    reference's Open3D hidden_point_removal and is this project's own.  Returns (T, H, W) fp32 metres, 0 where nothing landed."""
    depth, passes = _lidar_depth_passes(sweeps, objects, intr, c2w, hw_native, hw_out, frame_ids=frame_ids, window=window, point_size=point_size,
                                       occlusion=occlusion, reach=reach, rel_tol=rel_tol, occluder_size=occluder_size, znear=znear, zfar=zfar)
    for occluders, visible in passes:
        occluders()
        visible()
    return depth


def _lidar_depth_passes(sweeps, objects, intr, c2w, hw_native, hw_out=None, *, frame_ids=None, window=(-2, 3), point_size=2.0, occlusion=True,
                       reach=4, rel_tol=0.05, occluder_size=1.0, znear=render.ZNEAR, zfar=render.ZFAR):
    """lidar_depth_maps' arguments, checked, and its work laid out: (depth (T, H, W), [(occluders, visible)] per frame) — calling every
    pair in order fills depth.  occluders() draws the frame's candidates into Z (nothing without occlusion); visible() draws those Z does
    not hide and resolves into depth[t], which leaves both key images empty.  tools/lidar_depth_bench.py times the two apart."""
    if not isinstance(sweeps, render.FrameSweeps) or (objects is not None and not isinstance(objects, render.ObjectSet)):
        raise hip.MudgError("lidar_depth_maps: the sweeps are a render.FrameSweeps and the objects a render.ObjectSet (on the GPU; there is no CPU path)")
    c2w = np.asarray(c2w, dtype=np.float64)
    if c2w.ndim != 3 or c2w.shape[1:] != (4, 4) or c2w.shape[0] == 0:
        raise hip.MudgError(f"lidar_depth_maps: cameras {c2w.shape}, expected (T > 0, 4, 4)")
    T = c2w.shape[0]
    frame_ids = list(range(T)) if frame_ids is None else [int(f) for f in frame_ids]
    n_frames = sweeps.frames
    if len(frame_ids) != T or min(frame_ids) < 0 or max(frame_ids) >= n_frames or (objects is not None and objects.frames != n_frames):
        raise hip.MudgError(f"lidar_depth_maps: frames {frame_ids} for {T} cameras, sweeps of {n_frames} frames"
                            + (f" and objects of {objects.frames}" if objects is not None else ""))
    intr = np.asarray(intr, dtype=np.float64)
    if intr.shape not in ((3, 3), (T, 3, 3)):
        raise hip.MudgError(f"lidar_depth_maps: intrinsics {intr.shape} for {T} frames, expected (3, 3) or (T, 3, 3)")
    intr = np.broadcast_to(intr, (T, 3, 3))
    window = tuple(int(v) for v in window)
    if len(window) != 2 or window[0] > window[1] or window[1] - window[0] >= ops.LIDAR_MAX_SEGMENTS:
        raise hip.MudgError(f"lidar_depth_maps: window {window} (first <= last, at most {ops.LIDAR_MAX_SEGMENTS} frames)")
    if not (isinstance(reach, int) and 1 <= reach <= ops.LIDAR_MAX_REACH) or not 0.0 <= float(rel_tol) < 1.0:
        raise hip.MudgError(f"lidar_depth_maps: reach {reach} (an integer, 1 .. {ops.LIDAR_MAX_REACH}) and rel_tol {rel_tol} (0 <= rel_tol < 1)")
    hw_out = hw_native if hw_out is None else hw_out
    H, W = (int(v) for v in hw_out)
    if H <= 0 or W <= 0:
        raise hip.MudgError(f"lidar_depth_maps: size {hw_out}")
    dev = sweeps.points.device

    w2c = np.linalg.inv(c2w)                                                              # host, float64; one upload for the call
    bg_mats = torch.from_numpy(np.ascontiguousarray(w2c[:, :3, :].reshape(T, 1, 12)).astype(np.float32)).to(dev)
    obj_mats = None
    if objects is not None:
        obj_mats = np.stack([objects.matrices(w2c[t:t + 1], frame_ids[t])[0] for t in range(T)]).reshape(T, -1, 12)
        obj_mats = torch.from_numpy(obj_mats.astype(np.float32)).to(dev)
    offsets = sweeps.offsets.tolist()
    depth = torch.empty((T, H, W), dtype=torch.float32, device=dev)
    keys = ops.splat_keys(1, H, W, dev)
    Z = ops.splat_keys(1, H, W, dev) if occlusion else None
    kw = dict(znear=znear, zfar=zfar)
    def frame(t):
        cam = render.scaled_intrinsics(intr[t], hw_native, hw_out).astype(np.float32)
        runs = []                                                                         # neighbouring frames are one run of the cloud
        for f in sorted(set(window_frames(frame_ids[t], n_frames, window))):
            if offsets[f + 1] > offsets[f]:
                if runs and runs[-1][0] + runs[-1][1] == offsets[f]:
                    runs[-1] = (runs[-1][0], runs[-1][1] + offsets[f + 1] - offsets[f])
                else:
                    runs.append((offsets[f], offsets[f + 1] - offsets[f]))
        total = sum(r[1] for r in runs)
        with_objects = objects is not None and bool(objects.visible(frame_ids[t]))

        def occluders():
            if not occlusion:
                return
            for a, n in runs:
                ops.splat_points(sweeps.points[a:a + n], bg_mats[t:t + 1], Z, cam, occluder_size, **kw)
            if with_objects:
                ops.splat_points(objects.cloud.points, obj_mats[t:t + 1], Z, cam, occluder_size, ids=objects.ids, **kw)

        def visible():
            test = dict(occluder_keys=Z[0] if occlusion else None, reach=reach, rel_tol=rel_tol, **kw)
            if runs:
                ops.lidar_splat_visible(sweeps.points, runs, bg_mats[t], keys[0], cam, point_size, **test)
            if with_objects:
                ops.lidar_splat_visible(objects.cloud.points, [(0, len(objects.cloud))], obj_mats[t], keys[0], cam, point_size, ids=objects.ids,
                                        index_base=total, **test)
            ops.lidar_depth_resolve(keys[0], depth[t], Z[0] if occlusion else None)
        return occluders, visible
    return depth, [frame(t) for t in range(T)]


def complete_depth(lidar_depth, labels=None, *, max_depth=MAX_DEPTH, extrapolate=True, sky_label=SKY_LABEL, return_source=False):
    """A sparse depth map made dense: the classical morphological completion of Ku et al. 2018 with this project's
    border rules, in place of the reference's learned inpainting model (DepthLab) — parity with either is not claimed.  lidar_depth:
    (T, H, W) fp32 metres, 0 where there is none (lidar_depth_maps'); labels: (T, H, W) int64 or None (no sky rule).  Inverted depths are
    dilated by a 13-pixel diamond, closed by 5 x 5, filled from 7 x 7, with extrapolate extended to the top of every column and filled
    from 31 x 31, then the 5 x 5 median and a 5 x 5 binomial blur over the filled pixels; the sky is max_depth.
    Returns (T, H, W) fp32 metres, 0 where nothing reached — with return_source also (T, H, W) uint8: 0 empty, 1 measured, 2 filled by
    the closing, 3 by the extension, 4 sky."""
    depth = _on_gpu("complete_depth", "the LiDAR depth", lidar_depth, torch.float32)
    if depth.dim() != 3:
        raise hip.MudgError(f"complete_depth: expected (T, H, W) depths, got {tuple(depth.shape)}")
    if labels is not None:
        labels = _on_gpu("complete_depth", "the label image", labels, torch.int64, depth.shape)
    return ops.depth_complete(depth, labels, max_depth=max_depth, extrapolate=extrapolate, sky_label=sky_label, return_source=return_source)


def depth_labels_from_lidar(scene, frame_ids, hw_out=None, labels=None, **kw):
    """The scene's own depth labels: lidar_depth_maps on scene.sweeps / scene.objects at the scene's camera, then complete_depth.
    scene: a render.Scene made with keep_sweeps=True; frame_ids: positions in the scene's frames; **kw goes to whichever of the two
    takes it.  Returns (lidar_depth, dense_depth, source); the dense map at native size is what frames.SceneFrames(images, depth=) takes."""
    if getattr(scene, "sweeps", None) is None:
        raise hip.MudgError("depth_labels_from_lidar: the scene has no sweeps (render.Scene.from_scenario(..., keep_sweeps=True) keeps them)")
    rows = [int(f) for f in frame_ids]
    dense_kw = {k: kw.pop(k) for k in ("max_depth", "extrapolate", "sky_label") if k in kw}
    intr = np.asarray(scene.intr, dtype=np.float64)
    lidar = lidar_depth_maps(scene.sweeps, scene.objects, intr if intr.ndim == 2 else intr[rows], np.asarray(scene.c2w)[rows], scene.hw_native, hw_out,
                             frame_ids=rows, **kw)
    dense, source = complete_depth(lidar, labels, return_source=True, **dense_kw)
    return lidar, dense, source


def lift_views(depth, rgb, intr, c2w, hw_native, labels=None, *, min_depth=0.0, max_depth=MAX_DEPTH, sky_label=SKY_LABEL, keep=None):
    """Generated views as coloured world-space points in the renderer's packed format.  depth: (T, H, W) fp32 metres; rgb: (T, H, W, 3)
    uint8; intr: (3, 3) or (T, 3, 3) at hw_native; c2w: (T, 4, 4), the poses the views were generated at (OpenCV convention);
    labels: (T, H, W) int64 or None.  A pixel becomes a point iff min_depth < depth < max_depth and it is not sky — with the defaults
    the sky's 100 m is out — and, with keep ((T, H, W) uint8: consistent_views' "keep"), keep is non-zero there.  Returns a render.PointCloud in
    (frame, row, column) order."""
    rgb = _on_gpu("lift_views", "the colour stream", rgb, torch.uint8)
    if rgb.dim() != 4 or rgb.shape[3] != 3:
        raise hip.MudgError(f"lift_views: expected (T, H, W, 3) colours, got {tuple(rgb.shape)}")
    shape = tuple(rgb.shape[:3])
    depth = _on_gpu("lift_views", "the depth", depth, torch.float32, shape)
    if labels is not None:
        labels = _on_gpu("lift_views", "the label image", labels, torch.int64, shape)
    if keep is not None:
        keep = _on_gpu("lift_views", "the keep bytes", keep, torch.uint8, shape)
    table = camera_table(intr, c2w, hw_native, shape[1:])
    if table.shape[0] != shape[0]:
        raise hip.MudgError(f"lift_views: {table.shape[0]} cameras for {shape[0]} frames")
    points, valid = ops.depth_unproject(depth, rgb, torch.from_numpy(table).to(rgb.device), labels, sky_label=sky_label, min_depth=min_depth,
                                        max_depth=max_depth)
    chosen = valid.bool() if keep is None else valid.bool() & (keep.reshape(-1) != 0)
    return render.PointCloud(points[chosen])                                 # stable: (frame, row, column) order


# ------------------------------------------------------------------------------------------------ cross-view consistency
def witness_table(c2w, source_table=None):
    """Host, float64: the top three rows of every view's world-to-camera matrix (cloud.inverse_rigid of c2w (V, 4, 4)), (V, 12) — with
    source_table (camera_table's (V, 16)) followed by its fx, fy, cx, cy: (V, 16), the witness rows of ops.view_consistency."""
    from . import cloud
    c2w = np.asarray(c2w, dtype=np.float64)
    if c2w.ndim != 3 or c2w.shape[1:] != (4, 4):
        raise hip.MudgError(f"witness_table: cameras {c2w.shape}, expected (V, 4, 4)")
    rows = np.stack([cloud.inverse_rigid(m).reshape(12) for m in c2w]) if len(c2w) else np.zeros((0, 12))
    if source_table is None:
        return rows
    source_table = np.asarray(source_table, dtype=np.float64)
    if source_table.shape != (c2w.shape[0], 16):
        raise hip.MudgError(f"witness_table: source table {source_table.shape} for {c2w.shape[0]} cameras")
    return np.concatenate([rows, source_table[:, 12:]], axis=1)


def default_witnesses(times, poses=None, reach=2):
    """Host: the witness lists of a view set, (V, N) int32.  times (V,): the frame each view shows; poses (V,): its pose's number, or
    None: every view is a pose of its own, so that views of one frame always witness each other.  View v's list holds the other poses
    of its own frame first, then every view (of any pose, its own included) whose frame is 1 .. reach frames away — each group in
    ascending view number — and is padded with -1 to the longest list (at least one column)."""
    times = np.asarray(times)
    poses = np.arange(times.size).reshape(times.shape) if poses is None else np.asarray(poses)
    if times.ndim != 1 or times.shape != poses.shape or times.dtype.kind not in "iu" or poses.dtype.kind not in "iu" or int(reach) < 0:
        raise hip.MudgError(f"default_witnesses: times {times.shape} {times.dtype} and poses {poses.shape} {poses.dtype} (two integer vectors of one "
                            f"length), reach {reach}")
    times = times.astype(np.int64)
    lists = []
    for v in range(len(times)):
        gap = np.abs(times - times[v])
        same = [w for w in range(len(times)) if w != v and gap[w] == 0 and poses[w] != poses[v]]
        near = [w for w in range(len(times)) if 0 < gap[w] <= int(reach)]
        lists.append(same + near)
    n = max([len(l) for l in lists] + [1])
    if n > ops.VIEW_MAX_WITNESSES:
        raise hip.MudgError(f"default_witnesses: {n} witnesses for a view, at most {ops.VIEW_MAX_WITNESSES}")
    out = np.full((len(lists), n), -1, dtype=np.int32)
    for v, l in enumerate(lists):
        out[v, :len(l)] = l
    return out


def consistent_views(depth, intr, c2w, hw_native, labels=None, *, times=None, witnesses=None, reach=None, min_depth=0.0, max_depth=MAX_DEPTH,
                     sky_label=SKY_LABEL, dynamic_mask=ops.VIEW_DYNAMIC_MASK, r=1, min_agree=2, max_violate=0, rel_tol=0.02, abs_tol=0.2):
    """Which pixels of a set of views the other views confirm (a rule of this project's own).  depth: (V, H, W) fp32
    metres, a window's frames x poses flattened; intr: (3, 3) or (V, 3, 3) at hw_native; c2w: (V, 4, 4); labels: (V, H, W) int64 or None
    (nothing is sky, nothing is dynamic); times: (V,) host integers, the frame each view shows (default 0 .. V-1: every view its own
    frame); witnesses: (V, N <= 64) host integers, -1 for empty (default: default_witnesses(times, None, reach) — every other view whose
    frame is at most reach frames away, those of the view's own frame first; reach defaults to 2 and is refused beside witnesses).  A usable pixel (lift_views' validity) is lifted to its world point and projected into each witness; a witness agrees
    if a usable pixel within r of the projection has a depth within abs_tol + rel_tol z of the point's, violates if every such pixel
    lies farther — it saw through the point — and otherwise says nothing; a pixel tagged dynamic (dynamic_mask: a bit per class) is
    tested against, and counted by, views of its own time only.  keep = usable, agree >= min_agree and violate <= max_violate.
    Returns {"agree", "violate", "keep", "flags": (V, H, W) uint8, "stats": (V, 6) int64 — usable, tested, kept, sum agree, sum violate,
    pixels with a violation}; metrics.view_consistency turns the stats into scores."""
    depth = _on_gpu("consistent_views", "the depth", depth, torch.float32)
    if depth.dim() != 3:
        raise hip.MudgError(f"consistent_views: expected (V, H, W) depths, got {tuple(depth.shape)}")
    if labels is not None:
        labels = _on_gpu("consistent_views", "the label image", labels, torch.int64, depth.shape)
    V = depth.shape[0]
    source = camera_table(intr, c2w, hw_native, depth.shape[1:])
    if source.shape[0] != V:
        raise hip.MudgError(f"consistent_views: {source.shape[0]} cameras for {V} views")
    times = np.arange(V, dtype=np.int32) if times is None else np.asarray(times)
    if witnesses is not None and reach is not None:
        raise hip.MudgError("consistent_views: reach makes the default witness lists; with witnesses given it would be ignored — give one of the two")
    if witnesses is None:
        witnesses = default_witnesses(times, None, 2 if reach is None else reach)
    flags = ops.view_flags(depth, labels, sky_label=sky_label, dynamic_mask=dynamic_mask, min_depth=min_depth, max_depth=max_depth)
    tables = torch.from_numpy(np.stack([source, witness_table(c2w, source)])).to(depth.device)
    agree, violate, keep, stats = ops.view_consistency(depth, flags, tables[0], tables[1], times, witnesses, r=r, min_agree=min_agree,
                                                       max_violate=max_violate, rel_tol=rel_tol, abs_tol=abs_tol)
    return {"agree": agree, "violate": violate, "keep": keep, "stats": stats, "flags": flags}


def fuse_views(depth, rgb, intr, c2w, hw_native, labels=None, *, voxel_size=-1, neighbour_radius=None, min_neighbours=0, **rule):
    """consistent_views, then lift_views of the pixels it keeps, then (neighbour_radius given) cloud.remove_outliers — a point stays iff
    min_neighbours others lie within neighbour_radius metres: the flying pixels every view shares are isolated in space
    —, then (voxel_size > 0) cloud.voxel_downsample: generated views as one filtered cloud.  **rule: consistent_views' keywords (times,
    witnesses or reach — not both —, the bounds and the tolerances).  Returns (render.PointCloud, consistent_views' result)."""
    from . import cloud
    result = consistent_views(depth, intr, c2w, hw_native, labels, **rule)
    bounds = {k: rule[k] for k in ("min_depth", "max_depth", "sky_label") if k in rule}
    points = lift_views(depth, rgb, intr, c2w, hw_native, labels, keep=result["keep"], **bounds)
    if neighbour_radius is not None and len(points):
        points = cloud.remove_outliers(points, neighbour_radius, min_neighbours)
    if voxel_size > 0 and len(points):
        points = cloud.voxel_downsample(points, voxel_size)
    return points, result
