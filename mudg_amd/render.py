"""The sparse conditions, rendered on the GPU: a fused point cloud drawn into the camera at virtual poses.

The reference makes the sparse colour and sparse depth images with pyrender point sprites in an offscreen GL context
(data_process/tools/generate_sparse.py:116-223), for two hard-coded poses, through JPEG and .npy files.  Here the cloud lives on the
GPU as packed 16-byte points and three kernels (csrc/splat.hip) turn (cloud, per-frame camera, poses) into the (3, T, H, W) condition
tensors the driver consumes.  DESIGN.md §12 states the raster rule; it is a definition of this project (pixel parity with pyrender is
not claimed: pyrender cannot run where this is built).  The host's share is float64 matrix algebra per (frame, pose), uploaded once
per call.  There is no CPU fallback: a cloud that is not on the GPU is an error.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import hip, ops

BACKGROUND_POINT_SIZE = 2.5      # generate_sparse.py:168
OBJECT_POINT_SIZE = 4.0          # generate_sparse.py:192
ZNEAR, ZFAR = 1e-4, 200.0        # generate_sparse.py:153
CLASS_LABELS = (0, 500, 1)       # colour, depth, semantic: virtual_render/data_tools.py:61, 153, 212


def _pack(xyz, rgb, device):
    """(n, 3) coordinates and (n, 3) colours (uint8, or float in [0, 1] converted once by round(c * 255)) -> (n, 4) int32."""
    xyz = torch.as_tensor(np.asarray(xyz) if not torch.is_tensor(xyz) else xyz)
    rgb = torch.as_tensor(np.asarray(rgb) if not torch.is_tensor(rgb) else rgb)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or tuple(rgb.shape) != tuple(xyz.shape) or xyz.shape[0] == 0:
        raise hip.MudgError(f"a point cloud is (n > 0, 3) coordinates and (n, 3) colours, got {tuple(xyz.shape)} and {tuple(rgb.shape)}")
    if rgb.dtype.is_floating_point:
        rgb = torch.round(rgb.to(torch.float64) * 255.0).clamp_(0, 255)
    rgb = rgb.to(torch.int32)
    bits = xyz.to(torch.float32).contiguous().view(torch.int32)
    word = rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)
    return torch.cat([bits, word[:, None]], dim=1).contiguous().to(device)


class PointCloud:
    """A device-resident cloud: `points` (n, 4) int32 — x, y, z as fp32 bits, the colour r | g << 8 | b << 16 in the fourth word."""

    def __init__(self, points: torch.Tensor):
        if not torch.is_tensor(points) or not points.is_cuda or points.dtype != torch.int32 or points.dim() != 2 or points.shape[1] != 4:
            raise hip.MudgError("PointCloud: expected packed (n, 4) int32 points on the GPU (PointCloud.from_arrays packs and uploads)")
        self.points = points.contiguous()

    @classmethod
    def from_arrays(cls, xyz, rgb, device="cuda"):
        return cls(_pack(xyz, rgb, torch.device(device)))

    @classmethod
    def concatenated(cls, *clouds):
        """The clouds' packed buffers one after the other, nothing else (data_process/tools/merge_points.py:77-90 on packed points)."""
        if not clouds or not all(isinstance(c, PointCloud) for c in clouds):
            raise hip.MudgError("PointCloud.concatenated: expected one or more PointClouds")
        if len({c.points.device for c in clouds}) != 1:
            raise hip.MudgError("PointCloud.concatenated: the clouds are on different devices")
        return cls(torch.cat([c.points for c in clouds], dim=0))

    def __len__(self):
        return self.points.shape[0]


class FrameSweeps:
    """The background returns of a scene frame by frame (cloud.frame_sweeps): `points` packed like PointCloud.points, frame f owning
    points[offsets[f]:offsets[f + 1]] in ray order; `offsets` (frames + 1,) int64 on the host.  What the reference's load_lidar_data
    (data_process/pipeline_depth.py:16-60) returns as lists."""

    def __init__(self, points: torch.Tensor, offsets):
        if not torch.is_tensor(points) or not points.is_cuda or points.dtype != torch.int32 or points.dim() != 2 or points.shape[1] != 4:
            raise hip.MudgError("FrameSweeps: expected packed (n, 4) int32 points on the GPU (there is no CPU path)")
        offsets = torch.as_tensor(offsets, dtype=torch.int64).cpu()
        if offsets.dim() != 1 or offsets.numel() < 2 or int(offsets[0]) != 0 or int(offsets[-1]) != points.shape[0] or bool((offsets[1:] < offsets[:-1]).any()):
            raise hip.MudgError(f"FrameSweeps: offsets {offsets.tolist()} do not cut {points.shape[0]} points into frames")
        self.points = points.contiguous()
        self.offsets = offsets

    @property
    def frames(self):
        return self.offsets.numel() - 1

    def frame(self, f):
        return self.points[int(self.offsets[f]):int(self.offsets[f + 1])]


class ObjectSet:
    """The moving objects of a scene (the reference's objects_info.pkl): per object a cloud, `transform_obj` (frames, 4, 4) taking it
    to the world and `visibility` (frames,).  All clouds sit in one concatenated device buffer with a per-point object id; a frame
    draws it with one matrix per (pose, object), w2c @ transform_obj[frame] — an object that is not visible gets the zero matrix, whose
    zc = 0 fails the near test.  This replaces the reference's merge_all_obj (a transformed host copy per frame)."""

    def __init__(self, clouds: Sequence, transform_obj, visibility, device="cuda"):
        self.xyz = [np.asarray(c[0], dtype=np.float64) for c in clouds]
        self.rgb = [np.asarray(c[1]) for c in clouds]
        self.transform_obj = np.asarray(transform_obj, dtype=np.float64)          # (objects, frames, 4, 4)
        self.visibility = np.asarray(visibility)                                  # (objects, frames)
        n = len(self.xyz)
        if n == 0 or self.transform_obj.shape[:1] != (n,) or self.transform_obj.shape[2:] != (4, 4) or self.visibility.shape != self.transform_obj.shape[:2]:
            raise hip.MudgError(f"ObjectSet: {n} clouds with transforms {self.transform_obj.shape} and visibility {self.visibility.shape}")
        dev = torch.device(device)
        self.cloud = PointCloud(torch.cat([_pack(x, c, dev) for x, c in zip(self.xyz, self.rgb)]))
        self.ids = torch.cat([torch.full((len(x),), i, dtype=torch.int32) for i, x in enumerate(self.xyz)]).to(dev)

    @classmethod
    def from_obj_info(cls, obj_info, device="cuda"):
        """From the reference's list of dicts ('point_cloud': {'points', 'colors'}, 'transform_obj', 'visibility')."""
        return cls([(o["point_cloud"]["points"], o["point_cloud"]["colors"]) for o in obj_info],
                   np.stack([np.asarray(o["transform_obj"]) for o in obj_info]), np.stack([np.asarray(o["visibility"]) for o in obj_info]), device)

    @property
    def frames(self):
        return self.transform_obj.shape[1]

    def visible(self, frame):
        return [i for i in range(len(self.xyz)) if self.visibility[i, frame] == 1]

    def merged(self, frame):
        """What the reference's merge_all_obj returns for the frame (host arrays, its arithmetic and its one-point sentinel): kept for
        inspection and tests; the renderer does not call it."""
        return merge_objects(self.xyz, self.rgb, self.transform_obj, self.visibility, frame)

    def matrices(self, w2c, frame):
        """(poses, 4, 4) float64 world-to-camera -> (poses, objects, 3, 4) float64: w2c @ transform_obj[frame], zero where not visible."""
        return object_matrices(w2c, self.transform_obj, self.visibility, frame)


def object_matrices(w2c, transform_obj, visibility, frame):
    """Host, float64: M[pose][object] = (w2c[pose] @ transform_obj[object][frame])[:3], zero for an object the frame does not show."""
    w2c = np.asarray(w2c, dtype=np.float64)
    transform_obj = np.asarray(transform_obj, dtype=np.float64)
    out = np.zeros((w2c.shape[0], transform_obj.shape[0], 3, 4))
    for i in range(transform_obj.shape[0]):
        if visibility[i][frame] == 1:
            out[:, i] = (w2c @ transform_obj[i, frame])[:, :3]
    return out


def merge_objects(xyz, rgb, transform_obj, visibility, frame):
    """generate_sparse.py:238-260 on arrays: the visible objects of a frame, transformed to the world and concatenated."""
    pts, cols = [], []
    for i in range(len(xyz)):
        if visibility[i][frame] == 1:
            tr = transform_obj[i][frame]
            pts.append(xyz[i] @ tr[:3, :3].T + tr[:3, 3])
            cols.append(rgb[i])
    if not pts:
        return np.array([[1000, 1000, 1000]]), np.array([[0, 0, 0]])
    return np.concatenate(pts, axis=0), np.concatenate(cols, axis=0)


def virtual_poses(c2w, shift=2.0, with_ori_pose=False):
    """generate_virtual_pose (generate_sparse.py:263-279): the camera moved `shift` metres to its left and to its right."""
    c2w = np.asarray(c2w, dtype=np.float64)
    ret = [c2w] if with_ori_pose else []
    for direction in (-1.0, 1.0):
        vcam2cam = np.eye(4)
        vcam2cam[0, 3] += round(direction * shift, 4)
        ret.append(c2w @ vcam2cam)
    return ret


def scaled_intrinsics(intr, hw_native, hw_out):
    """(3, 3) K at the camera's size -> (fx, fy, cx, cy) at the model's size, float64 (a stated deviation: the reference renders at
    the native size and resizes the image afterwards)."""
    (h0, w0), (h, w) = hw_native, hw_out
    k = np.asarray(intr, dtype=np.float64)
    return np.array([k[0, 0] * w / w0, k[1, 1] * h / h0, k[0, 2] * w / w0, k[1, 2] * h / h0])


def render_conditions(background: PointCloud, objects: Optional[ObjectSet], intr, c2w_frames, hw_native, hw_out, poses=None, *,
                      frame_ids=None, shift=2.0, return_images=False, znear=ZNEAR, zfar=ZFAR, early_reject=True, stats=None):
    """Render T frames at P poses.  intr: (3, 3) or (T, 3, 3); c2w_frames: (T, 4, 4) camera-to-world, OpenCV convention; poses: None
    (the original pose and virtual_poses(c2w, shift): P = 3) or explicit camera-to-world matrices (T, P, 4, 4); frame_ids: the scene's
    frame numbers of the T frames for the objects' transforms (default 0 .. T-1).

    Returns {"sparse_frames", "sparse_depth"}: (P, 3, T, H, W) fp32 in [-1, 1], entry p being what the reference's loaders make of
    pose p's files; with return_images also "rgb" (P, T, H, W, 3) uint8, "depth" (P, T, H, W) fp32 metres, "mask" and the two layers
    "bg_rgb", "bg_depth", "obj_rgb", "obj_depth"."""
    if not isinstance(background, PointCloud) or (objects is not None and not isinstance(objects, ObjectSet)):
        raise hip.MudgError("render_conditions: the background is a PointCloud and the objects an ObjectSet (on the GPU; there is no CPU path)")
    c2w_frames = np.asarray(c2w_frames, dtype=np.float64)
    T = c2w_frames.shape[0]
    if poses is None:
        poses = np.stack([np.stack(virtual_poses(c, shift, with_ori_pose=True)) for c in c2w_frames])
    poses = np.asarray(poses, dtype=np.float64)
    if c2w_frames.shape != (T, 4, 4) or poses.ndim != 4 or poses.shape[0] != T or poses.shape[2:] != (4, 4):
        raise hip.MudgError(f"render_conditions: cameras {c2w_frames.shape} with poses {poses.shape}")
    P = poses.shape[1]
    frame_ids = list(range(T)) if frame_ids is None else [int(f) for f in frame_ids]
    intr = np.asarray(intr, dtype=np.float64)
    intr = np.broadcast_to(intr, (T, 3, 3))
    H, W = (int(v) for v in hw_out)
    dev = background.points.device

    # host, float64, once per (frame, pose); one upload for the call
    w2c = np.linalg.inv(poses)                                                            # (T, P, 4, 4)
    bg_mats = torch.from_numpy(np.ascontiguousarray(w2c[:, :, None, :3, :].reshape(T, P, 1, 12)).astype(np.float32)).to(dev)
    obj_mats = None
    if objects is not None:
        obj_mats = np.stack([objects.matrices(w2c[t], frame_ids[t]) for t in range(T)]).reshape(T, P, -1, 12)
        obj_mats = torch.from_numpy(obj_mats.astype(np.float32)).to(dev)
    cams = [scaled_intrinsics(intr[t], hw_native, hw_out).astype(np.float32) for t in range(T)]

    sparse = torch.empty((P, 3, T, H, W), dtype=torch.float32, device=dev)
    sdepth = torch.empty_like(sparse)
    bg_keys = ops.splat_keys(P, H, W, dev)
    obj_keys = ops.splat_keys(P, H, W, dev) if objects is not None else None
    kw = dict(znear=znear, zfar=zfar, early_reject=early_reject, stats=stats)
    kept = {k: [] for k in ("rgb", "depth", "mask", "bg_rgb", "bg_depth", "obj_rgb", "obj_depth")} if return_images else None
    for t in range(T):
        ops.splat_points(background.points, bg_mats[t], bg_keys, cams[t], BACKGROUND_POINT_SIZE, **kw)
        bg = ops.splat_resolve(bg_keys, background.points)
        obj = None
        if objects is not None and objects.visible(frame_ids[t]):
            ops.splat_points(objects.cloud.points, obj_mats[t], obj_keys, cams[t], OBJECT_POINT_SIZE, ids=objects.ids, **kw)
            obj = ops.splat_resolve(obj_keys, objects.cloud.points)
        images = ops.splat_compose(bg, obj, sparse, sdepth, t, images=return_images)
        if return_images:
            empty = (torch.zeros_like(bg[0]), torch.zeros_like(bg[1]))
            for name, value in zip(("rgb", "depth", "mask"), images):
                kept[name].append(value)
            for name, (d, c) in (("bg", bg), ("obj", obj or empty)):
                kept[name + "_rgb"].append(c.view(torch.uint8).reshape(P, H, W, 4)[..., :3].contiguous())
                kept[name + "_depth"].append(d)
    out = {"sparse_frames": sparse, "sparse_depth": sdepth}
    if return_images:
        out.update({k: torch.stack(v, dim=1) for k, v in kept.items()})
    return out


@dataclass
class Scene:
    """What render_windows needs of a scene: the clouds and, per frame, the camera (the reference's scenario.pt observer data)."""
    background: PointCloud
    objects: Optional[ObjectSet]
    intr: np.ndarray            # (3, 3) or (frames, 3, 3)
    c2w: np.ndarray             # (frames, 4, 4)
    hw_native: tuple            # (H0, W0) the intrinsics refer to
    sweeps: Optional[FrameSweeps] = None      # the background frame by frame (depth.lidar_depth_maps), kept on request

    @classmethod
    def from_scenario(cls, scenario, load_lidar, load_image, camera="camera_FRONT", *, frames=None, keep_sweeps=False, **kwargs):
        """Build the clouds from the scenario's LiDAR sweeps (cloud.build_scene_clouds, which takes **kwargs) and take `camera`'s
        intrinsics, poses and size for the frames used.  keep_sweeps: also keep the background pass frame by frame, before any voxel
        thinning, for the LiDAR depth maps."""
        from . import cloud
        background, objects, _, sweeps = cloud._build_scene(scenario, load_lidar, load_image, frames=frames, keep_sweeps=keep_sweeps, **kwargs)
        data = scenario["observers"][camera]["data"]
        rows = list(range(scenario["observers"]["lidar_TOP"]["n_frames"])) if frames is None else [int(f) for f in frames]
        return cls(background, objects, np.asarray(data["intr"], dtype=np.float64)[rows], np.asarray(data["c2w"], dtype=np.float64)[rows],
                   tuple(int(v) for v in data["hw"][rows[0]]), sweeps)
