"""The scene's point clouds, built on the GPU from LiDAR sweeps: the last link of "scene -> conditions -> clips".

The reference makes the background cloud and the per-object clouds with a per-frame numpy loop (data_process/tools/process_lidar.py)
that needs open3d.  Here a batch of sweeps is one launch of csrc/cloud.hip: every return is taken to the world, coloured by the
cameras, labelled by the tracked boxes and written as a packed 16-byte point; voxel thinning is a sort by voxel key (torch) around three
more kernels.  DESIGN.md §13 states both rules and every deviation.  The host's share is float64 matrix algebra per (frame, camera)
and (frame, object), and reading files stays with the caller (load_lidar, load_image).  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip, ops, render

CAMERAS = ("camera_FRONT", "camera_FRONT_LEFT", "camera_FRONT_RIGHT", "camera_SIDE_LEFT", "camera_SIDE_RIGHT")   # process_lidar.py:53-54
CLASSES = ("Vehicle", "Pedestrian")                                                                                # process_lidar.py:155
MIN_OBJECT_POINTS = 100                                                                                            # process_lidar.py:191
MAX_CAMERAS = 8
KEY_LIMIT = 1 << 20
FRAMES_PER_LAUNCH = 16


def inverse_rigid(m):
    """(4, 4) or (3, 4) float64 -> the (3, 4) inverse the way the reference takes it: inv(R) and -inv(R) t (process_lidar.py:59-62)."""
    m = np.asarray(m, dtype=np.float64)
    r = np.linalg.inv(m[:3, :3])
    return np.concatenate([r, (-r @ m[:3, 3])[:, None]], axis=1)


def object_tables(obj, n_frames):
    """save_object_from_pt:159-171: the per-frame transform (n, 4, 4), scale (n, 3) and visibility (n,) of an object's segments."""
    transform, scale, visibility = np.zeros((n_frames, 4, 4)), np.zeros((n_frames, 3)), np.zeros(n_frames)
    for seg in obj["segments"]:
        s, n = seg["start_frame"], seg["n_frames"]
        transform[s:s + n] = seg["data"]["transform"]
        scale[s:s + n] = seg["data"]["scale"]
        visibility[s:s + n] = 1
    return transform, scale, visibility


def is_object_motion(transforms, visibilities):
    """process_lidar.py:265-280 with its own arithmetic: the norm of the difference of the whole 4 x 4 matrices of the first and the
    last visible frame (index -1, the last frame, when none is)."""
    first = last = -1
    for i in range(len(visibilities)):
        if first == -1 and visibilities[i] == 1:
            first = i
        if visibilities[i] == 1:
            last = i
    return bool(np.linalg.norm(transforms[last] - transforms[first]) > 0.5)


def moving_objects(scenario, frames):
    """The objects the reference keeps before it looks at a point: Vehicle or Pedestrian, and moving over `frames`."""
    n_frames = scenario["observers"]["lidar_TOP"]["n_frames"]
    out = []
    for obj in scenario["objects"].values():
        if obj["class_name"] not in CLASSES:
            continue
        transform, scale, visibility = (t[frames] for t in object_tables(obj, n_frames))
        if is_object_motion(transform, visibility):
            out.append({"id": obj["id"], "class_name": obj["class_name"], "visibility": visibility, "bbox": scale, "transform_obj": transform})
    return out


def camera_table(scenario, frames, cameras, images):
    """(frames, ncam, 24) float64 and the flat image buffer: per entry w2c[12], K[9], then h, w and the image's byte offset as int64.
    images[t][c] is the uint8 (h, w, 3) image of camera c in frame frames[t]; the cameras come in the scenario's own order."""
    obs = scenario["observers"]
    names = [s for s in obs.keys() if s in cameras]
    if len(names) > MAX_CAMERAS:
        raise hip.MudgError(f"build_scene_clouds: {len(names)} cameras (at most {MAX_CAMERAS})")
    table = np.zeros((len(frames), max(len(names), 1), 24))
    words = table.view(np.int64)
    flat, at = [], 0
    for t, frame in enumerate(frames):
        for c, s in enumerate(names):
            image = np.ascontiguousarray(images[t][c])
            h, w = (int(v) for v in obs[s]["data"]["hw"][frame])
            if image.dtype != np.uint8 or image.shape != (h, w, 3):
                raise hip.MudgError(f"build_scene_clouds: the image of {s} in frame {frame} is {image.dtype} {image.shape}, the scenario says uint8 ({h}, {w}, 3)")
            table[t, c, :12] = inverse_rigid(obs[s]["data"]["c2w"][frame]).reshape(12)
            table[t, c, 12:21] = np.asarray(obs[s]["data"]["intr"][frame], dtype=np.float64).reshape(9)
            words[t, c, 21:] = (h, w, at)
            flat.append(image.reshape(-1))
            at += image.size
    return (table if names else None), (np.concatenate(flat) if flat else None)


def object_table(objects, rows):
    """(len(rows), nobj, 16) float64: w2l[12], the box extents, visible — row t is the objects' frame rows[t]."""
    if not objects:
        return None
    table = np.zeros((len(rows), len(objects), 16))
    for k, o in enumerate(objects):
        for t, row in enumerate(rows):
            if o["visibility"][row] == 1:
                table[t, k, :12] = inverse_rigid(o["transform_obj"][row]).reshape(12)
                table[t, k, 12:15] = o["bbox"][row]
                table[t, k, 15] = 1.0
    return table


class _Batch:
    """The sweeps of a few frames on the GPU, ready for mudg_cloud_sweep (kept for the background pass)."""

    def __init__(self, scenario, frames, rows, cameras, load_lidar, load_image, device):
        obs = scenario["observers"]
        names = [s for s in obs.keys() if s in cameras]
        sweeps = []
        for frame in frames:
            o, d, r = load_lidar(frame)
            o, d, r = (np.ascontiguousarray(a, dtype=np.float32) for a in (o, d, r))
            o, d, r = o.reshape(-1, 3), d.reshape(-1, 3), r.reshape(-1)
            if not (len(o) == len(d) == len(r)) or len(r) == 0:
                raise hip.MudgError(f"build_scene_clouds: frame {frame} has rays {o.shape}, {d.shape} and ranges {r.shape}")
            sweeps.append((o, d, r))
        counts = [len(s[2]) for s in sweeps]
        table, flat = camera_table(scenario, frames, cameras, [[load_image(s, frame) for s in names] for frame in frames])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.rows = rows
        self.rays_o, self.rays_d, self.ranges = (up(np.concatenate([s[i] for s in sweeps])) for i in range(3))
        self.offsets = up(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
        self.max_rays = max(counts)
        self.l2w = up(np.stack([np.asarray(obs["lidar_TOP"]["data"]["l2w"][f], dtype=np.float64)[:3].reshape(12) for f in frames]))
        self.cams = up(table) if table is not None else None
        self.images = up(flat) if flat is not None else None

    def run(self, objects):
        table = object_table(objects, self.rows)
        objs = torch.from_numpy(table).to(self.rays_o.device) if table is not None else None
        return ops.cloud_sweep(self.rays_o, self.rays_d, self.ranges, self.offsets, self.max_rays, self.l2w, self.cams, objs, self.images)


def voxel_downsample(cloud: render.PointCloud, voxel_size) -> render.PointCloud:
    """One point per occupied voxel of an absolute grid: the mean position and the round-half-up mean colour, in ascending key order
    (a rule of this project — parity with open3d's voxel_down_sample is not claimed)."""
    if not isinstance(cloud, render.PointCloud):
        raise hip.MudgError("voxel_downsample: expected a render.PointCloud (on the GPU; there is no CPU path)")
    v = float(voxel_size)
    if not (v > 0.0 and np.isfinite(v)):
        raise hip.MudgError(f"voxel_downsample: voxel size {voxel_size}")
    pts = cloud.points
    xyz = pts[:, :3].view(torch.float32)
    lo, hi = (float(t) for t in torch.aminmax(xyz))                       # the bounds, to the host: nothing is launched on a bad cloud
    if not (np.isfinite(lo) and np.isfinite(hi)) or np.floor(lo / v) <= -KEY_LIMIT or np.floor(hi / v) >= KEY_LIMIT:
        raise hip.MudgError(f"voxel_downsample: coordinates in [{lo}, {hi}] leave the key's range at voxel size {v} (|index| < 2^20)")
    keys = ops.cloud_voxel_keys(pts, v)
    keys, order = torch.sort(keys, stable=True)
    flags = torch.zeros_like(keys)
    flags[1:] = keys[1:] != keys[:-1]
    segments = torch.cumsum(flags, dim=0)
    voxels = int(segments[-1]) + 1
    return render.PointCloud(ops.cloud_voxel_finish(ops.cloud_voxel_reduce(pts, order, segments, v, voxels), v))


# ------------------------------------------------------------------------------------------------ neighbour search
class NeighbourGrid:
    """A reference cloud ready to be searched within `radius`: `points` (n, 4) int32 in ascending cell-key order, `keys` (n,) int64,
    `order` (n,) int64 — the original index of each sorted point —, and the doubles `radius`, `cell` = radius (1 + 2^-10), `r2`."""

    def __init__(self, points, keys, order, radius, cell, r2):
        self.points, self.keys, self.order, self.radius, self.cell, self.r2 = points, keys, order, radius, cell, r2

    def __len__(self):
        return self.points.shape[0]

    @classmethod
    def build(cls, cloud: render.PointCloud, radius):
        """Keys (mudg_cloud_voxel_keys at the cell edge), a stable sort, a gather.  A radius outside (0, 64], an empty cloud, or
        coordinates beyond 2^20 - 2 cells — so that a neighbour cell always fits the key — raise before anything is launched."""
        if not isinstance(cloud, render.PointCloud):
            raise hip.MudgError("NeighbourGrid.build: expected a render.PointCloud (on the GPU; there is no CPU path)")
        try:
            r = float(radius)
        except (TypeError, ValueError):
            raise hip.MudgError(f"NeighbourGrid.build: radius {radius!r}") from None
        if not (0.0 < r <= ops.NEIGHBOUR_MAX_RADIUS):
            raise hip.MudgError(f"NeighbourGrid.build: radius {radius} (0 < radius <= {ops.NEIGHBOUR_MAX_RADIUS:g})")
        if len(cloud) == 0:
            raise hip.MudgError("NeighbourGrid.build: an empty cloud")
        cell = r * ops.NEIGHBOUR_MARGIN
        pts = cloud.points
        lo, hi = (float(t) for t in torch.aminmax(pts[:, :3].view(torch.float32)))    # the bounds, to the host: nothing is launched on a bad cloud
        if not (np.isfinite(lo) and np.isfinite(hi)) or np.floor(lo / cell) < -(KEY_LIMIT - 2) or np.floor(hi / cell) > KEY_LIMIT - 2:
            raise hip.MudgError(f"NeighbourGrid.build: coordinates in [{lo}, {hi}] leave the grid at radius {r} (|cell index| <= 2^20 - 2)")
        keys, order = torch.sort(ops.cloud_voxel_keys(pts, cell), stable=True)
        return cls(pts[order].contiguous(), keys, order, r, cell, r * r)


def _queries(name, grid, queries):
    if not isinstance(grid, NeighbourGrid):
        raise hip.MudgError(f"{name}: expected a NeighbourGrid (NeighbourGrid.build makes one)")
    points = queries.points if isinstance(queries, render.PointCloud) else queries
    if not torch.is_tensor(points) or not points.is_cuda or points.dtype != torch.int32 or points.dim() != 2 or points.shape[1] != 4:
        raise hip.MudgError(f"{name}: expected the queries as a render.PointCloud or packed (nq, 4) int32 points on the GPU (there is no CPU path)")
    return points.contiguous()


def _visit(grid, points):
    """The queries in the order of their own cells: a wave's lanes then walk the same or adjacent intervals.  Any permutation gives the
    same results — a query outside the key's range, or one that is not finite, merely gets an arbitrary place in it."""
    return torch.sort(ops.cloud_voxel_keys(points, grid.cell))[1]


def nearest(grid, queries):
    """For every query (a render.PointCloud or packed points) the nearest point of the grid's cloud within its radius: (d2 (nq,) float64,
    index (nq,) int64) in the caller's order — the squared distance in fp64 and the point's index in the cloud the grid was built
    from, the lowest on a tie; +inf and -1 where nothing is within the radius."""
    points = _queries("nearest", grid, queries)
    if points.shape[0] == 0:
        return torch.empty((0,), dtype=torch.float64, device=points.device), torch.empty((0,), dtype=torch.int64, device=points.device)
    return ops.cloud_nearest(grid.points, grid.keys, grid.order, points, grid.cell, grid.r2, visit=_visit(grid, points))


def neighbour_counts(grid, queries, cap):
    """min(points of the grid's cloud within its radius, cap) for every query, (nq,) int32."""
    if not (isinstance(cap, (int, np.integer)) and 1 <= cap < 2 ** 31):
        raise hip.MudgError(f"neighbour_counts: cap {cap!r} (an integer, at least 1)")
    points = _queries("neighbour_counts", grid, queries)
    if points.shape[0] == 0:
        return torch.empty((0,), dtype=torch.int32, device=points.device)
    return ops.cloud_count(grid.points, grid.keys, grid.order, points, grid.cell, grid.r2, int(cap), visit=_visit(grid, points))


def radius_outliers(cloud: render.PointCloud, radius, min_neighbours):
    """The keep mask (n,) bool of a radius outlier filter: a point stays iff at least min_neighbours other points of the cloud lie
    within radius of it (a duplicate at its own position is another point).  A rule of this project — parity with open3d's
    remove_radius_outlier is not claimed."""
    if not (isinstance(min_neighbours, (int, np.integer)) and 0 <= min_neighbours < 2 ** 31 - 1):
        raise hip.MudgError(f"radius_outliers: min_neighbours {min_neighbours!r} (an integer, at least 0)")
    grid = NeighbourGrid.build(cloud, radius)
    need = int(min_neighbours) + 1                                          # a point counts itself
    return neighbour_counts(grid, cloud, need) >= need


def remove_outliers(cloud: render.PointCloud, radius, min_neighbours) -> render.PointCloud:
    """The points radius_outliers keeps, in their order."""
    return render.PointCloud(cloud.points[radius_outliers(cloud, radius, min_neighbours)])


def _arrays(points):
    """Packed points on the GPU -> host (n, 3) float32 and (n, 3) uint8."""
    p = points.cpu()
    word = p[:, 3]
    return p[:, :3].contiguous().view(torch.float32).numpy(), torch.stack([word & 255, (word >> 8) & 255, (word >> 16) & 255], dim=1).to(torch.uint8).numpy()


def build_scene_clouds(scenario, load_lidar, load_image, *, frames=None, cameras=CAMERAS, voxel_size=-1, object_voxel_size=-1,
                       frames_per_launch=FRAMES_PER_LAUNCH, device="cuda"):
    """save_object_from_pt and save_background_from_pt (process_lidar.py:141-262) on arrays.  scenario: the reference's scenario.pt
    dict; load_lidar(frame) -> (rays_o, rays_d, ranges); load_image(camera, frame) -> uint8 (h, w, 3); frames: the scenario's frame
    numbers to use (default all).  Returns (background PointCloud, ObjectSet or None, obj_info): obj_info is the reference's list of
    dicts (objects_info.pkl; 'ply_path' is None, nothing is written), ObjectSet.from_obj_info(obj_info) is the set returned.

    Objects first, with the moving Vehicle / Pedestrian objects; one with fewer than 100 points is dropped, and the background is
    what no surviving object's box holds.  A point in two boxes belongs to the lower-numbered object (a stated deviation)."""
    return _build_scene(scenario, load_lidar, load_image, frames=frames, cameras=cameras, voxel_size=voxel_size, object_voxel_size=object_voxel_size,
                       frames_per_launch=frames_per_launch, device=device)[:3]


def _batches(scenario, frames, cameras, frames_per_launch, load_lidar, load_image, device):
    step = len(frames) if not frames_per_launch or frames_per_launch < 0 else int(frames_per_launch)
    for s in range(0, len(frames), step):
        yield _Batch(scenario, frames[s:s + step], list(range(s, min(s + step, len(frames)))), cameras, load_lidar, load_image, device)


def _split_frames(points, labels, batches):
    """The label-0 points of a pass in (frame, ray) order as render.FrameSweeps: a prefix count of the labels read at the frames' ends."""
    ends = torch.cat([b.offsets[1:] + base for b, base in zip(batches, np.cumsum([0] + [int(b.ranges.numel()) for b in batches[:-1]]).tolist())])
    count = torch.cumsum(labels == 0, dim=0)                              # ends >= 1: _Batch refuses a frame without rays, so ends - 1 never wraps
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), count[ends - 1].cpu()])
    return render.FrameSweeps(points[labels == 0], offsets)


def frame_sweeps(scenario, load_lidar, load_image, obj_info, *, frames=None, cameras=CAMERAS, frames_per_launch=FRAMES_PER_LAUNCH, device="cuda"):
    """The reference's load_lidar_data (data_process/pipeline_depth.py:16-60) on arrays: per frame, the returns a camera sees that lie
    in no box of obj_info's objects (build_scene_clouds' third result, whose tables are indexed by position in `frames`), in ray order.
    Concatenated they are build_scene_clouds' background at voxel_size = -1.  Returns a render.FrameSweeps."""
    device, frames = _checked(scenario, frames, device, "frame_sweeps")
    batches = list(_batches(scenario, frames, cameras, frames_per_launch, load_lidar, load_image, device))
    out = [b.run(obj_info) for b in batches]
    return _split_frames(torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out]), batches)


def _checked(scenario, frames, device, name):
    device = torch.device(device)
    if device.type != "cuda":
        raise hip.MudgError(f"{name}: the clouds are built on the GPU (there is no CPU path)")
    n_frames = scenario["observers"]["lidar_TOP"]["n_frames"]
    frames = list(range(n_frames)) if frames is None else [int(f) for f in frames]
    if not frames or min(frames) < 0 or max(frames) >= n_frames:
        raise hip.MudgError(f"{name}: frames {frames} of a scenario with {n_frames}")
    return device, frames


def _build_scene(scenario, load_lidar, load_image, *, frames=None, cameras=CAMERAS, voxel_size=-1, object_voxel_size=-1,
                frames_per_launch=FRAMES_PER_LAUNCH, device="cuda", keep_sweeps=False):
    """build_scene_clouds with a fourth result: with keep_sweeps the background pass frame by frame (a render.FrameSweeps, what
    frame_sweeps returns for the third result), taken from the pass that made the background — the rays are not walked again."""
    device, frames = _checked(scenario, frames, device, "build_scene_clouds")
    candidates = moving_objects(scenario, frames)
    batches, points, labels = [], [], []
    for batch in _batches(scenario, frames, cameras, frames_per_launch, load_lidar, load_image, device):
        batches.append(batch)
        p, l = batch.run(candidates)
        points.append(p)
        labels.append(l)
    points, labels = torch.cat(points), torch.cat(labels)

    obj_info = []
    for k, o in enumerate(candidates):
        mine = points[labels == k + 1]                                  # stable: (frame, ray) order, the reference's concatenation
        if object_voxel_size > 0 and len(mine):
            mine = voxel_downsample(render.PointCloud(mine), object_voxel_size).points
        if len(mine) < MIN_OBJECT_POINTS:
            continue
        xyz, rgb = _arrays(mine)
        obj_info.append(dict(o, point_cloud={"points": xyz.astype(np.float64), "colors": rgb / 255.0, "normals": np.zeros((len(xyz), 3))}, ply_path=None))
    if len(obj_info) != len(candidates):                                # the background pass sees only the objects that survived
        out = [b.run(obj_info) for b in batches]
        points, labels = torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])
    sweeps = _split_frames(points, labels, batches) if keep_sweeps else None
    ground = sweeps.points if sweeps is not None else points[labels == 0]
    if len(ground) == 0:
        raise hip.MudgError("build_scene_clouds: no LiDAR return is seen by a camera outside the objects' boxes")
    background = render.PointCloud(ground)
    if voxel_size > 0:
        background = voxel_downsample(background, voxel_size)
    objects = render.ObjectSet.from_obj_info(obj_info, device) if obj_info else None
    return background, objects, obj_info, sweeps
