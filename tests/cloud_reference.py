"""The CPU definition of the scene-cloud rules, in numpy: elementwise float64 operations in the stated order (no `@`:
the order of a BLAS product is not the rule) and integer sums.  Written independently of csrc/cloud.hip and mudg_amd/cloud.py; the
GPU tests demand bit-equality with it, the CPU tests check it against what the reference's process_lidar.py computed."""
import numpy as np

F = np.float64
CAMERAS = ("camera_FRONT", "camera_FRONT_LEFT", "camera_FRONT_RIGHT", "camera_SIDE_LEFT", "camera_SIDE_RIGHT")
CLASSES = ("Vehicle", "Pedestrian")
MIN_POINTS = 100


def _row3(m, x, y, z):
    return (m[0] * x + m[1] * y) + m[2] * z


def _row4(m, x, y, z):
    return _row3(m, x, y, z) + m[3]


def world_points(rays_o, rays_d, ranges, l2w):
    """p = (R o + t) + (R d) range, every row as ((r0 x + r1 y) + r2 z) (+ t): (n, 3) float64."""
    o, d, r = np.asarray(rays_o, F).reshape(-1, 3), np.asarray(rays_d, F).reshape(-1, 3), np.asarray(ranges, F).reshape(-1)
    m = np.asarray(l2w, F)
    return np.stack([_row4(m[a], o[:, 0], o[:, 1], o[:, 2]) + _row3(m[a], d[:, 0], d[:, 1], d[:, 2]) * r for a in range(3)], axis=1)


def project(p, w2c, K, h, w):
    """One camera: (mask, ix, iy); the pixel indices are meaningful where the mask is set."""
    w2c, K = np.asarray(w2c, F), np.asarray(K, F)
    with np.errstate(all="ignore"):
        xc, yc, zc = (_row4(w2c[a], p[:, 0], p[:, 1], p[:, 2]) for a in range(3))
        xn, yn = xc / zc, yc / zc
        x = (K[0, 0] * xn + K[0, 1] * yn) + K[0, 2]
        y = (K[1, 0] * xn + K[1, 1] * yn) + K[1, 2]
        fits = (x > -2147483649.0) & (x < 2147483648.0) & (y > -2147483649.0) & (y < 2147483648.0)
        ix = np.where(fits, x, 0.0).astype(np.int32)               # truncation toward zero
        iy = np.where(fits, y, 0.0).astype(np.int32)
    mask = (zc > 0) & fits & (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
    return mask, ix, iy


def colours(p, cams):
    """cams: [(w2c, K, image uint8 (h, w, 3))] in table order; the last camera that sees a point colours it.  -> (n, 3) uint8, seen."""
    rgb = np.zeros((p.shape[0], 3), np.uint8)
    seen = np.zeros(p.shape[0], bool)
    for w2c, K, image in cams:
        mask, ix, iy = project(p, w2c, K, image.shape[0], image.shape[1])
        rgb[mask] = image[iy[mask], ix[mask]]
        seen |= mask
    return rgb, seen


def in_box(p, w2l, box):
    """(mask, q): q = w2l p; inside iff |q.x| < bx / 2, |q.y| < by / 2, -bz / 2 + 0.25 < q.z < bz / 2."""
    w2l, box = np.asarray(w2l, F), np.asarray(box, F)
    q = np.stack([_row4(w2l[a], p[:, 0], p[:, 1], p[:, 2]) for a in range(3)], axis=1)
    hx, hy, hz = box[0] / 2, box[1] / 2, box[2] / 2
    mask = (q[:, 0] > -hx) & (q[:, 0] < hx) & (q[:, 1] > -hy) & (q[:, 1] < hy) & (q[:, 2] > -hz + 0.25) & (q[:, 2] < hz)
    return mask, q


def sweep(rays_o, rays_d, ranges, l2w, cams, objs):
    """One frame.  objs: [(w2l, box, visible)] in table order.  -> xyz (n, 3) float32, rgb (n, 3) uint8, labels (n,) int32: -1 unseen,
    0 background, 1 + the first visible object that holds the point (whose coordinates are then the object's own)."""
    p = world_points(rays_o, rays_d, ranges, l2w)
    rgb, seen = colours(p, cams)
    labels = np.where(seen, 0, -1).astype(np.int32)
    xyz = p.copy()
    for k, (w2l, box, visible) in enumerate(objs):
        if not visible:
            continue
        mask, q = in_box(p, w2l, box)
        take = mask & (labels == 0)
        labels[take] = k + 1
        xyz[take] = q[take]
    return xyz.astype(np.float32), rgb, labels


def pack(xyz, rgb):
    """(n, 3) float32 and (n, 3) uint8 -> (n, 4) int32, the renderer's packed points."""
    word = rgb[:, 0].astype(np.int32) | (rgb[:, 1].astype(np.int32) << 8) | (rgb[:, 2].astype(np.int32) << 16)
    return np.concatenate([np.ascontiguousarray(xyz, dtype=np.float32).view(np.int32), word[:, None]], axis=1)


# ---------------------------------------------------------------------------------------------------------------------- voxel thinning
def voxel_indices(xyz, v):
    return np.floor(np.asarray(xyz, np.float32).astype(F) / F(v)).astype(np.int64)


def voxel_keys(idx):
    if np.any(np.abs(idx) >= 1 << 20):
        raise ValueError("voxel index out of range")
    return ((idx[:, 0] + (1 << 20)) << 42) | ((idx[:, 1] + (1 << 20)) << 21) | (idx[:, 2] + (1 << 20))


def voxel_downsample(xyz, rgb, v):
    """-> xyz (voxels, 3) float32, rgb (voxels, 3) uint8 in ascending key order."""
    v = F(v)
    p = np.asarray(xyz, np.float32).astype(F)
    idx = voxel_indices(xyz, v)
    keys = voxel_keys(idx)
    frac = np.floor(((p - idx.astype(F) * v) / v) * F(2.0 ** 32))
    frac = np.clip(frac, 0.0, 4294967295.0).astype(np.uint64)
    uniq, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    count = np.zeros(len(uniq), np.uint64)
    np.add.at(count, inverse, np.uint64(1))
    pos = np.zeros((len(uniq), 3), np.uint64)
    col = np.zeros((len(uniq), 3), np.uint64)
    for a in range(3):
        np.add.at(pos[:, a], inverse, frac[:, a])
        np.add.at(col[:, a], inverse, np.asarray(rgb)[:, a].astype(np.uint64))
    scale = count.astype(F) * F(2.0 ** 32)
    out = idx[first].astype(F) * v + v * (pos.astype(F) / scale[:, None])
    colour = (np.uint64(2) * col + count[:, None]) // (np.uint64(2) * count[:, None])
    return out.astype(np.float32), colour.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the host logic of process_lidar.py
def object_tables(obj, n_frames):
    """save_object_from_pt:159-171: per-frame transform, scale and visibility from the segments."""
    transform, scale, visibility = np.zeros((n_frames, 4, 4)), np.zeros((n_frames, 3)), np.zeros(n_frames)
    for seg in obj["segments"]:
        s, n = seg["start_frame"], seg["n_frames"]
        transform[s:s + n] = seg["data"]["transform"]
        scale[s:s + n] = seg["data"]["scale"]
        visibility[s:s + n] = 1
    return transform, scale, visibility


def is_object_motion(transforms, visibility):
    """process_lidar.py:265-280: the norm of the difference of the whole 4 x 4 matrices of the first and last visible frame."""
    shown = [i for i in range(len(visibility)) if visibility[i] == 1]
    first, last = (shown[0], shown[-1]) if shown else (-1, -1)
    diff = np.asarray(transforms[last], F) - np.asarray(transforms[first], F)
    return bool(np.sqrt(np.sum(diff * diff)) > 0.5)


def w2c_of(c2w):
    c2w = np.asarray(c2w, F)
    r = np.linalg.inv(c2w[:3, :3])
    return np.concatenate([r, (-r @ c2w[:3, 3])[:, None]], axis=1)


def frame_cameras(scenario, frame, cameras, load_image):
    obs = scenario["observers"]
    return [(w2c_of(obs[s]["data"]["c2w"][frame]), np.asarray(obs[s]["data"]["intr"][frame], F), np.asarray(load_image(s, frame)))
            for s in obs.keys() if s in cameras]


def scene_clouds(scenario, load_lidar, load_image, frames=None, cameras=CAMERAS, voxel_size=-1, object_voxel_size=-1):
    """The whole of build_scene_clouds on the CPU -> (bg_xyz float32, bg_rgb uint8, obj_info)."""
    lidar = scenario["observers"]["lidar_TOP"]
    frames = list(range(lidar["n_frames"])) if frames is None else list(frames)
    cand = []
    for obj in scenario["objects"].values():
        if obj["class_name"] not in CLASSES:
            continue
        transform, scale, visibility = (t[frames] for t in object_tables(obj, lidar["n_frames"]))
        if is_object_motion(transform, visibility):
            cand.append({"id": obj["id"], "class_name": obj["class_name"], "visibility": visibility, "bbox": scale, "transform_obj": transform})

    def run(objects):
        out = []
        for t, frame in enumerate(frames):
            objs = [(w2c_of(o["transform_obj"][t]), o["bbox"][t], o["visibility"][t] == 1) if o["visibility"][t] == 1 else (None, None, False)
                    for o in objects]
            out.append(sweep(*load_lidar(frame), np.asarray(lidar["data"]["l2w"][frame], F)[:3], frame_cameras(scenario, frame, cameras, load_image), objs))
        return [np.concatenate([o[i] for o in out]) for i in range(3)]

    xyz, rgb, labels = run(cand)
    obj_info = []
    for k, o in enumerate(cand):
        pts, col = xyz[labels == k + 1], rgb[labels == k + 1]
        if object_voxel_size > 0 and len(pts):
            pts, col = voxel_downsample(pts, col, object_voxel_size)
        if len(pts) < MIN_POINTS:
            continue
        obj_info.append(dict(o, point_cloud={"points": pts.astype(F), "colors": col / 255.0, "normals": np.zeros((len(pts), 3))}, ply_path=None))
    if len(obj_info) != len(cand):
        xyz, rgb, labels = run(obj_info)
    bg_xyz, bg_rgb = xyz[labels == 0], rgb[labels == 0]
    if voxel_size > 0:
        bg_xyz, bg_rgb = voxel_downsample(bg_xyz, bg_rgb, voxel_size)
    return bg_xyz, bg_rgb, obj_info
