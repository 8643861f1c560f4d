"""TEST INFRASTRUCTURE: the CPU definition of the LiDAR depth maps and their dense completion, in numpy, written from
the rules and not from the kernels.  The raster rule is splat_reference's (its splat draws both the occluder buffer and the result: one
copy of the cover arithmetic); the per-frame returns are cloud_reference's sweep.  Every operation is a single correctly rounded one or
a selection, so the GPU tests ask for bit-equality.  Nothing in the product imports it."""
import numpy as np

import cloud_reference as cr
import splat_reference as sr

F = np.float32
ZNEAR, ZFAR = sr.ZNEAR, sr.ZFAR
DIRECTIONS = ((0, 1), (1, 0), (1, 1), (1, -1))                   # (rows, columns) per step: the row, the column, the two diagonals
EMPTY_BELOW = F(0.1)


# ------------------------------------------------------------------------------------------------ the window and the candidates
def window_frames(i, n_frames, window=(-2, 3)):
    """The frames pooled for frame i: i + window[0] .. i + window[1], each replaced by i when it is outside [0, n_frames)."""
    return [f if 0 <= f < n_frames else i for f in range(i + window[0], i + window[1] + 1)]


def frame_sweeps(scenario, load_lidar, load_image, obj_info, frames=None, cameras=cr.CAMERAS):
    """Per frame (xyz float32, rgb uint8): the returns a camera sees outside the boxes of obj_info's objects, in ray order."""
    lidar = scenario["observers"]["lidar_TOP"]
    frames = list(range(lidar["n_frames"])) if frames is None else list(frames)
    out = []
    for t, frame in enumerate(frames):
        objs = [(cr.w2c_of(o["transform_obj"][t]), o["bbox"][t], True) if o["visibility"][t] == 1 else (None, None, False) for o in obj_info]
        xyz, rgb, labels = cr.sweep(*load_lidar(frame), np.asarray(lidar["data"]["l2w"][frame], np.float64)[:3],
                                    cr.frame_cameras(scenario, frame, cameras, load_image), objs)
        out.append((xyz[labels == 0], rgb[labels == 0]))
    return out


def candidates(sweeps_xyz, objects, transform_obj, visibility, c2w, frame, window=(-2, 3)):
    """(xyz (n, 3) float32, mats (n, 3, 4) float32): the window's sweeps, a frame that occurs twice taken once, then the points of the
    objects the frame shows with w2c @ transform_obj[frame].  sweeps_xyz: per-frame (n_f, 3) arrays; objects: [(xyz, rgb)] or None."""
    xyz, mats = [], []
    for f in sorted(set(window_frames(frame, len(sweeps_xyz), window))):
        p = np.asarray(sweeps_xyz[f], dtype=F).reshape(-1, 3)
        xyz.append(p)
        mats.append(np.broadcast_to(sr.host_matrix(c2w), (len(p), 3, 4)))
    for k in range(len(objects) if objects else 0):
        if visibility[k][frame] == 1:
            p = np.asarray(objects[k][0]).astype(F)
            xyz.append(p)
            mats.append(np.broadcast_to(sr.host_matrix(c2w, transform_obj[k][frame]), (len(p), 3, 4)))
    if not xyz:
        return np.zeros((0, 3), F), np.zeros((0, 3, 4), F)
    return np.concatenate(xyz), np.concatenate(mats)


# ------------------------------------------------------------------------------------------------ visibility and the splat
def project(xyz, mats, cam, znear=ZNEAR, zfar=ZFAR):
    """§12's projection, operation by operation in float32 (as splat_reference.splat forms it): zc, u, v and znear < zc < zfar.
    A second copy of that arithmetic, of necessity: splat_reference offers only splat(), which keeps u, v and zc to itself, and the
    visibility rule needs the home pixel; that file is an existing yardstick and stays as it is.  Only the hidden test reads this
    copy — both images are drawn by sr.splat — and tests/test_lidar_depth_cpu.py ties the two together (every depth sr.splat draws is a
    zc of this function, and without the filter the map is one sr.splat of the candidates)."""
    xyz = np.asarray(xyz).astype(F)
    m = np.broadcast_to(np.asarray(mats, dtype=F), (xyz.shape[0], 3, 4))
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    fx, fy, cx, cy = (F(v) for v in cam)
    with np.errstate(all="ignore"):
        xc = ((m[:, 0, 0] * x + m[:, 0, 1] * y) + m[:, 0, 2] * z) + m[:, 0, 3]
        yc = ((m[:, 1, 0] * x + m[:, 1, 1] * y) + m[:, 1, 2] * z) + m[:, 1, 3]
        zc = ((m[:, 2, 0] * x + m[:, 2, 1] * y) + m[:, 2, 2] * z) + m[:, 2, 3]
        ok = (zc > F(znear)) & (zc < F(zfar))
        u = fx * (xc / zc) + cx
        v = fy * (yc / zc) + cy
    assert zc.dtype == F and u.dtype == F and v.dtype == F
    return zc, u, v, ok


def hidden(zc, u, v, ok, Z, reach=4, rel_tol=0.05):
    """Z: the occluder depth image (0 where empty).  near(q) iff q is in the image, Z[q] is not empty and Z[q] < fp32(zc * fp32(1 - rel_tol));
    a point is hidden iff for one direction d both some home + k d and some home - k' d, k, k' in 1 .. reach, are near."""
    H, W = Z.shape
    with np.errstate(all="ignore"):
        sane = ok & (np.abs(u) < 2.0 ** 24) & (np.abs(v) < 2.0 ** 24)            # everything else is culled before the test
        jh = np.floor(np.where(sane, v, F(0))).astype(np.int64)
        ih = np.floor(np.where(sane, u, F(0))).astype(np.int64)
        limit = zc * F(1.0 - float(rel_tol))
    assert limit.dtype == F

    def near(j, i):
        inside = (j >= 0) & (j < H) & (i >= 0) & (i < W)
        z = Z[np.clip(j, 0, H - 1), np.clip(i, 0, W - 1)]
        return inside & (z > 0) & (z < limit)

    out = np.zeros(len(zc), dtype=bool)
    for dj, di in DIRECTIONS:
        plus = np.zeros(len(zc), dtype=bool)
        minus = np.zeros(len(zc), dtype=bool)
        for k in range(1, reach + 1):
            plus |= near(jh + k * dj, ih + k * di)
            minus |= near(jh - k * dj, ih - k * di)
        out |= plus & minus
    return out & sane


def lidar_depth(xyz, mats, cam, H, W, point_size=2.0, occlusion=True, reach=4, rel_tol=0.05, occluder_size=1.0, znear=ZNEAR, zfar=ZFAR,
                return_hidden=False):
    """One frame: the candidates drawn at occluder_size give Z; the points Z does not hide are drawn at point_size; the depth image is the
    resolve (the key's depth, 0 where nothing landed)."""
    n = len(xyz)
    keep = np.ones(n, dtype=bool)
    if occlusion and n:
        Z = sr.splat(xyz, np.zeros((n, 3), np.uint8), mats, cam, occluder_size, H, W, znear, zfar)[1]
        keep = ~hidden(*project(xyz, mats, cam, znear, zfar), Z, reach, rel_tol)
    depth = np.zeros((H, W), F)
    if keep.any():
        depth = sr.splat(xyz[keep], np.zeros((int(keep.sum()), 3), np.uint8), np.broadcast_to(np.asarray(mats, F), (n, 3, 4))[keep], cam, point_size,
                         H, W, znear, zfar)[1]
    return (depth, ~keep) if return_hidden else depth


def lidar_depth_maps(sweeps_xyz, objects, transform_obj, visibility, intr, c2w, hw_native, hw_out=None, frame_ids=None, window=(-2, 3), **kw):
    """The whole rule for T frames -> (T, H, W) float32."""
    c2w = np.asarray(c2w, dtype=np.float64)
    T = c2w.shape[0]
    frame_ids = list(range(T)) if frame_ids is None else list(frame_ids)
    intr = np.broadcast_to(np.asarray(intr, dtype=np.float64), (T, 3, 3))
    hw_out = hw_native if hw_out is None else hw_out
    out = []
    for t in range(T):
        xyz, mats = candidates(sweeps_xyz, objects, transform_obj, visibility, c2w[t], frame_ids[t], window)
        out.append(lidar_depth(xyz, mats, sr.scaled_camera(intr[t], hw_native, hw_out), hw_out[0], hw_out[1], **kw))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ the completion
def _neighbours(x, offsets, outside, mode="constant"):
    """(len(offsets), H, W): x at every offset (rows, columns); what is outside the image is `outside` (or the border, mode="edge")."""
    r = max(max(abs(a), abs(b)) for a, b in offsets)
    H, W = x.shape
    pad = np.pad(x, r, mode="edge") if mode == "edge" else np.pad(x, r, mode="constant", constant_values=outside)
    return np.stack([pad[r + a:r + a + H, r + b:r + b + W] for a, b in offsets])


def _box(k):
    return [(a, b) for a in range(-k, k + 1) for b in range(-k, k + 1)]


DIAMOND = [(a, b) for a, b in _box(2) if abs(a) + abs(b) <= 2]
BLUR = np.outer([1.0, 4.0, 6.0, 4.0, 1.0], [1.0, 4.0, 6.0, 4.0, 1.0]).reshape(-1)


def step1(d, max_depth=100.0):
    with np.errstate(all="ignore"):
        d = np.asarray(d, dtype=F)
        x = np.where(d > EMPTY_BELOW, F(max_depth) - d, F(0)).astype(F)
        return np.where(x >= EMPTY_BELOW, x, F(0)).astype(F)                    # not a number, infinite, too far: empty, and 0


def step2(x):
    return _neighbours(x, DIAMOND, F(0)).max(axis=0)


def step3(x):
    x = _neighbours(x, _box(2), F(0)).max(axis=0)
    return _neighbours(x, _box(2), F(np.inf)).min(axis=0)                       # outside the image: absent from the minimum


def step4(x):
    return np.where(x < EMPTY_BELOW, _neighbours(x, _box(3), F(0)).max(axis=0), x)


def step5(x):
    has = x >= EMPTY_BELOW
    first = np.argmax(has, axis=0)                                              # the first filled row of a column (0 when none is)
    above = (np.arange(x.shape[0])[:, None] < first[None, :]) & has.any(axis=0)[None, :]
    x = np.where(above, x[first, np.arange(x.shape[1])][None, :], x)
    rows = _neighbours(x, [(0, b) for b in range(-15, 16)], F(0)).max(axis=0)  # a maximum over a box is the maximum of its rows' maxima
    return np.where(x < EMPTY_BELOW, _neighbours(rows, [(a, 0) for a in range(-15, 16)], F(0)).max(axis=0), x)


def step6(x):
    return np.sort(_neighbours(x, _box(2), None, mode="edge"), axis=0)[12]


def step7(x):
    nb = _neighbours(x, _box(2), F(0)).astype(np.float64)                       # outside the image: empty, so it does not count
    w = BLUR[:, None, None] * (nb >= np.float64(EMPTY_BELOW))
    num, den = np.zeros(x.shape), np.zeros(x.shape)
    for k in range(25):                                                         # exact sums: any order gives these bits
        num = num + w[k] * nb[k]
        den = den + w[k]
    with np.errstate(all="ignore"):
        return np.where(x >= EMPTY_BELOW, (num / den).astype(F), x)


def complete_depth(d, labels=None, max_depth=100.0, extrapolate=True, sky_label=10, stages=False):
    """One frame (H, W) -> (dense float32, source uint8): the nine steps.  stages: also the list of x after steps 1 .. 7."""
    x1 = step1(d, max_depth)
    x4 = step4(step3(step2(x1)))
    x5 = step5(x4) if extrapolate else x4
    x6 = step6(x5)
    x7 = step7(x6)
    has = x7 >= EMPTY_BELOW
    out = np.where(has, F(max_depth) - x7, F(0)).astype(F)
    source = np.where(~has, 0, np.where(x1 >= EMPTY_BELOW, 1, np.where(x4 >= EMPTY_BELOW, 2, 3))).astype(np.uint8)
    if labels is not None:
        sky = np.asarray(labels) == sky_label
        out = np.where(sky, F(max_depth), out).astype(F)
        source = np.where(sky, 4, source).astype(np.uint8)
    assert out.dtype == F
    return (out, source, [x1, x4, x5, x6, x7]) if stages else (out, source)


def complete_depth_frames(d, labels=None, **kw):
    res = [complete_depth(d[t], None if labels is None else labels[t], **kw) for t in range(len(d))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# ------------------------------------------------------------------------------------------------ the analytic depth of street_sweeps' world
def analytic_depth(scenario, camera, frame, hw=None):
    """A ray through every pixel centre of `camera` in `frame` against mudg_amd.synthetic.street_sweeps' world — the ground z = 0, the
    walls y = +-12 and the boxes the frame has — as camera depth (H, W) float64, inf where the ray hits nothing."""
    data = scenario["observers"][camera]["data"]
    c2w, K = np.asarray(data["c2w"][frame], np.float64), np.asarray(data["intr"][frame], np.float64)
    h0, w0 = (int(v) for v in data["hw"][frame])
    H, W = (h0, w0) if hw is None else hw
    fx, fy, cx, cy = sr.scaled_camera(K, (h0, w0), (H, W)).astype(np.float64)
    j, i = np.mgrid[0:H, 0:W]
    dc = np.stack([(i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, np.ones((H, W))], axis=-1).reshape(-1, 3)
    o, d = c2w[:3, 3], dc @ c2w[:3, :3].T                                      # the ray parameter is the camera depth: dc.z = 1
    with np.errstate(all="ignore"):
        t = np.where(d[:, 2] < 0, -o[2] / d[:, 2], np.inf)
        for wall in (-12.0, 12.0):
            tw = (wall - o[1]) / d[:, 1]
            t = np.minimum(t, np.where(tw > 0, tw, np.inf))
        n_frames = scenario["observers"]["lidar_TOP"]["n_frames"]
        for obj in scenario["objects"].values():
            transform, scale, visibility = cr.object_tables(obj, n_frames)
            if visibility[frame] != 1:
                continue
            inv = np.linalg.inv(transform[frame])
            ol, dl = inv[:3, :3] @ o + inv[:3, 3], d @ inv[:3, :3].T
            t0, t1 = (-scale[frame] / 2 - ol) / dl, (scale[frame] / 2 - ol) / dl
            near, far = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
            t = np.minimum(t, np.where((near < far) & (near > 0), near, np.inf))
    return t.reshape(H, W)


def leaked(depth, g):
    """Pixels whose depth exceeds the analytic depth g by more than max(0.5, 0.05 g)."""
    with np.errstate(all="ignore"):
        return (depth > 0) & np.isfinite(g) & (depth > g + np.maximum(0.5, 0.05 * g))
