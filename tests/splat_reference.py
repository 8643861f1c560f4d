"""TEST INFRASTRUCTURE: the CPU definition of the point-splat raster rule, in numpy, written from the rule and not
from the kernels.  Every per-point operation is a single correctly rounded float32 operation in the rule's order; the depth test is
np.minimum.at on uint64 keys (bits(zc) << 32 | index), so the result does not depend on any order.  Nothing in the product imports it."""
import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
ZNEAR, ZFAR = 1e-4, 200.0


def to_u8(rgb):
    """Colours enter as uint8; a float cloud in [0, 1] is converted once by round(c * 255)."""
    rgb = np.asarray(rgb)
    if np.issubdtype(rgb.dtype, np.floating):
        return np.clip(np.round(rgb.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    return rgb.astype(np.uint8)


def host_matrix(c2w_virtual, transform=None):
    """Host, float64: w2c = inv(c2w_virtual) (OpenCV convention), M = w2c (@ transform_obj[frame]); the top three rows cast to fp32."""
    m = np.linalg.inv(np.asarray(c2w_virtual, dtype=np.float64))
    if transform is not None:
        m = m @ np.asarray(transform, dtype=np.float64)
    return m[:3].astype(F)


def scaled_camera(intr, hw_native, hw_out):
    (h0, w0), (h, w) = hw_native, hw_out
    k = np.asarray(intr, dtype=np.float64)
    return np.array([k[0, 0] * w / w0, k[1, 1] * h / h0, k[0, 2] * w / w0, k[1, 2] * h / h0]).astype(F)


def _axis_cover(centre, half, n, span):
    """Candidate pixel indices (points, span) and whether lo <= i + 0.5 < hi holds, lo, hi and i + 0.5 formed and compared in fp32."""
    lo, hi = centre - half, centre + half                                        # float32 - float32
    first = np.floor(lo).astype(np.int64) - 1
    idx = first[:, None] + np.arange(span, dtype=np.int64)[None, :]
    mid = idx.astype(F) + F(0.5)
    ok = (lo[:, None] <= mid) & (mid < hi[:, None]) & (idx >= 0) & (idx < n)
    return idx, ok


def splat(xyz, rgb, mats, cam, size, H, W, znear=ZNEAR, zfar=ZFAR):
    """One layer at one pose.  xyz (n, 3); rgb (n, 3) uint8; mats: (3, 4) for all points or (n, 3, 4) per point, float32; cam =
    (fx, fy, cx, cy) float32.  Returns (rgb (H, W, 3) uint8, depth (H, W) float32)."""
    xyz = np.asarray(xyz).astype(F)
    rgb = to_u8(rgb)
    n = xyz.shape[0]
    m = np.broadcast_to(np.asarray(mats, dtype=F), (n, 3, 4))
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    fx, fy, cx, cy = (F(v) for v in cam)
    with np.errstate(all="ignore"):
        xc = ((m[:, 0, 0] * x + m[:, 0, 1] * y) + m[:, 0, 2] * z) + m[:, 0, 3]
        yc = ((m[:, 1, 0] * x + m[:, 1, 1] * y) + m[:, 1, 2] * z) + m[:, 1, 3]
        zc = ((m[:, 2, 0] * x + m[:, 2, 1] * y) + m[:, 2, 2] * z) + m[:, 2, 3]
        keep = (zc > F(znear)) & (zc < F(zfar))
        index = np.nonzero(keep)[0]
        xc, yc, zc = xc[keep], yc[keep], zc[keep]
        u = fx * (xc / zc) + cx
        v = fy * (yc / zc) + cy
        half = F(size) / F(2)
        # clipping to the image: a pixel of [0, W) x [0, H) can only be covered from here (also drops what is not a number)
        near = (u + half > 0) & (u - half < W) & (v + half > 0) & (v - half < H)
    index, u, v, zc = index[near], u[near], v[near], zc[near]
    assert xc.dtype == F and u.dtype == F and zc.dtype == F
    keys = np.full(H * W, EMPTY, dtype=np.uint64)
    key = (zc.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index.astype(np.uint64)
    span = int(np.ceil(size)) + 3
    cols, cok = _axis_cover(u, half, W, span)
    rows, rok = _axis_cover(v, half, H, span)
    for a in range(span):
        for b in range(span):
            sel = rok[:, a] & cok[:, b]
            if sel.any():
                np.minimum.at(keys, rows[sel, a] * W + cols[sel, b], key[sel])
    hit = keys != EMPTY
    depth = np.zeros(H * W, dtype=F)
    depth[hit] = (keys[hit] >> np.uint64(32)).astype(np.uint32).view(F)
    out = np.zeros((H * W, 3), dtype=np.uint8)
    out[hit] = rgb[(keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    return out.reshape(H, W, 3), depth.reshape(H, W)


def dilate13(mask):
    """One 13 x 13 box, pixels outside the image unset (= three dilations by a 5 x 5 box)."""
    mask = np.asarray(mask, dtype=bool)
    H, W = mask.shape
    pad = np.zeros((H + 12, W + 12), dtype=bool)
    pad[6:6 + H, 6:6 + W] = mask
    rows = np.zeros((H + 12, W), dtype=bool)
    for k in range(13):
        rows |= pad[:, k:k + W]
    out = np.zeros((H, W), dtype=bool)
    for k in range(13):
        out |= rows[k:k + H]
    return out


def merge(bg_rgb, bg_depth, obj_rgb, obj_depth):
    """generate_sparse.py:208-223: mask = all(obj_rgb > 0) dilated; the object's colour and depth under it, the background's elsewhere."""
    mask = dilate13(np.all(obj_rgb > 0, axis=2))
    return np.where(mask[:, :, None], obj_rgb, bg_rgb), np.where(mask, obj_depth, bg_depth), mask


def conditions(rgb, depth):
    """data_tools.py:53-54, 82, 93-94 -> (3, H, W) float32 each."""
    sparse = (rgb.astype(F) / F(255) - F(0.5)) * F(2)
    d = (np.clip(depth.astype(F), F(0), F(100)) / F(100) - F(0.5)) * F(2)
    assert sparse.dtype == F and d.dtype == F
    return np.ascontiguousarray(sparse.transpose(2, 0, 1)), np.repeat(d[None], 3, axis=0)


def render_conditions(bg_xyz, bg_rgb, objects, transform_obj, visibility, intr, c2w_frames, hw_native, hw_out, poses, frame_ids=None):
    """The whole rule for T frames and P poses.  objects: list of (xyz, rgb) or None; transform_obj (objects, frames, 4, 4);
    visibility (objects, frames); intr (3, 3) or (T, 3, 3); poses (T, P, 4, 4) virtual camera-to-world.  Returns arrays named as the
    product's render_conditions(..., return_images=True) names its tensors."""
    poses = np.asarray(poses, dtype=np.float64)
    T, P = poses.shape[:2]
    H, W = hw_out
    frame_ids = list(range(T)) if frame_ids is None else list(frame_ids)
    intr = np.broadcast_to(np.asarray(intr, dtype=np.float64), (T, 3, 3))
    names = ("rgb", "depth", "mask", "bg_rgb", "bg_depth", "obj_rgb", "obj_depth", "sparse_frames", "sparse_depth")
    out = {k: [[None] * T for _ in range(P)] for k in names}
    for t in range(T):
        cam = scaled_camera(intr[t], hw_native, hw_out)
        f = frame_ids[t]
        vis = [i for i in range(len(objects))] if objects else []
        vis = [i for i in vis if visibility[i][f] == 1]
        for p in range(P):
            bg_c, bg_d = splat(bg_xyz, bg_rgb, host_matrix(poses[t, p]), cam, 2.5, H, W)
            if vis:
                xyz = np.concatenate([np.asarray(objects[i][0]) for i in vis])
                rgb = np.concatenate([to_u8(objects[i][1]) for i in vis])
                mats = np.concatenate([np.broadcast_to(host_matrix(poses[t, p], transform_obj[i][f]), (len(objects[i][0]), 3, 4)) for i in vis])
                ob_c, ob_d = splat(xyz, rgb, mats, cam, 4.0, H, W)
            else:                                                   # the reference's one-point sentinel draws nothing
                ob_c, ob_d = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), F)
            rgb_m, depth_m, mask = merge(bg_c, bg_d, ob_c, ob_d)
            sparse, sdepth = conditions(rgb_m, depth_m)
            for k, val in zip(names, (rgb_m, depth_m, mask.astype(np.uint8), bg_c, bg_d, ob_c, ob_d, sparse, sdepth)):
                out[k][p][t] = val
    res = {k: np.stack([np.stack(v) for v in out[k]]) for k in names}
    for k in ("sparse_frames", "sparse_depth"):
        res[k] = np.ascontiguousarray(res[k].transpose(0, 2, 1, 3, 4))             # (P, T, 3, H, W) -> (P, 3, T, H, W)
    return res
