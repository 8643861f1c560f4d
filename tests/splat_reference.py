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


def clamp_ids(ids, nmat):
    """The rule for per-point matrix ids: an id below 0 takes matrix 0, an id of nmat or more takes matrix nmat - 1."""
    return np.clip(np.asarray(ids).astype(np.int64), 0, nmat - 1)


def sprites(xyz, mats, cam, size, H, W, znear=ZNEAR, zfar=ZFAR, ids=None):
    """What the rule draws at one pose, before the depth test: (index, key, rows, rok, cols, cok, u, v) of the points that pass the
    culling.  index (m,) int64 into the cloud, key (m,) uint64, rows / cols (m, span) int64 candidate pixel indices and rok / cok whether
    the sprite covers them, u / v (m,) float32 the image positions.  mats: (3, 4) for all points, (n, 3, 4) per point, or with ids (n,)
    a table (nmat, 3, 4) indexed by clamp_ids."""
    xyz = np.asarray(xyz).astype(F)
    n = xyz.shape[0]
    if ids is not None:
        table = np.asarray(mats, dtype=F).reshape(-1, 3, 4)
        m = table[clamp_ids(ids, table.shape[0])]
    else:
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
    key = (zc.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index.astype(np.uint64)
    span = int(np.ceil(size)) + 3
    cols, cok = _axis_cover(u, half, W, span)
    rows, rok = _axis_cover(v, half, H, span)
    return index, key, rows, rok, cols, cok, u, v


def splat_keys(xyz, mats, cam, size, H, W, znear=ZNEAR, zfar=ZFAR, ids=None, seed=None):
    """The key image (H, W) uint64 of one layer at one pose: per pixel the minimum of (bits(zc) << 32 | index) over the covering points,
    EMPTY where nothing landed.  seed: a key image to draw on top of (keys only ever decrease)."""
    index, key, rows, rok, cols, cok, _, _ = sprites(xyz, mats, cam, size, H, W, znear, zfar, ids)
    keys = np.full(H * W, EMPTY, dtype=np.uint64) if seed is None else np.array(seed, dtype=np.uint64).reshape(H * W)
    for a in range(rows.shape[1]):
        for b in range(cols.shape[1]):
            sel = rok[:, a] & cok[:, b]
            if sel.any():
                np.minimum.at(keys, rows[sel, a] * W + cols[sel, b], key[sel])
    return keys.reshape(H, W)


def covers(xyz, mats, cam, size, H, W, znear=ZNEAR, zfar=ZFAR, ids=None):
    """The number of (point, pixel) covers at one pose: what the kernel's `covered` counter adds up."""
    _, _, _, rok, _, cok, _, _ = sprites(xyz, mats, cam, size, H, W, znear, zfar, ids)
    return int((rok.sum(axis=1) * cok.sum(axis=1)).sum())


def splat(xyz, rgb, mats, cam, size, H, W, znear=ZNEAR, zfar=ZFAR, ids=None):
    """One layer at one pose.  xyz (n, 3); rgb (n, 3) uint8; mats: (3, 4) for all points or (n, 3, 4) per point (with ids: a table
    (nmat, 3, 4), see sprites), float32; cam = (fx, fy, cx, cy) float32.  Returns (rgb (H, W, 3) uint8, depth (H, W) float32)."""
    rgb = to_u8(rgb)
    keys = splat_keys(xyz, mats, cam, size, H, W, znear, zfar, ids).reshape(H * W)
    hit = keys != EMPTY
    depth = np.zeros(H * W, dtype=F)
    depth[hit] = (keys[hit] >> np.uint64(32)).astype(np.uint32).view(F)
    out = np.zeros((H * W, 3), dtype=np.uint8)
    out[hit] = rgb[(keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    return out.reshape(H, W, 3), depth.reshape(H, W)


def pack(xyz, rgb, top=0):
    """Packed points (n, 4) uint32 as they lie in HBM: x, y, z fp32 bits and r | g << 8 | b << 16 (| top << 24) in the fourth word."""
    xyz, rgb = np.asarray(xyz).astype(F), to_u8(rgb).astype(np.uint32)
    out = np.empty((xyz.shape[0], 4), dtype=np.uint32)
    out[:, :3] = xyz.view(np.uint32)
    out[:, 3] = rgb[:, 0] | rgb[:, 1] << np.uint32(8) | rgb[:, 2] << np.uint32(16) | np.asarray(top, dtype=np.uint32) << np.uint32(24)
    return out


def resolve(keys, packed_points, n):
    """Key image -> (depth float32, colour word uint32, the key image afterwards), shaped like keys: an empty key or an index >= n
    gives 0, 0; else the key's upper half as a float and the point's fourth word & 0x00ffffff.  The image is empty afterwards."""
    keys = np.asarray(keys, dtype=np.uint64)
    packed = np.asarray(packed_points, dtype=np.uint32).reshape(-1, 4)
    flat = keys.reshape(-1)
    index = (flat & np.uint64(0xFFFFFFFF)).astype(np.int64)
    hit = (flat != EMPTY) & (index < n)
    depth = np.zeros(flat.size, dtype=F)
    depth[hit] = (flat[hit] >> np.uint64(32)).astype(np.uint32).view(F)
    colour = np.zeros(flat.size, dtype=np.uint32)
    colour[hit] = packed[index[hit], 3] & np.uint32(0x00FFFFFF)
    return depth.reshape(keys.shape), colour.reshape(keys.shape), np.full(keys.shape, EMPTY, dtype=np.uint64)


def unpack_colour(words):
    """Colour words (...,) uint32 -> (..., 3) uint8."""
    w = np.asarray(words, dtype=np.uint32)
    return np.stack([w & np.uint32(0xFF), (w >> np.uint32(8)) & np.uint32(0xFF), (w >> np.uint32(16)) & np.uint32(0xFF)], axis=-1).astype(np.uint8)


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


def compose_frame(sparse, sdepth, pose_stride, T, t, bg_colour, bg_depth, obj_colour=None, obj_depth=None):
    """Frame t of P poses written into the flat float32 arrays sparse and sdepth, which hold (P, 3, T, H, W) tensors whose poses lie
    pose_stride elements apart; everything else in them is left as it was.  bg_colour / obj_colour (P, H, W) uint32 colour words and
    bg_depth / obj_depth (P, H, W) float32 as resolve() gives them; no object layer: the background alone, an empty mask.
    Returns (rgb (P, H, W, 3) uint8, depth (P, H, W) float32, mask (P, H, W) uint8)."""
    P, H, W = np.asarray(bg_depth).shape
    plane = H * W
    rgbs, depths, masks = [], [], []
    for p in range(P):
        bg_rgb = unpack_colour(bg_colour[p])
        if obj_colour is None:
            rgb, depth, mask = bg_rgb, np.asarray(bg_depth[p], dtype=F), np.zeros((H, W), bool)
        else:
            rgb, depth, mask = merge(bg_rgb, np.asarray(bg_depth[p], dtype=F), unpack_colour(obj_colour[p]), np.asarray(obj_depth[p], dtype=F))
        cond, cdepth = conditions(rgb, depth)
        for ch in range(3):
            at = p * pose_stride + (ch * T + t) * plane
            sparse[at:at + plane] = cond[ch].reshape(-1)
            sdepth[at:at + plane] = cdepth[ch].reshape(-1)
        rgbs.append(rgb), depths.append(depth), masks.append(mask.astype(np.uint8))
    return np.stack(rgbs), np.stack(depths), np.stack(masks)


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
