"""TEST INFRASTRUCTURE: what a raw call of the frame path's 13 entry points (csrc/frames.hip, normals.hip, lidar_depth.hip, post.hip)
computes, on flat buffers as a C caller hands them over.  The rules on well-formed input are those of frames_reference,
normals_reference, lidar_depth_reference and splat_reference, which this module calls; it adds what a raw call additionally needs,
written from include/mudg_hip.h and DESIGN.md §12, §16, §19, §20 and never from what a kernel returned:
  * the resize rules driven by the caller's tables, a spoiled source index clamped into the source (the coefficients stay);
  * a stream's planes placed by the header's address formula, everything between them untouched;
  * counts that are added to what `hist` held; a key that is the minimum of what it held and what lands; a resolve that leaves both
    key images empty;
  * post.hip's four entry points operation by operation in fp32, fmaxf / fminf's treatment of NaN included.
Some functions take a keyword that switches one rule off (clamp=False, across=True, ...): tests/test_frame_path_cpu.py uses it to show
that a case reaches the rule (the result changes without it); the GPU tests never pass one.
tests/test_frame_path_cpu.py asserts that on well-formed input every function here equals the existing definition."""
import numpy as np

import frames_reference as fr
import lidar_depth_reference as ld
import normals_reference as nm
import splat_reference as sr
from scene_raw_reference import added

F, D = np.float32, np.float64
LINEAR, NEAREST = 0, 1
COLOUR, SEMANTIC, DEPTH = 0, 1, 2
EMPTY = sr.EMPTY
PALETTE19 = fr.PALETTE[:19].astype(np.int64)                    # post.hip's PAL: the first 19 of the 21 class colours


# ------------------------------------------------------------------------------------------------ tables (frames.hip, normal_stream)
def table_u8(n_src, n_dst):
    """(n_dst, 4) int32: s0, s1 and the 8-bit rule's coefficients (they sum to 2048)."""
    s0, s1, f = fr.linear_coords(n_src, n_dst)
    c0, c1 = fr.coefficients(f)
    return np.stack([s0, s1, c0.astype(np.int64), c1.astype(np.int64)], axis=1).astype(np.int32)


def table_nearest(n_src, n_dst):
    s = fr.nearest_coords(n_src, n_dst)
    return np.stack([s, s, np.full_like(s, 2048), np.zeros_like(s)], axis=1).astype(np.int32)


def table_f32(n_src, n_dst):
    """(n_dst, 4) int32: s0, s1 and the fp32 bit patterns of 1 - f and f."""
    s0, s1, f = fr.linear_coords(n_src, n_dst)
    w0 = (F(1) - f).astype(F)
    return np.stack([s0.astype(np.int32), s1.astype(np.int32), w0.view(np.int32), f.astype(F).view(np.int32)], axis=1)


def spoiled(table, n_src):
    """The table with s0 = -1 and s1 = n_src in its first and its last entry: one sample past either end of the axis."""
    t = np.array(table)
    t[0, 0], t[0, 1], t[-1, 0], t[-1, 1] = -1, n_src, -1, n_src
    return t


def clamped(table, n_src):
    """The rule for a source index outside the axis: it is clamped to [0, n_src - 1]; the coefficients are used as they are."""
    t = np.array(table)
    t[:, :2] = np.clip(t[:, :2], 0, n_src - 1)
    return t


def _weights(tab):
    return tab[:, 2].copy().view(F), tab[:, 3].copy().view(F)


# ------------------------------------------------------------------------------------------------ frames.hip (§16)
def resize_u8(src, xtab, ytab, mode=LINEAR, palette=False, clamp=True):
    """src (T, H0, W0, C) uint8, or (T, H0, W0) ids with the palette -> (T, H, W, C) uint8 (three channels with the palette)."""
    s = fr.colourise(src) if palette else np.asarray(src)
    assert s.dtype == np.uint8 and s.ndim == 4
    H0, W0 = s.shape[1:3]
    xt, yt = (clamped(xtab, W0), clamped(ytab, H0)) if clamp else (np.asarray(xtab), np.asarray(ytab))
    s = s.astype(np.int32)
    if mode == NEAREST:
        return s[:, yt[:, 0]][:, :, xt[:, 0]].astype(np.uint8)
    a0, a1 = (xt[:, k].astype(np.int32)[None, None, :, None] for k in (2, 3))
    b0, b1 = (yt[:, k].astype(np.int32)[None, :, None, None] for k in (2, 3))
    rows = s[:, :, xt[:, 0]] * a0 + s[:, :, xt[:, 1]] * a1
    out = (((b0 * (rows[:, yt[:, 0]] >> 4)) >> 16) + ((b1 * (rows[:, yt[:, 1]] >> 4)) >> 16) + 2) >> 2
    return (out & 255).astype(np.uint8)


def resize_f32(src, xtab, ytab, clamp=True):
    """src (T, H0, W0) or (T, H0, W0, 3) fp32 -> (T, H, W[, 3]): R = S[x0] w0 + S[x1] w1 per source row, out = R0 v0 + R1 v1, every
    operation rounded to fp32 on its own."""
    s = np.asarray(src)
    assert s.dtype == F
    H0, W0 = s.shape[1:3]
    xt, yt = (clamped(xtab, W0), clamped(ytab, H0)) if clamp else (np.asarray(xtab), np.asarray(ytab))
    shape = (1, 1, -1) + (1,) * (s.ndim - 3)
    w0, w1 = (w.reshape(shape) for w in _weights(xt))
    v0, v1 = (v.reshape((1, -1, 1) + (1,) * (s.ndim - 3)) for v in _weights(yt))
    with np.errstate(all="ignore"):
        rows = ((s[:, :, xt[:, 0]] * w0).astype(F) + (s[:, :, xt[:, 1]] * w1).astype(F)).astype(F)
        out = ((rows[:, yt[:, 0]] * v0).astype(F) + (rows[:, yt[:, 1]] * v1).astype(F)).astype(F)
    return out


def norm_table():
    """The caller's 256 values (v / 255 - 0.5) * 2, each step in fp32."""
    return fr.norm_u8(np.arange(256, dtype=np.uint8).reshape(1, 1, 256, 1).repeat(3, axis=3))[0, 0, 0].copy()


def depth_norm(d):
    """clamp(d, 0, 100) / 100, - 0.5, * 2 in that order in fp32; what is not a number stays so."""
    with np.errstate(all="ignore"):
        d = np.where(d < F(0), F(0), np.where(d > F(100), F(100), d)).astype(F)
        return (((d / F(100)).astype(F) - F(0.5)).astype(F) * F(2)).astype(F)


def dense_stream(kind, src, xtab, ytab, norm=None):
    """-> (planes (3, T, H, W) fp32, bytes (T, H, W, 3) uint8 or None for depth)."""
    if kind == DEPTH:
        d = depth_norm(resize_f32(src, xtab, ytab))
        return np.ascontiguousarray(np.broadcast_to(d[None], (3,) + d.shape)), None
    u8 = resize_u8(src, xtab, ytab, LINEAR, palette=kind == SEMANTIC)
    return np.ascontiguousarray(np.asarray(norm, dtype=F)[u8].transpose(3, 0, 1, 2)), u8


def normal_stream(src, xtab, ytab):
    """(T, H0, W0, 3) fp32 -> planes (3, T, H, W) fp32: resize_f32's rule on every channel, nothing else."""
    return np.ascontiguousarray(resize_f32(src, xtab, ytab).transpose(3, 0, 1, 2))


def stream_offsets(T, H, W, stream_stride, channel_stride, frame_stride, slab, frame0):
    """(3, T, H, W) int64: the float of dst that value (c, t, y, x) goes to, by the header's formula."""
    c, t, y, x = np.meshgrid(np.arange(3), np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    return (slab * stream_stride + (frame0 + t) * frame_stride + c * channel_stride + y * W + x).astype(np.int64)


def placed(before, planes, offsets):
    """The destination afterwards: `before` (flat) with the planes stored at their offsets; every other element as it was."""
    out = np.array(before).reshape(-1)
    assert offsets.min() >= 0 and offsets.max() < out.size and len(np.unique(offsets)) == offsets.size
    out[offsets.reshape(-1)] = np.asarray(planes).reshape(-1).view(out.dtype)
    return out


# ------------------------------------------------------------------------------------------------ normals.hip (§19)
def depth_normals(depth, table, labels=None, sky_label=10, min_depth=0.0, max_depth=100.0, max_rel_step=-1.0, across=False):
    """depth (frames, H, W) fp32, table (frames, 4) doubles -> normals (frames, H, W, 3) fp32, valid (frames, H, W) uint8.  A negative
    step limit is none.  A neighbour is in the frame: the row above a frame's first row is absent, whatever lies before it in memory
    (across=True takes the frames as one tall image instead: what a kernel without the frame test would compute, with frame 0's table)."""
    r = None if max_rel_step < 0 else max_rel_step
    kw = dict(sky_label=sky_label, min_depth=min_depth, max_depth=max_depth, max_rel_step=r)
    if across:
        f, H, W = depth.shape
        n, v = nm.depth_normals(depth.reshape(f * H, W), table[0], None if labels is None else labels.reshape(f * H, W), **kw)
        return n.reshape(f, H, W, 3), v.reshape(f, H, W)
    return nm.depth_normals_frames(depth, table, labels, **kw)


def metric_normals(pred_u8, gt, valid, start):
    """(frames, H, W, 3) uint8 and fp32, (frames, H, W) bytes or None, start (frames, 720) uint64 -> the counts added to start."""
    hists = [nm.normal_hist(pred_u8[f], gt[f], None if valid is None else valid[f]) for f in range(len(pred_u8))]
    return added(start, np.stack(hists))


# ------------------------------------------------------------------------------------------------ lidar_depth.hip (§20)
def candidate_points(segments):
    """segments (nseg, 2) = (first point, length) -> the cloud index of every candidate, in candidate order."""
    return np.concatenate([np.arange(a, a + n, dtype=np.int64) for a, n in np.asarray(segments, dtype=np.int64).reshape(-1, 2)])


def key_depth(keys):
    """The high word of every key as fp32."""
    return (np.asarray(keys, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32).view(F)


def make_keys(depth, index):
    return (np.asarray(depth, dtype=F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(index).astype(np.uint64)


def hidden(zc, u, v, Z, reach, rel_keep, directions=ld.DIRECTIONS, both_sides=True):
    """Z: the occluder key image (H, W) uint64.  near(q) iff q is in the image, Z[q] is not all ones and its depth < fp32(zc rel_keep);
    hidden iff for one direction some home + k d and some home - k' d, k, k' in 1 .. reach, are near (both_sides=False: either)."""
    H, W = Z.shape
    depth, there = key_depth(Z), Z != EMPTY
    jh, ih = np.floor(v).astype(np.int64), np.floor(u).astype(np.int64)
    limit = (zc * F(rel_keep)).astype(F)

    def near(j, i):
        inside = (j >= 0) & (j < H) & (i >= 0) & (i < W)
        jj, ii = np.clip(j, 0, H - 1), np.clip(i, 0, W - 1)
        return inside & there[jj, ii] & (depth[jj, ii] < limit)

    out = np.zeros(len(zc), dtype=bool)
    for dj, di in directions:
        plus, minus = np.zeros(len(zc), dtype=bool), np.zeros(len(zc), dtype=bool)
        for k in range(1, reach + 1):
            plus |= near(jh + k * dj, ih + k * di)
            minus |= near(jh - k * dj, ih - k * di)
        out |= (plus & minus) if both_sides else (plus | minus)
    return out


def lidar_splat_visible(xyz, ids, segments, mats, occluder_keys, keys, cam, size, reach=4, rel_keep=0.95, index_base=0, znear=sr.ZNEAR,
                        zfar=sr.ZFAR, minimum=True, **knobs):
    """xyz (n, 3) fp32 the cloud, ids (n,) or None, segments (nseg, 2), mats (nmat, 3, 4), occluder_keys (H, W) uint64 or None, keys
    (H, W) uint64 as they stand -> (keys afterwards, hidden (candidates,) bool).  A candidate's number is its place among the runs (a
    point that two runs name is two candidates); its id is read at its place in the cloud."""
    H, W = keys.shape
    at = candidate_points(segments)
    pts = np.asarray(xyz, dtype=F)[at]
    m = np.asarray(mats, dtype=F).reshape(-1, 3, 4)
    index, key, rows, rok, cols, cok, u, v = sr.sprites(pts, m if ids is not None else m[0], cam, size, H, W, znear, zfar, None if ids is None else np.asarray(ids)[at])
    zc = key_depth(key)
    key = make_keys(zc, (index_base + index) & 0xFFFFFFFF)
    hid = np.zeros(len(index), dtype=bool) if occluder_keys is None else hidden(zc, u, v, np.asarray(occluder_keys, dtype=np.uint64), reach, rel_keep, **knobs)
    out = np.array(keys, dtype=np.uint64).reshape(H * W)
    if not minimum:
        out[:] = EMPTY
    for a in range(rows.shape[1]):
        for b in range(cols.shape[1]):
            sel = rok[:, a] & cok[:, b] & ~hid
            if sel.any():
                np.minimum.at(out, rows[sel, a] * W + cols[sel, b], key[sel])
    whole = np.zeros(len(at), dtype=bool)
    whole[index] = hid
    return out.reshape(H, W), whole


def lidar_depth_resolve(keys):
    """-> (depth fp32 like keys: the key's high word, bit for bit, 0 where the key is all ones; a key image of all ones: what keys —
    and the occluder keys, if given — hold afterwards)."""
    keys = np.asarray(keys, dtype=np.uint64)
    depth = np.where(keys == EMPTY, np.uint32(0), (keys >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(F)
    return depth, np.full(keys.shape, EMPTY, dtype=np.uint64)


def complete_scratch(frames, H, W):
    """The header's formula: x and the row maxima, fp32, and the stage bytes, each rounded up to 16 bytes."""
    px = frames * H * W
    r16 = lambda v: (v + 15) // 16 * 16
    return 2 * r16(4 * px) + r16(px)


def depth_complete(depth, labels=None, sky_label=10, max_depth=100.0, extrapolate=True, source=True, across=False):
    """(frames, H, W) fp32 -> (out fp32, source uint8 or None).  Every step's neighbourhood ends at the frame (across=True: the frames
    as one tall image, what a halo taken across the frame boundary would give)."""
    if across:
        f, H, W = depth.shape
        out, src = ld.complete_depth(depth.reshape(f * H, W), None if labels is None else labels.reshape(f * H, W), max_depth=max_depth,
                                     extrapolate=bool(extrapolate), sky_label=sky_label)
        out, src = out.reshape(f, H, W), src.reshape(f, H, W)
    else:
        out, src = ld.complete_depth_frames(depth, labels, max_depth=max_depth, extrapolate=bool(extrapolate), sky_label=sky_label)
    return out, (src if source else None)


# ------------------------------------------------------------------------------------------------ post.hip
def _fmax(x, lo):
    """fmaxf(x, lo): the other operand where one is not a number."""
    return np.where(np.isnan(x), F(lo), np.maximum(x, F(lo))).astype(F)


def _fmin(x, hi):
    return np.where(np.isnan(x), F(hi), np.minimum(x, F(hi))).astype(F)


def clamp_unit(x, nan_to_low=True):
    """fminf(fmaxf(x, -1), 1): NaN becomes -1 (nan_to_low=False: NaN stays, as in torch.clamp — then its byte is undefined)."""
    x = np.asarray(x, dtype=F)
    return _fmin(_fmax(x, -1), 1) if nan_to_low else np.minimum(np.maximum(x, F(-1)), F(1)).astype(F)


def _truncate(g):
    """(uint8)(int) g, truncation toward zero, for -1 < g < 256; the header defines no byte for anything else."""
    assert bool(((g > -1) & (g < 256)).all()), "a value whose byte the header does not define"
    return np.trunc(g).astype(np.int64).astype(np.uint8)


def frames_to_u8(video):
    """(B, C, T, HW) fp32 -> (B, T, HW, C) uint8: clamp, + 1, / 2, * 255 each rounded to fp32, truncated."""
    x = clamp_unit(video)
    g = (((x + F(1)).astype(F) / F(2)).astype(F) * F(255)).astype(F)
    return np.ascontiguousarray(_truncate(g).transpose(0, 2, 3, 1))


def log_sheet(video, clamp, rescale):
    """(N, C, T, H, W) fp32, C = 1 or 3 -> (T, N H, W, 3) uint8."""
    x = np.asarray(video, dtype=F)
    N, C, T, H, W = x.shape
    if clamp:
        x = clamp_unit(x)
    if rescale:
        x = ((x + F(1)).astype(F) / F(2)).astype(F)
    b = _truncate((x * F(255)).astype(F))
    if C == 1:
        b = np.repeat(b, 3, axis=1)
    return np.ascontiguousarray(b.transpose(2, 0, 3, 4, 1).reshape(T, N * H, W, 3))


def depth_from_u8(frames):
    """(n, 3) uint8 -> (n,) fp32: ((r + g) + b) / 3 / 255, every operation in fp32."""
    f = np.asarray(frames).astype(F)
    s = ((f[:, 0] + f[:, 1]).astype(F) + f[:, 2]).astype(F)
    return ((s / F(3)).astype(F) / F(255)).astype(F)


def palette_distances(img):
    """(3, hw) uint8 -> (19, hw) integer squared distances to the palette."""
    p = np.asarray(img).astype(np.int64)
    return ((p[None] - PALETTE19[:, :, None]) ** 2).sum(axis=1)


def semantic_nearest(img, first=True):
    """(3, hw) uint8 -> (vis (3, hw) uint8, labels (hw,) int64): the nearest palette colour, the first of equals (first=False: the last)."""
    d = palette_distances(img)
    labels = np.argmin(d, axis=0) if first else 18 - np.argmin(d[::-1], axis=0)
    return np.ascontiguousarray(PALETTE19[labels].T.astype(np.uint8)), labels.astype(np.int64)
