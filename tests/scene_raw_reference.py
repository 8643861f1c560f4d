"""TEST INFRASTRUCTURE: what a raw call of the scene half's 18 entry points (csrc/cloud.hip, neighbours.hip, depth.hip, consistency.hip,
metrics.hip) computes, on flat buffers as a C caller hands them over.  The rules on well-formed input are those of cloud_reference,
neighbours_reference, depth_reference, consistency_reference and metrics_reference, which this module calls; it adds what a raw call
additionally needs, written from the kernels' comments and DESIGN.md §13-§15, §21, §22 and never from what a kernel returned:
  * sums that are added into whatever the buffer holds (modulo 2^64), and the one word that is stored (the voxel key);
  * slots that stay unwritten: None in a result here means "the buffer keeps what it held";
  * what a spoiled table entry does: it is dropped, and nothing else changes.
tests/test_scene_cpu.py asserts that on well-formed input every function here equals the existing definition."""
import numpy as np

import cloud_reference as cr
import consistency_reference as vr
import depth_reference as dr
import metrics_reference as mr
import neighbours_reference as nr

F, D = np.float32, np.float64
MASK64 = (1 << 64) - 1
FIELD = (1 << 21) - 1                                          # a key's field per axis
HALF = 1 << 20


def added(start, sums):
    """start (any shape) uint64 + Python integers of the same shape, modulo 2^64 -> uint64."""
    start = np.asarray(start, dtype=np.uint64)
    flat = [(int(a) + int(b)) & MASK64 for a, b in zip(start.reshape(-1), np.asarray(sums, dtype=object).reshape(-1))]
    return np.array(flat, dtype=np.uint64).reshape(start.shape)


# ------------------------------------------------------------------------------------------------ depth.hip (§14)
def align_sums(frames_u8, lidar, start):
    """(F, H, W, 3) uint8, (F, H, W) fp32, start (F, 5) uint64 -> (F, 5) uint64: the five sums of each frame added to start."""
    return added(start, [dr.align_sums(f, y) for f, y in zip(frames_u8, lidar)])


def align_solve(sums):
    """(F, 5) uint64 -> coef (F, 2) float64, fitted (F,) uint8.  The words are read as unsigned and rounded to fp64 once."""
    lines = [dr.align_solve(tuple(int(v) for v in row)) for row in np.asarray(sums, dtype=np.uint64)]
    return np.array([[m, c] for m, c, _ in lines], dtype=D), np.array([f for _, _, f in lines], dtype=np.uint8)


def finish(frames_u8, coef, labels=None, sky_label=10):
    """-> depth (F, H, W) fp32, vis (F, H, W, 3) uint8."""
    done = [dr.finish(f, coef[t, 0], coef[t, 1], None if labels is None else labels[t], sky_label) for t, f in enumerate(frames_u8)]
    return np.stack([d for d, _ in done]), np.stack([v for _, v in done])


def colormap(values, val_min, val_max, reversed):
    """(n,) fp32 -> bytes (n, 3) uint8, colours (n, 3) fp32."""
    return dr.colormap(values, val_min, val_max, reversed, bytes=True), dr.colormap(values, val_min, val_max, reversed, bytes=False)


def unproject(depth, rgb, table, labels=None, sky_label=10, min_depth=0.0, max_depth=100.0):
    """(F, H, W) fp32, (F, H, W, 3) uint8, (F, 16) float64 -> points (F H W, 4) int32, valid (F H W,) uint8."""
    done = [dr.unproject(depth[t], rgb[t], table[t], None if labels is None else labels[t], sky_label, min_depth, max_depth) for t in range(len(depth))]
    return np.concatenate([p for p, _ in done]), np.concatenate([v for _, v in done])


# ------------------------------------------------------------------------------------------------ consistency.hip (§21)
def view_flags(depth, labels=None, sky_label=10, dynamic_mask=vr.DYNAMIC_MASK, min_depth=0.0, max_depth=100.0):
    return vr.flags(depth, labels, sky_label, dynamic_mask, min_depth, max_depth)


def kept_witnesses(witnesses, V):
    """(V, N) int32 -> the boolean (V, N) of the entries that are a witness: an id below 0 (empty, or any other negative number), an id
    of V or more, and the view's own id give no evidence and are skipped; nothing is read at such an id."""
    w = np.asarray(witnesses, dtype=np.int64)
    return (w >= 0) & (w < V) & (w != np.arange(V)[:, None])


def view_consistency(depth, flags, src_table, wit_table, times, witnesses, start, *, r, min_agree, max_violate, rel_tol, abs_tol):
    """depth (V, H, W) fp32, flags (V, H, W) uint8 as given (not derived here), the (V, 16) tables, times (V,), witnesses (V, N) of any
    int32 -> agree, violate, keep (V, H, W) uint8 and start (V, 6) uint64 with the six sums of each view added."""
    depth, flags = np.asarray(depth, dtype=F), np.asarray(flags, dtype=np.uint8)
    V = depth.shape[0]
    ok = kept_witnesses(witnesses, V)
    agree, violate = np.zeros(depth.shape, dtype=np.int64), np.zeros(depth.shape, dtype=np.int64)
    for s in range(V):
        usable, dynamic = (flags[s] & 1) != 0, (flags[s] & 2) != 0
        P = vr.world_points(depth[s], src_table[s])
        for n, w in enumerate(witnesses[s]):
            if not ok[s, n]:
                continue
            w = int(w)
            same_time = bool(times[w] == times[s])
            active = usable if same_time else usable & ~dynamic
            a, b, _ = vr.verdicts(P, active, same_time, wit_table[w], depth[w], flags[w], r, rel_tol, abs_tol)
            agree[s] += a
            violate[s] += b
    usable = (flags & 1) != 0
    keep = usable & (agree >= min_agree) & (violate <= max_violate)
    per_view = lambda a: [int(x) for x in a.reshape(V, -1).sum(axis=1)]
    sums = np.array([per_view(usable), per_view((agree + violate) > 0), per_view(keep), per_view(agree), per_view(violate), per_view(violate > 0)],
                    dtype=object).T
    return agree.astype(np.uint8), violate.astype(np.uint8), keep.astype(np.uint8), added(start, sums)


# ------------------------------------------------------------------------------------------------ metrics.hip (§15)
def metric_sse(a, b, start):
    return added(start, [mr.sse(x, y) for x, y in zip(a, b)])


def metric_ssim(a, b, start):
    """start (F,) as uint64 words: the signed sum of q is added modulo 2^64."""
    return added(start, [mr.ssim_sum(x, y) for x, y in zip(a, b)])


def metric_depth(z, y, start, min_depth, max_depth):
    """start (F, 8) uint64: seven sums are added, the eighth word (spare) is left as it is."""
    return added(start, [mr.depth_sums(z[f], y[f], min_depth, max_depth) for f in range(len(z))])


def metric_confusion(pred, gt, classes, start, start_bad):
    """pred, gt (F, H W) int64 of any value; start (F, classes, classes), start_bad (F,) uint64.  A pixel whose gt is outside [0, classes)
    is not counted at all, one whose prediction is outside adds to bad."""
    pairs = [mr.confusion(pred[f], gt[f], classes) for f in range(len(pred))]
    return added(start, np.stack([p[0] for p in pairs])), added(start_bad, [p[1] for p in pairs])


# ------------------------------------------------------------------------------------------------ neighbours.hip (§22)
def sorted_reference(ref, r):
    """(n, 3) fp32 -> what the search takes: the key-sorted points, their keys and the original index of each (a stable sort)."""
    ref = np.asarray(ref, F).reshape(-1, 3)
    cell = nr.cell_edge(r)
    keys = nr.cell_keys(np.floor(nr.cell_quotients(ref, cell)).astype(np.int64))
    order = np.argsort(keys, kind="stable")
    return ref[order], keys[order], order.astype(np.int64), float(cell)


def visited(visit, nq):
    """The queries that some lane owns: lane j < nq owns query visit[j] (j itself without a table); an entry outside [0, nq) is dropped,
    an entry that occurs twice is computed twice with the same result.  A query that no lane owns keeps its slot."""
    if visit is None:
        return np.ones(nq, dtype=bool)
    v = np.asarray(visit, dtype=np.int64)[:nq]
    out = np.zeros(nq, dtype=bool)
    out[v[(v >= 0) & (v < nq)]] = True
    return out


def cloud_nearest(ref_sorted, order, queries, visit, r):
    """-> d2 (nq,) float64, index (nq,) int64, owned (nq,) bool.  The index is order[s] of the attaining sorted position s, the lowest
    such value on a tie; `order` is only ever returned, whatever it holds."""
    nq = len(queries)
    best, index = np.full(nq, np.inf), np.full(nq, -1, dtype=np.int64)
    order = np.asarray(order, dtype=np.int64)
    for s, d2 in nr.within_reach(ref_sorted, queries, r):
        m = d2.min(axis=1)
        attains = np.isfinite(d2) & (d2 == m[:, None])
        low = np.where(attains, order[None, :], np.iinfo(np.int64).max).min(axis=1)
        best[s:s + len(m)] = m
        index[s:s + len(m)] = np.where(np.isfinite(m), low, -1)
    return best, index, visited(visit, nq)


def cloud_count(ref_sorted, queries, visit, r, cap):
    return nr.counts(ref_sorted, queries, r, cap), visited(visit, len(queries))


def metric_cloud(d2, t2, r2, start):
    """start (2 + K,) uint64."""
    return added(start, nr.cloud_sums(d2, t2, r2))


# ------------------------------------------------------------------------------------------------ cloud.hip (§13)
def raw_colours(p, cams, images, image_bytes):
    """cams: [(w2c (3, 4), K (3, 3), h, w, base)] in table order, images: the flat uint8 buffer, image_bytes: its length as the call
    states it.  A camera sees the point iff the pixel is inside its h x w and the pixel's three bytes at base + (iy w + ix) 3 lie inside
    [0, image_bytes); the last camera that sees it colours it.  -> rgb (n, 3) uint8, seen (n,), refused (n,) int: the number of cameras
    whose inside test passed and whose address did not."""
    rgb, seen, refused = np.zeros((p.shape[0], 3), np.uint8), np.zeros(p.shape[0], bool), np.zeros(p.shape[0], np.int64)
    for w2c, K, h, w, base in cams:
        mask, ix, iy = cr.project(p, w2c, K, h, w)
        at = int(base) + (iy.astype(np.int64) * int(w) + ix.astype(np.int64)) * 3
        ok = mask & (at >= 0) & (at + 3 <= int(image_bytes))
        refused += mask & ~ok
        for c in range(3):
            rgb[ok, c] = images[at[ok] + c]
        seen |= ok
    return rgb, seen, refused


def raw_sweep_frame(rays_o, rays_d, ranges, l2w, cams, objs, images, image_bytes):
    """cloud_reference.sweep with raw_colours in the place of colours."""
    p = cr.world_points(rays_o, rays_d, ranges, l2w)
    rgb, seen, refused = raw_colours(p, cams, images, image_bytes)
    labels = np.where(seen, 0, -1).astype(np.int32)
    xyz = p.copy()
    for k, (w2l, box, visible) in enumerate(objs):
        if not visible:
            continue
        mask, q = cr.in_box(p, w2l, box)
        take = mask & (labels == 0)
        labels[take] = k + 1
        xyz[take] = q[take]
    return xyz.astype(np.float32), rgb, labels, refused


def cloud_sweep(rays_o, rays_d, ranges, offsets, total, max_rays, l2w, cams, objs, images, image_bytes):
    """offsets (frames + 1,) int64 of any value.  Frame f owns the returns first + i, 0 <= i < offsets[f + 1] - first (none for a count
    that is not positive); a return outside [0, total) is dropped.  cams[f], objs[f]: the frame's tables.  -> packed (total, 4) int32,
    labels (total,) int32, written (total,) bool (a return that no frame owns keeps its slots), and the counts of returns dropped by
    the offset check and of (return, camera) pairs refused by the address check.  Two frames must not own the same return."""
    frames = len(offsets) - 1
    packed, labels, written = np.zeros((total, 4), np.int32), np.zeros(total, np.int32), np.zeros(total, bool)
    dropped = refused = 0
    for f in range(frames):
        first, count = int(offsets[f]), int(offsets[f + 1]) - int(offsets[f])
        assert count <= max_rays, "which returns beyond max_rays a launch visits is not part of the rule"
        idx = np.arange(first, first + max(count, 0))
        inside = (idx >= 0) & (idx < total)
        dropped += int((~inside).sum())
        idx = idx[inside]
        if len(idx) == 0:
            continue
        assert not written[idx].any()
        xyz, rgb, lab, ref = raw_sweep_frame(rays_o[idx], rays_d[idx], ranges[idx], l2w[f], cams[f], objs[f], images, image_bytes)
        packed[idx], labels[idx], written[idx] = cr.pack(xyz, rgb), lab, True
        refused += int(ref.sum())
    return packed, labels, written, dropped, refused


def voxel_keys(xyz, v):
    """A voxel index outside [-2^20, 2^20) (which the host refuses) keeps its low 21 bits after the offset: the key wraps modulo 2^21
    per axis."""
    idx = cr.voxel_indices(xyz, v)
    u = (idx + HALF) & FIELD
    return (u[:, 0] << 42) | (u[:, 1] << 21) | u[:, 2]


def voxel_reduce(packed, order, segments, v, start):
    """packed (n, 4) int32, order and segments (n,) int64 of any value, start (voxels, 8) uint64.  Entry j names point order[j] and voxel
    segments[j]; an entry whose point is outside [0, n) or whose voxel is outside [0, voxels) is dropped.  Every other entry adds 1, its
    three colour bytes and its three in-voxel offsets (taken from the true index, not the wrapped one) to words 0 .. 6 of its voxel and
    stores its key in word 7.  -> (voxels, 8) uint64, and the number of dropped entries."""
    n, voxels = len(packed), len(start)
    xyz = np.ascontiguousarray(packed[:, :3]).view(F)
    word = packed[:, 3].astype(np.int64) & 0xFFFFFFFF
    idx = cr.voxel_indices(xyz, v)
    keys = voxel_keys(xyz, v)
    with np.errstate(all="ignore"):
        frac = np.floor(((xyz.astype(D) - idx.astype(D) * D(v)) / D(v)) * D(2.0 ** 32))
    frac = np.where(frac >= 0, frac, 0.0)                                              # not a number: 0
    frac = np.where(frac <= 4294967295.0, frac, 4294967295.0).astype(np.uint64)
    out = [[int(x) for x in row] for row in np.asarray(start, dtype=np.uint64)]
    dropped = 0
    for j in range(n):
        src, s = int(order[j]), int(segments[j])
        if not (0 <= src < n and 0 <= s < voxels):
            dropped += 1
            continue
        adds = (1, word[src] & 255, (word[src] >> 8) & 255, (word[src] >> 16) & 255, frac[src, 0], frac[src, 1], frac[src, 2])
        for k, a in enumerate(adds):
            out[s][k] = (out[s][k] + int(a)) & MASK64
        out[s][7] = int(keys[src])
    return np.array(out, dtype=np.uint64), dropped


def voxel_finish(sums, v):
    """(voxels, 8) uint64 -> (voxels, 4) int32: a voxel whose count is 0 is a zero point; otherwise per axis i = the key's field - 2^20,
    coordinate fp32(i v + v (double(S) / (double(count) 2^32))), colour (2 S + count) / (2 count) in integers."""
    out = np.zeros((len(sums), 4), dtype=np.uint32)
    for k, row in enumerate(np.asarray(sums, dtype=np.uint64)):
        cnt, key = int(row[0]), int(row[7])
        if cnt == 0:
            continue
        scale = D(float(cnt)) * D(2.0 ** 32)
        for a in range(3):
            i = ((key >> (42 - 21 * a)) & FIELD) - HALF
            mean = D(v) * (D(float(int(row[4 + a]))) / scale)
            out[k, a] = F(D(float(i)) * D(v) + mean).view(np.uint32)
        r, g, b = (((2 * int(row[1 + c]) + cnt) & MASK64) // (2 * cnt) for c in range(3))
        out[k, 3] = (r | (g << 8) | (b << 16)) & 0xFFFFFFFF
    return out.view(np.int32)
