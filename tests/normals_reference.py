"""TEST INFRASTRUCTURE: the CPU definition of the surface-normal rules, in numpy, written from the rules and not from the
kernels or the product's Python: normals from a depth map, the normal stream's resize, and the histogram of angular errors with its
scores.  Every floating-point operation is a single correctly rounded numpy operation of the stated precision in the stated order; the
counts are integers.  Nothing in the product imports it."""
import numpy as np

F = np.float32
D = np.float64
BINS = 720


# ------------------------------------------------------------------------------------------------ normals from depth
def _moved(a, dj, di, fill):
    """b[j, i] = a[j + dj, i + di] where that lies in the frame, else fill."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    dst_j, src_j = slice(max(-dj, 0), H - max(dj, 0)), slice(max(dj, 0), H - max(-dj, 0))
    dst_i, src_i = slice(max(-di, 0), W - max(di, 0)), slice(max(di, 0), W - max(-di, 0))
    b[dst_j, dst_i] = a[src_j, src_i]
    return b


def depth_normals(depth, cam, labels=None, sky_label=10, min_depth=0.0, max_depth=100.0, max_rel_step=None):
    """One frame: depth (H, W) fp32 metres, cam = (fx, fy, cx, cy) -> (normals (H, W, 3) fp32, valid (H, W) uint8)."""
    fx, fy, cx, cy = (D(v) for v in cam)
    z = np.asarray(depth, dtype=F).astype(D)
    H, W = z.shape
    with np.errstate(all="ignore"):
        usable = (z > D(min_depth)) & (z < D(max_depth))                   # not a number: no
        if labels is not None:
            usable &= np.asarray(labels) != sky_label
        xn = ((np.arange(W, dtype=D)[None, :] + D(0.5)) - cx) / fx
        yn = ((np.arange(H, dtype=D)[:, None] + D(0.5)) - cy) / fy
        P = np.stack([xn * z, yn * z, z], axis=-1)                          # §14's point without the pose

        def neighbour(dj, di):
            ok = _moved(usable, dj, di, False)
            if max_rel_step is not None:
                ok &= np.abs(_moved(z, dj, di, D(0)) - z) <= D(max_rel_step) * z
            return ok[..., None], _moved(P, dj, di, D(0))

        left, Pl = neighbour(0, -1)
        right, Pr = neighbour(0, 1)
        up, Pu = neighbour(-1, 0)
        down, Pd = neighbour(1, 0)
        dx = np.where(right, Pr, P) - np.where(left, Pl, P)                 # both: central; one: with the centre; none: unused
        dy = np.where(down, Pd, P) - np.where(up, Pu, P)
        nx = dy[..., 1] * dx[..., 2] - dy[..., 2] * dx[..., 1]             # n = dy x dx
        ny = dy[..., 2] * dx[..., 0] - dy[..., 0] * dx[..., 2]
        nz = dy[..., 0] * dx[..., 1] - dy[..., 1] * dx[..., 0]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok = usable & (left | right)[..., 0] & (up | down)[..., 0] & (length > 0) & np.isfinite(length)
        n = np.stack([nx / length, ny / length, nz / length], axis=-1).astype(F)
    n[~ok] = 0
    return n, ok.astype(np.uint8)


def depth_normals_frames(depth, cams, labels=None, **kw):
    done = [depth_normals(depth[f], cams[f], None if labels is None else labels[f], **kw) for f in range(len(depth))]
    return np.stack([n for n, _ in done]), np.stack([v for _, v in done])


# ------------------------------------------------------------------------------------------------ the normal stream
def _taps(n_src, n_dst):
    """§16's sample positions of one axis, one sample at a time: (first tap, second tap, fp32 weight of the first, of the second)."""
    out = []
    for d in range(n_dst):
        f = F((D(d) + D(0.5)) * (D(n_src) / D(n_dst)) - D(0.5))
        s = int(np.floor(f))
        f = F(f - F(s))
        if s < 0:
            s, f = 0, F(0)
        if s >= n_src - 1:
            s, f = n_src - 1, F(0)
        out.append((s, min(s + 1, n_src - 1), F(F(1) - f), f))
    return out


def normal_stream(normals, hw_out):
    """(T, H0, W0, 3) fp32 -> (3, T, h, w) fp32: out = (S[y0][x0] w0 + S[y0][x1] w1) v0 + (S[y1][x0] w0 + S[y1][x1] w1) v1 per channel,
    every product and sum rounded to fp32 on its own; nothing else."""
    src = np.asarray(normals)
    assert src.dtype == F and src.ndim == 4 and src.shape[3] == 3
    h, w = hw_out
    xs, ys = _taps(src.shape[2], w), _taps(src.shape[1], h)
    x0, x1 = np.array([t[0] for t in xs]), np.array([t[1] for t in xs])
    w0, w1 = np.array([t[2] for t in xs], dtype=F)[None, :, None], np.array([t[3] for t in xs], dtype=F)[None, :, None]
    out = np.empty((src.shape[0], h, w, 3), dtype=F)
    with np.errstate(all="ignore"):
        for y, (y0, y1, v0, v1) in enumerate(ys):
            r0 = src[:, y0][:, x0] * w0 + src[:, y0][:, x1] * w1
            r1 = src[:, y1][:, x0] * w0 + src[:, y1][:, x1] * w1
            assert r0.dtype == F and r1.dtype == F
            out[:, y] = r0 * v0 + r1 * v1
    return np.ascontiguousarray(out.transpose(3, 0, 1, 2))


# ------------------------------------------------------------------------------------------------ angular errors
def cos_table():
    """T[k] = cos((k * 0.25) * (pi / 180)), k = 0 .. 720, float64."""
    return np.cos((np.arange(BINS + 1, dtype=D) * D(0.25)) * (D(np.pi) / D(180.0)))


def cosines(pred_u8, gt):
    """(..., 3) uint8 and (..., 3) fp32 -> (c float64 before the clamp, gg float64)."""
    p = 2 * np.asarray(pred_u8).astype(np.int64) - 255
    g = np.asarray(gt, dtype=F).astype(D)
    pd = p.astype(D)
    with np.errstate(all="ignore"):
        dot = (pd[..., 0] * g[..., 0] + pd[..., 1] * g[..., 1]) + pd[..., 2] * g[..., 2]
        gg = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
        c = dot / np.sqrt((p * p).sum(-1).astype(D) * gg)
    return c, gg


def bins_of(c):
    """Clamped cosines -> bin k with T[k + 1] < c <= T[k]; c = -1 in bin 719."""
    ascending = cos_table()[::-1]
    return np.minimum(BINS - np.searchsorted(ascending, c, side="left"), BINS - 1)


def normal_hist(pred_u8, gt, valid=None):
    """One frame -> 720 counts (int64)."""
    c, gg = cosines(pred_u8, gt)
    with np.errstate(all="ignore"):
        counted = (gg > 0) & np.isfinite(gg) & ~np.isnan(c)
    if valid is not None:
        counted &= np.asarray(valid) != 0
    c = np.minimum(np.maximum(c[counted], D(-1)), D(1))
    return np.bincount(bins_of(c), minlength=BINS).astype(np.int64)


def scores(hist):
    """720 counts -> {"n", "mean", "median", "a11", "a22", "a30"}: Python integers up to one float64 division each; nan without counts."""
    h = [int(v) for v in hist]
    n = sum(h)
    if n == 0:
        return {"n": 0, **{k: D("nan") for k in ("mean", "median", "a11", "a22", "a30")}}
    below, middle = 0, None
    for k, v in enumerate(h):
        below += v
        if middle is None and 2 * below >= n:
            middle = k
    return {"n": n, "mean": D(sum(v * (2 * k + 1) for k, v in enumerate(h))) / D(8 * n), "median": D(2 * middle + 1) / D(8),
            "a11": D(sum(h[:45])) / D(n), "a22": D(sum(h[:90])) / D(n), "a30": D(sum(h[:120])) / D(n)}


def choose_label(train_labels, u):
    """The label of an item for the draw u in [0, 1), with the second triple: normal takes depth's quarter."""
    if len(train_labels) == 1:
        return train_labels[0]
    if len(train_labels) == 2:
        return train_labels[0] if u > 0.5 else train_labels[1]
    assert len(train_labels) == 3
    if u < 0.25:
        return "normal" if "normal" in train_labels else "depth"
    return "semantic" if u < 0.5 else "color"
