"""TEST INFRASTRUCTURE: the CPU definition of the metric-depth and view-lifting rules, in numpy, written from the rules
and not from the kernels.  The sums are Python integers; every floating-point operation is a single correctly rounded numpy operation of
the stated precision in the stated order.  Nothing in the product imports it."""
import numpy as np

F = np.float32
D = np.float64
Q_SCALE = 2 ** 20
SPECTRAL = np.array([(0.61960784313725492, 0.003921568627450980, 0.25882352941176473),
                     (0.83529411764705885, 0.24313725490196078, 0.30980392156862746),
                     (0.95686274509803926, 0.42745098039215684, 0.2627450980392157),
                     (0.99215686274509807, 0.68235294117647061, 0.38039215686274508),
                     (0.99607843137254903, 0.8784313725490196, 0.54509803921568623),
                     (1.0, 1.0, 0.74901960784313726),
                     (0.90196078431372551, 0.96078431372549022, 0.59607843137254901),
                     (0.6705882352941176, 0.8666666666666667, 0.64313725490196083),
                     (0.4, 0.76078431372549016, 0.6470588235294118),
                     (0.19607843137254902, 0.53333333333333333, 0.74117647058823533),
                     (0.36862745098039218, 0.30980392156862746, 0.63529411764705879)]).astype(F)


def k_of(frame_u8):
    """(..., 3) uint8 -> r + g + b as int64, 0 .. 765."""
    return np.asarray(frame_u8).astype(np.int64).sum(axis=-1)


def counted(k, lidar):
    """The pixels of the fit: k > 0 and 0 < lidar < 256 (the upper bound keeps the sums inside 64 bits; the renderer's zfar is 200)."""
    lidar = np.asarray(lidar, dtype=F)
    return (k > 0) & (lidar > F(0)) & (lidar < F(256))


def q_of(lidar):
    """rint(lidar * 2^20) in fp64 (the product is exact), half to even, as int64."""
    with np.errstate(invalid="ignore"):                                    # what is not a number is never counted
        return np.rint(np.asarray(lidar, dtype=F).astype(D) * D(Q_SCALE)).astype(np.int64)


def align_sums(frame_u8, lidar):
    """One frame -> the five sums (n, sum k, sum k^2, sum q, sum k q) as Python integers."""
    k = k_of(frame_u8)
    use = counted(k, lidar)
    ks = [int(v) for v in k[use]]
    qs = [int(v) for v in q_of(lidar)[use]]
    return (len(ks), sum(ks), sum(a * a for a in ks), sum(qs), sum(a * b for a, b in zip(ks, qs)))


def align_solve(sums):
    """The five sums -> (m, c, fitted): fp64, one operation at a time, in the rule's order."""
    n = sums[0]
    N, Sk, Skk, Sq, Skq = (D(float(s)) for s in sums)                      # int -> double rounds to nearest
    den = N * Skk - Sk * Sk
    if n < 2 or not den > 0:
        return D(100.0), D(0.0), 0
    m1 = (N * Skq - Sk * Sq) / den
    c1 = (Sq - m1 * Sk) / N
    return m1 * D(765.0) / D(Q_SCALE), c1 / D(Q_SCALE), 1


def spectral(x, reversed=False):
    """fp32 values already on [0, 1]'s scale -> (..., 3) fp32 colours: the reference's method_custom in fp32, operation for operation."""
    x = np.asarray(x, dtype=F)
    table = SPECTRAL[::-1] if reversed else SPECTRAL
    clamped = np.where(x > F(0), x, F(0))                                  # not a number: 0
    clamped = np.where(clamped < F(1), clamped, F(1))
    pos = clamped * F(10)
    left = pos.astype(np.int64)                                            # truncation; pos >= 0
    right = np.minimum(left + 1, 10)
    d = (pos - left.astype(F))[..., None]
    out = (F(1) - d) * table[left] + d * table[right]
    assert pos.dtype == F and d.dtype == F and out.dtype == F
    return out


def to_bytes(colours):
    out = colours * F(255)
    assert out.dtype == F
    return out.astype(np.int64).astype(np.uint8)                           # truncation toward zero of a value in [0, 255]


def colormap(values, val_min=0.0, val_max=1.0, reversed=False, bytes=True):
    """visualize_depth's rescale (only when the range is not (0, 1); the bounds enter as fp32(val_min) and fp32(val_max - val_min)),
    then the Spectral rule."""
    x = np.asarray(values, dtype=F)
    if val_min != 0.0 or val_max != 1.0:
        x = (x - F(val_min)) / F(float(val_max) - float(val_min))
        assert x.dtype == F
    out = spectral(x, reversed)
    return to_bytes(out) if bytes else out


def sky_clip(z, labels=None, sky_label=10):
    """process_sky's two steps on fp64 metres: 100 where the label is sky, then the clip to [0, 100]."""
    z = np.asarray(z, dtype=D)
    if labels is not None:
        z = np.where(np.asarray(labels) == sky_label, D(100.0), z)
    return np.minimum(np.maximum(z, D(0.0)), D(100.0))


def finish(frame_u8, m, c, labels=None, sky_label=10):
    """One frame -> (depth fp32 metres, Spectral picture uint8): z = m (double(k) / 765) + c in fp64, 100 on sky, clipped to [0, 100],
    rounded to fp32; the picture is the Spectral rule on z32 / 100 (fp32)."""
    z = D(m) * (k_of(frame_u8).astype(D) / D(765.0)) + D(c)
    z32 = sky_clip(z, labels, sky_label).astype(F)
    x = z32 / F(100)
    assert z.dtype == D and x.dtype == F
    return z32, to_bytes(spectral(x))


def metric_depth(frames_u8, lidar, labels=None, sky_label=10):
    """(T, H, W, 3) uint8, (T, H, W) fp32 [, (T, H, W) labels] -> dict of arrays named as the product's metric_depth names them, plus
    "sums" (T, 5) as Python integers."""
    sums = [align_sums(f, y) for f, y in zip(frames_u8, lidar)]
    lines = [align_solve(s) for s in sums]
    done = [finish(f, m, c, None if labels is None else labels[t], sky_label) for t, (f, (m, c, _)) in enumerate(zip(frames_u8, lines))]
    return {"sums": sums, "coef": np.array([[m, c] for m, c, _ in lines], dtype=D), "fitted": np.array([f for _, _, f in lines], dtype=np.uint8),
            "depth": np.stack([d for d, _ in done]), "vis": np.stack([v for _, v in done])}


def row(m, x, y, z):
    """((m0 x + m1 y) + m2 z) + m3 in fp64, as §13's row."""
    return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]


def unproject(depth, rgb, table, labels=None, sky_label=10, min_depth=0.0, max_depth=100.0):
    """One frame: depth (H, W) fp32, rgb (H, W, 3) uint8, table = 16 doubles (c2w's top three rows, fx, fy, cx, cy) -> packed points
    (H * W, 4) int32 and valid (H * W,) uint8; a pixel that is not valid holds a zero point."""
    H, W = depth.shape
    t = np.asarray(table, dtype=D)
    fx, fy, cx, cy = t[12:]
    z = np.asarray(depth, dtype=F).astype(D)
    i = np.arange(W, dtype=D)[None, :]
    j = np.arange(H, dtype=D)[:, None]
    xn = ((i + D(0.5)) - cx) / fx
    yn = ((j + D(0.5)) - cy) / fy
    xc, yc = xn * z, yn * z
    xyz = np.stack([row(t[4 * a:4 * a + 4], xc, yc, z) for a in range(3)], axis=-1).astype(F)
    with np.errstate(invalid="ignore"):
        valid = (z > D(min_depth)) & (z < D(max_depth))
    if labels is not None:
        valid &= np.asarray(labels) != sky_label
    c = np.asarray(rgb).astype(np.uint32)
    word = c[..., 0] | (c[..., 1] << np.uint32(8)) | (c[..., 2] << np.uint32(16))
    packed = np.concatenate([xyz.view(np.uint32), word[..., None]], axis=-1)
    packed[~valid] = 0
    return packed.reshape(H * W, 4).view(np.int32), valid.reshape(-1).astype(np.uint8)
