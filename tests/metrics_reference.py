"""The scoring rules of DESIGN.md §15 in numpy: what csrc/metrics.hip must equal bit for bit.  Sums are int64 arrays or Python integers
(every bound is stated in §15), floating point is float64, one correctly rounded operation at a time in the stated order (numpy's
elementwise operations do not contract).  A helper module of the tests; the product does not import it."""
from fractions import Fraction

import numpy as np

D = np.float64
TWO32 = 4294967296.0
C1, C2 = 6.5025, 58.5225
E_SCALE = 1048576.0
Z_TOP = 256.0
THRESHOLDS = (1.25, 1.5625, 1.953125)


def window():
    """The eleven integer taps: rint(65536 g / sum g), g_i = exp(-(i - 5)^2 / 4.5), the centre corrected so that they sum to 2^16."""
    g = np.exp(-(np.arange(11, dtype=D) - 5.0) ** 2 / 4.5)
    w = np.rint(65536.0 * g / g.sum()).astype(np.int64)
    w[5] += 65536 - int(w.sum())
    return w


WINDOW = window()


# ------------------------------------------------------------------------------------------------ colour
def sse(a, b):
    """(H, W, 3) uint8 pair -> the Python integer sum of (a - b)^2."""
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def _blur(v):
    """(H, W) int64 -> (H - 10, W - 10) int64: sum_ij w_i w_j v, rows then columns (integers: any order gives the same)."""
    H, W = v.shape
    rows = sum(int(WINDOW[k]) * v[:, k:W - 10 + k] for k in range(11))
    return sum(int(WINDOW[k]) * rows[k:H - 10 + k] for k in range(11))


def ssim_moments(x, y):
    """(H, W) uint8 pair (one channel) -> Sx, Sy, Sxx, Syy, Sxy, each (H - 10, W - 10) int64 below 2^48."""
    x, y = x.astype(np.int64), y.astype(np.int64)
    return _blur(x), _blur(y), _blur(x * x), _blur(y * y), _blur(x * y)


def ssim_value(Sx, Sy, Sxx, Syy, Sxy):
    """The per-pixel formula on integer moments (arrays or scalars), float64 in the rule's order."""
    Sx, Sy, Sxx, Syy, Sxy = (np.asarray(v, dtype=np.int64).astype(D) for v in (Sx, Sy, Sxx, Syy, Sxy))
    mx, my = Sx / TWO32, Sy / TWO32
    mxx, myy, mxy = mx * mx, my * my, mx * my
    vx = Sxx / TWO32 - mxx
    vy = Syy / TWO32 - myy
    cxy = Sxy / TWO32 - mxy
    num = (2.0 * mxy + C1) * (2.0 * cxy + C2)
    den = ((mxx + myy) + C1) * ((vx + vy) + C2)
    return num / den


def ssim_q(x, y):
    """(H, W) uint8 pair -> (H - 10, W - 10) int64, rint(s 2^32) half to even."""
    return np.rint(ssim_value(*ssim_moments(x, y)) * TWO32).astype(np.int64)


def ssim_sum(a, b):
    """(H, W, 3) uint8 pair -> the Python integer sum of q over the valid region and the three channels."""
    return sum(int(ssim_q(a[..., c], b[..., c]).sum()) for c in range(3))


def psnr_ssim(a, b):
    """(F, H, W, 3) uint8 stacks -> {"sse", "ssim_sum": (F,) int64, "psnr", "ssim": (F,) float64}."""
    F_, H, W = a.shape[:3]
    s = np.array([sse(a[f], b[f]) for f in range(F_)], dtype=np.int64)
    q = np.array([ssim_sum(a[f], b[f]) for f in range(F_)], dtype=np.int64)
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10((255.0 ** 2 * 3 * H * W) / s.astype(D))
    return {"sse": s, "ssim_sum": q, "psnr": psnr, "ssim": q.astype(D) / (TWO32 * (3 * (H - 10) * (W - 10)))}


# ------------------------------------------------------------------------------------------------ depth
def depth_sums(z32, y32, min_depth=0.1, max_depth=80.0):
    """(H, W) fp32 pair -> the eight Python integers n, sum rint(e 2^20), sum rint(e e 2^20), sum rint(r 2^20), three counts, 0."""
    y, z = y32.astype(D).reshape(-1), z32.astype(D).reshape(-1)
    use = (y > D(min_depth)) & (y < D(max_depth)) & ~np.isnan(z)
    y, z = y[use], np.minimum(np.maximum(z[use], 0.0), Z_TOP)
    e = np.abs(z - y)
    r = e / y
    with np.errstate(divide="ignore"):
        t = np.maximum(z / y, y / z)
    q = lambda v: sum(int(i) for i in np.rint(v * E_SCALE).astype(np.int64))
    return (int(use.sum()), q(e), q(e * e), q(r)) + tuple(int((t < th).sum()) for th in THRESHOLDS) + (0,)


def depth_errors(z, y, min_depth=0.1, max_depth=80.0):
    """(F, H, W) fp32 stacks -> {"sums": (F, 8) int64 and the float64 scores}, nan for a frame with n = 0."""
    sums = np.array([depth_sums(z[f], y[f], min_depth, max_depth) for f in range(z.shape[0])], dtype=np.int64)
    s = sums.astype(D)
    n = s[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"sums": sums, "n": sums[:, 0], "mae": s[:, 1] / (E_SCALE * n), "rmse": np.sqrt(s[:, 2] / (E_SCALE * n)), "abs_rel": s[:, 3] / (E_SCALE * n),
                "d1": s[:, 4] / n, "d2": s[:, 5] / n, "d3": s[:, 6] / n}


def rint_fraction(v):
    """A Fraction -> the nearest integer, half to even (Python's round on a Fraction)."""
    return int(round(v))


def depth_sums_exact(z32, y32, min_depth=0.1, max_depth=80.0):
    """The same eight integers from Python integers and Fractions, one pixel at a time.  A float64 operation is the exact rational result
    rounded once: Fraction(float(...)) of the float64 operation on exactly converted operands is that, by IEEE 754."""
    out = [0] * 8
    lo, hi = Fraction(float(min_depth)), Fraction(float(max_depth))
    for z, y in zip(z32.reshape(-1), y32.reshape(-1)):
        if np.isnan(y) or np.isnan(z) or not lo < Fraction(float(y)) < hi:
            continue
        y, z = float(y), min(max(float(z), 0.0), Z_TOP)
        e = abs(z - y)
        r = e / y
        t = max(z / y, y / z) if z != 0 else float("inf")
        out[0] += 1
        out[1] += rint_fraction(Fraction(e) * 2 ** 20)
        out[2] += rint_fraction(Fraction(e * e) * 2 ** 20)
        out[3] += rint_fraction(Fraction(r) * 2 ** 20)
        for k, th in enumerate(THRESHOLDS):
            out[4 + k] += 1 if t < th else 0
    return tuple(out)


# ------------------------------------------------------------------------------------------------ labels
def confusion(pred, gt, classes=19):
    """(H, W) int64 pair -> ((classes, classes) int64 [gt][pred], bad)."""
    pred, gt = pred.reshape(-1), gt.reshape(-1)
    keep = (gt >= 0) & (gt < classes)
    pred, gt = pred[keep], gt[keep]
    good = (pred >= 0) & (pred < classes)
    m = np.zeros((classes, classes), dtype=np.int64)
    np.add.at(m, (gt[good], pred[good]), 1)
    return m, int((~good).sum())


def segmentation_scores(pred, gt, classes=19):
    """(F, H, W) int64 stacks -> {"confusion", "bad", "iou", "miou", "pixel_acc"} as mudg_amd.metrics forms them."""
    pairs = [confusion(pred[f], gt[f], classes) for f in range(pred.shape[0])]
    m, bad = np.stack([p[0] for p in pairs]), np.array([p[1] for p in pairs], dtype=np.int64)
    c = m.astype(D)
    diag = np.diagonal(c, axis1=1, axis2=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = diag / (c.sum(2) + c.sum(1) - diag)
        defined = ~np.isnan(iou)
        miou = np.where(defined, iou, 0.0).sum(1) / defined.sum(1).astype(D)
        acc = diag.sum(1) / (c.sum((1, 2)) + bad.astype(D))
    return {"confusion": m, "bad": bad, "iou": iou, "miou": miou, "pixel_acc": acc}
