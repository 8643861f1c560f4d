"""The image loss of the Gaussian fit off the GPU, twice.

`forward`, `finish` and `backward` are the rule in numpy fp32: the operations of csrc/gaussians_loss.hip one by one, in its order — the
horizontal pass and then the vertical pass with the taps added in ascending index from +0.0 over a zero-padded image, the per-pixel
formula in the kernel's association, the xor butterfly over a tile's 256 lanes, the four waves as ((w0 + w1) + w2) + w3, the partials
added by 256 lanes in strides in fp64 and combined the same way.  Every array it returns is bit-equal to what the kernels store.

`textbook` is the same loss in float64 torch: F.conv2d(padding=5, groups=3) with the window in float64, .abs().mean() and the masked
depth mean; gradients come from autograd.  `textbook_fit` is §24's float64 fit with this loss.  The product never imports this file."""
import numpy as np
import torch
import torch.nn.functional as TF

import gaussians_bwd_reference as gb

F, D = np.float32, np.float64
TILE, TAPS, HALO = 16, 11, 5
TAPS_INT = (67, 498, 2359, 7167, 13960, 17434, 13960, 7167, 2359, 498, 67)          # ops.SSIM_WINDOW (the CPU test compares them)
WINDOW = (np.array(TAPS_INT, D) / 65536.0).astype(F)                                # exact: every tap has at most 15 significant bits
C1, C2 = F(0.0001), F(0.0009)
_LANES = np.arange(64)


def tiles(hw):
    return (hw[1] + TILE - 1) // TILE, (hw[0] + TILE - 1) // TILE


def window_pass(img, axis):
    """One pass of the window along `axis` of (..., H, W) fp32 with zero padding: taps in ascending index, from +0.0."""
    img = np.asarray(img, F)
    pad = [(0, 0)] * img.ndim
    pad[axis] = (HALO, HALO)
    p = np.pad(img, pad)
    n = img.shape[axis]
    acc = np.zeros(img.shape, F)
    for k in range(TAPS):
        acc = acc + WINDOW[k] * np.take(p, np.arange(k, k + n), axis=axis)
    return acc


def convolve(img):
    """w * img: the horizontal pass, then the vertical pass."""
    return window_pass(window_pass(img, -1), -2)


def _tile_lanes(img):
    """(..., H, W) -> (..., NT, 256): each 16 x 16 tile's lanes (row * 16 + column), +0.0 where the tile leaves the image."""
    h, w = img.shape[-2:]
    tx, ty = tiles((h, w))
    p = np.zeros(img.shape[:-2] + (ty * TILE, tx * TILE), img.dtype)
    p[..., :h, :w] = img
    p = p.reshape(img.shape[:-2] + (ty, TILE, tx, TILE))
    return np.moveaxis(p, -3, -2).reshape(img.shape[:-2] + (ty * tx, 256))


def reduce_lanes(r):
    """(..., 256) -> (...): the butterfly inside each wave, then ((w0 + w1) + w2) + w3."""
    v = r.reshape(r.shape[:-1] + (4, 64))
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[..., _LANES ^ s]
    return ((v[..., 0, 0] + v[..., 1, 0]) + v[..., 2, 0]) + v[..., 3, 0]


def sgn(d):
    return ((d > 0).astype(F) - (d < 0).astype(F)).astype(F)


def forward(x, y, d=None, dt=None):
    """x, y (V, 3, H, W), d, dt (V, H, W) or None -> maps (V, 3, 3, H, W) fp32, partial (V, 3, NT, 4) fp32 whose fourth column holds the
    bits of an int32 count, and S (V, 3, H, W)."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    two = F(2.0)
    a, m = convolve(x), convolve(y)
    b, n, c = convolve(x * x), convolve(y * y), convolve(x * y)
    aa, mm, am = a * a, m * m, a * m
    s1, s2, s12 = b - aa, n - mm, c - am
    A1, A2 = two * am + C1, two * s12 + C2
    B1, B2 = (aa + mm) + C1, (s1 + s2) + C2
    num, den = A1 * A2, B1 * B2
    with np.errstate(all="ignore"):
        S = num / den
        Dm = ((two * m) * (A2 - A1) + ((two * a) * S) * (B1 - B2)) / den
        Ds1 = -(S / B2)
        Ds12 = (two * A1) / den
    maps = np.stack([Dm, Ds1, Ds12], axis=2).astype(F)
    V, _, H, W = x.shape
    tx, ty = tiles((H, W))
    partial = np.zeros((V, 3, tx * ty, 4), F)
    partial[..., 0] = reduce_lanes(_tile_lanes(np.abs(x - y)))
    partial[..., 1] = reduce_lanes(_tile_lanes(S.astype(F)))
    if d is not None:
        d, dt = np.asarray(d, F), np.asarray(dt, F)
        seen = dt > 0
        partial[:, 0, :, 2] = reduce_lanes(_tile_lanes(np.where(seen, np.abs(d - dt), F(0.0)).astype(F)))
        count = _tile_lanes(seen.astype(np.int32)).sum(axis=-1).astype(np.int32)
        partial[:, 0, :, 3] = count.view(F)
    assert S.dtype == F and maps.dtype == F
    return maps, partial, S, (num, den)


def finish(partial, hw, ssim_weight, depth_weight):
    """partial (V, 3, NT, 4) -> totals (8,) fp32: loss, mean |x - y|, mean S, depth mean, float(max(count, 1)), count (int32 bits), 0, 0."""
    rows = partial.reshape(-1, 4)
    P = rows.shape[0]
    N = D(3.0) * D(partial.shape[0]) * D(hw[0]) * D(hw[1])
    lanes = np.zeros((256, 3), D)
    counts = np.zeros(256, np.int64)
    for p in range(0, P, 256):                                              # lane l adds partials l, l + 256, ... in ascending order
        chunk = rows[p:p + 256]
        lanes[:len(chunk)] = lanes[:len(chunk)] + chunk[:, :3].astype(D)
        counts[:len(chunk)] += chunk[:, 3].copy().view(np.int32)
    L, S, Dsum = (reduce_lanes(lanes[:, k]) for k in range(3))
    count = int(counts.sum())
    seen = max(count, 1)
    lam, dw, one = F(ssim_weight), F(depth_weight), F(1.0)
    l1_mean, s_mean, d_mean = F(L / N), F(S / N), F(Dsum / D(seen))
    totals = np.zeros(8, F)
    with np.errstate(all="ignore"):
        totals[0] = ((one - lam) * l1_mean + lam * (one - s_mean)) + dw * d_mean
    totals[1], totals[2], totals[3] = l1_mean, s_mean, d_mean
    totals[4] = F(np.int64(seen))
    totals[5:6] = np.array([min(count, 2 ** 31 - 1)], np.int32).view(F)
    return totals


def backward(x, y, maps, totals, up, ssim_weight, depth_weight, d=None, dt=None):
    """d_rgb (V, 3, H, W) and d_depth (V, H, W) or None, fp32."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    lam, dw, up, one, two = F(ssim_weight), F(depth_weight), F(up), F(1.0), F(2.0)
    V, _, H, W = x.shape
    count = F(D(3.0) * D(V) * D(H) * D(W))
    with np.errstate(all="ignore"):
        g0, g1, g2 = convolve(maps[:, :, 0]), convolve(maps[:, :, 1]), convolve(maps[:, :, 2])
        g = (g0 + (two * x) * g1) + y * g2
        kl, ks = (one - lam) / count, lam / count
        d_rgb = up * (kl * sgn(x - y) - ks * g)
    d_depth = None
    if d is not None:
        d, dt = np.asarray(d, F), np.asarray(dt, F)
        kd = dw / totals[4]
        d_depth = (up * (kd * np.where(dt > 0, sgn(d - dt), F(0.0)).astype(F))).astype(F)
    assert d_rgb.dtype == F
    return d_rgb, d_depth


def loss_and_gradients(x, y, d=None, dt=None, *, ssim_weight, depth_weight=0.0, up=1.0):
    """Everything the three entry points store, as a dict of arrays."""
    maps, partial, S, _ = forward(x, y, d, dt)
    totals = finish(partial, x.shape[2:], ssim_weight, depth_weight)
    d_rgb, d_depth = backward(x, y, maps, totals, up, ssim_weight, depth_weight, d, dt)
    return dict(maps=maps, partial=partial, totals=totals, d_rgb=d_rgb, d_depth=d_depth, S=S)


# ------------------------------------------------------------------------------------------------ the textbook, in float64
def textbook_ssim_map(x, y):
    """x, y (V, 3, H, W) torch tensors of one dtype -> S (V, 3, H, W): grouped conv2d with the 11 x 11 window and zero padding."""
    w1 = torch.tensor(np.array(TAPS_INT, D) / 65536.0, dtype=x.dtype)
    w2 = torch.outer(w1, w1)[None, None].repeat(3, 1, 1, 1)
    conv = lambda t: TF.conv2d(t, w2, padding=HALO, groups=3)
    a, m = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - a * a, conv(y * y) - m * m, conv(x * y) - a * m
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * a * m + c1) * (2 * s12 + c2)) / ((a * a + m * m + c1) * (s1 + s2 + c2))


def textbook(x, y, d=None, dt=None, *, ssim_weight, depth_weight=0.0):
    """loss, (mean |x - y|, mean S, depth mean) in the tensors' precision."""
    l1 = (x - y).abs().mean()
    s = textbook_ssim_map(x, y).mean()
    depth = torch.zeros((), dtype=x.dtype)
    if d is not None:
        seen = dt > 0
        depth = ((d - dt).abs() * seen).sum() / seen.sum().clamp(min=1)
    return (1 - ssim_weight) * l1 + ssim_weight * (1 - s) + depth_weight * depth, (l1, s, depth)


def textbook_fit(start, views, cam, targets, hw, rates, iters, betas, eps, ssim_weight):
    """gb.textbook_fit with the textbook loss: torch.optim.Adam over the float64 renderer, the loss of every step."""
    params = {k: torch.tensor(v.astype(D), requires_grad=True) for k, v in start.items()}
    opt = torch.optim.Adam([{"params": [p], "lr": float(rates[k])} for k, p in params.items()], betas=betas, eps=eps)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        rgb = gb.textbook(params["xyz"], params["colour"], gb.covariance64(params["log_scale"], params["quat"]),
                          torch.sigmoid(params["opacity_logit"]), views, cam, hw)[0]
        loss = textbook(rgb, targets, ssim_weight=ssim_weight)[0]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def impulse_case(seed=8, at=(15, 15), hw=(33, 33), channel=1):
    """Seeded x, y (1, 3, H, W) in [0, 1] and the maps of gl.forward with everything but pixel `at` of `channel` zeroed: their backward at
    ssim_weight 1 is -1 / N times the gradient of that one pixel's S, which lives on the 11 x 11 pixels around it, in four tiles."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (1, 3) + tuple(hw)).astype(F)
    y = rng.uniform(0, 1, (1, 3) + tuple(hw)).astype(F)
    maps = forward(x, y)[0]
    impulse = np.zeros_like(maps)
    impulse[0, channel, :, at[0], at[1]] = maps[0, channel, :, at[0], at[1]]
    return x, y, maps, impulse


def seeded_images(V, hw, seed=11):
    """x uniform in [-0.5, 1.5], y in [0, 1], depth in [1, 50], a third of dt zero: fp32."""
    rng = np.random.default_rng(seed)
    H, W = hw
    x = rng.uniform(-0.5, 1.5, (V, 3, H, W)).astype(F)
    y = rng.uniform(0.0, 1.0, (V, 3, H, W)).astype(F)
    d = rng.uniform(1.0, 50.0, (V, H, W)).astype(F)
    dt = rng.uniform(1.0, 50.0, (V, H, W)).astype(F)
    dt[rng.uniform(size=dt.shape) < 1.0 / 3.0] = 0
    return x, y, d, dt
