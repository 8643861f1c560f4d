"""The Gaussian splat rule of DESIGN.md §23 on the CPU, written from the rule and not from the kernels.

`project`, `bin_entries`, `blend` and `render` are the definition: numpy fp32, one rounded operation per numpy call in the order the rule
writes them, vectorised over the Gaussians (project) or over a tile's pixels (blend) with a Python loop over the tile's entries.  min and
max are np.fmin / np.fmax (the operand that is a number), as fminf / fmaxf are.  `textbook_render` is a second, plain float64 renderer of
one view (np.exp, the same thresholds, one global depth order): what the fp32 rule is an approximation of, with a mask of the pixels at
which a float64 value comes close enough to a threshold for fp32 to decide otherwise.  The product never imports this module."""
import numpy as np

F, D = np.float32, np.float64
TILE = 16
MAX_RADIUS = F(4096.0)
MIN_ALPHA = F(1.0) / F(255.0)
MAX_ALPHA = F(0.99)
MIN_POWER = F(-5.55)
MIN_T = F(1e-4)
BLUR = F(0.3)
LOG2E = F(1.44269504)
EXP_COEFFICIENTS = tuple(F(float.fromhex(h)) for h in ("0x1.f06faep-10", "0x1.25429cp-7", "0x1.c99b9ep-5", "0x1.ebcf7ap-3", "0x1.62e526p-1", "0x1.0p+0"))
ZNEAR, ZFAR = 0.2, 200.0


def tiles(hw):
    return (hw[1] + TILE - 1) // TILE, (hw[0] + TILE - 1) // TILE


def exp_rule(p):
    """E(p) for fp32 p in [-5.6, 0]."""
    p = np.asarray(p, dtype=F)
    t = p * LOG2E
    n = np.floor(t)
    f = t - n
    r = np.full_like(f, EXP_COEFFICIENTS[0])
    for c in EXP_COEFFICIENTS[1:]:
        r = r * f
        r = r + c
    with np.errstate(invalid="ignore"):
        return np.ldexp(r, n.astype(np.int32))


def unpack(points):
    """Packed (n, 4) int32 points -> xyz (n, 3) fp32 and the colour words (n,) uint32."""
    points = np.ascontiguousarray(points, dtype=np.int32)
    return points[:, :3].copy().view(F), points[:, 3].astype(np.uint32) & np.uint32(0xffffff)


def project(xyz, cov, opacity, ids, mats, cam, hw, znear=ZNEAR, zfar=ZFAR):
    """xyz (n, 3), cov (n, 6), opacity (n,) fp32, ids (n,) or None, mats (V, nmat, 12) fp32, cam (fx, fy, cx, cy).  Returns uv (V, n, 2),
    conic (V, n, 4), depth (V, n) fp32, rect (V, n, 4), count (V, n) int32; zero where dropped."""
    xyz, cov, opacity, mats = (np.asarray(a, dtype=F) for a in (xyz, cov, opacity, mats))
    fx, fy, cx, cy = (F(c) for c in cam)
    znear, zfar = F(znear), F(zfar)
    H, W = hw
    TX, TY = tiles(hw)
    V, nmat = mats.shape[:2]
    n = len(xyz)
    which = np.zeros(n, dtype=np.int64) if ids is None else np.clip(np.asarray(ids, dtype=np.int64), 0, nmat - 1)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    s = {(0, 0): cov[:, 0], (0, 1): cov[:, 1], (0, 2): cov[:, 2], (1, 1): cov[:, 3], (1, 2): cov[:, 4], (2, 2): cov[:, 5]}
    S = lambda r, k: s[(min(r, k), max(r, k))]
    out = {"uv": np.zeros((V, n, 2), F), "conic": np.zeros((V, n, 4), F), "depth": np.zeros((V, n), F), "rect": np.zeros((V, n, 4), np.int32),
           "count": np.zeros((V, n), np.int32)}
    limx = F(1.3) * (F(0.5) * F(W) / fx)
    limy = F(1.3) * (F(0.5) * F(H) / fy)
    with np.errstate(all="ignore"):
        for view in range(V):
            m = mats[view][which]                                                  # (n, 12)
            row = lambda r: ((m[:, 4 * r] * x + m[:, 4 * r + 1] * y) + m[:, 4 * r + 2] * z) + m[:, 4 * r + 3]
            xc, yc, zc = row(0), row(1), row(2)
            keep = (zc > znear) & (zc < zfar)
            qx, qy = xc / zc, yc / zc
            u, v = fx * qx + cx, fy * qy + cy
            tx = np.fmin(limx, np.fmax(-limx, qx)) * zc
            ty = np.fmin(limy, np.fmax(-limy, qy)) * zc
            zz = zc * zc
            j00, j02 = fx / zc, -((fx * tx) / zz)
            j11, j12 = fy / zc, -((fy * ty) / zz)
            T0 = [j00 * m[:, k] + j02 * m[:, 8 + k] for k in range(3)]
            T1 = [j11 * m[:, 4 + k] + j12 * m[:, 8 + k] for k in range(3)]
            V0 = [(T0[0] * S(0, k) + T0[1] * S(1, k)) + T0[2] * S(2, k) for k in range(3)]
            V1 = [(T1[0] * S(0, k) + T1[1] * S(1, k)) + T1[2] * S(2, k) for k in range(3)]
            a = ((V0[0] * T0[0] + V0[1] * T0[1]) + V0[2] * T0[2]) + BLUR
            b = (V0[0] * T1[0] + V0[1] * T1[1]) + V0[2] * T1[2]
            c = ((V1[0] * T1[0] + V1[1] * T1[1]) + V1[2] * T1[2]) + BLUR
            det = a * c - b * b
            keep &= (det > 0) & np.isfinite(det)
            A, B, C = c / det, -(b / det), a / det
            mid = F(0.5) * (a + c)
            lam = mid + np.sqrt(np.fmax(F(0.1), mid * mid - det))
            rad = np.ceil(F(3.0) * np.sqrt(lam))
            keep &= np.isfinite(rad) & (rad <= MAX_RADIUS)
            keep &= np.isfinite(opacity) & ~(opacity < MIN_ALPHA)
            clamp = lambda t, hi: np.fmin(np.fmax(t, F(0.0)), F(hi))
            x0 = clamp(np.floor((u - rad) / F(16.0)), TX)
            x1 = clamp(np.floor((u + rad) / F(16.0)) + F(1.0), TX)
            y0 = clamp(np.floor((v - rad) / F(16.0)), TY)
            y1 = clamp(np.floor((v + rad) / F(16.0)) + F(1.0), TY)
            rect = np.stack([np.where(keep, t, F(0.0)).astype(np.int32) for t in (x0, x1, y0, y1)], axis=1)
            count = (rect[:, 1] - rect[:, 0]) * (rect[:, 3] - rect[:, 2])
            keep &= count > 0
            out["uv"][view] = np.where(keep[:, None], np.stack([u, v], axis=1), F(0.0))
            out["conic"][view] = np.where(keep[:, None], np.stack([A, B, C, opacity], axis=1), F(0.0))
            out["depth"][view] = np.where(keep, zc, F(0.0))
            out["rect"][view] = np.where(keep[:, None], rect, 0)
            out["count"][view] = np.where(keep, count, 0)
    return out


def bin_entries(proj, hw):
    """The entries of every (view, Gaussian) in index order, sorted stably by (view NT + tile) << 32 | bits(zc): sorted keys (E,) int64,
    sorted values (E,) int32 and ranges (V NT, 2) int32."""
    TX, TY = tiles(hw)
    NT = TX * TY
    V, n = proj["count"].shape
    bits = proj["depth"].view(np.uint32).astype(np.int64)
    keys, values = [], []
    for view in range(V):
        for g in np.nonzero(proj["count"][view])[0]:
            x0, x1, y0, y1 = (int(t) for t in proj["rect"][view, g])
            for ty in range(y0, y1):
                for tx in range(x0, x1):
                    keys.append(((view * NT + ty * TX + tx) << 32) | int(bits[view, g]))
                    values.append(g)
    keys, values = np.array(keys, dtype=np.int64), np.array(values, dtype=np.int32)
    order = np.argsort(keys, kind="stable")
    keys, values = keys[order], values[order]
    ranges = np.zeros((V * NT, 2), dtype=np.int32)
    tile = keys >> 32
    for e in range(len(keys)):
        if e == 0 or tile[e - 1] != tile[e]:
            ranges[tile[e], 0] = e
        if e == len(keys) - 1 or tile[e + 1] != tile[e]:
            ranges[tile[e], 1] = e + 1
    return keys, values, ranges


def blend(proj, words, values, ranges, hw):
    """rgb (V, 3, H, W), depth (V, H, W), alpha (V, H, W) fp32, and per tile the entries looked at before every pixel was done."""
    H, W = hw
    TX, TY = tiles(hw)
    NT = TX * TY
    V = proj["count"].shape[0]
    rgb, depth, alpha = np.zeros((V, 3, H, W), F), np.zeros((V, H, W), F), np.zeros((V, H, W), F)
    looked = np.zeros(V * NT, dtype=np.int64)
    with np.errstate(all="ignore"):
        for t in range(V * NT):
            view, tile = divmod(t, NT)
            j0, i0 = (tile // TX) * TILE, (tile % TX) * TILE
            jj, ii = np.meshgrid(np.arange(j0, min(j0 + TILE, H)), np.arange(i0, min(i0 + TILE, W)), indexing="ij")
            px, py = ii.astype(F) + F(0.5), jj.astype(F) + F(0.5)
            T = np.ones(px.shape, F)
            C = [np.zeros(px.shape, F) for _ in range(3)]
            Dd = np.zeros(px.shape, F)
            done = np.zeros(px.shape, bool)
            for e in range(ranges[t, 0], ranges[t, 1]):
                if done.all():
                    break
                looked[t] += 1
                g = values[e]
                u, v = proj["uv"][view, g]
                A, B, Cc, op = proj["conic"][view, g]
                zc = proj["depth"][view, g]
                dx, dy = u - px, v - py
                q = (A * dx) * dx + (Cc * dy) * dy
                p = (F(-0.5) * q) - (B * dx) * dy
                skip = (p > 0) | (p < MIN_POWER)
                al = np.fmin(MAX_ALPHA, op * exp_rule(p))
                skip |= al < MIN_ALPHA
                Tn = T * (F(1.0) - al)
                live = ~done & ~skip
                ends = live & (Tn < MIN_T)
                done |= ends
                add = live & ~ends
                w = al * T
                for k in range(3):
                    byte = F((int(words[g]) >> (8 * k)) & 0xff)
                    C[k] = np.where(add, C[k] + byte * w, C[k])
                Dd = np.where(add, Dd + zc * w, Dd)
                T = np.where(add, Tn, T)
            for k in range(3):
                rgb[view, k, jj, ii] = C[k] / F(255.0)
            depth[view, jj, ii] = Dd
            alpha[view, jj, ii] = F(1.0) - T
    return rgb, depth, alpha, looked


def render(points, cov, opacity, ids, mats, cam, hw, znear=ZNEAR, zfar=ZFAR):
    """The whole rule for packed points: a dict with the images and every intermediate."""
    xyz, words = unpack(points)
    proj = project(xyz, cov, opacity, ids, mats, cam, hw, znear, zfar)
    out = dict(proj, entries=int(proj["count"].astype(np.int64).sum()))
    V = proj["count"].shape[0]
    TX, TY = tiles(hw)
    if out["entries"] == 0:
        out.update(rgb=np.zeros((V, 3) + tuple(hw), F), depth_image=np.zeros((V,) + tuple(hw), F), alpha=np.zeros((V,) + tuple(hw), F),
                   values=np.zeros(0, np.int32), ranges=np.zeros((V * TX * TY, 2), np.int32), longest_tile=0)
        return out
    keys, values, ranges = bin_entries(proj, hw)
    rgb, depth, alpha, looked = blend(proj, words, values, ranges, hw)
    out.update(rgb=rgb, depth_image=depth, alpha=alpha, keys=keys, values=values, ranges=ranges, looked=looked,
               longest_tile=int((ranges[:, 1] - ranges[:, 0]).max()))
    return out


def rgb_u8(rgb):
    """floor(rgb 255 + 0.5) clamped, fp32: (..., 3, H, W) -> (..., H, W, 3) uint8."""
    v = np.clip(np.floor(np.asarray(rgb, dtype=F) * F(255.0) + F(0.5)), 0, 255).astype(np.uint8)
    return np.moveaxis(v, -3, -1)


def pack(xyz, rgb):
    """(n, 3) fp32 and (n, 3) uint8 -> packed (n, 4) int32 points."""
    rgb = np.asarray(rgb).astype(np.int32)
    word = rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)
    return np.concatenate([np.ascontiguousarray(xyz, dtype=F).view(np.int32), word[:, None]], axis=1)


def isotropic(scale, n):
    s = np.broadcast_to(np.asarray(scale, dtype=F), (n,))
    cov = np.zeros((n, 6), F)
    cov[:, 0] = cov[:, 3] = cov[:, 5] = s * s
    return cov


# ------------------------------------------------------------------------------------------------ the float64 textbook
def textbook_render(xyz, rgb, cov, opacity, mat, cam, hw, znear=ZNEAR, zfar=ZFAR, margins=(1e-5, 1e-5, 1e-6)):
    """One view in float64, as a textbook states it: EWA projection, 3-sigma tile rectangles, one depth order, np.exp.  Returns rgb
    (3, H, W), alpha (H, W) and `near` (H, W): the pixels at which some entry's p, alpha or Tn lies within margins of its threshold."""
    xyz, cov, opacity = (np.asarray(a, dtype=F).astype(D) for a in (xyz, cov, opacity))
    M = np.asarray(mat, dtype=F).astype(D).reshape(3, 4)
    fx, fy, cx, cy = (float(F(c)) for c in cam)
    H, W = hw
    TX, TY = tiles(hw)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    px, py = ii + 0.5, jj + 0.5
    T, near, done = np.ones((H, W)), np.zeros((H, W), bool), np.zeros((H, W), bool)
    colour, items = np.zeros((3, H, W)), []
    min_alpha, min_power, min_t = float(MIN_ALPHA), float(MIN_POWER), float(MIN_T)
    for g in range(len(xyz)):
        cam_p = M[:, :3] @ xyz[g] + M[:, 3]
        zc = cam_p[2]
        if not (float(F(znear)) < zc < float(F(zfar))) or not opacity[g] >= min_alpha:
            continue
        limx, limy = 1.3 * 0.5 * W / fx, 1.3 * 0.5 * H / fy
        tx, ty = np.clip(cam_p[0] / zc, -limx, limx) * zc, np.clip(cam_p[1] / zc, -limy, limy) * zc
        J = np.array([[fx / zc, 0.0, -fx * tx / zc ** 2], [0.0, fy / zc, -fy * ty / zc ** 2]])
        s = cov[g]
        Sigma = np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]])
        Tm = J @ M[:, :3]
        c2 = Tm @ Sigma @ Tm.T + 0.3 * np.eye(2)
        det = np.linalg.det(c2)
        if not det > 0:
            continue
        conic = np.linalg.inv(c2)
        mid = 0.5 * (c2[0, 0] + c2[1, 1])
        rad = np.ceil(3.0 * np.sqrt(mid + np.sqrt(max(0.1, mid * mid - det))))
        if not rad <= 4096:
            continue
        u, v = fx * cam_p[0] / zc + cx, fy * cam_p[1] / zc + cy
        x0, x1 = int(np.clip(np.floor((u - rad) / 16), 0, TX)), int(np.clip(np.floor((u + rad) / 16) + 1, 0, TX))
        y0, y1 = int(np.clip(np.floor((v - rad) / 16), 0, TY)), int(np.clip(np.floor((v + rad) / 16) + 1, 0, TY))
        if (x1 - x0) * (y1 - y0) > 0:
            items.append((zc, g, u, v, conic, (slice(16 * y0, min(16 * y1, H)), slice(16 * x0, min(16 * x1, W)))))
    for zc, g, u, v, conic, where in sorted(items, key=lambda t: (t[0], t[1])):
        dx, dy = u - px[where], v - py[where]
        p = -0.5 * (conic[0, 0] * dx * dx + conic[1, 1] * dy * dy) - conic[0, 1] * dx * dy
        al = np.minimum(0.99, opacity[g] * np.exp(p))
        Tn = T[where] * (1.0 - al)
        alive = ~done[where]
        near[where] |= alive & ((np.abs(p) < margins[0]) | (np.abs(p - min_power) < margins[0]))
        inside = (p <= 0) & (p >= min_power)
        near[where] |= alive & inside & (np.abs(al - min_alpha) < margins[1])
        live = alive & inside & (al >= min_alpha)
        near[where] |= live & (np.abs(Tn - min_t) < margins[2])
        ends = live & (Tn < min_t)
        add = live & ~ends
        w = np.where(add, al * T[where], 0.0)
        for k in range(3):
            colour[k][where] += float(rgb[g][k]) * w
        T[where] = np.where(add, Tn, T[where])
        done[where] |= ends
    return colour / 255.0, 1.0 - T, near


# ------------------------------------------------------------------------------------------------ shared cases
FOCAL = 128.0                                       # with z = FOCAL and cx = cy = 0 a point (i + 0.5, j + 0.5, FOCAL) lands exactly on pixel centre (i, j)
FLAT = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], dtype=F)     # the identity as a one-matrix table
FLAT_CAM = (FOCAL, FOCAL, 0.0, 0.0)


def flat_case(centres, scale, opacity=1.0, z=None, seed=0):
    """Gaussians at pixel positions `centres` (n, 2) in front of the flat camera (FLAT[None], FLAT_CAM): packed points, cov, opacity."""
    centres = np.asarray(centres, dtype=F).reshape(-1, 2)
    n = len(centres)
    depth = np.full(n, FOCAL, F) if z is None else np.asarray(z, dtype=F)
    xyz = np.stack([centres[:, 0] * depth / F(FOCAL), centres[:, 1] * depth / F(FOCAL), depth], axis=1).astype(F)
    rgb = np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)
    return pack(xyz, rgb), isotropic(scale, n), np.broadcast_to(np.asarray(opacity, dtype=F), (n,)).copy()


def seeded_scene(n=400, hw=(40, 56), seed=7):
    """About n isotropic Gaussians in front of a pinhole camera whose image is hw: xyz, rgb, cov, opacity, the matrix table and the camera."""
    rng = np.random.default_rng(seed)
    H, W = hw
    cam = (48.0, 48.0, W / 2.0, H / 2.0)
    z = rng.uniform(2.0, 20.0, n)
    xyz = np.stack([rng.uniform(-0.7, 0.7, n) * z * W / 96.0 * 2, rng.uniform(-0.7, 0.7, n) * z * H / 96.0 * 2, z], axis=1).astype(F)
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    cov = isotropic(rng.uniform(0.05, 0.4, n), n)
    opacity = rng.uniform(0.05, 1.0, n).astype(F)
    a = 0.1
    mat = np.array([[np.cos(a), 0, np.sin(a), 0.2, 0, 1, 0, -0.1, -np.sin(a), 0, np.cos(a), 0.5]], dtype=F)
    return xyz, rgb, cov, opacity, mat[None], cam
