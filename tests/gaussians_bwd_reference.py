"""The backward rule of DESIGN.md §24 on the CPU, written from the rule and not from the kernels, and what it approximates.

`blend_train`, `blend_bwd`, `project_bwd` and `render_backward` are the definition: numpy fp32, one rounded operation per numpy call in
the order the rule writes them, vectorised over a tile's 256 lanes (blend) or over the Gaussians (projection), with the reduction order of
the rule: an xor butterfly over 1, 2, 4, 8, 16, 32 inside each wave of 64 lanes, then ((w0 + w1) + w2) + w3.  `textbook` is a float64
differentiable renderer in torch (torch.exp, one depth order per view, transmittance by a cumulative product, §23's thresholds as
constant masks, the cap passing no gradient): autograd of it is the truth the fp32 rule is measured against.  The product never imports
this module."""
import numpy as np
import torch

import gaussians_reference as gr

F = np.float32
SUMS = 10
BATCH = 256
_LANES = np.arange(64)


# ------------------------------------------------------------------------------------------------ entries and their order
def bin_with_order(proj, hw):
    """gr.bin_entries that also returns `order` (E,) int64: sorted entry e was unsorted entry order[e], the unsorted entries lying at
    offsets[view, g] + k in (view, Gaussian, tile) order; and offsets (V, n) int64."""
    TX, TY = gr.tiles(hw)
    NT = TX * TY
    V, n = proj["count"].shape
    bits = proj["depth"].view(np.uint32).astype(np.int64)
    ends = np.cumsum(proj["count"].reshape(-1).astype(np.int64))
    offsets = (ends - proj["count"].reshape(-1)).reshape(V, n)
    keys, values = [], []
    for view in range(V):
        for g in np.nonzero(proj["count"][view])[0]:
            x0, x1, y0, y1 = (int(t) for t in proj["rect"][view, g])
            assert len(keys) == offsets[view, g]
            for ty in range(y0, y1):
                for tx in range(x0, x1):
                    keys.append(((view * NT + ty * TX + tx) << 32) | int(bits[view, g]))
                    values.append(g)
    keys, values = np.array(keys, dtype=np.int64), np.array(values, dtype=np.int32)
    order = np.argsort(keys, kind="stable").astype(np.int64)
    keys, values = keys[order], values[order]
    ranges = np.zeros((V * NT, 2), dtype=np.int32)
    tile = keys >> 32
    for e in range(len(keys)):
        if e == 0 or tile[e - 1] != tile[e]:
            ranges[tile[e], 0] = e
        if e == len(keys) - 1 or tile[e + 1] != tile[e]:
            ranges[tile[e], 1] = e + 1
    return keys, values, order, ranges, offsets


def _lanes(tile, TX, H, W):
    """The 256 lanes of a tile: pixel centres and which of them lie inside the image."""
    lane = np.arange(256)
    i, j = (tile % TX) * gr.TILE + (lane & 15), (tile // TX) * gr.TILE + (lane >> 4)
    return i, j, (i < W) & (j < H), i.astype(F) + F(0.5), j.astype(F) + F(0.5)


def _entry(proj, colour, view, g, n):
    if g < 0 or g >= n:                                                    # a sorted value outside the cloud: opacity 0
        return (F(0),) * 10
    u, v = proj["uv"][view, g]
    A, B, C, op = proj["conic"][view, g]
    return u, v, A, B, C, op, proj["depth"][view, g], colour[g, 0], colour[g, 1], colour[g, 2]


def _step(ent, px, py, T):
    """The forward's step of one entry at every lane: dx, dy, the exponential, the uncapped and capped alpha, Tn, and who skips."""
    u, v, A, B, C, op = ent[:6]
    dx, dy = u - px, v - py
    q = (A * dx) * dx + (C * dy) * dy
    p = (F(-0.5) * q) - (B * dx) * dy
    skip = (p > 0) | (p < gr.MIN_POWER)
    ge = gr.exp_rule(p)
    raw = op * ge
    al = np.fmin(gr.MAX_ALPHA, raw)
    skip |= al < gr.MIN_ALPHA
    om = F(1.0) - al
    return dx, dy, ge, raw, al, om, T * om, skip


# ------------------------------------------------------------------------------------------------ the training forward
def blend_train(proj, colour, values, ranges, hw):
    """gr.blend with fp32 colours (n, 3) in byte units: rgb, depth, alpha and state (V, 5, H, W) = (C0, C1, C2, D, T)."""
    H, W = hw
    TX, TY = gr.tiles(hw)
    NT = TX * TY
    V, n = proj["count"].shape
    colour = np.asarray(colour, dtype=F)
    state = np.zeros((V, 5, H, W), F)
    state[:, 4] = 1
    with np.errstate(all="ignore"):
        for t in range(V * NT):
            view, tile = divmod(t, NT)
            i, j, inside, px, py = _lanes(tile, TX, H, W)
            T, acc, done = np.ones(256, F), [np.zeros(256, F) for _ in range(4)], ~inside
            for e in range(ranges[t, 0], ranges[t, 1]):
                if done.all():
                    break
                ent = _entry(proj, colour, view, int(values[e]), n)
                _, _, _, _, al, _, Tn, skip = _step(ent, px, py, T)
                live = ~done & ~skip
                ends = live & (Tn < gr.MIN_T)
                done = done | ends
                add = live & ~ends
                w = al * T
                for k, c in enumerate((ent[7], ent[8], ent[9], ent[6])):
                    acc[k] = np.where(add, acc[k] + c * w, acc[k])
                T = np.where(add, Tn, T)
            for k in range(4):
                state[view, k, j[inside], i[inside]] = acc[k][inside]
            state[view, 4, j[inside], i[inside]] = T[inside]
    return state[:, :3] / F(255.0), state[:, 3].copy(), F(1.0) - state[:, 4], state


# ------------------------------------------------------------------------------------------------ the blend's backward
def reduce_tile(r):
    """(256, SUMS) fp32 -> (SUMS,): the butterfly inside each wave, then ((w0 + w1) + w2) + w3."""
    v = r.reshape(4, 64, SUMS)
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[:, _LANES ^ s, :]
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def blend_bwd(proj, colour, values, order, ranges, hw, state, d_rgb, d_depth, d_alpha, walked=None):
    """partial (E, SUMS) fp32 at the unsorted positions.  walked (V NT,) receives the entries each tile staged before it left."""
    H, W = hw
    TX, TY = gr.tiles(hw)
    NT = TX * TY
    V, n = proj["count"].shape
    E = len(values)
    colour, state = np.asarray(colour, dtype=F), np.asarray(state, dtype=F)
    d_rgb, d_depth, d_alpha = (np.asarray(a, dtype=F) for a in (d_rgb, d_depth, d_alpha))
    partial = np.zeros((E, SUMS), F)
    with np.errstate(all="ignore"):
        for t in range(V * NT):
            view, tile = divmod(t, NT)
            i, j, inside, px, py = _lanes(tile, TX, H, W)
            ii, jj = np.where(inside, i, 0), np.where(inside, j, 0)
            pick = lambda a: np.where(inside, a[jj, ii], F(0.0)).astype(F)
            gC = [pick(d_rgb[view, k]) / F(255.0) for k in range(3)]
            gD = pick(d_depth[view])
            S = [pick(state[view, k]) for k in range(4)]
            gAT = pick(d_alpha[view]) * pick(state[view, 4])
            T, acc, done = np.ones(256, F), [np.zeros(256, F) for _ in range(4)], ~inside
            start, end = int(ranges[t, 0]), int(ranges[t, 1])
            if start < 0 or end > E or start > end:
                start = end = 0
            staged = 0
            for base in range(start, end, BATCH):
                if done.all():
                    break
                m = min(BATCH, end - base)
                staged += m
                for e in range(base, base + m):
                    ent = _entry(proj, colour, view, int(values[e]), n)
                    u, v, A, B, C, op, zc, k0, k1, k2 = ent
                    dx, dy, ge, raw, al, om, Tn, skip = _step(ent, px, py, T)
                    live = ~done & ~skip
                    ends = live & (Tn < gr.MIN_T)
                    done = done | ends
                    add = live & ~ends
                    w = al * T
                    for k, c in enumerate((k0, k1, k2, zc)):
                        acc[k] = np.where(add, acc[k] + c * w, acc[k])
                    own = ((gC[0] * k0 + gC[1] * k1) + gC[2] * k2) + gD * zc
                    behind = ((gC[0] * (S[0] - acc[0]) + gC[1] * (S[1] - acc[1])) + gC[2] * (S[2] - acc[2])) + gD * (S[3] - acc[3])
                    dal = (T * own - behind / om) + gAT / om
                    dp = (dal * op) * ge
                    free = add & ~(raw > gr.MAX_ALPHA)
                    r = np.zeros((256, SUMS), F)
                    for k in range(3):
                        r[:, k] = np.where(add, gC[k] * w, F(0.0))
                    r[:, 3] = np.where(add, gD * w, F(0.0))
                    r[:, 4] = np.where(free, dal * ge, F(0.0))
                    r[:, 5] = np.where(free, dp * (F(-0.5) * (dx * dx)), F(0.0))
                    r[:, 6] = np.where(free, dp * -(dx * dy), F(0.0))
                    r[:, 7] = np.where(free, dp * (F(-0.5) * (dy * dy)), F(0.0))
                    r[:, 8] = np.where(free, dp * -(A * dx + B * dy), F(0.0))
                    r[:, 9] = np.where(free, dp * -(C * dy + B * dx), F(0.0))
                    T = np.where(add, Tn, T)
                    at = int(order[e])
                    if 0 <= at < E:
                        partial[at] = reduce_tile(r)
            if walked is not None:
                walked[t] = staged
    return partial


# ------------------------------------------------------------------------------------------------ the projection's backward
def project_bwd(xyz, cov, ids, mats, cam, hw, count, offsets, partial, znear=gr.ZNEAR, zfar=gr.ZFAR):
    """d_xyz (n, 3), d_cov (n, 6), d_opacity (n,), d_colour (n, 3) fp32: the views added in order."""
    xyz, cov, mats, partial = (np.asarray(a, dtype=F) for a in (xyz, cov, mats, partial))
    fx, fy, cx, cy = (F(c) for c in cam)
    znear, zfar = F(znear), F(zfar)
    H, W = hw
    V, nmat = mats.shape[:2]
    n, E = len(xyz), len(partial)
    which = np.zeros(n, dtype=np.int64) if ids is None else np.clip(np.asarray(ids, dtype=np.int64), 0, nmat - 1)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    s = {(0, 0): cov[:, 0], (0, 1): cov[:, 1], (0, 2): cov[:, 2], (1, 1): cov[:, 3], (1, 2): cov[:, 4], (2, 2): cov[:, 5]}
    S = lambda r, k: s[(min(r, k), max(r, k))]
    limx = F(1.3) * (F(0.5) * F(W) / fx)
    limy = F(1.3) * (F(0.5) * F(H) / fy)
    d_xyz, d_cov, d_op, d_col = np.zeros((n, 3), F), np.zeros((n, 6), F), np.zeros(n, F), np.zeros((n, 3), F)
    two = F(2.0)
    with np.errstate(all="ignore"):
        for view in range(V):
            m = mats[view][which]
            M = lambda k: m[:, k]
            row = lambda r: ((M(4 * r) * x + M(4 * r + 1) * y) + M(4 * r + 2) * z) + M(4 * r + 3)
            xc, yc, zc = row(0), row(1), row(2)
            cnt, off = count[view].astype(np.int64), np.asarray(offsets[view], dtype=np.int64)
            ok = (cnt > 0) & (off >= 0) & (off <= E - cnt) & (zc > znear) & (zc < zfar)
            acc = np.zeros((n, SUMS), F)
            for g in np.nonzero(ok)[0]:
                for k in range(cnt[g]):
                    acc[g] = acc[g] + partial[off[g] + k]
            qx, qy = xc / zc, yc / zc
            kx, ky = np.fmin(limx, np.fmax(-limx, qx)), np.fmin(limy, np.fmax(-limy, qy))
            tx, ty = kx * zc, ky * zc
            zz = zc * zc
            j00, j02 = fx / zc, -((fx * tx) / zz)
            j11, j12 = fy / zc, -((fy * ty) / zz)
            T0 = [j00 * M(k) + j02 * M(8 + k) for k in range(3)]
            T1 = [j11 * M(4 + k) + j12 * M(8 + k) for k in range(3)]
            V0 = [(T0[0] * S(0, k) + T0[1] * S(1, k)) + T0[2] * S(2, k) for k in range(3)]
            V1 = [(T1[0] * S(0, k) + T1[1] * S(1, k)) + T1[2] * S(2, k) for k in range(3)]
            a = ((V0[0] * T0[0] + V0[1] * T0[1]) + V0[2] * T0[2]) + gr.BLUR
            b = (V0[0] * T1[0] + V0[1] * T1[1]) + V0[2] * T1[2]
            c = ((V1[0] * T1[0] + V1[1] * T1[1]) + V1[2] * T1[2]) + gr.BLUR
            det = a * c - b * b
            A, B, C = c / det, -(b / det), a / det
            gA, hB, gC = acc[:, 5], F(0.5) * acc[:, 6], acc[:, 7]
            x00, x01 = gA * A + hB * B, gA * B + hB * C
            x10, x11 = hB * A + gC * B, hB * B + gC * C
            da = -(A * x00 + B * x10)
            db = F(-2.0) * (A * x01 + B * x11)
            dc = -(B * x01 + C * x11)
            da2, dc2 = two * da, two * dc
            e = 0
            for r in range(3):
                for k in range(r, 3):
                    if r == k:
                        g = (da * (T0[r] * T0[r]) + db * (T0[r] * T1[r])) + dc * (T1[r] * T1[r])
                    else:
                        g = (da2 * (T0[r] * T0[k]) + db * (T0[r] * T1[k] + T0[k] * T1[r])) + dc2 * (T1[r] * T1[k])
                    d_cov[:, e] = np.where(ok, d_cov[:, e] + g, d_cov[:, e])
                    e += 1
            dT0 = [da2 * V0[k] + db * V1[k] for k in range(3)]
            dT1 = [dc2 * V1[k] + db * V0[k] for k in range(3)]
            dj00 = (dT0[0] * M(0) + dT0[1] * M(1)) + dT0[2] * M(2)
            dj02 = (dT0[0] * M(8) + dT0[1] * M(9)) + dT0[2] * M(10)
            dj11 = (dT1[0] * M(4) + dT1[1] * M(5)) + dT1[2] * M(6)
            dj12 = (dT1[0] * M(8) + dT1[1] * M(9)) + dT1[2] * M(10)
            dtx, dty = -((dj02 * fx) / zz), -((dj12 * fy) / zz)
            dzz = -((dj02 * j02) / zz + (dj12 * j12) / zz)
            dzc = acc[:, 3]
            dzc = dzc - (dj00 * j00) / zc
            dzc = dzc - (dj11 * j11) / zc
            dzc = dzc + (two * zc) * dzz
            dzc = dzc + dtx * kx
            dzc = dzc + dty * ky
            dqx, dqy = acc[:, 8] * fx, acc[:, 9] * fy
            dqx = np.where(kx == qx, dqx + dtx * zc, dqx)
            dqy = np.where(ky == qy, dqy + dty * zc, dqy)
            dxc, dyc = dqx / zc, dqy / zc
            dzc = dzc - (dqx * qx) / zc
            dzc = dzc - (dqy * qy) / zc
            for k in range(3):
                g = (dxc * M(k) + dyc * M(4 + k)) + dzc * M(8 + k)
                d_xyz[:, k] = np.where(ok, d_xyz[:, k] + g, d_xyz[:, k])
                d_col[:, k] = np.where(ok, d_col[:, k] + acc[:, k], d_col[:, k])
            d_op = np.where(ok, d_op + acc[:, 4], d_op)
    return d_xyz, d_cov, d_op, d_col


def render_backward(xyz, colour, cov, opacity, ids, mats, cam, hw, d_rgb, d_depth, d_alpha, znear=gr.ZNEAR, zfar=gr.ZFAR):
    """The whole rule: forward with fp32 colours, then both backward halves.  A dict with the images, state, partial and the gradients."""
    xyz, colour, cov, opacity = (np.asarray(a, dtype=F) for a in (xyz, colour, cov, opacity))
    proj = gr.project(xyz, cov, opacity, ids, mats, cam, hw, znear, zfar)
    V, n = proj["count"].shape
    out = dict(proj, entries=int(proj["count"].astype(np.int64).sum()))
    if out["entries"] == 0:
        out.update(rgb=np.zeros((V, 3) + tuple(hw), F), depth_image=np.zeros((V,) + tuple(hw), F), alpha=np.zeros((V,) + tuple(hw), F),
                   d_xyz=np.zeros((n, 3), F), d_cov=np.zeros((n, 6), F), d_opacity=np.zeros(n, F), d_colour=np.zeros((n, 3), F))
        return out
    keys, values, order, ranges, offsets = bin_with_order(proj, hw)
    rgb, depth, alpha, state = blend_train(proj, colour, values, ranges, hw)
    walked = np.zeros(len(ranges), np.int64)
    partial = blend_bwd(proj, colour, values, order, ranges, hw, state, d_rgb, d_depth, d_alpha, walked)
    d_xyz, d_cov, d_op, d_col = project_bwd(xyz, cov, ids, mats, cam, hw, proj["count"], offsets, partial, znear, zfar)
    out.update(rgb=rgb, depth_image=depth, alpha=alpha, state=state, values=values, order=order, ranges=ranges, offsets=offsets,
               partial=partial, walked=walked, d_xyz=d_xyz, d_cov=d_cov, d_opacity=d_op, d_colour=d_col)
    return out


# ------------------------------------------------------------------------------------------------ the float64 textbook in torch
def textbook(xyz, colour, cov, opacity, mats, cam, hw, ids=None, znear=gr.ZNEAR, zfar=gr.ZFAR):
    """float64 torch tensors (xyz (n, 3), colour (n, 3) byte units, cov (n, 6), opacity (n,)), differentiable; mats (V, nmat, 12).  Returns
    rgb (V, 3, H, W), depth (V, H, W), alpha (V, H, W).  Which Gaussians are drawn, their tile rectangles, the skips, the stopping entry
    and whether the cap took effect are decided on detached values: constant masks."""
    D = torch.float64
    mats = torch.as_tensor(np.asarray(mats), dtype=D)
    V, nmat = mats.shape[:2]
    n = xyz.shape[0]
    fx, fy, cx, cy = (float(F(c)) for c in cam)
    znear, zfar = float(F(znear)), float(F(zfar))
    H, W = hw
    TX, TY = gr.tiles(hw)
    which = torch.zeros(n, dtype=torch.long) if ids is None else torch.as_tensor(np.asarray(ids)).long().clamp(0, nmat - 1)
    jj, ii = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    px, py = (ii + 0.5).to(D), (jj + 0.5).to(D)
    min_alpha, min_power, min_t, max_alpha = float(gr.MIN_ALPHA), float(gr.MIN_POWER), float(gr.MIN_T), float(gr.MAX_ALPHA)
    limx, limy = 1.3 * 0.5 * W / fx, 1.3 * 0.5 * H / fy
    images = []
    for view in range(V):
        M = mats[view][which].reshape(n, 3, 4)
        with torch.no_grad():
            zc0 = (M[:, 2, :3] * xyz).sum(1) + M[:, 2, 3]
            first = torch.nonzero((zc0 > znear) & (zc0 < zfar) & (opacity >= min_alpha) & torch.isfinite(opacity))[:, 0]
        Mk = M[first]
        cam_p = (Mk[:, :, :3] @ xyz[first][:, :, None])[:, :, 0] + Mk[:, :, 3]
        xc, yc, zc = cam_p.unbind(1)
        qx, qy = xc / zc, yc / zc
        inx, iny = (qx.detach().abs() <= limx), (qy.detach().abs() <= limy)
        tx = torch.where(inx, qx, qx.detach().clamp(-limx, limx)) * zc
        ty = torch.where(iny, qy, qy.detach().clamp(-limy, limy)) * zc
        zero = torch.zeros_like(zc)
        J = torch.stack([torch.stack([fx / zc, zero, -fx * tx / zc ** 2], 1), torch.stack([zero, fy / zc, -fy * ty / zc ** 2], 1)], 1)
        s = cov[first]
        Sigma = torch.stack([s[:, 0], s[:, 1], s[:, 2], s[:, 1], s[:, 3], s[:, 4], s[:, 2], s[:, 4], s[:, 5]], 1).reshape(-1, 3, 3)
        Tm = J @ Mk[:, :, :3]
        c2 = Tm @ Sigma @ Tm.transpose(1, 2) + 0.3 * torch.eye(2, dtype=D)
        a, b, c = c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1]
        det = a * c - b * b
        u, v = fx * qx + cx, fy * qy + cy
        with torch.no_grad():
            mid = 0.5 * (a + c)
            rad = torch.ceil(3.0 * torch.sqrt(mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1))))
            x0, x1 = torch.floor((u - rad) / 16).clamp(0, TX), (torch.floor((u + rad) / 16) + 1).clamp(0, TX)
            y0, y1 = torch.floor((v - rad) / 16).clamp(0, TY), (torch.floor((v + rad) / 16) + 1).clamp(0, TY)
            keep = (det > 0) & torch.isfinite(det) & (rad <= 4096) & ((x1 - x0) * (y1 - y0) > 0)
            kept = torch.nonzero(keep)[:, 0]
            kept = kept[torch.sort(zc[kept], stable=True)[1]]                 # one depth order, the lower index first among equals
        sel = lambda t: t[kept]
        A, B, C = sel(c / det)[:, None, None], sel(-b / det)[:, None, None], sel(a / det)[:, None, None]
        dx, dy = sel(u)[:, None, None] - px, sel(v)[:, None, None] - py
        p = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
        raw = sel(opacity[first])[:, None, None] * torch.exp(p)
        with torch.no_grad():
            rect = ((ii >= 16 * sel(x0)[:, None, None]) & (ii < 16 * sel(x1)[:, None, None]) & (jj >= 16 * sel(y0)[:, None, None])
                    & (jj < 16 * sel(y1)[:, None, None]))
            capped = raw > max_alpha
        al = torch.where(capped, torch.full_like(raw, max_alpha), raw)
        with torch.no_grad():
            live = rect & (p <= 0) & (p >= min_power) & (al >= min_alpha)
        om = torch.where(live, 1.0 - al, torch.ones_like(al))
        incl = torch.cumprod(om, 0)
        Tex = torch.cat([torch.ones_like(incl[:1]), incl[:-1]], 0)
        with torch.no_grad():
            stop = live & (Tex * om < min_t)
            add = live & ~(torch.cumsum(stop.to(torch.int64), 0) > 0)
        w = torch.where(add, al * Tex, torch.zeros_like(al))
        col = colour[first][kept]
        rgb = torch.einsum("nk,nhw->khw", col, w) / 255.0
        depth = (sel(zc)[:, None, None] * w).sum(0)
        alpha = 1.0 - torch.prod(torch.where(add, 1.0 - al, torch.ones_like(al)), 0)
        images.append((rgb, depth, alpha))
    return torch.stack([i[0] for i in images]), torch.stack([i[1] for i in images]), torch.stack([i[2] for i in images])


# ------------------------------------------------------------------------------------------------ the fit, in float64
def covariance64(log_scale, quat):
    """R exp(log_scale)^2 R^T as (n, 6), in the tensors' own precision."""
    w, x, y, z = (quat / quat.norm(dim=1, keepdim=True)).unbind(1)
    rot = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                       2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    m = rot * torch.exp(log_scale)[:, None, :]
    full = m @ m.transpose(1, 2)
    return torch.stack([full[:, 0, 0], full[:, 0, 1], full[:, 0, 2], full[:, 1, 1], full[:, 1, 2], full[:, 2, 2]], dim=1)


def fit_problem(n=200, hw=(40, 56), seed=7):
    """The fit both tests run: gr.seeded_scene seen from three cameras (the scene's own and two moved 0.3 m sideways); the target is the
    scene itself, the start has every colour at 128, the opacity halved and the positions jittered by a seeded 0.02 m.  Returns the
    start as fp32 arrays (xyz, colour, log_scale, quat, opacity_logit), the matrices (3, 1, 12), the camera and the targets (3, 3, H, W)
    float64 drawn by `textbook`."""
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene(n, hw, seed)
    views = np.repeat(mats, 3, axis=0).copy()
    views[1, 0, 3] += F(0.3)
    views[2, 0, 3] -= F(0.3)
    opacity = np.minimum(opacity, F(0.98))
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=F).astype(np.float64))
    with torch.no_grad():
        targets = textbook(t64(xyz), t64(rgb), t64(cov), t64(opacity), views, cam, hw)[0]
    start_xyz = (xyz + np.random.default_rng(seed + 1).normal(size=xyz.shape).astype(F) * F(0.02)).astype(F)
    half = (opacity * F(0.5)).astype(F)
    quat = np.zeros((len(xyz), 4), F)
    quat[:, 0] = 1
    start = dict(xyz=start_xyz, colour=np.full((len(xyz), 3), 128, F), log_scale=np.repeat(np.log(np.sqrt(cov[:, :1])), 3, axis=1).astype(F),
                 quat=quat, opacity_logit=(np.log(half) - np.log1p(-half)).astype(F))
    return start, views, cam, targets


def textbook_fit(start, views, cam, targets, hw, rates, iters, betas, eps):
    """torch.optim.Adam over the float64 textbook with per-parameter learning rates: the loss (mean absolute rgb difference) of every step."""
    params = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in start.items()}
    opt = torch.optim.Adam([{"params": [p], "lr": float(rates[k])} for k, p in params.items()], betas=betas, eps=eps)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        rgb = textbook(params["xyz"], params["colour"], covariance64(params["log_scale"], params["quat"]),
                       torch.sigmoid(params["opacity_logit"]), views, cam, hw)[0]
        loss = (rgb - targets).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses
