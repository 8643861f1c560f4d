"""The rule of DESIGN.md §29 (semantic Gaussians) on the CPU, written from the rule and not from the kernels.

`blend_feat`, `blend_bwd_feat`, `feat_bwd`, `class_loss` and `class_loss_bwd` are the definition: numpy fp32, one rounded operation per
numpy call in the order the rule writes them, vectorised over a tile's 256 lanes, with §24's reduction order (an xor butterfly over 1, 2,
4, 8, 16, 32 inside each wave of 64 lanes, then ((w0 + w1) + w2) + w3).  Sums over the channel k run ascending from +0.0.  `log_rule` is
L, the fixed-rule logarithm on [1, 32]; E is gaussians_reference.exp_rule.  `textbook_features` adds feature images to the float64
renderer of gaussians_bwd_reference.  The product never imports this module."""
import numpy as np
import torch

import gaussians_bwd_reference as gb
import gaussians_reference as gr

F = np.float32
SUMS = gb.SUMS
FEAT_MAX = 32
MIN_SCORE = F(-80.0)
SQRT_HALF = F(float.fromhex("0x1.6a09e6p-1"))
LN2 = F(float.fromhex("0x1.62e430p-1"))
# P of log(1 + t) = t P(t) on sqrt(1/2) - 1 <= t < sqrt(2) - 1, highest degree first: a least-squares fit at 4000 Chebyshev nodes, rounded to fp32
LOG_COEFFICIENTS = tuple(F(float.fromhex(h)) for h in ("0x1.6626eap-4", "-0x1.26729ep-3", "0x1.322850p-3", "-0x1.5329bep-3", "0x1.98b80ap-3",
                                                       "-0x1.0005a6p-2", "0x1.555790p-2", "-0x1.fffff8p-2", "0x1.0p+0"))
_LANES = np.arange(64)


def log_rule(s):
    """L(s) for fp32 s in [1, 32]: s = 2^e m with sqrt(1/2) <= m < sqrt(2), t = m - 1, e ln 2 + t P(t)."""
    s = np.asarray(s, dtype=F)
    m, e = np.frexp(s)
    m, e = m.astype(F), e.astype(np.int32)
    low = m < SQRT_HALF
    m = np.where(low, m * F(2.0), m)
    e = np.where(low, e - 1, e)
    t = m - F(1.0)
    r = np.full_like(t, LOG_COEFFICIENTS[0])
    for c in LOG_COEFFICIENTS[1:]:
        r = r * t
        r = r + c
    return e.astype(F) * LN2 + r * t


def reduce_tile(r):
    """(256, C) -> (C,): the butterfly inside each wave, then ((w0 + w1) + w2) + w3, in r's dtype."""
    v = r.reshape(4, 64, -1)
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[:, _LANES ^ s, :]
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def _range(ranges, t, E):
    start, end = int(ranges[t, 0]), int(ranges[t, 1])
    return (0, 0) if start < 0 or end > E or start > end else (start, end)


def _row(feat, g):
    return feat[g] if 0 <= g < len(feat) else np.zeros(feat.shape[1], F)    # a sorted value outside the cloud reads no row


# ------------------------------------------------------------------------------------------------ the forward
def blend_feat(proj, colour, feat, values, ranges, hw):
    """gb.blend_train with the features' line.  colour (n, 3) or (V, n, 3), feat (n, Fn).  Returns rgb, depth, alpha, state (V, 5, H, W)
    and feat_out (V, Fn, H, W), the raw sums."""
    H, W = hw
    TX, TY = gr.tiles(hw)
    NT = TX * TY
    V, n = proj["count"].shape
    E = len(values)
    colour, feat = np.asarray(colour, dtype=F), np.asarray(feat, dtype=F)
    Fn = feat.shape[1]
    state = np.zeros((V, 5, H, W), F)
    state[:, 4] = 1
    feat_out = np.zeros((V, Fn, H, W), F)
    with np.errstate(all="ignore"):
        for t in range(V * NT):
            view, tile = divmod(t, NT)
            col = colour[view] if colour.ndim == 3 else colour
            i, j, inside, px, py = gb._lanes(tile, TX, H, W)
            T, acc, fk, done = np.ones(256, F), [np.zeros(256, F) for _ in range(4)], np.zeros((256, Fn), F), ~inside
            start, end = _range(ranges, t, E)
            for e in range(start, end):
                if done.all():
                    break
                g = int(values[e])
                ent = gb._entry(proj, col, view, g, n)
                _, _, _, _, al, _, Tn, skip = gb._step(ent, px, py, T)
                live = ~done & ~skip
                ends = live & (Tn < gr.MIN_T)
                done = done | ends
                add = live & ~ends
                w = al * T
                for k, c in enumerate((ent[7], ent[8], ent[9], ent[6])):
                    acc[k] = np.where(add, acc[k] + c * w, acc[k])
                fk = np.where(add[:, None], fk + _row(feat, g)[None, :] * w[:, None], fk)
                T = np.where(add, Tn, T)
            for k in range(4):
                state[view, k, j[inside], i[inside]] = acc[k][inside]
            state[view, 4, j[inside], i[inside]] = T[inside]
            feat_out[view][:, j[inside], i[inside]] = fk[inside].T
    return state[:, :3] / F(255.0), state[:, 3].copy(), F(1.0) - state[:, 4], state, feat_out


# ------------------------------------------------------------------------------------------------ the blend's backward
def blend_bwd_feat(proj, colour, feat, values, order, ranges, hw, state, feat_out, d_rgb, d_depth, d_alpha, d_feat):
    """partial (E, 10) and partial_feat (E, Fn) fp32 at the unsorted positions."""
    H, W = hw
    TX, TY = gr.tiles(hw)
    NT = TX * TY
    V, n = proj["count"].shape
    E = len(values)
    colour, feat, state, feat_out = (np.asarray(a, dtype=F) for a in (colour, feat, state, feat_out))
    d_rgb, d_depth, d_alpha, d_feat = (np.asarray(a, dtype=F) for a in (d_rgb, d_depth, d_alpha, d_feat))
    Fn = feat.shape[1]
    partial, partial_feat = np.zeros((E, SUMS), F), np.zeros((E, Fn), F)
    with np.errstate(all="ignore"):
        for t in range(V * NT):
            view, tile = divmod(t, NT)
            col = colour[view] if colour.ndim == 3 else colour
            i, j, inside, px, py = gb._lanes(tile, TX, H, W)
            ii, jj = np.where(inside, i, 0), np.where(inside, j, 0)
            pick = lambda a: np.where(inside, a[jj, ii], F(0.0)).astype(F)
            gC = [pick(d_rgb[view, k]) / F(255.0) for k in range(3)]
            gD = pick(d_depth[view])
            S = [pick(state[view, k]) for k in range(4)]
            gAT = pick(d_alpha[view]) * pick(state[view, 4])
            gF = [pick(d_feat[view, k]) for k in range(Fn)]
            Stot, P = np.zeros(256, F), np.zeros(256, F)
            for k in range(Fn):
                Stot = Stot + gF[k] * pick(feat_out[view, k])
            T, acc, done = np.ones(256, F), [np.zeros(256, F) for _ in range(4)], ~inside
            start, end = _range(ranges, t, E)
            for base in range(start, end, gb.BATCH):
                if done.all():
                    break
                for e in range(base, min(base + gb.BATCH, end)):
                    g = int(values[e])
                    ent = gb._entry(proj, col, view, g, n)
                    u, v, A, B, C, op, zc, k0, k1, k2 = ent
                    row = _row(feat, g)
                    dx, dy, ge, raw, al, om, Tn, skip = gb._step(ent, px, py, T)
                    live = ~done & ~skip
                    ends = live & (Tn < gr.MIN_T)
                    done = done | ends
                    add = live & ~ends
                    w = al * T
                    for k, c in enumerate((k0, k1, k2, zc)):
                        acc[k] = np.where(add, acc[k] + c * w, acc[k])
                    s = np.zeros(256, F)
                    for k in range(Fn):
                        s = s + gF[k] * row[k]
                    P = np.where(add, P + s * w, P)
                    own = (((gC[0] * k0 + gC[1] * k1) + gC[2] * k2) + gD * zc) + s
                    behind = ((gC[0] * (S[0] - acc[0]) + gC[1] * (S[1] - acc[1])) + gC[2] * (S[2] - acc[2])) + gD * (S[3] - acc[3])
                    behind = behind + (Stot - P)
                    dal = (T * own - behind / om) + gAT / om
                    dp = (dal * op) * ge
                    free = add & ~(raw > gr.MAX_ALPHA)
                    r = np.zeros((256, SUMS + Fn), F)
                    for k in range(3):
                        r[:, k] = np.where(add, gC[k] * w, F(0.0))
                    r[:, 3] = np.where(add, gD * w, F(0.0))
                    r[:, 4] = np.where(free, dal * ge, F(0.0))
                    r[:, 5] = np.where(free, dp * (F(-0.5) * (dx * dx)), F(0.0))
                    r[:, 6] = np.where(free, dp * -(dx * dy), F(0.0))
                    r[:, 7] = np.where(free, dp * (F(-0.5) * (dy * dy)), F(0.0))
                    r[:, 8] = np.where(free, dp * -(A * dx + B * dy), F(0.0))
                    r[:, 9] = np.where(free, dp * -(C * dy + B * dx), F(0.0))
                    for k in range(Fn):
                        r[:, SUMS + k] = np.where(add, gF[k] * w, F(0.0))
                    T = np.where(add, Tn, T)
                    at = int(order[e])
                    if 0 <= at < E:
                        sums = reduce_tile(r)
                        partial[at], partial_feat[at] = sums[:SUMS], sums[SUMS:]
    return partial, partial_feat


def feat_bwd(count, offsets, partial_feat):
    """d_feat_g (n, Fn): per view the Gaussian's rows in ascending order from +0, the views' sums added in view order from +0."""
    partial_feat = np.asarray(partial_feat, dtype=F)
    V, n = count.shape
    E, Fn = partial_feat.shape
    out = np.zeros((n, Fn), F)
    for view in range(V):
        for g in range(n):
            cnt, off = int(count[view, g]), int(offsets[view, g])
            if cnt <= 0 or off < 0 or off > E - cnt:
                continue
            acc = np.zeros(Fn, F)
            for k in range(cnt):
                acc = acc + partial_feat[off + k]
            out[g] = out[g] + acc
    return out


# ------------------------------------------------------------------------------------------------ the class loss
def class_loss(x, labels, weight=1.0):
    """x (V, Fn, H, W) fp32, labels (V, H, W) uint8.  Returns maps (V, Fn, H, W), partial (V NT, 2) fp32 (the second word the labelled
    count's int32 bits) and totals (4,) fp32 = (sum l, the count's int32 bits, float(max(count, 1)), the loss)."""
    x, labels = np.asarray(x, dtype=F), np.asarray(labels, dtype=np.uint8)
    V, Fn, H, W = x.shape
    TX, TY = gr.tiles((H, W))
    NT = TX * TY
    lab = labels.astype(np.int64)
    labelled = lab < Fn
    with np.errstate(all="ignore"):
        m = x[:, 0]
        for k in range(1, Fn):
            m = np.fmax(m, x[:, k])
        p = np.fmax(x - m[:, None], MIN_SCORE)
        e = gr.exp_rule(p)
        S = np.zeros_like(m)
        for k in range(Fn):
            S = S + e[:, k]
        hot = (np.arange(Fn)[None, :, None, None] == lab[:, None]).astype(F)
        maps = np.where(labelled[:, None], e / S[:, None] - hot, F(0.0)).astype(F)
        p_label = np.take_along_axis(p, np.clip(lab, 0, Fn - 1)[:, None], axis=1)[:, 0]
        l = np.where(labelled, log_rule(S) - p_label, F(0.0)).astype(F)
    partial = np.zeros((V * NT, 2), F)
    counts = np.zeros(V * NT, np.int32)
    for t in range(V * NT):
        view, tile = divmod(t, NT)
        i, j, inside, _, _ = gb._lanes(tile, TX, H, W)
        ii, jj = np.where(inside, i, 0), np.where(inside, j, 0)
        partial[t, 0] = reduce_tile(np.where(inside, l[view][jj, ii], F(0.0)).astype(F)[:, None])[0]
        counts[t] = int((inside & labelled[view][jj, ii]).sum())
    partial[:, 1] = counts.view(F)
    # the finish: lane l adds the tiles l, l + 256, ... in fp64, then the tile's order over the 256 lanes
    lanes = np.zeros(256, np.float64)
    for q in range(V * NT):
        lanes[q % 256] = lanes[q % 256] + np.float64(partial[q, 0])
    total = float(reduce_tile(lanes[:, None])[0])
    count = int(counts.astype(np.int64).sum())
    seen = max(count, 1)
    totals = np.zeros(4, F)
    totals[0] = F(total)
    totals[1:2] = np.array([min(count, 0x7fffffff)], np.int32).view(F)
    totals[2] = F(seen)
    totals[3] = F(weight) * F(total / float(seen))
    return maps, partial, totals


def class_loss_bwd(maps, totals, up, weight=1.0):
    """d_x = ((up weight) / max(count, 1)) maps."""
    return ((F(up) * F(weight)) / totals[2]) * np.asarray(maps, dtype=F)


def labels_of(feat_out, alpha, label_alpha=0.5):
    """render's label image: the argmax over k, the lowest index on ties, 255 where alpha <= label_alpha."""
    lab = np.argmax(np.asarray(feat_out), axis=1).astype(np.uint8)
    return np.where(np.asarray(alpha) > F(label_alpha), lab, np.uint8(255)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the whole rule
def render_backward(xyz, colour, feat, cov, opacity, ids, mats, cam, hw, d_rgb, d_depth, d_alpha, d_feat, znear=gr.ZNEAR, zfar=gr.ZFAR):
    """Forward with features, then the three backward steps.  A dict with the images, the states, both partial buffers and the gradients."""
    xyz, colour, feat, cov, opacity = (np.asarray(a, dtype=F) for a in (xyz, colour, feat, cov, opacity))
    proj = gr.project(xyz, cov, opacity, ids, mats, cam, hw, znear, zfar)
    out = dict(proj, entries=int(proj["count"].astype(np.int64).sum()))
    assert out["entries"] > 0
    keys, values, order, ranges, offsets = gb.bin_with_order(proj, hw)
    rgb, depth, alpha, state, feat_out = blend_feat(proj, colour, feat, values, ranges, hw)
    partial, partial_feat = blend_bwd_feat(proj, colour, feat, values, order, ranges, hw, state, feat_out, d_rgb, d_depth, d_alpha, d_feat)
    d_xyz, d_cov, d_op, d_col = gb.project_bwd(xyz, cov, ids, mats, cam, hw, proj["count"], offsets, partial, znear, zfar)
    out.update(rgb=rgb, depth_image=depth, alpha=alpha, state=state, feat_out=feat_out, values=values, order=order, ranges=ranges,
               offsets=offsets, partial=partial, partial_feat=partial_feat, d_xyz=d_xyz, d_cov=d_cov, d_opacity=d_op, d_colour=d_col,
               d_feat_g=feat_bwd(proj["count"], offsets, partial_feat))
    return out


# ------------------------------------------------------------------------------------------------ the float64 textbook
def textbook_features(xyz, colour, feat, cov, opacity, mats, cam, hw):
    """gb.textbook with F more channels: rgb, depth, alpha and feat (V, Fn, H, W), float64 and differentiable.  The textbook blends any
    number of `colour` columns with the same weights, so the features ride as extra columns in groups of three; its division by 255 is
    undone."""
    Fn = feat.shape[1]
    pad = (-Fn) % 3
    cols = torch.cat([feat, torch.zeros((feat.shape[0], pad), dtype=feat.dtype)], dim=1) if pad else feat
    rgb, depth, alpha = gb.textbook(xyz, colour, cov, opacity, mats, cam, hw)
    groups = [gb.textbook(xyz, cols[:, k:k + 3], cov, opacity, mats, cam, hw)[0] * 255.0 for k in range(0, Fn + pad, 3)]
    return rgb, depth, alpha, torch.cat(groups, dim=1)[:, :Fn]
