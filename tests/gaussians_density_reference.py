"""Density control for the Gaussian fit on the CPU, written from the rule and not from the kernels, and what it is
measured against.

`accumulate`, `plan` and `apply` are the definition: numpy, one rounded operation per numpy call in the order the rule writes them,
vectorised over the Gaussians, in the precision of their inputs (fp32 for the definition the kernels are bit-equal to, float64 inside
`textbook_fit_density`).  `textbook_centres` is gaussians_bwd_reference.textbook with the projected centres of every view returned, so
that autograd's gradient with respect to them is the float64 truth of the statistic; `textbook_fit_density` is the float64 fit with the
same schedule as mudg_amd.gaussians.fit.  The product never imports this module."""
import numpy as np
import torch

import gaussians_bwd_reference as gb
import gaussians_reference as gr

F = np.float32
KEEP, PRUNE, CLONE, SPLIT = 0, 1, 2, 3
PARAMETERS = ("xyz", "colour", "log_scale", "quat", "opacity_logit")


# ------------------------------------------------------------------------------------------------ the rule
def accumulate(partial, count, offsets, hw, grad_sum, seen):
    """grad_sum (n,) and seen (n,) int32 after one backward: new arrays.  partial (E, 10), count (V, n), offsets (V, n) int64."""
    partial = np.asarray(partial)
    T = partial.dtype.type
    E = len(partial)
    V, n = count.shape
    grad_sum, seen = np.array(grad_sum, dtype=partial.dtype), np.array(seen, dtype=np.int32)
    half_w, half_h = T(0.5) * T(hw[1]), T(0.5) * T(hw[0])
    with np.errstate(all="ignore"):
        for view in range(V):
            for g in range(n):
                cnt, off = int(count[view, g]), int(offsets[view, g])
                if cnt <= 0 or off < 0 or off > E - cnt:
                    continue
                su, sv = T(0.0), T(0.0)
                for k in range(cnt):
                    su = su + partial[off + k, 8]
                    sv = sv + partial[off + k, 9]
                a, b = half_w * su, half_h * sv
                grad_sum[g] = grad_sum[g] + np.sqrt(a * a + b * b)
                seen[g] += 1
    return grad_sum, seen


def plan(grad_sum, seen, opacity, scale, grad_threshold, split_scale, min_opacity, max_scale, grow=True):
    """action (n,) and rows (n,) int32."""
    grad_sum, opacity, scale = np.asarray(grad_sum), np.asarray(opacity), np.asarray(scale)
    T = grad_sum.dtype.type
    seen = np.asarray(seen, dtype=np.int32)
    smax = np.fmax(np.fmax(scale[:, 0], scale[:, 1]), scale[:, 2])
    with np.errstate(all="ignore"):
        prune = (np.isnan(grad_sum) | np.isnan(opacity) | np.isnan(scale).any(axis=1) | (opacity < T(min_opacity)) | (smax > T(max_scale)))
        mean = grad_sum / seen.astype(grad_sum.dtype)
        grows = bool(grow) & (seen > 0) & (mean >= T(grad_threshold))
    action = np.where(prune, PRUNE, np.where(grows, np.where(smax > T(split_scale), SPLIT, CLONE), KEEP)).astype(np.int32)
    rows = np.array([1, 0, 2, 2], dtype=np.int32)[action]
    return action, rows


def apply(action, start, n_out, scale, rot, tensors, split_offset, log_shrink, ids=None, fill=None):
    """tensors: the fifteen arrays (value, m, v of each of PARAMETERS).  Returns the fifteen with n_out rows and ids (or None).  Rows that no
    start reaches hold `fill` (a list of fifteen arrays and one for ids to write into) or zero."""
    n = len(action)
    T = np.asarray(tensors[0]).dtype.type
    outs = [np.zeros((n_out,) + np.asarray(t).shape[1:], np.asarray(t).dtype) for t in tensors] if fill is None else fill[:15]
    ids_out = None if ids is None else (np.zeros(n_out, np.int32) if fill is None else fill[15])
    for g in range(n):
        act = int(action[g])
        if act not in (KEEP, CLONE, SPLIT):
            continue
        copies = 1 if act == KEEP else 2
        at = int(start[g])
        if at < 0 or at > n_out - copies:
            continue
        shift = None
        if act == SPLIT:
            s = scale[g]
            k = 0 if (s[0] >= s[1] and s[0] >= s[2]) else (1 if s[1] >= s[2] else 2)
            d = T(split_offset) * s[k]
            shift = d * np.asarray(rot[g]).reshape(3, 3)[:, k]
        for p in range(5):
            x, m, v = tensors[3 * p][g], tensors[3 * p + 1][g], tensors[3 * p + 2][g]
            for r in range(copies):
                y = x
                if act == SPLIT and p == 0:
                    y = x + shift if r == 0 else x - shift
                if act == SPLIT and p == 2:
                    y = x - T(log_shrink)
                carries = act == KEEP or (act == CLONE and r == 0)
                outs[3 * p][at + r] = y
                outs[3 * p + 1][at + r] = m if carries else 0
                outs[3 * p + 2][at + r] = v if carries else 0
        if ids is not None:
            ids_out[at:at + copies] = ids[g]
    return outs, ids_out


def rotation(quat):
    """(n, 4) -> (n, 9): the rotation of the normalised quaternion, row-major, in the array's precision."""
    q = quat / np.sqrt((quat * quat).sum(axis=1, keepdims=True))
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)


def densify(params, moments, ids, grad_sum, seen, control, grow=True):
    """plan -> exclusive sum -> apply on host arrays, with mudg_amd.gaussians.densify_and_prune's fall-back to prune-only.  params and
    moments: dicts over PARAMETERS (moments: (m, v)).  Returns new params, moments, ids and the counts."""
    T = params["xyz"].dtype.type
    scale = np.exp(params["log_scale"])
    opacity = T(1.0) / (T(1.0) + np.exp(-params["opacity_logit"]))
    for grew in ((True, False) if grow else (False,)):
        action, rows = plan(grad_sum, seen, opacity, scale, control.grad_threshold, control.split_scale, control.min_opacity, control.max_scale, grew)
        total = int(rows.astype(np.int64).sum())
        if not grew or control.max_gaussians is None or total <= control.max_gaussians:
            break
    if total <= 0:
        raise ValueError("every Gaussian would be pruned")
    start = np.cumsum(rows.astype(np.int64)) - rows
    tensors = []
    for name in PARAMETERS:
        tensors += [params[name], moments[name][0], moments[name][1]]
    outs, ids = apply(action, start, total, scale, rotation(params["quat"]), tensors, control.split_offset, control.log_shrink, ids)
    counts = np.bincount(action, minlength=4).tolist()
    return ({n: outs[3 * k] for k, n in enumerate(PARAMETERS)}, {n: (outs[3 * k + 1], outs[3 * k + 2]) for k, n in enumerate(PARAMETERS)}, ids,
            dict(before=len(action), after=total, kept=counts[0], pruned=counts[1], cloned=counts[2], split=counts[3], grew=grew))


# ------------------------------------------------------------------------------------------------ the float64 textbook with its centres
def textbook_centres(xyz, colour, cov, opacity, mats, cam, hw, ids=None, znear=gr.ZNEAR, zfar=gr.ZFAR):
    """gaussians_bwd_reference.textbook, statement for statement, that also returns per view (index, u, v): the Gaussians the view draws
    (indices into xyz, in depth order) and their projected centres as tensors of the graph, gradients retained."""
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
    images, centres = [], []
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
        uk, vk = sel(u), sel(v)
        if uk.requires_grad:
            uk.retain_grad()
            vk.retain_grad()
        centres.append((first[kept], uk, vk))
        A, B, C = sel(c / det)[:, None, None], sel(-b / det)[:, None, None], sel(a / det)[:, None, None]
        dx, dy = uk[:, None, None] - px, vk[:, None, None] - py
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
    return (torch.stack([i[0] for i in images]), torch.stack([i[1] for i in images]), torch.stack([i[2] for i in images])), centres


def centre_gradient_norms(centres, n, hw):
    """After backward: (V, n) float64, sqrt((0.5 W du)^2 + (0.5 H dv)^2) of every view (zero where the view does not draw the Gaussian),
    and (V, n) bool, which Gaussians each view draws."""
    gn, drawn = np.zeros((len(centres), n)), np.zeros((len(centres), n), dtype=bool)
    for view, (index, u, v) in enumerate(centres):
        if len(index) and u.grad is not None:
            gn[view, index.numpy()] = torch.sqrt((0.5 * hw[1] * u.grad) ** 2 + (0.5 * hw[0] * v.grad) ** 2).numpy()
        drawn[view, index.numpy()] = True
    return gn, drawn


# ------------------------------------------------------------------------------------------------ the fit with density control, float64
def holed_start(start, views, cam, hw):
    """gb.fit_problem()'s start without the Gaussians whose centre projects into the middle third of the image width in view 0."""
    xyz = start["xyz"].astype(np.float64)
    m = np.asarray(views[0, 0], dtype=np.float64).reshape(3, 4)
    p = xyz @ m[:, :3].T + m[:, 3]
    u = float(F(cam[0])) * p[:, 0] / p[:, 2] + float(F(cam[2]))
    keep = ~((u >= hw[1] / 3.0) & (u < 2.0 * hw[1] / 3.0) & (p[:, 2] > 0))
    return {k: np.ascontiguousarray(v[keep]) for k, v in start.items()}, keep


def textbook_fit_density(start, views, cam, targets, hw, rates, iters, betas, eps, control):
    """The float64 counterpart of mudg_amd.gaussians.fit(..., density=control): Adam with explicit moments and one running step count,
    statistics from autograd's gradient of the projected centres, `densify` on the schedule of DensityControl.  Returns the losses and
    the steps' counts."""
    params = {k: start[k].astype(np.float64) for k in PARAMETERS}
    moments = {k: (np.zeros_like(params[k]), np.zeros_like(params[k])) for k in PARAMETERS}
    b1, b2 = betas
    losses, history = [], []
    grad_sum = seen = None
    for it in range(iters):
        leaves = {k: torch.tensor(params[k], requires_grad=True) for k in PARAMETERS}
        (rgb, _, _), centres = textbook_centres(leaves["xyz"], leaves["colour"], gb.covariance64(leaves["log_scale"], leaves["quat"]),
                                                torch.sigmoid(leaves["opacity_logit"]), views, cam, hw)
        loss = (rgb - targets).abs().mean()
        loss.backward()
        losses.append(float(loss.detach()))
        n = len(params["xyz"])
        gathers = control is not None and control.gathers(it)
        if gathers:
            if grad_sum is None:
                grad_sum, seen = np.zeros(n), np.zeros(n, np.int32)
            gn, drawn = centre_gradient_norms(centres, n, hw)
            for view in range(len(centres)):
                grad_sum = grad_sum + gn[view]
                seen = seen + drawn[view].astype(np.int32)
        for k in PARAMETERS:
            g = np.zeros_like(params[k]) if leaves[k].grad is None else leaves[k].grad.numpy()
            m = b1 * moments[k][0] + (1 - b1) * g
            v = b2 * moments[k][1] + (1 - b2) * g * g
            moments[k] = (m, v)
            step = float(rates[k]) / (1 - b1 ** (it + 1))
            params[k] = params[k] - step * m / (np.sqrt(v) / np.sqrt(1 - b2 ** (it + 1)) + eps)
        if gathers and control.densifies_after(it):
            params, moments, _, counts = densify(params, moments, None, grad_sum, seen, control)
            history.append(dict(counts, iteration=it))
            grad_sum = seen = None
        if gathers and control.resets_after(it):
            params["opacity_logit"] = np.minimum(params["opacity_logit"], control.reset_logit)
            moments["opacity_logit"] = (np.zeros_like(params["opacity_logit"]), np.zeros_like(params["opacity_logit"]))
    return losses, history
