"""The view-dependent colour rule of DESIGN.md §27 on the CPU, written from the rule and not from the kernels, and what it approximates.

`basis`, `basis_gradient`, `directions`, `colours`, `gather`, `colours_backward` and `render_backward` are the definition: numpy, one
rounded operation per numpy call in the order the rule writes them, vectorised over the Gaussians.  With dtype = float32 (the default)
every operation is a single rounded fp32 operation, which is what the kernels of csrc/gaussians_sh.hip perform; with dtype = float64 the
same expressions run in double precision on the same fp32 inputs, which is what the comparison with autograd uses.  `textbook_colours`
is a float64 differentiable evaluation in torch that follows the published formulas and not this file's order; `textbook_render` and
`textbook_fit` put it in front of gaussians_bwd_reference.textbook.  The product never imports this module."""
import numpy as np
import torch

import gaussians_bwd_reference as gb
import gaussians_reference as gr

F = np.float32
D = np.float64
MAX_DEGREE = 3
# the real spherical harmonics of the 3DGS code: its constants, order and signs
C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)


def terms(degree):
    """K = (L + 1)^2."""
    return (int(degree) + 1) ** 2


def degree_of(sh):
    """L of coefficients (n, K - 1, 3)."""
    L = {terms(d) - 1: d for d in range(1, MAX_DEGREE + 1)}.get(sh.shape[1])
    assert L is not None and sh.ndim == 3 and sh.shape[2] == 3, sh.shape
    return L


# ------------------------------------------------------------------------------------------------ the basis and its gradient
def _pairs(x, y, z):
    return x * x, y * y, z * z, x * y, y * z, x * z


def basis(d, degree, dtype=F):
    """d (n, 3) unit directions -> the K functions B_0 .. B_{K-1}, each (n,).  B_0 is the constant the rule folds into `colour`."""
    T = dtype
    x, y, z = (np.asarray(d[:, k], dtype=T) for k in range(3))
    xx, yy, zz, xy, yz, xz = _pairs(x, y, z)
    B = [np.full(x.shape, T(C0), T), T(-C1) * y, T(C1) * z, T(-C1) * x]
    if degree >= 2:
        B += [T(C2[0]) * xy, T(C2[1]) * yz, T(C2[2]) * ((T(2) * zz - xx) - yy), T(C2[3]) * xz, T(C2[4]) * (xx - yy)]
    if degree >= 3:
        B += [(T(C3[0]) * y) * (T(3) * xx - yy),
              (T(C3[1]) * xy) * z,
              (T(C3[2]) * y) * ((T(4) * zz - xx) - yy),
              (T(C3[3]) * z) * ((T(2) * zz - T(3) * xx) - T(3) * yy),
              (T(C3[4]) * x) * ((T(4) * zz - xx) - yy),
              (T(C3[5]) * z) * (xx - yy),
              (T(C3[6]) * x) * (xx - T(3) * yy)]
    return B


def basis_gradient(d, s, degree, dtype=F):
    """sum_k s[k] dB_k/dd for k = 1 .. K - 1 as (gx, gy, gz): the terms in ascending k and within a k in the order x, y, z; every term is
    (constant polynomial) s[k]."""
    T = dtype
    x, y, z = (np.asarray(d[:, k], dtype=T) for k in range(3))
    xx, yy, zz, xy, yz, xz = _pairs(x, y, z)
    gy = T(-C1) * s[1]
    gz = T(C1) * s[2]
    gx = T(-C1) * s[3]
    if degree >= 2:
        gx = gx + (T(C2[0]) * y) * s[4]
        gy = gy + (T(C2[0]) * x) * s[4]
        gy = gy + (T(C2[1]) * z) * s[5]
        gz = gz + (T(C2[1]) * y) * s[5]
        gx = gx + (T(C2[2]) * (T(-2) * x)) * s[6]
        gy = gy + (T(C2[2]) * (T(-2) * y)) * s[6]
        gz = gz + (T(C2[2]) * (T(4) * z)) * s[6]
        gx = gx + (T(C2[3]) * z) * s[7]
        gz = gz + (T(C2[3]) * x) * s[7]
        gx = gx + (T(C2[4]) * (T(2) * x)) * s[8]
        gy = gy + (T(C2[4]) * (T(-2) * y)) * s[8]
    if degree >= 3:
        gx = gx + (T(C3[0]) * (T(6) * xy)) * s[9]
        gy = gy + (T(C3[0]) * (T(3) * xx - T(3) * yy)) * s[9]
        gx = gx + (T(C3[1]) * yz) * s[10]
        gy = gy + (T(C3[1]) * xz) * s[10]
        gz = gz + (T(C3[1]) * xy) * s[10]
        gx = gx + (T(C3[2]) * (T(-2) * xy)) * s[11]
        gy = gy + (T(C3[2]) * ((T(4) * zz - xx) - T(3) * yy)) * s[11]
        gz = gz + (T(C3[2]) * (T(8) * yz)) * s[11]
        gx = gx + (T(C3[3]) * (T(-6) * xz)) * s[12]
        gy = gy + (T(C3[3]) * (T(-6) * yz)) * s[12]
        gz = gz + (T(C3[3]) * ((T(6) * zz - T(3) * xx) - T(3) * yy)) * s[12]
        gx = gx + (T(C3[4]) * ((T(4) * zz - T(3) * xx) - yy)) * s[13]
        gy = gy + (T(C3[4]) * (T(-2) * xy)) * s[13]
        gz = gz + (T(C3[4]) * (T(8) * xz)) * s[13]
        gx = gx + (T(C3[5]) * (T(2) * xz)) * s[14]
        gy = gy + (T(C3[5]) * (T(-2) * yz)) * s[14]
        gz = gz + (T(C3[5]) * (xx - yy)) * s[14]
        gx = gx + (T(C3[6]) * (T(3) * xx - T(3) * yy)) * s[15]
        gy = gy + (T(C3[6]) * (T(-6) * xy)) * s[15]
    return gx, gy, gz


# ------------------------------------------------------------------------------------------------ the forward
def _which(ids, n, nmat):
    return np.zeros(n, dtype=np.int64) if ids is None else np.clip(np.asarray(ids, dtype=np.int64), 0, nmat - 1)


def directions(xyz, m, dtype=F):
    """xyz (n, 3) and every Gaussian's matrix m (n, 12) -> d (n, 3) and |p - c| (n,): c = -R^T t, d = (p - c) / |p - c|."""
    T = dtype
    xyz, m = np.asarray(xyz, dtype=T), np.asarray(m, dtype=T)
    w = []
    for j in range(3):
        c = -((m[:, j] * m[:, 3] + m[:, 4 + j] * m[:, 7]) + m[:, 8 + j] * m[:, 11])
        w.append(xyz[:, j] - c)
    length = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    return np.stack([w[0] / length, w[1] / length, w[2] / length], axis=1), length


def _sums(B, colour, sh, Ka):
    """colour + sum over 1 <= k < Ka of B_k sh[k - 1], (n, 3), before the clamp."""
    a = colour.copy()
    for k in range(1, Ka):
        for ch in range(3):
            a[:, ch] = a[:, ch] + B[k] * sh[:, k - 1, ch]
    return a


def colours(xyz, ids, mats, count, colour, sh, active=None, dtype=F):
    """(V, n, 3): max(0, colour + sum B_k(d) sh[k - 1]) where count (V, n) is positive, +0 elsewhere."""
    T = dtype
    L = degree_of(sh)
    Ka = terms(L if active is None else active)
    mats, colour, sh = np.asarray(mats, dtype=F), np.asarray(colour, dtype=F).astype(T), np.asarray(sh, dtype=F).astype(T)
    V, nmat = mats.shape[:2]
    n = len(xyz)
    which = _which(ids, n, nmat)
    out = np.zeros((V, n, 3), T)
    with np.errstate(all="ignore"):
        for view in range(V):
            d, _ = directions(xyz, mats[view][which], T)
            a = _sums(basis(d, L, T), colour, sh, Ka)
            a = np.where(a < 0, T(0), a)
            out[view] = np.where((np.asarray(count[view]) > 0)[:, None], a, T(0))
    return out


# ------------------------------------------------------------------------------------------------ the backward
def gather(partial, count, offsets):
    """Columns 0 .. 2 of every (view, Gaussian)'s partials added in ascending order from +0 -> g (V, n, 3) fp32 and which (view,
    Gaussian) pairs counted (V, n): count > 0 and the offset inside [0, E - count]."""
    partial = np.asarray(partial, dtype=F)
    E = len(partial)
    V, n = np.asarray(count).shape
    g, ok = np.zeros((V, n, 3), F), np.zeros((V, n), bool)
    for view in range(V):
        cnt, off = np.asarray(count[view]).astype(np.int64), np.asarray(offsets[view], dtype=np.int64)
        ok[view] = (cnt > 0) & (off >= 0) & (off <= E - cnt)
        for i in np.nonzero(ok[view])[0]:
            for k in range(cnt[i]):
                g[view, i] = g[view, i] + partial[off[i] + k, :3]
    return g, ok


def colours_backward(xyz, ids, mats, ok, g, colour, sh, active=None, dtype=F):
    """g (V, n, 3): the gradient of every (view, Gaussian)'s colour; ok (V, n): the pairs that count.  Returns d_colour (n, 3), d_sh
    (n, K - 1, 3) and d_xyz_dir (n, 3), the views added in ascending order from +0."""
    T = dtype
    L = degree_of(sh)
    K, Ka = terms(L), terms(L if active is None else active)
    mats, colour, sh = np.asarray(mats, dtype=F), np.asarray(colour, dtype=F).astype(T), np.asarray(sh, dtype=F).astype(T)
    V, nmat = mats.shape[:2]
    n = len(xyz)
    which = _which(ids, n, nmat)
    d_colour, d_sh, d_xyz = np.zeros((n, 3), T), np.zeros((n, K - 1, 3), T), np.zeros((n, 3), T)
    with np.errstate(all="ignore"):
        for view in range(V):
            on = np.asarray(ok[view], dtype=bool)
            d, length = directions(xyz, mats[view][which], T)
            B = basis(d, L, T)
            a = _sums(B, colour, sh, Ka)
            ge = np.where(a < 0, T(0), np.asarray(g[view], dtype=T))                  # where the clamp cut, nothing passes
            for ch in range(3):
                d_colour[:, ch] = np.where(on, d_colour[:, ch] + ge[:, ch], d_colour[:, ch])
            s = [np.zeros(n, T) for _ in range(K)]
            for k in range(1, Ka):
                s[k] = (ge[:, 0] * sh[:, k - 1, 0] + ge[:, 1] * sh[:, k - 1, 1]) + ge[:, 2] * sh[:, k - 1, 2]
                for ch in range(3):
                    d_sh[:, k - 1, ch] = np.where(on, d_sh[:, k - 1, ch] + B[k] * ge[:, ch], d_sh[:, k - 1, ch])
            gd = basis_gradient(d, s, L, T)
            dot = (d[:, 0] * gd[0] + d[:, 1] * gd[1]) + d[:, 2] * gd[2]
            for j in range(3):
                d_xyz[:, j] = np.where(on, d_xyz[:, j] + (gd[j] - d[:, j] * dot) / length, d_xyz[:, j])
    return d_colour, d_sh, d_xyz


# ------------------------------------------------------------------------------------------------ the chain: bin, colours, blends, backward
def _view(proj, view):
    return {k: v[view:view + 1] for k, v in proj.items()}


def blend_views(proj, cols, values, ranges, hw):
    """gb.blend_train with cols (V, n, 3): a view's tiles take that view's colours.  rgb, depth, alpha, state."""
    V = cols.shape[0]
    NT = len(ranges) // V
    outs = [gb.blend_train(_view(proj, v), cols[v], values, ranges[v * NT:(v + 1) * NT], hw) for v in range(V)]
    return tuple(np.concatenate([o[k] for o in outs], axis=0) for k in range(4))


def blend_bwd_views(proj, cols, values, order, ranges, offsets, hw, state, d_rgb, d_depth, d_alpha):
    """gb.blend_bwd with cols (V, n, 3): partial (E, 10).  A view's entries are the unsorted rows [offsets[view, 0], offsets[view + 1, 0])."""
    V = cols.shape[0]
    NT = len(ranges) // V
    E = len(values)
    partial = np.zeros((E, gb.SUMS), F)
    first = [int(offsets[v, 0]) for v in range(V)] + [E]
    for v in range(V):
        p = gb.blend_bwd(_view(proj, v), cols[v], values, order, ranges[v * NT:(v + 1) * NT], hw, state[v:v + 1], d_rgb[v:v + 1], d_depth[v:v + 1],
                         d_alpha[v:v + 1])
        partial[first[v]:first[v + 1]] = p[first[v]:first[v + 1]]
    return partial


def render_backward(xyz, colour, sh, cov, opacity, ids, mats, cam, hw, d_rgb, d_depth, d_alpha, active=None, znear=gr.ZNEAR, zfar=gr.ZFAR):
    """The differentiable render with harmonics, forward and backward, fp32: a dict with colours, the images, state, partial and the
    gradients d_xyz (projection + direction, one fp32 add), d_xyz_dir, d_cov, d_opacity, d_colour, d_sh."""
    xyz, colour, sh, cov, opacity = (np.asarray(a, dtype=F) for a in (xyz, colour, sh, cov, opacity))
    proj = gr.project(xyz, cov, opacity, ids, mats, cam, hw, znear, zfar)
    out = dict(proj, entries=int(proj["count"].astype(np.int64).sum()))
    assert out["entries"] > 0
    keys, values, order, ranges, offsets = gb.bin_with_order(proj, hw)
    cols = colours(xyz, ids, mats, proj["count"], colour, sh, active)
    rgb, depth, alpha, state = blend_views(proj, cols, values, ranges, hw)
    partial = blend_bwd_views(proj, cols, values, order, ranges, offsets, hw, state, d_rgb, d_depth, d_alpha)
    d_xyz, d_cov, d_op, _ = gb.project_bwd(xyz, cov, ids, mats, cam, hw, proj["count"], offsets, partial, znear, zfar)
    g, ok = gather(partial, proj["count"], offsets)
    d_col, d_sh, d_dir = colours_backward(xyz, ids, mats, ok, g, colour, sh, active)
    out.update(colours=cols, rgb=rgb, depth_image=depth, alpha=alpha, state=state, values=values, order=order, ranges=ranges, offsets=offsets,
               partial=partial, d_xyz=d_xyz + d_dir, d_xyz_dir=d_dir, d_cov=d_cov, d_opacity=d_op, d_colour=d_col, d_sh=d_sh)
    return out


# ------------------------------------------------------------------------------------------------ the float64 textbook in torch
def textbook_basis(d, degree):
    """d (..., 3) float64 torch -> (..., K): the published formulas (the 3DGS code's eval_sh), the constant term first."""
    x, y, z = d.unbind(-1)
    B = [torch.full_like(x, C0), -C1 * y, C1 * z, -C1 * x]
    if degree >= 2:
        B += [C2[0] * x * y, C2[1] * y * z, C2[2] * (2 * z * z - x * x - y * y), C2[3] * x * z, C2[4] * (x * x - y * y)]
    if degree >= 3:
        B += [C3[0] * y * (3 * x * x - y * y), C3[1] * x * y * z, C3[2] * y * (4 * z * z - x * x - y * y),
              C3[3] * z * (2 * z * z - 3 * x * x - 3 * y * y), C3[4] * x * (4 * z * z - x * x - y * y), C3[5] * z * (x * x - y * y),
              C3[6] * x * (x * x - 3 * y * y)]
    return torch.stack(B, dim=-1)


def textbook_colours(xyz, colour, sh, mats, ids=None, active=None):
    """float64 torch tensors xyz (n, 3), colour (n, 3), sh (n, K - 1, 3), differentiable; mats (V, nmat, 12) -> (V, n, 3), no count mask."""
    mats = torch.as_tensor(np.asarray(mats), dtype=torch.float64)
    V, nmat = mats.shape[:2]
    n = xyz.shape[0]
    L = degree_of(sh)
    Ka = terms(L if active is None else active)
    which = torch.zeros(n, dtype=torch.long) if ids is None else torch.as_tensor(np.asarray(ids)).long().clamp(0, nmat - 1)
    out = []
    for view in range(V):
        M = mats[view][which].reshape(n, 3, 4)
        centre = -(M[:, :, :3].transpose(1, 2) @ M[:, :, 3:])[:, :, 0]
        w = xyz - centre
        B = textbook_basis(w / w.norm(dim=1, keepdim=True), L)
        out.append(torch.clamp(colour + torch.einsum("nk,nkc->nc", B[:, 1:Ka], sh[:, :Ka - 1]), min=0.0))
    return torch.stack(out)


def textbook_render(xyz, colour, sh, cov, opacity, mats, cam, hw, ids=None, active=None):
    """gb.textbook with view-dependent colour (sh None: constant colour): rgb (V, 3, H, W), depth, alpha; float64, differentiable."""
    mats = np.asarray(mats)
    V = mats.shape[0]
    cols = colour[None].expand(V, -1, -1) if sh is None else textbook_colours(xyz, colour, sh, mats, ids, active)
    views = [gb.textbook(xyz, cols[v], cov, opacity, mats[v:v + 1], cam, hw, ids) for v in range(V)]
    return tuple(torch.cat([v[k] for v in views]) for k in range(3))


# ------------------------------------------------------------------------------------------------ a view-dependent fit
FIT_HW = (40, 56)
FIT_ITERS = 300


def fit_problem(n=200, hw=FIT_HW, seed=7):
    """gb.fit_problem with a target whose colour depends on the direction: gr.seeded_scene seen from three cameras that stand around it
    (the scene's own and two turned by 0.35 rad about the vertical axis through the scene's middle), every Gaussian with seeded degree-2
    coefficients of up to 40 byte units; the targets (3, 3, H, W) float64 are drawn by textbook_render.  The start is gb.fit_problem's:
    every colour 128, the opacity halved, the positions jittered."""
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene(n, hw, seed)
    base = np.concatenate([mats[0, 0].astype(D).reshape(3, 4), [[0, 0, 0, 1]]])
    middle = np.array([0.0, 0.0, 11.0])
    views = []
    for angle in (0.0, 0.35, -0.35):
        c, s = np.cos(angle), np.sin(angle)
        turn = np.eye(4)
        turn[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        turn[:3, 3] = middle - turn[:3, :3] @ middle                                 # a rotation about the vertical axis through `middle`
        views.append((base @ turn)[:3].reshape(1, 12))
    views = np.stack(views).astype(F)
    opacity = np.minimum(opacity, F(0.98))
    truth = (np.random.default_rng(seed + 2).uniform(-40.0, 40.0, (len(xyz), terms(2) - 1, 3))).astype(F)
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=F).astype(D))
    with torch.no_grad():
        targets = textbook_render(t64(xyz), t64(rgb), t64(truth), t64(cov), t64(opacity), views, cam, hw)[0]
    start = gb.fit_problem(n, hw, seed)[0]
    return start, views, cam, targets


def textbook_fit(start, views, cam, targets, hw, rates, iters, betas, eps, degree=0):
    """gb.textbook_fit with harmonics of degrees 1 .. `degree` that start at zero and learn at rates["sh"]; all degrees from the start."""
    params = {k: torch.tensor(v.astype(D), requires_grad=True) for k, v in start.items()}
    if degree:
        params["sh"] = torch.zeros((len(start["xyz"]), terms(degree) - 1, 3), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([{"params": [p], "lr": float(rates[k])} for k, p in params.items()], betas=betas, eps=eps)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        rgb = textbook_render(params["xyz"], params["colour"], params.get("sh"), gb.covariance64(params["log_scale"], params["quat"]),
                              torch.sigmoid(params["opacity_logit"]), views, cam, hw)[0]
        loss = (rgb - targets).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


# ------------------------------------------------------------------------------------------------ shared cases
def seeded_case(degree, n=300, hw=(40, 56), seed=3):
    """The GPU tests' case: gr.seeded_scene's n Gaussians, V = 3 views and nmat = 2 with ids (every third Gaussian goes through the second
    matrix, the first turned and moved), some Gaussians behind the camera in view 1 only, colours of which some are negative enough to
    clamp, and seeded coefficients.  Returns xyz, colour, sh, cov, opacity, ids, mats (3, 2, 12), cam."""
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene(n, hw, seed)
    rng = np.random.default_rng(seed + 10)
    ids = (np.arange(n) % 3 == 2).astype(np.int32)
    table = np.zeros((3, 2, 12), F)
    base = np.concatenate([mats[0, 0].astype(D).reshape(3, 4), [[0, 0, 0, 1]]])
    for view, (angle, shift) in enumerate(((0.0, 0.0), (0.3, 0.4), (-0.25, -0.3))):
        c, s = np.cos(angle), np.sin(angle)
        turn = np.eye(4)
        turn[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        turn[0, 3] = shift
        obj = np.eye(4)
        obj[:3, :3] = [[np.cos(0.2), -np.sin(0.2), 0], [np.sin(0.2), np.cos(0.2), 0], [0, 0, 1]]
        obj[:3, 3] = (0.3, -0.2, 0.5)
        table[view, 0] = (turn @ base)[:3].reshape(12)
        table[view, 1] = (turn @ base @ obj)[:3].reshape(12)
    xyz = xyz.copy()
    behind = np.arange(n) % 17 == 5                                                  # the first 0.3 rad turn of view 1 puts these behind it
    xyz[behind, 0] = -30.0
    xyz[behind, 2] = F(1.0)
    colour = rng.uniform(-40.0, 255.0, (n, 3)).astype(F)
    sh = rng.uniform(-50.0, 50.0, (n, terms(degree) - 1, 3)).astype(F)
    return xyz.astype(F), colour, sh, cov, np.minimum(opacity, F(0.98)), ids, table, cam
