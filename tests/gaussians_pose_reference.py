"""The pose-gradient rule of DESIGN.md §28 on the CPU, written from the rule and not from the kernels, and what it approximates.

`pose_bwd` and `sh_pose_bwd` are the definition of the two entry points: numpy fp32, one rounded operation per numpy call in the order the
rule writes them, vectorised over the Gaussians, with the rule's order of the sum over the Gaussians of a (view, matrix): chunks of 256
through the tile's butterfly-and-waves order, then the chunk sums lane by lane and the same order once more.  `textbook_mats_grad` is the
truth they are measured against: gaussians_bwd_reference.textbook is differentiable in xyz and cov, so every view is fed the camera-space
positions R xyz + t and covariances R S R^T built in float64 torch from matrices that require a gradient, with an identity matrix in the
renderer's own slot.  `pose_fit_problem` and `textbook_pose_fit` are the registration the GPU fit is held to.  The product never imports
this module."""
import numpy as np
import torch

import gaussians_bwd_reference as gb
import gaussians_reference as gr
import gaussians_sh_reference as gs

F = np.float32
D = np.float64
CHUNK = 256
POSE_SUMS = 12
_LANES = np.arange(64)


# ------------------------------------------------------------------------------------------------ the order of the sum
def tile_sum(v):
    """(..., 256, N) fp32 -> (..., N): the xor butterfly over 1 .. 32 inside each wave of 64, then ((w0 + w1) + w2) + w3."""
    v = v.reshape(v.shape[:-2] + (4, 64, v.shape[-1]))
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[..., _LANES ^ s, :]
    return ((v[..., 0, 0, :] + v[..., 1, 0, :]) + v[..., 2, 0, :]) + v[..., 3, 0, :]


def chunk_sums(vals, mask):
    """vals (n, N) fp32, mask (n,) -> (C, N): per chunk of 256 consecutive Gaussians; a Gaussian outside the mask or past n adds +0.0."""
    n, N = vals.shape
    C = (n + CHUNK - 1) // CHUNK
    pad = np.zeros((C * CHUNK, N), F)
    pad[:n] = np.where(mask[:, None], vals, F(0.0))
    return tile_sum(pad.reshape(C, CHUNK, N))


def finish(chunks):
    """(C, N) chunk sums -> (N,): lane l adds chunks l, l + 256, ... in ascending order from +0.0; the 256 lane sums through tile_sum."""
    C, N = chunks.shape
    lanes = np.zeros((CHUNK, N), F)
    for first in range(0, C, CHUNK):
        part = chunks[first:first + CHUNK]
        lanes[:len(part)] = lanes[:len(part)] + part
    return tile_sum(lanes)


def sum_over_gaussians(vals, which, ok, nmat):
    """(n, N) per-Gaussian values -> (nmat, N): matrix o takes the Gaussians with which == o and ok."""
    with np.errstate(all="ignore"):
        return np.stack([finish(chunk_sums(vals, ok & (which == o))) for o in range(nmat)])


def gather(partial, count, offsets, columns):
    """The partials' `columns` of every Gaussian of one view added in ascending order from +0 -> (n, len(columns)) fp32 and which
    Gaussians count: count > 0 and the offset inside [0, E - count].  Vectorised over the Gaussians."""
    partial = np.asarray(partial, dtype=F)
    E = len(partial)
    cnt, off = np.asarray(count).astype(np.int64), np.asarray(offsets, dtype=np.int64)
    ok = (cnt > 0) & (off >= 0) & (off <= E - cnt)
    acc = np.zeros((len(cnt), len(columns)), F)
    with np.errstate(all="ignore"):
        for k in range(int(cnt[ok].max()) if ok.any() else 0):
            on = ok & (k < cnt)
            rows = partial[np.where(on, off + k, 0)][:, columns]
            acc = np.where(on[:, None], acc + rows, acc)
    return acc, ok


# ------------------------------------------------------------------------------------------------ the two entry points
def pose_bwd(xyz, cov, ids, mats, cam, hw, count, offsets, partial, znear=gr.ZNEAR, zfar=gr.ZFAR):
    """d_mats (V, nmat, 12) fp32: §24's chain quantities of every counted (view, Gaussian) and §28's twelve contributions, summed."""
    xyz, cov, mats = (np.asarray(a, dtype=F) for a in (xyz, cov, mats))
    fx, fy, cx, cy = (F(c) for c in cam)
    znear, zfar = F(znear), F(zfar)
    H, W = hw
    V, nmat = mats.shape[:2]
    n = len(xyz)
    which = gs._which(ids, n, nmat)
    p = [xyz[:, 0], xyz[:, 1], xyz[:, 2]]
    s = {(0, 0): cov[:, 0], (0, 1): cov[:, 1], (0, 2): cov[:, 2], (1, 1): cov[:, 3], (1, 2): cov[:, 4], (2, 2): cov[:, 5]}
    S = lambda r, k: s[(min(r, k), max(r, k))]
    limx = F(1.3) * (F(0.5) * F(W) / fx)
    limy = F(1.3) * (F(0.5) * F(H) / fy)
    two = F(2.0)
    out = np.zeros((V, nmat, POSE_SUMS), F)
    with np.errstate(all="ignore"):
        for view in range(V):
            m = mats[view][which]
            M = lambda k: m[:, k]
            row = lambda r: ((M(4 * r) * p[0] + M(4 * r + 1) * p[1]) + M(4 * r + 2) * p[2]) + M(4 * r + 3)
            xc, yc, zc = row(0), row(1), row(2)
            acc, ok = gather(partial, count[view], offsets[view], list(range(gb.SUMS)))
            ok = ok & (zc > znear) & (zc < zfar)
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
            g = np.zeros((n, POSE_SUMS), F)
            for k in range(3):                                              # §28
                g[:, k] = dxc * p[k] + dT0[k] * j00
                g[:, 4 + k] = dyc * p[k] + dT1[k] * j11
                g[:, 8 + k] = dzc * p[k] + (dT0[k] * j02 + dT1[k] * j12)
            g[:, 3], g[:, 7], g[:, 11] = dxc, dyc, dzc
            out[view] = sum_over_gaussians(g, which, ok, nmat)
    return out


def sh_pose_bwd(xyz, ids, mats, count, offsets, partial, colour, sh, active=None):
    """d_mats_dir (V, nmat, 12) fp32: what reaches the matrices through the direction of §27, summed as pose_bwd sums."""
    L = gs.degree_of(sh)
    K, Ka = gs.terms(L), gs.terms(L if active is None else active)
    xyz, mats, colour, sh = (np.asarray(a, dtype=F) for a in (xyz, mats, colour, sh))
    V, nmat = mats.shape[:2]
    n = len(xyz)
    which = gs._which(ids, n, nmat)
    out = np.zeros((V, nmat, POSE_SUMS), F)
    with np.errstate(all="ignore"):
        for view in range(V):
            m = mats[view][which]
            up, ok = gather(partial, count[view], offsets[view], [0, 1, 2])
            d, length = gs.directions(xyz, m, F)
            B = gs.basis(d, L, F)
            a = gs._sums(B, colour, sh, Ka)
            ge = np.where(a < 0, F(0), up)
            s = [np.zeros(n, F) for _ in range(K)]
            for k in range(1, Ka):
                s[k] = (ge[:, 0] * sh[:, k - 1, 0] + ge[:, 1] * sh[:, k - 1, 1]) + ge[:, 2] * sh[:, k - 1, 2]
            gd = gs.basis_gradient(d, s, L, F)
            dot = (d[:, 0] * gd[0] + d[:, 1] * gd[1]) + d[:, 2] * gd[2]
            dv = [(gd[j] - d[:, j] * dot) / length for j in range(3)]
            g = np.zeros((n, POSE_SUMS), F)
            for r in range(3):                                              # §28
                for k in range(3):
                    g[:, 4 * r + k] = dv[k] * m[:, 4 * r + 3]
                g[:, 4 * r + 3] = (dv[0] * m[:, 4 * r] + dv[1] * m[:, 4 * r + 1]) + dv[2] * m[:, 4 * r + 2]
            out[view] = sum_over_gaussians(g, which, ok, nmat)
    return out


def render_pose_backward(xyz, colour, cov, opacity, ids, mats, cam, hw, d_rgb, d_depth, d_alpha, sh=None, active=None):
    """The whole fp32 rule from the scene to d_mats: the forward and the blend's backward of §24 (§27 with sh), then the entry points above.
    Returns the chain's dict with "d_mats" (and with sh "d_mats_dir", already added to it)."""
    if sh is None:
        out = gb.render_backward(xyz, colour, cov, opacity, ids, mats, cam, hw, d_rgb, d_depth, d_alpha)
    else:
        out = gs.render_backward(xyz, colour, sh, cov, opacity, ids, mats, cam, hw, d_rgb, d_depth, d_alpha, active)
    out["d_mats"] = pose_bwd(xyz, cov, ids, mats, cam, hw, out["count"], out["offsets"], out["partial"])
    if sh is not None:
        out["d_mats_dir"] = sh_pose_bwd(xyz, ids, mats, out["count"], out["offsets"], out["partial"], colour, sh, active)
        out["d_mats"] = out["d_mats"] + out["d_mats_dir"]
    return out


# ------------------------------------------------------------------------------------------------ the float64 truth
EYE = np.array([[[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]]], dtype=D)


def _full(cov6):
    s = cov6
    return torch.stack([s[:, 0], s[:, 1], s[:, 2], s[:, 1], s[:, 3], s[:, 4], s[:, 2], s[:, 4], s[:, 5]], 1).reshape(-1, 3, 3)


def textbook_through(mats, xyz, colour, cov, opacity, cam, hw, ids=None, sh=None, active=None):
    """gb.textbook with matrices that may require a gradient: mats (V, nmat, 12) float64 torch; the rest float64 torch as gb.textbook takes
    them.  Per view every Gaussian is moved into the camera's frame by its own matrix (position R p + t, covariance R S R^T, with harmonics
    the colour at the direction from c = -R^T t) and drawn through the identity.  rgb (V, 3, H, W), depth (V, H, W), alpha (V, H, W)."""
    V, nmat = mats.shape[:2]
    n = xyz.shape[0]
    which = torch.zeros(n, dtype=torch.long) if ids is None else torch.as_tensor(np.asarray(ids)).long().clamp(0, nmat - 1)
    images = []
    for view in range(V):
        M = mats[view][which].reshape(n, 3, 4)
        R, t = M[:, :, :3], M[:, :, 3]
        pos = (R @ xyz[:, :, None])[:, :, 0] + t
        full = R @ _full(cov) @ R.transpose(1, 2)
        cov_c = torch.stack([full[:, 0, 0], full[:, 0, 1], full[:, 0, 2], full[:, 1, 1], full[:, 1, 2], full[:, 2, 2]], dim=1)
        cols = colour
        if sh is not None:
            L = gs.degree_of(sh)
            Ka = gs.terms(L if active is None else active)
            w = xyz + (R.transpose(1, 2) @ t[:, :, None])[:, :, 0]
            Bk = gs.textbook_basis(w / w.norm(dim=1, keepdim=True), L)
            cols = torch.clamp(colour + torch.einsum("nk,nkc->nc", Bk[:, 1:Ka], sh[:, :Ka - 1]), min=0.0)
        images.append(gb.textbook(pos, cols, cov_c, opacity, EYE, cam, hw))
    return tuple(torch.cat([i[k] for i in images]) for k in range(3))


def textbook_mats_grad(xyz, colour, cov, opacity, ids, mats, cam, hw, d_rgb, d_depth, d_alpha, sh=None, active=None):
    """float64 d_mats (V, nmat, 12) of sum(rgb d_rgb) + sum(depth d_depth) + sum(alpha d_alpha) by autograd through textbook_through."""
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=F).astype(D))
    m = t64(mats).requires_grad_(True)
    rgb, depth, alpha = textbook_through(m, t64(xyz), t64(colour), t64(cov), t64(opacity), cam, hw, ids, None if sh is None else t64(sh), active)
    loss = (rgb * t64(d_rgb)).sum() + (depth * t64(d_depth)).sum() + (alpha * t64(d_alpha)).sum()
    return torch.autograd.grad(loss, m)[0].numpy()


# ------------------------------------------------------------------------------------------------ shared cases
# The fp32 rule against textbook_mats_grad, relative to the largest |d_mats| of the case: measured with this file on the three cases below
# at their default seeds (2.9e-6, 2.4e-6, 1.4e-6) and at seeds 11 and 12 (up to 4.7e-6).  The bound is 4 x the largest value seen; the
# factor is headroom for other seeds.  The GPU is held bit-equal to the fp32 rule, so the bound is its bound too.
MEASURED_GAP = 4.7e-6
GAP_BOUND = 4 * MEASURED_GAP


def upstream(V, hw, seed=5):
    """Seeded d_rgb (V, 3, H, W), d_depth (V, H, W) and d_alpha (V, H, W) fp32."""
    rng = np.random.default_rng(seed)
    hw = tuple(hw)
    return (rng.normal(size=(V, 3) + hw).astype(F), (rng.normal(size=(V,) + hw) * 0.05).astype(F), rng.normal(size=(V,) + hw).astype(F))


def _case(xyz, colour, cov, opacity, ids, mats, cam, hw, sh=None):
    return dict(xyz=xyz, colour=np.asarray(colour, dtype=F), cov=cov, opacity=np.minimum(opacity, F(0.98)), ids=ids, mats=mats, cam=cam,
                hw=tuple(hw), sh=sh)


def case_scene(n=200, hw=(40, 56), seed=7):
    """gr.seeded_scene: one view, one matrix."""
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene(n, hw, seed)
    return _case(xyz, rgb, cov, opacity, None, mats, cam, hw)


def case_three(n=200, hw=(40, 56), seed=7):
    """gr.seeded_scene in two views with three matrices a view (the camera's, and two objects turned and moved) and interleaved ids i % 3."""
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene(n, hw, seed)
    ids = (np.arange(len(xyz)) % 3).astype(np.int32)
    base = np.concatenate([mats[0, 0].astype(D).reshape(3, 4), [[0, 0, 0, 1]]])
    table = np.zeros((2, 3, 12), F)
    for view, shift in enumerate((0.0, 0.3)):
        camera = base.copy()
        camera[0, 3] += shift
        for o, (angle, move) in enumerate(((0.0, (0.0, 0.0, 0.0)), (0.15, (0.2, -0.1, 0.3)), (-0.2, (-0.3, 0.1, -0.2)))):
            obj = np.eye(4)
            obj[:3, :3] = [[np.cos(angle), -np.sin(angle), 0], [np.sin(angle), np.cos(angle), 0], [0, 0, 1]]
            obj[:3, 3] = move
            table[view, o] = (camera @ obj)[:3].reshape(12)
    return _case(xyz, rgb, cov, opacity, ids, table, cam, hw)


def case_sh(degree=2, n=200, hw=(40, 56), seed=3):
    """gs.seeded_case: three views, two matrices, harmonics of `degree`, colours that clamp, Gaussians behind one camera."""
    xyz, colour, sh, cov, opacity, ids, table, cam = gs.seeded_case(degree, n, hw, seed)
    return _case(xyz, colour, cov, opacity, ids, table, cam, hw, sh)


def case_backward(case, active=None):
    """render_pose_backward of a case with upstream(V, hw)."""
    return render_pose_backward(case["xyz"], case["colour"], case["cov"], case["opacity"], case["ids"], case["mats"], case["cam"], case["hw"],
                                *upstream(case["mats"].shape[0], case["hw"]), sh=case["sh"], active=active)


def case_truth(case, active=None):
    return textbook_mats_grad(case["xyz"], case["colour"], case["cov"], case["opacity"], case["ids"], case["mats"], case["cam"], case["hw"],
                              *upstream(case["mats"].shape[0], case["hw"]), sh=case["sh"], active=active)


# ------------------------------------------------------------------------------------------------ poses in float64
def exp_twist(twist):
    """(V, 6) float64 torch (omega, tau) -> (V, 4, 4): [exp([omega]x) | tau], the rotation by torch.linalg.matrix_exp."""
    x, y, z = twist[:, 0], twist[:, 1], twist[:, 2]
    zero = torch.zeros_like(x)
    k = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], dim=1).reshape(-1, 3, 3)
    top = torch.cat([torch.linalg.matrix_exp(k), twist[:, 3:, None]], dim=2)
    last = torch.tensor([[[0.0, 0.0, 0.0, 1.0]]], dtype=twist.dtype).expand(twist.shape[0], 1, 4)
    return torch.cat([top, last], dim=1)


def apply_twist(twist, mats):
    """[R(omega_v) | tau_v] o mats[v][o] for mats (V, nmat, 12) float64 torch."""
    V, nmat = mats.shape[:2]
    m = mats.reshape(V, nmat, 3, 4)
    c = exp_twist(twist)[:, None]
    return torch.cat([c[..., :3, :3] @ m[..., :3], c[..., :3, :3] @ m[..., 3:] + c[..., :3, 3:]], dim=-1).reshape(V, nmat, 12)


def pose_error(estimate, truth):
    """(3, 4) or (12,) world-to-camera matrices -> (the distance between the camera centres in metres, the angle between the rotations in
    radians), float64."""
    e, t = np.asarray(estimate, dtype=D).reshape(3, 4), np.asarray(truth, dtype=D).reshape(3, 4)
    centre = lambda m: -m[:, :3].T @ m[:, 3]
    d = e[:, :3] @ t[:, :3].T
    sin = 0.5 * np.linalg.norm([d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]])     # small angles: the sine resolves them
    return float(np.linalg.norm(centre(e) - centre(t))), float(np.arctan2(sin, (np.trace(d) - 1.0) / 2.0))


# ------------------------------------------------------------------------------------------------ pose-only registration
POSE_FIT_HW = (24, 40)
POSE_FIT_ITERS = 80
POSE_FIT_RATE = 1e-3
POSE_FIT_TWISTS = ((0.0,) * 6, (0.004, -0.01, 0.006, 0.05, -0.03, 0.04), (-0.006, 0.008, 0.003, -0.04, 0.02, -0.05))
# textbook_pose_fit(pose_fit_problem()): the last loss over the first, measured with this file's code
R64 = 0.0132


def pose_fit_problem(n=120, hw=POSE_FIT_HW, seed=7):
    """gr.seeded_scene seen from gb.fit_problem's three cameras; the targets (3, 3, H, W) float64 are drawn by gb.textbook at the true
    cameras and the Gaussians stay at the truth.  Views 1 and 2 are handed over with POSE_FIT_TWISTS applied on the left (about 12 mrad
    and 7 cm off), rounded to fp32; view 0 is exact.  Returns the scene (xyz, rgb, cov, opacity as fp32 arrays), the true matrices
    (3, 1, 12) fp32, the perturbed ones (3, 1, 12) fp32, the camera and the targets."""
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene(n, hw, seed)
    truth = np.repeat(mats, 3, axis=0).copy()
    truth[1, 0, 3] += F(0.3)
    truth[2, 0, 3] -= F(0.3)
    opacity = np.minimum(opacity, F(0.98))
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=F).astype(D))
    with torch.no_grad():
        targets = gb.textbook(t64(xyz), t64(rgb), t64(cov), t64(opacity), truth, cam, hw)[0]
        start = apply_twist(torch.tensor(POSE_FIT_TWISTS, dtype=torch.float64), t64(truth)).numpy().astype(F)
    return (xyz, rgb.astype(F), cov, opacity), truth, start, cam, targets


def textbook_pose_fit(problem, iters=POSE_FIT_ITERS, rate=POSE_FIT_RATE, betas=(0.9, 0.999), eps=1e-15, fixed=(0,)):
    """torch.optim.Adam on a float64 twist (V, 6) from zero, the views in `fixed` masked to the identity, the loss the mean absolute rgb
    difference of textbook_through.  Returns the loss of every step and the corrected matrices (V, 1, 12) float64."""
    (xyz, rgb, cov, opacity), truth, start, cam, targets = problem
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=F).astype(D))
    scene = tuple(t64(a) for a in (xyz, rgb, cov, opacity))
    twist = torch.zeros((len(start), 6), dtype=torch.float64, requires_grad=True)
    free = torch.ones((len(start), 1), dtype=torch.float64)
    free[list(fixed)] = 0.0
    opt = torch.optim.Adam([twist], lr=rate, betas=betas, eps=eps)
    hw = tuple(targets.shape[2:])
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        loss = (textbook_through(apply_twist(twist * free, t64(start)), *scene, cam, hw)[0] - targets).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        final = apply_twist(twist * free, t64(start)).numpy()
    return losses, final
