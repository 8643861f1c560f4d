"""The reference of DESIGN.md §27 (tests/gaussians_sh_reference.py) checked on the CPU before anything trusts it: the basis is
orthonormal, the float64 definition agrees with autograd of a textbook evaluation, the fp32 definition lies within a measured distance of
the float64 one, the clamp and the active degree cut what they should, the density rule moves coefficient rows as it moves colours, and
the float64 fit gains from harmonics what the GPU test holds the product to.  The host-side refusals of the new interface are here too."""
import os

import numpy as np
import pytest
import torch

import gaussians_reference as gr
import gaussians_sh_reference as gs

F, D = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (40, 56)
# The largest distance between the fp32 and the float64 definition over gs.seeded_case(L), L = 1, 2, 3, relative to the largest float64
# magnitude of the quantity, measured on the CPU.  The asserted tolerance is four times the measured value, §24's margin.
MEASURED = {"colours": 2.2e-7, "d_colour": 6.7e-8, "d_sh": 1.9e-7, "d_xyz_dir": 1.6e-7}
# The float64 fits of gs.fit_problem(): final loss after gs.FIT_ITERS Adam steps with L = 0 and with L = 2, and their ratio, measured on
# the CPU.
LOSS0_64, LOSS2_64 = 0.00265, 0.00084
RATIO64 = 0.318


def _t64(a):
    return torch.tensor(np.asarray(a, dtype=F).astype(D), requires_grad=True)


def _rel(a, b):
    return float(np.abs(np.asarray(a, dtype=D) - np.asarray(b, dtype=D)).max() / np.abs(np.asarray(b, dtype=D)).max())


def _case(L):
    xyz, colour, sh, cov, op, ids, mats, cam = gs.seeded_case(L)
    count = gr.project(xyz, cov, op, ids, mats, cam, HW)["count"]
    return xyz, colour, sh, ids, mats, count


# ------------------------------------------------------------------------------------------------ the basis
def test_the_sixteen_basis_functions_are_orthonormal_on_the_sphere():
    # Gauss-Legendre with 8 nodes in cos(theta) is exact to degree 15, a uniform grid of 16 in phi to frequency 15: products have degree 6
    nodes, weights = np.polynomial.legendre.leggauss(8)
    phi = (np.arange(16) + 0.5) * (2 * np.pi / 16)
    ct, ph = np.meshgrid(nodes, phi, indexing="ij")
    st = np.sqrt(1 - ct * ct)
    d = np.stack([st * np.cos(ph), st * np.sin(ph), ct], axis=-1).reshape(-1, 3)
    w = (weights[:, None] * np.full((1, 16), 2 * np.pi / 16)).reshape(-1)
    B = np.stack(gs.basis(d, 3, D), axis=1)
    assert B.shape == (128, 16)
    gram = B.T @ (B * w[:, None])
    assert np.abs(gram - np.eye(16)).max() < 1e-12, np.abs(gram - np.eye(16)).max()


def test_the_constants_are_the_ones_the_kernels_round():
    src = open(os.path.join(ROOT, "mudg_amd", "csrc", "gaussians_sh.hip")).read()
    for c in (gs.C1,) + gs.C2 + gs.C3:
        assert repr(abs(c)) + "f" in src, c
    from mudg_amd import ops
    assert ops.GAUSS_SH_MAX_DEGREE == gs.MAX_DEGREE and [ops.gauss_sh_rows(d) for d in (1, 2, 3)] == [gs.terms(d) - 1 for d in (1, 2, 3)]


# ------------------------------------------------------------------------------------------------ float64 against autograd, fp32 against float64
@pytest.mark.parametrize("L", [1, 2, 3])
def test_the_float64_definition_matches_autograd_and_the_fp32_one_lies_within_the_measured_gap(L):
    xyz, colour, sh, ids, mats, count = _case(L)
    ok = count > 0
    assert ok.any() and not ok.all()
    X, C, S = _t64(xyz), _t64(colour), _t64(sh)
    book = gs.textbook_colours(X, C, S, mats, ids)
    g = np.random.default_rng(L).normal(size=book.shape)
    (book * torch.tensor(g * ok[:, :, None])).sum().backward()
    c64 = gs.colours(xyz, ids, mats, count, colour, sh, dtype=D)
    assert (c64[ok] == 0).any() and (c64[ok] > 0).any()                                # some colours are clamped, most are not
    grads64 = gs.colours_backward(xyz, ids, mats, ok, g, colour, sh, dtype=D)
    gaps = {"colours": _rel(c64, np.where(ok[:, :, None], book.detach().numpy(), 0.0))}
    for name, mine, theirs in zip(("d_colour", "d_sh", "d_xyz_dir"), grads64, (C.grad, S.grad, X.grad)):
        gaps[name] = _rel(mine, theirs.numpy())
    print(f"L = {L}: float64 definition against autograd {gaps}")
    assert max(gaps.values()) < 1e-10, gaps
    c32 = gs.colours(xyz, ids, mats, count, colour, sh)
    grads32 = gs.colours_backward(xyz, ids, mats, ok, g.astype(F), colour, sh)
    assert c32.dtype == F and all(a.dtype == F for a in grads32)
    grads64 = gs.colours_backward(xyz, ids, mats, ok, g.astype(F), colour, sh, dtype=D)
    gaps = {"colours": _rel(c32, c64), **{k: _rel(a, b) for k, a, b in zip(("d_colour", "d_sh", "d_xyz_dir"), grads32, grads64)}}
    print(f"L = {L}: fp32 against float64 {gaps} (recorded {MEASURED})")
    for k, v in gaps.items():
        assert v <= 4 * MEASURED[k], (k, v)


# ------------------------------------------------------------------------------------------------ the clamp and the active degree
def test_a_colour_clamped_in_one_view_gets_nothing_from_that_view():
    # one Gaussian at the origin, three cameras on the x axis, the y axis and the -x axis looking at it: B_3 = -C1 dx is -C1, 0 and +C1
    look = lambda right, up, fwd, pos: np.concatenate([np.stack([right, up, fwd]), -np.stack([right, up, fwd]) @ np.asarray(pos, D)[:, None]], axis=1)
    ex, ey, ez = np.eye(3)
    mats = np.stack([look(ey, ez, -ex, (5, 0, 0)), look(-ex, ez, -ey, (0, 5, 0)), look(-ey, ez, ex, (-5, 0, 0))]).reshape(3, 1, 12).astype(F)
    xyz, colour = np.zeros((1, 3), F), np.full((1, 3), 10.0, F)
    sh = np.zeros((1, 3, 3), F)
    sh[0, 2] = 100.0                                                                   # the coefficient of B_3
    count = np.ones((3, 1), np.int32)
    d = np.stack([gs.directions(xyz, mats[v], D)[0][0] for v in range(3)])
    assert np.allclose(d, [[-1, 0, 0], [0, -1, 0], [1, 0, 0]], atol=1e-7)
    cols = gs.colours(xyz, None, mats, count, colour, sh)
    assert (cols[2] == 0).all() and not np.signbit(cols[2]).any() and (cols[0] > 50).all() and (cols[1] == 10).all()
    g = np.ones((3, 1, 3), F)
    ok = count > 0
    per_view = [gs.colours_backward(xyz, None, mats[v:v + 1], ok[v:v + 1], g[v:v + 1], colour, sh) for v in range(3)]
    for a in per_view[2]:
        assert not a.any()                                                             # the clamped view: zero for colour, sh and xyz
    for v in (0, 1):
        assert (per_view[v][0] == 1).all() and per_view[v][1].any()
    # B_3's gradient points along x: radial in view 0, where the normalisation removes it, and tangential in view 1
    assert not per_view[0][2].any() and per_view[1][2][0, 0] != 0 and not per_view[1][2][0, 1:].any()
    total = gs.colours_backward(xyz, None, mats, ok, g, colour, sh)
    assert (total[0] == 2).all()
    for k in range(3):
        assert np.array_equal(total[k], per_view[0][k] + per_view[1][k])


@pytest.mark.parametrize("L,active", [(3, 1), (3, 0), (2, 1), (3, 2)])
def test_coefficients_above_the_active_degree_take_no_part_and_get_exactly_zero(L, active):
    xyz, colour, sh, ids, mats, count = _case(L)
    ok = count > 0
    Ka = gs.terms(active)
    cut = gs.colours(xyz, ids, mats, count, colour, sh, active)
    g = np.random.default_rng(5).normal(size=cut.shape).astype(F)
    d_colour, d_sh, d_xyz = gs.colours_backward(xyz, ids, mats, ok, g, colour, sh, active)
    assert not d_sh[:, Ka - 1:].any() and not np.signbit(d_sh[:, Ka - 1:]).any()
    if active == 0:
        lit = ok[:, :, None] & np.ones(3, bool)
        assert np.array_equal(cut[lit], np.where(colour < 0, F(0), colour)[None].repeat(3, axis=0)[lit]) and not d_xyz.any()
        return
    low = np.ascontiguousarray(sh[:, :Ka - 1])                                         # the same sums with coefficients of degree `active` only
    assert np.array_equal(cut, gs.colours(xyz, ids, mats, count, colour, low))
    want = gs.colours_backward(xyz, ids, mats, ok, g, colour, low)
    assert np.array_equal(d_colour, want[0]) and np.array_equal(d_sh[:, :Ka - 1], want[1]) and d_sh[:, :Ka - 1].any()
    assert np.array_equal(d_xyz, want[2]) and d_xyz.any()


# ------------------------------------------------------------------------------------------------ density control
def test_the_density_rule_moves_coefficient_rows_and_moments_as_it_moves_colours():
    from mudg_amd import gaussians, ops
    action = torch.tensor([ops.GAUSS_KEEP, ops.GAUSS_PRUNE, ops.GAUSS_CLONE, ops.GAUSS_SPLIT, ops.GAUSS_KEEP], dtype=torch.int32)
    rows = torch.tensor([1, 0, 2, 2, 1], dtype=torch.int32)
    sh = torch.arange(5 * 3 * 3, dtype=torch.float32).reshape(5, 3, 3) + 1
    m, v = sh * 10, sh * 100
    got, got_m, got_v = gaussians.density_rows(action, rows, sh, m, v)
    z = torch.zeros(3, 3)
    want = [sh[0], sh[2], sh[2], sh[3], sh[3], sh[4]]                                  # survivors in order, children adjacent
    want_m = [m[0], m[2], z, z, z, m[4]]                                               # kept: moments; clone: moments, then zeros; split: zeros twice
    want_v = [v[0], v[2], z, z, z, v[4]]
    assert torch.equal(got, torch.stack(want)) and torch.equal(got_m, torch.stack(want_m)) and torch.equal(got_v, torch.stack(want_v))
    one = gaussians.density_rows(action, rows, sh[:, 0, 0].contiguous(), m[:, 0, 0].contiguous(), v[:, 0, 0].contiguous())
    assert torch.equal(one[0], got[:, 0, 0]) and torch.equal(one[1], got_m[:, 0, 0])   # any per-Gaussian shape


# ------------------------------------------------------------------------------------------------ the fit, in float64
def test_the_float64_fit_of_a_view_dependent_target_gains_from_harmonics():
    from mudg_amd import gaussians
    start, views, cam, targets = gs.fit_problem()
    rates, betas, eps = gaussians.LEARNING_RATES, gaussians.ADAM_BETAS, gaussians.ADAM_EPS
    assert rates["sh"] == rates["colour"] / 20 and gaussians.PARAMETERS == ("xyz", "colour", "log_scale", "quat", "opacity_logit")
    flat = gs.textbook_fit(start, views, cam, targets, gs.FIT_HW, rates, gs.FIT_ITERS, betas, eps, degree=0)
    lit = gs.textbook_fit(start, views, cam, targets, gs.FIT_HW, rates, gs.FIT_ITERS, betas, eps, degree=2)
    ratio = lit[-1] / flat[-1]
    print(f"float64 fits, {gs.FIT_ITERS} steps from {flat[0]:.5f}: L = 0 ends at {flat[-1]:.5f}, L = 2 at {lit[-1]:.5f}, ratio {ratio:.4f} "
          f"(recorded {LOSS0_64}, {LOSS2_64}, {RATIO64})")
    assert flat[0] == lit[0]                                                           # zero coefficients: the same first image
    assert abs(flat[-1] / LOSS0_64 - 1) < 0.02 and abs(lit[-1] / LOSS2_64 - 1) < 0.02 and abs(ratio / RATIO64 - 1) < 0.02


# ------------------------------------------------------------------------------------------------ the host side
def test_the_interface_refuses_what_is_not_on_the_gpu_or_has_no_degree():
    from mudg_amd import gaussians, hip, ops
    from mudg_amd.render import PointCloud
    n = 4
    f = lambda *s: torch.zeros(s, dtype=torch.float32)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        ops.gauss_sh_colour(torch.zeros((n, 4), dtype=torch.int32), f(1, 1, 12), torch.zeros((1, n), dtype=torch.int32), f(n, 3), f(n, 3, 3))
    with pytest.raises(hip.MudgError, match="on the GPU"):
        ops.gauss_blend_views(f(1, n, 3), f(1, n, 2), f(1, n, 4), f(1, n), torch.zeros(3, dtype=torch.int32), torch.zeros((1, 2), dtype=torch.int32), (16, 16))
    with pytest.raises(hip.MudgError, match="on the GPU"):
        gaussians.render_differentiable(f(n, 3), f(n, 3), f(n, 6), f(n), f(1, 1, 12), (1.0, 1.0, 0.0, 0.0), (16, 16), sh=f(n, 3, 3))
    with pytest.raises(hip.MudgError, match="K = 4, 9 or 16"):
        gaussians._sh_rows_of("x", f(n, 5, 3))
    assert [gaussians._sh_rows_of("x", f(n, r, 3)) for r in (3, 8, 15)] == [3, 8, 15]
    assert set(gaussians.LEARNING_RATES) == set(gaussians.PARAMETERS) | {"sh"}
    import inspect
    from virtual_render import virtual_pose_render
    for fn, names in ((gaussians.fit, ("sh_degree", "sh_raise_every")), (gaussians.render_differentiable, ("sh", "sh_degree"))):
        params = inspect.signature(fn).parameters
        assert all(k in params for k in names), fn
    assert inspect.signature(gaussians.fit).parameters["sh_degree"].default == 0
    assert "sh_degree" in virtual_pose_render.fit_cloud_views.__doc__
