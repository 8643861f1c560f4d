"""Density control for the Gaussian fit on the GPU (csrc/gaussians_density.hip through mudg_amd/ops.py and gaussians.py) against the CPU
definition of the rule (tests/gaussians_density_reference.py): torch.equal for the statistics, the plan and all fifteen rewritten tensors
— both sides perform the same correctly rounded fp32 operations in the same order, so there is no tolerance — and the fit with density
control against its float64 counterpart."""
import numpy as np
import pytest
import torch

import gaussians_bwd_reference as gb
import gaussians_density_reference as gd
from helpers import rel_l2
from sentinel_buffers import Flat
from test_gaussians_bwd_gpu import _direct, _inputs, _model, _t
from test_gaussians_density_cpu import HOLED_CONTROL, HW, R_DENSE64, _control, toy
from test_gaussians_gpu import _scene_case

pytestmark = pytest.mark.gpu
F = np.float32
THRESHOLDS = dict(grad_threshold=2e-4, split_scale=0.2, min_opacity=0.005, max_scale=0.55)
WIDTHS = (3, 3, 3, 4, 1)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ the statistics
def _accumulate(cuda, partial, count, offsets, hw, grad_sum, seen):
    """ops.gauss_density_accumulate twice from the same state (a repeat must give the same bits), and the definition."""
    from mudg_amd import ops
    runs = []
    for _ in range(2):
        g, s = _t(grad_sum).to(cuda), _t(seen).to(cuda)
        ops.gauss_density_accumulate(partial, count, offsets, hw, g, s)
        runs.append((g, s))
    assert _bits(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "a repeat run differs"
    want = gd.accumulate(partial.cpu().numpy(), count.cpu().numpy(), offsets.cpu().numpy(), hw, grad_sum, seen)
    g, s = runs[0]
    assert g.dtype == torch.float32 and s.dtype == torch.int32
    assert _bits(g.cpu(), _t(want[0])) and torch.equal(s.cpu(), _t(want[1]))
    return want


@pytest.mark.parametrize("hw,views", [((17, 33), 1), ((40, 56), 1), ((40, 56), 3)])
def test_statistics_of_a_real_backward(cuda, hw, views):
    case = _scene_case(200, hw, 13, views=views)
    xyz, colour, up = _inputs(case)
    got, mid = _direct(cuda, case, colour, up)
    rng = np.random.default_rng(1)
    grad_sum, seen = _accumulate(cuda, got["partial"], mid["count"], mid["offsets"], hw, np.zeros(200, F), np.zeros(200, np.int32))
    assert grad_sum.any() and np.isfinite(grad_sum).all() and seen.max() == views
    assert np.array_equal(seen, (mid["count"].cpu().numpy() > 0).sum(axis=0))
    if views == 3:
        assert (seen < 3).any() and len(set(seen.tolist())) > 1              # dropped in one view and drawn in another: counted less often
    _accumulate(cuda, got["partial"], mid["count"], mid["offsets"], hw, rng.uniform(0, 5, 200).astype(F), rng.integers(0, 9, 200).astype(np.int32))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_statistics_at_the_block_edges_with_spoiled_offsets(cuda, n):
    rng = np.random.default_rng(n)
    count = rng.integers(0, 4, (2, n)).astype(np.int32)
    count[0, 0] = 2
    ends = np.cumsum(count.reshape(-1).astype(np.int64))
    E = int(ends[-1])
    offsets = (ends - count.reshape(-1)).reshape(2, n)
    partial = rng.normal(size=(E, 10)).astype(F)
    clean = gd.accumulate(partial, count, offsets, (40, 56), np.zeros(n, F), np.zeros(n, np.int32))
    offsets[0, ::3], offsets[1, 1::4], offsets[1, -1] = -1, E, E - int(count[1, -1]) + 1          # before 0, past the end, one row too far
    count[1, ::5] = -2
    d = lambda a: _t(a).to(cuda)
    grad_sum, seen = _accumulate(cuda, d(partial), d(count), d(offsets), (40, 56), np.zeros(n, F), np.zeros(n, np.int32))
    assert seen[0] == 0 and clean[1][0] >= 1 and seen.sum() < clean[1].sum()         # Gaussian 0: offset -1 in view 0, count -2 in view 1


# ------------------------------------------------------------------------------------------------ plan and apply
def _plan_apply(cuda, n, seed, ids, mix="mixed"):
    """ops.gauss_density_plan and gauss_density_apply, each twice, against the definition.  Returns the definition's action."""
    from mudg_amd import ops
    control = _control()
    rng = np.random.default_rng(seed)
    params, moments = toy(n, seed)
    opacity = rng.uniform(0.0, 1.0, n).astype(F)
    grad_sum, seen = rng.uniform(0, 1e-3, n).astype(F), rng.integers(0, 4, n).astype(np.int32)
    if mix == "keep":
        opacity[:], grad_sum[:] = 0.5, 0.0
        params["log_scale"] = np.minimum(params["log_scale"], F(np.log(0.5)))
    elif mix == "one left":
        opacity[:] = 0.001
        opacity[n // 2], params["log_scale"][n // 2] = 0.5, np.log(F(0.1))
    else:
        params["log_scale"][1::4] = np.log(rng.uniform(0.02, 0.15, params["log_scale"][1::4].shape)).astype(F)       # small enough to clone
        params["log_scale"][0] = np.log(F(0.3))
        opacity[0] = 0.5
        if n > 7:
            opacity[6::7] = 0.004                                            # below min_opacity
            opacity[3], grad_sum[2] = np.nan, np.nan
    scale = np.exp(params["log_scale"])
    rot = gd.rotation(params["quat"])
    ids_np = None if not ids else (np.arange(n, dtype=np.int32) * 7) % 5
    d = lambda a: None if a is None else _t(np.ascontiguousarray(a)).to(cuda)
    w_action, w_rows = gd.plan(grad_sum, seen, opacity, scale, **THRESHOLDS)
    plans = [ops.gauss_density_plan(d(grad_sum), d(seen), d(opacity), d(scale), **THRESHOLDS) for _ in range(2)]
    for action, rows in plans:
        assert action.dtype == torch.int32 and torch.equal(action.cpu(), _t(w_action)) and torch.equal(rows.cpu(), _t(w_rows))
    frozen = ops.gauss_density_plan(d(grad_sum), d(seen), d(opacity), d(scale), grow=False, **THRESHOLDS)[0].cpu().numpy()
    assert np.array_equal(frozen, gd.plan(grad_sum, seen, opacity, scale, grow=False, **THRESHOLDS)[0]) and frozen.max() <= gd.PRUNE
    total = int(w_rows.sum())
    if total == 0:
        return w_action
    start = np.cumsum(w_rows.astype(np.int64)) - w_rows
    tensors = []
    for k in gd.PARAMETERS:
        tensors += [params[k], *moments[k]]
    want, want_ids = gd.apply(w_action, start, total, scale, rot, tensors, control.split_offset, control.log_shrink, ids_np)
    runs = [ops.gauss_density_apply(plans[0][0], d(start), total, d(scale), d(rot.astype(F)), [d(t) for t in tensors],
                                    split_offset=control.split_offset, log_shrink=control.log_shrink, ids=d(ids_np)) for _ in range(2)]
    for outs, ids_out in runs:
        for k, (got, w) in enumerate(zip(outs, want)):
            assert _bits(got.cpu(), _t(w)), (n, mix, k)
        assert (ids_out is None) == (ids_np is None) and (ids_np is None or torch.equal(ids_out.cpu(), _t(want_ids)))
    return w_action


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("ids", [False, True])
def test_plan_and_apply_at_the_block_edges(cuda, n, ids):
    action = _plan_apply(cuda, n, 40 + n, ids)
    if n >= 255:
        assert set(action.tolist()) == {gd.KEEP, gd.PRUNE, gd.CLONE, gd.SPLIT}


def test_all_keep_and_all_but_one_pruned(cuda):
    assert set(_plan_apply(cuda, 300, 5, True, "keep").tolist()) == {gd.KEEP}
    action = _plan_apply(cuda, 300, 6, True, "one left")
    assert (action == gd.PRUNE).sum() == 299 and action[150] != gd.PRUNE


def test_no_entry_point_writes_outside_its_outputs_or_follows_an_unchecked_value(cuda):
    from mudg_amd import hip
    import ctypes
    lib = hip.lib()
    n = 300
    control = _control()
    rng = np.random.default_rng(8)
    params, moments = toy(n, 8)
    scale, rot = np.exp(params["log_scale"]), gd.rotation(params["quat"]).astype(F)
    opacity = rng.uniform(0.0, 1.0, n).astype(F)
    grad_sum0, seen0 = rng.uniform(0, 1e-3, n).astype(F), rng.integers(0, 4, n).astype(np.int32)
    d = lambda a: _t(np.ascontiguousarray(a)).to(cuda)
    # accumulate: grad_sum and seen inside sentinels
    count = rng.integers(0, 3, (2, n)).astype(np.int32)
    ends = np.cumsum(count.reshape(-1).astype(np.int64))
    E, offsets = int(ends[-1]), (ends - count.reshape(-1)).reshape(2, n)
    offsets[0, ::9] = E
    partial = rng.normal(size=(E, 10)).astype(F)
    g_buf, s_buf = Flat(n, torch.float32).put(_t(grad_sum0), cuda), Flat(n, torch.int32).put(_t(seen0), cuda)
    d_partial, d_count, d_offsets = d(partial), d(count), d(offsets)
    hip.check(lib.mudg_gauss_density_accumulate(d_partial.data_ptr(), d_count.data_ptr(), d_offsets.data_ptr(), n, 2, 40, 56, E, g_buf.ptr, s_buf.ptr,
                                                None), "accumulate")
    torch.cuda.synchronize()
    w_sum, w_seen = gd.accumulate(partial, count, offsets, (40, 56), grad_sum0, seen0)
    assert _bits(g_buf.read("grad_sum"), _t(w_sum)) and torch.equal(s_buf.read("seen"), _t(w_seen))
    # plan: action and rows inside sentinels
    a_buf, r_buf = Flat(n, torch.int32).blank(cuda), Flat(n, torch.int32).blank(cuda)
    ins = [d(w_sum), d(w_seen), d(opacity), d(scale)]
    hip.check(lib.mudg_gauss_density_plan(*[t.data_ptr() for t in ins], n, *[THRESHOLDS[k] for k in ("grad_threshold", "split_scale", "min_opacity",
                                                                                                   "max_scale")], 1, a_buf.ptr, r_buf.ptr, None), "plan")
    torch.cuda.synchronize()
    w_action, w_rows = gd.plan(w_sum, w_seen, opacity, scale, **THRESHOLDS)
    assert torch.equal(a_buf.read("action"), _t(w_action)) and torch.equal(r_buf.read("rows"), _t(w_rows))
    # apply: action codes that are none of the four, starts outside [0, n' - rows]; rows nobody writes keep the sentinel
    total = int(w_rows.sum())
    start = np.cumsum(w_rows.astype(np.int64)) - w_rows
    action = w_action.copy()
    action[::11], action[5::13] = 4, -1
    start[3::10], start[7::17], start[-1] = -1, total, total - 1 if action[-1] in (gd.CLONE, gd.SPLIT) else total
    tensors = []
    for k in gd.PARAMETERS:
        tensors += [params[k], *moments[k]]
    ids = (np.arange(n, dtype=np.int32) * 3) % 4
    sizes = [total * WIDTHS[k // 3] for k in range(15)]
    outs = [Flat(s, torch.float32).blank(cuda) for s in sizes]
    ids_out = Flat(total, torch.int32).blank(cuda)
    fill = [o.view(o.cpu).clone().numpy().reshape((total, -1) if WIDTHS[k // 3] > 1 else (total,)) for k, o in enumerate(outs)]
    fill.append(ids_out.view(ids_out.cpu).clone().numpy())
    want, want_ids = gd.apply(action, start, total, scale, rot, tensors, control.split_offset, control.log_shrink, ids, fill=fill)
    d_in = [d(t) for t in tensors]
    table = ctypes.c_void_p * 15
    d_action, d_start, d_scale, d_rot, d_ids = d(action), d(start), d(scale), d(rot), d(ids)
    hip.check(lib.mudg_gauss_density_apply(d_action.data_ptr(), d_start.data_ptr(), n, total, d_scale.data_ptr(), d_rot.data_ptr(),
                                           control.split_offset, control.log_shrink, table(*[t.data_ptr() for t in d_in]), table(*[o.ptr for o in outs]),
                                           d_ids.data_ptr(), ids_out.ptr, None), "apply")
    torch.cuda.synchronize()
    for k, (o, w) in enumerate(zip(outs, want)):
        assert _bits(o.read(f"tensor {k}"), _t(w).reshape(-1)), k
    assert torch.equal(ids_out.read("ids"), _t(want_ids))
    untouched = np.ones(total, bool)
    for g in range(n):
        c = {gd.KEEP: 1, gd.CLONE: 2, gd.SPLIT: 2}.get(int(action[g]), 0)
        if c and 0 <= start[g] <= total - c:
            untouched[start[g]:start[g] + c] = False
    assert untouched.any() and not untouched.all()                           # the spoiled values did leave rows unwritten


# ------------------------------------------------------------------------------------------------ the autograd Function and the fit
def test_backward_with_statistics_equals_the_direct_call_and_changes_no_gradient(cuda):
    from mudg_amd import gaussians
    case = _scene_case(200, (40, 56), 13, views=3)
    pts, cov, op, ids, mats, cam, hw = case
    xyz, colour, up = _inputs(case)
    d_mats, d_up = _t(mats).to(cuda), [_t(u).to(cuda) for u in up]
    grads = {}
    for density in (None, gaussians.DensityStats(200, cuda)):
        leaves = [_t(a).to(cuda).requires_grad_(True) for a in (xyz, colour, cov, op)]
        out = gaussians.render_differentiable(*leaves, d_mats, cam, hw, density=density)
        torch.autograd.backward(out, d_up)
        grads[density is None] = [leaf.grad for leaf in leaves] + list(out)
    for a, b in zip(grads[True], grads[False]):
        assert _bits(a.detach(), b.detach())
    got, mid = _direct(cuda, case, colour, up)
    want = gd.accumulate(got["partial"].cpu().numpy(), mid["count"].cpu().numpy(), mid["offsets"].cpu().numpy(), hw, np.zeros(200, F), np.zeros(200, np.int32))
    assert _bits(density.grad_sum.cpu(), _t(want[0])) and torch.equal(density.seen.cpu(), _t(want[1])) and want[1].any()
    density.reset()
    assert len(density) == 200 and not density.grad_sum.any() and not density.seen.any()
    with pytest.raises(gaussians.hip.MudgError, match="DensityStats"):
        gaussians.render_differentiable(*leaves, d_mats, cam, hw, density=gaussians.DensityStats(199, cuda))


def _problem(cuda):
    start, views, cam, targets = gb.fit_problem()
    return start, views, cam, _t(views).to(cuda), targets.to(torch.float32).to(cuda)


def test_a_fit_whose_window_is_empty_is_the_fit_without_density_control(cuda):
    from mudg_amd import gaussians
    start, views, cam, mats, tgt = _problem(cuda)
    plain, empty = _model(cuda, start), _model(cuda, start)
    control = gaussians.DensityControl(3, 3, 1, split_scale=0.2, max_scale=2.0, reset_every=1)
    a = gaussians.fit(plain, tgt, mats, cam, HW, iters=6)
    b = gaussians.fit(empty, tgt, mats, cam, HW, iters=6, density=control)
    assert a == b and control.history == []
    for k in gaussians.PARAMETERS:
        assert _bits(getattr(plain, k).detach(), getattr(empty, k).detach()), k


def test_one_densify_step_inside_fit_then_one_adam_step_matches_torch_adam(cuda):
    from mudg_amd import gaussians
    start, views, cam, mats, tgt = _problem(cuda)
    kw = dict(split_scale=0.2, max_scale=2.0)
    # iteration 0 by hand: the gradients, the statistics and the moments one Adam step leaves
    first = _model(cuda, start)
    stats = gaussians.DensityStats(len(first), cuda)
    rgb, _, _ = gaussians.render_differentiable(first.xyz, first.colour, first.covariance(), first.opacity(), mats, cam, HW, density=stats)
    (rgb - tgt).abs().mean().backward()
    b1, b2 = gaussians.ADAM_BETAS
    moments = {k: (((1 - b1) * getattr(first, k).grad).cpu().numpy(), ((1 - b2) * getattr(first, k).grad ** 2).cpu().numpy()) for k in gaussians.PARAMETERS}
    stepped = _model(cuda, start)
    gaussians.fit(stepped, tgt, mats, cam, HW, iters=1)
    params = {k: getattr(stepped, k).detach().cpu().numpy() for k in gaussians.PARAMETERS}
    control = gaussians.DensityControl(0, 1, 1, **kw)
    rows, row_moments, _, counts = gd.densify(params, moments, None, stats.grad_sum.cpu().numpy(), stats.seen.cpu().numpy(), control)
    assert counts["cloned"] > 0 and counts["split"] > 0 and counts["after"] > counts["before"]
    # the product: two iterations with one densify step between them
    mine = _model(cuda, start)
    losses = gaussians.fit(mine, tgt, mats, cam, HW, iters=2, density=control)
    assert len(losses) == 2 and [dict(h) for h in control.history] == [dict(counts, iteration=0)] and len(mine) == counts["after"]
    # torch.optim.Adam on the reference's rows, its state at step 1
    ref = gaussians.GaussianModel(*[_t(rows[k]).to(cuda) for k in gaussians.PARAMETERS])
    leaves = [getattr(ref, k) for k in gaussians.PARAMETERS]
    opt = torch.optim.Adam([{"params": [p], "lr": gaussians.LEARNING_RATES[k]} for k, p in zip(gaussians.PARAMETERS, leaves)],
                           betas=gaussians.ADAM_BETAS, eps=gaussians.ADAM_EPS)
    for k, p in zip(gaussians.PARAMETERS, leaves):
        opt.state[p] = {"step": torch.tensor(1.0), "exp_avg": _t(row_moments[k][0]).to(cuda), "exp_avg_sq": _t(row_moments[k][1]).to(cuda)}
    rgb, _, _ = gaussians.render_differentiable(ref.xyz, ref.colour, ref.covariance(), ref.opacity(), mats, cam, HW)
    loss = (rgb - tgt).abs().mean()
    loss.backward()
    opt.step()
    assert abs(losses[1] - float(loss.detach())) <= 1e-6 * float(loss.detach())
    for k in gaussians.PARAMETERS:
        err = rel_l2(getattr(mine, k), getattr(ref, k))
        print(f"{k}: rel-L2 to torch.optim.Adam on the reference's rows {err:.3e}")
        assert getattr(mine, k).requires_grad and getattr(mine, k).is_leaf and err < 1e-6, k


def test_densify_and_prune_falls_back_to_pruning_and_refuses_an_empty_model(cuda):
    from mudg_amd import gaussians, hip
    params, moments = toy(5, scale=(0.02, 0.15))
    params["opacity_logit"][:] = 0.0
    params["opacity_logit"][4] = -9.0
    d = lambda a: _t(a).to(cuda)
    ids = torch.arange(5, dtype=torch.int32, device=cuda)

    def fresh():
        stats = gaussians.DensityStats(5, cuda)
        stats.grad_sum.fill_(1.0)
        stats.seen.fill_(1)
        return gaussians.GaussianModel(*[d(params[k]) for k in gaussians.PARAMETERS], ids=ids), stats, {k: (d(m), d(v)) for k, (m, v) in moments.items()}

    model, stats, mom = fresh()
    counts = gaussians.densify_and_prune(model, stats, mom, _control(max_gaussians=8))
    assert counts == dict(before=5, after=8, kept=0, pruned=1, cloned=4, split=0, grew=True) and len(model) == 8 and len(stats) == 8
    assert model.ids.tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and not stats.grad_sum.any() and model.xyz.requires_grad and model.xyz.is_leaf
    assert _bits(mom["quat"][0][::2].cpu(), _t(moments["quat"][0][:4])) and not mom["quat"][0][1::2].any()
    model, stats, mom = fresh()
    del mom["colour"]                                                        # a parameter the fit does not move: zero moments
    counts = gaussians.densify_and_prune(model, stats, mom, _control(max_gaussians=7))
    assert counts == dict(before=5, after=4, kept=4, pruned=1, cloned=0, split=0, grew=False) and model.ids.tolist() == [0, 1, 2, 3]
    assert _bits(model.xyz.detach().cpu(), _t(params["xyz"][:4])) and not mom["colour"][0].any()
    assert gaussians.densify_and_prune(model, stats, mom, _control(), grow=False)["kept"] == 4
    model, stats, mom = fresh()
    with torch.no_grad():
        model.opacity_logit.fill_(-9.0)
    before = model.xyz
    with pytest.raises(hip.MudgError, match="prune all"):
        gaussians.densify_and_prune(model, stats, mom, _control())
    assert model.xyz is before and len(model) == 5 and len(stats) == 5 and stats.grad_sum.all()
    control = _control(reset_opacity=0.01)
    model, stats, mom = fresh()
    gaussians.reset_opacity(model, mom, control)
    assert float(model.opacity().max()) <= 0.01 + 1e-6 and float(model.opacity_logit[4]) == -9.0 and not mom["opacity_logit"][0].any()
    assert mom["xyz"][0].any()


def test_the_holed_fit_gains_from_density_control_as_the_float64_fit_does(cuda):
    from mudg_amd import gaussians
    start, views, cam, mats, tgt = _problem(cuda)
    holed, keep = gd.holed_start(start, views, cam, HW)
    plain, dense = _model(cuda, holed), _model(cuda, holed)
    a = gaussians.fit(plain, tgt, mats, cam, HW, iters=200)
    kw = dict(HOLED_CONTROL)
    control = gaussians.DensityControl(kw.pop("start"), kw.pop("stop"), kw.pop("every"), **kw)
    b = gaussians.fit(dense, tgt, mats, cam, HW, iters=200, density=control)
    r_plain, r_dense = a[-1] / a[0], b[-1] / b[0]
    # 2 r_dense64: §24's factor for fp32 rounding and hard thresholds moving an Adam trajectory
    print(f"holed fit: plain {a[0]:.5f} -> {a[-1]:.5f} (ratio {r_plain:.5f}); with density control {b[0]:.5f} -> {b[-1]:.5f} (ratio {r_dense:.5f}; "
          f"float64 {R_DENSE64}, bound {2 * R_DENSE64}); {len(plain)} -> {len(dense)} Gaussians")
    for h in control.history:
        print(h)
    assert len(b) == 200 and len(control.history) == 7 and len(dense) == control.history[-1]["after"] <= HOLED_CONTROL["max_gaussians"]
    assert r_dense <= 2 * R_DENSE64
    assert r_dense < r_plain
    out = gaussians.render(dense.gaussians(), mats, cam, HW)
    assert float((out["rgb"] - tgt).abs().mean()) <= 0.5 * b[0]


def test_fit_cloud_views_with_density_control_fills_a_thinned_cloud(cuda):
    from mudg_amd import gaussians, metrics, render, synthetic
    from virtual_render import virtual_pose_render as vpr
    s = synthetic.street_scene(n_background=2500, frames=2, seed=3, n_objects=2, object_points=200)
    dense = synthetic.street_scene(n_background=40000, frames=2, seed=3, n_objects=2, object_points=200)
    thin = render.PointCloud.from_arrays(s["bg_xyz"][::2], s["bg_rgb"][::2], cuda)
    scene = render.Scene(thin, None, s["intr"], s["c2w"], s["hw_native"])
    hw = (64, 96)
    target, _ = vpr.render_cloud_views(render.PointCloud.from_arrays(dense["bg_xyz"], dense["bg_rgb"], cuda), scene, [0, 1], 0, hw, 0.05)
    before, _ = vpr.render_cloud_views(thin, scene, [0, 1], 0, hw, 0.1)
    control = gaussians.DensityControl(5, 50, 15, split_scale=0.15, max_scale=1.0, max_gaussians=5000)
    history = []
    g = vpr.fit_cloud_views(thin, scene, [0, 1], target, 0, hw, 0.1, iters=60, history=history, density=control)
    after = gaussians.render_scene(g, None, s["intr"], s["c2w"], s["hw_native"], hw, poses=s["c2w"][:, None])["rgb_u8"][0]
    p0, p1 = metrics.psnr_ssim(before, target)["psnr"], metrics.psnr_ssim(after, target)["psnr"]
    print(f"PSNR against the target frames: {p0.tolist()} -> {p1.tolist()} dB after {len(history)} iterations; {len(thin)} -> {len(g)} Gaussians")
    for h in control.history:
        print(h)
    assert len(history) == 60 and len(control.history) == 3 and bool((p1 > p0).all())
    assert len(g) != len(thin) and len(g) == control.history[-1]["after"]
