"""The training half of the Gaussian splat renderer on the GPU (csrc/gaussians_bwd.hip through mudg_amd/ops.py and gaussians.py) against
the CPU definition of the rule (tests/gaussians_bwd_reference.py): torch.equal for state, the partial buffer and every gradient — both
sides perform the same correctly rounded fp32 operations in the same order, so there is no tolerance — and the fit loop against its
float64 counterpart."""
import numpy as np
import pytest
import torch

import gaussians_bwd_reference as gb
import gaussians_reference as gr
from helpers import rel_l2
from sentinel_buffers import Flat
from test_gaussians_bwd_cpu import R64
from test_gaussians_gpu import _flat_case, _ids_case, _scene_case

pytestmark = pytest.mark.gpu
F = np.float32
GRADS = ("d_xyz", "d_cov", "d_opacity", "d_colour")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _inputs(case, seed=5):
    """A case of the forward tests with fp32 colours that are no whole bytes and seeded upstream gradients."""
    pts, cov, op, ids, mats, cam, hw = case
    xyz, _ = gr.unpack(pts)
    rng = np.random.default_rng(seed)
    colour = rng.uniform(0.0, 255.0, (len(xyz), 3)).astype(F)
    V = mats.shape[0]
    up = (rng.normal(size=(V, 3) + tuple(hw)).astype(F), (rng.normal(size=(V,) + tuple(hw)) * 0.05).astype(F), rng.normal(size=(V,) + tuple(hw)).astype(F))
    return xyz, colour, up


def _direct(cuda, case, colour, up, corrupt=None):
    """The entry points one after the other through mudg_amd.ops, each of the three new ones twice: a repeat must give the same bits."""
    from mudg_amd import ops
    pts, cov, op, ids, mats, cam, hw = case
    d = lambda a: None if a is None else _t(a).to(cuda)
    d_pts, d_cov, d_op, d_ids, d_mats, d_col = d(pts), d(cov), d(op), d(ids), d(mats), d(colour)
    d_up = [d(u) for u in up]
    uv, conic, depth, rect, count = ops.gauss_project(d_pts, d_cov, d_op, d_mats, cam, hw, ids=d_ids)
    ends = torch.cumsum(count.reshape(-1), 0, dtype=torch.int64)
    offsets = (ends - count.reshape(-1)).reshape(count.shape)
    E = int(ends[-1])
    assert E > 0
    keys, values = ops.gauss_keys(depth, rect, count, offsets, E, hw)
    keys, order = torch.sort(keys, stable=True)
    values = values[order]
    tx, ty = gr.tiles(hw)
    ranges = ops.gauss_ranges(keys, mats.shape[0] * tx * ty)
    if corrupt is not None:
        values, order, ranges = corrupt(values, order, ranges)
    runs = []
    for _ in range(2):
        rgb, dimg, alpha, state = ops.gauss_blend_train(d_col, uv, conic, depth, values, ranges, hw)
        partial = ops.gauss_blend_bwd(d_col, uv, conic, depth, values, order, ranges, hw, state, *d_up)
        grads = ops.gauss_project_bwd(d_pts, d_cov, d_mats, cam, hw, count, offsets, partial, ids=d_ids)
        runs.append(dict(rgb=rgb, depth_image=dimg, alpha=alpha, state=state, partial=partial, **dict(zip(GRADS, grads))))
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(torch.int32), runs[1][k].view(torch.int32)), f"{k}: a repeat run differs"
    return runs[0], dict(values=values, order=order, ranges=ranges, offsets=offsets, count=count)


def _check(cuda, case, what):
    xyz, colour, up = _inputs(case)
    pts, cov, op, ids, mats, cam, hw = case
    want = gb.render_backward(xyz, colour, cov, op, ids, mats, cam, hw, *up)
    got, mid = _direct(cuda, case, colour, up)
    assert torch.equal(mid["order"].cpu(), _t(want["order"])) and torch.equal(mid["values"].cpu(), _t(want["values"])), what
    bad = {k: int((got[k].cpu() != _t(want[k])).sum()) for k in got}
    print(f"{what}: {want['entries']} entries, {int((want['partial'] != 0).any(axis=1).sum())} with a partial; elements that differ: {bad}")
    for k in got:
        assert got[k].dtype == torch.float32 and torch.equal(got[k].cpu(), _t(want[k])), (what, k)
    assert np.isfinite(want["partial"]).all() and all(np.isfinite(want[k]).all() for k in GRADS)
    return got, want


# ------------------------------------------------------------------------------------------------ image sizes, batch edges
@pytest.mark.parametrize("hw", [(1, 1), (16, 16), (17, 33), (40, 56)])
def test_images_that_are_and_are_not_whole_tiles(cuda, hw):
    got, want = _check(cuda, _scene_case(150, hw, 11), f"{hw[0]} x {hw[1]}")
    assert want["d_xyz"].any() and want["d_cov"].any() and want["d_opacity"].any() and want["d_colour"].any()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_a_tile_with_entries_at_the_batch_edges(cuda, n):
    rng = np.random.default_rng(n)
    case = _flat_case(rng.uniform(5.0, 11.0, (n, 2)), 0.5, (17, 33), opacity=rng.uniform(0.004, 0.02, n).astype(F), z=rng.uniform(60.0, 180.0, n).astype(F), seed=n)
    got, want = _check(cuda, case, f"{n} Gaussians on one tile")
    assert want["entries"] == n and want["walked"][0] == n                                               # no pixel finishes: the tile is walked to its end
    assert want["partial"].any(axis=1).sum() >= 0.8 * n                                                # an opacity below 1 / 255 is skipped everywhere


def test_a_tile_that_finishes_in_its_first_batch_leaves_the_rest_at_zero(cuda):
    rng = np.random.default_rng(21)
    n = 556
    case = _flat_case(rng.uniform(2.0, 14.0, (n, 2)), 40.0, (16, 16), z=rng.uniform(60.0, 180.0, n).astype(F), seed=21)
    got, want = _check(cuda, case, "opaque after a few entries, 556 on the tile")
    assert want["walked"].tolist() == [256] and want["entries"] - 256 == 300
    behind = _t(want["order"][256:]).to(cuda)
    assert not got["partial"][behind].any()                                                            # exactly zero: never staged
    assert int(got["partial"].any(dim=1).sum()) < 10


def test_a_tile_where_a_pixel_never_finishes_is_walked_to_its_end(cuda):
    rng = np.random.default_rng(22)
    n = 300
    case = _flat_case(np.full((n, 2), 5.5, F), 3.0, (16, 16), z=rng.uniform(120.0, 180.0, n).astype(F), seed=22)
    got, want = _check(cuda, case, "300 entries, the far corner untouched")
    assert want["walked"].tolist() == [300] and want["alpha"][0, 15, 15] == 0


def test_one_gaussian_over_every_tile_is_one_long_gather(cuda):
    got, want = _check(cuda, _flat_case([[28.0, 20.0]], 60.0, (40, 56), opacity=0.7), "one Gaussian over twelve tiles")
    assert want["count"][0, 0] == 12 and want["partial"].any(axis=1).all() and want["d_opacity"][0] != 0


def test_equal_depths(cuda):
    rng = np.random.default_rng(23)
    _check(cuda, _flat_case(rng.uniform(0.0, 33.0, (60, 2)), 2.0, (17, 33), opacity=0.5, seed=23), "sixty Gaussians at one depth")


def test_three_views_in_one_call_equal_three_calls_added_in_view_order(cuda):
    case = _scene_case(200, (40, 56), 13, views=3)
    got, want = _check(cuda, case, "three views")
    xyz, colour, up = _inputs(case)
    pts, cov, op, ids, mats, cam, hw = case
    total = None
    for v in range(3):
        one, _ = _direct(cuda, (pts, cov, op, ids, mats[v:v + 1], cam, hw), colour, [u[v:v + 1] for u in up])
        assert torch.equal(one["state"][0], got["state"][v])
        total = {k: one[k] for k in GRADS} if total is None else {k: total[k] + one[k] for k in GRADS}
    for k in GRADS:
        assert torch.equal(total[k], got[k]), k


def test_object_ids_a_zero_matrix_and_ids_out_of_range(cuda):
    case = _ids_case()
    got, want = _check(cuda, case, "three matrices a view")
    ids = case[3]
    clamped = case[:3] + (np.clip(ids, 0, 2),) + case[4:]
    xyz, colour, up = _inputs(case)
    again, _ = _direct(cuda, clamped, colour, up)
    assert all(torch.equal(again[k], got[k]) for k in got)


# ------------------------------------------------------------------------------------------------ the autograd Function
def _leaves(cuda, xyz, colour, cov, op):
    return [_t(a).to(cuda).requires_grad_(True) for a in (xyz, colour, cov, op)]


def test_everything_culled_gives_zero_gradients(cuda):
    from mudg_amd import gaussians
    pts, cov, op, ids, mats, cam, hw = _flat_case([[8.5, 8.5], [3.0, 4.0]], 0.5, (17, 33), z=[250.0, 300.0])
    xyz, colour, up = _inputs((pts, cov, op, ids, mats, cam, hw))
    leaves = _leaves(cuda, xyz, colour, cov, op)
    rgb, depth, alpha = gaussians.render_differentiable(*leaves, _t(mats).to(cuda), cam, hw)
    assert not rgb.any() and not depth.any() and not alpha.any()
    (rgb.sum() + depth.sum() + alpha.sum()).backward()
    for leaf in leaves:
        assert leaf.grad is not None and leaf.grad.shape == leaf.shape and not leaf.grad.any()


def test_whole_byte_colours_equal_the_inference_render_and_backward_equals_the_direct_calls(cuda):
    from mudg_amd import gaussians, render
    case = _scene_case(200, (40, 56), 13, views=3)
    pts, cov, op, ids, mats, cam, hw = case
    xyz, words = gr.unpack(pts)
    whole = np.stack([(words >> (8 * k)) & 0xff for k in range(3)], axis=1).astype(F)
    d_mats = _t(mats).to(cuda)
    with torch.no_grad():
        rgb, depth, alpha = gaussians.render_differentiable(*_leaves(cuda, xyz, whole, cov, op), d_mats, cam, hw)
    ref = gaussians.render(gaussians.Gaussians(render.PointCloud(_t(pts).to(cuda)), _t(cov).to(cuda), _t(op).to(cuda)), d_mats, cam, hw)
    assert torch.equal(rgb, ref["rgb"]) and torch.equal(depth, ref["depth"]) and torch.equal(alpha, ref["alpha"])
    _, colour, up = _inputs(case)
    leaves = _leaves(cuda, xyz, colour, cov, op)
    out = gaussians.render_differentiable(*leaves, d_mats, cam, hw)
    torch.autograd.backward(out, [_t(u).to(cuda) for u in up])
    direct, _ = _direct(cuda, case, colour, up)
    for leaf, k in zip(leaves, ("d_xyz", "d_colour", "d_cov", "d_opacity")):
        assert torch.equal(leaf.grad, direct[k]), k
    for o, k in zip(out, ("rgb", "depth_image", "alpha")):
        assert torch.equal(o, direct[k]), k


# ------------------------------------------------------------------------------------------------ the entry points, outputs inside sentinels
def test_no_entry_point_writes_outside_its_outputs_or_follows_an_unchecked_value(cuda):
    from mudg_amd import hip
    case = _ids_case()
    pts, cov, op, ids, mats, cam, hw = case
    xyz, colour, up = _inputs(case)
    lib = hip.lib()
    V, n, (H, W) = mats.shape[0], len(pts), hw

    def spoil(values, order, ranges):                                        # values outside the cloud, positions outside [0, E), ranges outside [0, E]
        values, order, ranges = values.clone(), order.clone(), ranges.clone()
        E = values.numel()
        values[::7], values[3::11] = -5, n
        order[::5], order[2::9] = -1, E
        ranges[1], ranges[2] = torch.tensor([-4, 3], dtype=torch.int32), torch.tensor([0, E + 1], dtype=torch.int32)
        return values, order, ranges

    for corrupt in (None, spoil):
        _, mid = _direct(cuda, case, colour, up, corrupt)
        values, order, ranges = (mid[k].cpu().numpy() for k in ("values", "order", "ranges"))
        E = len(values)
        proj = gr.project(xyz, cov, op, ids, mats, cam, hw)
        w_rgb, w_depth, w_alpha, w_state = gb.blend_train(proj, colour, values, np.where((ranges[:, :1] < 0) | (ranges[:, 1:] > E) | (ranges[:, :1] > ranges[:, 1:]), 0, ranges), hw)
        w_partial = gb.blend_bwd(proj, colour, values, order, ranges, hw, w_state, *up)
        w_grads = gb.project_bwd(xyz, cov, ids, mats, cam, hw, proj["count"], mid["offsets"].cpu().numpy(), w_partial)
        d = lambda a: _t(a).to(cuda)
        uv, conic, depth, d_col = d(proj["uv"]), d(proj["conic"]), d(proj["depth"]), d(colour)
        rgb, dimg, alpha, state = (Flat(V * c * H * W, torch.float32).blank(cuda) for c in (3, 1, 1, 5))
        hip.check(lib.mudg_gauss_blend_train(d_col.data_ptr(), uv.data_ptr(), conic.data_ptr(), depth.data_ptr(), mid["values"].data_ptr(),
                                             mid["ranges"].data_ptr(), n, E, V, H, W, rgb.ptr, dimg.ptr, alpha.ptr, state.ptr, None), "blend_train")
        torch.cuda.synchronize()
        assert torch.equal(rgb.read("rgb"), _t(w_rgb).reshape(-1)) and torch.equal(dimg.read("depth"), _t(w_depth).reshape(-1))
        assert torch.equal(alpha.read("alpha"), _t(w_alpha).reshape(-1))
        got_state = state.read("state")
        assert torch.equal(got_state, _t(w_state).reshape(-1))
        partial = Flat(E * 10, torch.float32).blank(cuda)
        d_state, d_up = got_state.to(cuda), [d(u) for u in up]
        hip.check(lib.mudg_gauss_blend_bwd(d_col.data_ptr(), uv.data_ptr(), conic.data_ptr(), depth.data_ptr(), mid["values"].data_ptr(),
                                           mid["order"].data_ptr(), mid["ranges"].data_ptr(), n, E, V, H, W, d_state.data_ptr(), d_up[0].data_ptr(),
                                           d_up[1].data_ptr(), d_up[2].data_ptr(), partial.ptr, None), "blend_bwd")
        torch.cuda.synchronize()
        got_partial = partial.read("partial")
        assert torch.equal(got_partial, _t(w_partial).reshape(-1))
        outs = [Flat(n * c, torch.float32).blank(cuda) for c in (3, 6, 1, 3)]
        d_partial, d_pts, d_cov, d_ids, d_mats = got_partial.to(cuda), d(pts), d(cov), d(ids), d(mats)
        hip.check(lib.mudg_gauss_project_bwd(d_pts.data_ptr(), d_cov.data_ptr(), d_ids.data_ptr(), n, d_mats.data_ptr(), V, mats.shape[1], H, W,
                                             *[float(c) for c in cam], gr.ZNEAR, gr.ZFAR, mid["count"].data_ptr(), mid["offsets"].data_ptr(),
                                             d_partial.data_ptr(), E, *[o.ptr for o in outs], None), "project_bwd")
        torch.cuda.synchronize()
        for o, k, w in zip(outs, GRADS, w_grads):
            assert torch.equal(o.read(k), _t(w).reshape(-1)), k


# ------------------------------------------------------------------------------------------------ the model and the fit
def _model(cuda, start):
    from mudg_amd import gaussians
    return gaussians.GaussianModel(*[_t(start[k]).to(cuda) for k in gaussians.PARAMETERS])


def test_one_adam_step_through_fit_matches_torch_adam(cuda):
    from mudg_amd import gaussians
    start, views, cam, targets = gb.fit_problem()
    hw = (40, 56)
    mats, tgt = _t(views).to(cuda), targets.to(torch.float32).to(cuda)
    mine, ref = _model(cuda, start), _model(cuda, start)
    losses = gaussians.fit(mine, tgt, mats, cam, hw, iters=1)
    params = [getattr(ref, k) for k in gaussians.PARAMETERS]
    opt = torch.optim.Adam([{"params": [p], "lr": gaussians.LEARNING_RATES[k]} for k, p in zip(gaussians.PARAMETERS, params)],
                           betas=gaussians.ADAM_BETAS, eps=gaussians.ADAM_EPS)
    rgb, _, _ = gaussians.render_differentiable(ref.xyz, ref.colour, ref.covariance(), ref.opacity(), mats, cam, hw)
    loss = (rgb - tgt).abs().mean()
    loss.backward()
    opt.step()
    assert abs(losses[0] - float(loss)) <= 1e-6 * float(loss)
    for k in gaussians.PARAMETERS:
        moved = float((getattr(mine, k).detach() - _t(start[k]).to(cuda)).abs().max())
        err = rel_l2(getattr(mine, k), getattr(ref, k))
        print(f"{k}: moved by at most {moved:.3e}, rel-L2 to torch.optim.Adam {err:.3e}")
        assert (moved > 0 or k == "quat") and err < 1e-6, k      # test_training_gpu.py's AdamW tolerance; an isotropic seed's rotation has no gradient


def test_the_fit_lowers_the_loss_as_the_float64_loop_does_and_its_result_renders(cuda):
    from mudg_amd import gaussians
    start, views, cam, targets = gb.fit_problem()
    hw = (40, 56)
    mats, tgt = _t(views).to(cuda), targets.to(torch.float32).to(cuda)
    model = _model(cuda, start)
    losses = gaussians.fit(model, tgt, mats, cam, hw, iters=200)
    ratio = losses[-1] / losses[0]
    # 2 r64: fp32 rounding and the hard skip thresholds move an Adam trajectory; r64 is the float64 loop's ratio, measured on the CPU
    print(f"fit: loss {losses[0]:.5f} -> {losses[-1]:.5f}, ratio {ratio:.5f} (float64: {R64}, bound {2 * R64})")
    assert len(losses) == 200 and ratio <= 2 * R64
    g = model.gaussians()
    assert isinstance(g, gaussians.Gaussians) and len(g) == len(model)
    byte = torch.floor(model.colour.detach() + 0.5).clamp(0, 255).to(torch.int32)
    assert torch.equal(g.cloud.points[:, 3], byte[:, 0] | (byte[:, 1] << 8) | (byte[:, 2] << 16))
    assert torch.equal(g.cloud.points[:, :3].contiguous().view(torch.float32), model.xyz.detach())
    assert torch.equal(g.cov, model.covariance().detach()) and torch.equal(g.opacity, model.opacity().detach())
    out = gaussians.render(g, mats, cam, hw)
    err = float((out["rgb"] - tgt).abs().mean())
    print(f"the exported Gaussians through the inference renderer: mean absolute difference {err:.5f}")
    assert err <= losses[0] * 0.5                                                                     # bytes are rounded: not the last loss exactly
    back = gaussians.GaussianModel.from_cloud(g.cloud, torch.sqrt(g.cov[:, 0]), g.opacity)
    assert torch.equal(back.xyz.detach(), model.xyz.detach()) and torch.equal(back.colour.detach(), byte.to(torch.float32))


def test_fit_cloud_views_raises_the_psnr_of_render_cloud_views(cuda):
    from mudg_amd import gaussians, metrics, render, synthetic
    from virtual_render import virtual_pose_render as vpr
    s = synthetic.street_scene(n_background=2500, frames=2, seed=3, n_objects=2, object_points=200)
    dense = synthetic.street_scene(n_background=40000, frames=2, seed=3, n_objects=2, object_points=200)
    background = render.PointCloud.from_arrays(s["bg_xyz"], s["bg_rgb"], cuda)
    scene = render.Scene(background, None, s["intr"], s["c2w"], s["hw_native"])
    hw = (64, 96)
    target, _ = vpr.render_cloud_views(render.PointCloud.from_arrays(dense["bg_xyz"], dense["bg_rgb"], cuda), scene, [0, 1], 0, hw, 0.05)
    before, _ = vpr.render_cloud_views(background, scene, [0, 1], 0, hw, 0.1)
    history = []
    g = vpr.fit_cloud_views(background, scene, [0, 1], target, 0, hw, 0.1, iters=60, history=history)
    after = gaussians.render_scene(g, None, s["intr"], s["c2w"], s["hw_native"], hw, poses=s["c2w"][:, None])["rgb_u8"][0]
    p0, p1 = metrics.psnr_ssim(before, target)["psnr"], metrics.psnr_ssim(after, target)["psnr"]
    print(f"PSNR against the target frames: {p0.tolist()} -> {p1.tolist()} dB after {len(history)} iterations, loss {history[0]:.4f} -> {history[-1]:.4f}")
    assert len(history) == 60 and bool((p1 > p0).all())
