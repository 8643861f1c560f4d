"""The image loss of the Gaussian fit on the GPU (csrc/gaussians_loss.hip through mudg_amd/ops.py and gaussians.py) against
the CPU definition of the rule (tests/gaussians_loss_reference.py): torch.equal on int32 views for the maps, the partials, the finish buffer
and both gradients — both sides perform the same correctly rounded fp32 operations in the same order, so there is no tolerance — then the
autograd surface, and the fit with the SSIM term against its float64 counterpart."""
import functools

import numpy as np
import pytest
import torch

import gaussians_bwd_reference as gb
import gaussians_loss_reference as gl
from sentinel_buffers import Flat
from test_gaussians_loss_cpu import R64S

pytestmark = pytest.mark.gpu
F = np.float32
# an image that is all padding, one smaller than the window, exactly one window, exactly one tile, tiles that are not whole in either
# direction, more than one view
SHAPES = ((1, 1, 1), (1, 5, 7), (1, 11, 11), (1, 16, 16), (1, 17, 33), (2, 40, 56), (3, 40, 56))
WEIGHTS, UPSTREAMS, DEPTH_WEIGHT = (0.0, 0.2, 1.0), (1.0, 2.5), 0.1


def _t(a):
    return torch.from_numpy(np.array(a))                                    # a copy: the cached cases stay as they are


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _case(shape, with_depth):
    """Seeded images of one shape and the definition's forward, computed once and left unchanged."""
    V, H, W = shape
    x, y, d, dt = gl.seeded_images(V, (H, W), seed=11 + H)
    if not with_depth:
        d = dt = None
    maps, partial, _, _ = gl.forward(x, y, d, dt)
    for a in (x, y, d, dt, maps, partial):
        if a is not None:
            a.setflags(write=False)
    return x, y, d, dt, maps, partial


@functools.lru_cache(maxsize=None)
def _want(shape, with_depth, lam, up):
    x, y, d, dt, maps, partial = _case(shape, with_depth)
    dw = DEPTH_WEIGHT if with_depth else 0.0
    totals = gl.finish(partial, shape[1:], lam, dw)
    d_rgb, d_depth = gl.backward(x, y, maps, totals, up, lam, dw, d, dt)
    return totals, d_rgb, d_depth


# ------------------------------------------------------------------------------------------------ bit-equality with the definition
@pytest.mark.parametrize("with_depth", (False, True), ids=("rgb", "rgb+depth"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_output_has_the_definitions_bits_and_a_repeat_has_them_again(cuda, shape, with_depth):
    from mudg_amd import ops
    x, y, d, dt, maps, partial = _case(shape, with_depth)
    dev = lambda a: None if a is None else _t(a).to(cuda)
    dx, dy, dd, ddt = dev(x), dev(y), dev(d), dev(dt)
    dw = DEPTH_WEIGHT if with_depth else 0.0
    for run in range(2):
        got_maps, got_partial = ops.gauss_loss(dx, dy, dd, ddt)
        assert _bits(got_maps.cpu(), _t(maps)), ("maps", run)
        assert _bits(got_partial.cpu(), _t(partial)), ("partial", run)
        for lam in WEIGHTS:
            totals = ops.gauss_loss_finish(got_partial, shape[1:], ssim_weight=lam, depth_weight=dw)
            for up in UPSTREAMS:
                want_totals, want_rgb, want_depth = _want(shape, with_depth, lam, up)
                assert _bits(totals.cpu(), _t(want_totals)), ("totals", lam, run, totals.cpu(), want_totals)
                d_rgb, d_depth = ops.gauss_loss_bwd(dx, dy, got_maps, totals, torch.tensor([up], dtype=torch.float32, device=cuda), dd, ddt,
                                                    ssim_weight=lam, depth_weight=dw)
                assert _bits(d_rgb.cpu(), _t(want_rgb)), ("d_rgb", lam, up, run)
                assert (d_depth is None) == (not with_depth)
                if with_depth:
                    assert _bits(d_depth.cpu(), _t(want_depth)), ("d_depth", lam, up, run)
    if with_depth:                                                          # a backward that is not asked for the depth gradient stores none
        assert ops.gauss_loss_bwd(dx, dy, got_maps, totals, torch.ones(1, device=cuda), dd, ddt, ssim_weight=1.0, depth_weight=dw,
                                  want_depth=False)[1] is None


# ------------------------------------------------------------------------------------------------ answers known without arithmetic
def test_equal_images_have_ssim_one_in_every_pixel(cuda):
    from mudg_amd import gaussians, ops
    x = _t(np.random.default_rng(5).uniform(-0.5, 1.5, (2, 3, 17, 33)).astype(F)).to(cuda)
    maps, partial = ops.gauss_loss(x, x.clone())
    assert float(partial[..., 1].double().sum()) == 2 * 3 * 17 * 33 and not bool(partial[..., 0].any())      # sum S == N: every S is 1.0
    totals = ops.gauss_loss_finish(partial, (17, 33), ssim_weight=0.2)
    assert totals[:4].tolist() == [0.0, 0.0, 1.0, 0.0]
    d_rgb, _ = ops.gauss_loss_bwd(x, x.clone(), maps, totals, torch.full((1,), 2.5, device=cuda), ssim_weight=0.0)
    assert not bool(d_rgb.any())                                            # the L1 part: sgn(0) = 0
    terms = gaussians.image_loss.terms(x, x.clone(), ssim_weight=0.2)
    assert float(terms["ssim"]) == 1.0 and float(terms["l1"]) == 0.0 and float(terms["loss"]) == 0.0


def test_depth_targets_that_are_all_zero_count_nothing(cuda):
    from mudg_amd import ops
    x, y, d, dt = (_t(a).to(cuda) for a in gl.seeded_images(2, (17, 33)))
    maps, partial = ops.gauss_loss(x, y, d, torch.zeros_like(dt))
    totals = ops.gauss_loss_finish(partial, (17, 33), ssim_weight=0.2, depth_weight=0.5)
    plain = ops.gauss_loss_finish(ops.gauss_loss(x, y)[1], (17, 33), ssim_weight=0.2)
    assert totals[3:5].tolist() == [0.0, 1.0] and int(totals.view(torch.int32)[5]) == 0 and _bits(totals[:1], plain[:1])
    d_rgb, d_depth = ops.gauss_loss_bwd(x, y, maps, totals, torch.full((1,), 2.5, device=cuda), d, torch.zeros_like(dt), ssim_weight=0.2,
                                        depth_weight=0.5)
    assert d_depth.shape == d.shape and not bool(d_depth.any())


def test_one_pixels_ssim_reaches_the_four_tiles_around_a_corner_as_the_definition_says(cuda):
    from mudg_amd import ops
    x, y, maps, impulse = gl.impulse_case()
    totals = gl.finish(gl.forward(x, y)[1], (33, 33), 1.0, 0.0)
    want, _ = gl.backward(x, y, impulse, totals, 1.0, 1.0, 0.0)
    got, _ = ops.gauss_loss_bwd(_t(x).to(cuda), _t(y).to(cuda), _t(impulse).to(cuda), _t(totals).to(cuda), torch.ones(1, device=cuda),
                                ssim_weight=1.0)
    assert _bits(got.cpu(), _t(want))
    hit = torch.nonzero(got[0, 1]).cpu()
    assert len(hit) == 121 and hit.min(0).values.tolist() == [10, 10] and hit.max(0).values.tolist() == [20, 20]


# ------------------------------------------------------------------------------------------------ raw entry points, in sentinels
def test_the_entry_points_write_their_outputs_and_nothing_else_and_a_refusal_writes_nothing(cuda):
    from mudg_amd import hip
    lib = hip.lib()
    shape, lam, up = (2, 17, 33), 0.2, 2.5
    V, H, W = shape
    x, y, d, dt, maps, partial = _case(shape, True)
    want_totals, want_rgb, want_depth = _want(shape, True, lam, up)
    dx, dy, dd, ddt = (_t(a).to(cuda) for a in (x, y, d, dt))
    d_up = torch.tensor([up], dtype=torch.float32, device=cuda)
    m_buf, p_buf = Flat(maps.size, torch.float32, off=1).blank(cuda), Flat(partial.size, torch.float32, off=3).blank(cuda)
    t_buf = Flat(8, torch.float32, off=1).blank(cuda)
    g_buf, gd_buf = Flat(x.size, torch.float32, off=5).blank(cuda), Flat(d.size, torch.float32, off=7).blank(cuda)
    fwd = [dx.data_ptr(), dy.data_ptr(), dd.data_ptr(), ddt.data_ptr(), V, H, W, m_buf.ptr, p_buf.ptr, None]
    fin = [p_buf.ptr, V, H, W, lam, DEPTH_WEIGHT, t_buf.ptr, None]
    bwd = [dx.data_ptr(), dy.data_ptr(), m_buf.ptr, dd.data_ptr(), ddt.data_ptr(), t_buf.ptr, d_up.data_ptr(), V, H, W, lam, DEPTH_WEIGHT, g_buf.ptr,
           gd_buf.ptr, None]

    def refusals(fn, good, outs, required, pointers, at, weights=None, extra=()):
        """Every refusal of the entry point: a null among `required`, a pointer among `pointers` off by two bytes, V, H, W (at `at`) not
        positive, V NT >= 2^31, more workgroups than a grid, weights out of range.  No byte of `outs` may change."""
        cases = [{k: None} for k in required] + [{k: good[k] + 2} for k in pointers] + list(extra)
        for k in range(3):
            cases += [{at + k: 0}, {at + k: -1}]
        cases += [{at: 2 ** 19, at + 1: 1024, at + 2: 1024}, {at: 2 ** 18, at + 1: 1024, at + 2: 1024}]
        if weights is not None:
            cases += [{weights: v} for v in (-0.01, 1.01, float("nan"))] + [{weights + 1: v} for v in (-0.5, float("nan"), float("inf"))]
        before = [o.dev.clone() for o in outs]
        for change in cases:
            args = list(good)
            for k, v in change.items():
                args[k] = v
            assert fn(*args) == -1, (fn.__name__, change)
        torch.cuda.synchronize()
        for o, was in zip(outs, before):
            assert torch.equal(o.dev.view(torch.uint8), was.view(torch.uint8)), (fn.__name__, "a refused call wrote")
        return len(cases)

    n = refusals(lib.mudg_gauss_loss, fwd, (m_buf, p_buf), (0, 1, 7, 8), (0, 1, 2, 3, 7, 8), 4, extra=[{2: None}, {3: None}])
    m_buf.unchanged("maps before the forward")
    p_buf.unchanged("partial before the forward")
    hip.check(lib.mudg_gauss_loss(*fwd), "mudg_gauss_loss")
    torch.cuda.synchronize()
    assert _bits(m_buf.read("maps"), _t(maps).reshape(-1)) and _bits(p_buf.read("partial"), _t(partial).reshape(-1))
    n += refusals(lib.mudg_gauss_loss_finish, fin, (t_buf,), (0, 6), (0, 6), 1, weights=4)
    t_buf.unchanged("totals before the finish")
    hip.check(lib.mudg_gauss_loss_finish(*fin), "mudg_gauss_loss_finish")
    torch.cuda.synchronize()
    assert _bits(t_buf.read("totals"), _t(want_totals))
    n += refusals(lib.mudg_gauss_loss_bwd, bwd, (g_buf, gd_buf), (0, 1, 2, 5, 6, 12), (0, 1, 2, 3, 4, 5, 6, 12, 13), 7, weights=10,
                  extra=[{3: None}, {4: None}, {3: None, 4: None}])
    g_buf.unchanged("d_rgb before the backward")
    gd_buf.unchanged("d_depth before the backward")
    hip.check(lib.mudg_gauss_loss_bwd(*bwd), "mudg_gauss_loss_bwd")
    torch.cuda.synchronize()
    assert _bits(g_buf.read("d_rgb"), _t(want_rgb).reshape(-1)) and _bits(gd_buf.read("d_depth"), _t(want_depth).reshape(-1))
    assert _bits(m_buf.read("maps after the backward"), _t(maps).reshape(-1)) and _bits(t_buf.read("totals after the backward"), _t(want_totals))
    print(f"{n} refused calls left every sentinel and every output as it was")
    # a backward that is given no d_depth writes d_rgb alone
    again = Flat(x.size, torch.float32, off=5).blank(cuda)
    args = list(bwd)
    args[12], args[13] = again.ptr, None
    hip.check(lib.mudg_gauss_loss_bwd(*args), "mudg_gauss_loss_bwd")
    torch.cuda.synchronize()
    assert _bits(again.read("d_rgb without d_depth"), _t(want_rgb).reshape(-1))


# ------------------------------------------------------------------------------------------------ autograd
def test_image_loss_backward_is_the_three_entry_points(cuda):
    from mudg_amd import gaussians, ops
    x, y, d, dt = (_t(a).to(cuda) for a in gl.seeded_images(2, (40, 56)))
    rgb, depth = x.clone().requires_grad_(True), d.clone().requires_grad_(True)
    loss = gaussians.image_loss(rgb, y, depth, dt, ssim_weight=0.2, depth_weight=0.1)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    (loss * 2.5).backward()
    maps, partial = ops.gauss_loss(x, y, d, dt)
    totals = ops.gauss_loss_finish(partial, (40, 56), ssim_weight=0.2, depth_weight=0.1)
    d_rgb, d_depth = ops.gauss_loss_bwd(x, y, maps, totals, torch.full((1,), 2.5, device=cuda), d, dt, ssim_weight=0.2, depth_weight=0.1)
    assert _bits(loss.detach().reshape(1), totals[:1]) and _bits(rgb.grad, d_rgb) and _bits(depth.grad, d_depth)
    terms = gaussians.image_loss.terms(x, y, d, dt, ssim_weight=0.2, depth_weight=0.1)
    assert [float(terms[k]) for k in ("loss", "l1", "ssim", "depth")] == totals[:4].tolist() and int(terms["depth_count"]) == int((dt > 0).sum())
    only = x.clone().requires_grad_(True)                                   # no depth pair, default weights
    gaussians.image_loss(only, y).backward()
    assert _bits(only.grad, ops.gauss_loss_bwd(x, y, maps, ops.gauss_loss_finish(partial, (40, 56), ssim_weight=0.2), torch.ones(1, device=cuda),
                                               ssim_weight=0.2)[0])


def test_without_the_ssim_term_image_loss_is_the_mean_absolute_difference(cuda):
    from mudg_amd import gaussians
    x, y, _, _ = (_t(a).to(cuda) for a in gl.seeded_images(3, (40, 56)))
    rgb = x.clone().requires_grad_(True)
    loss = gaussians.image_loss(rgb, y, ssim_weight=0.0, depth_weight=0.0)
    loss.backward()
    want = (x.double() - y.double()).abs().mean()
    assert abs(loss.item() - want.item()) <= 1e-6 * want.item()
    sign = torch.sign(x - y).double() / x.numel()
    ulp = 2.0 ** (np.floor(np.log2(1.0 / x.numel())) - 23)                  # one ulp of fl(1 / N)
    assert float((rgb.grad.double() - sign).abs().max()) <= ulp


def test_tensors_off_the_gpu_are_refused(cuda):
    from mudg_amd import gaussians, hip
    x = torch.zeros(1, 3, 8, 8)
    for call in (lambda: gaussians.image_loss(x, x.to(cuda)), lambda: gaussians.image_loss(x.to(cuda), x),
                 lambda: gaussians.image_loss(x.to(cuda), x.to(cuda), torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, device=cuda), depth_weight=1.0),
                 lambda: gaussians.image_loss(x.to(cuda), x.to(cuda), ssim_weight=1.5)):
        with pytest.raises(hip.MudgError):
            call()


# ------------------------------------------------------------------------------------------------ the fit
def _model(cuda, start):
    from mudg_amd import gaussians
    return gaussians.GaussianModel(*[_t(start[k]).to(cuda) for k in gaussians.PARAMETERS])


def test_a_fit_without_the_ssim_term_is_the_fit_it_was(cuda):
    from mudg_amd import gaussians
    start, views, cam, targets = gb.fit_problem()
    mats, tgt = _t(views).to(cuda), targets.to(torch.float32).to(cuda)
    old, new = _model(cuda, start), _model(cuda, start)
    depth_targets = gaussians.render_differentiable(old.xyz, old.colour, old.covariance(), old.opacity(), mats, cam, (40, 56))[1].detach() * 1.1
    a = gaussians.fit(old, tgt, mats, cam, (40, 56), iters=20, depth_targets=depth_targets, depth_weight=0.05)
    b = gaussians.fit(new, tgt, mats, cam, (40, 56), iters=20, depth_targets=depth_targets, depth_weight=0.05, ssim_weight=0.0)
    assert a == b and len(a) == 20
    for k in gaussians.PARAMETERS:
        assert _bits(getattr(old, k).detach(), getattr(new, k).detach()), k
    with pytest.raises(Exception, match="ssim_weight"):
        gaussians.fit(new, tgt, mats, cam, (40, 56), iters=1, ssim_weight=1.5)


def test_the_fit_with_the_ssim_term_lowers_the_loss_as_the_float64_loop_does(cuda):
    from mudg_amd import gaussians
    start, views, cam, targets = gb.fit_problem()
    mats, tgt = _t(views).to(cuda), targets.to(torch.float32).to(cuda)
    model = _model(cuda, start)
    losses = gaussians.fit(model, tgt, mats, cam, (40, 56), iters=200, ssim_weight=0.2)
    ratio = losses[-1] / losses[0]
    # 2 r64s: fp32 rounding and the hard skip thresholds move an Adam trajectory; r64s is the float64 loop's ratio, measured on the CPU
    print(f"fit at ssim_weight 0.2: loss {losses[0]:.5f} -> {losses[-1]:.5f}, ratio {ratio:.5f} (float64: {R64S}, bound {2 * R64S})")
    assert len(losses) == 200 and ratio <= 2 * R64S


def test_fit_cloud_views_with_the_ssim_term_raises_the_ssim_of_render_cloud_views(cuda):
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
    g = vpr.fit_cloud_views(background, scene, [0, 1], target, 0, hw, 0.1, iters=60, history=history, ssim_weight=0.2)
    after = gaussians.render_scene(g, None, s["intr"], s["c2w"], s["hw_native"], hw, poses=s["c2w"][:, None])["rgb_u8"][0]
    s0, s1 = metrics.psnr_ssim(before, target)["ssim"], metrics.psnr_ssim(after, target)["ssim"]
    print(f"SSIM against the target frames: {s0.tolist()} -> {s1.tolist()} after {len(history)} iterations, loss {history[0]:.4f} -> {history[-1]:.4f}")
    assert len(history) == 60 and bool((s1 > s0).all())
