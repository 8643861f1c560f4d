"""View-dependent colour on the GPU (csrc/gaussians_sh.hip and the three `_views` blends through mudg_amd/ops.py and gaussians.py)
against the CPU definition of DESIGN.md §27 (tests/gaussians_sh_reference.py): torch.equal on the bits of the colours, the images, the
state, the partial buffer and every gradient, since both sides perform the same rounded fp32 operations in the same order; the five
entry points raw inside sentinels; the old path's bits where the harmonics take no part; and the fit against its float64 counterpart.
The shapes are the smallest that can go wrong: 300 Gaussians (two workgroups, a ragged last wave), three views, two matrices a view
with ids, a 40 x 56 image (not whole tiles), Gaussians behind the camera in one view only, colours negative enough to clamp.
The size, active-degree, ids, clamp, guard and batch-edge cases of the raw kernels live in tests/test_gaussians_sh_kernels_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import gaussians_bwd_reference as gb
import gaussians_reference as gr
import gaussians_sh_reference as gs
from sentinel_buffers import Flat
from test_gaussians_sh_cpu import RATIO64

pytestmark = pytest.mark.gpu
F = np.float32
HW = (40, 56)
EINVAL = -1
I32, I64, F32 = torch.int32, torch.int64, torch.float32
CASES = [(1, None), (2, None), (3, None), (3, 1)]                                      # (L, active degree)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _same(got, want, what):
    got, want = got.cpu().reshape(-1), _t(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bits = torch.int32 if got.dtype == torch.float32 else got.dtype
    differ = int((got.view(bits) != want.view(bits)).sum())
    assert differ == 0, f"{what}: {differ} of {got.numel()} elements differ"


@functools.lru_cache(maxsize=None)
def _reference(L, active):
    """The case and the definition's answer, computed once and shared."""
    xyz, colour, sh, cov, op, ids, mats, cam = gs.seeded_case(L)
    V = mats.shape[0]
    rng = np.random.default_rng(5)
    ups = (rng.normal(size=(V, 3) + HW).astype(F), (rng.normal(size=(V,) + HW) * 0.05).astype(F), rng.normal(size=(V,) + HW).astype(F))
    want = gs.render_backward(xyz, colour, sh, cov, op, ids, mats, cam, HW, *ups, active=active)
    return dict(xyz=xyz, colour=colour, sh=sh, cov=cov, op=op, ids=ids, mats=mats, cam=cam, ups=ups), want


def _device(case, cuda):
    d = {k: _t(case[k]).to(cuda) for k in ("colour", "sh", "cov", "op", "ids", "mats")}
    d["xyz"] = _t(case["xyz"]).to(cuda)
    d["pts"] = _t(gr.pack(case["xyz"], np.zeros((len(case["xyz"]), 3), np.uint8))).to(cuda)
    d["ups"] = [_t(u).to(cuda) for u in case["ups"]]
    return d


def _binned(d, cam):
    from mudg_amd import ops
    uv, conic, depth, rect, count = ops.gauss_project(d["pts"], d["cov"], d["op"], d["mats"], cam, HW, ids=d["ids"])
    ends = torch.cumsum(count.reshape(-1), 0, dtype=torch.int64)
    offsets = (ends - count.reshape(-1)).reshape(count.shape)
    E = int(ends[-1])
    keys, values = ops.gauss_keys(depth, rect, count, offsets, E, HW)
    keys, order = torch.sort(keys, stable=True)
    tx, ty = gr.tiles(HW)
    return dict(uv=uv, conic=conic, depth=depth, count=count, offsets=offsets, E=E, values=values[order], order=order,
                ranges=ops.gauss_ranges(keys, d["mats"].shape[0] * tx * ty))


# ------------------------------------------------------------------------------------------------ the kernels against the definition
@pytest.mark.parametrize("L,active", CASES)
def test_the_kernels_are_bit_equal_to_the_definition_and_to_a_repeat(cuda, L, active):
    from mudg_amd import ops
    case, want = _reference(L, active)
    count = want["count"]
    assert ((count[1] == 0) & (count[0] > 0) & (count[2] > 0)).sum() > 10                # dropped by view 1 only
    assert (want["colours"][count > 0] == 0).any() and (want["colours"][count > 0] > 0).any()
    d = _device(case, cuda)
    b = _binned(d, case["cam"])
    _same(b["values"], want["values"], "values")
    _same(b["order"], want["order"], "order")
    runs = []
    for _ in range(2):
        cols = ops.gauss_sh_colour(d["pts"], d["mats"], b["count"], d["colour"], d["sh"], ids=d["ids"], active=active)
        rgb, dimg, alpha, state = ops.gauss_blend_train_views(cols, b["uv"], b["conic"], b["depth"], b["values"], b["ranges"], HW)
        plain = ops.gauss_blend_views(cols, b["uv"], b["conic"], b["depth"], b["values"], b["ranges"], HW)
        partial = ops.gauss_blend_bwd_views(cols, b["uv"], b["conic"], b["depth"], b["values"], b["order"], b["ranges"], HW, state, *d["ups"])
        d_colour, d_sh, d_dir = ops.gauss_sh_bwd(d["pts"], d["mats"], b["count"], b["offsets"], partial, d["colour"], d["sh"], ids=d["ids"],
                                                 active=active)
        for a, c, name in zip(plain, (rgb, dimg, alpha), ("rgb", "depth", "alpha")):
            assert torch.equal(a.view(I32), c.view(I32)), f"gauss_blend_views: {name} differs from the training blend's"
        runs.append(dict(colours=cols, rgb=rgb, depth_image=dimg, alpha=alpha, state=state, partial=partial, d_colour=d_colour, d_sh=d_sh,
                         d_xyz_dir=d_dir))
    for k in runs[0]:
        assert torch.equal(runs[0][k].view(I32), runs[1][k].view(I32)), f"{k}: a repeat run differs"
        _same(runs[0][k], want[k], k)
    assert want["d_sh"].any() and want["d_xyz_dir"].any() and want["d_colour"].any()
    if active is not None:
        Ka = gs.terms(active)
        assert not runs[0]["d_sh"][:, Ka - 1:].any() and not torch.signbit(runs[0]["d_sh"][:, Ka - 1:]).any()


@pytest.mark.parametrize("L,active", [(2, None), (3, 1)])
def test_render_differentiable_with_harmonics_is_the_definition(cuda, L, active):
    from mudg_amd import gaussians
    case, want = _reference(L, active)
    d = _device(case, cuda)
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("xyz", "colour", "cov", "op", "sh")}
    out = gaussians.render_differentiable(leaves["xyz"], leaves["colour"], leaves["cov"], leaves["op"], d["mats"], case["cam"], HW, ids=d["ids"],
                                          sh=leaves["sh"], sh_degree=active)
    for got, name in zip(out, ("rgb", "depth_image", "alpha")):
        _same(got.detach(), want[name], name)
    torch.autograd.backward(out, d["ups"])
    for k, name in (("xyz", "d_xyz"), ("colour", "d_colour"), ("cov", "d_cov"), ("op", "d_opacity"), ("sh", "d_sh")):
        _same(leaves[k].grad, want[name], name)


def test_with_degree_zero_active_the_old_path_returns_the_same_bits(cuda):
    from mudg_amd import gaussians
    case, _ = _reference(3, None)
    d = _device(case, cuda)
    colour = d["colour"].abs()                                                         # not negative: the clamp takes no part
    results = []
    for harmonics in (dict(), dict(sh=d["sh"].clone().requires_grad_(True), sh_degree=0)):
        leaves = {k: t.clone().requires_grad_(True) for k, t in (("xyz", d["xyz"]), ("colour", colour), ("cov", d["cov"]), ("op", d["op"]))}
        out = gaussians.render_differentiable(leaves["xyz"], leaves["colour"], leaves["cov"], leaves["op"], d["mats"], case["cam"], HW, ids=d["ids"],
                                              **harmonics)
        torch.autograd.backward(out, d["ups"])
        results.append([o.detach() for o in out] + [leaves[k].grad for k in ("xyz", "colour", "cov", "op")])
        if harmonics:
            assert not harmonics["sh"].grad.any()
    for a, b, name in zip(*results, ("rgb", "depth", "alpha", "d_xyz", "d_colour", "d_cov", "d_opacity")):
        assert a.any() and torch.equal(a.view(I32), b.view(I32)), name


# ------------------------------------------------------------------------------------------------ the five entry points, raw
def _lib():
    from mudg_amd import hip
    return hip.lib()


def _put(a, dev, dtype):
    t = _t(a).reshape(-1)
    return Flat(t.numel(), dtype, nan=dtype == F32).put(t, dev)


def _call(fn, *args):
    rc = fn(*args, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("L,active", [(1, None), (2, None), (3, 1)])
def test_the_two_harmonics_entry_points_raw_in_sentinels(cuda, L, active):
    case, want = _reference(L, active)
    lib = _lib()
    n, (V, nmat) = len(case["xyz"]), case["mats"].shape[:2]
    rows = gs.terms(L) - 1
    act = L if active is None else active
    E = len(want["partial"])
    ins = dict(pts=_put(gr.pack(case["xyz"], np.zeros((n, 3), np.uint8)), cuda, I32), ids=_put(case["ids"], cuda, I32),
               mats=_put(case["mats"], cuda, F32), count=_put(want["count"], cuda, I32), offsets=_put(want["offsets"], cuda, I64),
               partial=_put(want["partial"], cuda, F32), colour=_put(case["colour"], cuda, F32), sh=_put(case["sh"], cuda, F32))
    colours = Flat(V * n * 3, F32).blank(cuda)
    head = (ins["pts"].ptr, ins["ids"].ptr, n, ins["mats"].ptr, V, nmat, ins["count"].ptr)
    assert _call(lib.mudg_gauss_sh_colour, *head, ins["colour"].ptr, ins["sh"].ptr, L, act, colours.ptr) == 0
    _same(colours.read("colours"), want["colours"], "colours")
    outs = [Flat(n * 3, F32).blank(cuda), Flat(n * rows * 3, F32).blank(cuda), Flat(n * 3, F32).blank(cuda)]
    tail = (ins["offsets"].ptr, ins["partial"].ptr, E, ins["colour"].ptr, ins["sh"].ptr, L, act)
    assert _call(lib.mudg_gauss_sh_bwd, *head, *tail, *[o.ptr for o in outs]) == 0
    for o, name in zip(outs, ("d_colour", "d_sh", "d_xyz_dir")):
        _same(o.read(name), want[name], name)
    for k, b in ins.items():
        b.unchanged(k)
    # refusals: the error code, and not one byte written
    blank = [Flat(V * n * 3, F32).blank(cuda)] + [Flat(n * c, F32).blank(cuda) for c in (3, rows * 3, 3)]
    c_out, b_out = blank[0], blank[1:]
    bad_colour = [
        (None, *head[1:], ins["colour"].ptr, ins["sh"].ptr, L, act, c_out.ptr), (*head, None, ins["sh"].ptr, L, act, c_out.ptr),
        (*head, ins["colour"].ptr, None, L, act, c_out.ptr), (*head, ins["colour"].ptr, ins["sh"].ptr, L, act, None),
        (*head[:6], None, ins["colour"].ptr, ins["sh"].ptr, L, act, c_out.ptr),
        (head[0], None, *head[2:], ins["colour"].ptr, ins["sh"].ptr, L, act, c_out.ptr),                       # two matrices need ids
        (*head[:2], 0, *head[3:], ins["colour"].ptr, ins["sh"].ptr, L, act, c_out.ptr), (*head[:4], 0, *head[5:], ins["colour"].ptr, ins["sh"].ptr, L, act, c_out.ptr),
        (*head[:4], 65536, *head[5:], ins["colour"].ptr, ins["sh"].ptr, L, act, c_out.ptr), (*head[:5], 0, head[6], ins["colour"].ptr, ins["sh"].ptr, L, act, c_out.ptr),
        (*head, ins["colour"].ptr, ins["sh"].ptr, 0, 0, c_out.ptr), (*head, ins["colour"].ptr, ins["sh"].ptr, 4, act, c_out.ptr),
        (*head, ins["colour"].ptr, ins["sh"].ptr, L, L + 1, c_out.ptr), (*head, ins["colour"].ptr, ins["sh"].ptr, L, -1, c_out.ptr),
        (*head, ins["colour"].ptr, ins["sh"].ptr + 4, L, act, c_out.ptr), (head[0] + 4, *head[1:], ins["colour"].ptr, ins["sh"].ptr, L, act, c_out.ptr),
    ]
    for args in bad_colour:
        assert _call(lib.mudg_gauss_sh_colour, *args) == EINVAL, args
    o = [x.ptr for x in b_out]
    bad_bwd = [
        (*head, None, *tail[1:], *o), (*head, tail[0], None, *tail[2:], *o), (*head, *tail[:3], None, *tail[4:], *o), (*head, *tail[:4], None, *tail[5:], *o),
        (*head, *tail, None, o[1], o[2]), (*head, *tail, o[0], None, o[2]), (*head, *tail, o[0], o[1], None),
        (*head, *tail[:2], 0, *tail[3:], *o), (*head, *tail[:2], 2 ** 31, *tail[3:], *o), (*head[:2], 0, *head[3:], *tail, *o),
        (*head, *tail[:5], 0, 0, *o), (*head, *tail[:5], 4, act, *o), (*head, *tail[:5], L, L + 1, *o),
        (*head, *tail, o[0], o[1] + 4, o[2]), (*head, *tail[:4], tail[4] + 4, *tail[5:], *o), (head[0], None, *head[2:], *tail, *o),
    ]
    for args in bad_bwd:
        assert _call(lib.mudg_gauss_sh_bwd, *args) == EINVAL, args
    for x in blank:
        x.unchanged("a refused call's output")


def test_the_three_views_blends_raw_in_sentinels(cuda):
    case, want = _reference(2, None)
    lib = _lib()
    n, V, (H, W) = len(case["xyz"]), case["mats"].shape[0], HW
    E = len(want["partial"])
    ins = dict(colours=_put(want["colours"], cuda, F32), uv=_put(want["uv"], cuda, F32), conic=_put(want["conic"], cuda, F32),
               depth=_put(want["depth"], cuda, F32), values=_put(want["values"], cuda, I32), order=_put(want["order"], cuda, I64),
               ranges=_put(want["ranges"], cuda, I32), state=_put(want["state"], cuda, F32))
    ins.update({f"up{k}": _put(u, cuda, F32) for k, u in enumerate(case["ups"])})
    head = (ins["colours"].ptr, ins["uv"].ptr, ins["conic"].ptr, ins["depth"].ptr, ins["values"].ptr)
    size = (n, E, V, H, W)
    images = lambda: [Flat(V * c * H * W, F32).blank(cuda) for c in (3, 1, 1)]
    a = images()
    assert _call(lib.mudg_gauss_blend_views, *head, ins["ranges"].ptr, *size, *[x.ptr for x in a]) == 0
    b = images() + [Flat(V * 5 * H * W, F32).blank(cuda)]
    assert _call(lib.mudg_gauss_blend_train_views, *head, ins["ranges"].ptr, *size, *[x.ptr for x in b]) == 0
    for outs in (a, b):
        for x, name in zip(outs, ("rgb", "depth_image", "alpha", "state")):
            _same(x.read(name), want[name], name)
    partial = Flat(E * 10, F32).blank(cuda)
    ups = [ins[f"up{k}"].ptr for k in range(3)]
    assert _call(lib.mudg_gauss_blend_bwd_views, *head, ins["order"].ptr, ins["ranges"].ptr, *size, ins["state"].ptr, *ups, partial.ptr) == 0
    _same(partial.read("partial"), want["partial"], "partial")
    for k, x in ins.items():
        x.unchanged(k)
    # refusals
    a, b, partial = images(), images() + [Flat(V * 5 * H * W, F32).blank(cuda)], Flat(E * 10, F32).blank(cuda)
    pa, pb = [x.ptr for x in a], [x.ptr for x in b]
    sizes = [(0, E, V, H, W), (n, 0, V, H, W), (n, 2 ** 31, V, H, W), (n, E, 0, H, W), (n, E, V, 0, W), (n, E, V, H, 0), (2 ** 31, E, V, H, W)]
    for s in sizes:
        assert _call(lib.mudg_gauss_blend_views, *head, ins["ranges"].ptr, *s, *pa) == EINVAL, s
        assert _call(lib.mudg_gauss_blend_train_views, *head, ins["ranges"].ptr, *s, *pb) == EINVAL, s
        assert _call(lib.mudg_gauss_blend_bwd_views, *head, ins["order"].ptr, ins["ranges"].ptr, *s, ins["state"].ptr, *ups, partial.ptr) == EINVAL, s
    for k in range(5):
        nulled = head[:k] + (None,) + head[k + 1:]
        assert _call(lib.mudg_gauss_blend_views, *nulled, ins["ranges"].ptr, *size, *pa) == EINVAL
        assert _call(lib.mudg_gauss_blend_train_views, *nulled, ins["ranges"].ptr, *size, *pb) == EINVAL
        assert _call(lib.mudg_gauss_blend_bwd_views, *nulled, ins["order"].ptr, ins["ranges"].ptr, *size, ins["state"].ptr, *ups, partial.ptr) == EINVAL
    assert _call(lib.mudg_gauss_blend_views, *head, None, *size, *pa) == EINVAL
    assert _call(lib.mudg_gauss_blend_views, *head, ins["ranges"].ptr, *size, pa[0], None, pa[2]) == EINVAL
    assert _call(lib.mudg_gauss_blend_train_views, *head, ins["ranges"].ptr, *size, *pb[:3], None) == EINVAL     # training needs the state
    assert _call(lib.mudg_gauss_blend_bwd_views, *head, None, ins["ranges"].ptr, *size, ins["state"].ptr, *ups, partial.ptr) == EINVAL
    assert _call(lib.mudg_gauss_blend_bwd_views, *head, ins["order"].ptr, ins["ranges"].ptr, *size, None, *ups, partial.ptr) == EINVAL
    assert _call(lib.mudg_gauss_blend_bwd_views, *head, ins["order"].ptr, ins["ranges"].ptr, *size, ins["state"].ptr, *ups, None) == EINVAL
    assert _call(lib.mudg_gauss_blend_views, head[0], head[1] + 4, *head[2:], ins["ranges"].ptr, *size, *pa) == EINVAL   # uv is 8-byte aligned
    for x in a + b + [partial]:
        x.unchanged("a refused call's output")


# ------------------------------------------------------------------------------------------------ inference
def test_render_with_harmonics_equals_the_definition_at_two_poses(cuda):
    from mudg_amd import gaussians
    from mudg_amd.render import PointCloud
    case, _ = _reference(3, None)
    d = _device(case, cuda)
    xyz, cov, op, ids, cam = (case[k] for k in ("xyz", "cov", "op", "ids", "cam"))
    mats = np.ascontiguousarray(case["mats"][[0, 2]])
    g = gaussians.Gaussians(PointCloud(d["pts"]), d["cov"], d["op"], d["ids"], sh=d["sh"], colour=d["colour"])
    out = gaussians.render(g, _t(mats).to(cuda), cam, HW)
    proj = gr.project(xyz, cov, op, ids, mats, cam, HW)
    keys, values, order, ranges, offsets = gb.bin_with_order(proj, HW)
    cols = gs.colours(xyz, ids, mats, proj["count"], case["colour"], case["sh"])
    rgb, depth, alpha, _ = gs.blend_views(proj, cols, values, ranges, HW)
    for k, w in (("rgb", rgb), ("depth", depth), ("alpha", alpha)):
        _same(out[k], w, k)
    flat = gaussians.render(gaussians.Gaussians(PointCloud(d["pts"]), d["cov"], d["op"], d["ids"]), _t(mats).to(cuda), cam, HW)
    assert not torch.equal(flat["rgb"], out["rgb"]) and torch.equal(flat["alpha"].view(I32), out["alpha"].view(I32))
    with pytest.raises(Exception, match="comes with sh"):
        gaussians.Gaussians(PointCloud(d["pts"]), d["cov"], d["op"], d["ids"], colour=d["colour"])


# ------------------------------------------------------------------------------------------------ the fit
def _model(cuda, start, **kw):
    from mudg_amd import gaussians
    return gaussians.GaussianModel(*[_t(start[k]).to(cuda) for k in gaussians.PARAMETERS], **kw)


def test_the_fit_gains_from_harmonics_what_the_float64_fit_gains(cuda):
    from mudg_amd import gaussians
    start, views, cam, targets = gs.fit_problem()
    mats, tgt = _t(views).to(cuda), targets.to(torch.float32).to(cuda)
    flat, lit = _model(cuda, start), _model(cuda, start)
    a = gaussians.fit(flat, tgt, mats, cam, gs.FIT_HW, iters=gs.FIT_ITERS)
    b = gaussians.fit(lit, tgt, mats, cam, gs.FIT_HW, iters=gs.FIT_ITERS, sh_degree=2)
    ratio = b[-1] / a[-1]
    print(f"fp32 fits, {gs.FIT_ITERS} steps from {a[0]:.5f}: L = 0 ends at {a[-1]:.5f}, L = 2 at {b[-1]:.5f}, ratio {ratio:.4f} (float64: {RATIO64})")
    assert a[0] == b[0] and flat.sh is None and tuple(lit.sh.shape) == (len(lit), 8, 3) and "sh" in lit.parameters()
    assert abs(ratio / RATIO64 - 1) <= 0.10, (ratio, RATIO64)
    g = lit.gaussians()                                                                # the result renders: the unrounded coefficients travel
    assert torch.equal(g.sh, lit.sh.detach()) and torch.equal(g.colour, lit.colour.detach())
    out = gaussians.render(g, mats, cam, gs.FIT_HW)["rgb"]
    assert float((out - tgt).abs().mean()) < 1.5 * b[-1]


def test_without_harmonics_the_fit_is_the_fit_it_was_and_the_degree_rises_on_schedule(cuda):
    from mudg_amd import gaussians, hip
    start, views, cam, targets = gs.fit_problem()
    mats, tgt = _t(views).to(cuda), targets.to(torch.float32).to(cuda)
    plain, keyword = _model(cuda, start), _model(cuda, start)
    a = gaussians.fit(plain, tgt, mats, cam, gs.FIT_HW, iters=6)
    b = gaussians.fit(keyword, tgt, mats, cam, gs.FIT_HW, iters=6, sh_degree=0, sh_raise_every=3)
    assert a == b and keyword.sh is None and tuple(keyword.parameters()) == gaussians.PARAMETERS
    for k in gaussians.PARAMETERS:
        assert torch.equal(getattr(plain, k).view(I32), getattr(keyword, k).view(I32)), k
    waits = _model(cuda, start)
    gaussians.fit(waits, tgt, mats, cam, gs.FIT_HW, iters=3, sh_degree=2, sh_raise_every=3)
    assert waits.sh is not None and not waits.sh.any()                                 # the active degree is still 0
    gaussians.fit(waits, tgt, mats, cam, gs.FIT_HW, iters=4, sh_degree=2, sh_raise_every=3)
    assert waits.sh[:, :3].any() and not waits.sh[:, 3:].any()                         # iteration 3 reaches degree 1, degree 2 waits for 6
    with pytest.raises(hip.MudgError, match="harmonics of degree 2"):
        gaussians.fit(waits, tgt, mats, cam, gs.FIT_HW, iters=1)
    with pytest.raises(hip.MudgError, match="harmonics of degree 2"):
        gaussians.fit(waits, tgt, mats, cam, gs.FIT_HW, iters=1, sh_degree=3)


def test_density_control_carries_the_coefficients_and_their_moments(cuda):
    from mudg_amd import gaussians, ops
    start, views, cam, targets = gs.fit_problem()
    mats, tgt = _t(views).to(cuda), targets.to(torch.float32).to(cuda)
    model = _model(cuda, start)
    control = gaussians.DensityControl(2, 12, 5, split_scale=0.15, max_scale=2.0, max_gaussians=2000)
    losses = gaussians.fit(model, tgt, mats, cam, gs.FIT_HW, iters=14, sh_degree=2, density=control)
    assert len(losses) == 14 and len(control.history) == 2
    assert tuple(model.sh.shape) == (len(model), 8, 3) and len(model) == control.history[-1]["after"] and model.sh.any()
    # one step by hand: every Gaussian's coefficients and moments name it, so the rows say where they came from
    n = len(model)
    tag = torch.arange(1, n + 1, dtype=torch.float32, device=cuda)
    with torch.no_grad():
        model.sh.copy_(tag[:, None, None].expand(n, 8, 3))
    moments = {"sh": (model.sh.detach() * 2, model.sh.detach() * 3)}
    stats = gaussians.DensityStats(n, cuda)
    stats.grad_sum[::3] = 1.0
    stats.seen[:] = 1
    action, rows = ops.gauss_density_plan(stats.grad_sum, stats.seen, model.opacity().detach().contiguous(), torch.exp(model.log_scale.detach()).contiguous(),
                                          grad_threshold=control.grad_threshold, split_scale=control.split_scale, min_opacity=control.min_opacity,
                                          max_scale=control.max_scale, grow=True)
    counts = gaussians.densify_and_prune(model, stats, moments, gaussians.DensityControl(0, 1, 1, split_scale=0.15, max_scale=2.0))
    assert counts["cloned"] > 0 and counts["split"] > 0 and counts["kept"] > 0
    sh, (m, v) = model.sh.detach(), moments["sh"]
    assert sh.requires_grad is False and model.sh.requires_grad and tuple(sh.shape) == (counts["after"], 8, 3) == tuple(m.shape) == tuple(v.shape)
    parent = sh[:, 0, 0].to(torch.int64) - 1
    assert torch.equal(sh, (parent + 1).to(torch.float32)[:, None, None].expand_as(sh))
    assert bool((parent[1:] >= parent[:-1]).all())                                     # survivors in order, children adjacent
    assert torch.equal(torch.bincount(parent, minlength=n).to(torch.int32), rows)
    first = torch.ones_like(parent, dtype=torch.bool)
    first[1:] = parent[1:] != parent[:-1]
    act = action[parent]
    carries = (act == ops.GAUSS_KEEP) | ((act == ops.GAUSS_CLONE) & first)
    assert torch.equal(m, torch.where(carries[:, None, None], sh * 2, torch.zeros_like(sh)))
    assert torch.equal(v, torch.where(carries[:, None, None], sh * 3, torch.zeros_like(sh)))
