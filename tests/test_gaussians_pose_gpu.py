"""The pose gradient of DESIGN.md §28 on the GPU: mudg_gauss_pose_bwd and mudg_gauss_sh_pose_bwd raw against the numpy definition
(tests/gaussians_pose_reference.py), the matrices' gradient through render_differentiable, and fit(..., poses=).

Raw calls: every input sits in a NaN-filled (integers: sentinel-filled) allocation and is compared with itself after each call; the stage
buffer and d_mats sit in NaN-filled allocations of exactly their size, so the entry must clear or overwrite all it reads and write nothing
else.  Every comparison is torch.equal on the bits with no element left out: the definition performs the kernels' rounded fp32 operations
in the kernels' order, the order of the sum over the Gaussians included.  Each call is made twice and must give the same bits."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gaussians_bwd_reference as gb
import gaussians_pose_reference as gp
import gaussians_reference as gr
import gaussians_sh_reference as gs
from sentinel_buffers import Flat

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
I32, I64, F32 = torch.int32, torch.int64, torch.float32


def _t(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


def _lib():
    from mudg_amd import hip
    return hip.lib()


def _put(a, dev, dtype):
    t = _t(a).reshape(-1)
    return Flat(t.numel(), dtype, nan=dtype == F32).put(t, dev)


def _bits(t):
    return t.view(I32) if t.dtype == F32 else t


def _same(got, want, what):
    got, want = _t(got).reshape(-1), _t(want).reshape(-1)
    assert got.dtype == want.dtype == F32 and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    differ = int((_bits(got) != _bits(want)).sum())
    assert differ == 0 and torch.equal(_bits(got), _bits(want)), f"{what}: {differ} of {got.numel()} elements differ"


def _plus_zero(got, what):
    got = _t(got).reshape(-1)
    assert torch.equal(_bits(got), torch.zeros(got.numel(), dtype=I32)), f"{what}: not +0 everywhere"


def _pack(xyz):
    xyz = np.ascontiguousarray(xyz, dtype=F)
    return np.concatenate([xyz.view(np.int32), np.zeros((len(xyz), 1), np.int32)], axis=1)


def _raw(cuda, c, views=None):
    """mudg_gauss_pose_bwd (and, with c.sh, mudg_gauss_sh_pose_bwd) on a case, twice, in sentinels -> d_mats (d_mats_dir) (V, nmat, 12) on
    the CPU.  views: a slice of the case's views (count and offsets rows go with the matrices; the partials stay whole)."""
    lib = _lib()
    sl = slice(None) if views is None else views
    mats, count, offsets = c.mats[sl], c.count[sl], c.offsets[sl]
    V, nmat = mats.shape[:2]
    n, E = len(c.xyz), len(c.partial)
    H, W = c.hw
    ins = dict(pts=_put(_pack(c.xyz), cuda, I32), cov=_put(c.cov, cuda, F32), mats=_put(mats, cuda, F32), count=_put(count, cuda, I32),
               offsets=_put(offsets, cuda, I64), partial=_put(c.partial, cuda, F32))
    if c.ids is not None:
        ins["ids"] = _put(c.ids, cuda, I32)
    ids = ins["ids"].ptr if c.ids is not None else None
    sizes = [V * nmat * ((n + 255) // 256) * 12, V * nmat * 12]
    calls = {"d_mats": lambda stage, out: lib.mudg_gauss_pose_bwd(ins["pts"].ptr, ins["cov"].ptr, ids, n, ins["mats"].ptr, V, nmat, H, W, *c.cam,
                                                                 float(gr.ZNEAR), float(gr.ZFAR), ins["count"].ptr, ins["offsets"].ptr, ins["partial"].ptr, E,
                                                                 stage, out, None)}
    if getattr(c, "sh", None) is not None:
        ins.update(colour=_put(c.colour, cuda, F32), sh=_put(c.sh, cuda, F32))
        L = gs.degree_of(c.sh)
        calls["d_mats_dir"] = lambda stage, out: lib.mudg_gauss_sh_pose_bwd(ins["pts"].ptr, ids, n, ins["mats"].ptr, V, nmat, ins["count"].ptr,
                                                                            ins["offsets"].ptr, ins["partial"].ptr, E, ins["colour"].ptr,
                                                                            ins["sh"].ptr, L, L if c.active is None else c.active, stage, out, None)
    got = SimpleNamespace()
    for name, call in calls.items():
        runs = []
        for _ in range(2):
            stage, out = (Flat(size, F32, nan=True).blank(cuda) for size in sizes)           # NaN: what the entry reads it must have written
            assert call(stage.ptr, out.ptr) == 0, lib.mudg_last_error()
            torch.cuda.synchronize()
            for k, b in ins.items():
                b.unchanged(k)
            assert not torch.isnan(stage.read(f"{name}: stage")).any(), f"{name}: the stage buffer was not cleared"
            runs.append(out.read(name))
        assert torch.equal(_bits(runs[0]), _bits(runs[1])), f"{name}: a repeat run differs"
        setattr(got, name, runs[0].reshape(V, nmat, 12))
    return got


def _definition(c):
    want = SimpleNamespace(d_mats=gp.pose_bwd(c.xyz, c.cov, c.ids, c.mats, c.cam, c.hw, c.count, c.offsets, c.partial))
    if getattr(c, "sh", None) is not None:
        want.d_mats_dir = gp.sh_pose_bwd(c.xyz, c.ids, c.mats, c.count, c.offsets, c.partial, c.colour, c.sh, c.active)
    for k, v in vars(want).items():
        assert np.isfinite(v).all(), k                                                        # bits of a NaN are nobody's promise
    return want


def _is_the_definition(got, want, what):
    assert vars(got).keys() == vars(want).keys()
    for k in vars(got):
        _same(getattr(got, k), getattr(want, k), f"{what}: {k}")


def _three_views(mats):
    views = np.repeat(mats, 3, axis=0).copy()
    views[1, 0, 3] += F(0.3)
    views[2, 0, 3] -= F(0.3)
    return views


# ------------------------------------------------------------------------------------------------ direct calls on real partials
def _partials(cuda, xyz, colour, cov, opacity, ids, mats, cam, hw, seed=5):
    """The product's own forward and blend backward on a scene with seeded upstream gradients: count, offsets, partial on the CPU."""
    from mudg_amd import gaussians, ops
    dev = lambda a, dt=None: _t(np.ascontiguousarray(a)).to(cuda)
    pts, col = dev(_pack(xyz)), dev(np.asarray(colour, dtype=F))
    m = dev(mats)
    b = gaussians._bin("test", pts, dev(cov), dev(opacity), m, cam, hw, None if ids is None else dev(ids), gr.ZNEAR, gr.ZFAR, 2 ** 28)
    assert b.entries > 0
    state = ops.gauss_blend_train(col, b.uv, b.conic, b.depth, b.values, b.ranges, hw)[3]
    ups = [dev(u) for u in gp.upstream(mats.shape[0], hw, seed)]
    partial = ops.gauss_blend_bwd(col, b.uv, b.conic, b.depth, b.values, b.order, b.ranges, hw, state, *ups)
    return b.count.cpu().numpy(), b.offsets.cpu().numpy(), partial.cpu().numpy()


@pytest.mark.parametrize("hw", ((1, 1), (17, 33), (40, 56)))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 513))
def test_real_partials_at_sizes_around_a_chunk_and_images_that_are_no_whole_tiles(cuda, n, hw):
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene(n, hw, 7)
    mats = _three_views(mats)[:2]
    count, offsets, partial = _partials(cuda, xyz, rgb, cov, opacity, None, mats, cam, hw)
    c = SimpleNamespace(xyz=xyz, cov=cov, ids=None, mats=mats, cam=cam, hw=hw, count=count, offsets=offsets, partial=partial)
    want = _definition(c)
    _is_the_definition(_raw(cuda, c), want, f"n = {n}, {hw[0]} x {hw[1]}")
    assert n == 1 or want.d_mats.any(axis=2).all()                                           # one Gaussian alone may leave its pixels unblended


# ------------------------------------------------------------------------------------------------ direct calls on synthetic tables
def _synthetic(n, V, nmat, seed, ids):
    """gr.seeded_scene's Gaussians (full covariances) in V views of nmat matrices (the camera's, then objects turned and moved), every
    (view, Gaussian) with one partial row of its own: count 1, offsets arange, a seeded partial."""
    hw = (40, 56)
    xyz, _, cov, _, mats, cam = gr.seeded_scene(n, hw, seed)
    rng = np.random.default_rng(seed + 1)
    cov = cov + (rng.uniform(-0.3, 0.3, (n, 1)) * cov[:, :1] * np.array([[0, 1, 1, 0, 1, 0]])).astype(F)     # off-diagonal, still positive definite
    base = np.concatenate([mats[0, 0].astype(D).reshape(3, 4), [[0, 0, 0, 1]]])
    table = np.zeros((V, nmat, 12), F)
    for v in range(V):
        camera = base.copy()
        camera[0, 3] += 0.3 * v
        for o in range(nmat):
            angle = 0.1 * o * (-1) ** o
            obj = np.eye(4)
            obj[:3, :3] = [[np.cos(angle), -np.sin(angle), 0], [np.sin(angle), np.cos(angle), 0], [0, 0, 1]]
            obj[:3, 3] = (0.1 * o, -0.05 * o, 0.2 * o)
            table[v, o] = (camera @ obj)[:3].reshape(12)
    return SimpleNamespace(xyz=xyz, cov=cov.astype(F), ids=ids, mats=table, cam=cam, hw=hw, count=np.ones((V, n), np.int32),
                           offsets=np.arange(V * n, dtype=np.int64).reshape(V, n), partial=rng.normal(size=(V * n, gb.SUMS)).astype(F))


def test_sixty_five_thousand_gaussians_wrap_the_finishing_lanes_with_every_id_in_every_chunk(cuda):
    n = 65537                                                                                # 257 chunks; the last holds one live lane
    c = _synthetic(n, 2, 3, 31, (np.arange(n) % 3).astype(np.int32))
    want = _definition(c)
    _is_the_definition(_raw(cuda, c), want, "n = 65537, V = 2, nmat = 3")
    assert want.d_mats.any(axis=2).all()
    last = gp.chunk_sums(np.ones((n, 1), F), np.arange(n) % 3 == (n - 1) % 3)
    assert len(last) == 257 and last[256, 0] == 1


def test_ids_out_of_range_an_idle_id_a_hidden_object_a_culled_view_spoiled_tables_and_the_clamped_jacobian(cuda):
    n, V, nmat = 1000, 3, 5
    rng = np.random.default_rng(32)
    ids = rng.choice(np.array([-7, 0, 1, 3, 4, 9], np.int32), n)                             # -7 -> 0, 9 -> 4; nobody holds 2
    ids[:300] = np.sort(ids[:300])                                                           # some chunks with runs, as from_scene lays them out
    c = _synthetic(n, V, nmat, 33, ids)
    c.mats[:, 1] = 0                                                                         # a hidden object: zc = 0 is outside the depth range
    c.mats[2, :, 8:11] *= -1                                                                 # view 2 looks away: everything behind it
    c.mats[2, :, 11] = -1.0
    c.count[0, 10:14], c.count[0, 14] = 0, -3                                                # not drawn
    c.count[1, 20] = 2 ** 30                                                                 # more rows than the buffer has
    c.offsets[0, 30], c.offsets[0, 31], c.offsets[1, 32] = -1, V * n, 2 ** 40                # outside [0, E - count]
    far = np.arange(40, n, 97)
    c.xyz[far, 0] = c.xyz[far, 2] * F(1.2)                                                   # |x / z| beyond 1.3 x the half image: kx != qx
    want = _definition(c)
    got = _raw(cuda, c)
    _is_the_definition(got, want, "the spoiled case")
    clipped = SimpleNamespace(**{**vars(c), "ids": np.clip(ids, 0, nmat - 1)})
    _same(_raw(cuda, clipped).d_mats, got.d_mats, "ids clipped by the caller")
    _plus_zero(got.d_mats[:, 2], "the id nobody holds")
    _plus_zero(got.d_mats[:, 1], "the hidden object's zero matrix")
    _plus_zero(got.d_mats[2], "the view in which everything is culled")
    assert got.d_mats[:2][:, [0, 3, 4]].any(dim=2).all()
    m = c.mats[0][np.clip(ids, 0, nmat - 1)][far]                                            # the clamp's branch ran in the definition
    with np.errstate(all="ignore"):
        q = ((m[:, 0] * c.xyz[far, 0] + m[:, 1] * c.xyz[far, 1]) + m[:, 2] * c.xyz[far, 2] + m[:, 3]) / \
            ((m[:, 8] * c.xyz[far, 0] + m[:, 9] * c.xyz[far, 1]) + m[:, 10] * c.xyz[far, 2] + m[:, 11])
    assert (np.abs(q[ids[far] != 1]) > 1.3 * 0.5 * 56 / 48).any()
    skipped = SimpleNamespace(**vars(c))                                                     # the spoiled pairs are skipped, not clamped
    skipped.count = c.count.copy()
    skipped.count[0, [30, 31]] = skipped.count[1, [20, 32]] = 0
    _same(_raw(cuda, skipped).d_mats, got.d_mats, "spoiled pairs against pairs that are not drawn")


def test_three_views_in_one_call_equal_three_one_view_calls(cuda):
    n = 513
    c = _synthetic(n, 3, 2, 34, (np.arange(n) % 2).astype(np.int32))
    whole = _raw(cuda, c).d_mats
    for v in range(3):
        _same(_raw(cuda, c, slice(v, v + 1)).d_mats[0], whole[v], f"view {v} alone")
    one = _synthetic(n, 1, 1, 35, None)                                                      # one matrix, no ids: one reduction a chunk
    _is_the_definition(_raw(cuda, one), _definition(one), "nmat = 1 without ids")


# ------------------------------------------------------------------------------------------------ harmonics
@pytest.mark.parametrize("L,active", ((1, 0), (1, 1), (2, 1), (2, 2), (3, 2), (3, 3)))
def test_the_directions_share_at_every_degree_and_active_degree(cuda, L, active):
    n = 257
    xyz, colour, sh, cov, opacity, ids, mats, cam = gs.seeded_case(L, n)
    rng = np.random.default_rng(40 + L)
    V = mats.shape[0]
    count = np.ones((V, n), np.int32)
    count[1, 100:110] = 0
    c = SimpleNamespace(xyz=xyz, cov=cov, ids=ids, mats=mats, cam=cam, hw=(40, 56), count=count, colour=colour, sh=sh, active=active,
                        offsets=np.arange(V * n, dtype=np.int64).reshape(V, n), partial=rng.normal(size=(V * n, gb.SUMS)).astype(F))
    want = _definition(c)
    got = _raw(cuda, c)
    _is_the_definition(got, want, f"L = {L}, active = {active}")
    if active == 0:
        _plus_zero(got.d_mats_dir, "no active degree: the direction has no say")
    else:
        assert want.d_mats_dir.any(axis=2).all()


# ------------------------------------------------------------------------------------------------ through autograd
def _differentiable(cuda, case, mats_grad=True, active=None):
    """render_differentiable on a gp case with gp.upstream as the images' gradients -> the leaves (with .grad) by name."""
    from mudg_amd import gaussians
    leaf = lambda a: _t(np.asarray(a, dtype=F)).to(cuda).requires_grad_(True)
    t = SimpleNamespace(xyz=leaf(case["xyz"]), colour=leaf(case["colour"]), cov=leaf(case["cov"]), opacity=leaf(case["opacity"]),
                        mats=_t(case["mats"]).to(cuda).requires_grad_(mats_grad), sh=None if case["sh"] is None else leaf(case["sh"]))
    ids = None if case["ids"] is None else _t(case["ids"]).to(cuda)
    extra = {} if t.sh is None else dict(sh=t.sh, sh_degree=active)
    out = gaussians.render_differentiable(t.xyz, t.colour, t.cov, t.opacity, t.mats, case["cam"], case["hw"], ids=ids, **extra)
    torch.autograd.backward(out, [_t(u).to(cuda) for u in gp.upstream(case["mats"].shape[0], case["hw"])])
    return t


@pytest.mark.parametrize("name", ("scene", "three", "sh"))
def test_mats_grad_is_the_direct_calls_and_the_whole_numpy_chain(cuda, name):
    case = {"scene": gp.case_scene, "three": gp.case_three, "sh": gp.case_sh}[name]()
    t = _differentiable(cuda, case)
    assert t.mats.grad is not None and tuple(t.mats.grad.shape) == case["mats"].shape     # fails without §28: the matrices got no gradient
    want = gp.case_backward(case)
    _same(t.mats.grad.cpu(), want["d_mats"], f"{name}: mats.grad against the numpy chain")
    _same(t.xyz.grad.cpu(), want["d_xyz"], f"{name}: d_xyz beside it")
    c = SimpleNamespace(xyz=case["xyz"], cov=case["cov"], ids=case["ids"], mats=case["mats"], cam=case["cam"], hw=case["hw"], count=want["count"],
                        offsets=want["offsets"], partial=want["partial"], colour=case["colour"], sh=case["sh"], active=None)
    raw = _raw(cuda, c)
    direct = raw.d_mats if case["sh"] is None else raw.d_mats + raw.d_mats_dir
    _same(t.mats.grad.cpu(), direct, f"{name}: mats.grad against the raw calls")
    truth = gp.case_truth(case)
    gap = float(np.abs(t.mats.grad.cpu().numpy().astype(D) - truth).max() / np.abs(truth).max())
    print(f"{name}: mats.grad against float64 autograd {gap:.3g} (bound {gp.GAP_BOUND:.3g})")
    assert gap <= gp.GAP_BOUND


def test_matrices_that_ask_for_no_gradient_launch_nothing_new_and_change_no_bit(cuda, monkeypatch):
    from mudg_amd import ops
    case = gp.case_sh()
    asked = _differentiable(cuda, case)
    launched = []
    for fn in ("gauss_pose_bwd", "gauss_sh_pose_bwd"):
        monkeypatch.setattr(ops, fn, lambda *a, _fn=fn, **k: launched.append(_fn))
    plain = _differentiable(cuda, case, mats_grad=False)
    assert launched == [] and plain.mats.grad is None
    for k in ("xyz", "colour", "cov", "opacity", "sh"):
        _same(getattr(plain, k).grad.cpu(), getattr(asked, k).grad.cpu(), f"{k}.grad with and without the matrices' gradient")


def test_a_call_that_draws_nothing_gives_zero_mats_grad(cuda):
    case = gp.case_three()
    case["mats"] = case["mats"].copy()
    case["mats"][:, :, 11] = F(500.0)                                                       # everything beyond zfar
    t = _differentiable(cuda, case)
    _plus_zero(t.mats.grad.cpu(), "mats.grad")
    assert tuple(t.mats.grad.shape) == case["mats"].shape
    _plus_zero(t.xyz.grad.cpu(), "xyz.grad")


# ------------------------------------------------------------------------------------------------ the fit
def _truth_model(cuda, scene):
    from mudg_amd import gaussians
    xyz, rgb, cov, opacity = scene
    n = len(xyz)
    quat = np.zeros((n, 4), F)
    quat[:, 0] = 1
    logit = (np.log(opacity.astype(D)) - np.log1p(-opacity.astype(D))).astype(F)
    parts = (xyz, rgb, np.repeat(np.log(np.sqrt(cov[:, :1])), 3, axis=1).astype(F), quat, logit)
    return gaussians.GaussianModel(*[_t(np.ascontiguousarray(p, dtype=F)).to(cuda) for p in parts])


def _full(m):
    return np.concatenate([np.asarray(m, dtype=D).reshape(3, 4), [[0, 0, 0, 1]]])


def test_pose_only_registration_converges_as_the_float64_loop_does(cuda):
    from mudg_amd import gaussians, hip
    scene, truth, start, cam, targets = gp.pose_fit_problem()
    model = _truth_model(cuda, scene)
    before = {k: v.detach().clone() for k, v in model.parameters().items()}
    tgt, mats = targets.to(torch.float32).to(cuda), _t(start).to(cuda)
    with pytest.raises(hip.MudgError, match="trainable"):
        gaussians.fit(model, tgt, mats, cam, gp.POSE_FIT_HW, iters=1, trainable=())        # nothing moves: refused without poses
    poses = gaussians.CameraPoses(3, fixed=(0,), device=cuda)
    losses = gaussians.fit(model, tgt, mats, cam, gp.POSE_FIT_HW, iters=gp.POSE_FIT_ITERS, lr={"pose": gp.POSE_FIT_RATE}, trainable=(), poses=poses)
    ratio = losses[-1] / losses[0]
    # 2 R64: fp32 rounding and the hard skip thresholds move an Adam trajectory; R64 is the float64 loop's ratio, measured on the CPU
    print(f"pose fit: loss {losses[0]:.6f} -> {losses[-1]:.6f}, ratio {ratio:.5f} (float64: {gp.R64}, bound {2 * gp.R64})")
    assert len(losses) == gp.POSE_FIT_ITERS and all(np.isfinite(losses))
    assert ratio <= 2 * gp.R64
    for k, v in model.parameters().items():
        assert torch.equal(v.detach(), before[k]), f"{k} moved in a pose-only fit"
    assert not poses.twist[0].any() and poses.twist[1:].detach().abs().sum(1).min() > 0
    fitted = poses.world_to_camera(np.stack([_full(m[0]) for m in start]))
    for v in (1, 2):
        c0, a0 = gp.pose_error(start[v, 0], truth[v, 0])
        c1, a1 = gp.pose_error(fitted[v, :3], truth[v, 0])
        print(f"view {v}: centre {1e3 * c0:.1f} -> {1e3 * c1:.2f} mm, angle {1e3 * a0:.2f} -> {1e3 * a1:.3f} mrad")
        assert c1 < c0 / 10 and a1 < a0 / 10


def _fit_problem_model(cuda):
    from mudg_amd import gaussians
    start, views, cam, targets = gb.fit_problem()
    model = gaussians.GaussianModel(*[_t(start[k]).to(cuda) for k in gaussians.PARAMETERS])
    return model, targets.to(torch.float32).to(cuda), _t(views).to(cuda), cam


def test_a_joint_fit_runs_and_keeps_the_fixed_view(cuda):
    from mudg_amd import gaussians
    model, tgt, mats, cam = _fit_problem_model(cuda)
    poses = gaussians.CameraPoses(3, fixed=(0,), device=cuda)
    losses = gaussians.fit(model, tgt, mats, cam, (40, 56), iters=30, poses=poses)
    assert len(losses) == 30 and all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert not poses.twist[0].any() and poses.twist[1:].detach().abs().sum(1).min() > 0
    assert all(torch.isfinite(p).all() for p in model.parameters().values()) and torch.isfinite(poses.twist).all()


def test_poses_none_is_the_fit_without_the_keyword_bit_for_bit(cuda):
    from mudg_amd import gaussians
    runs = []
    for kw in ({}, {"poses": None}):
        model, tgt, mats, cam = _fit_problem_model(cuda)
        losses = gaussians.fit(model, tgt, mats, cam, (40, 56), iters=10, **kw)
        runs.append((losses, {k: v.detach().cpu() for k, v in model.parameters().items()}))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        _same(runs[0][1][k], runs[1][1][k], k)
