"""The reference of DESIGN.md §28 (tests/gaussians_pose_reference.py) checked on the CPU before anything trusts it: the fp32 rule of the
matrices' gradient lies within a measured distance of float64 autograd, the order of its sum is what the rule says, CameraPoses.apply is
a matrix exponential on the left, and the float64 registration converges as recorded.  The ABI of the two new entry points and the
host-side refusals of the new interface are here too."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import gaussians_bwd_reference as gb
import gaussians_pose_reference as gp

F, D = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("mudg_gauss_pose_bwd", 22), ("mudg_gauss_sh_pose_bwd", 17))


# ------------------------------------------------------------------------------------------------ the rule against float64 autograd
@pytest.fixture(scope="module", params=("scene", "three", "sh"))
def measured(request):
    case = {"scene": gp.case_scene, "three": gp.case_three, "sh": gp.case_sh}[request.param]()
    return request.param, case, gp.case_backward(case), gp.case_truth(case)


def test_the_fp32_rule_lies_within_the_measured_gap_of_float64_autograd(measured):
    name, case, out, truth = measured
    assert out["d_mats"].dtype == F and out["d_mats"].shape == case["mats"].shape == truth.shape
    scale = np.abs(truth).max()
    gap = float(np.abs(out["d_mats"].astype(D) - truth).max() / scale)
    print(f"{name}: largest |d_mats| {scale:.4g}, fp32 rule against float64 {gap:.3g} (bound {gp.GAP_BOUND:.3g})")
    assert scale > 1.0 and gap <= gp.GAP_BOUND


def test_every_matrix_of_every_view_gets_a_gradient_of_its_own(measured):
    _, case, out, truth = measured
    per_matrix = np.abs(truth).max(axis=2)
    assert (per_matrix > 1e-3 * per_matrix.max()).all()                              # no matrix of these cases is idle: the gap test covers each
    if case["sh"] is not None:
        assert np.abs(out["d_mats_dir"]).max() > 1e-3 * np.abs(out["d_mats"]).max()  # and the direction's share is not rounding noise


def test_the_float64_route_through_camera_space_is_the_direct_call():
    c = gp.case_three()
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=F).astype(D))
    scene = tuple(t64(c[k]) for k in ("xyz", "colour", "cov", "opacity"))
    with torch.no_grad():
        direct = gb.textbook(*scene, c["mats"], c["cam"], c["hw"], c["ids"])
        through = gp.textbook_through(t64(c["mats"]), *scene, c["cam"], c["hw"], c["ids"])
    for a, b in zip(direct, through):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))


def test_the_float64_gradient_matches_central_differences():
    c = gp.case_scene(n=60, hw=(24, 40))
    ups = gp.upstream(1, c["hw"])
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=F).astype(D))
    scene = tuple(t64(c[k]) for k in ("xyz", "colour", "cov", "opacity"))
    u = tuple(t64(a) for a in ups)

    def loss(m):
        with torch.no_grad():
            rgb, depth, alpha = gb.textbook(*scene, m, c["cam"], c["hw"])
        return float((rgb * u[0]).sum() + (depth * u[1]).sum() + (alpha * u[2]).sum())

    truth = gp.textbook_mats_grad(c["xyz"], c["colour"], c["cov"], c["opacity"], None, c["mats"], c["cam"], c["hw"], *ups)
    base = c["mats"].astype(D)
    for k in (0, 3, 6, 9, 11):
        h = 1e-6
        hi, lo = base.copy(), base.copy()
        hi[0, 0, k] += h
        lo[0, 0, k] -= h
        fd = (loss(hi) - loss(lo)) / (2 * h)
        assert abs(fd - truth[0, 0, k]) <= 1e-5 * np.abs(truth).max(), (k, fd, truth[0, 0, k])


# ------------------------------------------------------------------------------------------------ the order of the sum
def test_the_sum_over_gaussians_has_the_rules_order():
    rng = np.random.default_rng(0)
    n = 256 * 257 + 1                                                                # 258 chunks: the finishing lanes wrap
    vals = (rng.normal(size=(n, 2)) * 10.0 ** rng.integers(-3, 4, (n, 2))).astype(F)
    mask = rng.random(n) < 0.7
    chunks = gp.chunk_sums(vals, mask)
    assert chunks.shape == (258, 2)
    lane = lambda c: np.where(mask[256 * c:256 * c + 256], vals[256 * c:256 * c + 256, 0], F(0))
    v = lane(3).reshape(4, 64).copy()
    for s in (1, 2, 4, 8, 16, 32):
        v = v + v[:, np.arange(64) ^ s]
    assert chunks[3, 0] == ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]
    assert chunks[257, 0] == (vals[n - 1, 0] if mask[n - 1] else F(0))               # one live lane, 255 times +0.0
    total = gp.finish(chunks)
    lanes = chunks[:256, 0].copy()
    lanes[0] = lanes[0] + chunks[256, 0]
    lanes[1] = lanes[1] + chunks[257, 0]
    assert total[0] == gp.tile_sum(lanes[None, :, None])[0, 0]
    assert abs(float(total[0]) - float(vals[mask, 0].astype(D).sum())) <= 1e-4 * float(np.abs(vals[mask, 0]).astype(D).sum())
    empty = gp.sum_over_gaussians(vals, np.zeros(n, np.int64), np.ones(n, bool), 2)[1]
    assert (empty == 0).all() and not np.signbit(empty).any()                        # a matrix nobody goes through: +0.0


def test_the_vectorised_gather_is_the_loop():
    import gaussians_sh_reference as gs
    rng = np.random.default_rng(1)
    n, E = 300, 900
    count = rng.integers(0, 4, (1, n)).astype(np.int32)
    offsets = (np.cumsum(count.reshape(-1).astype(np.int64)) - count.reshape(-1)).reshape(1, n)
    offsets[0, 5], offsets[0, 6], count[0, 7] = -1, E, 0
    partial = rng.normal(size=(E, gb.SUMS)).astype(F)
    g, ok = gs.gather(partial, count, offsets)
    mine, mine_ok = gp.gather(partial, count[0], offsets[0], [0, 1, 2])
    assert (mine_ok == ok[0]).all() and mine[ok[0]].tobytes() == g[0][ok[0]].tobytes()


# ------------------------------------------------------------------------------------------------ CameraPoses on the host
def _expm(twist):
    """[exp([omega]x) | tau] (4, 4) float64 by the exponential's power series."""
    x, y, z = twist[:3]
    k = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], dtype=D)
    r, term = np.eye(3), np.eye(3)
    for j in range(1, 30):
        term = term @ k / j
        r = r + term
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = r, twist[3:]
    return out


def _table(rng, views, nmat):
    m = rng.normal(size=(views, nmat, 12)).astype(F)
    m[np.abs(m) < 1e-3] = 0.5
    return m


def test_camera_poses_apply_is_the_matrix_exponential_on_the_left():
    from mudg_amd import gaussians
    rng = np.random.default_rng(2)
    poses = gaussians.CameraPoses(4, device="cpu")
    twists = np.array([[0.3, -0.2, 0.5, 0.1, -0.4, 0.2], [1e-3, 2e-3, -1e-3, 0.05, 0.0, -0.02], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                       [3e-6, 0.0, -2e-6, 0.0, 1e-3, 0.0]])
    assert np.linalg.norm(twists[1, :3]) < gaussians.SMALL_ANGLE < np.linalg.norm(twists[0, :3])      # both branches
    with torch.no_grad():
        poses.twist.copy_(torch.tensor(twists, dtype=torch.float32))
    mats = _table(rng, 4, 3)
    out = poses.apply(torch.tensor(mats)).detach().numpy()
    used = poses.twist.detach().numpy().astype(D)
    for v in range(4):
        for o in range(3):
            want = (_expm(used[v]) @ np.concatenate([mats[v, o].astype(D).reshape(3, 4), [[0, 0, 0, 1]]]))[:3].reshape(12)
            assert np.abs(out[v, o] - want).max() <= 4e-7 * max(1.0, np.abs(want).max()), (v, o)
    picked = poses.apply(torch.tensor(mats[[2, 0]]), pick=torch.tensor([2, 0])).detach().numpy()
    assert picked.tobytes() == out[[2, 0]].tobytes()
    w2c = np.stack([np.concatenate([mats[v, 0].astype(D).reshape(3, 4), [[0, 0, 0, 1]]]) for v in range(4)])
    corrected = poses.world_to_camera(w2c)
    assert corrected.dtype == D and np.abs(corrected[:, :3].reshape(4, 12) - out[:, 0]).max() <= 4e-6
    assert np.abs(poses.camera_to_world(np.linalg.inv(w2c)) @ corrected - np.eye(4)).max() <= 1e-9


def test_a_zero_twist_returns_the_matrices_bit_for_bit_and_still_has_a_gradient():
    from mudg_amd import gaussians
    mats = torch.tensor(_table(np.random.default_rng(3), 3, 2))
    poses = gaussians.CameraPoses(3, device="cpu")
    out = poses.apply(mats)
    assert out.detach().numpy().tobytes() == mats.numpy().tobytes()
    weight = torch.tensor(np.random.default_rng(4).normal(size=tuple(mats.shape)).astype(F))
    grad = torch.autograd.grad((out * weight).sum(), poses.twist)[0].numpy().astype(D)
    assert np.isfinite(grad).all()
    m, w = mats.numpy().astype(D).reshape(3, 2, 3, 4), weight.numpy().astype(D).reshape(3, 2, 3, 4)
    for v in range(3):                                                               # d/d tau = the weights' last column; d/d omega = sum m x w
        assert np.allclose(grad[v, 3:], w[v, :, :, 3].sum(0), rtol=1e-5, atol=1e-6)
        torque = sum(np.cross(m[v, o, :, c], w[v, o, :, c]) for o in range(2) for c in range(4))
        assert np.allclose(grad[v, :3], torque, rtol=1e-4, atol=1e-5)


def test_fixed_views_get_the_identity_and_no_gradient():
    from mudg_amd import gaussians
    mats = torch.tensor(_table(np.random.default_rng(5), 3, 2))
    poses = gaussians.CameraPoses(3, fixed=(1,), device="cpu")
    with torch.no_grad():
        poses.twist.fill_(0.01)                                                      # even a fixed row that an optimiser disturbed
    out = poses.apply(mats)
    assert out[1].detach().numpy().tobytes() == mats[1].numpy().tobytes()
    assert out[0].detach().numpy().tobytes() != mats[0].numpy().tobytes()
    grad = torch.autograd.grad(out.square().sum(), poses.twist)[0]
    assert (grad[1] == 0).all() and (grad[0] != 0).any() and (grad[2] != 0).any()
    for bad in (dict(views=0), dict(views=2, fixed=(2,)), dict(views=2, fixed=(-1,))):
        with pytest.raises(gaussians.hip.MudgError, match="CameraPoses"):
            gaussians.CameraPoses(device="cpu", **bad)
    with pytest.raises(gaussians.hip.MudgError, match="views of matrices"):
        poses.apply(mats[:2])


# ------------------------------------------------------------------------------------------------ the float64 registration
def test_the_float64_registration_converges_as_recorded():
    problem = gp.pose_fit_problem()
    losses, final = gp.textbook_pose_fit(problem)
    ratio = losses[-1] / losses[0]
    print(f"float64 pose fit: loss {losses[0]:.6f} -> {losses[-1]:.6f}, ratio {ratio:.4f} (recorded {gp.R64})")
    assert abs(ratio - gp.R64) <= 0.02 * gp.R64                                      # the recorded figure is this code's, to its digits
    _, truth, start, _, _ = problem
    assert gp.pose_error(final[0, 0], truth[0, 0]) == gp.pose_error(start[0, 0], truth[0, 0]) == (0.0, 0.0)
    for v in (1, 2):
        c0, a0 = gp.pose_error(start[v, 0], truth[v, 0])
        c1, a1 = gp.pose_error(final[v, 0], truth[v, 0])
        print(f"view {v}: centre {1e3 * c0:.1f} -> {1e3 * c1:.2f} mm, angle {1e3 * a0:.2f} -> {1e3 * a1:.3f} mrad")
        assert 0.06 < c0 < 0.08 and 0.01 < a0 < 0.013
        assert c1 < c0 / 30 and a1 < a0 / 30                                         # the GPU test asks a tenth: more than 3 x inside


# ------------------------------------------------------------------------------------------------ C-ABI
def test_pose_entry_points_are_declared_bound_and_exported():
    from mudg_amd import build, hip
    header = open(os.path.join(ROOT, "include", "mudg_hip.h")).read()
    for name, nargs in ENTRIES:
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, header, re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == nargs
        assert hasattr(hip.lib(), name)
        for path in hip.LIB_PATHS.values():                                          # operand-type independent: in every build
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert "gaussians_pose.hip" in build.SOURCES


def test_bad_arguments_are_refused_before_any_launch():
    from mudg_amd import hip
    lib = hip.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)                              # never dereferenced: every call below is rejected first

    def refused(fn, good, changes, text=None):
        args = list(good)
        for k, v in changes.items():
            args[k] = v
        assert fn(*args) == -1, (fn.__name__, changes)
        if text:
            assert text in lib.mudg_last_error(), (fn.__name__, changes, lib.mudg_last_error())

    # points cov ids n mats V nmat H W fx fy cx cy znear zfar count offsets partial E stage d_mats stream
    good = [one, one, one, 10, one, 1, 2, 32, 32, 50.0, 50.0, 16.0, 16.0, 0.2, 100.0, one, one, one, 5, one, one, None]
    for k in (0, 1, 4, 15, 16, 17, 19, 20):
        refused(lib.mudg_gauss_pose_bwd, good, {k: None}, b"null")
    refused(lib.mudg_gauss_pose_bwd, good, {0: odd}, b"unaligned")
    refused(lib.mudg_gauss_pose_bwd, good, {16: odd}, b"unaligned")
    refused(lib.mudg_gauss_pose_bwd, good, {2: None}, b"need per-point ids")
    refused(lib.mudg_gauss_pose_bwd, good, {5: 65536}, b"65535")
    for k in (3, 5, 6, 7, 8):
        for v in (0, -1):
            refused(lib.mudg_gauss_pose_bwd, good, {k: v})
    refused(lib.mudg_gauss_pose_bwd, good, {3: 2 ** 31}, b"32-bit index")
    refused(lib.mudg_gauss_pose_bwd, good, {5: 65535, 7: 4096, 8: 4096}, b"2^31")
    for e in (0, -1, 2 ** 31):
        refused(lib.mudg_gauss_pose_bwd, good, {18: e}, b"entries")
    refused(lib.mudg_gauss_pose_bwd, good, {13: 0.0}, b"znear")
    refused(lib.mudg_gauss_pose_bwd, good, {9: float("nan")}, b"intrinsics")

    # points ids n mats V nmat count offsets partial E colour sh degree active stage d_mats_dir stream
    good = [one, one, 10, one, 1, 2, one, one, one, 5, one, one, 2, 2, one, one, None]
    for k in (0, 3, 6, 7, 8, 10, 11, 14, 15):
        refused(lib.mudg_gauss_sh_pose_bwd, good, {k: None}, b"null")
    refused(lib.mudg_gauss_sh_pose_bwd, good, {11: odd}, b"unaligned")
    refused(lib.mudg_gauss_sh_pose_bwd, good, {1: None}, b"need per-point ids")
    refused(lib.mudg_gauss_sh_pose_bwd, good, {4: 65536}, b"65535")
    for degree, active in ((0, 0), (4, 1), (2, 3), (2, -1)):
        refused(lib.mudg_gauss_sh_pose_bwd, good, {12: degree, 13: active}, b"degree")
    for e in (0, -1, 2 ** 31):
        refused(lib.mudg_gauss_sh_pose_bwd, good, {9: e}, b"entries")


def test_the_interface_refuses_what_it_cannot_do():
    from mudg_amd import gaussians, hip, ops
    from virtual_render import virtual_pose_render
    n = 4
    f = lambda *s: torch.zeros(s, dtype=torch.float32)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        ops.gauss_pose_bwd(i32(n, 4), f(n, 6), f(1, 1, 12), (1.0, 1.0, 0.0, 0.0), (16, 16), i32(1, n), torch.zeros((1, n), dtype=torch.int64), f(3, 10))
    with pytest.raises(hip.MudgError, match="on the GPU"):
        ops.gauss_sh_pose_bwd(i32(n, 4), f(1, 1, 12), i32(1, n), torch.zeros((1, n), dtype=torch.int64), f(3, 10), f(n, 3), f(n, 3, 3))
    with pytest.raises(hip.MudgError, match="at most 65535"):
        ops._gauss_pose_buffers("x", n, 65536, 1, "cpu")
    stage, d_mats = ops._gauss_pose_buffers("x", 257, 2, 3, "cpu")
    assert tuple(stage.shape) == (2, 3, 2, 12) and tuple(d_mats.shape) == (2, 3, 12)
    params = inspect.signature(gaussians.fit).parameters
    assert params["poses"].default is None and "No pose gradient" not in gaussians.fit.__doc__
    assert "poses" in virtual_pose_render.fit_cloud_views.__doc__
    assert "none for the matrices" not in gaussians.render_differentiable.__doc__
    assert gaussians.POSE_LEARNING_RATE == gp.POSE_FIT_RATE
