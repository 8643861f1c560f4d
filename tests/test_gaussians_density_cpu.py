"""What density control for the Gaussian fit can show without a GPU: the fp32 statistic of the definition
(tests/gaussians_density_reference.py) against float64 autograd of the projected centres, answers known without arithmetic, the float64
fit with and without density control on a start with a hole, and the C-ABI and generated code of csrc/gaussians_density.hip."""
import os
import re

import numpy as np
import pytest
import torch

import gaussians_bwd_reference as gb
import gaussians_density_reference as gd
import gaussians_reference as gr
from test_gaussians_bwd_cpu import _upstream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
ENTRIES = (("mudg_gauss_density_accumulate", 11), ("mudg_gauss_density_plan", 13), ("mudg_gauss_density_apply", 13))
# The fp32 statistic against float64 autograd on gr.seeded_scene(400, (40, 56), 7) with §24's seeded upstream gradients, zeroed on the
# pixels the textbook's margins exclude: the largest difference relative to the largest norm, measured on the CPU.  The bound is four
# times the measured value, §23's and §24's margin.
MEASURED_GN = 1.52e-6
# The float64 fits of the holed start of gb.fit_problem(): final / initial loss after 200 Adam steps without and with HOLED_CONTROL,
# measured on the CPU.
R_PLAIN64, R_DENSE64 = 0.2069, 0.1299
HOLED_CONTROL = dict(start=20, stop=160, every=20, split_scale=0.2, max_scale=2.0, max_gaussians=400)
HW = (40, 56)


def _control(**kw):
    from mudg_amd import gaussians
    kw = dict(dict(start=0, stop=10, every=1, split_scale=0.2, max_scale=2.0), **kw)
    return gaussians.DensityControl(kw.pop("start"), kw.pop("stop"), kw.pop("every"), **kw)


def toy(n, seed=3, scale=(0.02, 0.6)):
    """n Gaussians with seeded parameters and non-zero moments: params, moments (dicts over gd.PARAMETERS), fp32."""
    rng = np.random.default_rng(seed)
    shapes = {"xyz": (n, 3), "colour": (n, 3), "log_scale": (n, 3), "quat": (n, 4), "opacity_logit": (n,)}
    params = {k: rng.normal(size=s).astype(F) for k, s in shapes.items()}
    params["log_scale"] = np.log(rng.uniform(*scale, (n, 3))).astype(F)
    params["colour"] = rng.uniform(0, 255, (n, 3)).astype(F)
    moments = {k: (rng.normal(size=s).astype(F), rng.uniform(0.1, 1.0, s).astype(F)) for k, s in shapes.items()}
    return params, moments


def _apply(params, moments, action, ids=None, control=None):
    control = control or _control()
    rows = np.array([1, 0, 2, 2], np.int32)[action]
    start = np.cumsum(rows.astype(np.int64)) - rows
    tensors = []
    for k in gd.PARAMETERS:
        tensors += [params[k], *moments[k]]
    outs, ids_out = gd.apply(action, start, int(rows.sum()), np.exp(params["log_scale"]), gd.rotation(params["quat"]), tensors,
                             control.split_offset, control.log_shrink, ids)
    return outs, ids_out, start


# ------------------------------------------------------------------------------------------------ the statistic against float64 autograd
def test_the_fp32_statistic_follows_float64_autograd_of_the_projected_centres():
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene(400, HW, 7)
    _, _, near = gr.textbook_render(xyz, rgb, cov, opacity, mats[0, 0], cam, HW)
    d_rgb, d_depth, d_alpha = _upstream(HW, near)
    out = gb.render_backward(xyz, rgb.astype(F), cov, opacity, None, mats, cam, HW, d_rgb, d_depth, d_alpha)
    grad_sum, seen = gd.accumulate(out["partial"], out["count"], out["offsets"], HW, np.zeros(400, F), np.zeros(400, np.int32))
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=F).astype(D), requires_grad=True)
    (r, d, a), centres = gd.textbook_centres(t64(xyz), t64(rgb), t64(cov), t64(opacity), mats, cam, HW)
    ((r * torch.tensor(d_rgb.astype(D))).sum() + (d * torch.tensor(d_depth.astype(D))).sum() + (a * torch.tensor(d_alpha.astype(D))).sum()).backward()
    want, drawn = gd.centre_gradient_norms(centres, 400, HW)
    assert grad_sum.dtype == F and seen.dtype == np.int32
    assert np.array_equal(seen, drawn[0].astype(np.int32)) and 0 < seen.sum() < 400        # counted where the view draws it, and only once
    err = np.abs(grad_sum.astype(D) - want[0]).max() / want[0].max()
    print(f"{int(seen.sum())} Gaussians counted, largest norm {want[0].max():.4g}, relative difference {err:.3e} (bound {4 * MEASURED_GN:.3e})")
    assert want[0].max() > 0 and err <= 4 * MEASURED_GN
    again, seen2 = gd.accumulate(out["partial"], out["count"], out["offsets"], HW, grad_sum, seen)     # a second backward adds
    assert np.array_equal(again, grad_sum + grad_sum) and np.array_equal(seen2, 2 * seen)


def test_a_spoiled_offset_or_a_dropped_gaussian_counts_nothing():
    partial = np.ones((6, 10), F)
    count = np.array([[2, 0, 3, 1]], np.int32)
    offsets = np.array([[0, 2, 4, -1]], np.int64)                            # Gaussian 2 would read rows 4 .. 6 of six; Gaussian 3 starts before 0
    grad_sum, seen = gd.accumulate(partial, count, offsets, (10, 20), np.zeros(4, F), np.zeros(4, np.int32))
    assert seen.tolist() == [1, 0, 0, 0] and grad_sum[1:].tolist() == [0, 0, 0]
    assert grad_sum[0] == np.sqrt(F(20.0) * F(20.0) + F(10.0) * F(10.0))     # su = sv = 2: (0.5 20 2, 0.5 10 2)


# ------------------------------------------------------------------------------------------------ answers known without arithmetic
def test_a_plan_of_keeps_returns_the_inputs():
    params, moments = toy(7)
    ids = np.arange(7, dtype=np.int32) % 3
    action, rows = gd.plan(np.zeros(7, F), np.ones(7, np.int32), np.full(7, 0.5, F), np.exp(params["log_scale"]), 2e-4, 0.2, 0.005, 2.0)
    assert action.tolist() == [gd.KEEP] * 7 and rows.tolist() == [1] * 7
    outs, ids_out, _ = _apply(params, moments, action, ids)
    for k, name in enumerate(gd.PARAMETERS):
        assert np.array_equal(outs[3 * k], params[name]) and np.array_equal(outs[3 * k + 1], moments[name][0])
        assert np.array_equal(outs[3 * k + 2], moments[name][1])
    assert np.array_equal(ids_out, ids)


def test_a_transparent_gaussian_disappears_and_its_neighbours_move_up_by_one():
    params, moments = toy(6)
    opacity = np.full(6, 0.5, F)
    opacity[2] = 0.004
    action, rows = gd.plan(np.zeros(6, F), np.ones(6, np.int32), opacity, np.exp(params["log_scale"]), 2e-4, 0.2, 0.005, 2.0)
    assert action.tolist() == [0, 0, gd.PRUNE, 0, 0, 0] and rows.tolist() == [1, 1, 0, 1, 1, 1]
    outs, _, start = _apply(params, moments, action)
    assert start.tolist() == [0, 1, 2, 2, 3, 4]
    rest = [0, 1, 3, 4, 5]
    for k, name in enumerate(gd.PARAMETERS):
        assert len(outs[3 * k]) == 5 and np.array_equal(outs[3 * k], params[name][rest]) and np.array_equal(outs[3 * k + 1], moments[name][0][rest])
    huge = np.exp(params["log_scale"])
    huge[4, 1] = 2.5                                                         # larger than max_scale: pruned whatever its opacity
    nan = np.full(6, 0.5, F)
    nan[0] = np.nan
    assert gd.plan(np.zeros(6, F), np.ones(6, np.int32), nan, huge, 2e-4, 0.2, 0.005, 2.0)[0].tolist() == [1, 0, 0, 0, 1, 0]


def test_a_clone_keeps_its_moments_and_its_copy_starts_at_zero():
    params, moments = toy(3, scale=(0.02, 0.15))                             # every scale below split_scale
    grad_sum, seen = np.array([0.0, 3e-4 * 4, 0.0], F), np.array([4, 4, 4], np.int32)
    action, rows = gd.plan(grad_sum, seen, np.full(3, 0.5, F), np.exp(params["log_scale"]), 2e-4, 0.2, 0.005, 2.0)
    assert action.tolist() == [0, gd.CLONE, 0] and rows.tolist() == [1, 2, 1]
    outs, _, _ = _apply(params, moments, action)
    for k, name in enumerate(gd.PARAMETERS):
        assert np.array_equal(outs[3 * k], params[name][[0, 1, 1, 2]])
        for j in (0, 1):
            got = outs[3 * k + 1 + j]
            assert np.array_equal(got[[0, 1, 3]], moments[name][j][[0, 1, 2]]) and not got[2].any() and got[1].all()


def test_a_split_is_symmetric_along_the_longest_axis_and_keeps_the_variance_along_it():
    params, moments = toy(2, seed=9)
    params["log_scale"][1] = np.log(np.array([0.1, 0.5, 0.5], F))            # two largest scales: the first of them, axis 1
    params["xyz"][1] = [0.3, -0.4, 0.7]
    control = _control()
    action = np.array([gd.KEEP, gd.SPLIT], np.int32)
    assert gd.plan(np.array([0, 1.0], F), np.array([1, 2], np.int32), np.full(2, 0.5, F), np.exp(params["log_scale"]), 2e-4, 0.2, 0.005,
                   2.0)[0].tolist() == action.tolist()
    outs, _, _ = _apply(params, moments, action, control=control)
    xyz, log_scale = outs[0], outs[6]
    axis = gd.rotation(params["quat"])[1].reshape(3, 3)[:, 1].astype(D)
    up, down = xyz[1].astype(D) - params["xyz"][1], xyz[2].astype(D) - params["xyz"][1]
    # x + t and x - t are each rounded once at |x| < 1: half an ulp of 1, 6e-8, against an offset of 0.39
    assert np.abs(up + down).max() <= 2 * 6e-8 and np.abs(np.cross(up, axis)).max() <= 4 * 6e-8
    assert np.array_equal(log_scale[1], log_scale[2]) and np.array_equal(log_scale[1], params["log_scale"][1] - F(control.log_shrink))
    for k in (1, 2, 4, 5, 7, 8, 10, 11, 13, 14):
        assert not outs[k][1:].any() and np.array_equal(outs[k][0], (moments[gd.PARAMETERS[k // 3]][(k % 3) - 1])[0])
    for k in (3, 9, 12):                                                     # colour, quaternion and opacity logit are copied
        assert np.array_equal(outs[k][1], outs[k][2]) and np.array_equal(outs[k][1], params[gd.PARAMETERS[k // 3]][1])
    # two children of equal weight: variance along the axis = the children's own + the squared offset of their centres.  The rounded
    # steps: log_shrink (6e-8 of 0.47), two subtractions and the offsets above (3e-7 of d^2): 1e-6 relative is above their sum
    child = np.exp(log_scale[1].astype(D))[1] ** 2
    offset = (0.5 * np.dot(up - down, axis)) ** 2
    parent = float(np.exp(params["log_scale"][1].astype(D))[1]) ** 2
    print(f"variance along the split axis: parent {parent:.9f}, children {child + offset:.9f}")
    assert abs(child + offset - parent) <= 1e-6 * parent
    assert abs(control.split_offset ** 2 + 1 / control.split_shrink ** 2 - 1) < 1e-12 and control.split_shrink == 1.6


def test_a_gaussian_never_seen_is_never_grown_and_growing_can_be_forbidden():
    scale = np.full((4, 3), 0.1, F)
    scale[3] = 0.5
    grad_sum, seen = np.array([9.0, 9.0, 1e-5, 9.0], F), np.array([0, 1, 1, 2], np.int32)
    args = (grad_sum, seen, np.full(4, 0.5, F), scale, 2e-4, 0.2, 0.005, 2.0)
    assert gd.plan(*args)[0].tolist() == [gd.KEEP, gd.CLONE, gd.KEEP, gd.SPLIT]
    assert gd.plan(*args, grow=False)[0].tolist() == [gd.KEEP] * 4
    args[0][0] = np.nan                                                      # 0 / 0 views is never evaluated into a decision, a NaN sum is
    assert gd.plan(*args)[0].tolist() == [gd.PRUNE, gd.CLONE, gd.KEEP, gd.SPLIT]


def test_max_gaussians_falls_back_to_pruning_only_and_an_empty_result_is_refused():
    params, moments = toy(5, scale=(0.02, 0.15))
    params["opacity_logit"][:] = 0.0
    params["opacity_logit"][4] = -9.0                                        # sigmoid(-9) < 0.005
    grad_sum, seen = np.full(5, 1.0, F), np.ones(5, np.int32)
    p, m, _, counts = gd.densify(params, moments, None, grad_sum, seen, _control(max_gaussians=8))
    assert counts == dict(before=5, after=8, kept=0, pruned=1, cloned=4, split=0, grew=True) and len(p["xyz"]) == 8
    p, m, _, counts = gd.densify(params, moments, None, grad_sum, seen, _control(max_gaussians=7))
    assert counts == dict(before=5, after=4, kept=4, pruned=1, cloned=0, split=0, grew=False)
    assert np.array_equal(p["xyz"], params["xyz"][:4]) and np.array_equal(m["quat"][1], moments["quat"][1][:4])
    params["opacity_logit"][:] = -9.0
    with pytest.raises(ValueError, match="pruned"):
        gd.densify(params, moments, None, grad_sum, seen, _control())


def test_the_control_states_its_schedule_and_refuses_nonsense():
    from mudg_amd import gaussians, hip
    c = gaussians.DensityControl(20, 160, 20, split_scale=0.2, max_scale=2.0, reset_every=50)
    assert (c.grad_threshold, c.min_opacity, c.reset_opacity, c.split_shrink, c.max_gaussians) == (2e-4, 0.005, 0.01, 1.6, None)
    assert [i for i in range(200) if c.densifies_after(i)] == [39, 59, 79, 99, 119, 139, 159]
    assert [i for i in range(200) if c.resets_after(i)] == [49, 99, 149] and not c.gathers(19) and c.gathers(20) and not c.gathers(160)
    assert c.history == [] and abs(c.reset_logit - np.log(0.01 / 0.99)) < 1e-12 and c.log_shrink == float(F(np.log(1.6)))
    empty = gaussians.DensityControl(5, 5, 1, split_scale=0.2, max_scale=2.0)
    assert not any(empty.gathers(i) or empty.densifies_after(i) for i in range(20))
    with pytest.raises(TypeError):
        gaussians.DensityControl(0, 10, 1)                                   # split_scale and max_scale have no default
    for bad in (dict(every=0), dict(split_scale=float("nan")), dict(reset_opacity=1.0), dict(split_shrink=1.0), dict(max_gaussians=0), dict(start=-1)):
        with pytest.raises(hip.MudgError, match="DensityControl"):
            _control(**bad)


# ------------------------------------------------------------------------------------------------ the fit in float64, with a hole
def test_the_float64_fit_of_a_holed_start_gains_from_density_control():
    from mudg_amd import gaussians
    start, views, cam, targets = gb.fit_problem()
    holed, keep = gd.holed_start(start, views, cam, HW)
    assert 0.2 * len(keep) <= (~keep).sum() <= 0.5 * len(keep)
    rates, betas, eps = gaussians.LEARNING_RATES, gaussians.ADAM_BETAS, gaussians.ADAM_EPS
    plain = gb.textbook_fit(holed, views, cam, targets, HW, rates, 200, betas, eps)
    kw = dict(HOLED_CONTROL)
    control = gaussians.DensityControl(kw.pop("start"), kw.pop("stop"), kw.pop("every"), **kw)
    dense, history = gd.textbook_fit_density(holed, views, cam, targets, HW, rates, 200, betas, eps, control)
    r_plain, r_dense = plain[-1] / plain[0], dense[-1] / dense[0]
    print(f"float64, {int(keep.sum())} of {len(keep)} Gaussians at the start: plain {plain[0]:.5f} -> {plain[-1]:.5f}, r_plain64 = {r_plain:.5f} "
          f"(recorded {R_PLAIN64}); with density control {dense[0]:.5f} -> {dense[-1]:.5f}, r_dense64 = {r_dense:.5f} (recorded {R_DENSE64})")
    for h in history:
        print(h)
    assert dense[0] == pytest.approx(plain[0], rel=1e-12) and len(history) == 7
    assert history[-1]["after"] > int(keep.sum()) and history[-1]["after"] <= HOLED_CONTROL["max_gaussians"]
    assert r_dense <= 0.8 * r_plain                                          # the problem is one where the reference alone shows the gain
    assert R_PLAIN64 / 1.5 <= r_plain <= 1.5 * R_PLAIN64 and R_DENSE64 / 1.5 <= r_dense <= 1.5 * R_DENSE64    # the recorded values are of this run's size


# ------------------------------------------------------------------------------------------------ the Python surface off the GPU
def test_tensors_off_the_gpu_are_refused():
    from mudg_amd import gaussians, hip, ops
    n = 3
    f = lambda *s: torch.zeros(s)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    i64 = lambda *s: torch.zeros(s, dtype=torch.int64)
    tensors = [f(n, 3)] * 9 + [f(n, 4)] * 3 + [f(n)] * 3
    for call in (lambda: ops.gauss_density_accumulate(f(2, 10), i32(1, n), i64(1, n), (16, 16), f(n), i32(n)),
                 lambda: ops.gauss_density_plan(f(n), i32(n), f(n), f(n, 3), grad_threshold=2e-4, split_scale=0.2, min_opacity=0.005, max_scale=2.0),
                 lambda: ops.gauss_density_apply(i32(n), i64(n), n, f(n, 3), f(n, 9), tensors, split_offset=0.78, log_shrink=0.47),
                 lambda: gaussians.DensityStats(n, "cpu")):
        with pytest.raises(hip.MudgError, match="on the GPU"):
            call()
    assert ops.GAUSS_PARAMETER_WIDTHS == (3, 3, 3, 4, 1) and gaussians.PARAMETERS == gd.PARAMETERS
    assert (ops.GAUSS_KEEP, ops.GAUSS_PRUNE, ops.GAUSS_CLONE, ops.GAUSS_SPLIT) == (gd.KEEP, gd.PRUNE, gd.CLONE, gd.SPLIT)


def test_the_rotation_helper_is_the_one_the_covariance_uses():
    from mudg_amd import gaussians
    rng = np.random.default_rng(4)
    q, s = torch.tensor(rng.normal(size=(20, 4)).astype(F)), torch.tensor(rng.uniform(0.1, 1.0, (20, 3)).astype(F))
    rot = gaussians.rotation_from_quaternions(q)
    m = rot * s[:, None, :]
    full = m @ m.transpose(1, 2)
    want = torch.stack([full[:, 0, 0], full[:, 0, 1], full[:, 0, 2], full[:, 1, 1], full[:, 1, 2], full[:, 2, 2]], dim=1)
    assert torch.equal(gaussians.covariance_from_scales_rotations(s, q), want)
    assert np.abs(rot.reshape(20, 9).numpy() - gd.rotation(q.numpy().astype(D))).max() <= 1e-6


def test_the_product_does_not_import_the_cpu_definition():
    for d in ("mudg_amd", "lvdm", "utils", "virtual_render", "main", "tools"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith(".py"):
                    assert "gaussians_density_reference" not in open(os.path.join(base, f)).read(), f


# ------------------------------------------------------------------------------------------------ C-ABI and generated code
def test_density_entry_points_are_declared_bound_and_exported():
    import ctypes
    from mudg_amd import build, hip
    header = open(os.path.join(ROOT, "include", "mudg_hip.h")).read()
    for name, nargs in ENTRIES:
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, header, re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == nargs
        assert hasattr(hip.lib(), name)
        for path in hip.LIB_PATHS.values():                                          # operand-type independent: in every build
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert "gaussians_density.hip" in build.SOURCES


def test_bad_arguments_are_refused_before_any_launch():
    import ctypes
    from mudg_amd import hip
    lib = hip.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)                              # never dereferenced: every call below is rejected first
    nan = float("nan")

    def refused(fn, good, changes, text=None):
        args = list(good)
        for k, v in changes.items():
            args[k] = v
        assert fn(*args) == -1, (fn.__name__, changes)
        if text:
            assert text in lib.mudg_last_error(), (fn.__name__, changes, lib.mudg_last_error())

    # partial count offsets n V H W E grad_sum seen stream
    good = [one, one, one, 10, 1, 32, 32, 5, one, one, None]
    for k in (0, 1, 2, 8, 9):
        refused(lib.mudg_gauss_density_accumulate, good, {k: None}, b"null")
    refused(lib.mudg_gauss_density_accumulate, good, {2: odd}, b"unaligned")
    for k in (3, 4, 5, 6):
        for v in (0, -1):
            refused(lib.mudg_gauss_density_accumulate, good, {k: v})
    refused(lib.mudg_gauss_density_accumulate, good, {3: 2 ** 31}, b"32-bit index")
    refused(lib.mudg_gauss_density_accumulate, good, {4: 2 ** 20, 5: 1024, 6: 1024}, b"2^31")
    for e in (0, -1, 2 ** 31, 2 ** 40):
        refused(lib.mudg_gauss_density_accumulate, good, {7: e}, b"entries")

    # grad_sum seen opacity scale n grad_threshold split_scale min_opacity max_scale grow action rows stream
    good = [one, one, one, one, 10, 2e-4, 0.2, 0.005, 2.0, 1, one, one, None]
    for k in (0, 1, 2, 3, 10, 11):
        refused(lib.mudg_gauss_density_plan, good, {k: None}, b"null")
    for v in (0, -1, 2 ** 31, 2 ** 40):
        refused(lib.mudg_gauss_density_plan, good, {4: v}, b"Gaussians")
    for k in (5, 6, 7, 8):
        refused(lib.mudg_gauss_density_plan, good, {k: nan}, b"are numbers")

    # action start n n_out scale rot split_offset log_shrink src dst ids ids_out stream
    table = ctypes.c_void_p * 15
    src, dst = table(*[16] * 15), table(*[16] * 15)
    good = [one, one, 10, 12, one, one, 0.78, 0.47, src, dst, one, one, None]
    for k in (0, 1, 4, 5, 8, 9):
        refused(lib.mudg_gauss_density_apply, good, {k: None}, b"null")
    for k in (0, 7, 14):
        for side in (8, 9):
            holed = table(*[16] * 15)
            holed[k] = None
            refused(lib.mudg_gauss_density_apply, good, {side: holed}, b"null")
    refused(lib.mudg_gauss_density_apply, good, {10: None}, b"ids")                   # ids without ids_out, and the other way round
    refused(lib.mudg_gauss_density_apply, good, {11: None}, b"ids")
    refused(lib.mudg_gauss_density_apply, good, {1: odd}, b"unaligned")
    for v in (0, -1, 2 ** 31, 2 ** 40):
        refused(lib.mudg_gauss_density_apply, good, {2: v}, b"Gaussians")
        refused(lib.mudg_gauss_density_apply, good, {3: v}, b"rows out")
    for k in (6, 7):
        refused(lib.mudg_gauss_density_apply, good, {k: nan}, b"are numbers")


def test_density_kernels_use_no_scratch_no_atomics_and_no_lds(tmp_path):
    """Facts about the generated gfx950 code as DESIGN.md §25 records them: no scratch, no spill and no LDS in any of the three kernels, no
    atomic, no flat access, no transcendental."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "gaussians_density.s"
    done = subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S", "-Rpass-analysis=kernel-resource-usage",
                           os.path.join(ROOT, "mudg_amd", "csrc", "gaussians_density.hip"), "-o", str(out)], check=True, capture_output=True,
                          timeout=600, text=True)
    remarks = done.stderr
    assert len(re.findall(r"ScratchSize \[bytes/lane\]: 0\b", remarks)) == 3 and len(re.findall(r"VGPRs Spill: 0\b", remarks)) == 3, remarks
    assert len(re.findall(r"SGPRs Spill: 0\b", remarks)) == 3 and len(re.findall(r"LDS Size \[bytes/block\]: 0\b", remarks)) == 3, remarks
    s = out.read_text()
    md = s[s.index("amdhsa.kernels"):]
    seen = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", md, re.S):
        kind = re.search(r"gauss_density_(accumulate|plan|apply)_kernel", m.group(2))
        assert kind, m.group(2)
        seen[kind.group(1)] = int(m.group(4))
        print(f"{m.group(2)}: {m.group(1)} bytes of LDS, {m.group(4)} VGPRs")
        assert int(m.group(1)) == 0 and int(m.group(3)) == 0 and int(m.group(5)) == 0, m.groups()
    assert set(seen) == {"accumulate", "plan", "apply"}, seen
    assert max(seen.values()) <= 128                                                  # four waves a SIMD at the least
    for name in sorted(set(re.findall(r"^(_Z\S*gauss_density_\w+_kernel\S*):", s, re.M))):
        body = s[s.index(name + ":"):]
        lines = [l.strip() for l in body[:body.index(".end_amdhsa_kernel")].splitlines()]
        assert not any(l.startswith(("scratch_", "flat_", "global_atomic", "buffer_atomic", "ds_")) for l in lines), name
        assert not any(l.startswith(("v_exp_f32", "v_log_f32", "v_sin_f32", "v_cos_f32")) for l in lines), name
