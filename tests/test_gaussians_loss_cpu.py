"""What the image loss of the Gaussian fit can show without a GPU: the fp32 rule of tests/gaussians_loss_reference.py against
float64 autograd of the textbook, answers known without arithmetic, the structure of the window, the float64 fit with the SSIM term, and
the C-ABI and generated code of csrc/gaussians_loss.hip."""
import os
import re

import numpy as np
import pytest
import torch

import gaussians_bwd_reference as gb
import gaussians_loss_reference as gl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
ENTRIES = (("mudg_gauss_loss", 10), ("mudg_gauss_loss_finish", 8), ("mudg_gauss_loss_bwd", 15))
LDS_BYTES = {"gauss_loss_kernel": 13792, "gauss_loss_finish_kernel": 128, "gauss_loss_bwd_kernel": 13104}
# The fp32 rule against float64 autograd on gl.seeded_images(3, (40, 56)) with depth_weight 0.1, over ssim_weight 0, 0.2 and 1: per group
# the largest difference relative to the float64 group's largest magnitude, measured on the CPU.  The bound is four times
# the measured value, §23's and §24's margin for accumulation order.
MEASURED = dict(loss=7.70e-8, l1=6.78e-9, ssim=6.37e-9, depth=2.14e-8, d_rgb=4.09e-7, d_depth=2.46e-8)
# The float64 fit of gb.fit_problem() with the textbook loss at ssim_weight 0.2: final / initial loss after 200 Adam steps, measured on the
# CPU (0.14224 -> 0.00075).
R64S = 0.00525
HW = (40, 56)


def _t64(a, grad=False):
    return torch.tensor(np.asarray(a, F).astype(D), requires_grad=grad)


# ------------------------------------------------------------------------------------------------ the rule against float64 autograd
def test_the_fp32_rule_follows_float64_autograd_of_the_textbook():
    x, y, d, dt = gl.seeded_images(3, HW)
    assert x.min() < -0.4 and x.max() > 1.4 and 0.25 < (dt == 0).mean() < 0.42 and not (x == y).any()
    worst = dict.fromkeys(MEASURED, 0.0)
    for lam in (0.0, 0.2, 1.0):
        out = gl.loss_and_gradients(x, y, d, dt, ssim_weight=lam, depth_weight=0.1)
        tx, td = _t64(x, True), _t64(d, True)
        loss, (l1, s, depth) = gl.textbook(tx, _t64(y), td, _t64(dt), ssim_weight=lam, depth_weight=0.1)
        loss.backward()
        totals = out["totals"]
        groups = dict(loss=(totals[0], loss.item()), l1=(totals[1], l1.item()), ssim=(totals[2], s.item()), depth=(totals[3], depth.item()),
                      d_rgb=(out["d_rgb"], tx.grad.numpy()), d_depth=(out["d_depth"], td.grad.numpy()))
        for k, (got, want) in groups.items():
            assert np.asarray(got).dtype == F
            err = float(np.abs(np.asarray(got, D) - want).max() / np.abs(want).max())      # no pixel is excluded
            worst[k] = max(worst[k], err)
            print(f"ssim_weight {lam}: {k} differs by {err:.3e} of the largest magnitude {np.abs(want).max():.4g} (bound {4 * MEASURED[k]:.3e})")
            assert err <= 4 * MEASURED[k], (lam, k, err)
        assert int(totals[5:6].view(np.int32)[0]) == int((dt > 0).sum()) and totals[4] == F((dt > 0).sum())
    print("measured:", {k: f"{v:.3e}" for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------ answers known without arithmetic
def test_equal_images_have_ssim_one_in_every_pixel_and_no_l1_gradient():
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.5, 1.5, (2, 3, 17, 33)).astype(F)
    maps, partial, S, (num, den) = gl.forward(x, x.copy())
    assert np.array_equal(num.view(np.int32), den.view(np.int32))           # the same bits above and below the line
    assert np.array_equal(S, np.ones_like(S))
    for lam in (0.0, 0.2, 1.0):
        totals = gl.finish(partial, (17, 33), lam, 0.0)
        assert totals[1] == 0 and totals[2] == 1 and totals[0] == 0          # sum S == N: the mean is 1 exactly, and the loss is 0
    assert float(partial[..., 1].astype(D).sum()) == 2 * 3 * 17 * 33 and not partial[..., 0].any()
    totals = gl.finish(partial, (17, 33), 0.0, 0.0)
    d_rgb, _ = gl.backward(x, x.copy(), maps, totals, 2.5, 0.0, 0.0)
    assert not d_rgb.any()                                                   # ssim_weight 0 leaves the L1 part alone: sgn(0) = 0


def test_depth_targets_that_are_all_zero_count_nothing():
    x, y, d, dt = gl.seeded_images(2, (17, 33))
    out = gl.loss_and_gradients(x, y, d, np.zeros_like(dt), ssim_weight=0.2, depth_weight=0.5, up=2.5)
    plain = gl.loss_and_gradients(x, y, ssim_weight=0.2, up=2.5)
    totals = out["totals"]
    assert int(totals[5:6].view(np.int32)[0]) == 0 and totals[4] == 1 and totals[3] == 0
    assert totals[0] == plain["totals"][0] and not out["d_depth"].any() and out["d_depth"].shape == d.shape
    assert np.array_equal(out["d_rgb"], plain["d_rgb"]) and plain["d_depth"] is None


def test_without_the_ssim_term_the_gradient_is_the_sign_over_n():
    x, y, _, _ = gl.seeded_images(2, (17, 33))
    N = 2 * 3 * 17 * 33
    for up in (1.0, 2.5):
        out = gl.loss_and_gradients(x, y, ssim_weight=0.0, up=up)
        want = F(up) * ((F(1.0) / F(N)) * np.sign(x - y).astype(F))           # up (fl(1 / N) sgn): the association of §26
        assert np.array_equal(out["d_rgb"], want) and out["d_rgb"].dtype == F
    assert out["totals"][0] == out["totals"][1]                             # (1 l1 + 0 (1 - s)) + 0 0


def test_a_one_pixel_image_has_one_tap():
    x, y = np.full((1, 3, 1, 1), 0.75, F), np.full((1, 3, 1, 1), 0.25, F)
    w = F(17434.0 / 65536.0)
    assert gl.WINDOW[5] == w and np.array_equal(gl.convolve(x), (w * (w * x)).astype(F))
    a, m, b, n, c = w * (w * x), w * (w * y), w * (w * (x * x)), w * (w * (y * y)), w * (w * (x * y))
    S = ((F(2) * (a * m) + gl.C1) * (F(2) * (c - a * m) + gl.C2)) / (((a * a + m * m) + gl.C1) * (((b - a * a) + (n - m * m)) + gl.C2))
    _, partial, got, _ = gl.forward(x, y)
    assert np.array_equal(got, S) and partial.shape == (1, 3, 1, 4) and np.array_equal(partial[..., 1], S.reshape(1, 3, 1))
    assert np.array_equal(partial[..., 0], np.full((1, 3, 1), 0.5, F))


# ------------------------------------------------------------------------------------------------ structure
def test_the_window_is_the_projects_ssim_window_and_sums_to_one():
    from mudg_amd import ops
    assert tuple(ops.SSIM_WINDOW) == gl.TAPS_INT and sum(ops.SSIM_WINDOW) == 65536
    assert gl.WINDOW.dtype == F and np.array_equal(gl.WINDOW.astype(D) * 65536.0, np.array(ops.SSIM_WINDOW, D))      # every tap exact
    total = F(0.0)
    for w in gl.WINDOW:
        total = total + w
    assert total == F(1.0) and float(gl.WINDOW.astype(D).sum()) == 1.0
    assert gl.C1 == F(0.01 ** 2) and gl.C2 == F(0.03 ** 2)                  # §15's 6.5025 and 58.5225 over 255^2


def test_the_zero_padded_window_is_its_own_adjoint():
    rng = np.random.default_rng(2)
    u, v = rng.normal(size=(1, 3, 13, 9)), rng.normal(size=(1, 3, 13, 9))
    w = torch.tensor(np.array(gl.TAPS_INT, D) / 65536.0)
    conv = lambda t: torch.nn.functional.conv2d(torch.tensor(t), torch.outer(w, w)[None, None].repeat(3, 1, 1, 1), padding=5, groups=3)
    lhs, rhs = float((conv(u) * torch.tensor(v)).sum()), float((torch.tensor(u) * conv(v)).sum())
    assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), 1.0)
    # and the fp32 passes are that convolution: exact taps, so float64 differs by the rounding of 22 additions only
    got = gl.convolve(u.astype(F))
    assert np.abs(got.astype(D) - conv(u.astype(F).astype(D)).numpy()).max() <= 22 * 6e-8 * np.abs(u).max()


def test_one_pixels_ssim_has_a_gradient_on_an_eleven_by_eleven_footprint_in_four_tiles():
    x, y, maps, impulse = gl.impulse_case()
    assert (33, 33) == x.shape[2:] and np.count_nonzero(impulse) == 3
    totals = gl.finish(gl.forward(x, y)[1], (33, 33), 1.0, 0.0)
    got, _ = gl.backward(x, y, impulse, totals, 1.0, 1.0, 0.0)
    hit = np.argwhere(got[0, 1] != 0)
    assert len(hit) == 121 and hit.min(axis=0).tolist() == [10, 10] and hit.max(axis=0).tolist() == [20, 20]
    assert {(int(j) // 16, int(i) // 16) for j, i in hit} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert not got[0, 0].any() and not got[0, 2].any()
    # float64 autograd of that pixel's S alone, times -1 / N
    tx = _t64(x, True)
    gl.textbook_ssim_map(tx, _t64(y))[0, 1, 15, 15].backward()
    want = -tx.grad.numpy() / x.size
    assert np.abs(got.astype(D) - want).max() <= 4 * MEASURED["d_rgb"] * np.abs(want).max()
    # and a moved pixel moves S only inside that footprint
    moved = x.copy()
    moved[0, 1, 15, 15] += F(0.25)
    changed = np.argwhere(gl.forward(moved, y)[2] != gl.forward(x, y)[2])
    assert len(changed) > 60 and (changed[:, :2] == [0, 1]).all() and changed[:, 2:].min() >= 10 and changed[:, 2:].max() <= 20


# ------------------------------------------------------------------------------------------------ the fit in float64
def test_the_float64_fit_with_the_ssim_term_lowers_the_loss():
    from mudg_amd import gaussians
    start, views, cam, targets = gb.fit_problem()
    losses = gl.textbook_fit(start, views, cam, targets, HW, gaussians.LEARNING_RATES, 200, gaussians.ADAM_BETAS, gaussians.ADAM_EPS, 0.2)
    ratio = losses[-1] / losses[0]
    print(f"float64 fit at ssim_weight 0.2: loss {losses[0]:.5f} -> {losses[-1]:.5f}, ratio r64s = {ratio:.5f} (recorded {R64S})")
    assert ratio < 0.5
    assert ratio <= 1.5 * R64S                                               # the recorded r64s is of this run's size


# ------------------------------------------------------------------------------------------------ the Python surface off the GPU
def test_tensors_off_the_gpu_are_refused():
    from mudg_amd import gaussians, hip, ops
    x, d = torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8)
    for call in (lambda: ops.gauss_loss(x, x), lambda: ops.gauss_loss_finish(torch.zeros(1, 3, 1, 4), (8, 8), ssim_weight=0.2),
                 lambda: ops.gauss_loss_bwd(x, x, torch.zeros(1, 3, 3, 8, 8), torch.zeros(8), torch.ones(1), ssim_weight=0.2),
                 lambda: gaussians.image_loss(x, x), lambda: gaussians.image_loss(x, x, d, d, depth_weight=0.1),
                 lambda: gaussians.image_loss.terms(x, x)):
        with pytest.raises(hip.MudgError, match="on the GPU"):
            call()
    assert (ops.GAUSS_LOSS_COLS, ops.GAUSS_LOSS_TOTALS) == (4, 8)


def test_the_product_does_not_import_the_cpu_definition():
    for d in ("mudg_amd", "lvdm", "utils", "virtual_render", "main", "tools"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith(".py"):
                    assert "gaussians_loss_reference" not in open(os.path.join(base, f)).read(), f


def test_fit_takes_an_ssim_weight_and_its_docstring_no_longer_lists_the_term_as_missing():
    import inspect
    from mudg_amd import gaussians
    from virtual_render import virtual_pose_render as vpr
    sig = inspect.signature(gaussians.fit)
    assert sig.parameters["ssim_weight"].default == 0.0 and sig.parameters["ssim_weight"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "SSIM term" not in gaussians.fit.__doc__ and "ssim_weight" in gaussians.fit.__doc__ and "ssim_weight" in vpr.fit_cloud_views.__doc__
    assert inspect.signature(gaussians.image_loss).parameters["ssim_weight"].default == 0.2 and callable(gaussians.image_loss.terms)


# ------------------------------------------------------------------------------------------------ C-ABI and generated code
def test_loss_entry_points_are_declared_bound_and_exported():
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
    assert "gaussians_loss.hip" in build.SOURCES


def test_bad_arguments_are_refused_before_any_launch():
    from mudg_amd import hip
    import ctypes
    lib = hip.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(18)                              # never dereferenced: every call below is rejected first
    nan, inf = float("nan"), float("inf")

    def refused(fn, good, changes, text=None):
        args = list(good)
        for k, v in changes.items():
            args[k] = v
        assert fn(*args) == -1, (fn.__name__, changes)
        if text:
            assert text in lib.mudg_last_error(), (fn.__name__, changes, lib.mudg_last_error())

    def images(fn, good, at):
        """V, H, W at argument `at`: not positive, V NT >= 2^31, more workgroups than a grid."""
        for k in range(3):
            for v in (0, -1):
                refused(fn, good, {at + k: v})
        refused(fn, good, {at: 2 ** 19, at + 1: 1024, at + 2: 1024}, b"2^31")        # 2^19 views of 2^12 tiles
        refused(fn, good, {at: 2 ** 18, at + 1: 1024, at + 2: 1024}, b"grid")        # V NT = 2^30 < 2^31, three channels of it are not

    # rgb targets depth depth_targets V H W maps partial stream
    good = [one, one, one, one, 2, 40, 56, one, one, None]
    for k in (0, 1, 7, 8):
        refused(lib.mudg_gauss_loss, good, {k: None}, b"null")
        refused(lib.mudg_gauss_loss, good, {k: odd}, b"unaligned")
    for k in (2, 3):
        refused(lib.mudg_gauss_loss, good, {k: None}, b"together")
        refused(lib.mudg_gauss_loss, good, {k: odd}, b"unaligned")
    images(lib.mudg_gauss_loss, good, 4)

    # partial V H W ssim_weight depth_weight totals stream
    good = [one, 2, 40, 56, 0.2, 0.1, one, None]
    for k in (0, 6):
        refused(lib.mudg_gauss_loss_finish, good, {k: None}, b"null")
        refused(lib.mudg_gauss_loss_finish, good, {k: odd}, b"unaligned")
    images(lib.mudg_gauss_loss_finish, good, 1)
    for v in (-0.01, 1.01, nan, inf):
        refused(lib.mudg_gauss_loss_finish, good, {4: v}, b"SSIM weight")
    for v in (-0.5, nan, inf):
        refused(lib.mudg_gauss_loss_finish, good, {5: v}, b"depth weight")

    # rgb targets maps depth depth_targets totals upstream V H W ssim_weight depth_weight d_rgb d_depth stream
    good = [one, one, one, one, one, one, one, 2, 40, 56, 0.2, 0.1, one, one, None]
    for k in (0, 1, 2, 5, 6, 12):
        refused(lib.mudg_gauss_loss_bwd, good, {k: None}, b"null")
    for k in (0, 1, 2, 3, 4, 5, 6, 12, 13):
        refused(lib.mudg_gauss_loss_bwd, good, {k: odd}, b"unaligned")
    for k in (3, 4):
        refused(lib.mudg_gauss_loss_bwd, good, {k: None}, b"together")
    refused(lib.mudg_gauss_loss_bwd, good, {3: None, 4: None}, b"d_depth without depth")
    images(lib.mudg_gauss_loss_bwd, good, 7)
    for v in (-0.01, 1.01, nan, inf):
        refused(lib.mudg_gauss_loss_bwd, good, {10: v}, b"SSIM weight")
    for v in (-0.5, nan, inf):
        refused(lib.mudg_gauss_loss_bwd, good, {11: v}, b"depth weight")


def test_loss_kernels_use_no_scratch_and_the_lds_the_design_states(tmp_path):
    """The compiler's resource-usage remarks for the three gfx950 kernels as DESIGN.md §26 records them: no scratch, no spill, the LDS of
    the aprons and the pass buffers, at most 64 VGPRs (eight waves a SIMD)."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    done = subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S", "-Rpass-analysis=kernel-resource-usage",
                           os.path.join(ROOT, "mudg_amd", "csrc", "gaussians_loss.hip"), "-o", str(tmp_path / "gaussians_loss.s")], check=True,
                          capture_output=True, timeout=600, text=True)
    remarks = done.stderr
    blocks = re.split(r"remark: Function Name: ", remarks)[1:]
    seen = {}
    for block in blocks:
        name = re.search(r"gauss_loss(?:_finish|_bwd)?_kernel", block.split()[0])
        assert name, block
        field = lambda label: int(re.search(re.escape(label) + r": (\d+)", block).group(1))
        seen[name.group(0)] = field("LDS Size [bytes/block]")
        print(f"{name.group(0)}: {field('VGPRs')} VGPRs, {field('TotalSGPRs')} SGPRs, {field('LDS Size [bytes/block]')} bytes of LDS, "
              f"{field('Occupancy [waves/SIMD]')} waves a SIMD")
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0, block
        assert field("VGPRs") <= 64 and field("Occupancy [waves/SIMD]") == 8, block
    assert seen == LDS_BYTES, seen
