"""What the backward rule of the Gaussian splat renderer can show without a GPU: the fp32 definition
(tests/gaussians_bwd_reference.py) against float64 autograd of a textbook renderer and against answers known without arithmetic, the
model's parametrisation against float64 autograd, the fit in float64, and the C-ABI and generated code of csrc/gaussians_bwd.hip."""
import os
import re

import numpy as np
import pytest
import torch

import gaussians_bwd_reference as gb
import gaussians_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
ENTRIES = (("mudg_gauss_blend_train", 16), ("mudg_gauss_blend_bwd", 18), ("mudg_gauss_project_bwd", 24))
# The fp32 rule against float64 autograd on gr.seeded_scene(400, (40, 56), 7) with seeded upstream gradients, zeroed on the 0.85 % of the
# pixels the textbook's margins exclude: the largest difference relative to the group's largest gradient, measured on the CPU.  The bound
# is four times the measured value, the margin DESIGN.md §23 chose for float64's accumulation order.
MEASURED = {"xyz": 1.43e-6, "cov": 1.02e-6, "opacity": 6.1e-7, "colour": 3.5e-7}
# The float64 fit of gb.fit_problem(): final / initial loss after 200 Adam steps, measured on the CPU.
R64 = 0.0119


def _upstream(hw, near=None, seed=11, views=1):
    rng = np.random.default_rng(seed)
    d_rgb = rng.normal(size=(views, 3) + hw).astype(F)
    d_depth = (rng.normal(size=(views,) + hw) * 0.05).astype(F)
    d_alpha = rng.normal(size=(views,) + hw).astype(F)
    if near is not None:
        for a in (d_rgb, d_depth, d_alpha):
            a[..., near] = 0
    return d_rgb, d_depth, d_alpha


# ------------------------------------------------------------------------------------------------ the rule against float64 autograd
def test_the_fp32_backward_rule_follows_float64_autograd():
    hw = (40, 56)
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene(400, hw, 7)
    _, _, near = gr.textbook_render(xyz, rgb, cov, opacity, mats[0, 0], cam, hw)
    assert near.mean() <= 0.05
    d_rgb, d_depth, d_alpha = _upstream(hw, near)
    out = gb.render_backward(xyz, rgb.astype(F), cov, opacity, None, mats, cam, hw, d_rgb, d_depth, d_alpha)
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=F).astype(D), requires_grad=True)
    tx, tc, tv, to = t64(xyz), t64(rgb), t64(cov), t64(opacity)
    r, d, a = gb.textbook(tx, tc, tv, to, mats, cam, hw)
    ((r * torch.tensor(d_rgb.astype(D))).sum() + (d * torch.tensor(d_depth.astype(D))).sum() + (a * torch.tensor(d_alpha.astype(D))).sum()).backward()
    keep = ~near
    assert np.abs(out["rgb"][0] - r[0].detach().numpy())[:, keep].max() <= 4 * 1.18e-6        # §23's bound: the same forward
    print(f"{near.mean():.4f} of the pixels excluded, {out['entries']} entries")
    for name, mine, want in (("xyz", out["d_xyz"], tx.grad), ("cov", out["d_cov"], tv.grad), ("opacity", out["d_opacity"], to.grad),
                             ("colour", out["d_colour"], tc.grad)):
        want = want.numpy()
        err = np.abs(mine.astype(D) - want).max() / np.abs(want).max()
        print(f"{name}: largest gradient {np.abs(want).max():.4g}, relative difference {err:.3e} (bound {4 * MEASURED[name]:.3e})")
        assert np.abs(want).max() > 0 and err <= 4 * MEASURED[name], name


def test_whole_byte_colours_through_the_training_blend_are_the_byte_blend():
    hw = (40, 56)
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene(400, hw, 7)
    ref = gr.render(gr.pack(xyz, rgb), cov, opacity, None, mats, cam, hw)
    proj = gr.project(xyz, cov, opacity, None, mats, cam, hw)
    got_rgb, got_depth, got_alpha, state = gb.blend_train(proj, rgb.astype(F), ref["values"], ref["ranges"], hw)
    assert np.array_equal(got_rgb, ref["rgb"]) and np.array_equal(got_depth, ref["depth_image"]) and np.array_equal(got_alpha, ref["alpha"])
    assert np.array_equal(state[:, 3], ref["depth_image"]) and np.array_equal(F(1.0) - state[:, 4], ref["alpha"])
    order = gb.bin_with_order(proj, hw)[2]
    assert sorted(order.tolist()) == list(range(ref["entries"]))


# ------------------------------------------------------------------------------------------------ answers known without arithmetic
def _flat_backward(centres, scale, hw, pixel, d_depth_at=0.0, **kw):
    pts, cov, op = gr.flat_case(centres, scale, **kw)
    xyz, words = gr.unpack(pts)
    colour = np.stack([(words >> (8 * k)) & 0xff for k in range(3)], axis=1).astype(F)
    d_rgb, d_depth, d_alpha = np.zeros((1, 3) + hw, F), np.zeros((1,) + hw, F), np.zeros((1,) + hw, F)
    d_rgb[0, :, pixel[0], pixel[1]] = [0.5, -2.0, 3.0]
    d_alpha[0, pixel[0], pixel[1]] = 1.5
    d_depth[0, pixel[0], pixel[1]] = d_depth_at
    return d_rgb, gb.render_backward(xyz, colour, cov, op, None, gr.FLAT[None], gr.FLAT_CAM, hw, d_rgb, d_depth, d_alpha)


def test_the_alpha_cap_passes_colour_and_nothing_else():
    d_rgb, out = _flat_backward([[8.5, 8.5]], 0.5, (16, 16), (8, 8))
    assert out["alpha"][0, 8, 8] == gr.MAX_ALPHA                                             # opacity g = 1 > 0.99: the cap took effect
    assert out["d_colour"][0].tolist() == [(g / F(255.0)) * gr.MAX_ALPHA for g in d_rgb[0, :, 8, 8]]
    assert not out["d_opacity"].any() and not out["d_xyz"].any() and not out["d_cov"].any()
    assert not out["partial"][0, 3:].any()


def test_a_pixel_that_finishes_gives_nothing_to_the_stopping_entry_or_behind_it():
    _, out = _flat_backward([[8.5, 8.5]] * 3, 0.5, (16, 16), (8, 8), d_depth_at=1.0, z=[128.0, 160.0, 192.0])
    assert out["values"].tolist() == [0, 1, 2] and out["order"].tolist() == [0, 1, 2]
    assert out["partial"][0, :4].all() and not out["partial"][1:].any()
    for k in ("d_xyz", "d_cov", "d_opacity", "d_colour"):
        assert not out[k][1:].any(), k
    assert out["d_xyz"][0, 2] == F(1.0) * gr.MAX_ALPHA and not out["d_xyz"][0, :2].any()     # the depth term alone: d zc / d z = 1


def test_a_dropped_gaussian_has_zero_gradients():
    _, out = _flat_backward([[8.5, 8.5], [8.5, 8.5], [200.0, 8.5]], 3.0, (16, 16), (6, 10), d_depth_at=1.0, opacity=0.5,
                            z=[128.0, 0.1, 128.0])                                          # a pixel off the centre: dx, dy != 0
    assert out["count"][0].tolist() == [1, 0, 0]                                             # in front of znear; off the image
    for k in ("d_xyz", "d_cov", "d_opacity", "d_colour"):
        assert out[k][0].any() and not out[k][1:].any(), k


def test_entries_behind_a_finished_tile_have_zero_partials():
    n = 2 + 556
    z = np.concatenate([[100.0, 101.0], np.linspace(110.0, 190.0, 556)]).astype(F)
    pts, cov, op = gr.flat_case([[8.0, 8.0]] * n, 60.0, z=z)
    xyz, _ = gr.unpack(pts)
    d_rgb, d_depth, d_alpha = _upstream((16, 16))
    out = gb.render_backward(xyz, np.full((n, 3), 100, F), cov, op, None, gr.FLAT[None], gr.FLAT_CAM, (16, 16), d_rgb, d_depth, d_alpha)
    assert out["entries"] == n and out["walked"].tolist() == [256]                           # the second batch is never staged
    assert (out["alpha"] == gr.MAX_ALPHA).all()                                              # the first is capped everywhere, the second ends every pixel
    assert out["partial"][0, :4].all() and not out["partial"][1:].any()
    assert not out["d_colour"][1:].any() and not out["d_xyz"][1:].any()


# ------------------------------------------------------------------------------------------------ the model's parametrisation
def _host_model(n=50, seed=5):
    from mudg_amd import gaussians
    rng = np.random.default_rng(seed)
    m = gaussians.GaussianModel.__new__(gaussians.GaussianModel)
    m.xyz = torch.tensor(rng.normal(size=(n, 3)).astype(F), requires_grad=True)
    m.colour = torch.tensor(rng.uniform(0, 255, (n, 3)).astype(F), requires_grad=True)
    m.log_scale = torch.tensor(rng.uniform(-3, 0.5, (n, 3)).astype(F), requires_grad=True)
    m.quat = torch.tensor(rng.normal(size=(n, 4)).astype(F), requires_grad=True)
    m.opacity_logit = torch.tensor(rng.normal(size=n).astype(F) * 3, requires_grad=True)
    m.ids = None
    return m


def test_scales_quaternions_and_activations_against_float64_autograd():
    m = _host_model()
    rng = np.random.default_rng(6)
    g_cov, g_op = rng.normal(size=(50, 6)), rng.normal(size=50)
    ((m.covariance() * torch.tensor(g_cov, dtype=torch.float32)).sum() + (m.opacity() * torch.tensor(g_op, dtype=torch.float32)).sum()).backward()
    ls, q, ol = (t.detach().double().requires_grad_(True) for t in (m.log_scale, m.quat, m.opacity_logit))
    cov64, op64 = gb.covariance64(ls, q), torch.sigmoid(ol)
    ((cov64 * torch.tensor(g_cov)).sum() + (op64 * torch.tensor(g_op)).sum()).backward()
    # a few dozen fp32 roundings on values of size max(s)^2 <= e: 1e-5 relative to the largest entry is several times their sum
    assert (m.covariance().detach().double() - cov64.detach()).abs().max() <= 1e-5 * cov64.detach().abs().max()
    assert (m.opacity().detach().double() - op64.detach()).abs().max() <= 1e-6
    for mine, want in ((m.log_scale.grad, ls.grad), (m.quat.grad, q.grad), (m.opacity_logit.grad, ol.grad)):
        assert (mine.double() - want).abs().max() <= 1e-5 * want.abs().max()
    assert m.xyz.grad is None and set(m.parameters()) == {"xyz", "colour", "log_scale", "quat", "opacity_logit"}


# ------------------------------------------------------------------------------------------------ the fit in float64
def test_the_float64_fit_lowers_the_loss():
    from mudg_amd import gaussians
    start, views, cam, targets = gb.fit_problem()
    losses = gb.textbook_fit(start, views, cam, targets, (40, 56), gaussians.LEARNING_RATES, 200, gaussians.ADAM_BETAS, gaussians.ADAM_EPS)
    ratio = losses[-1] / losses[0]
    print(f"float64 fit: loss {losses[0]:.5f} -> {losses[-1]:.5f}, ratio r64 = {ratio:.5f} (recorded {R64})")
    assert ratio < 0.5
    assert ratio <= 1.5 * R64                                                                # the recorded r64 is of this run's size


# ------------------------------------------------------------------------------------------------ the Python surface off the GPU
def test_tensors_off_the_gpu_are_refused():
    from mudg_amd import gaussians, hip, ops
    from virtual_render import virtual_pose_render
    n = 3
    f = lambda *s: torch.zeros(s)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    entries = (f(n, 3), f(1, n, 2), f(1, n, 4), f(1, n), i32(2), i32(1, 2), (16, 16))
    for call in (lambda: ops.gauss_blend_train(*entries),
                 lambda: ops.gauss_blend_bwd(*entries[:5], torch.zeros(2, dtype=torch.int64), *entries[5:], f(1, 5, 16, 16), f(1, 3, 16, 16),
                                             f(1, 16, 16), f(1, 16, 16)),
                 lambda: ops.gauss_project_bwd(i32(n, 4), f(n, 6), f(1, 1, 12), (1.0, 1.0, 0.0, 0.0), (16, 16), i32(1, n),
                                               torch.zeros((1, n), dtype=torch.int64), f(2, 10)),
                 lambda: gaussians.render_differentiable(f(n, 3), f(n, 3), f(n, 6), f(n), f(1, 1, 12), (1.0, 1.0, 0.0, 0.0), (16, 16)),
                 lambda: gaussians.GaussianModel(f(n, 3), f(n, 3), f(n, 3), f(n, 4), f(n))):
        with pytest.raises(hip.MudgError, match="on the GPU"):
            call()
    pc = gaussians.PointCloud.__new__(gaussians.PointCloud)
    pc.points = i32(n, 4)
    for make in (lambda: gaussians.GaussianModel.from_cloud(pc, 0.1), lambda: gaussians.GaussianModel.from_scene(pc, None, 0.1)):
        with pytest.raises(hip.MudgError, match="on the GPU"):
            make()
    m = _host_model(n)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        gaussians.fit(m, f(1, 3, 16, 16), f(1, 1, 12), (1.0, 1.0, 0.0, 0.0), (16, 16), iters=1)
    with pytest.raises(hip.MudgError, match="GaussianModel"):
        gaussians.fit(pc, f(1, 3, 16, 16), f(1, 1, 12), (1.0, 1.0, 0.0, 0.0), (16, 16), iters=1)
    assert callable(virtual_pose_render.fit_cloud_views) and ops.GAUSS_SUMS == gb.SUMS
    shared = open(os.path.join(ROOT, "mudg_amd", "csrc", "gauss_shared.h")).read()
    assert [int(v) for v in re.findall(r"constexpr int GAUSS_SUMS = (\d+);", shared)] == [ops.GAUSS_SUMS]
    assert [int(v) for v in re.findall(r"constexpr int TILE = (\d+);", shared)] == [ops.GAUSS_TILE]


def test_the_product_does_not_import_the_cpu_definition():
    for d in ("mudg_amd", "lvdm", "utils", "virtual_render", "main", "tools"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith(".py"):
                    assert "gaussians_bwd_reference" not in open(os.path.join(base, f)).read(), f


# ------------------------------------------------------------------------------------------------ C-ABI and generated code
def test_backward_entry_points_are_declared_bound_and_exported():
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
    assert "gaussians_bwd.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "mudg_amd", "csrc", "gauss_shared.h"))


def test_bad_arguments_are_refused_before_any_launch():
    import ctypes
    from mudg_amd import hip
    lib = hip.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)                              # never dereferenced: every call below is rejected first
    nan, inf = float("nan"), float("inf")

    def refused(fn, good, changes, text=None):
        args = list(good)
        for k, v in changes.items():
            args[k] = v
        assert fn(*args) == -1, (fn.__name__, changes)
        if text:
            assert text in lib.mudg_last_error(), (fn.__name__, changes, lib.mudg_last_error())

    # colour uv conic depth values ranges n E V H W rgb depth alpha state stream
    good = [one, one, one, one, one, one, 10, 5, 1, 32, 32, one, one, one, one, None]
    for k in (0, 1, 2, 3, 4, 5, 11, 12, 13, 14):
        refused(lib.mudg_gauss_blend_train, good, {k: None}, b"null")
    for k in (1, 2):
        refused(lib.mudg_gauss_blend_train, good, {k: odd}, b"unaligned")
    for k in (6, 8, 9, 10):
        for v in (0, -1):
            refused(lib.mudg_gauss_blend_train, good, {k: v})
    refused(lib.mudg_gauss_blend_train, good, {6: 2 ** 31}, b"32-bit index")
    for e in (0, -1, 2 ** 31):
        refused(lib.mudg_gauss_blend_train, good, {7: e}, b"entries")
    refused(lib.mudg_gauss_blend_train, good, {8: 2 ** 20, 9: 1024, 10: 1024}, b"2^31")
    refused(lib.mudg_gauss_blend_train, good, {9: 2 ** 23}, b"image")

    # colour uv conic depth values order ranges n E V H W state d_rgb d_depth d_alpha partial stream
    good = [one, one, one, one, one, one, one, 10, 5, 1, 32, 32, one, one, one, one, one, None]
    for k in (0, 1, 2, 3, 4, 5, 6, 12, 13, 14, 15, 16):
        refused(lib.mudg_gauss_blend_bwd, good, {k: None}, b"null")
    for k in (1, 2, 5):
        refused(lib.mudg_gauss_blend_bwd, good, {k: odd}, b"unaligned")
    for k in (7, 9, 10, 11):
        for v in (0, -1):
            refused(lib.mudg_gauss_blend_bwd, good, {k: v})
    for e in (0, -1, 2 ** 31, 2 ** 40):
        refused(lib.mudg_gauss_blend_bwd, good, {8: e}, b"entries")
    refused(lib.mudg_gauss_blend_bwd, good, {9: 2 ** 20, 10: 1024, 11: 1024}, b"2^31")
    refused(lib.mudg_gauss_blend_bwd, good, {9: 2 ** 19, 10: 1024, 11: 1024}, b"2^31")       # V NT = 2^31 exactly

    # points cov ids n mats V nmat H W fx fy cx cy znear zfar count offsets partial E d_xyz d_cov d_opacity d_colour stream
    good = [one, one, one, 10, one, 1, 2, 32, 32, 50.0, 50.0, 16.0, 16.0, 0.2, 200.0, one, one, one, 5, one, one, one, one, None]
    for k in (0, 1, 4, 15, 16, 17, 19, 20, 21, 22):
        refused(lib.mudg_gauss_project_bwd, good, {k: None}, b"null")
    refused(lib.mudg_gauss_project_bwd, good, {2: None}, b"ids")                      # two matrices per view and no ids
    refused(lib.mudg_gauss_project_bwd, good, {0: odd}, b"unaligned")
    refused(lib.mudg_gauss_project_bwd, good, {16: odd}, b"unaligned")
    for k in (3, 5, 6, 7, 8):
        for v in (0, -1):
            refused(lib.mudg_gauss_project_bwd, good, {k: v})
    refused(lib.mudg_gauss_project_bwd, good, {3: 2 ** 31}, b"32-bit index")
    refused(lib.mudg_gauss_project_bwd, good, {5: 2 ** 20, 7: 1024, 8: 1024}, b"2^31")
    for e in (0, -1, 2 ** 31):
        refused(lib.mudg_gauss_project_bwd, good, {18: e}, b"entries")
    for znear, zfar in ((0.0, 200.0), (-1.0, 200.0), (nan, 200.0), (0.2, nan), (0.2, inf), (inf, inf), (0.2, 0.2), (5.0, 1.0)):
        refused(lib.mudg_gauss_project_bwd, good, {13: znear, 14: zfar}, b"znear")
    for k in (9, 10):
        for v in (0.0, -50.0, nan, inf):
            refused(lib.mudg_gauss_project_bwd, good, {k: v}, b"intrinsics")
    refused(lib.mudg_gauss_project_bwd, good, {11: nan}, b"intrinsics")


def test_backward_kernels_use_no_scratch_no_atomics_and_keep_their_lds(tmp_path):
    """Facts about the generated gfx950 code as DESIGN.md §24 records them: no scratch and no spill in any kernel, no atomic on global
    memory, no flat access, no hardware exponential; LDS: 12 KiB of entries in the training blend, 12 KiB of entries and 40 KiB of
    per-wave sums in the blend's backward (plus the 256 bytes the counting barrier keeps), none in the projection's backward."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "gaussians_bwd.s"
    subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S",
                    os.path.join(ROOT, "mudg_amd", "csrc", "gaussians_bwd.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    s = out.read_text()
    md = s[s.index("amdhsa.kernels"):]
    seen = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", md, re.S):
        kind = re.search(r"gauss_(blend_train|blend_bwd|project_bwd)_kernel", m.group(2))
        assert kind, m.group(2)
        seen[kind.group(1)] = (int(m.group(1)), int(m.group(4)))
        print(f"{m.group(2)}: {m.group(1)} bytes of LDS, {m.group(4)} VGPRs")
        assert int(m.group(3)) == 0 and int(m.group(5)) == 0, m.groups()
    assert set(seen) == {"blend_train", "blend_bwd", "project_bwd"}, seen
    assert 12288 <= seen["blend_train"][0] <= 12288 + 256
    assert 12288 + 40960 <= seen["blend_bwd"][0] <= 12288 + 40960 + 256
    assert seen["project_bwd"][0] == 0
    assert seen["blend_train"][1] <= 64 and seen["blend_bwd"][1] <= 128 and seen["project_bwd"][1] <= 128
    for name in sorted(set(re.findall(r"^(_Z\S*gauss_\w+_kernel\S*):", s, re.M))):
        body = s[s.index(name + ":"):]
        lines = [l.strip() for l in body[:body.index(".end_amdhsa_kernel")].splitlines()]
        assert not any(l.startswith(("scratch_", "flat_", "global_atomic", "buffer_atomic")) for l in lines), name
        assert not any(l.startswith("v_exp_f32") for l in lines), name                # the polynomial, not the hardware exponential
