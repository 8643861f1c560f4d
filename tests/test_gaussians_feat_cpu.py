"""What semantic Gaussians can show without a GPU: the two fixed-rule functions against numpy, the fp32 definition
(tests/gaussians_feat_reference.py) against float64 autograd of a textbook renderer with features and F.cross_entropy, answers known
without arithmetic, and the C-ABI and generated code of csrc/gaussians_feat.hip."""
import os
import re

import numpy as np
import pytest
import torch

import gaussians_bwd_reference as gb
import gaussians_feat_reference as gf
import gaussians_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
ENTRIES = (("mudg_gauss_blend_feat", 20), ("mudg_gauss_blend_bwd_feat", 24), ("mudg_gauss_feat_bwd", 9), ("mudg_gauss_class_loss", 9),
           ("mudg_gauss_class_loss_finish", 7), ("mudg_gauss_class_loss_bwd", 10))
# The two fixed rules against numpy in float64 on dense grids, measured on the CPU: E's largest relative error on
# [-80, 0] and L's largest absolute error on [1, 32].  E's grows with |p|: p log2(e) is rounded to fp32 before it is split, half an ulp of
# a t near -115 is 3.8e-6, and 2^t carries ln 2 of that; on §23's own range [-5.55, 0] it stays below 2e-7.  The bounds below are twice
# the measured values: the grids do not visit every float.
E_RELATIVE, L_ABSOLUTE = 3.94e-6, 1.66e-7
# The fp32 rule against float64 autograd on gr.seeded_scene(400, (40, 56), 7) with F = 19 seeded scores and labels, the class loss (weight
# 1) on the blended scores plus seeded upstream gradients for rgb, depth and alpha, zeroed (unlabelled) on the 0.85 % of the pixels the
# textbook's margins exclude: the largest difference relative to the group's largest gradient, measured on the CPU.  The bound is four
# times the measured value, the margin DESIGN.md §23 chose for float64's accumulation order.
MEASURED = {"xyz": 1.55e-6, "cov": 1.10e-6, "opacity": 5.2e-7, "colour": 3.1e-7, "features": 2.7e-7, "feat_out": 1.22e-6, "loss": 5.6e-8}


# ------------------------------------------------------------------------------------------------ the two fixed rules
def test_the_exponential_and_the_logarithm_against_numpy():
    p = np.linspace(-80.0, 0.0, 1 << 20).astype(F)
    e = gr.exp_rule(p)
    rel = np.abs(e.astype(D) - np.exp(p.astype(D))) / np.exp(p.astype(D))
    s = np.linspace(1.0, 32.0, 1 << 18).astype(F)
    l = gf.log_rule(s)
    err = np.abs(l.astype(D) - np.log(s.astype(D)))
    print(f"E on [-80, 0]: largest relative error {rel.max():.3e} (recorded {E_RELATIVE}); L on [1, 32]: largest absolute error {err.max():.3e} "
          f"(recorded {L_ABSOLUTE})")
    assert rel.max() <= 2 * E_RELATIVE and err.max() <= 2 * L_ABSOLUTE
    assert gf.log_rule(F(1.0)) == 0 and not np.signbit(gf.log_rule(F(1.0))) and gr.exp_rule(F(0.0)) == 1
    assert (np.diff(e) >= 0).all() and (np.diff(l) >= 0).all()                               # non-decreasing on the grids
    assert e.min() > 0 and np.isfinite(e).all() and e[0] >= np.finfo(F).tiny                 # the floor of -80 keeps E a normal number
    seam = np.nextafter(gf.SQRT_HALF * F(2.0), F(0.0))                                        # either side of the mantissa's split
    around = np.array([seam, gf.SQRT_HALF * F(2.0), np.nextafter(gf.SQRT_HALF * F(2.0), F(4.0))], F)
    assert (np.abs(gf.log_rule(around).astype(D) - np.log(around.astype(D))) <= 2 * L_ABSOLUTE).all()


# ------------------------------------------------------------------------------------------------ the rule against float64 autograd
def test_the_fp32_rule_follows_float64_autograd_of_a_textbook_renderer_and_cross_entropy():
    hw, Fn = (40, 56), 19
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene(400, hw, 7)
    _, _, near = gr.textbook_render(xyz, rgb, cov, opacity, mats[0, 0], cam, hw)
    assert near.mean() <= 0.05
    rng = np.random.default_rng(19)
    feat = (rng.normal(size=(len(xyz), Fn)) * 3.0).astype(F)
    labels = rng.integers(0, Fn, (1,) + hw).astype(np.uint8)
    labels[0][near] = 255
    d_rgb, d_depth, d_alpha = (rng.normal(size=(1, 3) + hw).astype(F), (rng.normal(size=(1,) + hw) * 0.05).astype(F), rng.normal(size=(1,) + hw).astype(F))
    for a in (d_rgb, d_depth, d_alpha):
        a[..., near] = 0
    proj = gr.project(xyz, cov, opacity, None, mats, cam, hw)
    keys, values, order, ranges, offsets = gb.bin_with_order(proj, hw)
    colour = rgb.astype(F)
    _, _, _, state, feat_out = gf.blend_feat(proj, colour, feat, values, ranges, hw)
    maps, _, totals = gf.class_loss(feat_out, labels, 1.0)
    d_feat = gf.class_loss_bwd(maps, totals, 1.0, 1.0)
    partial, partial_feat = gf.blend_bwd_feat(proj, colour, feat, values, order, ranges, hw, state, feat_out, d_rgb, d_depth, d_alpha, d_feat)
    d_xyz, d_cov, d_op, d_col = gb.project_bwd(xyz, cov, None, mats, cam, hw, proj["count"], offsets, partial)
    d_features = gf.feat_bwd(proj["count"], offsets, partial_feat)

    t64 = lambda a: torch.tensor(np.asarray(a, dtype=F).astype(D), requires_grad=True)
    tx, tc, tf, tv, to = t64(xyz), t64(rgb), t64(feat), t64(cov), t64(opacity)
    r, d, a, f = gf.textbook_features(tx, tc, tf, tv, to, mats, cam, hw)
    target = torch.from_numpy(np.where(labels < Fn, labels.astype(np.int64), -100))
    ce = torch.nn.functional.cross_entropy(f, target, ignore_index=-100)
    (ce + (r * torch.tensor(d_rgb.astype(D))).sum() + (d * torch.tensor(d_depth.astype(D))).sum() + (a * torch.tensor(d_alpha.astype(D))).sum()).backward()
    keep = ~near
    got = {"feat_out": np.abs(feat_out[0] - f[0].detach().numpy())[:, keep].max() / np.abs(f[0].detach().numpy()).max(),
           "loss": abs(float(totals[3]) - float(ce.detach())) / float(ce.detach())}
    for name, mine, want in (("xyz", d_xyz, tx.grad), ("cov", d_cov, tv.grad), ("opacity", d_op, to.grad), ("colour", d_col, tc.grad),
                             ("features", d_features, tf.grad)):
        want = want.numpy()
        assert np.abs(want).max() > 0
        got[name] = np.abs(mine.astype(D) - want).max() / np.abs(want).max()
    print(f"{near.mean():.4f} of the pixels excluded, {len(values)} entries, {int(totals[1:2].view(np.int32)[0])} labelled pixels, loss {float(ce.detach()):.5f}")
    for name, err in got.items():
        print(f"{name}: relative difference {err:.3e} (bound {4 * MEASURED[name]:.3e})")
    for name, err in got.items():
        assert err <= 4 * MEASURED[name], name


# ------------------------------------------------------------------------------------------------ answers known without arithmetic
def _flat(centres, scale, hw, Fn, **kw):
    pts, cov, op = gr.flat_case(centres, scale, **kw)
    xyz, words = gr.unpack(pts)
    colour = np.stack([(words >> (8 * k)) & 0xff for k in range(3)], axis=1).astype(F)
    feat = (np.random.default_rng(3).normal(size=(len(xyz), Fn)) * 2.0).astype(F)
    return xyz, colour, feat, cov, op


def test_one_opaque_gaussian_at_a_pixel_centre_gives_its_scores_times_the_cap():
    xyz, colour, feat, cov, op = _flat([[8.5, 8.5]], 0.5, (16, 16), 19)
    zero = lambda *s: np.zeros(s, F)
    out = gf.render_backward(xyz, colour, feat, cov, op, None, gr.FLAT[None], gr.FLAT_CAM, (16, 16), zero(1, 3, 16, 16), zero(1, 16, 16),
                             zero(1, 16, 16), zero(1, 19, 16, 16))
    assert np.array_equal(out["feat_out"][0, :, 8, 8], feat[0] * gr.MAX_ALPHA) and out["alpha"][0, 8, 8] == gr.MAX_ALPHA
    assert not out["partial"].any() and not out["partial_feat"].any() and not out["d_feat_g"].any()


def test_no_upstream_for_the_features_leaves_the_existing_partials_and_images():
    hw = (40, 56)
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene(400, hw, 7)
    rng = np.random.default_rng(2)
    feat = rng.normal(size=(len(xyz), 19)).astype(F)
    up = (rng.normal(size=(1, 3) + hw).astype(F), (rng.normal(size=(1,) + hw) * 0.05).astype(F), rng.normal(size=(1,) + hw).astype(F))
    out = gf.render_backward(xyz, rgb.astype(F), feat, cov, opacity, None, mats, cam, hw, *up, np.zeros((1, 19) + hw, F))
    ref = gb.render_backward(xyz, rgb.astype(F), cov, opacity, None, mats, cam, hw, *up)
    for k in ("rgb", "depth_image", "alpha", "state", "partial", "d_xyz", "d_cov", "d_opacity", "d_colour"):
        assert torch.equal(torch.from_numpy(out[k]), torch.from_numpy(ref[k])), k
    assert not out["partial_feat"].any() and out["feat_out"].any()


def test_the_features_gradient_is_the_sum_of_the_weights_times_the_upstream():
    """feat_out is linear in feat: with an upstream of one at a single pixel and channel, d_feat_g[g][k] is w_g at that pixel, and the
    weights of all entries add up to the pixel's alpha when no entry is capped or skipped late."""
    xyz, colour, feat, cov, op = _flat([[6.0, 6.0], [7.0, 6.5], [5.5, 7.0]], 2.0, (16, 16), 3, opacity=0.4, z=[100.0, 120.0, 140.0])
    zero = lambda *s: np.zeros(s, F)
    d_feat = zero(1, 3, 16, 16)
    d_feat[0, 1, 6, 6] = 1.0
    out = gf.render_backward(xyz, colour, feat, cov, op, None, gr.FLAT[None], gr.FLAT_CAM, (16, 16), zero(1, 3, 16, 16), zero(1, 16, 16),
                             zero(1, 16, 16), d_feat)
    w = out["d_feat_g"][:, 1]
    assert (w > 0).all() and not out["d_feat_g"][:, [0, 2]].any()
    assert abs(float(w.astype(D).sum()) - float(out["alpha"][0, 6, 6])) <= 4e-7
    assert abs(float((w.astype(D) * feat[:, 1]).sum()) - float(out["feat_out"][0, 1, 6, 6])) <= 1e-6
    assert out["d_opacity"].any() and out["d_xyz"].any()                                     # the scores pull on the geometry too


def test_the_class_loss_on_answers_known_without_arithmetic():
    hw = (17, 33)
    rng = np.random.default_rng(4)
    x = rng.normal(size=(2, 1) + hw).astype(F)
    maps, partial, totals = gf.class_loss(x, np.zeros((2,) + hw, np.uint8))
    assert not maps.any() and not np.signbit(maps).any() and totals[0] == 0 and totals[3] == 0          # F = 1: the map is +0
    assert totals[1:2].view(np.int32)[0] == 2 * 17 * 33 and totals[2] == 2 * 17 * 33
    x = rng.normal(size=(2, 19) + hw).astype(F)
    for none in (19, 200, 255):                                                                         # every label >= F is unlabelled
        maps, partial, totals = gf.class_loss(x, np.full((2,) + hw, none, np.uint8), 0.5)
        assert not maps.any() and not np.signbit(maps).any() and not partial.view(np.int32).any()
        assert totals.view(np.int32).tolist() == [0, 0, np.array([1.0], F).view(np.int32)[0], 0]
        assert not gf.class_loss_bwd(maps, totals, 1.0, 0.5).any()
    labels = rng.integers(0, 19, (2,) + hw).astype(np.uint8)
    sure = np.full((2, 19) + hw, -30.0, F)
    np.put_along_axis(sure, labels[:, None].astype(np.int64), F(30.0), axis=1)                            # the label wins by a margin of 60
    maps, _, totals = gf.class_loss(sure, labels)
    assert 0 <= totals[3] <= 1e-6 and np.abs(maps).max() <= 1e-6
    labels[1] = 255                                                                                     # an unlabelled view beside a labelled one
    maps, partial, totals = gf.class_loss(x, labels)
    assert maps[0].any() and not maps[1].any() and totals[1:2].view(np.int32)[0] == 17 * 33
    rows = np.take_along_axis(maps[0], labels[0][None].astype(np.int64), axis=0)[0]
    assert (rows < 0).all() and np.abs(maps[0].astype(D).sum(axis=0)).max() <= 1e-6                     # softmax - onehot sums to zero
    ref = torch.nn.functional.cross_entropy(torch.from_numpy(x[:1].astype(D)), torch.from_numpy(labels[:1].astype(np.int64)))
    assert abs(float(totals[3]) - float(ref)) <= 1e-5 * float(ref)


def test_label_images():
    feat = np.zeros((1, 3, 2, 2), F)
    feat[0, :, 0, 0] = [1, 5, 5]                                                                        # a tie: the lowest index
    feat[0, :, 0, 1] = [-1, -2, -3]
    alpha = np.array([[[0.9, 0.5], [0.51, 0.0]]], F)
    assert gf.labels_of(feat, alpha).tolist() == [[[1, 255], [0, 255]]]
    from mudg_amd import gaussians
    got = gaussians.label_image(torch.from_numpy(feat), torch.from_numpy(alpha))
    assert got.dtype == torch.uint8 and got.tolist() == [[[1, 255], [0, 255]]]
    assert gaussians.label_image(torch.from_numpy(feat), torch.from_numpy(alpha), 0.6).tolist() == [[[1, 255], [255, 255]]]


# ------------------------------------------------------------------------------------------------ the Python surface off the GPU
def test_tensors_off_the_gpu_and_bad_widths_are_refused():
    from mudg_amd import gaussians, hip, ops
    f = lambda *s: torch.zeros(s)
    n = 3
    entries = (f(n, 3), f(n, 19), f(1, n, 2), f(1, n, 4), f(1, n), torch.zeros(2, dtype=torch.int32), torch.zeros((1, 2), dtype=torch.int32), (16, 16))
    for call in (lambda: ops.gauss_blend_feat(*entries), lambda: ops.gauss_feat_bwd(torch.zeros((1, n), dtype=torch.int32), torch.zeros((1, n), dtype=torch.int64), f(2, 19)),
                 lambda: ops.gauss_class_loss(f(1, 19, 16, 16), torch.zeros((1, 16, 16), dtype=torch.uint8)),
                 lambda: gaussians.class_loss(f(1, 19, 16, 16), torch.zeros((1, 16, 16), dtype=torch.uint8)),
                 lambda: gaussians.render_differentiable(f(n, 3), f(n, 3), f(n, 6), f(n), f(1, 1, 12), (1.0, 1.0, 0.0, 0.0), (16, 16), features=f(n, 19))):
        with pytest.raises(hip.MudgError, match="on the GPU"):
            call()
    with pytest.raises(hip.MudgError, match="1 <= F <= 32"):
        gaussians.render_differentiable(f(n, 3), f(n, 3), f(n, 6), f(n), f(1, 1, 12), (1.0, 1.0, 0.0, 0.0), (16, 16), features=f(n, 33))
    with pytest.raises(hip.MudgError, match="weight"):
        gaussians.class_loss(f(1, 19, 16, 16), torch.zeros((1, 16, 16), dtype=torch.uint8), weight=-1.0)
    assert ops.GAUSS_FEAT_MAX == gf.FEAT_MAX == 32 and gaussians.CLASS_LEARNING_RATE > 0
    source = open(os.path.join(ROOT, "mudg_amd", "csrc", "gaussians_feat.hip")).read()
    assert [int(v) for v in re.findall(r"constexpr int FEAT_MAX = (\d+);", source)] == [ops.GAUSS_FEAT_MAX]
    written = [F(float.fromhex(m)) for m in re.findall(r"-?0x1\.[0-9a-f]+p[-+]\d+", source)]
    for c in gf.LOG_COEFFICIENTS[:-1] + (gf.SQRT_HALF, gf.LN2):                                         # the kernel's constants are the rule's
        assert c in written, float(c).hex()
    for d in ("mudg_amd", "lvdm", "virtual_render", "main", "tools"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for name in files:
                if name.endswith(".py"):
                    assert "gaussians_feat_reference" not in open(os.path.join(base, name)).read(), name


# ------------------------------------------------------------------------------------------------ C-ABI and generated code
def test_entry_points_are_declared_bound_and_exported():
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
    assert "gaussians_feat.hip" in build.SOURCES


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

    # colours colour_views feat F uv conic depth values ranges n E V H W rgb depth alpha feat_out state stream
    good = [one, 0, one, 19, one, one, one, one, one, 10, 5, 1, 32, 32, one, one, one, one, one, None]
    fn = lib.mudg_gauss_blend_feat
    for k in (0, 2, 4, 5, 6, 7, 8, 14, 15, 16, 17):                                 # state (18) may be null: inference
        refused(fn, good, {k: None}, b"null")
    for k in (4, 5):
        refused(fn, good, {k: odd}, b"unaligned")
    for v in (0, -1, 33):
        refused(fn, good, {3: v}, b"features")
    for v in (-1, 2):
        refused(fn, good, {1: v}, b"colour_views")
    for k in (9, 11, 12, 13):
        for v in (0, -1):
            refused(fn, good, {k: v})
    refused(fn, good, {9: 2 ** 31}, b"32-bit index")
    for e in (0, -1, 2 ** 31):
        refused(fn, good, {10: e}, b"entries")
    refused(fn, good, {11: 2 ** 20, 12: 1024, 13: 1024}, b"2^31")
    refused(fn, good, {12: 2 ** 23}, b"image")

    # colours colour_views feat F uv conic depth values order ranges n E V H W state feat_out d_rgb d_depth d_alpha d_feat partial partial_feat stream
    good = [one, 0, one, 19, one, one, one, one, one, one, 10, 5, 1, 32, 32, one, one, one, one, one, one, one, one, None]
    fn = lib.mudg_gauss_blend_bwd_feat
    for k in (0, 2, 4, 5, 6, 7, 8, 9, 15, 16, 17, 18, 19, 20, 21, 22):
        refused(fn, good, {k: None}, b"null")
    for k in (4, 5, 8):
        refused(fn, good, {k: odd}, b"unaligned")
    for v in (0, -1, 33):
        refused(fn, good, {3: v}, b"features")
    for v in (-1, 2):
        refused(fn, good, {1: v}, b"colour_views")
    for k in (10, 12, 13, 14):
        for v in (0, -1):
            refused(fn, good, {k: v})
    for e in (0, -1, 2 ** 31, 2 ** 40):
        refused(fn, good, {11: e}, b"entries")
    refused(fn, good, {11: 2 ** 31 // 19 + 1}, b"E F < 2^31")
    refused(fn, good, {3: 32, 11: 2 ** 26}, b"E F < 2^31")                          # E F = 2^31 exactly
    refused(fn, good, {12: 2 ** 20, 13: 1024, 14: 1024}, b"2^31")

    # count offsets partial_feat E n V F d_feat_g stream
    good = [one, one, one, 5, 10, 1, 19, one, None]
    fn = lib.mudg_gauss_feat_bwd
    for k in (0, 1, 2, 7):
        refused(fn, good, {k: None}, b"null")
    refused(fn, good, {1: odd}, b"unaligned")
    for v in (0, -1, 33):
        refused(fn, good, {6: v}, b"features")
    for k in (4, 5):
        for v in (0, -1):
            refused(fn, good, {k: v}, b"Gaussians")
    refused(fn, good, {4: 2 ** 31}, b"Gaussians")
    for e in (0, -1, 2 ** 31):
        refused(fn, good, {3: e}, b"entries")
    refused(fn, good, {3: 2 ** 27}, b"E F < 2^31")

    # x labels V F H W maps partial stream
    good = [one, one, 1, 19, 32, 32, one, one, None]
    fn = lib.mudg_gauss_class_loss
    for k in (0, 1, 6, 7):
        refused(fn, good, {k: None}, b"null")
    for k in (0, 6, 7):
        refused(fn, good, {k: ctypes.c_void_p(18)}, b"unaligned")
    for v in (0, -1, 33):
        refused(fn, good, {3: v}, b"features")
    for k in (2, 4, 5):
        for v in (0, -1):
            refused(fn, good, {k: v})
    refused(fn, good, {2: 2 ** 20, 4: 1024, 5: 1024}, b"2^31")

    # partial V H W weight totals stream
    good = [one, 1, 32, 32, 0.5, one, None]
    fn = lib.mudg_gauss_class_loss_finish
    for k in (0, 5):
        refused(fn, good, {k: None}, b"null")
        refused(fn, good, {k: ctypes.c_void_p(18)}, b"unaligned")
    for k in (1, 2, 3):
        for v in (0, -1):
            refused(fn, good, {k: v})
    for v in (-0.5, nan, inf):
        refused(fn, good, {4: v}, b"weight")

    # maps totals up weight V F H W d_x stream
    good = [one, one, one, 0.5, 1, 19, 32, 32, one, None]
    fn = lib.mudg_gauss_class_loss_bwd
    for k in (0, 1, 2, 8):
        refused(fn, good, {k: None}, b"null")
        refused(fn, good, {k: ctypes.c_void_p(18)}, b"unaligned")
    for v in (0, -1, 33):
        refused(fn, good, {5: v}, b"features")
    for k in (4, 6, 7):
        for v in (0, -1):
            refused(fn, good, {k: v})
    for v in (-0.5, nan, inf):
        refused(fn, good, {3: v}, b"weight")


def test_kernels_use_no_scratch_no_atomics_and_keep_their_lds(tmp_path):
    """Facts about the generated gfx950 code as DESIGN.md §29 records them: no scratch and no spill in any kernel, no atomic on global
    memory, no flat access, no hardware exponential or logarithm; the blend's backward stays at or below 64 KiB of LDS for every
    template bound (12 KiB of entries, 32 rows of features and the four waves' sums of 32 entries), so two workgroups fit a CU."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "gaussians_feat.s"
    subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S",
                    os.path.join(ROOT, "mudg_amd", "csrc", "gaussians_feat.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    s = out.read_text()
    md = s[s.index("amdhsa.kernels"):]
    seen = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", md, re.S):
        kind = re.search(r"gauss_(blend_feat|blend_bwd_feat|feat_bwd|class_loss_finish|class_loss_bwd|class_loss)_kernel(?:ILi(\d+)E)?", m.group(2))
        assert kind, m.group(2)
        seen[(kind.group(1), int(kind.group(2) or 0))] = (int(m.group(1)), int(m.group(4)))
        print(f"{m.group(2)}: {m.group(1)} bytes of LDS, {m.group(4)} VGPRs")
        assert int(m.group(3)) == 0 and int(m.group(5)) == 0, m.groups()
    bounds = (4, 8, 16, 24, 32)
    assert set(seen) == {(k, b) for k in ("blend_feat", "blend_bwd_feat", "class_loss") for b in bounds} | {("feat_bwd", 0), ("class_loss_finish", 0),
                                                                                                           ("class_loss_bwd", 0)}, seen
    for b in bounds:
        assert 12288 + 256 * b * 4 <= seen[("blend_feat", b)][0] <= 12288 + 256 * b * 4 + 256
        want = 12288 + 32 * b * 4 + 4 * 32 * (10 + b) * 4
        assert want <= seen[("blend_bwd_feat", b)][0] <= want + 256 and seen[("blend_bwd_feat", b)][0] <= 65536 // 2 + 8192
        assert seen[("blend_bwd_feat", b)][1] <= 128 and seen[("blend_feat", b)][1] <= 128
    for name in sorted(set(re.findall(r"^(_Z\S*gauss_\w+_kernel\S*):", s, re.M))):
        body = s[s.index(name + ":"):]
        lines = [l.strip() for l in body[:body.index(".end_amdhsa_kernel")].splitlines()]
        assert not any(l.startswith(("scratch_", "flat_", "global_atomic", "buffer_atomic")) for l in lines), name
        assert not any(l.startswith(("v_exp_f32", "v_log_f32")) for l in lines), name                  # the polynomials, not the hardware's
