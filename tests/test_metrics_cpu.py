"""What the scoring rules can show without a GPU: the CPU definition (tests/metrics_reference.py) against brute-force
loops in Python integers and Fractions, against answers the definition gives exactly, against an independent float64 SSIM and
scikit-learn's confusion matrix, and the C-ABI and generated code of csrc/metrics.hip."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import metrics_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
ENTRIES = (("mudg_metric_sse", 7), ("mudg_metric_ssim", 7), ("mudg_metric_depth", 9), ("mudg_metric_confusion", 9))
# |mean SSIM of the definition - float64 Wang SSIM| measured on the seeded pair of the test below (printed there); the bound is four
# times that, and never above 1e-4: SSIM is reported to four decimals
SSIM_MEASURED = 3.01e-6
SSIM_BOUND = min(4 * SSIM_MEASURED, 1e-4)


# ------------------------------------------------------------------------------------------------ the window
def test_the_window_table_is_its_formula_sums_to_two_to_the_sixteen_and_is_symmetric():
    from mudg_amd import ops
    g = [np.exp(-((i - 5) ** 2) / 4.5) for i in range(11)]
    w = [int(np.rint(65536.0 * v / sum(g))) for v in g]
    w[5] += 65536 - sum(w)
    assert tuple(w) == ops.SSIM_WINDOW == tuple(int(v) for v in mr.WINDOW)
    assert sum(w) == 65536 and w == w[::-1] and all(v > 0 for v in w) and w[5] == max(w)
    src = open(os.path.join(ROOT, "mudg_amd", "csrc", "metrics.hip")).read()
    taps = re.search(r"#define SSIM_TAPS \{(.*?)\}", src).group(1)
    assert [int(t.strip().rstrip("u")) for t in taps.split(",")] == w                                       # the kernel's table
    assert 65025 * 65536 < 2 ** 32 and 65025 * 65536 * 65536 < 2 ** 48                                       # the moments' headroom


# ------------------------------------------------------------------------------------------------ colour
def test_sse_and_the_five_moments_equal_a_brute_force_loop_in_python_integers():
    rng = np.random.default_rng(1)
    H, W = 13, 12
    a, b = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    a[0, 0], b[0, 0] = 255, 0
    assert mr.sse(a, b) == sum((int(p) - int(q)) ** 2 for p, q in zip(a.reshape(-1), b.reshape(-1)))
    w = [int(v) for v in mr.WINDOW]
    for c in range(3):
        got = mr.ssim_moments(a[..., c], b[..., c])
        assert all(m.shape == (H - 10, W - 10) and m.dtype == np.int64 for m in got)
        for j in range(H - 10):
            for i in range(W - 10):
                want = [0] * 5
                for dj in range(11):
                    for di in range(11):
                        x, y, ww = int(a[j + dj, i + di, c]), int(b[j + dj, i + di, c]), w[dj] * w[di]
                        for k, v in enumerate((x, y, x * x, y * y, x * y)):
                            want[k] += ww * v
                assert [int(m[j, i]) for m in got] == want, (c, j, i)
                assert max(want) < 2 ** 48


def test_identical_frames_score_exactly_one_and_infinite_psnr():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (2, 17, 23, 3), dtype=np.uint8)
    got = mr.psnr_ssim(a, a.copy())
    n = 3 * 7 * 13
    assert got["sse"].tolist() == [0, 0] and got["ssim_sum"].tolist() == [n * 2 ** 32] * 2
    assert np.all(np.isinf(got["psnr"])) and np.all(got["psnr"] > 0) and got["ssim"].tolist() == [1.0, 1.0]


@pytest.mark.parametrize("va,vb", [(255, 0), (200, 100), (1, 2), (0, 0)])
def test_two_constant_frames_score_the_formula_evaluated_once(va, vb):
    a, b = np.full((1, 12, 14, 3), va, np.uint8), np.full((1, 12, 14, 3), vb, np.uint8)
    mx, my = D(va), D(vb)
    s = ((2.0 * (mx * my) + mr.C1) * (2.0 * 0.0 + mr.C2)) / (((mx * mx + my * my) + mr.C1) * ((0.0 + 0.0) + mr.C2))
    q = int(np.rint(s * 2.0 ** 32))
    for c in range(3):
        assert np.all(mr.ssim_q(a[0, ..., c], b[0, ..., c]) == q)
    got = mr.psnr_ssim(a, b)
    assert got["ssim_sum"].tolist() == [3 * 2 * 4 * q] and got["sse"].tolist() == [3 * 12 * 14 * (va - vb) ** 2]
    if va == 255 and vb == 0:
        assert got["psnr"][0] == 0.0 and abs(got["ssim"][0] - mr.C1 / (65025.0 + mr.C1)) < 2.0 ** -32


def test_the_definition_is_within_its_bound_of_an_independent_float64_wang_ssim():
    """scipy's correlate1d with the Gaussian itself (not quantised), float64 throughout, cropped to the valid region; one frame is noise, the
    other a smoothed copy plus noise.  The two differ only by the window's rounding (2^-17 per tap) and the 2^-32 grid."""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    H, W = 24, 32
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    smooth = ndimage.uniform_filter(a.astype(D), size=(1, 3, 1), mode="nearest")                       # three pixels along a row
    b = np.clip(np.rint(smooth + rng.normal(0, 12.0, (H, W, 3))), 0, 255).astype(np.uint8)
    g = np.exp(-(np.arange(11, dtype=D) - 5.0) ** 2 / 4.5)
    g /= g.sum()
    blur = lambda v: ndimage.correlate1d(ndimage.correlate1d(v, g, axis=0, mode="constant"), g, axis=1, mode="constant")[5:-5, 5:-5]
    values = []
    for c in range(3):
        x, y = a[..., c].astype(D), b[..., c].astype(D)
        mx, my = blur(x), blur(y)
        vx, vy, cxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
        values.append(((2 * mx * my + mr.C1) * (2 * cxy + mr.C2)) / ((mx * mx + my * my + mr.C1) * (vx + vy + mr.C2)))
    want = float(np.mean(values))
    got = float(mr.psnr_ssim(a[None], b[None])["ssim"][0])
    print(f"float64 Wang SSIM {want:.9f}, the definition {got:.9f}, difference {abs(got - want):.3e}, bound {SSIM_BOUND:.3e}")
    assert 0.2 < want < 0.8                                                                                  # neither near 0 nor near 1
    assert abs(got - want) <= SSIM_BOUND


# ------------------------------------------------------------------------------------------------ depth
def _depth_case():
    """5 x 7: no-return pixels, y outside the range on both sides, z = 0, a z that is not a number, and ratios on each side of every
    threshold, none within 1e-9 of one."""
    rng = np.random.default_rng(11)
    y = rng.uniform(1.0, 70.0, (5, 7)).astype(F)
    ratio = np.array([1.1, 1.24, 1.26, 1.5, 1.57, 1.9, 1.96, 2.5] * 5, dtype=D)[:35].reshape(5, 7)
    ratio[rng.random((5, 7)) < 0.5] **= -1                                                                   # z / y and y / z both occur
    z = (y.astype(D) * ratio).astype(F)
    y[0, :2] = 0.0
    y[1, 0], y[1, 1], y[1, 2], y[1, 3] = 0.05, 0.1, 80.0, 120.0                                              # 0.1 and 80 are fp32(0.1) > 0.1: inside; 80: outside
    z[2, 0], z[2, 1] = 0.0, np.nan
    return z, y


def test_the_depth_sums_equal_python_integers_and_fractions():
    z, y = _depth_case()
    got = mr.depth_sums(z, y)
    assert got == mr.depth_sums_exact(z, y) and got[7] == 0
    # counted by hand: 35 - 2 (no return) - 0.05 - 80 - 120 - the z that is not a number; fp32(0.1) is above the double 0.1
    assert float(F(0.1)) > 0.1 and got[0] == 35 - 2 - 3 - 1
    use = (y.astype(D) > 0.1) & (y.astype(D) < 80.0) & ~np.isnan(z)
    with np.errstate(divide="ignore"):
        t = np.maximum(z.astype(D) / y.astype(D), y.astype(D) / np.where(z == 0, np.nan, z.astype(D)))
    t[z == 0] = np.inf
    for th in mr.THRESHOLDS:
        assert np.abs(t[use] - th).min() > 1e-9
        assert (t[use] < th).any() and ((t[use] > th) & (t[use] < 2 * th)).any()                             # each side of every threshold
    assert got[4] < got[5] < got[6] < got[0]
    # the first counted pixel, entirely in Fractions
    j, i = np.argwhere(use)[0]
    zz, yy = Fraction(float(z[j, i])), Fraction(float(y[j, i]))
    e = abs(zz - yy)
    assert Fraction(abs(float(z[j, i]) - float(y[j, i]))) == e                                               # fp32 operands: the difference is exact
    assert abs(mr.rint_fraction(e * 2 ** 20) - e * 2 ** 20) <= Fraction(1, 2)
    scores = mr.depth_errors(z[None], y[None])
    assert abs(scores["mae"][0] - float(sum(abs(Fraction(float(a)) - Fraction(float(b))) for a, b in zip(np.clip(z[use], 0, 256), y[use])) / got[0])) < 2.0 ** -20
    assert np.isnan(mr.depth_errors(np.ones((1, 3, 3), F), np.zeros((1, 3, 3), F))["mae"][0])
    # the headroom at 2^24 pixels: e <= 256, r <= 256 / 2^-6
    assert 2 ** 24 * 256 * 2 ** 20 < 2 ** 62 and 2 ** 24 * 256 * 256 * 2 ** 20 < 2 ** 62 and 2 ** 24 * (256 * 64) * 2 ** 20 < 2 ** 62


# ------------------------------------------------------------------------------------------------ labels
def test_the_confusion_matrix_equals_scikit_learns_and_the_iou_a_hand_count():
    skm = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(13)
    gt = rng.integers(0, 19, (9, 11)).astype(np.int64)
    pred = np.where(rng.random((9, 11)) < 0.6, gt, rng.integers(0, 19, (9, 11))).astype(np.int64)
    gt[0, :3], gt[1, 0] = 255, -1                                                                            # ignored
    m, bad = mr.confusion(pred, gt)
    keep = (gt >= 0) & (gt < 19)
    assert bad == 0 and m.sum() == keep.sum() == 99 - 4
    assert np.array_equal(m, skm.confusion_matrix(gt[keep], pred[keep], labels=list(range(19))))
    pred[2, 2], gt[2, 2] = 19, 3                                                                             # an out-of-range prediction
    m2, bad2 = mr.confusion(pred, gt)
    assert bad2 == 1 and m2.sum() == m.sum() - 1
    # three classes by hand: gt 0 0 0 1 1 2 / pred 0 0 1 1 1 0: class 2 is predicted nowhere
    s = mr.segmentation_scores(np.array([[[0, 0, 1, 1, 1, 0]]], dtype=np.int64), np.array([[[0, 0, 0, 1, 1, 2]]], dtype=np.int64), classes=3)
    assert s["confusion"][0].tolist() == [[2, 1, 0], [0, 2, 0], [1, 0, 0]]
    assert s["iou"][0].tolist() == [2 / 4, 2 / 3, 0.0] and s["miou"][0] == (2 / 4 + 2 / 3 + 0.0) / 3 and s["pixel_acc"][0] == 4 / 6
    s = mr.segmentation_scores(np.array([[[0, 0, 1]]], dtype=np.int64), np.array([[[0, 0, 1]]], dtype=np.int64), classes=3)
    assert np.isnan(s["iou"][0, 2]) and s["miou"][0] == 1.0 and s["pixel_acc"][0] == 1.0                     # a class in neither map is not averaged


# ------------------------------------------------------------------------------------------------ the interface off the GPU
def test_inputs_off_the_gpu_raise():
    from mudg_amd import hip, metrics, ops
    from virtual_render import eval_tools
    u8, f32, i64 = torch.zeros(2, 16, 16, 3, dtype=torch.uint8), torch.zeros(2, 16, 16), torch.zeros(2, 16, 16, dtype=torch.int64)
    calls = (lambda: metrics.psnr_ssim(u8, u8), lambda: metrics.depth_errors(f32, f32), lambda: metrics.segmentation_scores(i64, i64),
             lambda: metrics.score_window({"color": u8}, color=u8), lambda: eval_tools.score_window({"depth": f32}, lidar_depth=f32),
             lambda: ops.metric_sse(u8, u8), lambda: ops.metric_ssim(u8, u8), lambda: ops.metric_depth(f32, f32), lambda: ops.metric_confusion(i64, i64))
    for call in calls:
        with pytest.raises(hip.MudgError, match="on the GPU"):
            call()
    assert metrics.score_window({}) == {}                                                                    # no truth: no keys


def test_the_product_does_not_import_the_cpu_definition():
    for d in ("mudg_amd", "lvdm", "utils", "virtual_render", "tools"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith(".py"):
                    assert "metrics_reference" not in open(os.path.join(base, f)).read(), f


# ------------------------------------------------------------------------------------------------ C-ABI and generated code
def test_metric_entry_points_are_declared_bound_and_exported():
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
    assert "metrics.hip" in build.SOURCES
    lib = hip.lib()
    one = ctypes.c_void_p(16)                                                        # never dereferenced: every call below is rejected first
    for fn in (lib.mudg_metric_sse, lib.mudg_metric_ssim):
        assert fn(None, None, 1, 16, 16, None, None) == -1
        assert fn(one, one, 1, 4097, 4096, one, None) == -1 and b"2^24" in lib.mudg_last_error()
        assert fn(one, one, 0, 16, 16, one, None) == -1 and fn(one, one, 65536, 16, 16, one, None) == -1
    assert lib.mudg_metric_ssim(one, one, 1, 10, 16, one, None) == -1 and b"11 x 11" in lib.mudg_last_error()
    assert lib.mudg_metric_ssim(one, one, 1, 16, 10, one, None) == -1
    assert lib.mudg_metric_depth(None, None, 1, 8, 8, 0.1, 80.0, None, None) == -1
    assert lib.mudg_metric_depth(one, one, 1, 4097, 4096, 0.1, 80.0, one, None) == -1
    assert lib.mudg_metric_depth(one, one, 1, 8, 8, 2.0 ** -7, 80.0, one, None) == -1 and b"headroom" in lib.mudg_last_error()
    assert lib.mudg_metric_depth(one, one, 1, 8, 8, 0.1, 256.5, one, None) == -1
    assert lib.mudg_metric_depth(one, one, 1, 8, 8, 80.0, 0.1, one, None) == -1
    assert lib.mudg_metric_depth(one, one, 1, 8, 8, float("nan"), 80.0, one, None) == -1
    assert lib.mudg_metric_confusion(None, None, 1, 8, 8, 19, None, None, None) == -1
    assert lib.mudg_metric_confusion(one, one, 1, 8, 8, 33, one, one, None) == -1 and b"classes" in lib.mudg_last_error()
    assert lib.mudg_metric_confusion(one, one, 1, 8, 8, 0, one, one, None) == -1
    assert lib.mudg_metric_confusion(one, one, 1, 4097, 4096, 19, one, one, None) == -1


def test_metric_kernels_use_no_scratch_and_the_ssim_kernel_keeps_its_footprint(tmp_path):
    """Facts about the generated gfx950 code that do not depend on the compiler's scheduling, and the SSIM kernel's LDS bytes and VGPR
    count as DESIGN.md §15 records them (30944 bytes: five workgroups per CU; 104 VGPRs: four waves per SIMD)."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "metrics.s"
    subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S",
                    os.path.join(ROOT, "mudg_amd", "csrc", "metrics.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    s = out.read_text()
    md = s[s.index("amdhsa.kernels"):]
    families = ("metric_sse_kernel", "metric_ssim_kernel", "metric_depth_kernel", "metric_confusion_kernel")
    seen, ssim = {}, None
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", md, re.S):
        for family in families:
            if family in m.group(2):
                seen[family] = seen.get(family, 0) + 1
                assert int(m.group(3)) == 0 and int(m.group(5)) == 0, m.groups()
                if family == "metric_ssim_kernel":
                    ssim = (int(m.group(1)), int(m.group(4)))
    assert seen == {"metric_sse_kernel": 2, "metric_ssim_kernel": 1, "metric_depth_kernel": 2, "metric_confusion_kernel": 1}, seen
    print(f"metric_ssim_kernel: {ssim[0]} bytes of LDS, {ssim[1]} VGPRs")
    assert ssim[0] <= 32768 and 2 * ssim[0] <= 160 * 1024                            # at least two workgroups per CU (five fit)
    assert ssim[1] <= 128                                                            # 256 lanes: four waves per SIMD at up to 128 VGPRs
    assert "cmpswap" not in s                                                        # every atomic is a native integer add
    for name in sorted(set(re.findall(r"^(_Z\S*metric_\w+_kernel\S*):", s, re.M))):
        body = s[s.index(name + ":"):]
        lines = [l.strip() for l in body[:body.index(".end_amdhsa_kernel")].splitlines()]
        assert not any(l.startswith(("scratch_", "flat_")) for l in lines), name
        assert sum(l.startswith("global_atomic_add_x2") for l in lines) == {"sse": 1, "ssim": 1, "depth": 7, "confusion": 1}[re.search(r"metric_(\w+?)_kernel", name).group(1)], name
        assert not any(l.startswith("global_atomic") and not l.startswith("global_atomic_add_x2") for l in lines), name
