"""What the surface-normal rules can show without a GPU: the CPU definition (tests/normals_reference.py) against things
known without it — analytic planes, hand-made differences, tests/frames_reference.py's resize rule, a brute-force inverse cosine — and the
product's host side: the label draw, the cosine table, the C-ABI and the generated code of csrc/normals.hip."""
import os
import re

import numpy as np
import pytest
import torch

import frames_reference as fr
import normals_reference as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
ENTRIES = (("mudg_depth_normals", 13), ("mudg_normal_stream", 15), ("mudg_metric_normals", 9))
CAM = (20.0, 22.0, 8.3, 5.7)                                                 # fx, fy, cx, cy of a 12 x 16 frame


def _points(z, cam=CAM):
    """float64 points of a depth map by plain expressions (the test's own unprojection)."""
    fx, fy, cx, cy = cam
    H, W = z.shape
    xn = (np.arange(W)[None, :] + 0.5 - cx) / fx
    yn = (np.arange(H)[:, None] + 0.5 - cy) / fy
    return np.stack([xn * z, yn * z, z * np.ones_like(xn)], axis=-1)


def _plane_depth(a, b, c, d, hw=(12, 16), cam=CAM):
    fx, fy, cx, cy = cam
    xn = (np.arange(hw[1])[None, :] + 0.5 - cx) / fx
    yn = (np.arange(hw[0])[:, None] + 0.5 - cy) / fy
    return d / (a * xn + b * yn + c)


# ------------------------------------------------------------------------------------------------ normals from depth
def test_a_constant_depth_frame_is_exactly_the_wall_normal():
    """Exact, not 1e-15: with equal depths dx = (a, 0, 0) and dy = (0, b, 0) with exact zeros (x z - x z, z - z), so n = (0 - 0, 0 - 0,
    0 - b a), len = sqrt(fl(b a)^2) = |fl(b a)| (the square root of a correctly rounded square is exact) and n / len = (0, 0, -1)."""
    for depth in (7.25, 33.3):
        n, valid = nr.depth_normals(np.full((5, 7), depth, dtype=F), (9.0, 9.5, 3.4, 2.6))
        assert valid.all()                                                   # a border pixel has its one-sided differences
        assert np.array_equal(n, np.broadcast_to(F([0, 0, -1]), (5, 7, 3)))


def test_a_tilted_plane_gives_the_analytic_normal_within_the_rounding_of_the_stored_depth():
    """z solves a X + b Y + c Z = d at the pixel centres and is stored in fp32: every point moves along its ray by at most 2^-24 of its
    length, a difference of two points by at most e(|P+| + |P-|), the cross product by |ddy||dx| + |dy||ddx| + |ddy||ddx|, and a unit
    vector by at most twice the relative change of the vector it is made from.  Added: 2^-24 for the fp32 result and 1e-12 for float64
    arithmetic.  The bound is computed per pixel from the plane's exact points, not chosen."""
    worst = 0.0
    for a, b, c, d in ((0.3, -0.2, 1.0, 10.0), (-0.8, 0.5, 0.6, 6.0), (0.0, 1.2, 0.4, 3.0)):
        z = _plane_depth(a, b, c, d)
        assert z.min() > 0.5 and z.max() < 100
        n, valid = nr.depth_normals(z.astype(F), CAM)
        assert valid.all()
        want = -np.array([a, b, c]) / np.linalg.norm([a, b, c])              # d > 0: the side that faces the origin
        P = _points(z)
        H, W = z.shape
        e = 2.0 ** -24
        for j in range(H):
            for i in range(W):
                ip, im, jp, jm = min(i + 1, W - 1), max(i - 1, 0), min(j + 1, H - 1), max(j - 1, 0)
                dx, dy = P[j, ip] - P[j, im], P[jp, i] - P[jm, i]
                ddx = e * (np.linalg.norm(P[j, ip]) + np.linalg.norm(P[j, im]))
                ddy = e * (np.linalg.norm(P[jp, i]) + np.linalg.norm(P[jm, i]))
                ndx, ndy = np.linalg.norm(dx), np.linalg.norm(dy)
                bound = 2 * (ddy * ndx + ndy * ddx + ddy * ddx) / np.linalg.norm(np.cross(dy, dx)) + 2.0 ** -24 + 1e-12
                err = float(np.abs(n[j, i].astype(D) - want).max())
                assert err <= bound and bound < 1e-3, (a, b, c, j, i, err, bound)
                worst = max(worst, err / bound)
    print(f"tilted planes: the largest error is {worst:.3f} of its bound")
    assert worst > 0                                                         # fp32 depths against an exact plane: not a copy


def _hand_normal(dx, dy):
    n = np.array([dy[1] * dx[2] - dy[2] * dx[1], dy[2] * dx[0] - dy[0] * dx[2], dy[0] * dx[1] - dy[1] * dx[0]])
    return (n / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])).astype(F)


def test_one_sided_differences_at_the_border_and_beside_an_unusable_pixel():
    z = _plane_depth(0.3, -0.2, 1.0, 10.0).astype(F)
    z[5, 8] = np.nan                                                         # unusable: its four neighbours fall back to one side
    z[9, 3] = 0.0                                                            # the bounds are exclusive
    z[2, 12] = 100.0
    n, valid = nr.depth_normals(z, CAM)
    assert valid.sum() == z.size - 3 and not valid[5, 8] and not valid[9, 3] and not valid[2, 12]
    assert not n[5, 8].any() and not n[9, 3].any() and not n[2, 12].any()   # zeros, not NaN
    zd = z.astype(D)
    fx, fy, cx, cy = CAM
    P = np.stack([((np.arange(16)[None, :] + 0.5) - cx) / fx * zd, ((np.arange(12)[:, None] + 0.5) - cy) / fy * zd, zd], axis=-1)
    cases = {(0, 0): ((0, 1), (0, 0), (1, 0), (0, 0)),                       # corner: both one-sided
             (11, 15): ((11, 15), (11, 14), (11, 15), (10, 15)),
             (4, 0): ((4, 1), (4, 0), (5, 0), (3, 0)),                       # left border: dx one-sided, dy central
             (5, 7): ((5, 7), (5, 6), (6, 7), (4, 7)),                       # beside the NaN: dx from the left side only
             (5, 9): ((5, 10), (5, 9), (6, 9), (4, 9)),
             (4, 8): ((4, 9), (4, 7), (4, 8), (3, 8)),                       # above it: dy from the upper side only
             (6, 8): ((6, 9), (6, 7), (7, 8), (6, 8)),
             (6, 6): ((6, 7), (6, 5), (7, 6), (5, 6))}                       # interior: central both ways
    for (j, i), (xp, xm, yp, ym) in cases.items():
        assert np.array_equal(n[j, i], _hand_normal(P[xp] - P[xm], P[yp] - P[ym])), (j, i)


def test_a_pixel_without_a_horizontal_or_a_vertical_neighbour_is_not_valid():
    z = np.full((5, 6), 4.0, dtype=F)
    z[2, 1] = z[2, 3] = 0.0                                                  # (2, 2) has no horizontal neighbour
    z[1, 5] = z[3, 5] = np.inf                                               # (2, 5) has no vertical one
    n, valid = nr.depth_normals(z, (5.0, 5.0, 3.0, 2.5))
    want = np.ones((5, 6), np.uint8)
    for j, i in ((2, 1), (2, 3), (1, 5), (3, 5), (2, 2), (2, 5), (2, 0), (0, 5), (4, 5)):   # the last three: the frame's edge on one
        want[j, i] = 0                                                                      # side, an unusable pixel on the other
    assert np.array_equal(valid, want) and not n[valid == 0].any()
    assert np.array_equal(n[2, 4], F([0, 0, -1])) and np.array_equal(n[1, 1], F([0, 0, -1]))  # one side left: still the wall
    for hw in ((1, 1), (1, 5), (5, 1)):                                      # a row or a column has no second direction
        n, valid = nr.depth_normals(np.full(hw, 4.0, dtype=F), (5.0, 5.0, 0.5, 0.5))
        assert n.shape == hw + (3,) and not valid.any() and not n.any()


def test_sky_pixels_with_and_without_labels():
    z = np.full((5, 6), 30.0, dtype=F)
    labels = np.zeros((5, 6), np.int64)
    labels[2, 2] = labels[2, 3] = 10
    n, valid = nr.depth_normals(z, (5.0, 5.0, 3.0, 2.0), labels)
    assert valid.sum() == 28 and not valid[2, 2] and not valid[2, 3] and np.array_equal(n[2, 1], F([0, 0, -1]))
    assert nr.depth_normals(z, (5.0, 5.0, 3.0, 2.0))[1].all()                # no labels: no sky rule
    assert nr.depth_normals(z, (5.0, 5.0, 3.0, 2.0), labels, sky_label=11)[1].all()
    sky_row = np.zeros((5, 6), np.int64)
    sky_row[0] = sky_row[2] = 10
    assert not nr.depth_normals(z, (5.0, 5.0, 3.0, 2.0), sky_row)[1][1].any()   # row 1 between two sky rows: no dy


def test_the_step_limit_takes_the_side_that_lies_on_the_surface():
    z = np.full((5, 8), 5.0, dtype=F)
    z[:, 4:] = 20.0                                                          # two walls, a step between columns 3 and 4
    cam = (6.0, 6.0, 4.2, 2.4)
    free, valid = nr.depth_normals(z, cam)
    assert valid.all() and abs(float(free[2, 3, 0])) > 0.5 and abs(float(free[2, 4, 0])) > 0.5   # across the step: tilted
    assert np.array_equal(free[2, 1], F([0, 0, -1])) and np.array_equal(free[2, 6], F([0, 0, -1]))
    held, valid = nr.depth_normals(z, cam, max_rel_step=0.1)
    assert valid.all() and np.array_equal(held, np.broadcast_to(F([0, 0, -1]), (5, 8, 3)))
    lone = z.copy()
    lone[2, 2] = 50.0                                                        # nothing within the limit on any side
    assert not nr.depth_normals(lone, cam, max_rel_step=0.1)[1][2, 2]


def test_every_valid_normal_of_a_smooth_surface_faces_the_camera():
    j, i = np.mgrid[0:40, 0:56]
    z = (12.0 + 3.0 * np.sin(0.31 * i + 0.4) * np.cos(0.23 * j) + 0.05 * i - 0.04 * j).astype(F)
    z[::9, ::11] = 0.0
    cam = (60.0, 58.0, 27.1, 20.6)
    n, valid = nr.depth_normals(z, cam)
    assert valid.sum() > 0.9 * z.size
    P = _points(z.astype(D), cam)
    dots = (n.astype(D) * P).sum(-1)
    assert np.all(dots[valid == 1] < 0)
    lengths = np.sqrt((n.astype(D) ** 2).sum(-1))[valid == 1]
    assert np.abs(lengths - 1).max() < 2e-7                                  # unit, up to the fp32 rounding of three components


# ------------------------------------------------------------------------------------------------ the normal stream
def _unit_field(rng, shape):
    v = rng.normal(size=shape + (3,))
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


@pytest.mark.parametrize("hw_in,hw_out", [((7, 9), (3, 5)), ((5, 6), (11, 13)), ((37, 53), (16, 29)), ((6, 10), (6, 10))])
def test_the_stream_rule_is_the_fp32_resize_rule_on_every_channel(hw_in, hw_out):
    src = _unit_field(np.random.default_rng(hw_in[0]), (2,) + hw_in)
    got = nr.normal_stream(src, hw_out)
    assert got.dtype == F and got.shape == (3, 2) + hw_out
    for c in range(3):
        assert np.array_equal(got[c].view(np.uint32), fr.resize_f32_linear(np.ascontiguousarray(src[..., c]), hw_out).view(np.uint32)), c
    if hw_in == hw_out:
        assert np.array_equal(got, src.transpose(3, 0, 1, 2))                # weights 1 and 0: the input itself
    else:
        assert not np.allclose(np.sqrt((got.astype(D) ** 2).sum(0)), 1.0, atol=1e-3)   # no renormalisation: blends are shorter


def test_a_constant_field_stays_constant_and_a_nan_stays_one():
    """Exactly where the weights are dyadic (8 -> 4: 1/2, 1/2; 6 -> 12: 1/4, 3/4 and the clamped ends) and the values short enough for
    every product to be exact; for any weights v (1 - f) + v f is v up to the rounding of 1 - f, two products and a sum per pass: six
    roundings of 2^-24 at the most."""
    value = F([0.625, -0.75, 0.125])
    src = np.broadcast_to(value, (1, 8, 6, 3)).copy()
    got = nr.normal_stream(src, (4, 12))
    assert np.array_equal(got, np.broadcast_to(value[:, None, None, None], (3, 1, 4, 12)))
    value = F([0.6, -0.8, 0.123])
    src = np.broadcast_to(value, (1, 7, 9, 3)).copy()
    got = nr.normal_stream(src, (12, 5)).astype(D)
    assert np.all(np.abs(got - value.astype(D)[:, None, None, None]) <= 6 * 2.0 ** -24 * np.abs(value.astype(D))[:, None, None, None])
    src[0, 3, 4, 1] = np.nan
    got = nr.normal_stream(src, (7, 9))
    where = {tuple(int(v) for v in at) for at in np.argwhere(np.isnan(got))}
    assert where == {(1, 0, 3, 4), (1, 0, 3, 3), (1, 0, 2, 4), (1, 0, 2, 3)}    # its own channel; a second tap of weight 0 is still a tap


# ------------------------------------------------------------------------------------------------ the histogram of angular errors
def _drawn_off_the_edges():
    """Predictions and truths none of whose angles lies within 1e-6 degrees of a bin edge: redrawn with fixed seeds until that holds."""
    for seed in range(100, 120):
        rng = np.random.default_rng(seed)
        pred = rng.integers(0, 256, size=(60, 80, 3), dtype=np.uint8)
        gt = (rng.normal(size=(60, 80, 3)) * rng.uniform(0.2, 3.0, size=(60, 80, 1))).astype(F)
        gt[:20] = ((2.0 * pred[:20] - 255) / 255 + rng.normal(scale=0.08, size=(20, 80, 3))).astype(F)        # a third of them close
        p = 2.0 * pred.astype(D) - 255
        g = gt.astype(D)
        cos = (p * g).sum(-1) / (np.linalg.norm(p, axis=-1) * np.linalg.norm(g, axis=-1))
        angle = np.degrees(np.arccos(np.clip(cos, -1, 1)))
        steps = angle / 0.25
        if np.abs(steps - np.rint(steps)).min() * 0.25 > 1e-6:
            return pred, gt, angle
    raise AssertionError("no draw kept clear of the bin edges")


def test_the_histogram_equals_a_brute_force_inverse_cosine():
    pred, gt, angle = _drawn_off_the_edges()
    want_bins = np.floor(angle / 0.25).astype(np.int64)
    assert want_bins.min() >= 0 and want_bins.max() <= 719 and (want_bins < 40).sum() > 500
    c, gg = nr.cosines(pred, gt)
    got_bins = nr.bins_of(np.clip(c, -1, 1))
    assert np.array_equal(got_bins, want_bins)                               # every pixel: zero exceptions
    hist = nr.normal_hist(pred, gt)
    assert hist.dtype == np.int64 and hist.shape == (720,) and np.array_equal(hist, np.bincount(want_bins.reshape(-1), minlength=720))
    s = nr.scores(hist)
    n = angle.size
    assert s["n"] == n
    assert s["a11"] == (angle < 11.25).sum() / n and s["a22"] == (angle < 22.5).sum() / n and s["a30"] == (angle < 30.0).sum() / n
    assert 0 < s["a11"] < s["a22"] < s["a30"] < 1
    assert abs(s["mean"] - angle.mean()) <= 0.125                            # bin centres: half a bin at the most
    assert abs(s["median"] - np.sort(angle.reshape(-1))[(n - 1) // 2]) <= 0.125    # the lower median's bin
    mirrored = nr.normal_hist(255 - pred, gt)                                # 2 (255 - u) - 255 = -(2 u - 255)
    assert np.array_equal(mirrored, hist[::-1])
    valid = (np.arange(60 * 80).reshape(60, 80) % 3 != 0).astype(np.uint8)
    assert np.array_equal(nr.normal_hist(pred, gt, valid), np.bincount(want_bins[valid == 1], minlength=720))


def test_the_ends_and_the_edges_of_the_bins():
    T = nr.cos_table()
    assert T.dtype == D and T.shape == (721,) and T[0] == 1.0 and T[720] == -1.0 and np.all(np.diff(T) < 0)
    up, down = np.nextafter(T[5], 2.0), np.nextafter(T[5], -2.0)
    assert nr.bins_of(np.array([1.0, -1.0, T[5], up, down, T[719], T[1]])).tolist() == [0, 719, 5, 4, 5, 719, 1]
    white, grey = np.array([[255, 255, 255]], np.uint8), np.array([[128, 128, 128]], np.uint8)
    ones = np.array([[1, 1, 1]], F)
    assert nr.cosines(white, ones)[0][0] == 1.0 and nr.cosines(white, -ones)[0][0] == -1.0      # sqrt(195075 * 3) = 765 exactly
    assert nr.normal_hist(white, ones)[0] == 1 and nr.normal_hist(white, -ones)[719] == 1 and nr.normal_hist(grey, ones)[0] == 1
    bad = np.array([[0, 0, 0], [np.inf, 0, 0], [np.nan, 1, 0], [3e38, 3e38, 3e38]], F)         # the last: gg is finite in float64
    assert nr.normal_hist(np.repeat(white, 4, axis=0), bad).tolist() == [1] + [0] * 719
    empty = nr.scores(np.zeros(720, np.int64))
    assert empty["n"] == 0 and all(np.isnan(empty[k]) for k in ("mean", "median", "a11", "a22", "a30"))
    one = np.zeros(720, np.int64)
    one[44], one[45] = 3, 1
    s = nr.scores(one)
    assert s["a11"] == 0.75 and s["a22"] == 1.0 and s["median"] == 11.125 and s["mean"] == (3 * 11.125 + 11.375) / 4


# ------------------------------------------------------------------------------------------------ the product's host side
def test_the_label_draw_with_the_normal_triple():
    from mudg_amd import frames, hip
    three = ("color", "semantic", "normal")
    below_one = float(np.nextafter(1.0, 0.0))
    for choose in (frames.choose_label, nr.choose_label):
        assert [choose(three, u) for u in (0.0, 0.2499, 0.25, 0.4999, 0.5, below_one)] == ["normal", "normal", "semantic", "semantic", "color", "color"]
        assert choose(("normal", "color", "semantic"), 0.1) == "normal" and choose(("color", "semantic", "depth"), 0.1) == "depth"
        assert choose(("normal",), 0.9) == "normal" and [choose(("color", "normal"), u) for u in (0.5, 0.51)] == ["normal", "color"]
    with pytest.raises(hip.MudgError, match="4 labels"):
        frames.choose_label(("color", "semantic", "normal", "depth"), 0.1)
    assert frames.MODALITY_LABEL == {"color": 0, "semantic": 1, "depth": 500, "normal": 1000}
    assert callable(frames.stream_from_normals) and frames._STREAM["normal"] is frames.stream_from_normals


def test_the_products_cosine_table_is_the_definitions():
    from mudg_amd import ops
    assert ops.NORMAL_BINS == nr.BINS and np.array_equal(ops.normal_cos_table(), nr.cos_table())


def test_inputs_off_the_gpu_raise():
    from mudg_amd import depth, frames, hip, metrics, ops
    z, n, u = torch.zeros(2, 8, 8), torch.zeros(2, 8, 8, 3), torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        depth.normals_from_depth(z, np.eye(3), (8, 8))
    with pytest.raises(hip.MudgError, match="on the GPU"):
        metrics.normal_errors(u, n)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        frames.stream_from_normals(n, (4, 4))
    with pytest.raises(hip.MudgError, match="on the GPU"):
        ops.metric_normals(u, n)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        frames.SceneFrames(u, normals=n)


def test_the_product_does_not_import_the_cpu_definition():
    for d in ("mudg_amd", "lvdm", "utils", "virtual_render", "tools"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith(".py"):
                    assert "normals_reference" not in open(os.path.join(base, f)).read(), f


# ------------------------------------------------------------------------------------------------ C-ABI and generated code
def test_normal_entry_points_are_declared_bound_and_exported():
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
    assert "normals.hip" in build.SOURCES
    assert len(hip.SIGNATURES["mudg_dense_stream"][1]) == 18 and len(hip.SIGNATURES["mudg_resize_f32"][1]) == 10   # untouched


def test_the_entry_points_reject_bad_arguments_without_touching_the_gpu():
    from mudg_amd import hip
    lib = hip.lib()
    table = np.zeros((4, 4), dtype=np.int32)
    p = table.ctypes.data                                                            # never read: every call fails its checks first
    assert lib.mudg_depth_normals(None, None, 10, None, 1, 1, 1, 0.0, 100.0, -1.0, None, None, None) == -1 and b"null" in lib.mudg_last_error()
    assert lib.mudg_depth_normals(p, None, 10, p, 0, 8, 8, 0.0, 100.0, -1.0, p, p, None) == -1 and b"frames" in lib.mudg_last_error()
    assert lib.mudg_depth_normals(p, None, 10, p, 65536, 8, 8, 0.0, 100.0, -1.0, p, p, None) == -1 and b"65535" in lib.mudg_last_error()
    assert lib.mudg_depth_normals(p, None, 10, p, 1, 4097, 4096, 0.0, 100.0, -1.0, p, p, None) == -1 and b"2^24" in lib.mudg_last_error()
    assert lib.mudg_depth_normals(p, None, 10, p, 1, 8, 8, 5.0, 5.0, -1.0, p, p, None) == -1 and b"range" in lib.mudg_last_error()
    assert lib.mudg_depth_normals(p, None, 10, p, 1, 8, 8, 0.0, 100.0, float("nan"), p, p, None) == -1 and b"step" in lib.mudg_last_error()
    assert lib.mudg_normal_stream(None, 1, 2, 2, 2, 2, None, None, None, 0, 4, 4, 0, 0, None) == -1 and b"null" in lib.mudg_last_error()
    assert lib.mudg_normal_stream(p, 0, 2, 2, 2, 2, p, p, p, 0, 4, 4, 0, 0, None) == -1 and b"frames" in lib.mudg_last_error()
    assert lib.mudg_normal_stream(p, 1, 2, 2, 2, 2, p, p, p, 0, 4, 3, 0, 0, None) == -1 and b"strides" in lib.mudg_last_error()
    assert lib.mudg_normal_stream(p, 1, 20000, 20000, 2, 2, p, p, p, 0, 4, 4, 0, 0, None) == -1 and b"2^28" in lib.mudg_last_error()
    assert lib.mudg_metric_normals(None, None, None, None, 1, 1, 1, None, None) == -1 and b"null" in lib.mudg_last_error()
    assert lib.mudg_metric_normals(p, p, None, p, 0, 8, 8, p, None) == -1 and b"frames" in lib.mudg_last_error()
    assert lib.mudg_metric_normals(p, p, None, p, 1, 4097, 4096, p, None) == -1 and b"2^24" in lib.mudg_last_error()
    assert lib.mudg_dense_stream(3, p, 1, 2, 2, 2, 2, p, p, p, p, 0, 4, 4, 0, 0, None, None) == -1 and b"kind" in lib.mudg_last_error()   # no fourth kind


def test_normal_kernels_use_no_scratch_and_only_integer_atomics(tmp_path):
    """Facts about the generated gfx950 code that do not depend on the compiler's scheduling."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "normals.s"
    subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S",
                    os.path.join(ROOT, "mudg_amd", "csrc", "normals.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    s = out.read_text()
    md = s[s.index("amdhsa.kernels"):]
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", md, re.S):
        for family in ("depth_normals_kernel", "normal_stream_kernel", "metric_normals_kernel"):
            if family in m.group(1):
                seen[family] = seen.get(family, 0) + 1
                assert int(m.group(2)) == 0, m.groups()
    assert seen == {"depth_normals_kernel": 2, "normal_stream_kernel": 2, "metric_normals_kernel": 2}, seen
    assert "cmpswap" not in s and not re.search(r"atomic\w*_f(16|32|64)", s)
    for name in sorted(set(re.findall(r"^(_Z\S*metric_normals_kernel\S*):", s, re.M))):
        body = s[s.index(name + ":"):]
        lines = [l.strip() for l in body[:body.index(".end_amdhsa_kernel")].splitlines()]
        assert sum(l.startswith("global_atomic_add_x2") for l in lines) >= 1 and any(l.startswith("ds_add_u32") for l in lines), name
        assert not any(l.startswith(("scratch_", "flat_")) for l in lines), name
    for name in sorted(set(re.findall(r"^(_Z\S*(?:depth_normals_kernelILi4E|normal_stream_kernelILb1E)\S*):", s, re.M))):   # the wide forms
        body = s[s.index(name + ":"):]
        lines = [l.strip() for l in body[:body.index(".end_amdhsa_kernel")].splitlines()]
        assert any(l.startswith("global_store_dwordx4") for l in lines), name
        assert not any(l.startswith(("scratch_", "flat_")) for l in lines), name
