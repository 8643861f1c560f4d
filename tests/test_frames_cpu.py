"""The frame-resize rules held to things known without them: tests/frames_reference.py, the definition the GPU tests
compare with bit for bit, against identities, fp64 bilinear interpolation, direct indexing and torch's own expressions; and the host
side of the product (the tables of mudg_amd/ops.py, the label choice of mudg_amd/frames.py) against the definition."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frames_reference as fr

SIZES = [((7, 9), (3, 5)), ((5, 6), (11, 13)), ((8, 12), (4, 6)), ((6, 10), (6, 10)), ((1, 1), (3, 2)), ((2, 3), (1, 1)),
         ((37, 53), (16, 29)), ((9, 130), (5, 67)), ((20, 600), (9, 320)), ((1280, 1920), (576, 1024))]
IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SIZES]


def _u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _f32(shape, seed):
    return np.random.default_rng(seed).uniform(-10.0, 110.0, size=shape).astype(np.float32)


@pytest.mark.parametrize("hw", [(1, 1), (6, 10), (37, 53)])
def test_equal_sizes_return_the_input_exactly(hw):
    img, dep = _u8((2,) + hw + (3,), 1), _f32((2,) + hw, 2)
    assert np.array_equal(fr.resize_u8_linear(img, hw), img)
    assert np.array_equal(fr.resize_u8_nearest(img, hw), img)
    assert np.array_equal(fr.resize_f32_linear(dep, hw), dep)


@pytest.mark.parametrize("hw_in,hw_out", SIZES, ids=IDS)
def test_a_constant_image_stays_constant_and_coefficient_pairs_sum_to_2048(hw_in, hw_out):
    for n_src, n_dst in zip(hw_in, hw_out):
        s0, s1, f = fr.linear_coords(n_src, n_dst)
        c0, c1 = fr.coefficients(f)
        assert c0.dtype == np.int16 and np.all(c0.astype(np.int32) + c1 == 2048) and c0.min() >= 0 and c1.min() >= 0
        assert s0.min() >= 0 and s1.max() <= n_src - 1 and np.all((s1 == s0 + 1) | (s1 == n_src - 1))
        assert np.all((f >= 0) & (f < 1))
    for value in (0, 1, 127, 254, 255):
        img = np.full((1,) + hw_in + (3,), value, dtype=np.uint8)
        assert np.all(fr.resize_u8_linear(img, hw_out) == value)
    assert np.all(fr.resize_f32_linear(np.full((1,) + hw_in, 37.25, dtype=np.float32), hw_out) == np.float32(37.25))


@pytest.mark.parametrize("hw_in,hw_out", SIZES, ids=IDS)
def test_the_8_bit_rule_is_within_one_grey_level_of_fp64_bilinear_at_the_same_coordinates(hw_in, hw_out):
    img = _u8((1,) + hw_in + (3,), 3)
    y0, y1, fy = fr.linear_coords(hw_in[0], hw_out[0])
    x0, x1, fx = fr.linear_coords(hw_in[1], hw_out[1])
    s = img.astype(np.float64)
    fx, fy = fx.astype(np.float64)[None, None, :, None], fy.astype(np.float64)[None, :, None, None]
    rows = s[:, :, x0] * (1 - fx) + s[:, :, x1] * fx
    want = rows[:, y0] * (1 - fy) + rows[:, y1] * fy
    err = float(np.abs(fr.resize_u8_linear(img, hw_out).astype(np.float64) - want).max())
    print(f"8-bit rule vs fp64 bilinear {hw_in} -> {hw_out}: max |error| {err:.4f} grey levels (bound: strictly below 1)")
    assert err < 1.0


@pytest.mark.parametrize("hw_in,hw_out", SIZES, ids=IDS)
def test_the_fp32_rule_against_interpolate_in_float64(hw_in, hw_out):
    """The rule rounds its coordinates to fp32: a coordinate is off by at most half an fp32 ulp of itself, which moves the value by at most
    that times the input's range, per axis; the four products and three sums add at most 4 x 2^-24 max |v|."""
    dep = _f32((1,) + hw_in, 4)
    want = F.interpolate(torch.from_numpy(dep).double()[None], size=hw_out, mode="bilinear", align_corners=False)[0].numpy()
    half_ulp = lambda n: 0.5 * float(np.spacing(np.float32(max(n - 1, 1))))
    bound = float(dep.max() - dep.min()) * (half_ulp(hw_in[1]) + half_ulp(hw_in[0])) + 4 * 2.0 ** -24 * float(np.abs(dep).max())
    err = float(np.abs(fr.resize_f32_linear(dep, hw_out).astype(np.float64) - want).max())
    print(f"fp32 rule vs fp64 interpolate {hw_in} -> {hw_out}: max |error| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


@pytest.mark.parametrize("hw_in,hw_out", SIZES[:-1], ids=IDS[:-1])
def test_nearest_against_direct_indexing(hw_in, hw_out):
    img = _u8((2,) + hw_in + (3,), 5)
    got = fr.resize_u8_nearest(img, hw_out)
    for y in range(hw_out[0]):
        for x in range(hw_out[1]):
            sy, sx = min(y * hw_in[0] // hw_out[0], hw_in[0] - 1), min(x * hw_in[1] // hw_out[1], hw_in[1] - 1)      # exact integer floor
            assert np.array_equal(got[:, y, x], img[:, sy, sx]), (y, x)


def test_the_normalisation_table_is_torchs_expression():
    from mudg_amd import ops
    v = torch.arange(256, dtype=torch.uint8)
    want = (v.float() / 255 - 0.5) * 2
    assert torch.equal(ops.norm_table(torch.device("cpu")), want)
    frames = v.reshape(1, 16, 16, 1).repeat(1, 1, 1, 3).numpy()
    assert torch.equal(torch.from_numpy(fr.norm_u8(frames)), want.reshape(1, 1, 16, 16).repeat(3, 1, 1, 1))
    depth = np.array([[[-3.0, 0.0, 1e-3, 49.99, 50.0, 99.5, 100.0, 250.0]]], dtype=np.float32)
    want = (torch.clamp(torch.from_numpy(depth), 0, 100) / 100.0 - 0.5) * 2
    assert torch.equal(torch.from_numpy(fr.depth_stream(depth, (1, 8)))[0], want)


def test_the_palette_is_the_nineteen_known_colours_and_two_more():
    assert fr.PALETTE.shape == (21, 3)
    ids = np.array([[[0, 18, 19, 20, 21, 255]]], dtype=np.uint8)
    rgb = fr.colourise(ids)
    assert rgb.shape == (1, 1, 6, 3) and np.array_equal(rgb[0, 0, :4], fr.PALETTE[[0, 18, 19, 20]]) and not rgb[0, 0, 4:].any()


@pytest.mark.parametrize("hw_in,hw_out", SIZES, ids=IDS)
def test_the_products_tables_are_the_definitions_coordinates(hw_in, hw_out):
    from mudg_amd import ops
    for n_src, n_dst in zip(hw_in, hw_out):
        s0, s1, f = fr.linear_coords(n_src, n_dst)
        c0, c1 = fr.coefficients(f)
        t = ops.resize_table(n_src, n_dst, "linear_u8")
        assert t.dtype == np.int32 and t.shape == (n_dst, 4)
        assert np.array_equal(t, np.stack([s0, s1, c0, c1], axis=1))
        t = ops.resize_table(n_src, n_dst, "linear_f32")
        assert np.array_equal(t[:, :2], np.stack([s0, s1], axis=1))
        assert np.array_equal(t[:, 2].view(np.float32), np.float32(1) - f) and np.array_equal(t[:, 3].view(np.float32), f)
        t = ops.resize_table(n_src, n_dst, "nearest")
        assert np.array_equal(t[:, 0], fr.nearest_coords(n_src, n_dst)) and np.array_equal(t[:, 0], t[:, 1])


def test_label_choice_intervals():
    from mudg_amd import frames
    three = ("color", "semantic", "depth")
    below_one = float(np.nextafter(1.0, 0.0))
    for choose in (frames.choose_label, fr.choose_label):
        assert [choose(three, u) for u in (0.0, 0.2499, 0.25, 0.4999, 0.5, below_one)] == ["depth", "depth", "semantic", "semantic", "color", "color"]
        assert choose(("depth",), 0.9) == "depth"
        assert [choose(("color", "depth"), u) for u in (0.0, 0.5, 0.51, below_one)] == ["depth", "depth", "color", "color"]
    assert frames.CAPTION == "A photo a of driving scene." and frames.FPS == 10
    assert frames.CLASS_LABEL == {"color": 0, "semantic": 1, "depth": 500}


def test_the_abi_has_the_frame_entry_points():
    from mudg_amd import hip
    assert {"mudg_resize_u8", "mudg_resize_f32", "mudg_dense_stream"} <= set(hip.SIGNATURES)
    assert len(hip.SIGNATURES["mudg_dense_stream"][1]) == 18


def test_the_entry_points_reject_bad_arguments_without_touching_the_gpu():
    from mudg_amd import hip
    lib = hip.lib()
    table = np.zeros((4, 4), dtype=np.int32)
    p = table.ctypes.data                                                     # never read: every call fails its checks first
    assert lib.mudg_resize_u8(None, None, 1, 2, 2, 3, 2, 2, 0, 0, None, None, None) == -1 and b"null" in lib.mudg_last_error()
    assert lib.mudg_resize_u8(p, p, 1, 2, 2, 2, 2, 2, 0, 0, p, p, None) == -1 and b"channels" in lib.mudg_last_error()
    assert lib.mudg_resize_u8(p, p, 1, 2, 2, 3, 2, 2, 1, 1, p, p, None) == -1 and b"palette" in lib.mudg_last_error()
    assert lib.mudg_resize_f32(p, p, 0, 2, 2, 2, 2, p, p, None) == -1 and b"frames" in lib.mudg_last_error()
    assert lib.mudg_dense_stream(3, p, 1, 2, 2, 2, 2, p, p, p, p, 0, 4, 4, 0, 0, None, None) == -1 and b"kind" in lib.mudg_last_error()
    assert lib.mudg_dense_stream(0, p, 1, 2, 2, 2, 2, p, p, p, p, 0, 4, 3, 0, 0, None, None) == -1 and b"strides" in lib.mudg_last_error()
    assert lib.mudg_dense_stream(2, p, 1, 2, 2, 2, 2, p, p, None, p, 0, 4, 4, 0, 0, p, None) == -1 and b"uint8" in lib.mudg_last_error()
