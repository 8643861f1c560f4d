"""What the metric-depth and view-lifting rules can show without a GPU: the CPU definition (tests/depth_reference.py)
against the REFERENCE's colormap, visualize_depth, align_depth and process_sky (tests/golden/depth_post.pt, made by
tests/golden/make_golden_depth.py), its sums against a brute-force loop, a lifted view re-projected through the splat's own CPU definition
(tests/splat_reference.py), and the C-ABI and generated code of csrc/depth.hip."""
import os
import re

import numpy as np
import pytest
import torch

import depth_reference as dr
import splat_reference as sr
from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
ENTRIES = (("mudg_depth_align_sums", 7), ("mudg_depth_align_solve", 5), ("mudg_depth_finish", 10), ("mudg_colormap_spectral", 8),
           ("mudg_depth_unproject", 13))


# ------------------------------------------------------------------------------------------------ against the reference's functions
def test_the_colour_map_definition_equals_the_reference_bytes_and_floats_exactly():
    g = golden("depth_post.pt")
    x = g["cm_in"].numpy()
    flat = x.reshape(-1)
    tenths = np.arange(11, dtype=F) / F(10)
    for j in range(11):                                                      # the fixture holds what it is meant to hold
        assert tenths[j] in flat and np.nextafter(tenths[j], F(-1)) in flat and np.nextafter(tenths[j], F(2)) in flat, j
    assert flat.min() < 0 and flat.max() > 1 and 0.0 in flat and 1.0 in flat
    for reverse, tag in ((False, "cm"), (True, "cm_r")):
        got_b, got_f = dr.colormap(x, reversed=reverse), dr.colormap(x, reversed=reverse, bytes=False)
        want_b, want_f = g[tag + "_bytes"].numpy(), g[tag + "_floats"].numpy()
        assert got_b.dtype == np.uint8 and got_b.shape == want_b.shape and np.array_equal(got_b, want_b), tag
        assert got_f.dtype == F and np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32)), tag       # the floats, bit for bit
    assert np.array_equal(dr.colormap(x), g["vd_default"].numpy())                                           # visualize_depth, default range
    lo, hi = (float(v) for v in g["vd_range"])
    assert (lo, hi) == (2.0, 50.0)
    assert np.array_equal(dr.colormap(g["vd_in"].numpy(), lo, hi), g["vd_bytes"].numpy())
    assert not np.array_equal(dr.colormap(g["vd_in"].numpy()), g["vd_bytes"].numpy())                        # the range is used


def test_the_sky_rule_equals_the_reference_expressions():
    g = golden("depth_post.pt")
    semantic = g["sky_semantic"].numpy()
    assert (semantic == 10).sum() >= 60 and g["sky_in"].min() < 0 and g["sky_in"].max() > 100
    got = dr.sky_clip(g["sky_in"].numpy(), semantic, 10).astype(F)
    assert np.array_equal(got, g["sky_out"].numpy())
    assert np.all(got[semantic == 10] == 100) and got.min() == 0 and got.max() == 100
    assert np.array_equal(dr.to_bytes(dr.spectral(got / F(100))), g["sky_vis"].numpy())
    # the same two steps inside finish: a white frame under m = 250, c = -50 is 200 m before the clip, a black one -50 m
    frame = np.zeros((4, 4, 3), np.uint8)
    frame[:2] = 255
    labels = np.zeros((4, 4), np.int64)
    labels[3, 3] = 10
    depth, vis = dr.finish(frame, 250.0, -50.0, labels)
    assert np.all(depth[:2] == 100) and np.all(depth[2:].reshape(-1)[:-1] == 0) and depth[3, 3] == 100
    assert np.array_equal(vis[0, 0], dr.to_bytes(dr.SPECTRAL[10])) and np.array_equal(vis[2, 0], dr.to_bytes(dr.SPECTRAL[0]))


def test_the_alignment_definition_is_within_its_bound_of_align_depth():
    """align_depth fits float64 least squares to fp32 u = mean(r, g, b) / 255 and the fp32 LiDAR depth; the definition fits integer sums
    of k = r + g + b and of the LiDAR depth on a 2^-20 m grid, and rounds its result to fp32.  Per pixel the two differ by at most
        (2^-21 + |m| 2^-24) (1 + L) + 2^-18  metres (+ 1e-9 for float64 arithmetic),  L = max |u - mean u| / std u over the counted pixels:
    the LiDAR grid (half a step) and the rounding of u to fp32, each of which moves the fitted line by at most (1 + L) times itself at a
    counted pixel's u, and the rounding of a result below 128 m to fp32.  DESIGN.md §14 derives it.  The bound is computed from the
    fixture, not chosen in advance."""
    g = golden("depth_post.pt")
    frames, lidar, want = g["align_frames"].numpy(), g["align_lidar"].numpy(), g["aligned"].numpy()
    assert want.dtype == D and 0.10 < (lidar == 0).mean() < 0.20 and (dr.k_of(frames) == 0).sum() == 4
    worst = 0.0
    for i in range(2):
        k = dr.k_of(frames[i])
        use = dr.counted(k, lidar[i])
        assert np.array_equal(use, (lidar[i] > 0) & (g["align_u"].numpy()[i, 0] > 0))                       # align_depth's own mask
        u = k[use].astype(D) / 765.0
        L = float(np.abs(u - u.mean()).max() / u.std())
        assert L <= 4, L
        m, c, fitted = dr.align_solve(dr.align_sums(frames[i], lidar[i]))
        assert fitted == 1 and 70 < m < 90 and 0 < c < 4                                                    # the fixture's line is 80 u + 2
        depth, _ = dr.finish(frames[i], m, c)
        bound = (2.0 ** -21 + abs(m) * 2.0 ** -24) * (1 + L) + 2.0 ** -18 + 1e-9
        diff = float(np.abs(depth.astype(D) - np.clip(want[i], 0, 100)).max())
        print(f"frame {i}: m = {m:.9f}, c = {c:.9f}, L = {L:.4f}, bound = {bound:.3e} m, max |definition - align_depth| = {diff:.3e} m")
        assert diff <= bound, (i, diff, bound)
        worst = max(worst, diff)
    assert worst > 0                                                                                         # fp32 against float64: not a copy


def test_the_sums_equal_a_brute_force_loop_in_python_integers():
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)
    frame[0, 0] = 0
    lidar = rng.uniform(0, 120, (7, 9)).astype(F)
    lidar[1, :3] = 0
    lidar[2, 0], lidar[2, 1], lidar[2, 2], lidar[2, 3] = 256.0, 255.99, -1.0, np.nan
    lidar[3, 0], lidar[3, 1] = 2.0 ** -21, 3 * 2.0 ** -21                                                    # ties: half to even, 0 and 2
    n = sk = skk = sq = skq = 0
    for j in range(7):
        for i in range(9):
            k = int(frame[j, i, 0]) + int(frame[j, i, 1]) + int(frame[j, i, 2])
            y = float(lidar[j, i])
            if k > 0 and 0 < y < 256:
                scaled = y * 2 ** 20                                                                         # exact in a double
                q = int(np.floor(scaled))
                rest = scaled - q
                q += 1 if rest > 0.5 or (rest == 0.5 and q % 2 == 1) else 0
                n, sk, skk, sq, skq = n + 1, sk + k, skk + k * k, sq + q, skq + k * q
    assert dr.align_sums(frame, lidar) == (n, sk, skk, sq, skq) and n == 63 - 1 - 3 - 3
    assert [int(v) for v in dr.q_of(F([2.0 ** -21, 3 * 2.0 ** -21, 1.0, 255.99]))] == [0, 2, 2 ** 20, 16776561 << 4]        # fp32(255.99) = 16776561 * 2^-16
    # the largest frame the kernels take, every pixel at the top of both ranges: the sums stay below 2^63
    top = 2 ** 24 * 765 * int(dr.q_of(F([255.99]))[0])
    assert top < 2 ** 63 and 2 ** 24 * 765 * 765 < 2 ** 63


def test_frames_that_cannot_be_fitted_keep_the_streams_own_scale():
    assert dr.align_solve((0, 0, 0, 0, 0)) == (100.0, 0.0, 0)
    assert dr.align_solve((1, 300, 90000, 5 << 20, 1500 << 20)) == (100.0, 0.0, 0)                          # one pixel
    assert dr.align_solve((4, 1200, 360000, 20 << 20, 6000 << 20)) == (100.0, 0.0, 0)                       # all k equal: den = 0
    m, c, fitted = dr.align_solve((2, 255 + 765, 255 * 255 + 765 * 765, 14 << 20, (255 * 4 + 765 * 10) << 20))  # (k = 255, 4 m) and (765, 10 m)
    assert fitted == 1 and abs(m - 9.0) < 1e-12 and abs(c - 1.0) < 1e-12                                     # 9 u + 1


# ------------------------------------------------------------------------------------------------ lifting, through the splat's definition
def test_a_lifted_view_reprojects_into_its_own_pixels_with_its_own_colours():
    """A 24 x 32 view, its camera 60 m from the origin and turned: every valid pixel's point, drawn again at the same pose with point
    size 1 by the splat's CPU definition, lands in the pixel it came from.  The splat works in fp32: with |coordinates| < 256 m (the
    camera within 100 m of the origin, depths below 100 m) a world coordinate carries at most 2^-17 m of rounding, the camera-space
    point a few times that (< 1e-4 m), and a pixel is fx * 1e-4 / z wide of its centre — below the half pixel that point size 1 allows
    for every depth above fx * 2e-4 m; the fixture keeps its depths above 0.5 m."""
    rng = np.random.default_rng(5)
    H, W = 24, 32
    a, b = 0.7, -0.2
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = rz @ rx, [40.0, -40.0, 20.0]
    assert np.linalg.norm(c2w[:3, 3]) == 60.0
    intr = np.array([[800.0, 0, 640.0], [0, 820.0, 480.0], [0, 0, 1]])
    cam = sr.scaled_camera(intr, (960, 1280), (H, W))
    table = np.concatenate([c2w[:3].reshape(12), cam.astype(D)])
    depth = rng.uniform(0.5, 99.0, (H, W)).astype(F)
    depth[0, :3] = [0.0, 100.0, 150.0]                                                                       # not valid: the bounds are exclusive
    labels = np.zeros((H, W), np.int64)
    labels[5, 5:9] = 10                                                                                      # sky: not lifted
    rgb = np.stack([np.arange(H)[:, None] + np.zeros(W, int), np.zeros(H, int)[:, None] + np.arange(W), np.full((H, W), 200)], axis=2).astype(np.uint8)
    packed, valid = dr.unproject(depth, rgb, table, labels)
    assert packed.dtype == np.int32 and packed.shape == (H * W, 4) and valid.sum() == H * W - 3 - 4
    assert not packed[valid == 0].any()
    xyz, word = packed[:, :3].copy().view(F), packed[:, 3]
    assert np.abs(xyz).max() < 256
    colours = np.stack([word & 255, (word >> 8) & 255, (word >> 16) & 255], axis=1).astype(np.uint8)
    mat = sr.host_matrix(c2w)
    for index in np.flatnonzero(valid):
        img, z = sr.splat(xyz[index:index + 1], colours[index:index + 1], mat, cam, 1.0, H, W)
        j, i = divmod(int(index), W)
        assert np.count_nonzero(z) == 1 and z[j, i] > 0, (j, i)
        assert tuple(img[j, i]) == (j, i, 200) and abs(float(z[j, i]) - float(depth[j, i])) < 1e-3, (j, i)
    # all at once: every valid pixel is drawn (no two points share a pixel) in its own colour
    keep = valid == 1
    img, z = sr.splat(xyz[keep], colours[keep], mat, cam, 1.0, H, W)
    assert np.array_equal(z.reshape(-1) > 0, keep) and np.array_equal(img.reshape(-1, 3)[keep], rgb.reshape(-1, 3)[keep])


def test_the_camera_table_is_the_pose_and_the_scaled_intrinsics():
    from mudg_amd import depth, render
    c2w = np.stack([np.eye(4), np.eye(4)])
    c2w[1, :3, 3] = [1.0, 2.0, 3.0]
    intr = np.array([[800.0, 0, 640.0], [0, 820.0, 480.0], [0, 0, 1]])
    table = depth.camera_table(intr, c2w, (960, 1280), (24, 32))
    assert table.dtype == D and table.shape == (2, 16)
    assert np.array_equal(table[1, :12].reshape(3, 4), c2w[1, :3]) and np.array_equal(table[0, 12:], render.scaled_intrinsics(intr, (960, 1280), (24, 32)))


# ------------------------------------------------------------------------------------------------ the interface off the GPU
def test_inputs_off_the_gpu_raise():
    from mudg_amd import depth, hip, ops, render
    frames, lidar = torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 8, 8)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        depth.metric_depth(frames, lidar)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        depth.lift_views(lidar, frames, np.eye(3), np.stack([np.eye(4)] * 2), (8, 8))
    with pytest.raises(hip.MudgError, match="on the GPU"):
        ops.depth_align_sums(frames, lidar)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        ops.colormap_spectral(torch.zeros(4))
    with pytest.raises(hip.MudgError, match="PointCloud"):
        render.PointCloud.concatenated()
    with pytest.raises(hip.MudgError, match="PointCloud"):
        render.PointCloud.concatenated(torch.zeros(4, 4, dtype=torch.int32))


def test_only_the_two_spectral_maps_exist():
    from virtual_render import eval_tools
    for call in (lambda: eval_tools.colormap(np.zeros((2, 2), F), cmap="viridis"), lambda: eval_tools.visualize_depth(np.zeros((2, 2), F), color_map="binary")):
        with pytest.raises(ValueError, match="'Spectral' and 'Spectral_r'"):
            call()
    with pytest.raises(ValueError, match="Invalid values range"):
        eval_tools.visualize_depth(np.zeros((2, 2), F), val_min=1.0, val_max=1.0)
    assert "matplotlib depth colour map" not in eval_tools.__doc__


def test_the_product_does_not_import_the_cpu_definition():
    for d in ("mudg_amd", "lvdm", "utils", "virtual_render", "tools"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith(".py"):
                    assert "depth_reference" not in open(os.path.join(base, f)).read(), f


# ------------------------------------------------------------------------------------------------ C-ABI and generated code
def test_depth_entry_points_are_declared_bound_and_exported():
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
    assert "depth.hip" in build.SOURCES
    lib = hip.lib()
    one = ctypes.c_void_p(16)                                                        # never dereferenced: every call below is rejected first
    assert lib.mudg_depth_align_sums(None, None, 1, 1, 1, None, None) == -1
    assert lib.mudg_depth_align_sums(one, one, 1, 4097, 4096, one, None) == -1 and b"2^24" in lib.mudg_last_error()
    assert lib.mudg_depth_align_sums(one, one, 0, 8, 8, one, None) == -1
    assert lib.mudg_depth_align_solve(None, 1, None, None, None) == -1
    assert lib.mudg_depth_finish(None, None, None, 10, 1, 1, 1, None, None, None) == -1
    assert lib.mudg_depth_finish(one, one, None, 10, 1, 4097, 4096, one, None, None) == -1
    assert lib.mudg_colormap_spectral(None, 1, 0.0, 1.0, 0, None, None, None) == -1
    assert lib.mudg_colormap_spectral(one, 0, 0.0, 1.0, 0, one, None, None) == -1
    assert lib.mudg_colormap_spectral(one, 1, 1.0, 1.0, 0, one, None, None) == -1 and b"range" in lib.mudg_last_error()
    assert lib.mudg_depth_unproject(None, None, None, 10, None, 1, 1, 1, 0.0, 100.0, None, None, None) == -1
    assert lib.mudg_depth_unproject(one, one, None, 10, one, 1, 4097, 4096, 0.0, 100.0, one, one, None) == -1


def test_depth_kernels_use_no_scratch_and_the_native_64_bit_integer_add(tmp_path):
    """Facts about the generated gfx950 code that do not depend on the compiler's scheduling."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "depth.s"
    subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S",
                    os.path.join(ROOT, "mudg_amd", "csrc", "depth.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    s = out.read_text()
    md = s[s.index("amdhsa.kernels"):]
    families = ("depth_align_sums_kernel", "depth_align_solve_kernel", "depth_finish_kernel", "colormap_spectral_kernel", "depth_unproject_kernel")
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", md, re.S):
        for family in families:
            if family in m.group(1):
                seen[family] = seen.get(family, 0) + 1
                assert int(m.group(2)) == 0, m.groups()
    assert seen == {"depth_align_sums_kernel": 2, "depth_align_solve_kernel": 1, "depth_finish_kernel": 2, "colormap_spectral_kernel": 1,
                    "depth_unproject_kernel": 2}, seen
    assert "cmpswap" not in s
    names = sorted(set(re.findall(r"^(_Z\S*depth_align_sums_kernel\S*):", s, re.M)))
    assert len(names) == 2
    for name in names:
        body = s[s.index(name + ":"):]
        lines = [l.strip() for l in body[:body.index(".end_amdhsa_kernel")].splitlines()]
        assert sum(l.startswith("global_atomic_add_x2") for l in lines) == 5, name
        assert not any(l.startswith(("scratch_", "flat_")) for l in lines), name
    for name in sorted(set(re.findall(r"^(_Z\S*depth_\w+_kernelILi4E\S*):", s, re.M))):                      # the four-pixel forms: 16-byte accesses
        body = s[s.index(name + ":"):]
        lines = [l.strip() for l in body[:body.index(".end_amdhsa_kernel")].splitlines()]
        assert any(l.startswith(("global_load_dwordx4", "global_store_dwordx4")) for l in lines), name
        assert not any(l.startswith(("scratch_", "flat_")) for l in lines), name
