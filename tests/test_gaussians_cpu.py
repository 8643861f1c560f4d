"""What the Gaussian splat rule can show without a GPU: the polynomial exponential, the fp32 definition
(tests/gaussians_reference.py) against a float64 textbook renderer and against answers known without arithmetic, the tile rectangles at
the image's edges, the host side of the Python surface, and the C-ABI and generated code of csrc/gaussians.hip."""
import os
import re

import numpy as np
import pytest
import torch

import gaussians_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
ENTRIES = (("mudg_gauss_project", 22), ("mudg_gauss_keys", 12), ("mudg_gauss_ranges", 5), ("mudg_gauss_blend", 16))
# The fp32 rule against the float64 textbook on gr.seeded_scene(), pixels near a threshold excluded: measured on the CPU 9.5e-7 on rgb and
# 1.18e-6 on alpha (0.85 % of the pixels excluded); the bound is four times the larger, the margin being float64's accumulation order.
MEASURED_FP32_ERROR = 1.18e-6
FP32_BOUND = 4 * MEASURED_FP32_ERROR


# ------------------------------------------------------------------------------------------------ E(p)
def test_the_polynomial_exponential_is_close_monotonic_and_exact_at_zero():
    p = np.linspace(-5.6, 0.0, 2_000_000).astype(F)
    e = gr.exp_rule(p)
    assert e.dtype == F
    rel = np.abs(e.astype(D) - np.exp(p.astype(D))) / np.exp(p.astype(D))
    print(f"E(p) over {len(p)} points of [-5.6, 0]: max relative error {rel.max():.3e}")
    assert rel.max() <= 1e-6
    assert (np.diff(e) >= 0).all()
    assert gr.exp_rule(F(0.0)) == F(1.0) and gr.exp_rule(F(-0.0)) == F(1.0)
    assert gr.exp_rule(F(-5.55)) < gr.MIN_ALPHA                                  # nothing of opacity <= 1 is lost below the cut
    assert np.floor(F(-5.55) * gr.LOG2E) == -9                                    # ldexp by n >= -9: no denormal


# ------------------------------------------------------------------------------------------------ the rule against the textbook
def test_the_fp32_rule_follows_the_float64_textbook():
    xyz, rgb, cov, opacity, mats, cam = gr.seeded_scene()
    hw = (40, 56)
    got = gr.render(gr.pack(xyz, rgb), cov, opacity, None, mats, cam, hw)
    want_rgb, want_alpha, near = gr.textbook_render(xyz, rgb, cov, opacity, mats[0, 0], cam, hw)
    keep = ~near
    e_rgb = np.abs(got["rgb"][0].astype(D) - want_rgb)[:, keep].max()
    e_alpha = np.abs(got["alpha"][0].astype(D) - want_alpha)[keep].max()
    print(f"{int((got['count'] > 0).sum())} of {len(xyz)} Gaussians drawn, {got['entries']} entries, longest tile {got['longest_tile']}; "
          f"{near.mean():.4f} of the pixels excluded; rgb {e_rgb:.3e}, alpha {e_alpha:.3e} (bound {FP32_BOUND:.3e})")
    assert (got["count"] > 0).sum() > 300 and got["longest_tile"] > 50 and (want_alpha > 0.5).mean() > 0.5
    assert near.mean() <= 0.05
    assert e_rgb <= FP32_BOUND and e_alpha <= FP32_BOUND


# ------------------------------------------------------------------------------------------------ answers known without arithmetic
def _flat(centres, scale, hw, **kw):
    pts, cov, op = gr.flat_case(centres, scale, **kw)
    return pts, gr.render(pts, cov, op, None, gr.FLAT[None], gr.FLAT_CAM, hw)


def test_one_opaque_gaussian_on_a_pixel_centre_gives_the_alpha_cap():
    pts, out = _flat([[8.5, 8.5]], 0.5, (16, 16))
    assert out["uv"][0, 0].tolist() == [8.5, 8.5] and out["depth"][0, 0] == F(gr.FOCAL) and out["count"][0, 0] == 1
    assert out["alpha"][0, 8, 8] == gr.MAX_ALPHA
    word = int(pts[0, 3])
    for k in range(3):
        assert out["rgb"][0, k, 8, 8] == (F((word >> (8 * k)) & 0xff) * gr.MAX_ALPHA) / F(255.0)
    assert out["depth_image"][0, 8, 8] == F(gr.FOCAL) * gr.MAX_ALPHA
    assert out["alpha"][0, 0, 0] == 0 and (out["rgb"][0, :, 0, 0] == 0).all()               # p < -5.55 there: skipped


def test_a_second_opaque_gaussian_ends_the_pixel_and_is_not_added():
    pts, out = _flat([[8.5, 8.5], [8.5, 8.5]], 0.5, (16, 16), z=[128.0, 160.0])
    one = gr.render(pts[:1], gr.isotropic(0.5, 1), np.ones(1, F), None, gr.FLAT[None], gr.FLAT_CAM, (16, 16))
    assert out["values"].tolist() == [0, 1]
    assert out["alpha"][0, 8, 8] == gr.MAX_ALPHA and (out["rgb"][0, :, 8, 8] == one["rgb"][0, :, 8, 8]).all()
    assert (F(1.0) - gr.MAX_ALPHA) * (F(1.0) - gr.MAX_ALPHA) < gr.MIN_T                      # why: Tn of the second is below the cut
    assert out["alpha"][0, 8, 10] > one["alpha"][0, 8, 10] > 0                               # further out both are added


def test_equal_depths_put_the_lower_index_in_front():
    pts, cov, op = gr.flat_case([[8.5, 8.5], [8.5, 8.5]], 0.5)
    pts[0, 3], pts[1, 3] = 0x0000ff, 0x00ff00                                                # red, then green
    out = gr.render(pts, cov, op, None, gr.FLAT[None], gr.FLAT_CAM, (16, 16))
    full = (F(255.0) * gr.MAX_ALPHA) / F(255.0)
    assert out["values"].tolist() == [0, 1] and out["rgb"][0, 0, 8, 8] == full and out["rgb"][0, 1, 8, 8] == 0
    swapped = gr.render(pts[::-1].copy(), cov, op, None, gr.FLAT[None], gr.FLAT_CAM, (16, 16))
    assert swapped["rgb"][0, 1, 8, 8] == full and swapped["rgb"][0, 0, 8, 8] == 0


def test_what_is_dropped_has_count_zero():
    z = np.full(9, gr.FOCAL, F)
    z[2], z[3] = 0.2, 200.0                                                                  # zc on either bound
    pts, cov, op = gr.flat_case([[8.5, 8.5]] * 9, 0.5, z=z)
    xyz, _ = gr.unpack(pts)
    cov[1] = [1.0, 0.0, 0.0, -1.0, 0.0, 1.0]                                                 # det <= 0 after the projection
    cov[4] = gr.isotropic(2000.0, 1)[0]                                                      # rad > 4096
    op[5], op[6] = F(1.0) / F(256.0), np.nan                                                 # below 1 / 255; not a number
    cov[7, 0] = np.inf
    ids = np.zeros(9, np.int32)
    ids[8] = 1
    mats = np.concatenate([gr.FLAT, np.zeros((1, 12), F)])[None]                             # id 1: the zero matrix, zc = 0
    proj = gr.project(xyz, cov, op, ids, mats, gr.FLAT_CAM, (16, 16))
    assert proj["count"][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0]
    for k in ("uv", "conic", "depth", "rect"):
        assert not proj[k][0, 1:].any(), k
    op[5] = gr.MIN_ALPHA                                                                     # exactly 1 / 255 is drawn
    z[2], z[3] = np.nextafter(F(0.2), F(1)), np.nextafter(F(200.0), F(0))                   # one step inside
    xyz = gr.unpack(gr.flat_case([[8.5, 8.5]] * 9, 0.5, z=z)[0])[0]
    cov[4] = gr.isotropic(1000.0, 1)[0]
    proj = gr.project(xyz, cov, op, ids, mats, gr.FLAT_CAM, (16, 16))
    assert proj["count"][0].tolist() == [1, 0, 1, 1, 1, 1, 0, 0, 0]


def test_the_tile_rectangle_is_clipped_at_every_edge_of_the_image():
    hw = (40, 56)                                                                            # TX = 4, TY = 3: the last column and row are partial
    centres = [[-2.0, 8.0], [-4.0, 8.0], [58.0, 8.0], [67.5, 8.0], [8.0, -2.0], [8.0, -4.0], [8.0, 42.0], [8.0, 51.5], [16.0, 16.0],
               [1e30, 8.0], [-1e30, 8.0], [8.0, 1e30], [8.0, -1e30], [28.0, 20.0]]
    pts, cov, op = gr.flat_case(centres, 0.5)
    proj = gr.project(gr.unpack(pts)[0], cov, op, None, gr.FLAT[None], gr.FLAT_CAM, hw)
    rect, count = proj["rect"][0].tolist(), proj["count"][0].tolist()
    assert rect[0] == [0, 1, 0, 1] and count[1] == 0 and rect[2] == [3, 4, 0, 1] and count[3] == 0
    assert rect[4] == [0, 1, 0, 1] and count[5] == 0 and rect[6] == [0, 1, 2, 3] and count[7] == 0
    assert rect[8] == [0, 2, 0, 2] and count[8] == 4                                         # on a tile corner: rad 3 reaches four tiles
    assert count[9:13] == [0, 0, 0, 0] and rect[13] == [1, 2, 1, 2]
    assert not proj["uv"][0, 9:13].any()
    wide = gr.flat_case([[28.0, 20.0]], 60.0)
    proj = gr.project(gr.unpack(wide[0])[0], wide[1], wide[2], None, gr.FLAT[None], gr.FLAT_CAM, hw)
    assert proj["rect"][0, 0].tolist() == [0, 4, 0, 3] and proj["count"][0, 0] == 12         # every tile of the image


def test_ranges_and_the_stable_order_of_one_tile():
    pts, cov, op = gr.flat_case([[8.5, 8.5], [24.5, 8.5], [8.5, 8.5], [16.0, 8.5]], 0.5, z=[160.0, 128.0, 128.0, 128.0])
    out = gr.render(pts, cov, op, None, gr.FLAT[None], gr.FLAT_CAM, (16, 48))
    assert out["count"][0].tolist() == [1, 1, 1, 2] and out["entries"] == 5
    assert out["values"].tolist() == [2, 3, 0, 1, 3] and out["ranges"].tolist() == [[0, 3], [3, 5], [0, 0]]     # an empty tile is [0, 0)
    assert out["longest_tile"] == 3


# ------------------------------------------------------------------------------------------------ the Python surface off the GPU
def test_covariances_from_scales_and_rotations_against_float64():
    from mudg_amd import gaussians
    rng = np.random.default_rng(3)
    n = 200
    scales = rng.uniform(0.01, 2.0, (n, 3)).astype(F)
    quats = rng.normal(size=(n, 4)).astype(F)
    quats[0], scales[0] = [1, 0, 0, 0], [1, 2, 3]
    quats[1], scales[1] = [np.sqrt(0.5), 0, 0, np.sqrt(0.5)], [1, 2, 3]                      # a quarter turn about z: x and y change places
    got = gaussians.covariance_from_scales_rotations(torch.from_numpy(scales), torch.from_numpy(quats)).numpy()
    q = quats.astype(D) / np.linalg.norm(quats.astype(D), axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)
    full = R @ (scales.astype(D)[:, :, None] ** 2 * np.swapaxes(R, 1, 2))
    want = np.stack([full[:, 0, 0], full[:, 0, 1], full[:, 0, 2], full[:, 1, 1], full[:, 1, 2], full[:, 2, 2]], axis=1)
    assert got.dtype == F and got.shape == (n, 6)
    assert got[0].tolist() == [1, 0, 0, 4, 0, 9]
    # about a dozen fp32 roundings on the way to an entry of size at most max(s)^2: 2e-6 of that is three times their sum
    assert (np.abs(got - want).max(axis=1) <= 2e-6 * (scales.astype(D) ** 2).max(axis=1)).all()
    assert np.allclose(got[1], [4, 0, 0, 1, 0, 9], atol=1e-5)
    assert (np.linalg.eigvalsh(full) > 0).all()


def _host_cloud(n=3):
    from mudg_amd import render
    pc = render.PointCloud.__new__(render.PointCloud)
    pc.points = torch.zeros((n, 4), dtype=torch.int32)
    return pc


def test_tensors_off_the_gpu_are_refused():
    from mudg_amd import gaussians, hip, ops
    pc = _host_cloud()
    cov, op = torch.zeros((3, 6)), torch.ones(3)
    for make in (lambda: gaussians.Gaussians(pc, cov, op), lambda: gaussians.Gaussians.from_cloud(pc, 0.1),
                 lambda: gaussians.Gaussians.from_scales_rotations(pc, torch.ones((3, 3)), torch.ones((3, 4))),
                 lambda: gaussians.Gaussians.from_scene(pc, None, 0.1)):
        with pytest.raises(hip.MudgError, match="on the GPU"):
            make()
    with pytest.raises(hip.MudgError, match="PointCloud"):
        gaussians.Gaussians(pc.points, cov, op)
    with pytest.raises(hip.MudgError, match="Gaussians"):
        gaussians.render(pc, torch.zeros((1, 1, 12)), (1.0, 1.0, 0.0, 0.0), (16, 16))
    g = gaussians.Gaussians.__new__(gaussians.Gaussians)
    g.cloud, g.cov, g.opacity, g.ids = pc, cov, op, None
    with pytest.raises(hip.MudgError, match="on the GPU"):
        gaussians.render(g, torch.zeros((1, 1, 12)), (1.0, 1.0, 0.0, 0.0), (16, 16))
    i32, f32 = pc.points, torch.zeros((1, 3))
    for call in (lambda: ops.gauss_project(i32, cov, op, torch.zeros((1, 1, 12)), (1.0, 1.0, 0.0, 0.0), (16, 16)),
                 lambda: ops.gauss_keys(f32, torch.zeros((1, 3, 4), dtype=torch.int32), torch.zeros((1, 3), dtype=torch.int32),
                                        torch.zeros((1, 3), dtype=torch.int64), 1, (16, 16)),
                 lambda: ops.gauss_ranges(torch.zeros(4, dtype=torch.int64), 1),
                 lambda: ops.gauss_blend(i32, torch.zeros((1, 3, 2)), torch.zeros((1, 3, 4)), f32, torch.zeros(1, dtype=torch.int32),
                                         torch.zeros((1, 2), dtype=torch.int32), (16, 16))):
        with pytest.raises(hip.MudgError, match="on the GPU"):
            call()
    assert gaussians.ZNEAR == gr.ZNEAR and gaussians.ZFAR == gr.ZFAR and gaussians.MAX_ENTRIES == 2 ** 28 and ops.GAUSS_TILE == gr.TILE


def test_the_product_does_not_import_the_cpu_definition():
    for d in ("mudg_amd", "lvdm", "utils", "virtual_render", "main", "tools"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith(".py"):
                    assert "gaussians_reference" not in open(os.path.join(base, f)).read(), f
    for f in ("bench.py", "__graft_entry__.py"):
        assert "gaussians_reference" not in open(os.path.join(ROOT, f)).read(), f


# ------------------------------------------------------------------------------------------------ C-ABI and generated code
def test_gauss_entry_points_are_declared_bound_and_exported():
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
    assert "gaussians.hip" in build.SOURCES and "-ffp-contract=off" in build.FLAGS


def test_bad_arguments_are_refused_before_any_launch():
    import ctypes
    from mudg_amd import hip
    lib = hip.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)                              # never dereferenced: every call below is rejected first
    nan, inf = float("nan"), float("inf")

    def refused(fn, good, changes, text=None):
        args = list(good)
        for k, v in changes.items():
            args[k] = v
        assert fn(*args) == -1, (fn.__name__, changes)
        if text:
            assert text in lib.mudg_last_error(), (fn.__name__, changes, lib.mudg_last_error())

    # points cov opacity ids n mats V nmat H W fx fy cx cy znear zfar uv conic depth rect count stream
    good = [one, one, one, one, 10, one, 1, 2, 32, 32, 50.0, 50.0, 16.0, 16.0, 0.2, 200.0, one, one, one, one, one, None]
    for k in (0, 1, 2, 5, 16, 17, 18, 19, 20):
        refused(lib.mudg_gauss_project, good, {k: None}, b"null")
    refused(lib.mudg_gauss_project, good, {3: None}, b"ids")                          # two matrices per view and no ids
    refused(lib.mudg_gauss_project, good, {0: odd}, b"unaligned")
    for k in (17, 19):
        refused(lib.mudg_gauss_project, good, {k: odd}, b"unaligned")
    for k in (4, 6, 7, 8, 9):
        for v in (0, -1):
            refused(lib.mudg_gauss_project, good, {k: v})
    refused(lib.mudg_gauss_project, good, {4: 2 ** 31}, b"32-bit index")
    refused(lib.mudg_gauss_project, good, {6: 2 ** 20, 8: 1024, 9: 1024}, b"2^31")    # V NT = 2^32
    refused(lib.mudg_gauss_project, good, {6: 2 ** 19, 8: 1024, 9: 1024}, b"2^31")    # V NT = 2^31 exactly
    refused(lib.mudg_gauss_project, good, {8: 2 ** 23}, b"image")
    for znear, zfar in ((0.0, 200.0), (-1.0, 200.0), (nan, 200.0), (0.2, nan), (0.2, inf), (inf, inf), (0.2, 0.2), (5.0, 1.0)):
        refused(lib.mudg_gauss_project, good, {14: znear, 15: zfar}, b"znear")
    for k in (10, 11):
        for v in (0.0, -50.0, nan, inf):
            refused(lib.mudg_gauss_project, good, {k: v}, b"intrinsics")
    refused(lib.mudg_gauss_project, good, {12: nan}, b"intrinsics")

    # depth rect count offsets n V H W E keys values stream
    good = [one, one, one, one, 10, 1, 32, 32, 5, one, one, None]
    for k in (0, 1, 2, 3, 9, 10):
        refused(lib.mudg_gauss_keys, good, {k: None}, b"null")
    refused(lib.mudg_gauss_keys, good, {1: odd}, b"unaligned")
    for k in (4, 5, 6, 7):
        refused(lib.mudg_gauss_keys, good, {k: 0})
    for e in (0, -1, 2 ** 31, 2 ** 40):
        refused(lib.mudg_gauss_keys, good, {8: e}, b"entries")
    refused(lib.mudg_gauss_keys, good, {5: 2 ** 20, 6: 1024, 7: 1024}, b"2^31")
    refused(lib.mudg_gauss_keys, good, {4: 2 ** 31 - 1, 5: 65536}, b"grid")           # more workgroups than a grid holds

    # keys E tiles ranges stream
    good = [one, 5, 4, one, None]
    for k in (0, 3):
        refused(lib.mudg_gauss_ranges, good, {k: None}, b"null")
    for e in (0, -1, 2 ** 31):
        refused(lib.mudg_gauss_ranges, good, {1: e}, b"entries")
    for t in (0, -1, 2 ** 31):
        refused(lib.mudg_gauss_ranges, good, {2: t}, b"tiles")

    # points uv conic depth values ranges n E V H W rgb depth alpha walked stream
    good = [one, one, one, one, one, one, 10, 5, 1, 32, 32, one, one, one, None, None]
    for k in (0, 1, 2, 3, 4, 5, 11, 12, 13):
        refused(lib.mudg_gauss_blend, good, {k: None}, b"null")
    for k in (0, 2):
        refused(lib.mudg_gauss_blend, good, {k: odd}, b"unaligned")
    for k in (6, 8, 9, 10):
        for v in (0, -1):
            refused(lib.mudg_gauss_blend, good, {k: v})
    for e in (0, -1, 2 ** 31):
        refused(lib.mudg_gauss_blend, good, {7: e}, b"entries")
    refused(lib.mudg_gauss_blend, good, {8: 2 ** 20, 9: 1024, 10: 1024}, b"2^31")


def test_gauss_kernels_use_no_scratch_and_the_blend_keeps_its_lds(tmp_path):
    """Facts about the generated gfx950 code as DESIGN.md §23 records them: no scratch and no spill in any kernel, LDS only in the blend
    kernel, 8 KiB of entries plus the 256 bytes the counting barrier keeps."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "gaussians.s"
    subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S",
                    os.path.join(ROOT, "mudg_amd", "csrc", "gaussians.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    s = out.read_text()
    md = s[s.index("amdhsa.kernels"):]
    seen = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", md, re.S):
        kind = re.search(r"gauss_(project|keys|ranges|blend)_kernel", m.group(2))
        assert kind, m.group(2)
        seen[kind.group(1)] = (int(m.group(1)), int(m.group(4)))
        print(f"{m.group(2)}: {m.group(1)} bytes of LDS, {m.group(4)} VGPRs")
        assert int(m.group(3)) == 0 and int(m.group(5)) == 0, m.groups()
    assert set(seen) == {"project", "keys", "ranges", "blend"}, seen
    assert all(seen[k][0] == 0 for k in ("project", "keys", "ranges"))
    assert 8192 <= seen["blend"][0] <= 8192 + 256
    assert seen["blend"][1] <= 64 and seen["project"][1] <= 72                       # eight and seven waves a SIMD
    for name in sorted(set(re.findall(r"^(_Z\S*gauss_\w+_kernel\S*):", s, re.M))):
        body = s[s.index(name + ":"):]
        lines = [l.strip() for l in body[:body.index(".end_amdhsa_kernel")].splitlines()]
        assert not any(l.startswith(("scratch_", "flat_", "global_atomic", "buffer_atomic")) for l in lines), name
        assert not any(l.startswith("v_exp_f32") for l in lines), name                # the polynomial, not the hardware exponential
