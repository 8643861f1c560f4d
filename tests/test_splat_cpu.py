"""Host side of the sparse-condition renderer that needs no GPU: virtual_poses and the object merge against the REFERENCE's functions
(tests/golden/splat_host.pt, made by tests/golden/make_golden_splat.py), the CPU definition of the raster rule (tests/splat_reference.py)
against hand-derived cases, the 13 x 13 box against three 5 x 5 dilations, and the C-ABI and generated code of csrc/splat.hip."""
import os
import re

import numpy as np
import pytest
import torch

import splat_reference as sr
from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ------------------------------------------------------------------------------------------------ against the reference's host functions
def test_virtual_poses_equal_the_reference_exactly():
    from mudg_amd.render import virtual_poses
    g = golden("splat_host.pt")
    for k, c2w in enumerate(g["c2w"].numpy()):
        for tag, kw in (("default", {}), ("with_ori", {"with_ori_pose": True}), ("shift", {"shift": g["shift"]})):
            got = np.stack(virtual_poses(c2w, **kw))
            want = g["poses"][tag][k].numpy()
            assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want), (k, tag)
    left, right = virtual_poses(np.eye(4))
    assert left[0, 3] == -2.0 and right[0, 3] == 2.0
    assert virtual_poses(np.eye(4), shift=1.23456789)[1][0, 3] == 1.2346            # the reference's round(., 4)


def test_object_merge_equals_the_reference_exactly():
    from mudg_amd.render import merge_objects
    g = golden("splat_host.pt")
    xyz, rgb = g["points"].numpy(), g["colors"].numpy()
    tr, vis = g["transform_obj"].numpy(), g["visibility"].numpy()
    assert np.array_equal(g["obj_vis"].numpy(), vis.T)
    sizes = []
    for f, want in enumerate(g["merged"]):
        got_xyz, got_rgb = merge_objects(xyz, rgb, tr, vis, f)
        assert got_xyz.dtype == want["xyz"].numpy().dtype and np.array_equal(got_xyz, want["xyz"].numpy()), f
        assert np.array_equal(got_rgb, want["rgb"].numpy()), f
        sizes.append(len(got_xyz))
    assert sizes == [150, 100, 150, 1]                                               # one object hidden in frame 1; the sentinel in frame 3
    assert np.array_equal(g["merged"][3]["xyz"].numpy(), [[1000, 1000, 1000]])


def test_host_matrices_compose_w2c_with_the_object_transform():
    from mudg_amd.render import object_matrices, virtual_poses
    g = golden("splat_host.pt")
    xyz, tr, vis = g["points"].numpy(), g["transform_obj"].numpy(), g["visibility"].numpy()
    for f in range(4):
        poses = np.stack(virtual_poses(g["c2w"].numpy()[f], with_ori_pose=True))
        w2c = np.linalg.inv(poses)
        m = object_matrices(w2c, tr, vis, f)
        assert m.shape == (3, 3, 3, 4) and m.dtype == np.float64
        shown = [i for i in range(3) if vis[i, f] == 1]
        merged = g["merged"][f]["xyz"].numpy()
        at = 0
        for i in range(3):
            for p in range(3):
                if i not in shown:
                    assert not m[p, i].any()                                        # zc = 0 fails the near test
                    continue
                assert np.array_equal(m[p, i].astype(F), sr.host_matrix(poses[p], tr[i, f]))
                # the fused matrix on the object's own points = w2c on what the reference merges, up to float64 rounding
                fused = xyz[i] @ m[p, i, :, :3].T + m[p, i, :, 3]
                two_step = merged[at:at + 50] @ w2c[p, :3, :3].T + w2c[p, :3, 3]
                assert np.allclose(fused, two_step, rtol=0, atol=1e-11)
            at += 50 if i in shown else 0


# ------------------------------------------------------------------------------------------------ the CPU definition, by hand
EYE = np.eye(4)[:3].astype(F)
CAM = np.array([1, 1, 0, 0], dtype=F)                                               # u = x / z, v = y / z


def _covered(u, v, size, z=1.0, H=24, W=24):
    rgb, depth = sr.splat(np.array([[u * z, v * z, z]]), np.array([[200, 100, 50]], np.uint8), EYE, CAM, size, H, W)
    rows, cols = np.nonzero(depth)
    assert np.array_equal(depth > 0, rgb.any(axis=2)) and np.all(rgb[depth > 0] == [200, 100, 50]) and np.all(depth[depth > 0] == F(z))
    return sorted(set(rows.tolist())), sorted(set(cols.tolist())), int((depth > 0).sum())


def test_sprite_coverage_by_hand():
    assert _covered(10.5, 10.5, 2.5) == ([9, 10, 11], [9, 10, 11], 9)
    assert _covered(10.0, 10.0, 2.5) == ([9, 10], [9, 10], 4)
    assert _covered(10.5, 10.5, 4) == ([8, 9, 10, 11], [8, 9, 10, 11], 16)
    assert _covered(10.0, 10.0, 4) == ([8, 9, 10, 11], [8, 9, 10, 11], 16)
    assert _covered(0.2, 0.2, 4) == ([0, 1], [0, 1], 4)                              # clipped at the top-left corner
    assert _covered(23.4, 10.5, 2.5) == ([9, 10, 11], [22, 23], 6)                   # [22.15, 24.65): column 24 is clipped at the right edge
    assert _covered(10.5, 24.9, 4) == ([23], [8, 9, 10, 11], 4)                      # only its first row is inside
    assert _covered(-2.0, 10.5, 4) == ([], [], 0) and _covered(26.1, 10.5, 4) == ([], [], 0)
    # projection happens: the same pixel from three times the distance
    assert _covered(10.5, 10.5, 2.5, z=3.0) == ([9, 10, 11], [9, 10, 11], 9)


def test_near_and_far_planes_are_exclusive():
    for z, n in ((sr.ZNEAR, 0), (sr.ZFAR, 0), (F(sr.ZNEAR) * F(2), 9), (199.0, 9), (-1.0, 0), (0.0, 0)):
        z = float(F(z))
        _, depth = sr.splat(np.array([[10.5 * z, 10.5 * z, z]]), np.array([[9, 9, 9]], np.uint8), EYE, CAM, 2.5, 24, 24)
        assert int((depth > 0).sum()) == n, z


def test_depth_test_smallest_zc_then_lowest_index():
    xyz = np.array([[10.5, 10.5, 1.0], [10.5, 10.5, 1.0], [21.0, 21.0, 2.0], [5.25, 5.25, 0.5]])
    rgb = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90], [1, 2, 3]], np.uint8)
    img, depth = sr.splat(xyz[:3], rgb[:3], EYE, CAM, 2.5, 24, 24)
    assert np.all(img[9:12, 9:12] == [10, 20, 30]) and np.all(depth[9:12, 9:12] == 1.0) and int((depth > 0).sum()) == 9
    img, depth = sr.splat(xyz[[1, 0, 2]], rgb[[1, 0, 2]], EYE, CAM, 2.5, 24, 24)    # the order of equals decides, not the colour
    assert np.all(img[9:12, 9:12] == [40, 50, 60])
    img, depth = sr.splat(xyz, rgb, EYE, CAM, 2.5, 24, 24)                           # a nearer point drawn last still wins
    assert np.all(img[9:12, 9:12] == [1, 2, 3]) and np.all(depth[9:12, 9:12] == 0.5)
    # per-point matrices: the second point moved one pixel to the right by its own matrix
    shift = EYE.copy()
    shift[0, 3] = 1.0
    img, depth = sr.splat(xyz[:2], rgb[:2], np.stack([EYE, shift]), CAM, 2.5, 24, 24)
    assert np.all(img[9:12, 9:12] == [10, 20, 30]) and np.all(img[9:12, 12] == [40, 50, 60]) and int((depth > 0).sum()) == 12


def test_float_colours_are_converted_once_by_rounding():
    assert np.array_equal(sr.to_u8(np.array([[0.0, 0.5, 1.0], [0.499, 0.002, 0.998]])), [[0, 128, 255], [127, 1, 254]])
    from mudg_amd.render import _pack
    packed = _pack(np.array([[1.0, -2.0, 3.5]]), np.array([[0.0, 0.5, 1.0]]), torch.device("cpu"))
    assert packed.dtype == torch.int32 and packed.shape == (1, 4)
    assert np.array_equal(packed[0, :3].numpy().view(F), F([1.0, -2.0, 3.5])) and int(packed[0, 3]) == 0 | 128 << 8 | 255 << 16
    assert torch.equal(_pack(np.array([[1.0, -2.0, 3.5]]), np.array([[0, 128, 255]], np.uint8), torch.device("cpu")), packed)


def test_merge_and_conditions_by_hand():
    H, W = 20, 30
    bg_rgb = np.full((H, W, 3), 100, np.uint8)
    bg_d = np.full((H, W), 150.0, F)
    ob_rgb = np.zeros((H, W, 3), np.uint8)
    ob_d = np.zeros((H, W), F)
    ob_rgb[10, 15] = [255, 1, 7]
    ob_d[10, 15] = 25.0
    ob_rgb[0, 0] = [255, 0, 7]                                                       # one channel zero: not in the mask
    rgb, depth, mask = sr.merge(bg_rgb, bg_d, ob_rgb, ob_d)
    want = np.zeros((H, W), bool)
    want[4:17, 9:22] = True
    assert np.array_equal(mask, want)
    assert np.all(rgb[~mask] == 100) and np.all(depth[~mask] == 150.0)
    assert int(rgb[mask].sum()) == 263 and np.all(rgb[10, 15] == [255, 1, 7]) and depth[10, 15] == 25.0 and float(depth[mask].sum()) == 25.0
    sparse, sdepth = sr.conditions(rgb, depth)
    assert sparse.shape == (3, H, W) and sdepth.shape == (3, H, W) and sparse.dtype == F and sdepth.dtype == F
    assert sparse[0, 10, 15] == 1.0 and sparse[0, 10, 14] == -1.0 and sparse[1, 0, 0] == (F(100) / F(255) - F(0.5)) * F(2)
    assert sdepth[2, 0, 0] == 1.0 and sdepth[0, 10, 15] == -0.5 and sdepth[1, 10, 14] == -1.0          # clamped at 100 m; 25 m; nothing


def test_the_13_box_equals_three_5_box_dilations():
    from scipy.ndimage import binary_dilation
    rng = np.random.default_rng(7)
    masks = [rng.random((37, 53)) < p for p in (0.001, 0.01, 0.2)]
    edges = np.zeros((40, 31), bool)
    edges[0, 5] = edges[39, 11] = edges[17, 0] = edges[23, 30] = edges[0, 0] = edges[39, 30] = True
    masks += [edges, np.zeros((9, 9), bool), np.ones((9, 9), bool), rng.random((5, 70)) < 0.05]
    for m in masks:
        want = binary_dilation(m, np.ones((5, 5)), iterations=3, border_value=0)
        assert np.array_equal(sr.dilate13(m), want)


# ------------------------------------------------------------------------------------------------ C-ABI and generated code
def test_splat_entry_points_are_declared_bound_and_exported():
    import ctypes
    from mudg_amd import build, hip
    header = open(os.path.join(ROOT, "include", "mudg_hip.h")).read()
    for name, nargs in (("mudg_splat_points", 19), ("mudg_splat_resolve", 7), ("mudg_splat_compose", 16)):
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, header, re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == nargs
        assert hasattr(hip.lib(), name)
        for path in hip.LIB_PATHS.values():                                          # operand-type independent: in every build
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert "splat.hip" in build.SOURCES
    lib = hip.lib()
    assert lib.mudg_splat_points(None, None, 1, None, 1, 1, None, 1, 1, 1.0, 1.0, 0.0, 0.0, 1e-4, 200.0, 2.5, 0, None, None) == -1
    assert lib.mudg_splat_resolve(None, None, 1, None, None, 1, None) == -1
    assert lib.mudg_splat_compose(None, None, None, None, None, None, 0, 1, 1, 0, 1, 1, None, None, None, None) == -1


def test_inputs_off_the_gpu_raise():
    from mudg_amd import hip, ops, render
    with pytest.raises(hip.MudgError, match="on the GPU"):
        render.PointCloud(torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(hip.MudgError, match="PointCloud"):
        render.render_conditions(np.zeros((4, 3)), None, np.eye(3), np.eye(4)[None], (8, 8), (8, 8))
    with pytest.raises(hip.MudgError, match="on the GPU"):
        ops.splat_points(torch.zeros(4, 4, dtype=torch.int32), torch.zeros(1, 1, 12), torch.zeros(1, 8, 8, dtype=torch.int64), (1, 1, 0, 0), 2.5)


def test_the_product_does_not_import_the_cpu_definition():
    for d in ("mudg_amd", "lvdm", "utils", "virtual_render"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith(".py"):
                    assert "splat_reference" not in open(os.path.join(base, f)).read(), f


def test_splat_kernels_use_no_scratch_a_native_64_bit_minimum_and_16_byte_point_loads(tmp_path):
    """Facts about the generated gfx950 code that do not depend on the compiler's scheduling."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "splat.s"
    subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S",
                    os.path.join(ROOT, "mudg_amd", "csrc", "splat.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    s = out.read_text()
    md = s[s.index("amdhsa.kernels"):]
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", md, re.S):
        for family in ("splat_points_kernel", "splat_resolve_kernel", "splat_compose_kernel"):
            if family in m.group(1):
                seen[family] = seen.get(family, 0) + 1
                assert int(m.group(2)) == 0, m.groups()
    assert seen == {"splat_points_kernel": 4, "splat_resolve_kernel": 2, "splat_compose_kernel": 1}, seen
    assert "cmpswap" not in s
    names = sorted(set(re.findall(r"^(_Z\S*splat_points_kernel\S*):", s, re.M)))
    assert len(names) == 4
    for name in names:
        body = s[s.index(name + ":"):]
        lines = [l.strip() for l in body[:body.index(".end_amdhsa_kernel")].splitlines()]
        assert any(l.startswith("global_atomic_umin_x2") for l in lines), name
        assert any(l.startswith("global_load_dwordx4") for l in lines), name
        assert not any(l.startswith(("scratch_", "flat_")) for l in lines), name
