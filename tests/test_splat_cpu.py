"""Host side of the sparse-condition renderer that needs no GPU: virtual_poses and the object merge against the REFERENCE's functions
(tests/golden/splat_host.pt, made by tests/golden/make_golden_splat.py), the CPU definition of the raster rule (tests/splat_reference.py)
against hand-derived cases, the 13 x 13 box against three 5 x 5 dilations, the C-ABI and generated code of csrc/splat.hip, and that
every case of tests/splat_cases.py (which tests/test_splat_kernels_gpu.py runs on the GPU) reaches the clause of the kernel it names."""
import os
import re

import numpy as np
import pytest
import torch

import splat_cases as sc
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


# ------------------------------------------------------------------------------------------------ the shared case table reaches its clauses
def _sprites(case, pose):
    m = case["mats"][pose]
    return sr.sprites(case["xyz"], m[0] if case["ids"] is None else m, sc.CAM, case["size"], case["H"], case["W"], case["znear"], case["zfar"],
                      ids=case["ids"])


def _winners(keys):
    return set((keys[keys != sr.EMPTY] & np.uint64(0xFFFFFFFF)).astype(np.int64).tolist())


def _reach(case, tag):
    H, W, size, P = case["H"], case["W"], case["size"], case["mats"].shape[0]
    keys, covered = sc.points_keys(case["name"])
    per_pose = [_sprites(case, p) for p in range(P)]
    if tag == "max_sprite":                                                             # the kernel's clamp never changes an image
        assert 0 < size <= sc.MAX_SPRITE - 1
        assert all(int(rok.sum(1).max(initial=0)) <= sc.MAX_SPRITE and int(cok.sum(1).max(initial=0)) <= sc.MAX_SPRITE
                   for _, _, _, rok, _, cok, _, _ in per_pose)
        assert covered > 0
    elif tag.startswith("side="):
        a = int(tag[5:])
        assert any(bool(((rok.sum(1) == a) & (cok.sum(1) == a)).any()) for _, _, _, rok, _, cok, _, _ in per_pose), tag
    elif tag == "every_border":                                                         # a sprite that covers the border pixel and reaches beyond the image
        half = F(size) / F(2)
        _, _, rows, rok, cols, cok, u, v = per_pose[0]
        for what, hit in (("column 0", (cok & (cols == 0)).any(1) & (u - half < 0)), ("column W - 1", (cok & (cols == W - 1)).any(1) & (u + half > W)),
                          ("row 0", (rok & (rows == 0)).any(1) & (v - half < 0)), ("row H - 1", (rok & (rows == H - 1)).any(1) & (v + half > H))):
            assert hit.any(), (case["name"], what)
    elif tag == "first_and_last_win":
        n = len(case["xyz"])
        assert n in sc.CLOUD_SIZES and {0, n - 1} <= _winners(keys[0])
    elif tag == "kept_and_culled":
        drawn = set(per_pose[0][0].tolist())
        assert set(case["kept"]) <= drawn and not set(case["culled"]) & drawn
        assert len(case["kept"]) >= 20 and len(case["culled"]) >= 20
    elif tag == "ties":
        index, key, rows, rok, cols, cok, _, _ = per_pose[0]
        for a, b in case["ties"]:
            ia, ib = int(np.nonzero(index == a)[0][0]), int(np.nonzero(index == b)[0][0])
            assert a < b and key[ia] >> np.uint64(32) == key[ib] >> np.uint64(32)
            pa = {(r, c) for r in rows[ia][rok[ia]] for c in cols[ia][cok[ia]]}
            pb = {(r, c) for r in rows[ib][rok[ib]] for c in cols[ib][cok[ib]]}
            assert pa & pb and all(int(keys[0][r, c] & np.uint64(0xFFFFFFFF)) == a for r, c in pa & pb)     # nothing nearer hides the tie
    elif tag == "zero_matrix":
        for p in case["empty_poses"]:
            assert not case["mats"][p].any() and bool((keys[p] == sr.EMPTY).all())
        assert bool((keys[0] != sr.EMPTY).any())
    elif tag == "on_the_bound":                                                         # lo == i + 0.5 (covered) and hi == i + 0.5 (not covered) occur
        half = F(size) / F(2)
        _, _, rows, rok, cols, cok, u, v = per_pose[0]
        for idx, ok, centre in ((cols, cok, u), (rows, rok, v)):
            mid = idx.astype(F) + F(0.5)
            assert bool((ok & (mid == (centre - half)[:, None])).any()) and bool((~ok & (mid == (centre + half)[:, None]) & (idx >= 0)).any())
    elif tag == "ids_clamped":
        ids, nmat = case["ids"], case["mats"].shape[1]
        out = list(case["out_of_range"])
        assert nmat == 3 and {-1, 3, sc.INT32_MIN, sc.INT32_MAX} <= set(ids[out].tolist()) and all(i < 0 or i >= nmat for i in ids[out])
        assert np.array_equal(sr.clamp_ids(ids[out], nmat), [0 if i < 0 else nmat - 1 for i in ids[out]])
        assert set(out) <= _winners(keys[0])                                            # each of them shows
        for wrong in (np.where((ids < 0) | (ids >= nmat), 0, ids), np.where((ids < 0) | (ids >= nmat), nmat - 1, ids), np.abs(ids.astype(np.int64)) % nmat):
            other = sr.splat_keys(case["xyz"], case["mats"][0], sc.CAM, size, H, W, ids=wrong)
            assert not np.array_equal(other, keys[0])                                   # and any other reading of them gives another image
    elif tag == "ids_do_not_matter":
        assert case["mats"].shape[1] == 1 and int(case["ids"].min()) < 0 and int(case["ids"].max()) > 0
        plain = np.stack([sr.splat_keys(case["xyz"], m[0], sc.CAM, size, H, W) for m in case["mats"]])
        assert np.array_equal(plain, keys)
    else:
        raise AssertionError(f"no such property: {tag}")


def test_every_points_case_reaches_its_clause():
    cases = sc.points_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    for c in cases:
        assert c["clause"] and c["reach"], c["name"]
        assert c["H"] <= 40 and c["W"] <= 140 and len(c["xyz"]) <= 4000
        for tag in c["reach"]:
            _reach(c, tag)
    # the table covers what it set out to cover
    assert {(c["H"], c["W"]) for c in cases} >= set(sc.IMAGE_SIZES) and {c["size"] for c in cases} == set(sc.SPRITE_SIZES)
    assert {len(c["xyz"]) for c in cases} >= set(sc.CLOUD_SIZES) and {c["mats"].shape[0] for c in cases} >= {1, 3}
    assert all(any(f"side={a}" in c["reach"] for c in cases if c["size"] == s) for s, sides in sc.SIDES.items() for a in sides)


def test_keys_decode_to_the_images_and_seeds_only_decrease():
    for c in sc.points_cases()[::5]:
        keys, _ = sc.points_keys(c["name"])
        m = c["mats"][0]
        rgb, depth = sr.splat(c["xyz"], c["rgb"], m[0] if c["ids"] is None else m, sc.CAM, c["size"], c["H"], c["W"], c["znear"], c["zfar"], ids=c["ids"])
        d, w, after = sr.resolve(keys[0], sr.pack(c["xyz"], c["rgb"], top=0xA5), len(c["xyz"]))
        assert np.array_equal(d.view(np.uint32), depth.view(np.uint32)) and np.array_equal(sr.unpack_colour(w), rgb) and bool((after == sr.EMPTY).all())
        seed = sc.seeded_keys(c)
        drawn = sr.splat_keys(c["xyz"], m[0] if c["ids"] is None else m, sc.CAM, c["size"], c["H"], c["W"], c["znear"], c["zfar"], ids=c["ids"], seed=seed[0])
        assert np.array_equal(drawn, np.minimum(seed[0], keys[0]))
        assert c["H"] * c["W"] < 100 or not (np.array_equal(drawn, keys[0]) or np.array_equal(drawn, seed[0]))       # both show through


def test_resolve_cases_hold_every_kind_of_key():
    packed = sc.resolve_points()
    assert packed.shape == (sc.RESOLVE_BUFFER, 4) and bool((packed[:, 3] >> np.uint32(24)).all())      # a non-zero top byte everywhere
    assert [c[2] for c in sc.RESOLVE_CASES] == [4, 1024, 1028, 1, 1961, 1024, 1024, 1024]
    for name, clause, pixels, offs, form in sc.RESOLVE_CASES:
        assert clause and form == (4 if pixels % 4 == 0 and not any(offs) else 1), name       # keys: 8 bytes an element; depth, colour: 4
        keys = sc.resolve_keys(pixels)
        index = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        empty, foreign = keys == sr.EMPTY, (keys != sr.EMPTY) & (index >= sc.RESOLVE_POINTS)
        assert bool((index[~empty] < sc.RESOLVE_BUFFER).all())
        if pixels >= 4:
            assert empty.any() and foreign.any() and (~empty & ~foreign).any(), name
        depth, colour, after = sr.resolve(keys, packed, sc.RESOLVE_POINTS)
        assert bool((after == sr.EMPTY).all()) and not depth[empty | foreign].any() and not colour[empty | foreign].any()
        assert bool((depth[~empty & ~foreign] > 0).all()) and bool((colour >> np.uint32(24) == 0).all())
        assert np.array_equal(colour[~empty & ~foreign], packed[index[~empty & ~foreign], 3] & np.uint32(0xFFFFFF))
    # by hand
    keys = np.array([sr.EMPTY, np.uint64(F(2.5).view(np.uint32)) << np.uint64(32) | np.uint64(1), np.uint64(F(7.0).view(np.uint32)) << np.uint64(32) | np.uint64(2)])
    depth, colour, _ = sr.resolve(keys, np.array([[0, 0, 0, 0x11223344], [0, 0, 0, 0xFF0A0B0C], [0, 0, 0, 0x55667788]], np.uint32), 2)
    assert depth.tolist() == [0.0, 2.5, 0.0] and colour.tolist() == [0, 0x0A0B0C, 0]


def test_compose_cases_place_their_object_pixels_where_they_say():
    assert set(sc.PLACED) == set(sc.COMPOSE_SIZES) and (17, 65) in sc.PLACED and (33, 130) in sc.PLACED
    for hw in sc.COMPOSE_SIZES:
        H, W = hw
        bg_c, bg_d, ob_c, ob_d = sc.compose_layers(hw)
        assert H <= 40 and W <= 140 and sc.compose_clause(hw)
        ob_rgb = sr.unpack_colour(ob_c[0])
        _, _, mask = sr.merge(sr.unpack_colour(bg_c[0]), bg_d[0], ob_rgb, ob_d[0])
        for r, c, want in sc.PLACED[hw]["probes"]:
            assert bool(mask[r, c]) == want, (hw, r, c)
        r, c = sc.PLACED[hw]["hole"]
        assert ob_rgb[r, c].any() and not ob_rgb[r, c].all()                            # one channel zero: coloured, not in the mask
        holes = ob_rgb.any(axis=2) & ~ob_rgb.all(axis=2)
        if W >= 3 and H * W > 100:                                                      # each channel is the zero one somewhere, outside every box
            assert {int(np.argmin(px)) for px in ob_rgb[holes]} == {0, 1, 2} and all((px > 0).sum() == 2 for px in ob_rgb[holes]) and not mask[holes].any()
        else:
            assert ob_rgb[r, c, 2] == 0 and sr.unpack_colour(ob_c[1])[r, c, 0] == 0     # blue in pose 0, red in pose 1
        for d in (bg_d, ob_d):                                                          # depths such as resolve gives
            assert bool(((d == 0) | ((d > 1e-4) & (d < 200))).all())
        assert (bg_d == 0).any() or H * W == 1
        assert (bg_d > 100).any() and ((bg_d > 0) & (bg_d < 100)).any() or H * W < 16
        assert bool(((bg_c == 0) == (bg_d == 0)).all())
    # the seams of the 64 x 16 tile are crossed in both directions, from a set pixel 6 away, and not from 7
    _, _, ob_c, _ = sc.compose_layers((33, 130))
    rows, cols = np.nonzero(np.all(sr.unpack_colour(ob_c[0]) > 0, axis=2))
    assert any(c < 64 <= c + sc.HALO for c in cols) and any(c - sc.HALO < 64 <= c for c in cols)
    assert any(r < 16 <= r + sc.HALO for r in rows) and any(r - sc.HALO < 16 <= r for r in rows)


def test_compose_frame_writes_one_frame_and_nothing_else():
    hw = (5, 3)
    H, W = hw
    bg_c, bg_d, ob_c, ob_d = sc.compose_layers(hw)
    T, stride = 3, 3 * 3 * H * W + 24
    for t in range(T):
        sparse, sdepth = np.full(2 * stride, F(7)), np.full(2 * stride, F(9))
        rgb, depth, mask = sr.compose_frame(sparse, sdepth, stride, T, t, bg_c, bg_d, ob_c, ob_d)
        for p in range(2):
            rgb_m, depth_m, m = sr.merge(sr.unpack_colour(bg_c[p]), bg_d[p], sr.unpack_colour(ob_c[p]), ob_d[p])
            a, b = sr.conditions(rgb_m, depth_m)
            got = sparse[p * stride:p * stride + 3 * T * H * W].reshape(3, T, H, W)
            assert np.array_equal(got[:, t], a) and bool((np.delete(got, t, axis=1) == 7).all())
            got = sdepth[p * stride:p * stride + 3 * T * H * W].reshape(3, T, H, W)
            assert np.array_equal(got[:, t], b) and bool((np.delete(got, t, axis=1) == 9).all())
            assert np.array_equal(rgb[p], rgb_m) and np.array_equal(depth[p], depth_m) and np.array_equal(mask[p], m.astype(np.uint8))
            assert bool((sparse[p * stride + 3 * T * H * W:(p + 1) * stride] == 7).all())
    rgb, depth, mask = sr.compose_frame(sparse, sdepth, stride, T, 0, bg_c, bg_d)
    assert not mask.any() and np.array_equal(rgb, sr.unpack_colour(bg_c)) and np.array_equal(depth, bg_d)


def test_every_refusal_names_an_entry_point_and_a_message():
    assert {r[0] for r in sc.REFUSALS} == {"points", "resolve", "compose"}
    assert len({r[:2] for r in sc.REFUSALS}) == len(sc.REFUSALS) and all(r[2] and r[3] for r in sc.REFUSALS)
    src = open(os.path.join(ROOT, "mudg_amd", "csrc", "splat.hip")).read()
    entry = src[src.index('extern "C"'):]
    assert entry.count("MUDG_REQUIRE") == 14                                             # a new clause needs a case here
    for piece in {r[3] for r in sc.REFUSALS}:
        assert piece in entry, piece
