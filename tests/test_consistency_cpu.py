"""What the cross-view consistency rule can show without a GPU: the CPU definition (tests/consistency_reference.py) on an
analytic scene whose answers are known, the rule's details, the host pieces of mudg_amd/depth.py, and the C-ABI and generated code of
csrc/consistency.hip."""
import os
import re

import numpy as np
import pytest
import torch

import consistency_reference as cr
import depth_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
HW = (24, 32)
ENTRIES = (("mudg_view_flags", 11), ("mudg_view_consistency", 20))
RULE = cr.DEFAULTS


def _tables(c2w, hw=HW):
    from mudg_amd import depth
    source = depth.camera_table(cr.SCENE_INTR, c2w, hw, hw)
    return source, depth.witness_table(c2w, source)


@pytest.fixture(scope="module")
def scene():
    """3 frames x 2 poses of the ground and the wall with the default witness lists and the definition's answer on the clean maps."""
    from mudg_amd import depth
    z, c2w, times, poses = cr.scene_views(HW)
    source, witness = _tables(c2w)
    lists = depth.default_witnesses(times, poses, reach=2)
    return {"depth": z, "c2w": c2w, "times": times, "poses": poses, "source": source, "witness": witness, "lists": lists,
            "clean": cr.consistency(z, None, source, witness, times, lists)}


def _seen(scene, s, w, depth_s):
    """Independently of the rule's arithmetic (4 x 4 matrices, numpy's inverse): where view s's pixels, lifted with depth_s, land in view
    w — (inside the image by a margin, pixel row, pixel column, depth in w)."""
    H, W = HW
    k = cr.SCENE_INTR
    xn = ((np.arange(W) + 0.5) - k[0, 2]) / k[0, 0]
    yn = ((np.arange(H) + 0.5) - k[1, 2]) / k[1, 1]
    cam = np.stack(np.broadcast_arrays(xn[None, :] * depth_s, yn[:, None] * depth_s, depth_s, np.ones(HW)), axis=-1)
    q = cam @ scene["c2w"][s].T @ np.linalg.inv(scene["c2w"][w]).T
    u, v = k[0, 0] * q[..., 0] / q[..., 2] + k[0, 2], k[1, 1] * q[..., 1] / q[..., 2] + k[1, 2]
    eps = 1e-6
    inside = (q[..., 2] > 1e-3) & (u > eps) & (u < W - eps) & (v > eps) & (v < H - eps)
    return inside, np.where(inside, v, 0).astype(int), np.where(inside, u, 0).astype(int), q[..., 2]


# ------------------------------------------------------------------------------------------------ the analytic scene
def test_clean_views_keep_every_pixel_that_enough_witnesses_can_see(scene):
    """The scene has no occlusion (a floor and a facing wall seen from above the floor, in front of the wall), so a witness can see a pixel's
    point iff it projects inside the witness's image.  First the scene's own condition: at every such projection the witness's pixel that
    holds it has a true depth within the rule's tolerance of the point's depth — so the rule must agree already at r = 0."""
    z, V = scene["depth"].astype(D), len(scene["depth"])
    assert z.min() > 5 and z.max() < 13 and (z < 11).any()                                                   # both surfaces are in view
    can_see = np.zeros((V,) + HW, dtype=int)
    worst = 0.0
    for s in range(V):
        for w in scene["lists"][s]:
            if w < 0:
                continue
            inside, jw, iw, qz = _seen(scene, s, w, z[s])
            gap = np.abs(z[w][jw, iw] - qz)[inside]
            tol = (RULE["abs_tol"] + RULE["rel_tol"] * qz)[inside]
            worst = max(worst, float((gap / tol).max()))
            can_see[s] += inside
    print(f"worst |true depth of the witness pixel - depth of the point| / tolerance = {worst:.3f}")
    assert worst < 0.9                                                                                       # the scene satisfies the condition
    for r in (0, 1, 2):
        got = cr.consistency(scene["depth"], None, scene["source"], scene["witness"], scene["times"], scene["lists"], **dict(RULE, r=r))
        assert got["flags"].min() == 1 and got["violate"].max() == 0
        assert np.all(got["agree"] >= can_see), r
        assert np.all(got["keep"][can_see >= RULE["min_agree"]] == 1), r
    enough = can_see >= RULE["min_agree"]
    assert 0.8 < enough.mean() <= 1.0
    assert scene["clean"]["stats"][:, 0].tolist() == [HW[0] * HW[1]] * V


def _planted(scene, factor):
    """View 0 with a 3 x 3 patch of the wall at `factor` times its true depth, and the definition's answer."""
    z = scene["depth"].copy()
    patch = (slice(6, 9), slice(25, 28))
    assert np.all(cr.scene_depth(scene["c2w"][0], HW)[patch] == 12.0)                                        # the wall, to the right of the middle: in front of both poses
    z[0][patch] = (z[0][patch].astype(D) * factor).astype(F)
    return z, patch, cr.consistency(z, None, scene["source"], scene["witness"], scene["times"], scene["lists"])


def test_a_floater_is_seen_through_and_dropped(scene):
    z, patch, got = _planted(scene, 0.5)
    lists = scene["lists"][0]
    expected = np.zeros((3, 3), dtype=int)
    for w in lists[lists >= 0]:
        inside, jw, iw, qz = _seen(scene, 0, w, z[0].astype(D))
        for a, j in enumerate(range(6, 9)):
            for b, i in enumerate(range(25, 28)):
                if not inside[j, i]:
                    continue
                window = z[w][max(jw[j, i] - 1, 0):jw[j, i] + 2, max(iw[j, i] - 1, 0):iw[j, i] + 2].astype(D)
                tol = RULE["abs_tol"] + RULE["rel_tol"] * qz[j, i]
                assert np.all(window > qz[j, i] + 2 * tol)                                                   # only background, well behind
                expected[a, b] += 1
    assert expected.min() >= 3                                                                               # most witnesses look at the patch
    assert np.array_equal(got["violate"][0][patch], expected) and np.all(got["agree"][0][patch] == 0) and np.all(got["keep"][0][patch] == 0)
    # nothing else is accused: the floater hides points of other views (no evidence), it is never seen through by them
    others = np.ones(z.shape, dtype=bool)
    others[0][patch] = False
    assert got["violate"][others].max() == 0
    assert np.all(got["keep"][others] >= (scene["clean"]["agree"][others] >= RULE["min_agree"] + 1))         # at most one witness was lost
    assert got["stats"][0, 4] == expected.sum() and got["stats"][0, 5] == 9 and got["stats"][1:, 4:].max() == 0


def test_a_patch_behind_the_wall_gets_no_evidence_never_a_violation(scene):
    z, patch, got = _planted(scene, 1.5)
    assert np.all(z[0][patch] == 18.0)
    assert np.all(got["violate"][0][patch] == 0) and np.all(got["agree"][0][patch] == 0) and np.all(got["keep"][0][patch] == 0)
    # The rule's known false accusation, bounded here: a correct wall point of another view whose whole window in view 0 lies inside the
    # 3 x 3 patch — so whose projection falls in the patch's one centre pixel — sees only the too-far depths and counts as seen through by
    # view 0: one verdict each.  A view up to 1 m nearer the wall has pixels 11 / 12 the size of view 0's, so at most 2 x 2 of them.
    others = np.ones(z.shape, dtype=bool)
    others[0][patch] = False
    assert got["violate"][others].max() <= 1 and got["stats"][0, 4] == 0 and all(int(n) <= 4 for n in got["stats"][1:, 4])


# ------------------------------------------------------------------------------------------------ the rule's details
def test_a_dynamic_pixel_is_tested_only_against_views_of_its_own_time(scene):
    labels = np.zeros(scene["depth"].shape, dtype=np.int64)
    labels[0, 4:20, 8:24] = 13                                                                               # a car in view 0 (frame 0, pose 0)
    args = (scene["source"], scene["witness"], scene["times"])
    got = cr.consistency(scene["depth"], labels, *args, scene["lists"])
    assert np.all(got["flags"][0, 4:20, 8:24] == 3) and np.all(got["flags"][1:] == 1)
    same_time = np.where(scene["times"][np.maximum(scene["lists"], 0)] == scene["times"][:, None], scene["lists"], -1)
    assert (same_time[0] >= 0).sum() == 1 and same_time[0][0] == 3                                           # the other pose of frame 0
    restricted = cr.consistency(scene["depth"], labels, *args, same_time)
    car = labels[0] == 13
    for name in ("agree", "violate"):
        assert np.array_equal(got[name][0][car], restricted[name][0][car]), name
    assert got["agree"][0][car].max() == 1 and got["keep"][0][car].max() == 0                                # one witness: below min_agree = 2
    assert np.array_equal(got["agree"][0][~car], scene["clean"]["agree"][0][~car])                           # static pixels: every witness


def test_repeated_time_ids_with_the_default_lists_keep_the_witnesses_of_the_own_frame(scene):
    """consistent_views' default when times are given: default_witnesses(times) — a dynamic pixel is judged by the other view of its frame."""
    from mudg_amd import depth
    lists = depth.default_witnesses(scene["times"])
    assert np.array_equal(lists, scene["lists"])                                                             # here one view per (frame, pose)
    labels = np.zeros(scene["depth"].shape, dtype=np.int64)
    labels[0, 4:20, 8:24] = 13
    got = cr.consistency(scene["depth"], labels, scene["source"], scene["witness"], scene["times"], lists)
    car = labels[0] == 13
    assert got["agree"][0][car].max() == 1 and got["stats"][0, 1] == HW[0] * HW[1] - int((got["agree"][0] == 0).sum())
    zeros = depth.default_witnesses(scene["times"], np.zeros(6, int))                                        # one pose id for all: no such witness
    assert not cr.consistency(scene["depth"], labels, scene["source"], scene["witness"], scene["times"], zeros)["agree"][0][car].any()


def test_a_dynamic_pixel_is_not_counted_by_views_of_another_time(scene):
    labels = np.zeros(scene["depth"].shape, dtype=np.int64)
    labels[3] = 13                                                                                           # all of view 3 (frame 0, pose 1)
    args = (scene["source"], scene["witness"], scene["times"])
    only3 = np.full((6, 1), 3, dtype=np.int32)
    got = cr.consistency(scene["depth"], labels, *args, only3, **dict(RULE, min_agree=1))
    static = cr.consistency(scene["depth"], None, *args, only3, **dict(RULE, min_agree=1))
    assert scene["times"].tolist() == [0, 1, 2, 0, 1, 2]
    assert static["agree"][[1, 2, 4, 5]].sum() > 1000                                                        # without the tag view 3 confirms them
    assert got["agree"][[1, 2, 4, 5]].max() == 0 and got["violate"].max() == 0                               # with it: no evidence at other times
    assert np.array_equal(got["agree"][0], static["agree"][0]) and got["agree"][0].sum() > 500               # frame 0's other pose still counts it
    assert got["agree"][3].max() == 0                                                                        # the view itself is skipped


def test_labels_decide_sky_and_the_dynamic_bit():
    z = np.full((1, 2, 8), 5.0, dtype=F)
    z[0, 1] = [0.0, np.nan, 100.0, np.nextafter(F(100.0), F(0)), -1.0, np.inf, 1e-30, 50.0]
    labels = np.array([[[10, 11, 18, 19, 63, 64, -1, 0], [0] * 8]], dtype=np.int64)
    assert cr.flags(z, labels)[0].tolist() == [[0, 3, 3, 1, 1, 1, 1, 1], [0, 0, 0, 1, 0, 0, 1, 1]]
    assert cr.flags(z, labels, dynamic_mask=(1 << 63) | 1)[0, 0].tolist() == [0, 1, 1, 1, 3, 1, 1, 3]
    assert cr.flags(z)[0].tolist() == [[1] * 8, [0, 0, 0, 1, 0, 0, 1, 1]]                                    # no labels: no sky, nothing dynamic
    assert cr.flags(z, labels, sky_label=-1)[0, 0].tolist() == [1, 3, 3, 1, 1, 1, 0, 1]


def test_the_statistics_equal_a_brute_force_count_in_python_integers(scene):
    z, _, got = _planted(scene, 0.5)
    for s in range(len(z)):
        count = [0] * 6
        for j in range(HW[0]):
            for i in range(HW[1]):
                a, b, k, f = (int(got[name][s, j, i]) for name in ("agree", "violate", "keep", "flags"))
                assert k == int(bool(f & 1) and a >= RULE["min_agree"] and b <= RULE["max_violate"])
                for n, add in enumerate((f & 1, int(a + b > 0), k, a, b, int(b > 0))):
                    count[n] += add
        assert got["stats"][s].tolist() == count, s
    per_view, overall = cr.scores(got["stats"])
    assert per_view[0]["violated"] == 9 / (HW[0] * HW[1]) and 0 < overall["kept"] < 1 and overall["mean_agree"] > 2


def test_the_score_is_the_ratio_of_the_integer_counts():
    from mudg_amd import hip, metrics
    with pytest.raises(hip.MudgError, match="on the GPU"):
        metrics.view_consistency({"stats": torch.zeros(2, 6, dtype=torch.int64)})
    per_view, overall = cr.scores(np.array([[10, 8, 4, 20, 3, 2], [0, 0, 0, 0, 0, 0]]))
    assert per_view[0] == {"tested": 0.8, "kept": 0.4, "violated": 0.2, "mean_agree": 2.5} and all(np.isnan(v) for v in per_view[1].values())
    assert overall == per_view[0]


def test_default_witnesses_order_and_padding():
    from mudg_amd import depth, hip
    times, poses = [0, 1, 2, 3, 0, 1, 2, 3], [0, 0, 0, 0, 1, 1, 1, 1]
    got = depth.default_witnesses(times, poses, reach=1)
    assert got.dtype == np.int32 and got.tolist() == [[4, 1, 5, -1, -1], [5, 0, 2, 4, 6], [6, 1, 3, 5, 7], [7, 2, 6, -1, -1],
                                                      [0, 1, 5, -1, -1], [1, 0, 2, 4, 6], [2, 1, 3, 5, 7], [3, 2, 6, -1, -1]]
    assert depth.default_witnesses(times, poses, reach=0).tolist() == [[4], [5], [6], [7], [0], [1], [2], [3]]
    assert depth.default_witnesses([5], [0]).tolist() == [[-1]]                                              # a single view: one empty column
    assert depth.default_witnesses(np.arange(4), np.zeros(4, int), reach=2).tolist() == [[1, 2, -1], [0, 2, 3], [0, 1, 3], [1, 2, -1]]
    full = depth.default_witnesses(np.repeat(np.arange(16), 3), np.tile(np.arange(3), 16))                   # 16 frames x 3 poses, reach 2
    assert full.shape == (48, 14) and (full[24] >= 0).all() and (full[0] >= 0).sum() == 8 and 0 not in full[0]
    # no pose ids: every view is a pose of its own, so views that share a time id witness each other (consistent_views' default)
    assert depth.default_witnesses([0, 0, 1, 1]).tolist() == [[1, 2, 3], [0, 2, 3], [3, 0, 1], [2, 0, 1]]
    assert depth.default_witnesses([0, 0, 1, 1], None, reach=0).tolist() == [[1], [0], [3], [2]]
    assert depth.default_witnesses([0, 0, 5, 5]).tolist() == [[1], [0], [3], [2]]
    assert np.array_equal(depth.default_witnesses(np.arange(4)), depth.default_witnesses(np.arange(4), np.zeros(4, int)))
    with pytest.raises(hip.MudgError, match="at most 64"):
        depth.default_witnesses(np.zeros(66, int), np.arange(66))
    with pytest.raises(hip.MudgError, match="default_witnesses"):
        depth.default_witnesses([0.5, 1.0], [0, 0])


def test_the_witness_table_is_the_rigid_inverse_and_the_source_intrinsics(scene):
    from mudg_amd import cloud, depth
    source, witness = scene["source"], scene["witness"]
    assert witness.dtype == D and witness.shape == (6, 16) and np.array_equal(witness[:, 12:], source[:, 12:])
    for v in range(6):
        assert np.array_equal(witness[v, :12].reshape(3, 4), cloud.inverse_rigid(scene["c2w"][v]))
        both = np.vstack([witness[v, :12].reshape(3, 4), [0, 0, 0, 1]]) @ scene["c2w"][v]
        assert np.abs(both - np.eye(4)).max() < 1e-12
    assert depth.witness_table(scene["c2w"]).shape == (6, 12)


def test_keep_selects_a_subsequence_of_the_lifted_points(scene):
    """lift_views' rule: points[valid] without keep, points[valid & keep != 0] with it — the same points in the same order, fewer."""
    z, patch, got = _planted(scene, 0.5)
    z[0, 0, :3] = [0.0, 100.0, np.nan]
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, HW + (3,), dtype=np.uint8)
    packed, valid = dr.unproject(z[0], rgb, scene["source"][0])
    keep = got["keep"][0].reshape(-1).copy()
    keep[:3] = 1                                                                                             # keep does not revive what is not valid
    plain, kept = packed[valid == 1], packed[(valid == 1) & (keep != 0)]
    assert 0 < len(kept) < len(plain) == HW[0] * HW[1] - 3
    index = np.flatnonzero(keep[valid == 1] != 0)
    assert np.all(np.diff(index) > 0) and np.array_equal(plain[index], kept)


# ------------------------------------------------------------------------------------------------ the interface off the GPU
def test_inputs_off_the_gpu_raise():
    from mudg_amd import depth, hip, ops
    z, rgb = torch.zeros(2, 8, 8), torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    cams = np.stack([np.eye(4)] * 2)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        depth.consistent_views(z, np.eye(3), cams, (8, 8))
    with pytest.raises(hip.MudgError, match="on the GPU"):
        depth.fuse_views(z, rgb, np.eye(3), cams, (8, 8))
    with pytest.raises(hip.MudgError, match="on the GPU"):
        depth.lift_views(z, rgb, np.eye(3), cams, (8, 8), keep=torch.ones(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(hip.MudgError, match="on the GPU"):
        ops.view_flags(z)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        ops.view_consistency(z, z.to(torch.uint8), torch.zeros(2, 16, dtype=torch.float64), torch.zeros(2, 16, dtype=torch.float64), [0, 1], [[1], [0]])


def test_the_host_rejects_witness_ids_outside_the_view_set():
    from mudg_amd import hip, ops
    times, lists = ops.view_witness_lists([3, 4, 5], [[1, 2, -1], [0, 1, -1], [-1, -1, -1]], 3)
    assert times.dtype == np.int32 and lists.dtype == np.int32 and lists.shape == (3, 3)
    for bad in ([[1], [2], [3]], [[1], [-2], [0]]):
        with pytest.raises(hip.MudgError, match="witness ids"):
            ops.view_witness_lists([0, 1, 2], bad, 3)
    with pytest.raises(hip.MudgError, match="view_consistency"):
        ops.view_witness_lists([0, 1, 2], np.zeros((3, 65), dtype=np.int32), 3)
    with pytest.raises(hip.MudgError, match="view_consistency"):
        ops.view_witness_lists([0, 1], [[0], [1], [2]], 3)
    with pytest.raises(hip.MudgError, match="host arrays"):
        ops.view_witness_lists(torch.zeros(3, dtype=torch.int32), [[0], [1], [2]], 3)


def test_the_product_does_not_import_the_cpu_definition():
    for d in ("mudg_amd", "lvdm", "utils", "virtual_render", "tools", "main"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith(".py"):
                    assert "import consistency_reference" not in open(os.path.join(base, f)).read(), f


# ------------------------------------------------------------------------------------------------ C-ABI and generated code
def test_consistency_entry_points_are_declared_bound_and_exported():
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
    assert "consistency.hip" in build.SOURCES


def test_consistency_entry_points_reject_bad_arguments():
    from mudg_amd import hip
    lib = hip.lib()
    one = 16                                                                         # never dereferenced: every call below is rejected first
    mask = cr.DYNAMIC_MASK
    assert lib.mudg_view_flags(None, None, 10, mask, 1, 8, 8, 0.0, 100.0, None, None) == -1 and b"null" in lib.mudg_last_error()
    assert lib.mudg_view_flags(one, None, 10, mask, 1, 8, 8, 0.0, 100.0, None, None) == -1
    assert lib.mudg_view_flags(one, None, 10, mask, 0, 8, 8, 0.0, 100.0, one, None) == -1
    assert lib.mudg_view_flags(one, None, 10, mask, 65536, 8, 8, 0.0, 100.0, one, None) == -1
    assert lib.mudg_view_flags(one, None, 10, mask, 1, 4097, 4096, 0.0, 100.0, one, None) == -1 and b"2^24" in lib.mudg_last_error()

    def call(V=2, N=1, H=8, W=8, r=1, min_agree=2, max_violate=0, rel_tol=0.02, abs_tol=0.2, pointers=(one,) * 10):
        p = pointers
        return lib.mudg_view_consistency(p[0], p[1], p[2], p[3], p[4], p[5], V, N, H, W, r, min_agree, max_violate, rel_tol, abs_tol, p[6], p[7], p[8], p[9], None)
    for k in range(10):                                                              # each of the ten pointers
        assert call(pointers=tuple(None if n == k else one for n in range(10))) == -1 and b"null" in lib.mudg_last_error(), k
    for bad, word in ((dict(V=0), b"views"), (dict(V=65536), b"views"), (dict(H=4097, W=4096), b"2^24"), (dict(N=0), b"witnesses"), (dict(N=65), b"witnesses"),
                      (dict(r=3), b"radius"), (dict(r=-1), b"radius"), (dict(rel_tol=-0.01), b"tolerances"), (dict(abs_tol=-1.0), b"tolerances"),
                      (dict(abs_tol=float("nan")), b"tolerances"), (dict(min_agree=-1), b"min_agree")):
        assert call(**bad) == -1 and word in lib.mudg_last_error(), bad


def test_consistency_kernels_use_no_scratch_and_no_compare_and_swap(tmp_path):
    """Facts about the generated gfx950 code that do not depend on the compiler's scheduling."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "consistency.s"
    subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S",
                    os.path.join(ROOT, "mudg_amd", "csrc", "consistency.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    s = out.read_text()
    md = s[s.index("amdhsa.kernels"):]
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", md, re.S):
        for family in ("view_flags_kernel", "view_consistency_kernel"):
            if family in m.group(1):
                seen[family] = seen.get(family, 0) + 1
                assert int(m.group(2)) == 0, m.groups()
    assert seen == {"view_flags_kernel": 2, "view_consistency_kernel": 1}, seen
    assert "cmpswap" not in s
