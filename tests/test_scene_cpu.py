"""What the GPU tests of the scene kernels (tests/test_scene_kernels_gpu.py) rest on, checked without a GPU: the entry-point level
definitions of tests/scene_raw_reference.py equal the existing definitions on well-formed input, their extra rules (sums added to a
start, slots left unwritten, spoiled table entries dropped) hold by hand, and every case of tests/scene_cases.py reaches the clause of
the kernel it names: a case that stops reaching it fails here, before any GPU run."""
import os

import numpy as np

import cloud_reference as cr
import consistency_reference as vr
import depth_reference as dr
import metrics_reference as mr
import neighbours_reference as nr
import scene_cases as sc
import scene_raw_reference as raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64


def _zeros(*shape):
    return np.zeros(shape, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ raw definitions = the existing ones
def test_raw_depth_definitions_equal_the_existing_ones_on_well_formed_input():
    c = sc.pixel_case((5, 7))
    whole = dr.metric_depth(c["frames"], c["lidar"], c["labels"], sc.SKY)
    sums = raw.align_sums(c["frames"], c["lidar"], _zeros(2, 5))
    assert sums.tolist() == [list(s) for s in whole["sums"]]
    coef, fitted = raw.align_solve(sums)
    assert np.array_equal(coef, whole["coef"]) and np.array_equal(fitted, whole["fitted"]) and fitted.all()
    depth, vis = raw.finish(c["frames"], coef, c["labels"], sc.SKY)
    assert np.array_equal(depth.view(np.uint32), whole["depth"].view(np.uint32)) and np.array_equal(vis, whole["vis"])
    start = sc.start_sums((2, 5), 1)
    assert (raw.align_sums(c["frames"], c["lidar"], start) - start).tolist() == sums.tolist()           # added, not stored
    assert raw.added(np.array([2 ** 64 - 1], dtype=np.uint64), [3]).tolist() == [2]                    # modulo 2^64
    pts, valid = raw.unproject(c["depth"], c["frames"], c["table"], c["labels"], sc.SKY)
    for f in range(2):
        p, v = dr.unproject(c["depth"][f], c["frames"][f], c["table"][f], c["labels"][f], sc.SKY)
        assert np.array_equal(pts[35 * f:35 * f + 35], p) and np.array_equal(valid[35 * f:35 * f + 35], v)
    x = sc.colormap_case(257, (0.0, 1.0))["values"]
    b, col = raw.colormap(x, 0.0, 1.0, True)
    assert np.array_equal(b, dr.colormap(x, reversed=True)) and np.array_equal(b, dr.to_bytes(col))


def test_raw_view_definition_equals_the_existing_one_on_well_formed_input():
    c = sc.view_case((16, 16), 64, "near")
    rng = np.random.default_rng(0)
    labels = rng.integers(0, 19, c["depth"].shape)
    witnesses = np.where((c["witnesses"] >= c["V"]), -1, c["witnesses"])                                # what the existing definition admits
    wit = np.array(c["wit"])
    wit[3:] = wit[:2]                                                                                   # finite rows
    p = dict(r=1, min_agree=2, max_violate=0, rel_tol=0.02, abs_tol=0.2)
    want = vr.consistency(c["depth"], labels, c["src"], wit, c["times"], witnesses, **p)
    agree, violate, keep, stats = raw.view_consistency(c["depth"], want["flags"], c["src"], wit, c["times"], witnesses, _zeros(5, 6), **p)
    assert np.array_equal(raw.view_flags(c["depth"], labels), want["flags"])
    assert np.array_equal(agree, want["agree"]) and np.array_equal(violate, want["violate"]) and np.array_equal(keep, want["keep"])
    assert np.array_equal(stats.astype(np.int64), want["stats"]) and want["agree"].any() and want["violate"].any()
    # the spoiled ids are the same as an empty entry, and so is the view's own id
    again = raw.view_consistency(c["depth"], want["flags"], c["src"], wit, c["times"], sc.view_case((16, 16), 64, "wild")["witnesses"], _zeros(5, 6), **p)
    same = np.where(raw.kept_witnesses(sc.view_case((16, 16), 64, "wild")["witnesses"], 5), sc.view_case((16, 16), 64, "wild")["witnesses"], -1)
    other = vr.consistency(c["depth"], labels, c["src"], wit, c["times"], same, **p)
    assert np.array_equal(again[0], other["agree"]) and np.array_equal(again[3].astype(np.int64), other["stats"])


def test_raw_metric_definitions_equal_the_existing_ones_on_well_formed_input():
    c = sc.ssim_case((12, 43))
    whole = mr.psnr_ssim(c["a"], c["b"])
    assert np.array_equal(raw.metric_sse(c["a"], c["b"], _zeros(2)).astype(np.int64), whole["sse"])
    assert np.array_equal(raw.metric_ssim(c["a"], c["b"], _zeros(2)).view(np.int64), whole["ssim_sum"])
    start = np.array([2 ** 64 - 5, 7], dtype=np.uint64)                                                # a signed sum added to a negative start
    assert np.array_equal(raw.metric_ssim(c["a"], c["b"], start).view(np.int64), whole["ssim_sum"] + np.array([-5, 7]))
    p = sc.pixel_case((37, 53))
    got = raw.metric_depth(p["depth"], p["lidar"], _zeros(2, 8), 0.1, 80.0)
    assert np.array_equal(got.astype(np.int64), mr.depth_errors(p["depth"], p["lidar"])["sums"])
    k = sc.confusion_case((17, 241), 19)
    scores = mr.segmentation_scores(k["pred"].reshape(2, 17, 241), k["gt"].reshape(2, 17, 241), 19)
    m, bad = raw.metric_confusion(k["pred"], k["gt"], 19, _zeros(2, 19, 19), _zeros(2))
    assert np.array_equal(m.astype(np.int64), scores["confusion"]) and np.array_equal(bad.astype(np.int64), scores["bad"])


def test_raw_search_definitions_equal_the_existing_ones_on_well_formed_input():
    c = sc.search_case(257)
    assert np.array_equal(c["ref_sorted"], c["ref"][c["order"]]) and bool((np.diff(c["keys"]) >= 0).all())
    order, first, last = nr.walk_intervals(c["ref"], c["queries"], sc.SEARCH_R)
    assert np.array_equal(order, c["order"]) and c["cell"] == float(nr.cell_edge(sc.SEARCH_R))
    d2, index, owned = raw.cloud_nearest(c["ref_sorted"], c["order"], c["queries"], None, sc.SEARCH_R)
    want_d2, want_index = nr.nearest(c["ref"], c["queries"], sc.SEARCH_R)
    assert np.array_equal(d2, want_d2) and np.array_equal(index, want_index) and owned.all()
    assert np.array_equal(index, nr.walk_nearest(c["ref"], c["queries"], sc.SEARCH_R)[1])
    for cap in (1, sc.BIG_CAP):
        counts, _ = raw.cloud_count(c["ref_sorted"], c["queries"], None, sc.SEARCH_R, cap)
        assert np.array_equal(counts, nr.counts(c["ref"], c["queries"], sc.SEARCH_R, cap)) and np.array_equal(counts, nr.walk_counts(c["ref"], c["queries"], sc.SEARCH_R, cap))
    m = sc.cloud_metric_case(2049)
    assert raw.metric_cloud(m["d2"], sc.CLOUD_T2, sc.CLOUD_R2, _zeros(10)).tolist() == nr.cloud_sums(m["d2"], sc.CLOUD_T2, sc.CLOUD_R2)


def test_raw_cloud_definitions_equal_the_existing_ones_on_well_formed_input():
    c = sc.sweep_case("whole")
    packed, labels, written, dropped, refused = raw.cloud_sweep(c["rays_o"], c["rays_d"], c["ranges"], c["offsets"], c["total"], c["max_rays"], c["l2w"],
                                                                c["cams"], c["objs"], c["images"], c["image_bytes"])
    assert written.all() and dropped == 0 and refused == 0
    for f in range(3):
        a, b = int(c["offsets"][f]), int(c["offsets"][f + 1])
        cams = [(w2c, K, c["images"][base:base + 3 * h * w].reshape(h, w, 3)) for w2c, K, h, w, base in c["cams"][f]]
        xyz, rgb, lab = cr.sweep(c["rays_o"][a:b], c["rays_d"][a:b], c["ranges"][a:b], c["l2w"][f], cams, c["objs"][f])
        assert np.array_equal(packed[a:b], cr.pack(xyz, rgb)) and np.array_equal(labels[a:b], lab)
    assert {-1, 0, 1, 2} <= set(labels.tolist())
    v = sc.voxel_case(257)
    assert np.array_equal(raw.voxel_keys(v["xyz"], sc.VOXEL), cr.voxel_keys(cr.voxel_indices(v["xyz"], sc.VOXEL)))
    sums, dropped = raw.voxel_reduce(v["packed"], v["order"], v["segments"], sc.VOXEL, _zeros(v["voxels"], 8))
    out = raw.voxel_finish(sums, sc.VOXEL)
    xyz, rgb = cr.voxel_downsample(v["xyz"], v["rgb"], sc.VOXEL)
    assert dropped == 0 and np.array_equal(out[:-1], cr.pack(xyz, rgb)) and not out[-1].any() and not sums[-1].any()
    assert sums[:, 0].tolist() == list(v["runs"]) + [0]


# ------------------------------------------------------------------------------------------------ the cases reach their clauses
def test_pixel_cases_reach_both_forms_and_their_partial_workgroups():
    assert [sc.lanes(hw, hw[1] % 4 == 0) for hw in sc.PIXEL_SIZES] == [(3, 3), (258, 2), (35, 35), (1961, 169)]
    assert sc.ALIGNED_SIZE in sc.PIXEL_SIZES and sc.ALIGNED_SIZE[1] % 4 == 0
    for hw in sc.PIXEL_SIZES:
        c = sc.pixel_case(hw)
        n = hw[0] * hw[1]
        assert c["clause"] and n <= 2000
        for f in range(2):
            k = dr.k_of(c["frames"][f]).reshape(-1)
            use = dr.counted(k, c["lidar"][f].reshape(-1))
            assert use[0] and use[n - 1] and 0 < use.sum() < n                                       # dropping the first or the last lane shows
            y, z = c["lidar"][f].reshape(-1), c["depth"][f].reshape(-1)
            assert 0.1 < y[n - 1] < 80 and (c["frames"][f].reshape(-1, 3)[n - 1] != c["other"][f].reshape(-1, 3)[n - 1]).any()
            fl = vr.flags(z, c["labels"][f].reshape(-1), sc.SKY, sc.DYNAMIC_MASK)
            assert fl[0] == 3 and fl[n - 1] == 3 and {0, 1, 2, 3} <= set(fl.tolist())
            q = dr.q_of(y[1:8])
            assert q[4] == 0 and q[5] == 2 and not use[1:5].any() and not use[7]                     # half to even, and the four that are not counted
            lab = c["labels"][f].reshape(-1)[3:11]
            assert vr.flags(np.full(8, 5, F), lab, sc.SKY, sc.DYNAMIC_MASK).tolist() == [1, 1, 1, 1, 0, 3, 3, 1]
        depth, _ = raw.finish(c["frames"], c["coef"], c["labels"], sc.SKY)
        assert (depth == 0).any() and (depth == 100).any() and ((depth > 0) & (depth < 100)).any()
        _, valid = raw.unproject(c["depth"], c["frames"], c["table"], c["labels"], sc.SKY)
        assert valid[0] and valid[-1] and 0 < valid.sum() < len(valid)
        sums = raw.metric_depth(c["depth"], c["lidar"], _zeros(2, 8), 0.1, 80.0)
        assert (sums[:, :7] > 0).all() and not sums[:, 7].any()


def test_solve_cases_hold_every_kind_of_row():
    for frames in sc.SOLVE_FRAMES:
        c = sc.solve_case(frames)
        coef, fitted = raw.align_solve(c["sums"])
        assert len(coef) == frames and c["kinds"][0] == "headroom" and c["kinds"][-1] == "headroom"
        for f, kind in enumerate(c["kinds"]):
            assert fitted[f] == (kind in ("headroom", "fitted")), (frames, f, kind)
            if not fitted[f]:
                assert coef[f].tolist() == [100.0, 0.0]
        if frames > 1:
            assert {"empty", "one pixel", "no spread", "fitted"} <= set(c["kinds"])
    n, sk, skk, sq, skq = sc.HEADROOM_ROW
    assert n == 2 ** 24 and skq > 2 ** 53 and float(skq) != skq - 1 and skq < 2 ** 62 and sq == 2 ** 51        # the conversion to fp64 rounds


def test_colormap_cases_stand_on_the_knots():
    knots = sc.knot_values()
    assert len(knots) == 11 and knots[10] == 1.0 and all(F(k) * F(10) == F(i) for i, k in enumerate(knots))
    c = sc.colormap_case(257, (0.0, 1.0))
    assert np.array_equal(c["values"][:11], knots) and np.isnan(c["values"][11]) and np.isinf(c["values"][12:14]).all()
    col = dr.colormap(c["values"], bytes=False)
    assert np.array_equal(col[:11], dr.SPECTRAL) and np.array_equal(col[11], dr.SPECTRAL[0]) and np.array_equal(col[12], dr.SPECTRAL[10])
    assert np.array_equal(dr.colormap(c["values"], reversed=True, bytes=False)[:11], dr.SPECTRAL[::-1])
    r = sc.colormap_case(257, (2.0, 50.0))
    assert r["val_min"] == 2.0 and not np.array_equal(dr.colormap(r["values"], 2.0, 50.0), dr.colormap(r["values"]))
    assert len(sc.colormap_case(1, (0.0, 1.0))["values"]) == 1


def test_ssim_cases_have_the_tiles_they_name():
    for hw in sc.SSIM_SIZES:
        H, W = hw
        ty, tx = -(-(H - 10) // 32), -(-(W - 10) // 32)
        assert (ty, tx, (W - 10) - 32 * (tx - 1)) == sc.SSIM_TILES[hw]
        c = sc.ssim_case(hw)
        q = mr.ssim_q(c["a"][1, :, :, 2], c["b"][1, :, :, 2])
        assert bool((q == 2 ** 32).all()) and mr.ssim_sum(c["a"][0], c["b"][0]) != 0


def test_confusion_cases_hold_the_wild_labels():
    assert [h * w for h, w in sc.CONFUSION_SIZES] == [1, 4096, 4097]
    for hw in sc.CONFUSION_SIZES:
        for classes in sc.CONFUSION_CLASSES:
            c = sc.confusion_case(hw, classes)
            m, bad = raw.metric_confusion(c["pred"], c["gt"], classes, _zeros(2, classes, classes), _zeros(2))
            n = hw[0] * hw[1]
            if n > 1:
                assert {2 ** 40, -2 ** 40, -1, classes} <= set(c["pred"][0].tolist()) & set(c["gt"][0].tolist())
                assert (bad >= 4).all() and m[0, classes - 1, 0] >= 1 and m[0, 0, classes - 1] >= 1 and int(m[0].sum()) + int(bad[0]) < n
            else:
                assert m.reshape(-1).tolist() == [1] + [0] * (2 * classes * classes - 1) and bad.tolist() == [0, 1]
            truncated = c["pred"].astype(np.int32).astype(np.int64)                                   # a test on 32 bits would count these
            assert n == 1 or not np.array_equal(raw.metric_confusion(truncated, c["gt"], classes, _zeros(2, classes, classes), _zeros(2))[1], bad)


def test_cloud_metric_cases_stand_on_the_thresholds():
    assert sc.CLOUD_T2[-1] == sc.CLOUD_R2 and list(sc.CLOUD_T2) == sorted(sc.CLOUD_T2)
    for n in sc.CLOUD_METRIC_SIZES:
        d2 = sc.cloud_metric_case(n)["d2"]
        sums = nr.cloud_sums(d2, sc.CLOUD_T2, sc.CLOUD_R2)
        assert len(d2) == n and np.isfinite(d2[-1]) and d2[-1] in sc.CLOUD_T2
        if n > 1:
            assert sums[0] == n - 3 and all(t in d2 for t in sc.CLOUD_T2) and sums[2:] == sorted(sums[2:]) and sums[-1] == n - 3
            assert sums != nr.cloud_sums(d2[:-1], sc.CLOUD_T2, sc.CLOUD_R2)


def test_search_cases_lose_the_lanes_they_say():
    for nq in sc.SEARCH_QUERIES:
        c = sc.search_case(nq)
        perm, spoiled = c["visit"]["permutation"], c["visit"]["spoiled"]
        assert sorted(perm.tolist()) == list(range(nq)) and raw.visited(perm, nq).all() and raw.visited(None, nq).all()
        lost = int((~raw.visited(spoiled, nq)).sum())
        assert lost == (3 if nq > 1 else 1) and spoiled.min() >= -1 and spoiled.max() <= nq             # one row past either end at the most
        d2, index, _ = raw.cloud_nearest(c["ref_sorted"], c["foreign"], c["queries"], None, sc.SEARCH_R)
        n = len(c["ref"])
        found = np.isfinite(d2)
        assert found.any() and ((index[found] < 0) | (index[found] >= n)).any() and not ((c["foreign"] >= 0) & (c["foreign"] < n))[::3].any()
    c = sc.search_case(257)
    counts, _ = raw.cloud_count(c["ref_sorted"], c["queries"], None, sc.SEARCH_R, sc.BIG_CAP)
    assert 1 < counts.max() < sc.BIG_CAP and (counts == 0).any()
    d2, index, _ = raw.cloud_nearest(c["ref_sorted"], c["order"], c["queries"], None, sc.SEARCH_R)
    assert d2[0] == 0.0625 and index[0] == 5 and d2[1] == 0.25 and np.isinf(d2[2:7]).all()            # the tie, exactly r, one step beyond, nothing
    one = sc.search_case(257, True)
    d2, index, _ = raw.cloud_nearest(one["ref_sorted"], one["order"], one["queries"], None, sc.SEARCH_R)
    assert len(one["ref"]) == 1 and d2[:3].tolist() == [0.0, 0.25, np.inf] and index[:3].tolist() == [0, 0, -1]


def _sweep(c):
    return raw.cloud_sweep(c["rays_o"], c["rays_d"], c["ranges"], c["offsets"], c["total"], c["max_rays"], c["l2w"], c["cams"], c["objs"], c["images"],
                           c["image_bytes"])


def test_sweep_cases_drop_and_refuse_what_they_say():
    whole = _sweep(sc.sweep_case("whole"))
    total = sc.sweep_case("whole")["total"]
    assert sc.sweep_case("whole")["max_rays"] == 300 == int(np.diff(sc.sweep_case("whole")["offsets"]).max())
    for at in (0, 299, 300, 556, 557):
        assert whole[1][at] >= 0, at                                                                 # the first and the last return of each frame are seen
    c = sc.sweep_case("spoiled offsets")
    packed, labels, written, dropped, refused = _sweep(c)
    assert dropped == 2 and written.all() and refused == 0 and c["offsets"].min() == -1 and c["offsets"].max() == total + 1
    assert np.diff(c["offsets"]).min() < 0 and np.diff(c["offsets"]).max() <= c["max_rays"]
    assert np.array_equal(packed[:300], whole[0][:300]) and not np.array_equal(packed[300:], whole[0][300:])       # frame 1's table now serves the last return
    c = sc.sweep_case("spoiled cameras")
    packed, labels, written, dropped, refused = _sweep(c)
    assert dropped == 0 and written.all() and c["image_bytes"] == c["buffer_bytes"] - 1
    per_frame = [raw.cloud_sweep(c["rays_o"], c["rays_d"], c["ranges"], np.array([a, b]), total, 300, c["l2w"][f:f + 1], c["cams"][f:f + 1], c["objs"][f:f + 1],
                                 c["images"], c["image_bytes"])[4] for f, (a, b) in enumerate(((0, 300), (300, 557), (557, 558)))]
    assert per_frame[0] > 0 and per_frame[1] > 0                                                      # at < 0; at + 3 > image_bytes
    last = raw.cloud_sweep(c["rays_o"][[299]], c["rays_d"][[299]], c["ranges"][[299]], np.array([0, 1]), 1, 1, c["l2w"][:1], [[c["cams"][2][1]]], [[]], c["images"],
                           c["image_bytes"])
    assert last[4] == 1 and last[1][0] == -1                                                          # the buffer's last pixel, one byte short
    assert min(cam[4] for row in c["cams"] for cam in row) == -3
    assert max(cam[4] + 3 * cam[2] * cam[3] for row in c["cams"] for cam in row) == c["buffer_bytes"] + 1
    assert {(cam[2], cam[3]) for row in c["cams"] for cam in row} >= {(0, 4), (3, 0)}
    none = _sweep(sc.sweep_case("no cameras"))
    assert (none[1] == -1).all() and not none[0][:, 3].any() and np.array_equal(none[0][:, :3], _sweep(sc.sweep_case("no objects"))[0][:, :3])
    flat = _sweep(sc.sweep_case("no objects"))
    assert set(flat[1].tolist()) == {-1, 0} and np.array_equal(flat[1] >= 0, whole[1] >= 0)
    cam, obj = sc.sweep_tables(sc.sweep_case("spoiled cameras"))
    assert cam.shape == (3, 2, 24) and obj.shape == (3, 2, 16) and cam[0, 1, 21:].tolist() == [2, 5, -3]


def _old_reduce(seg, cnt):
    """The segmented reduction as it compared ranks alone (a lane took the lane o further on whenever their ranks were equal), for one
    wave of up to 64 lanes: the count that each head adds.  With a dropped lane inside a run it adds the run's second part twice."""
    seg, cnt = list(seg) + [-1] * (64 - len(seg)), list(cnt) + [0] * (64 - len(cnt))
    o = 1
    while o < 64:
        cnt = [c + (cnt[l + o] if seg[l] >= 0 and l + o < 64 and seg[l + o] == seg[l] else 0) for l, c in enumerate(cnt)]
        o *= 2
    return sum(c for l, c in enumerate(cnt) if seg[l] >= 0 and (l == 0 or seg[l - 1] != seg[l]))


def _run_reduce(seg, cnt):
    """The same with runs bounded by the heads and the dropped lanes, as DESIGN.md §13 states it."""
    seg, cnt = list(seg) + [-1] * (64 - len(seg)), list(cnt) + [0] * (64 - len(cnt))
    ends = [seg[l] < 0 or l == 0 or seg[l - 1] != seg[l] for l in range(64)]
    o = 1
    while o < 64:
        cnt = [c + (cnt[l + o] if seg[l] >= 0 and l + o < 64 and not any(ends[l + 1:l + o + 1]) else 0) for l, c in enumerate(cnt)]
        o *= 2
    return sum(c for l, c in enumerate(cnt) if seg[l] >= 0 and ends[l])


def test_voxel_cases_cross_the_boundaries_and_split_a_run():
    for n, runs in sc.VOXEL_RUNS.items():
        assert sum(runs) == n
        starts = np.cumsum(np.r_[0, runs[:-1]])
        if n > 1:
            assert any(a < 64 < a + m for a, m in zip(starts, runs)) and 1 in runs                   # a run across a wave boundary
        if n > 256:
            assert any(a < 256 < a + m for a, m in zip(starts, runs)) and any(a < 64 and a + m > 128 for a, m in zip(starts, runs))
        whole = sc.voxel_case(n)
        assert np.array_equal(np.bincount(whole["segments"]), runs) and whole["voxels"] == (len(runs) + 1 if n > 1 else 1) <= n
        base, _ = raw.voxel_reduce(whole["packed"], whole["order"], whole["segments"], sc.VOXEL, _zeros(whole["voxels"], 8))
        start = sc.start_sums((whole["voxels"], 8), n)
        for spoil in ("order", "segments"):
            c = sc.voxel_case(n, spoil)
            bad = c["order"] if spoil == "order" else c["segments"]
            limit = n if spoil == "order" else c["voxels"]
            assert bad.min() >= -1 and bad.max() <= limit and {int(bad[j]) for j in c["spoiled"]} <= {-1, limit}
            sums, dropped = raw.voxel_reduce(c["packed"], c["order"], c["segments"], sc.VOXEL, start)
            assert dropped == len(c["spoiled"]) == (3 if n > 1 else 1)
            assert int((sums - start)[:, 0].sum()) == n - dropped and (n == 1 or np.array_equal(sums[-1], start[-1]))      # no entry names the last voxel
            named = np.unique(whole["segments"][[j for j in range(n) if j not in c["spoiled"]]]) if n > 1 else []
            assert np.array_equal(sums[named, 7], base[named, 7]) and np.array_equal((sums - start)[:, 1:7].sum(0) <= base[:, 1:7].sum(0), [True] * 6)
            if n > 1:
                j = c["spoiled"][0]
                seg = whole["segments"]
                assert seg[j - 1] == seg[j] == seg[j + 1] and j % 64 not in (0, 63)                  # inside a run, inside a wave
                wave = slice(64 * (j // 64), 64 * (j // 64) + 64)
                lane_seg = np.where(np.arange(n)[wave] == j, -1, seg[wave])
                cnt = (lane_seg >= 0).astype(int)
                assert _run_reduce(lane_seg, cnt) == cnt.sum() and _old_reduce(lane_seg, cnt) > cnt.sum()
                assert _run_reduce(seg[wave], np.ones(len(seg[wave]), int)) == _old_reduce(seg[wave], np.ones(len(seg[wave]), int)) == len(seg[wave])
    c = sc.voxel_case(257)
    sums, _ = raw.voxel_reduce(c["packed"], c["order"], c["segments"], sc.VOXEL, _zeros(c["voxels"], 8))
    assert sums[1, 0] == 2 and sums[1, 1:4].tolist() == [21, 1, 509] and raw.voxel_finish(sums, sc.VOXEL)[1, 3] == 11 | 1 << 8 | 255 << 16   # .5 rounds up
    xyz = sc.voxel_wrap_points()
    idx = cr.voxel_indices(xyz, sc.VOXEL)
    assert (np.abs(idx[:6]) >= 1 << 20).any(axis=1).all() and (np.abs(idx[6:]) < 1 << 20).all()
    keys = raw.voxel_keys(xyz, sc.VOXEL)
    assert (keys >= 0).all() and keys[2] == (1 << 20) << 42 | (1 << 20) << 21 | 0 and np.array_equal(keys[6:], cr.voxel_keys(idx[6:]))


def test_view_cases_reach_the_corners_and_skip_what_they_say():
    for hw in sc.VIEW_SIZES:
        for N in sc.VIEW_WITNESSES:
            near, wild = sc.view_case(hw, N, "near"), sc.view_case(hw, N, "wild")
            V = near["V"]
            assert near["witnesses"].min() == -1 or N == 1
            assert near["witnesses"].max() == V and wild["witnesses"].max() == sc.INT32_MAX and (wild["witnesses"].min() == sc.INT32_MIN or N == 1)
            assert all(s in near["witnesses"][s] for s in range(V)) or N == 1
            got = [raw.view_consistency(c["depth"], c["flags"], c["src"], c["wit"], c["times"], c["witnesses"], _zeros(V, 6),
                                        **{k: c[k] for k in sc.VIEW_PARAMS}) for c in (near, wild)]
            if N == 64:
                assert got[0][3][:, 0].all() and got[0][0].max() > 1 and hw[0] * hw[1] == 1 or got[0][1].any()
    c = sc.view_case((16, 16), 64, "near")
    corners = set()
    for s in range(c["V"]):
        P = vr.world_points(c["depth"][s], c["src"][s])
        for w in range(c["V"]):
            ok, jw, iw, _ = vr.projections(P, (c["flags"][s] & 1) != 0, c["wit"][w], (16, 16))
            corners |= {(int(j), int(i)) for j, i in zip(jw[ok], iw[ok]) if j in (0, 15) and i in (0, 15)}
            if w in (3, 4):
                assert not ok.any()                                                                   # a NaN row, 1e300: no evidence
    assert corners == {(0, 0), (0, 15), (15, 0), (15, 15)} and c["r"] == 2
    e = sc.view_exact_case()
    P = vr.world_points(e["depth"][0], e["src"][0])
    m = e["wit"][1]
    u = m[12] * (vr.row(m[0:4], *P) / vr.row(m[8:12], *P)) + m[14]
    assert np.array_equal(u, [[1, 2, 3, 4]] * 2)                                                      # column 3 lands on u == W exactly
    agree, violate, keep, stats = raw.view_consistency(e["depth"], e["flags"], e["src"], e["wit"], e["times"], e["witnesses"], _zeros(2, 6),
                                                       **{k: e[k] for k in sc.VIEW_PARAMS})
    assert agree[0].tolist() == [[1, 1, 1, 0]] * 2 and agree[1].tolist() == [[1, 1, 1, 1]] * 2 and not violate.any()
    assert stats.tolist() == [[8, 6, 6, 6, 0, 0], [8, 8, 8, 8, 0, 0]]


def test_every_entry_point_has_refusals_whose_message_is_in_its_source():
    assert len(sc.ENTRY_POINTS) == 18 and {r[0] for r in sc.REFUSALS} == set(sc.ENTRY_POINTS)
    assert len({r[:2] for r in sc.REFUSALS}) == len(sc.REFUSALS) and all(r[2] and r[3] for r in sc.REFUSALS)
    src = "".join(open(os.path.join(ROOT, "mudg_amd", "csrc", name)).read() for name in sc.SOURCES)
    for name in sc.ENTRY_POINTS:
        assert f'extern "C" int mudg_{name}(' in src, name
    for piece in {r[3] for r in sc.REFUSALS}:
        assert piece in src, piece
    assert src.count("MUDG_REQUIRE(") == 55                                                           # a new clause needs a case in REFUSALS
