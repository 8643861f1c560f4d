"""Neighbour search on the GPU (csrc/neighbours.hip through mudg_amd/cloud.py, mudg_amd/metrics.py and depth.fuse_views) against the CPU
definition of the rule (tests/neighbours_reference.py): torch.equal everywhere — both sides perform the same correctly rounded fp64
operations in the same order, a minimum with a stated tie rule, capped counts and integer sums, so there is no tolerance."""
import numpy as np
import pytest
import torch

import consistency_reference as cr
import neighbours_reference as nr

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
R = nr.LATTICE_RADIUS


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _cloud(xyz, device, seed=0):
    from mudg_amd import render
    rgb = np.random.default_rng(seed).integers(0, 256, (len(xyz), 3), dtype=np.uint8)
    return render.PointCloud.from_arrays(np.asarray(xyz, dtype=F), rgb, device)


@pytest.fixture(scope="module")
def cases():
    """The shared inputs with the definition's answers; computed once, left unchanged."""
    out = {}
    ref, queries, names = nr.lattice_case()
    out["lattice"] = {"ref": ref, "queries": queries, "names": names}
    ref, queries = nr.one_cell_case()
    out["one_cell"] = {"ref": ref, "queries": queries}
    out["one_point"] = {"ref": out["lattice"]["ref"][:1].copy(), "queries": np.concatenate([out["lattice"]["ref"][:1], out["lattice"]["queries"][:64]])}
    for c in out.values():
        c["nearest"] = nr.nearest(c["ref"], c["queries"], R)
        true = nr.counts(c["ref"], c["queries"], R, 10 ** 6)
        c["true"] = true
        c["caps"] = sorted({1, int(np.sort(true[true > 0])[(true > 0).sum() // 2]), int(true.max()), int(true.max()) + 7})
        c["counts"] = {cap: nr.counts(c["ref"], c["queries"], R, cap) for cap in c["caps"]}
    return out


def _nearest(cuda, ref, queries, r=R):
    from mudg_amd import cloud
    grid = cloud.NeighbourGrid.build(_cloud(ref, cuda), r)
    d2, index = cloud.nearest(grid, _cloud(queries, cuda, 1))
    assert d2.dtype == torch.float64 and index.dtype == torch.int64 and d2.shape == index.shape == (len(queries),)
    return grid, d2.cpu(), index.cpu()


def _assert_nearest(got_d2, got_index, want, what):
    d2, index = _t(want[0]), _t(want[1])
    print(f"{what}: {int((got_d2 != d2).sum())} of {len(d2)} distances and {int((got_index != index).sum())} indices differ; "
          f"{int(torch.isfinite(d2).sum())} queries find a neighbour")
    assert torch.equal(got_d2, d2) and torch.equal(got_index, index), what


@pytest.mark.parametrize("case", ["lattice", "one_cell", "one_point"])
def test_nearest_is_bit_equal_to_the_cpu_definition(cuda, cases, case):
    from mudg_amd import cloud
    c = cases[case]
    grid, d2, index = _nearest(cuda, c["ref"], c["queries"])
    _assert_nearest(d2, index, c["nearest"], case)
    assert len(grid) == len(c["ref"]) and grid.radius == R and grid.r2 == R * R and grid.cell == float(nr.cell_edge(R))
    keys = grid.keys.cpu()
    assert bool((keys[1:] >= keys[:-1]).all()) and torch.equal(grid.order.cpu().sort()[0], torch.arange(len(c["ref"])))
    assert torch.equal(grid.points.cpu()[:, :3].contiguous().view(torch.float32), _t(c["ref"])[grid.order.cpu()])
    # one query; the queries as packed points instead of a cloud; twice: equal bits
    for k in (0, len(c["queries"]) - 1):
        _, one_d2, one_index = _nearest(cuda, c["ref"], c["queries"][k:k + 1])
        assert torch.equal(one_d2, _t(c["nearest"][0][k:k + 1])) and torch.equal(one_index, _t(c["nearest"][1][k:k + 1])), (case, k)
    again = cloud.nearest(grid, _cloud(c["queries"], cuda, 2).points)
    assert torch.equal(again[0].cpu(), d2) and torch.equal(again[1].cpu(), index)
    if case == "lattice":
        n, want_d2, want_index = c["names"], c["nearest"][0], c["nearest"][1]
        assert want_index[n["tie"]] == 5 and want_d2[n["tie"]] == 0.0625 and index[n["tie"]] == 5               # the lower original index, at the higher key
        assert want_index[n["at_r"]] == 20 and d2[n["at_r"]] == 0.25 and index[n["beyond"]] == -1
        for name in ("nothing", "nan", "inf", "far", "outside", "past_top", "beyond"):
            assert index[n[name]] == -1 and d2[n[name]] == float("inf"), name
        assert index[n["top"]] == 30 and index[n["bottom"]] == 31 and index[11] == 0 and d2[11] == 0.0
        assert int((want_d2 == 0.25).sum()) >= 2 and int(np.isfinite(want_d2).sum()) > 100
    if case == "one_cell":
        assert int((keys != keys[0]).sum()) == 0                                                                 # one cell holds the whole cloud


def test_queries_in_shuffled_order_return_the_shuffled_results(cuda, cases):
    c = cases["lattice"]
    perm = np.random.default_rng(5).permutation(len(c["queries"]))
    _, d2, index = _nearest(cuda, c["ref"], c["queries"][perm])
    _assert_nearest(d2, index, (c["nearest"][0][perm], c["nearest"][1][perm]), "shuffled")
    # the entry point itself, with no visiting order and with a reversed one
    from mudg_amd import cloud, ops
    grid = cloud.NeighbourGrid.build(_cloud(c["ref"], cuda), R)
    q = _cloud(c["queries"], cuda).points
    for visit in (None, torch.arange(len(q) - 1, -1, -1, device=cuda)):
        got = ops.cloud_nearest(grid.points, grid.keys, grid.order, q, grid.cell, grid.r2, visit=visit)
        _assert_nearest(got[0].cpu(), got[1].cpu(), c["nearest"], "visit " + ("none" if visit is None else "reversed"))


@pytest.mark.parametrize("case", ["lattice", "one_cell", "one_point"])
def test_neighbour_counts_with_the_cap_below_at_and_above_the_count(cuda, cases, case):
    from mudg_amd import cloud
    c = cases[case]
    grid = cloud.NeighbourGrid.build(_cloud(c["ref"], cuda), R)
    q = _cloud(c["queries"], cuda)
    print(f"{case}: true counts up to {int(c['true'].max())}, caps {c['caps']}")
    for cap in c["caps"]:
        got = cloud.neighbour_counts(grid, q, cap)
        want = _t(c["counts"][cap])
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (case, cap, int((got.cpu() != want).sum()))
        assert torch.equal(cloud.neighbour_counts(grid, q, cap), got)
    top = c["counts"][c["caps"][-1]]
    assert np.array_equal(top, c["true"]) and (c["counts"][1] == (c["true"] > 0)).all()
    assert ((c["true"] > c["caps"][1]).any() and (c["true"] == c["caps"][1]).any()) or case == "one_point"     # below, at and above


def test_radius_outliers_drops_the_known_isolated_points(cuda):
    from mudg_amd import cloud
    g = np.stack(np.meshgrid(*[np.arange(6) * 0.25] * 3, indexing="ij"), axis=-1).reshape(-1, 3)               # 216 points 0.25 m apart
    lone = np.array([[10.0, 0.0, 0.0], [-7.0, 3.0, 2.0], [0.0, 0.0, 40.0]])                                     # nothing within metres
    pair = np.array([[20.0, 20.0, 20.0], [20.0, 20.0, 20.0]])                                                   # duplicates: each other's neighbour
    xyz = np.concatenate([lone[:1], g[:100], lone[1:2], pair, g[100:], lone[2:]]).astype(F)
    where_lone, where_pair = [0, 101, len(xyz) - 1], [102, 103]
    pc = _cloud(xyz, cuda)
    for m in (0, 1, 2, 3, 6, 7):
        keep = cloud.radius_outliers(pc, 0.25, m)
        want = nr.radius_outliers(xyz, 0.25, m)
        assert keep.dtype == torch.bool and torch.equal(keep.cpu(), _t(want)), m
        assert all(bool(keep[i]) == (m == 0) for i in where_lone) and all(bool(keep[i]) == (m <= 1) for i in where_pair), m
    keep = cloud.radius_outliers(pc, 0.25, 3)                                                                   # a corner of the block has three neighbours at 0.25
    assert int(keep.sum()) == 216
    kept = cloud.remove_outliers(pc, 0.25, 3)
    assert torch.equal(kept.points, pc.points[keep]) and len(kept) == 216                                       # stable: the order stays
    assert int(cloud.radius_outliers(pc, 0.25, 6).sum()) == 64 and int(cloud.radius_outliers(pc, 0.25, 7).sum()) == 0      # the interior has six


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 2048, 2049, 5000])
def test_metric_cloud_equals_python_integers(cuda, n):
    from mudg_amd import ops
    rng = np.random.default_rng(n)
    d2 = rng.integers(0, 17, n).astype(D) / 64.0
    d2[rng.random(n) < 0.2] = np.inf
    if n > 1:
        d2[0], d2[n - 1] = np.inf, 0.25
    t2 = [1 / 64, 4 / 64, 0.0625 + 2.0 ** -40, 0.25]
    for thresholds in (t2, t2[:1], []):
        got = ops.metric_cloud(_t(d2).to(cuda), thresholds, 0.25)
        assert got.dtype == torch.int64 and got.cpu().tolist() == nr.cloud_sums(d2, thresholds, 0.25), (n, thresholds)
    assert torch.equal(ops.metric_cloud(_t(d2).to(cuda), t2, 0.25), ops.metric_cloud(_t(d2).to(cuda), t2, 0.25))
    irrational = rng.uniform(0.0, 4096.0, n)                                                                    # roots that are not on the grid
    assert ops.metric_cloud(_t(irrational).to(cuda), [1.0, 4096.0], 4096.0).cpu().tolist() == nr.cloud_sums(irrational, [1.0, 4096.0], 4096.0)


def _assert_scores(got, want, what):
    assert set(got) == set(want)
    for k, w in want.items():
        w = torch.from_numpy(np.array(w))                                                                        # a score may have no dimensions
        g = got[k].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape)
        assert torch.equal(g.view(torch.int64), w.view(torch.int64)), (what, k, g, w)                           # the bits: nan equals nan


def test_cloud_scores_where_the_answer_is_known_without_arithmetic(cuda, cases):
    from mudg_amd import metrics
    g = np.stack(np.meshgrid(*[np.arange(5) * 0.5] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(F) - F(1.0)
    pc = _cloud(g, cuda)
    same = metrics.cloud_scores(pc, _cloud(g, cuda, 3))
    for k in ("accuracy", "completeness", "fscore"):
        assert same[k].cpu().tolist() == [1.0] * 4, k
    assert same["found"].cpu().tolist() == [1.0, 1.0] and float(same["mean_accuracy"]) == float(same["mean_completeness"]) == float(same["chamfer"]) == 0.0
    assert same["sums"].cpu().tolist() == [[125, 0, 125, 125, 125, 125]] * 2
    shifted = (g.astype(D) + [0.125, 0.0, 0.0]).astype(F)
    s = metrics.cloud_scores(pc, _cloud(shifted, cuda))
    assert s["sums"].cpu().tolist() == [[125, 125 * 2 ** 17, 0, 0, 125, 125]] * 2                                # every d2 is exactly 2^-6
    assert s["accuracy"].cpu().tolist() == s["completeness"].cpu().tolist() == [0.0, 0.0, 1.0, 1.0]
    assert float(s["mean_accuracy"]) == float(s["mean_completeness"]) == 0.125 and float(s["chamfer"]) == 0.25
    _assert_scores(s, nr.cloud_scores(g, shifted), "shifted")
    _assert_scores(metrics.cloud_scores(pc, _cloud(shifted, cuda), (0.125, 0.375)), nr.cloud_scores(g, shifted, (0.125, 0.375)), "two thresholds")
    apart = metrics.cloud_scores(pc, _cloud(g + F(100.0), cuda))
    _assert_scores(apart, nr.cloud_scores(g, g + F(100.0)), "apart")
    assert bool(torch.isnan(apart["chamfer"])) and bool(torch.isnan(apart["fscore"]).all())
    # two clouds of different sizes that are not each other's twins, and the same again: equal bits
    c = cases["lattice"]
    with np.errstate(invalid="ignore"):
        use = np.abs(c["queries"]).max(axis=1) < 100.0                                                           # a reference stays inside the grid
    a, b = _cloud(c["queries"][use], cuda), _cloud(c["ref"], cuda)
    first = metrics.cloud_scores(a, b, (0.125, 0.25, 0.5))
    _assert_scores(first, nr.cloud_scores(c["queries"][use], c["ref"], (0.125, 0.25, 0.5)), "lattice")
    _assert_scores(metrics.cloud_scores(a, b, (0.125, 0.25, 0.5)), {k: v.cpu().numpy() for k, v in first.items()}, "again")
    assert 0.0 < float(first["accuracy"][0]) < float(first["accuracy"][2]) < 1.0


def _window(cuda):
    """The analytic scene's six views with noise, so that the consistency filter keeps some pixels and drops others."""
    hw = (23, 29)
    rng = np.random.default_rng(71)
    z, c2w, times, poses = cr.scene_views(hw)
    z = (z.astype(D) * (1 + rng.normal(0, 0.03, z.shape))).astype(F)
    rgb = rng.integers(0, 256, z.shape + (3,), dtype=np.uint8)
    return (_t(z).to(cuda), _t(rgb).to(cuda), cr.SCENE_INTR, c2w, hw), dict(times=times)


def test_fuse_views_is_unchanged_by_default_and_removes_outliers_on_request(cuda):
    from mudg_amd import cloud, depth
    args, rule = _window(cuda)
    result = depth.consistent_views(args[0], *args[2:], **rule)
    lifted = depth.lift_views(*args, keep=result["keep"])
    points, got = depth.fuse_views(*args, **rule)
    assert torch.equal(points.points, lifted.points) and 0 < len(points) < args[0].numel()
    for k in result:
        assert torch.equal(got[k], result[k]), k
    thinned, _ = depth.fuse_views(*args, voxel_size=0.5, **rule)
    assert torch.equal(thinned.points, cloud.voxel_downsample(lifted, 0.5).points)
    radius = 1.0
    others = cloud.neighbour_counts(cloud.NeighbourGrid.build(lifted, radius), lifted, 10 ** 6) - 1
    need = int(others.median()) + 1                                                                              # more neighbours than the median point has
    print(f"{len(lifted)} lifted points, 0 .. {int(others.max())} others within {radius} m, median {need - 1}")
    keep = cloud.radius_outliers(lifted, radius, need)
    xyz = lifted.points.cpu()[:, :3].contiguous().view(torch.float32).numpy()
    assert torch.equal(keep.cpu(), _t(nr.radius_outliers(xyz, radius, need))) and 0 < int(keep.sum()) < len(lifted)
    filtered, again = depth.fuse_views(*args, neighbour_radius=radius, min_neighbours=need, **rule)
    assert torch.equal(filtered.points, cloud.remove_outliers(lifted, radius, need).points) and torch.equal(filtered.points, lifted.points[keep])
    assert torch.equal(again["keep"], result["keep"])
    both, _ = depth.fuse_views(*args, voxel_size=0.5, neighbour_radius=radius, min_neighbours=need, **rule)
    assert torch.equal(both.points, cloud.voxel_downsample(filtered, 0.5).points)                               # outliers go before the thinning
    everything, _ = depth.fuse_views(*args, neighbour_radius=radius, **rule)                                   # min_neighbours = 0 keeps every point
    assert torch.equal(everything.points, lifted.points)
