"""What the neighbour-search rule can show without a GPU: the brute-force definition (tests/neighbours_reference.py)
against exact arithmetic on lattice inputs, the 27-cell walk against the brute force on inputs that target the walk, the host checks of
the Python surface, and the C-ABI and generated code of csrc/neighbours.hip."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import neighbours_reference as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, D = np.float32, np.float64
ENTRIES = (("mudg_cloud_nearest", 12), ("mudg_cloud_count", 12), ("mudg_metric_cloud", 7))


# ------------------------------------------------------------------------------------------------ the rule against exact arithmetic
def _exact(ref, queries, r):
    """Every pair in Fractions: (d2 or None where not within reach) per query, per reference point."""
    r2 = Fraction(r) ** 2
    rows = []
    for q in queries:
        row = []
        for p in ref:
            if not all(math.isfinite(float(v)) for v in q):
                row.append(None)
                continue
            d2 = sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(q, p))
            row.append(d2 if d2 <= r2 else None)
        rows.append(row)
    return rows


def test_the_brute_force_definition_equals_exact_arithmetic_on_the_lattice():
    """Coordinates on multiples of 1/8 at r = 0.5: d2 == r2 exactly for some pairs (inside) and r2 + 1/64 for others (outside)."""
    rng = np.random.default_rng(3)
    ref = (rng.integers(-6, 7, (60, 3)) * nr.STEP).astype(F32)
    queries = (rng.integers(-8, 9, (40, 3)) * nr.STEP).astype(F32)
    ref[0], ref[1], queries[0] = [0.5, 0.0, 0.0], [0.5, 0.125, 0.0], [0.0, 0.0, 0.0]                         # exactly r, and one step beyond
    ref[2], ref[3], queries[1] = [0.25, 0.5, 0.5], [-0.25, 0.5, 0.5], [0.0, 0.5, 0.5]                        # a tie
    ref[5] = ref[4]                                                                                          # a duplicate
    queries[2] = [np.nan, 0.0, 0.0]
    for k in range(12):                                                                                      # exactly r along each axis, both ways
        ref[10 + k] = queries[3 + k] + np.eye(3, dtype=F32)[k % 3] * F32(0.5 if k < 6 else -0.5)
    exact = _exact(ref, queries, 0.5)
    assert exact[0][0] == Fraction(1, 4) and exact[0][1] is None                                             # d2 == r2 is inside, r2 + 1/64 is not
    assert sum(Fraction(float(a)) ** 2 for a in ref[1]) == Fraction(1, 4) + Fraction(1, 64)
    at_r = sum(1 for row in exact for v in row if v == Fraction(1, 4))
    beyond = sum(1 for q in queries[3:] for p in ref if sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(q, p)) == Fraction(17, 64))
    assert at_r > 5 and beyond > 5, (at_r, beyond)
    d2, index = nr.nearest(ref, queries, 0.5)
    for k, row in enumerate(exact):
        inside = [(v, i) for i, v in enumerate(row) if v is not None]
        if not inside:
            assert d2[k] == np.inf and index[k] == -1, k
        else:
            best = min(inside)                                                                               # the smallest d2, then the lowest index
            assert Fraction(float(d2[k])) == best[0] and index[k] == best[1], k
    assert index[1] == 2 and d2[1] == 0.0625 and d2[2] == np.inf and index[2] == -1
    true = [sum(v is not None for v in row) for row in exact]
    for cap in (1, 2, max(true), max(true) + 5):
        assert nr.counts(ref, queries, 0.5, cap).tolist() == [min(t, cap) for t in true], cap
    assert nr.counts(ref, queries, 0.5, 1).dtype == np.int32 and d2.dtype == D and index.dtype == np.int64
    keep = nr.radius_outliers(ref, 0.5, 1)
    own = [sum(v is not None for v in row) for row in _exact(ref, ref, 0.5)]
    assert keep.tolist() == [c >= 2 for c in own] and keep[4] and keep[5] and not keep.all()                                # a point counts itself; a duplicate is a neighbour


def test_the_sums_equal_python_integers_and_the_exact_square_root_within_one():
    rng = np.random.default_rng(5)
    d2 = rng.integers(0, 17, 300).astype(D) / 64.0                                                           # the lattice's squared distances up to r2
    d2[::7] = np.inf
    t2 = [1 / 64, 4 / 64, 0.25]
    got = nr.cloud_sums(d2, t2, 0.25)
    found = [Fraction(float(v)) for v in d2 if math.isfinite(v)]
    assert got[0] == len(found) == 300 - 43
    assert got[2:] == [sum(v <= Fraction(t) for v in found) for t in t2] and got[4] == got[0]
    exact = [math.isqrt(int(v * 2 ** 40)) for v in found]                                                    # floor(sqrt(v) 2^20), exactly
    each = [int(np.floor(np.sqrt(D(float(v))) * 2.0 ** 20)) for v in found]
    assert got[1] == sum(each) and all(abs(a - b) <= 1 for a, b in zip(each, exact))
    squares = [k * k / 64.0 for k in range(5)]                                                               # distances k / 8: the root is exact
    assert nr.cloud_sums(squares, [0.25], 0.25) == [5, sum(k * 2 ** 17 for k in range(5)), 5]
    assert nr.cloud_sums([np.inf, np.nan], [0.25], 0.25) == [0, 0, 0]
    assert (2 ** 31 - 1) * 64 * 2 ** 20 < 2 ** 57                                                            # the headroom at r = 64


def test_the_scores_of_known_clouds():
    g = np.stack(np.meshgrid(*[np.arange(4) * 0.5] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)
    same = nr.cloud_scores(g, g)
    assert same["accuracy"].tolist() == same["completeness"].tolist() == same["fscore"].tolist() == [1.0] * 4
    assert same["found"].tolist() == [1.0, 1.0] and same["mean_accuracy"] == same["mean_completeness"] == same["chamfer"] == 0.0
    shifted = (g.astype(D) + [0.125, 0.0, 0.0]).astype(F32)
    s = nr.cloud_scores(g, shifted)
    assert s["sums"].tolist() == [[64, 64 * 2 ** 17, 0, 0, 64, 64]] * 2                                      # every d2 is exactly 2^-6
    assert s["accuracy"].tolist() == s["completeness"].tolist() == [0.0, 0.0, 1.0, 1.0]
    assert np.isnan(s["fscore"][:2]).all() and s["fscore"][2:].tolist() == [1.0, 1.0]
    assert s["mean_accuracy"] == s["mean_completeness"] == 0.125 and s["chamfer"] == 0.25
    apart = nr.cloud_scores(g, g + F32(100.0))
    assert apart["found"].tolist() == [0.0, 0.0] and np.isnan(apart["chamfer"]) and np.isnan(apart["fscore"]).all()
    walked = nr.cloud_scores(g, shifted, search=lambda *a: nr.walk_nearest(*a)[:2])
    assert walked["sums"].tolist() == s["sums"].tolist()


# ------------------------------------------------------------------------------------------------ the walk against the brute force
def _same(ref, queries, r, caps=(1, 3, 10 ** 6)):
    d2, index = nr.nearest(ref, queries, r)
    w2, windex, examined = nr.walk_nearest(ref, queries, r)
    assert np.array_equal(d2, w2) and np.array_equal(index, windex)
    for cap in caps:
        assert np.array_equal(nr.counts(ref, queries, r, cap), nr.walk_counts(ref, queries, r, cap)), cap
    return d2, index, examined


def test_the_cell_walk_finds_what_brute_force_finds_on_the_shared_cases():
    ref, queries, names = nr.lattice_case()
    d2, index, examined = _same(ref, queries, nr.LATTICE_RADIUS)
    assert examined < len(ref) * len(queries) / 10                                                           # it is a walk, not brute force
    assert index[names["tie"]] == 5 and d2[names["tie"]] == 0.0625                                           # mirrored about the query: the lower index
    assert index[names["at_r"]] == 20 and d2[names["at_r"]] == 0.25 and index[names["beyond"]] == -1
    for name in ("nothing", "nan", "inf", "far", "outside", "past_top"):
        assert index[names[name]] == -1 and d2[names[name]] == np.inf, name
    assert index[names["top"]] == 30 and index[names["bottom"]] == 31
    assert d2[11] == 0.0 and index[11] == 0                                                                  # on a duplicate pair
    ref, queries = nr.one_cell_case()
    order, first, last = nr.walk_intervals(ref, queries, nr.LATTICE_RADIUS)
    assert (last - first).max() == len(ref)                                                                  # one interval holds the whole cloud
    _same(ref, queries, nr.LATTICE_RADIUS, caps=(1, 16, 17, 10 ** 6))
    _same(ref[:1], queries, nr.LATTICE_RADIUS)                                                               # a one-point reference


def test_the_cell_walk_on_cell_boundaries_negative_cells_and_the_grids_ends():
    r = 0.5
    c = float(nr.cell_edge(r))
    rng = np.random.default_rng(9)
    # points on and one fp32 step beside cell boundaries k c, k of both signs, and queries at exactly r and just past r of them
    k = rng.integers(-40, 41, (400, 3)).astype(D)
    on = (k * c).astype(F32)
    ref = np.concatenate([on, np.nextafter(on, F32(np.inf)), np.nextafter(on, F32(-np.inf))])
    axis = rng.integers(0, 3, len(ref))
    step = np.zeros((len(ref), 3))
    step[np.arange(len(ref)), axis] = rng.choice([-r, r], len(ref))
    at_r = (ref.astype(D) + step).astype(F32)
    queries = np.concatenate([at_r, np.nextafter(at_r, F32(np.inf)), np.nextafter(at_r, F32(-np.inf)), ref[::5]])
    d2, index, _ = _same(ref, queries, r)
    assert np.isfinite(d2).sum() > len(ref) and (d2 == r * r).sum() > 50 and np.isinf(d2).sum() > 50
    cells = np.floor(queries.astype(D) / c)
    assert (cells < 0).any() and (cells > 0).any()
    # the ends of the grid: reference cells +-(2^20 - 2), queries in the cells around them and outside the key's range
    top, bottom = nr.edge_coordinate(+1), nr.edge_coordinate(-1)
    ref = np.array([[top, top, top], [bottom, bottom, bottom], [top, bottom, 0.0], [top + 0.375, top, top]], dtype=F32)
    assert np.floor(ref.astype(D) / c).max() == nr.REF_MAX and np.floor(ref.astype(D) / c).min() == -nr.REF_MAX
    offsets = np.array([[a, b, e] for a in (-0.5, -0.125, 0.0, 0.125, 0.5, 0.625, 1.0, 1.5) for b in (-0.5, 0.0, 0.5) for e in (-0.125, 0.0)])
    queries = np.concatenate([ref[i].astype(D) + s * offsets for i, s in ((0, 1.0), (1, -1.0), (2, 1.0))]).astype(F32)
    cells = np.floor(queries.astype(D) / c)
    assert (cells == nr.HALF).any() and (cells == nr.CELL_MAX).any() and (cells == -nr.HALF).any() and (cells == -nr.HALF - 1).any()
    d2, index, _ = _same(ref, queries, r)
    assert np.isfinite(d2).any() and np.isinf(d2).any() and set(index.tolist()) >= {-1, 0, 1, 2, 3}
    with pytest.raises(AssertionError, match="leaves the grid"):
        nr.walk_intervals(np.array([[top + 0.5, 0.0, 0.0]], dtype=F32), queries, r)


def test_the_margin_keeps_every_pair_within_reach_in_adjacent_cells():
    """DESIGN.md §22's derivation, sampled: pairs at distance r (1 +- a few ulps) along random directions, at coordinates up to 4e4 m and
    radii from 0.05 to 64: whenever d2 <= r2 the cells differ by at most one per axis."""
    rng = np.random.default_rng(11)
    worst = 0
    for r in (0.05, 0.1, 0.5, 1.0, 7.3, 64.0):
        c = float(nr.cell_edge(r))
        p = rng.uniform(-4e4, 4e4, (20000, 3)).astype(F32)
        p[::3] = (np.rint(p[::3].astype(D) / c) * c).astype(F32)                                              # on cell boundaries
        u = rng.normal(size=(len(p), 3))
        u[::2] = np.eye(3)[rng.integers(0, 3, len(u[::2]))]                                                   # along an axis
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        q = (p.astype(D) + r * u).astype(F32)
        d = q.astype(D) - p.astype(D)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inside = d2 <= r * r
        assert inside.sum() > 1000 and (~inside).sum() > 1000
        gap = np.abs(np.floor(q.astype(D) / c) - np.floor(p.astype(D) / c)).max(axis=1)
        worst = max(worst, int(gap[inside].max()))
    assert worst == 1


# ------------------------------------------------------------------------------------------------ the interface off the GPU
def _host_cloud(xyz):
    """A PointCloud whose buffer is in host memory: enough for the checks that run before any launch."""
    from mudg_amd import render
    xyz = torch.from_numpy(np.asarray(xyz, dtype=F32).reshape(-1, 3))
    pc = render.PointCloud.__new__(render.PointCloud)
    pc.points = torch.cat([xyz.view(torch.int32), torch.zeros((len(xyz), 1), dtype=torch.int32)], dim=1)
    return pc


def test_the_host_checks_raise_before_any_launch():
    from mudg_amd import cloud, depth, hip, metrics, ops
    pc = _host_cloud([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    for radius in (0.0, -1.0, 64.5, float("nan"), float("inf"), "wide"):
        with pytest.raises(hip.MudgError, match="radius"):
            cloud.NeighbourGrid.build(pc, radius)
    with pytest.raises(hip.MudgError, match="empty"):
        cloud.NeighbourGrid.build(_host_cloud(np.zeros((0, 3))), 0.5)
    with pytest.raises(hip.MudgError, match="PointCloud"):
        cloud.NeighbourGrid.build(pc.points, 0.5)
    c = float(nr.cell_edge(0.5))
    for bad in ((nr.REF_MAX + 1) * c + 0.25, -(nr.REF_MAX) * c - 0.25, float("nan"), float("inf")):
        with pytest.raises(hip.MudgError, match="leave the grid"):
            cloud.NeighbourGrid.build(_host_cloud([[0.0, bad, 0.0]]), 0.5)
    with pytest.raises(hip.MudgError, match="on the GPU"):                                                   # in range: the first launch refuses host memory
        cloud.NeighbourGrid.build(_host_cloud([[0.0, nr.edge_coordinate(+1), nr.edge_coordinate(-1)]]), 0.5)
    with pytest.raises(hip.MudgError, match="NeighbourGrid"):
        cloud.nearest(pc, pc)
    grid = cloud.NeighbourGrid(pc.points, torch.zeros(2, dtype=torch.int64), torch.arange(2), 0.5, c, 0.25)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        cloud.nearest(grid, pc)
    for cap in (0, -1, 1.5, None):
        with pytest.raises(hip.MudgError, match="cap"):
            cloud.neighbour_counts(grid, pc, cap)
    for m in (-1, 1.5, None):
        with pytest.raises(hip.MudgError, match="min_neighbours"):
            cloud.radius_outliers(pc, 0.5, m)
    for th in ((0.2, 0.1), (0.1, 0.1), (0.0, 0.1), (-0.1, 0.2), (0.1, 64.5), tuple(0.01 * k for k in range(1, 10)), (), (float("nan"),), ("a",)):
        with pytest.raises(hip.MudgError, match="thresholds"):
            metrics.cloud_scores(pc, pc, th)
    with pytest.raises(hip.MudgError, match="PointCloud"):
        metrics.cloud_scores(pc.points, pc)
    with pytest.raises(hip.MudgError, match="on the GPU"):
        metrics.cloud_scores(pc, pc)
    i32, i64, f64 = pc.points, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.float64)
    for call in (lambda: ops.cloud_nearest(i32, i64, i64, i32, c, 0.25), lambda: ops.cloud_count(i32, i64, i64, i32, c, 0.25, 1),
                 lambda: ops.metric_cloud(f64, [0.25], 0.25)):
        with pytest.raises(hip.MudgError, match="on the GPU"):
            call()
    import inspect
    sig = inspect.signature(depth.fuse_views)
    assert [sig.parameters[k].kind for k in ("neighbour_radius", "min_neighbours")] == [inspect.Parameter.KEYWORD_ONLY] * 2
    assert sig.parameters["neighbour_radius"].default is None and sig.parameters["min_neighbours"].default == 0
    assert ops.NEIGHBOUR_MARGIN == nr.MARGIN and ops.NEIGHBOUR_MAX_RADIUS == nr.MAX_RADIUS and cloud.KEY_LIMIT == nr.HALF


def test_the_product_does_not_import_the_cpu_definition():
    for d in ("mudg_amd", "lvdm", "utils", "virtual_render", "tools"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith(".py"):
                    assert "neighbours_reference" not in open(os.path.join(base, f)).read(), f


# ------------------------------------------------------------------------------------------------ C-ABI and generated code
def test_neighbour_entry_points_are_declared_bound_and_exported():
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
    assert "neighbours.hip" in build.SOURCES


def test_bad_arguments_are_refused_before_any_launch():
    import ctypes
    from mudg_amd import hip
    lib = hip.lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(24)                              # never dereferenced: every call below is rejected first
    c = float(nr.cell_edge(0.5))
    for fn, tail in ((lib.mudg_cloud_nearest, (one, one, None)), (lib.mudg_cloud_count, (1, one, None))):
        good = [one, one, one, 10, one, None, 5, c, 0.25]
        assert fn(None, one, one, 10, one, None, 5, c, 0.25, *tail) == -1 and b"null" in lib.mudg_last_error()
        assert fn(one, one, one, 10, None, None, 5, c, 0.25, *tail) == -1
        assert fn(odd, one, one, 10, one, None, 5, c, 0.25, *tail) == -1 and b"unaligned" in lib.mudg_last_error()
        assert fn(one, one, one, 10, odd, None, 5, c, 0.25, *tail) == -1
        assert fn(one, one, one, 0, one, None, 5, c, 0.25, *tail) == -1 and fn(one, one, one, 10, one, None, 0, c, 0.25, *tail) == -1
        assert fn(one, one, one, 10, one, None, 2 ** 40, c, 0.25, *tail) == -1                                 # more workgroups than a grid holds
        for r2 in (0.0, -1.0, 4096.5, float("nan"), float("inf")):
            assert fn(one, one, one, 10, one, None, 5, 65.0 if r2 > 4096 else c, r2, *tail) == -1, r2
        assert b"radius" in lib.mudg_last_error()
        for cell in (0.5, 0.25, 64.07, float("nan"), float("inf")):                                           # not above r, or above 64 (1 + 2^-10)
            assert fn(*good[:7], cell, 0.25, *tail) == -1, cell
        assert b"cell" in lib.mudg_last_error()
    assert lib.mudg_cloud_nearest(one, one, one, 10, one, None, 5, c, 0.25, None, one, None) == -1
    assert lib.mudg_cloud_nearest(one, one, one, 10, one, None, 5, c, 0.25, one, None, None) == -1
    assert lib.mudg_cloud_count(one, one, one, 10, one, None, 5, c, 0.25, 1, None, None) == -1
    for cap in (0, -3):
        assert lib.mudg_cloud_count(one, one, one, 10, one, None, 5, c, 0.25, cap, one, None) == -1 and b"cap" in lib.mudg_last_error()
    t2 = (ctypes.c_double * 9)(*[0.01 * k for k in range(1, 10)])
    assert lib.mudg_metric_cloud(None, 10, t2, 3, 0.25, one, None) == -1 and lib.mudg_metric_cloud(one, 10, t2, 3, 0.25, None, None) == -1
    assert lib.mudg_metric_cloud(one, 10, None, 3, 0.25, one, None) == -1
    assert lib.mudg_metric_cloud(one, 0, t2, 3, 0.25, one, None) == -1 and lib.mudg_metric_cloud(one, 2 ** 31, t2, 3, 0.25, one, None) == -1
    assert b"2^31" in lib.mudg_last_error()
    assert lib.mudg_metric_cloud(one, 10, t2, 9, 0.25, one, None) == -1 and b"thresholds" in lib.mudg_last_error()
    assert lib.mudg_metric_cloud(one, 10, t2, -1, 0.25, one, None) == -1
    assert lib.mudg_metric_cloud(one, 10, t2, 3, 4097.0, one, None) == -1 and lib.mudg_metric_cloud(one, 10, t2, 3, 0.0, one, None) == -1
    assert lib.mudg_metric_cloud(one, 10, t2, 3, 0.02, one, None) == -1 and b"threshold" in lib.mudg_last_error()      # t2[2] = 0.03 > r2
    bad = (ctypes.c_double * 2)(0.0, float("nan"))
    assert lib.mudg_metric_cloud(one, 10, bad, 1, 0.25, one, None) == -1
    assert lib.mudg_metric_cloud(one, 10, (ctypes.c_double * 2)(0.1, float("nan")), 2, 0.25, one, None) == -1


def test_neighbour_kernels_use_no_scratch_and_keep_their_footprint(tmp_path):
    """Facts about the generated gfx950 code as DESIGN.md §22 records them: no scratch, no spills, at most 64 VGPRs (eight waves per
    SIMD), LDS only in the reduction, and native 64-bit integer atomics there."""
    import shutil
    import subprocess
    from mudg_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "neighbours.s"
    subprocess.run([hipcc, *build.FLAGS, "--cuda-device-only", "-I" + os.path.join(ROOT, "include"), "-S",
                    os.path.join(ROOT, "mudg_amd", "csrc", "neighbours.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    s = out.read_text()
    md = s[s.index("amdhsa.kernels"):]
    seen = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", md, re.S):
        family = "search" if "cloud_neighbours_kernel" in m.group(2) else "sums" if "metric_cloud_kernel" in m.group(2) else None
        assert family, m.group(2)
        seen[family] = seen.get(family, 0) + 1
        print(f"{m.group(2)}: {m.group(1)} bytes of LDS, {m.group(4)} VGPRs")
        assert int(m.group(3)) == 0 and int(m.group(5)) == 0 and int(m.group(4)) <= 64, m.groups()
        assert (int(m.group(1)) == 0) == (family == "search")
    assert seen == {"search": 2, "sums": 1}, seen
    assert "cmpswap" not in s
    for name in sorted(set(re.findall(r"^(_Z\S*(?:cloud_neighbours|metric_cloud)_kernel\S*):", s, re.M))):
        body = s[s.index(name + ":"):]
        lines = [l.strip() for l in body[:body.index(".end_amdhsa_kernel")].splitlines()]
        assert not any(l.startswith(("scratch_", "flat_")) for l in lines), name
        atomics = [l for l in lines if l.startswith("global_atomic")]
        assert all(l.startswith("global_atomic_add_x2") for l in atomics) and len(atomics) == (1 if "metric_cloud" in name else 0), (name, atomics)
