"""The CPU definition of the neighbour-search rule, in numpy: brute force in float64 over chunks — every squared distance
((dx dx + dy dy) + dz dz) as elementwise operations in the stated order —, a minimum with the stated tie rule, capped counts and integer
sums.  A second family finds its candidates by the 27-cell walk over the key-sorted cloud, the way the kernels do.  Written independently
of csrc/neighbours.hip and mudg_amd/cloud.py; the GPU tests demand bit-equality with it, the CPU tests check the brute force against exact
arithmetic and the walk against the brute force.  Clouds are (n, 3) float32 arrays."""
import numpy as np

F = np.float64
HALF = 1 << 20
CELL_MAX = HALF - 1                     # a neighbour cell beyond this holds nothing
REF_MAX = HALF - 2                      # reference cells end here, so that a neighbour's index fits the key
MAX_RADIUS = 64.0
MARGIN = 1.0 + 2.0 ** -10
SCALE = 2.0 ** 20                       # distances are summed on a 2^-20 grid
PAIRS = 1 << 22                         # pairs per chunk


def cell_edge(r):
    return F(r) * F(MARGIN)


def cell_quotients(xyz, c):
    with np.errstate(all="ignore"):
        return np.asarray(xyz, np.float32).reshape(-1, 3).astype(F) / F(c)


def cell_keys(idx):
    """(n, 3) int64 cell indices -> §13's keys, z in the low field."""
    idx = np.asarray(idx, np.int64)
    return ((idx[:, 0] + HALF) << 42) | ((idx[:, 1] + HALF) << 21) | (idx[:, 2] + HALF)


def _d2(q, p):
    """q (a, 1, 3) or (a, 3), p (b, 3) or (a, 3) float64, broadcast: ((dx dx + dy dy) + dz dz)."""
    with np.errstate(all="ignore"):
        d = q - p
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _checked(ref, queries, r):
    ref, queries = np.asarray(ref, np.float32).reshape(-1, 3), np.asarray(queries, np.float32).reshape(-1, 3)
    r = F(r)
    assert 0.0 < r <= MAX_RADIUS and len(ref) > 0
    return ref, queries, r, r * r


# ------------------------------------------------------------------------------------------------ brute force: the rule
def within_reach(ref, queries, r, chunk=None):
    """Chunks of (first query, d2 (rows, n) float64 with +inf where p is not within reach): d2 <= r2, false for a d2 that is not a number."""
    ref, queries, r, r2 = _checked(ref, queries, r)
    p = ref.astype(F)
    rows = max(1, PAIRS // len(ref)) if chunk is None else chunk
    for s in range(0, len(queries), rows):
        d2 = _d2(queries[s:s + rows].astype(F)[:, None, :], p[None, :, :])
        with np.errstate(invalid="ignore"):
            yield s, np.where(d2 <= r2, d2, np.inf)


def nearest(ref, queries, r):
    """(d2 (nq,) float64, index (nq,) int64): the smallest d2 within reach and the lowest index that attains it; +inf and -1 for none."""
    best, index = np.full(len(queries), np.inf), np.full(len(queries), -1, dtype=np.int64)
    for s, d2 in within_reach(ref, queries, r):
        at = np.argmin(d2, axis=1)                                           # the first occurrence of the minimum: the lowest index
        m = d2[np.arange(len(at)), at]
        best[s:s + len(at)] = m
        index[s:s + len(at)] = np.where(np.isfinite(m), at, -1)
    return best, index


def counts(ref, queries, r, cap):
    """(nq,) int32: min(points within reach, cap)."""
    assert cap >= 1
    out = np.zeros(len(queries), dtype=np.int32)
    for s, d2 in within_reach(ref, queries, r):
        out[s:s + len(d2)] = np.minimum(np.isfinite(d2).sum(axis=1), cap)
    return out


def radius_outliers(points, r, min_neighbours):
    """The keep mask: a point counts itself, so keep iff count >= min_neighbours + 1."""
    return counts(points, points, r, min_neighbours + 1) >= min_neighbours + 1


# ------------------------------------------------------------------------------------------------ the 27-cell walk
def walk_intervals(ref, queries, r):
    """The key-sorted reference and every query's nine candidate intervals (x + a, y + b, z - 1 .. z + 1) of it.  Returns (order (n,) —
    the original index of each sorted point —, first (nq, 9), last (nq, 9)); an interval that is skipped is empty."""
    ref, queries, r, _ = _checked(ref, queries, r)
    c = cell_edge(r)
    ri = np.floor(cell_quotients(ref, c))
    assert np.all(np.isfinite(ri)) and np.all(np.abs(ri) <= REF_MAX), "the reference leaves the grid"
    keys = cell_keys(ri.astype(np.int64))
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    t = cell_quotients(queries, c)
    with np.errstate(invalid="ignore"):
        ok = np.all(np.abs(t) < HALF + 1, axis=1)                            # in fp64, before any conversion; false for nan and inf
    qi = np.floor(np.where(ok[:, None], t, 0.0)).astype(np.int64)
    z0, z1 = np.maximum(qi[:, 2] - 1, -CELL_MAX), np.minimum(qi[:, 2] + 1, CELL_MAX)
    first, last = np.zeros((len(queries), 9), dtype=np.int64), np.zeros((len(queries), 9), dtype=np.int64)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            cx, cy = qi[:, 0] + a, qi[:, 1] + b
            use = ok & (np.abs(cx) <= CELL_MAX) & (np.abs(cy) <= CELL_MAX) & (z0 <= z1)
            cx, cy, lo, hi = (np.where(use, v, 0) for v in (cx, cy, z0, z1))
            f = np.searchsorted(keys, cell_keys(np.stack([cx, cy, lo], axis=1)), side="left")
            l = np.searchsorted(keys, cell_keys(np.stack([cx, cy, hi], axis=1)), side="right")
            k = 3 * (a + 1) + (b + 1)
            first[:, k], last[:, k] = np.where(use, f, 0), np.where(use, l, 0)
    return order, first, last


def walk_pairs(ref, queries, r):
    """Chunks of the walk's candidate pairs: (query (m,), original reference index (m,), d2 (m,) with +inf where not within reach), the
    pairs of a query adjacent and in walk order."""
    ref, queries, r, r2 = _checked(ref, queries, r)
    order, first, last = walk_intervals(ref, queries, r)
    p, q = ref.astype(F), queries.astype(F)
    lens = (last - first).reshape(-1)
    before = np.r_[0, np.cumsum(lens.reshape(-1, 9).sum(axis=1))]            # pairs of the queries in front of each one
    s = 0
    while s < len(queries):
        e = max(s + 1, int(np.searchsorted(before, before[s] + PAIRS, side="right")) - 1)
        ln, fs = lens[9 * s:9 * e], first[s:e].reshape(-1)
        starts = np.cumsum(ln) - ln
        slot = np.repeat(np.arange(len(ln)), ln)
        pos = fs[slot] + (np.arange(int(ln.sum())) - starts[slot])
        qq, at = s + slot // 9, order[pos]
        d2 = _d2(q[qq], p[at])
        with np.errstate(invalid="ignore"):
            yield qq, at, np.where(d2 <= r2, d2, np.inf)
        s = e


def walk_nearest(ref, queries, r):
    """nearest() by the walk; also the number of candidates examined."""
    best, index, examined = np.full(len(queries), np.inf), np.full(len(queries), -1, dtype=np.int64), 0
    for qq, at, d2 in walk_pairs(ref, queries, r):
        examined += len(qq)
        if len(qq) == 0:
            continue
        heads = np.flatnonzero(np.r_[True, qq[1:] != qq[:-1]])
        owner = qq[heads]
        m = np.minimum.reduceat(d2, heads)
        attains = np.isfinite(d2) & (d2 == np.repeat(m, np.diff(np.r_[heads, len(qq)])))
        lowest = np.minimum.reduceat(np.where(attains, at, np.iinfo(np.int64).max), heads)
        best[owner] = m
        index[owner] = np.where(np.isfinite(m), lowest, -1)
    return best, index, examined


def walk_counts(ref, queries, r, cap):
    out = np.zeros(len(queries), dtype=np.int64)
    for qq, at, d2 in walk_pairs(ref, queries, r):
        out += np.bincount(qq[np.isfinite(d2)], minlength=len(out))
    return np.minimum(out, cap).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the sums and the scores
def cloud_sums(d2, t2, r2):
    """[found, sum floor(sqrt(d2) 2^20) over the found, the counts of d2 <= t2[k]] as Python integers; found = finite, d2 taken into
    [0, r2] for the distance."""
    d2 = np.asarray(d2, F).reshape(-1)
    assert len(t2) <= 8 and all(0.0 < t <= r2 for t in t2) and 0.0 < r2 <= MAX_RADIUS ** 2
    found = np.isfinite(d2)
    inside = np.minimum(np.maximum(d2[found], 0.0), F(r2))
    fixed = np.floor(np.sqrt(inside) * SCALE).astype(np.int64)
    return [int(found.sum()), sum(int(v) for v in fixed)] + [int((d2[found] <= F(t)).sum()) for t in t2]


def cloud_scores(pred, truth, thresholds=(0.05, 0.1, 0.2, 0.5), search=nearest):
    """metrics.cloud_scores on (n, 3) float32 arrays; search: nearest (brute force) or walk_nearest."""
    th = [float(t) for t in thresholds]
    assert 1 <= len(th) <= 8 and all(0.0 < t <= MAX_RADIUS for t in th) and all(b > a for a, b in zip(th, th[1:]))
    radius, t2 = th[-1], [t * t for t in th]
    sums = np.array([cloud_sums(search(ref, queries, radius)[0], t2, radius * radius) for queries, ref in ((pred, truth), (truth, pred))], dtype=np.int64)
    s = sums.astype(F)
    total = np.array([len(pred), len(truth)], dtype=F)
    with np.errstate(all="ignore"):
        share = s[:, 2:] / total[:, None]
        a, c = share[0], share[1]
        mean = s[:, 1] / (F(SCALE) * s[:, 0])
        return {"accuracy": a, "completeness": c, "fscore": (2.0 * a * c) / (a + c), "found": s[:, 0] / total, "mean_accuracy": mean[0],
                "mean_completeness": mean[1], "chamfer": mean[0] + mean[1], "sums": sums}


# ------------------------------------------------------------------------------------------------ inputs the CPU and the GPU tests share
STEP = 0.125                            # every coordinate below is a multiple of 1/8: each d2 is exact, in fp32 and in fp64
LATTICE_RADIUS = 0.5                    # four steps: d2 == r2 at an offset of (4, 0, 0) steps, r2 + 1/64 at (4, 1, 0)


def edge_coordinate(sign):
    """A multiple of 1/8 whose cell at LATTICE_RADIUS is +(2^20 - 2) (sign > 0) or -(2^20 - 2), exact in fp32."""
    c = float(cell_edge(LATTICE_RADIUS))
    v = np.ceil(REF_MAX * c / STEP) * STEP if sign > 0 else -np.floor(REF_MAX * c / STEP) * STEP
    assert np.float32(v) == v and np.floor(v / c) == sign * REF_MAX
    return v


def lattice_case(seed=0, n=1000, nq=257):
    """ref (n, 3) and queries (nq, 3) float32 on the 1/8 lattice at r = 0.5, and the names of the special queries.  A dense block around
    the origin (cells of both signs, duplicates, many pairs at exactly r and one step beyond), and far from it, each alone:
      tie       two reference points mirrored about the query, the higher index at the lower key
      at_r      one reference point at exactly r           beyond    one at (4, 1, 0) steps: d2 = r2 + 1/64
      nothing   nothing anywhere near                      nan, inf  a coordinate that is not finite
      far       1e7 m away                                 outside   |q / c| >= 2^20 + 1
      top, bottom   beside reference points in the cells +(2^20 - 2) and -(2^20 - 2)      past_top   one metre beyond the top point"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(-12, 13, (n, 3)).astype(F) * STEP
    queries = rng.integers(-16, 17, (nq, 3)).astype(F) * STEP
    ref[1] = ref[0]                                                          # a duplicate
    ref[3] = ref[2] + [4 * STEP, 0, 0]                                       # a pair of reference points at exactly r of each other
    names = {}

    def put(name, at, q):
        names[name] = at
        queries[at] = q
    put("tie", 0, [10.0, 0.0, 0.0])
    ref[10], ref[5] = [10.0 - 2 * STEP, 0.0, 0.0], [10.0 + 2 * STEP, 0.0, 0.0]
    put("at_r", 1, [20.0, -7.0, 3.0])
    ref[20] = [20.0 + 4 * STEP, -7.0, 3.0]
    put("beyond", 2, [30.0, 5.0, -3.0])
    ref[21] = [30.0 + 4 * STEP, 5.0 + STEP, -3.0]
    put("nothing", 3, [50.0, 50.0, 50.0])
    put("nan", 4, [np.nan, 0.0, 0.0])
    put("inf", 5, [0.0, -np.inf, 0.0])
    put("far", 6, [1e7, 0.0, 0.0])
    top, bottom = edge_coordinate(+1), edge_coordinate(-1)
    ref[30], ref[31] = [top, top, top], [bottom, bottom, bottom]
    put("top", 7, [top + 2 * STEP, top, top])
    put("bottom", 8, [bottom, bottom - 3 * STEP, bottom])
    put("past_top", 9, [top + 1.0, top, top])
    put("outside", 10, [(HALF + 2) * float(cell_edge(LATTICE_RADIUS)), 0.0, 0.0])
    queries[11] = ref[0]                                                     # a query on a duplicate pair: d2 = 0, the lower index
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(F), ref)                              # nothing was rounded
    return ref32, queries.astype(np.float32), names


def one_cell_case(seed=1, n=1000, nq=257):
    """All n reference points in cell (0, 0, 0) at r = 0.5 (coordinates 0 .. 3/8: 64 positions, so every one is a stack of duplicates)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 4, (n, 3)) * STEP).astype(np.float32), (rng.integers(-8, 12, (nq, 3)) * STEP).astype(np.float32)
