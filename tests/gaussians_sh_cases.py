"""Hand-made inputs for the two harmonics kernels of csrc/gaussians_sh.hip and the three `_views` blends, each naming the clause of the
kernels it reaches.  numpy only: tests/test_gaussians_sh_cases_cpu.py asserts, without a GPU, that every case reaches its clause, and
tests/test_gaussians_sh_kernels_gpu.py runs the kernels on the cases and compares the bits with `definition`.

The harmonics kernels need no render: count, offsets and the partial buffer are made by hand.  A workgroup moves its 256 coefficient rows
through LDS as whole 16-byte pieces and then single floats (`last_block`); a row is 9, 24 or 45 floats, so single floats exist only at
degrees 1 and 3 and only where (n mod 256) mod 4 != 0."""
import functools
from types import SimpleNamespace

import numpy as np

import gaussians_bwd_reference as gb
import gaussians_reference as gr
import gaussians_sh_reference as gs

F = np.float32
NAN = F(np.nan)
DEGREES = (1, 2, 3)
SIZES = (1, 2, 3, 255, 256, 257, 258, 259, 513)
ACTIVE = tuple((L, a) for L in DEGREES for a in range(L + 1))                          # nine pairs
IDS = np.array([-3, 0, 1, 2, 7], dtype=np.int32)                                      # -3 -> 0, 7 -> nmat - 1
TILE_SIZES = (255, 256, 257, 513)
TILE_HW = (17, 33)


def row_floats(L):
    """Floats of a Gaussian's coefficients: 9, 24, 45."""
    return 3 * (gs.terms(L) - 1)


def last_block(L, n):
    """(whole 16-byte pieces, single floats) of the last workgroup's rows."""
    total = ((n - 1) % 256 + 1) * row_floats(L)
    return total // 4, total % 4


# ------------------------------------------------------------------------------------------------ the builder
def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def index(c, count):
    """Sets c.count (V, n) int32, c.offsets (their exclusive sum, int64) and c.E."""
    c.count = np.ascontiguousarray(count, dtype=np.int32)
    ends = np.cumsum(c.count.reshape(-1).astype(np.int64))
    c.offsets = (ends - c.count.reshape(-1)).reshape(c.count.shape)
    c.E = int(ends[-1])
    return c


def fill_partial(c, seed):
    """c.partial (E, 10): normal in the colour columns, NaN in columns 3 .. 9, which the harmonics' rule does not read."""
    assert c.E > 0, "the backward's entry point takes 1 .. 2^31 - 1 entries"
    c.partial = np.full((c.E, gb.SUMS), NAN, F)
    c.partial[:, :3] = np.random.default_rng(seed).normal(size=(c.E, 3)).astype(F)
    return c


def case(L, n, V, nmat, seed, ids="seeded", active=None, clause=""):
    """Positions uniform in [-1, 1]^3; every (view, matrix) a seeded rotation with a translation of norm in [3, 5], so the camera centre
    is at least 3 - sqrt(3) > 1.2 from every Gaussian; colour uniform in (-40, 255), sh in (-50, 50); count in 0 .. 3 (the last Gaussian's
    at least 1) with its offsets;
    partial normal in the colour columns and NaN elsewhere; the points packed.  ids: "seeded" (0 .. nmat - 1), None or an array."""
    rng = np.random.default_rng(seed)
    c = SimpleNamespace(L=L, n=n, V=V, nmat=nmat, seed=seed, active=L if active is None else active, clause=clause)
    c.xyz = rng.uniform(-1.0, 1.0, (n, 3)).astype(F)
    c.mats = np.zeros((V, nmat, 12), F)
    for v in range(V):
        for m in range(nmat):
            t = rng.normal(size=3)
            t = t / np.linalg.norm(t) * rng.uniform(3.0, 5.0)
            c.mats[v, m] = np.concatenate([_rotation(rng), t[:, None]], axis=1).reshape(12)
    c.colour = rng.uniform(-40.0, 255.0, (n, 3)).astype(F)
    c.sh = rng.uniform(-50.0, 50.0, (n, gs.terms(L) - 1, 3)).astype(F)
    count = rng.integers(0, 4, (V, n))
    count[:, n - 1] = np.maximum(count[:, n - 1], 1)                                   # every view reads the last block's last floats
    index(c, count)
    c.ids = rng.integers(0, nmat, n).astype(np.int32) if isinstance(ids, str) else (None if ids is None else np.asarray(ids, dtype=np.int32))
    assert c.ids is not None or nmat == 1
    c.pts = gr.pack(c.xyz, np.zeros((n, 3), np.uint8))
    if c.E:
        fill_partial(c, seed + 1)
    return c


def definition(c):
    """The definition's answer on a case: colours (V, n, 3), the gathered g and its mask ok, d_colour, d_sh, d_xyz_dir."""
    cols = gs.colours(c.xyz, c.ids, c.mats, c.count, c.colour, c.sh, c.active)
    g, ok = gs.gather(c.partial, c.count, c.offsets)
    d_colour, d_sh, d_dir = gs.colours_backward(c.xyz, c.ids, c.mats, ok, g, c.colour, c.sh, c.active)
    return SimpleNamespace(colours=cols, g=g, ok=ok, d_colour=d_colour, d_sh=d_sh, d_xyz_dir=d_dir)


def distances(c):
    """|p - c| of every (view, Gaussian), (V, n)."""
    which = np.zeros(c.n, np.int64) if c.ids is None else np.clip(c.ids.astype(np.int64), 0, c.nmat - 1)
    return np.stack([gs.directions(c.xyz, c.mats[v][which])[1] for v in range(c.V)])


def mixed(c):
    """Among the drawn pairs some colour channels clamp to 0 and some do not."""
    drawn = definition(c).colours[c.count > 0]
    return bool((drawn == 0).any() and (drawn > 0).any())


def last_floats_count(c):
    """The last coefficient of the last Gaussian reaches an unclamped colour in every channel: its three floats, the last block's last,
    have a gradient."""
    return bool(definition(c).d_sh[-1, -1].all())


def first_mixed(build, seed):
    """The first case from seed, seed + 1, ... with `mixed` and `last_floats_count`: one or two Gaussians rarely show all of it at any
    one seed."""
    for s in range(seed, seed + 500):
        c = build(s)
        if mixed(c) and last_floats_count(c):
            return c
    raise AssertionError("no seed mixes clamped and free colours")


# ------------------------------------------------------------------------------------------------ 1: sizes
@functools.lru_cache(maxsize=None)
def size_case(L, n):
    pieces, singles = last_block(L, n)
    return first_mixed(lambda s: case(L, n, 2, 2, s, clause=f"stage_rows / store_rows: the last block is {pieces} pieces and {singles} single floats"),
                       1000 * L + n)


# ------------------------------------------------------------------------------------------------ 2: the active degree
@functools.lru_cache(maxsize=None)
def active_case(L, active):
    """n = 259 (a last block with single floats at L = 1 and 3); the coefficients at and above Ka are NaN, since they take no part."""
    c = case(L, 259, 2, 2, 2000 + 10 * L + active, active=active, clause=f"sh_sum and the backward's `k < Ka` at Ka = {gs.terms(active)} of {gs.terms(L)}")
    c.sh[:, gs.terms(active) - 1:] = NAN
    return c


# ------------------------------------------------------------------------------------------------ 3: nothing drawn
@functools.lru_cache(maxsize=None)
def undrawn_cases(L=3):
    """n = 513, V = 3: view 1 draws nothing of Gaussians 256 .. 511 (the workgroup skips the fetch); and the same with every count 0,
    which keeps the first one's offsets, partial and E (the backward refuses E = 0)."""
    a = case(L, 513, 3, 2, 3000 + L, clause="gauss_sh_colour: __syncthreads_or(drawn) is false for workgroup 1 of view 1")
    count = a.count.copy()
    count[1, 256:512] = 0
    fill_partial(index(a, count), a.seed + 1)
    b = SimpleNamespace(**vars(a))
    b.count = np.zeros_like(a.count)
    b.clause = "every count 0: with_partials returns at once everywhere, no workgroup fetches"
    return a, b


# ------------------------------------------------------------------------------------------------ 4: ids
@functools.lru_cache(maxsize=None)
def ids_cases(L=2, n=259):
    """nmat = 3 with ids from {-3, 0, 1, 2, 7} and the same with the ids clipped; nmat = 1 with no ids at all.  Every id lies within
    [-3, nmat + 4]."""
    wild = case(L, n, 2, 3, 4000 + L, clause="sh_point: ids below 0 and at or above nmat are clamped")
    wild.ids = np.random.default_rng(4100).choice(IDS, n).astype(np.int32)
    clipped = SimpleNamespace(**vars(wild))
    clipped.ids = np.clip(wild.ids, 0, wild.nmat - 1).astype(np.int32)
    null = case(L, n, 2, 1, 4200 + L, ids=None, clause="sh_point: ids == NULL reads matrix 0 of every view")
    return wild, clipped, null


# ------------------------------------------------------------------------------------------------ 5: the clamp's edge
CLAMP_ZEROS = (0.0, -0.0, -1e-30, -1e-40)                                              # the last is subnormal in fp32


@functools.lru_cache(maxsize=None)
def clamp_case(L=2, n=16):
    """Rows 0 .. 3: colour +0.0, -0.0, -1e-30 and -1e-40 in every channel with zero coefficients (c < 0 cuts the last two only); rows
    4 .. 6: channel row - 4 far below zero, the other two far above, with small coefficients.  All of them are drawn in every view."""
    c = case(L, n, 2, 2, 5000 + L, clause="`c < 0 ? 0 : c` and the backward's `c < 0 ? 0 : g` at zero, minus zero and just below")
    for row, value in enumerate(CLAMP_ZEROS):
        c.colour[row] = F(value)
        c.sh[row] = 0
    for row in (4, 5, 6):
        c.colour[row] = 300.0
        c.colour[row, row - 4] = -300.0
        c.sh[row] = c.sh[row] * F(0.1)
    count = c.count.copy()
    count[:, :7] = 2
    fill_partial(index(c, count), c.seed + 1)
    return c


# ------------------------------------------------------------------------------------------------ 6: spoiled count and offsets
SPOILED = ((0, 3), (0, 255), (0, 256), (1, 0), (1, 255))          # (view, Gaussian): both views, both workgroups, the lone last lane
FIRST, LAST = (0, 0), (1, 256)                                    # the pairs whose offsets are 0 and E - count: they must still count
GUARDS = ("count 0", "count -2", "offset -1", "offset E - count + 1", "offset E", "last count + 1", "offset 0 and E - count")


@functools.lru_cache(maxsize=None)
def spoiled_cases(L=3):
    """n = 257, V = 2.  The clean case and, per guard term of with_partials, one whose table falsifies that term alone at SPOILED (the
    last one at LAST only): name -> (case, pairs).  The pairs have count 2, so no spoiled value points more than two rows outside the
    partial buffer.  "offset 0 and E - count" moves SPOILED to the two boundaries that still count."""
    clean = case(L, 257, 2, 2, 6000 + L, clause="with_partials: cnt <= 0, off < 0, off > E - cnt")
    count = clean.count.copy()
    for pair in SPOILED + (FIRST, LAST):
        count[pair] = 2
    fill_partial(index(clean, count), clean.seed + 1)
    E = clean.E
    out = {}
    for name in GUARDS:
        c = SimpleNamespace(**vars(clean))
        c.count, c.offsets, c.clause = clean.count.copy(), clean.offsets.copy(), f"with_partials: {name}"
        pairs = (LAST,) if name == "last count + 1" else SPOILED
        for k, pair in enumerate(pairs):
            if name == "count 0":
                c.count[pair] = 0
            elif name == "count -2":
                c.count[pair] = -2
            elif name == "offset -1":
                c.offsets[pair] = -1
            elif name == "offset E - count + 1":
                c.offsets[pair] = E - 2 + 1
            elif name == "offset E":
                c.offsets[pair] = E
            elif name == "last count + 1":
                c.count[pair] = 3
            else:
                c.offsets[pair] = (0, E - 2)[k % 2]
        out[name] = (c, pairs)
    return clean, out


# ------------------------------------------------------------------------------------------------ 7: one tile at the blends' batch edges
def _spoil(values, order, ranges, n):
    """As tests/test_gaussians_bwd_gpu.py spoils them: values outside the cloud, positions outside [0, E), ranges outside [0, E]."""
    values, order, ranges = values.copy(), order.copy(), ranges.copy()
    E = len(values)
    values[::7], values[3::11] = -5, n
    order[::5], order[2::9] = -1, E
    ranges[1], ranges[2] = (-4, 3), (0, E + 1)
    return values, order, ranges


def usable(ranges, E):
    """The ranges as the blends read them: one outside [0, E] or reversed is an empty tile."""
    bad = (ranges[:, :1] < 0) | (ranges[:, 1:] > E) | (ranges[:, :1] > ranges[:, 1:])
    return np.where(bad, 0, ranges).astype(np.int32)


@functools.lru_cache(maxsize=None)
def tile_case(n):
    """tests/test_gaussians_bwd_gpu.py's batch-edge case seen by two views through the same matrix: n faint Gaussians on tile 0 of a
    17 x 33 image, none of whose pixels finishes, so each view's tile 0 is walked through all its n entries in batches of 256.  colour
    (n, 3) is one colour per Gaussian, colours (2, n, 3) differ between the views."""
    rng = np.random.default_rng(n)
    pts, cov, op = gr.flat_case(rng.uniform(5.0, 11.0, (n, 2)), 0.5, opacity=rng.uniform(0.004, 0.02, n).astype(F), z=rng.uniform(60.0, 180.0, n).astype(F),
                                seed=n)
    t = SimpleNamespace(n=n, V=2, hw=TILE_HW, cov=cov, op=op, mats=np.stack([gr.FLAT, gr.FLAT]), cam=gr.FLAT_CAM)
    t.xyz = gr.unpack(pts)[0]
    t.proj = gr.project(t.xyz, cov, op, None, t.mats, t.cam, t.hw)
    _, t.values, t.order, t.ranges, t.offsets = gb.bin_with_order(t.proj, t.hw)
    t.E = len(t.values)
    t.colour = rng.uniform(0.0, 255.0, (n, 3)).astype(F)
    t.colours = np.stack([t.colour, rng.uniform(0.0, 255.0, (n, 3)).astype(F)])
    t.same = np.stack([t.colour, t.colour])
    H, W = t.hw
    t.ups = (rng.normal(size=(2, 3, H, W)).astype(F), (rng.normal(size=(2, H, W)) * 0.05).astype(F), rng.normal(size=(2, H, W)).astype(F))
    t.spoiled = _spoil(t.values, t.order, t.ranges, n)
    return t


def blend_definition(t, cols, values, order, ranges):
    """gs.blend_views and gs.blend_bwd_views on a tile case: rgb, depth, alpha, state, partial."""
    rgb, depth, alpha, state = gs.blend_views(t.proj, cols, values, usable(ranges, t.E), t.hw)
    partial = gs.blend_bwd_views(t.proj, cols, values, order, ranges, t.offsets, t.hw, state, *t.ups)
    return SimpleNamespace(rgb=rgb, depth=depth, alpha=alpha, state=state, partial=partial)
