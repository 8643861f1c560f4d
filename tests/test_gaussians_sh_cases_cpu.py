"""The hand-made cases of tests/gaussians_sh_cases.py reach the clauses they name: checked here on the CPU, so that the GPU file
(tests/test_gaussians_sh_kernels_gpu.py) compares the kernels' bits on inputs that are known to go where they should."""
import numpy as np
import pytest

import gaussians_sh_cases as sc
import gaussians_sh_reference as gs

F = np.float32


def _sound(c):
    """What every case holds: the camera centres well away, a definition without NaN (bit equality means something), drawn colours that
    clamp and drawn colours that do not, and a partial buffer whose other columns would poison a kernel that read them."""
    assert c.clause
    assert c.pts.shape == (c.n, 4) and c.mats.shape == (c.V, c.nmat, 12) and c.sh.shape == (c.n, gs.terms(c.L) - 1, 3)
    assert c.count.dtype == np.int32 and c.offsets.dtype == np.int64 and c.count.shape == c.offsets.shape == (c.V, c.n)
    assert float(sc.distances(c).min()) > 1.0
    assert c.E >= 1 and c.partial.shape == (c.E, 10) and np.isnan(c.partial[:, 3:]).all() and not np.isnan(c.partial[:, :3]).any()
    want = sc.definition(c)
    for k in ("colours", "g", "d_colour", "d_sh", "d_xyz_dir"):
        assert not np.isnan(getattr(want, k)).any(), k
    return want


def _mixed(c, want):
    drawn = want.colours[c.count > 0]
    assert (drawn == 0).any() and (drawn > 0).any()


# ------------------------------------------------------------------------------------------------ 1
def test_the_sizes_reach_every_count_of_single_floats():
    for L in (1, 3):
        assert {sc.last_block(L, n)[1] for n in sc.SIZES} == {0, 1, 2, 3}
    assert {sc.last_block(2, n)[1] for n in sc.SIZES} == {0}                            # a row of 24 floats is six whole pieces
    assert sc.last_block(1, 1) == (2, 1)
    for n in (200, 300):                                                                # gs.fit_problem's and gs.seeded_case's sizes reach none
        assert {sc.last_block(L, n)[1] for L in sc.DEGREES} == {0}
    assert {(n + 255) // 256 for n in sc.SIZES} == {1, 2, 3}


@pytest.mark.parametrize("L", sc.DEGREES)
def test_the_size_cases_are_sound(L):
    for n in sc.SIZES:
        c = sc.size_case(L, n)
        assert (c.L, c.n, c.V, c.nmat) == (L, n, 2, 2) and c.ids is not None and c.active == L
        want = _sound(c)
        _mixed(c, want)
        assert (c.count[:, -1] > 0).all() and want.d_sh[-1, -1].all()                   # the last block's last three floats are read and count
        if n > 3:
            assert set(c.ids.tolist()) == {0, 1} and set(c.count.reshape(-1).tolist()) == {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("L,active", sc.ACTIVE)
def test_the_active_degree_cases_hide_the_coefficients_that_take_no_part(L, active):
    c = sc.active_case(L, active)
    Ka = gs.terms(active)
    assert c.n == 259 and c.active == active and np.isnan(c.sh[:, Ka - 1:]).all() and not np.isnan(c.sh[:, :Ka - 1]).any()
    assert np.isnan(c.sh).any() == (active < L)
    want = _sound(c)
    _mixed(c, want)
    assert not want.d_sh[:, Ka - 1:].any() and not np.signbit(want.d_sh[:, Ka - 1:]).any()
    assert want.d_colour.any() and (want.d_sh.any(), want.d_xyz_dir.any()) == (active > 0, active > 0)
    if active == 0:                                                                     # the rule is max(0, colour) where drawn
        drawn = np.broadcast_to((c.count > 0)[:, :, None], want.colours.shape)
        assert np.array_equal(want.colours, np.where(drawn, np.maximum(c.colour, 0)[None], 0).astype(F))


# ------------------------------------------------------------------------------------------------ 3
def test_a_view_draws_nothing_of_a_workgroup_and_nothing_at_all():
    a, b = sc.undrawn_cases()
    assert (a.n, a.V) == (513, 3)
    want = _sound(a)
    _mixed(a, want)
    assert not a.count[1, 256:512].any() and (a.count[0, 256:512] > 0).any() and (a.count[2, 256:512] > 0).any()
    assert (a.count[1, :256] > 0).any() and a.count[1, 512] > 0                          # view 1's other workgroups fetch
    assert not want.colours[1, 256:512].any() and not np.signbit(want.colours[1, 256:512]).any()
    assert want.colours[1, :256].any() and want.colours[1, 512].any() and want.colours[0, 256:512].any()
    assert not b.count.any() and b.E == a.E and b.offsets is a.offsets and b.partial is a.partial
    zero = sc.definition(b)
    for k in ("colours", "d_colour", "d_sh", "d_xyz_dir"):
        v = getattr(zero, k)
        assert not v.any() and not np.signbit(v).any(), k
    assert not zero.ok.any()


# ------------------------------------------------------------------------------------------------ 4
def test_the_ids_cases():
    wild, clipped, null = sc.ids_cases()
    assert wild.nmat == 3 and set(wild.ids.tolist()) == set(sc.IDS.tolist()) and set(clipped.ids.tolist()) == {0, 1, 2}
    assert wild.ids.min() >= -3 and wild.ids.max() <= wild.nmat + 4
    a, b = _sound(wild), _sound(clipped)
    _mixed(wild, a)
    for k in ("colours", "d_colour", "d_sh", "d_xyz_dir"):
        assert np.array_equal(getattr(a, k).view(np.int32), getattr(b, k).view(np.int32)), k
    # an unclamped id would read another matrix: the nearest rows of the table differ
    for i in (-3, 7):
        rows = wild.ids == i
        assert rows.sum() > 10 and (wild.count[:, rows] > 0).any()
    assert null.nmat == 1 and null.ids is None
    _mixed(null, _sound(null))


# ------------------------------------------------------------------------------------------------ 5
def test_the_clamp_case_sits_on_the_edge():
    c = sc.clamp_case()
    want = _sound(c)
    assert (c.count[:, :7] > 0).all() and not c.sh[:4].any()
    bits = lambda a: np.asarray(a, dtype=F).view(np.int32)
    assert c.colour[3, 0] < 0 and abs(c.colour[3, 0]) < np.finfo(F).tiny                # subnormal, and not flushed by numpy
    for v in range(c.V):
        assert (bits(want.colours[v, 0]) == 0).all()                                    # +0 + (B 0) stays +0: not below zero, kept
        assert not want.colours[v, 1].any()                                             # -0 is not below zero either: it passes
        assert (bits(want.colours[v, 2]) == 0).all() and (bits(want.colours[v, 3]) == 0).all()   # just below: cut to +0
        for row in (4, 5, 6):
            cut = row - 4
            assert want.colours[v, row, cut] == 0 and (np.delete(want.colours[v, row], cut) > 0).all()
    # the backward: the gradient passes at +0 and -0, and is cut just below zero and in the one channel of rows 4 .. 6
    total = want.g[:, :7].sum(axis=0)
    assert want.ok[:, :7].all() and (want.g[:, :7] != 0).all() and (total != 0).all()
    assert (want.d_colour[:2] != 0).all() and not want.d_colour[2:4].any()
    for row in (4, 5, 6):
        cut = row - 4
        assert want.d_colour[row, cut] == 0 and (np.delete(want.d_colour[row], cut) != 0).all()
        assert not want.d_sh[row, :, cut].any() and np.delete(want.d_sh[row], cut, axis=1).all()


# ------------------------------------------------------------------------------------------------ 6
def test_each_spoiled_table_falsifies_one_guard_at_its_pairs_only():
    clean, spoiled = sc.spoiled_cases()
    assert (clean.n, clean.V) == (257, 2) and tuple(spoiled) == sc.GUARDS
    want = _sound(clean)
    _mixed(clean, want)
    E = clean.E
    assert clean.offsets[sc.FIRST] == 0 and clean.offsets[sc.LAST] == E - clean.count[sc.LAST] and clean.count[sc.LAST] == 2
    assert want.ok[sc.FIRST] and want.ok[sc.LAST] and want.g[sc.FIRST].any() and want.g[sc.LAST].any()
    for name, (c, pairs) in spoiled.items():
        assert c.E == E and c.partial is clean.partial
        got = _sound(c)
        differ = {tuple(p) for p in np.argwhere(got.ok != want.ok).tolist()}
        changed = {tuple(p) for p in np.argwhere((c.count != clean.count) | (c.offsets != clean.offsets)).tolist()}
        assert changed == set(pairs), name
        # what a kernel that followed the value would read lies no more than two rows outside the partial buffer
        for p in pairs:
            cnt, off = int(c.count[p]), int(c.offsets[p])
            assert off >= -2 and off + max(cnt, 0) <= E + 2, (name, p)
        if name == "offset 0 and E - count":
            assert not differ and got.ok[sc.FIRST] and got.ok[sc.LAST]
            assert all(got.ok[p] and not np.array_equal(got.g[p], want.g[p]) for p in pairs)
            assert sorted({int(c.offsets[p]) for p in pairs}) == [0, E - 2]
            continue
        assert differ == set(pairs), name
        assert all(want.ok[p] and not got.ok[p] and not got.g[p].any() for p in pairs), name
        if name != "last count + 1":
            assert got.ok[sc.FIRST] and got.ok[sc.LAST], name
        # exactly one of the guard's terms is false
        for p in pairs:
            cnt, off = int(c.count[p]), int(c.offsets[p])
            assert [cnt > 0, off >= 0, off <= E - cnt].count(False) == 1, (name, p)
        drawn = sc.definition(c).colours
        for p in pairs:                                                                 # the colour kernel reads the count alone
            assert drawn[p].any() == (c.count[p] > 0), (name, p)
    assert {p[1] // 256 for p in sc.SPOILED} == {0, 1} and {p[0] for p in sc.SPOILED} == {0, 1}


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("n", sc.TILE_SIZES)
def test_the_tile_cases_put_every_entry_on_tile_zero_of_both_views(n):
    t = sc.tile_case(n)
    NT = len(t.ranges) // 2
    assert NT == 6 and t.E == 2 * n and t.ranges[0].tolist() == [0, n] and t.ranges[NT].tolist() == [n, 2 * n]
    assert not np.delete(t.ranges, [0, NT], axis=0).any()
    assert t.offsets[1, 0] == n and t.colours.shape == (2, n, 3) and not np.array_equal(t.colours[0], t.colours[1])
    assert {-(-n // 256) for n in sc.TILE_SIZES} == {1, 2, 3}


def test_the_tile_case_tells_the_views_colours_apart_and_its_spoiled_tables_are_out_of_range():
    t = sc.tile_case(257)
    a = sc.blend_definition(t, t.colours, t.values, t.order, t.ranges)
    b = sc.blend_definition(t, t.same, t.values, t.order, t.ranges)
    for k in ("rgb", "depth", "alpha", "state", "partial"):
        assert not np.isnan(getattr(a, k)).any(), k
    assert np.array_equal(a.rgb[0], b.rgb[0]) and not np.array_equal(a.rgb[1], b.rgb[1])   # a colour stride of 0 would show in view 1
    assert np.array_equal(a.partial[:257], b.partial[:257]) and not np.array_equal(a.partial[257:], b.partial[257:])
    assert (a.partial[:, :3].any(axis=1).sum() >= 0.8 * t.E) and a.alpha.max() < 1         # no pixel finishes: every batch is walked
    values, order, ranges = t.spoiled
    E = t.E
    assert ((values < 0) | (values >= t.n)).sum() > 50 and ((order < 0) | (order >= E)).sum() > 50
    assert values.min() >= -5 and values.max() <= t.n and order.min() >= -1 and order.max() <= E
    assert ranges[1].tolist() == [-4, 3] and ranges[2].tolist() == [0, E + 1] and not sc.usable(ranges, E)[1:3].any()
    s = sc.blend_definition(t, t.colours, values, order, ranges)
    for k in ("rgb", "depth", "alpha", "state", "partial"):
        assert not np.isnan(getattr(s, k)).any(), k
    assert not np.array_equal(s.rgb, a.rgb) and not np.array_equal(s.partial, a.partial) and s.partial.any()
