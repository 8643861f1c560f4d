"""The hand-made cases of tests/gaussians_core_cases.py reach the clauses they name, the fp32 definitions hold for full covariances against
the float64 textbook, and the cases tell mutated definitions apart: all on the CPU, so that the GPU file
(tests/test_gaussians_core_kernels_gpu.py) compares the kernels' bits on inputs known to go where they should and known to be sharp.
`pytest -s` prints the census.  A mutant is a copy of a definition's source with one guard or one index changed, compiled inside the
test; no kernel is ever built with a guard removed."""
import inspect
import textwrap

import numpy as np
import pytest
import torch

import gaussians_bwd_reference as gb
import gaussians_core_cases as cc
import gaussians_reference as gr
from test_gaussians_bwd_cpu import MEASURED, _upstream
from test_gaussians_cpu import FP32_BOUND

F, D = np.float32, np.float64
GRADS = ("d_xyz", "d_cov", "d_opacity", "d_colour")
# cc.full_case((40, 56), 1, False) against float64 autograd, measured on the CPU as test_gaussians_bwd_cpu.MEASURED was: the 298 ordinary
# Gaussians stay inside the existing 4 x MEASURED of every group (cov 2.16e-6 of 4.08e-6).  With the needle (scales 0.01, 0.01, 1.5 m) the
# covariance gradients differ by 6.22e-6 of the group's largest, which is the needle's own: its footprint is so elongated that
# a c - b^2 cancels by a factor of 65 (printed and asserted below), a loss of fp32's, not of the rule's.  The bound is four times the measured
# value, as for the existing constants; they are not widened, and xyz, opacity and colour keep theirs with the needle in.
MEASURED_NEEDLE = {"cov": 6.22e-6}


def _mutant(fn, old, new, module):
    """fn with the one occurrence of `old` in its source replaced by `new`, compiled in a copy of its module's names."""
    src = textwrap.dedent(inspect.getsource(fn))
    assert src.count(old) == 1, (fn.__name__, old, src.count(old))
    names = dict(vars(module))
    exec(compile(src.replace(old, new), f"<{fn.__name__} with {new!r} for {old!r}>", "exec"), names)
    return names[fn.__name__]


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _told_apart(run, mutant_run, cases):
    """The names of the cases on which the mutant's answer is not the definition's (an index a guard would have stopped counts too)."""
    names = []
    for name, case in cases.items():
        try:
            if not _same(run(case), mutant_run(case)):
                names.append(name)
        except IndexError:
            names.append(name)
    return names


# ------------------------------------------------------------------------------------------------ A
def _clamped(c, view):
    """Per Gaussian: x / z or y / z lies outside the limit the Jacobian is evaluated at (float64; the margin to the limit is asserted)."""
    which = np.zeros(c.n, np.int64) if c.ids is None else np.clip(c.ids.astype(np.int64), 0, c.nmat - 1)
    M = c.mats[view][which].astype(D).reshape(c.n, 3, 4)
    with np.errstate(all="ignore"):
        p = np.einsum("nij,nj->ni", M[:, :, :3], c.xyz.astype(D)) + M[:, :, 3]
        qx, qy = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    H, W = c.hw
    limx, limy = 1.3 * 0.5 * W / c.cam[0], 1.3 * 0.5 * H / c.cam[1]
    return (np.abs(qx) > limx * (1 + 1e-5)) | (np.abs(qy) > limy * (1 + 1e-5))


@pytest.mark.parametrize("hw,views", cc.FULL_SHAPES)
def test_full_covariances_are_full_drawn_and_clamped(hw, views):
    c, want = cc.full_case(hw, views), cc.full_definition((hw, views))
    assert c.cov.shape == (cc.FULL_N, 6) and (c.cov != 0).all() and np.isfinite(c.cov).all()                  # every entry of every Gaussian
    assert tuple(c.scales[0]) == cc.NEEDLE and tuple(c.scales[1]) == cc.PANCAKE and (want["count"][:, :2] > 0).all()
    which = np.clip(c.ids, 0, c.nmat - 1)
    shown = np.ones((views, c.n), bool)
    shown[0] = which != 1                                                               # view 0 holds the zero matrix for id 1: a clause of B
    drawn = want["count"] > 0
    assert not drawn[~shown].any() and set(np.unique(c.ids).tolist()) == set(cc.IDS.tolist())
    clamped = sum(int((drawn[v] & _clamped(c, v)).sum()) for v in range(views))
    off = np.abs(c.cov[:, [1, 2, 4]]).min()
    print(f"A {hw} x {views}: {drawn[shown].mean():.3f} of the shown pairs drawn, {want['E']} entries, longest tile "
          f"{int((want['ranges'][:, 1] - want['ranges'][:, 0]).max())}, {clamped} drawn pairs with a clamped tx or ty, smallest |off-diagonal| {off:.2e}")
    assert drawn[shown].mean() >= 0.8 and clamped >= 5
    for k in ("partial",) + GRADS + ("rgb", "rgb8", "state"):
        assert np.isfinite(want[k]).all(), k
    assert all(want[k].any() for k in GRADS) and want["d_cov"][:, [1, 2, 4]].any(axis=0).all()


def test_the_flat_case_puts_257_full_covariances_on_one_tile():
    c, want = cc.flat_full_case(), cc.full_definition("flat")
    assert c.n == 257 and (c.cov != 0).all() and (want["count"] > 0).all()
    assert want["ranges"][0].tolist() == [0, 257] and want["walked"][0] == 257 and want["walked8"][0] == 257      # a second batch of one entry
    print(f"A flat: {want['E']} entries, tile 0 holds 257, alpha up to {want['alpha'].max():.3f}")


def test_the_definitions_hold_for_full_covariances_against_float64():
    hw = (40, 56)
    c = cc.full_case(hw, 1, False)
    got = gr.render(c.pts, c.cov, c.opacity, None, c.mats, c.cam, hw)
    want_rgb, want_alpha, near = gr.textbook_render(c.xyz, c.rgb, c.cov, c.opacity, c.mats[0, 0], c.cam, hw)
    keep = ~near
    e_rgb = np.abs(got["rgb"][0].astype(D) - want_rgb)[:, keep].max()
    e_alpha = np.abs(got["alpha"][0].astype(D) - want_alpha)[keep].max()
    print(f"A against float64: {int((got['count'] > 0).sum())} of {c.n} drawn, {near.mean():.4f} of the pixels excluded; rgb {e_rgb:.3e}, "
          f"alpha {e_alpha:.3e} (bound {FP32_BOUND:.3e})")
    assert near.mean() <= 0.05 and (got["count"] > 0).mean() >= 0.8
    assert e_rgb <= FP32_BOUND and e_alpha <= FP32_BOUND
    ups = _upstream(hw, near)
    out = gb.render_backward(c.xyz, c.rgb.astype(F), c.cov, c.opacity, None, c.mats, c.cam, hw, *ups)
    t64 = lambda a: torch.tensor(np.asarray(a, dtype=F).astype(D), requires_grad=True)
    tx, tc, tv, to = t64(c.xyz), t64(c.rgb), t64(c.cov), t64(c.opacity)
    r, d, a = gb.textbook(tx, tc, tv, to, c.mats, c.cam, hw)
    ((r * torch.tensor(ups[0].astype(D))).sum() + (d * torch.tensor(ups[1].astype(D))).sum() + (a * torch.tensor(ups[2].astype(D))).sum()).backward()
    ordinary = np.arange(c.n) >= 2                                                      # all but the needle and the pancake
    for name, mine, want in (("xyz", out["d_xyz"], tx.grad), ("cov", out["d_cov"], tv.grad), ("opacity", out["d_opacity"], to.grad),
                             ("colour", out["d_colour"], tc.grad)):
        want = want.numpy()
        err = np.abs(mine.astype(D) - want)[ordinary].max() / np.abs(want[ordinary]).max()
        whole = np.abs(mine.astype(D) - want).max() / np.abs(want).max()
        bound = 4 * MEASURED_NEEDLE.get(name, MEASURED[name])
        print(f"A against float64 autograd, {name}: largest gradient {np.abs(want).max():.4g}; relative difference {err:.3e} without the needle and "
              f"the pancake (bound {4 * MEASURED[name]:.3e}), {whole:.3e} with them (bound {bound:.3e})")
        assert np.abs(want).max() > 0 and err <= 4 * MEASURED[name] and whole <= bound, name
    A, B, C, _ = out["conic"][0, 0].astype(D)
    lost = A * C / (A * C - B * B)
    print(f"A: the needle's conic ({A:.3f}, {B:.3f}, {C:.3f}) has A C / (A C - B^2) = {lost:.1f}: its determinant loses that factor in fp32")
    assert lost > 30 and np.abs(tv.grad.numpy()[0]).max() == np.abs(tv.grad.numpy()).max()      # and its gradient is the group's largest


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("hw", [(16, 16), (40, 56)])
def test_each_drop_clause_drops_or_keeps_its_gaussian(hw):
    c = cc.drop_case(hw)
    proj = cc.project_case(c)
    count = proj["count"][0]
    for i, clause in enumerate(c.clauses):
        print(f"B {hw} {i:2d} count {count[i]:2d} rect {proj['rect'][0, i].tolist()}  {clause}")
        assert (count[i] > 0) == c.drawn[i], clause
        assert c.tiles[i] is None or not c.drawn[i] or count[i] == c.tiles[i], clause
    assert len(set(c.clauses)) == c.n and c.drawn.sum() >= 15 and (~c.drawn).sum() >= 20
    for k in ("uv", "conic", "depth", "rect"):
        assert not proj[k][0][~c.drawn].any() and np.isfinite(proj[k]).all(), k      # what is dropped stores zeros: nothing that is not a number
    kept, kept_rad, dropped, dropped_rad = cc.largest_kept_scale()
    print(f"B: the largest isotropic scale kept is {float(kept)!r} with rad {kept_rad}, the next one {float(dropped)!r} has rad {dropped_rad}")
    assert dropped == cc.up(kept) and kept_rad <= gr.MAX_RADIUS < dropped_rad
    below, above = c.clauses.index("mid^2 - det below the 0.1 floor"), c.clauses.index("mid^2 - det above the 0.1 floor")
    for i, sign in ((below, -1), (above, 1)):
        x, y, z = c.xyz[i].astype(D)
        J = np.array([[gr.FOCAL / z, 0, -gr.FOCAL * x / z ** 2], [0, gr.FOCAL / z, -gr.FOCAL * y / z ** 2]])
        s = c.cov[i].astype(D)
        c2 = J @ np.array([[s[0], s[1], s[2]], [s[1], s[3], s[4]], [s[2], s[4], s[5]]]) @ J.T + 0.3 * np.eye(2)
        gap = (0.5 * np.trace(c2)) ** 2 - np.linalg.det(c2) - 0.1
        print(f"B: {c.clauses[i]}: mid^2 - det - 0.1 = {gap:+.4f}")
        assert sign * gap > 1e-3                                                         # far more than fp32 rounding
    ids = c.ids.tolist()
    assert -3 in ids and c.nmat + 4 in ids and proj["uv"][0, c.clauses.index("id nmat + 4 is matrix nmat - 1"), 0] == F(10.5)


# ------------------------------------------------------------------------------------------------ C
def test_each_spoiled_key_table_falsifies_its_terms_and_silences_its_owner_only():
    clean, cases = cc.key_cases()
    keys, values, written = cc.keys_definition(clean)
    proj = cc.full_definition((cc.KEY_HW, cc.KEY_VIEWS))["proj"]
    want_keys, want_values, _ = gr.bin_entries(proj, clean.hw)
    order = np.argsort(keys, kind="stable")
    assert written.all() and np.array_equal(keys[order], want_keys) and np.array_equal(values[order], want_values)      # clean: gr.bin_entries
    assert {t for c, _ in cases.values() for t in c.terms} == set(cc.KEY_TERMS)
    for name, (c, o) in cases.items():
        assert cc.key_terms(c.rect, c.count, c.offsets, o, c.hw, c.E) == c.terms, name
        assert all(not cc.key_terms(c.rect, c.count, c.offsets, p, c.hw, c.E) for p in np.nonzero(clean.count.reshape(-1))[0] if p != o)
        k, v, w = cc.keys_definition(c)
        lo = int(clean.offsets.reshape(-1)[o])
        own = np.zeros(c.E, bool)
        own[lo:lo + int(clean.count.reshape(-1)[o])] = True
        print(f"C {name}: owner {o} falsifies {sorted(c.terms)}, {int((~w).sum())} entries not written")
        assert np.array_equal(w, ~own if c.terms else np.ones(c.E, bool)), name
        assert np.array_equal(k[w], keys[w]) and np.array_equal(v[w], values[w]), name
    last, o = cases["offset exactly E - count: accepted"]
    assert int(last.offsets.reshape(-1)[o]) == last.E - int(last.count.reshape(-1)[o])


KEY_GUARDS = {"x0 < 0": "if x0 < 0:", "x1 > TX": "if x1 > TX:", "y0 < 0": "if y0 < 0:", "y1 > TY": "if y1 > TY:",
              "area != c": "if (x1 - x0) * (y1 - y0) != c:", "at < 0": "if at < 0:", "at > E - c": "if at > E - c:"}
IMPLIED = {"c <= 0": "if c <= 0:", "x0 >= x1": "if x0 >= x1:", "y0 >= y1": "if y0 >= y1:"}


def test_the_key_cases_tell_every_mutated_guard_apart():
    clean, cases = cc.key_cases()
    tables = {name: c for name, (c, _) in cases.items()}
    tables["clean"] = clean
    run = lambda fn: (lambda c: fn(c.depth, c.rect, c.count, c.offsets, c.n, c.V, c.hw, c.E))
    for term, line in KEY_GUARDS.items():
        apart = _told_apart(run(cc.keys_raw), run(_mutant(cc.keys_raw, line, "if False:", cc)), tables)
        print(f"C without `{term}`: told apart by {apart}")
        assert apart and "clean" not in apart, term
    apart = _told_apart(run(cc.keys_raw), run(_mutant(cc.keys_raw, "if at > E - c:", "if at >= E - c:", cc)), tables)
    print(f"C with `at >= E - c`: told apart by {apart}")
    assert "offset exactly E - count: accepted" in apart
    # c <= 0 and the two `>=` are implied by the other terms (an empty or reversed rectangle has an area that is not a positive count, or
    # loops that do not run): a definition without one of them is the same function, which the cases confirm
    for term, line in IMPLIED.items():
        assert not _told_apart(run(cc.keys_raw), run(_mutant(cc.keys_raw, line, "if False:", cc)), tables), term


# ------------------------------------------------------------------------------------------------ D
def test_the_range_cases_are_sorted_and_shifted_as_they_say():
    cases = cc.range_cases()
    for name, (keys, E, tiles) in cases.items():
        assert len(keys) == E and (np.diff(keys) >= 0).all(), name
        got = cc.ranges_raw(keys, E, tiles)
        tile = keys >> 32
        want = np.zeros((tiles, 2), np.int32)
        for t in range(tiles):                                                         # by counting, not by neighbours
            at = np.nonzero(tile == t)[0]
            if len(at):
                want[t] = at[0], at[-1] + 1
        print(f"D {name}: E = {E}, tiles {int(tile.min())} .. {int(tile.max())} of {tiles}, {int((want[:, 1] > want[:, 0]).sum())} occupied")
        assert np.array_equal(got, want), name
    keys, E, tiles = cases["tiles below 0 in front and tiles >= tiles behind"]
    tile = keys >> 32
    assert (tile[:7] < 0).all() and (tile[-8:] >= tiles).all() and E > 512 and cc.ranges_raw(keys, E, tiles)[0, 0] == 7      # three workgroups
    assert cases["the first and the last tile, nothing between"][1] == 258 and cases["one entry"][1] == 1
    run = lambda fn: (lambda c: (fn(*c),))
    for line in ("if t < 0:", "if t >= tiles:"):
        apart = _told_apart(run(cc.ranges_raw), run(_mutant(cc.ranges_raw, line, "if False:", cc)), cases)
        print(f"D without `{line[3:-1]}`: told apart by {apart}")
        assert apart == ["tiles below 0 in front and tiles >= tiles behind"]


# ------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("hw,n", [((16, 16), n) for n in cc.TILE_SIZES] + [((17, 33), 60)])
def test_the_hand_made_tables_take_every_branch_of_the_blend_step(hw, n):
    t = cc.table_case(hw, n)
    counts, waves = cc.blend_trace(t)
    total = counts.sum(axis=0)
    print(f"E {hw} n = {n}: pixel-entries per branch {dict(zip(cc.BRANCHES, total.tolist()))}")
    assert (total > 0).all() and (total < counts.sum()).all()                        # each branch by some pixel, none by all
    col = {b: i for i, b in enumerate(cc.BRANCHES)}
    row = {clause: i for i, clause in enumerate(t.clauses)}                           # the specials are the tile's first entries
    live = counts.sum(axis=1)
    c = counts[row["A, C < 0: p > 0 at every pixel"]]
    assert c[col["p > 0"]] == 256 == live[0]
    c = counts[row["p crosses MIN_POWER inside the tile"]]
    assert c[col["p < MIN_POWER"]] > 0 and c[col["blends free"]] > 0
    c = counts[row["opacity E(p) crosses 1 / 255"]]
    assert c[col["alpha < 1 / 255"]] > 0 and c[col["blends free"]] > 0 and c[col["p < MIN_POWER"]] == 0
    c = counts[row["raw > 0.99 near the centre: capped"]]
    assert 0 < c[col["blends capped"]] < 16 and c[col["blends free"]] > 0
    i = row["the centre on a pixel centre: p = 0, E = 1"]
    u, v = t.proj["uv"][0, i]
    assert u % 1 == 0.5 and v % 1 == 0.5 and gr.exp_rule(F(0.0)) == 1
    i = row["only the rows of wave 0 blend it"]
    assert waves[i] == {0} and counts[i][col["blends free"]] > 0
    enders = [i for clause, i in row.items() if clause.startswith("opaque")]
    assert sum(counts[i][col["ends"]] > 0 for i in enders) >= 2                        # pixels end at different entries
    assert live[-1] > 0                                                                # some pixel is alive to the end: every batch is staged
    want = cc.table_definition(hw, n)
    NT = len(t.ranges)
    assert want.walked8.tolist() == [n] * NT and t.E == NT * n
    for k in ("rgb", "depth", "alpha", "state", "partial", "rgb8"):
        assert np.isfinite(getattr(want, k)).all() and getattr(want, k).any(), k
    assert not any(np.isnan(a).any() for a in t.proj.values())
    values, _, ranges = t.spoiled
    assert (values == -5).any() and (values == n).any() and (values[:len(t.clauses)] == t.values[:len(t.clauses)]).all()
    spoiled = cc.table_definition(hw, n, True)
    assert not np.array_equal(spoiled.partial, want.partial) and np.isfinite(spoiled.partial).all()
    if NT > 1:
        assert (ranges[:, 0] < 0).sum() == 1 and (ranges[:, 1] > t.E).sum() == 1 and (ranges[:, 0] > ranges[:, 1]).sum() == 1
        assert spoiled.walked8.tolist() == [n, 0, 0, n, 0, n]
        assert not spoiled.alpha[0, :16, 16:].any() and spoiled.alpha[0, 16:, :16].any()


def test_the_table_sizes_sit_on_the_batch_edges():
    assert cc.TILE_SIZES == (gb.BATCH - 1, gb.BATCH, gb.BATCH + 1, 2 * gb.BATCH + 1)


# ------------------------------------------------------------------------------------------------ F
def test_each_spoiled_gather_table_changes_its_owner_and_nobody_else():
    a = cc.full_case(cc.KEY_HW, cc.KEY_VIEWS)
    cases = cc.gather_cases()
    clean = cc.gather_definition("clean")
    want = cc.full_definition((cc.KEY_HW, cc.KEY_VIEWS))
    assert all(np.array_equal(x, want[k]) for x, k in zip(clean, GRADS))
    E = want["E"]
    for name, (count, offsets, partial, owner) in cases.items():
        if owner is None:
            continue
        got = cc.gather_definition(name)
        assert all(np.isfinite(g).all() for g in got), name
        changed = np.zeros(a.n, bool)
        for g, w in zip(got, clean):
            changed |= (g.reshape(a.n, -1) != w.reshape(a.n, -1)).any(axis=1)
        print(f"F {name}: owner (view, Gaussian) = {owner}, Gaussians whose gradients change: {np.nonzero(changed)[0].tolist()}")
        if name == "a count that says drawn where zc is out of range":
            assert not changed.any() and count[owner] > 0 and 0 <= offsets[owner] <= E - count[owner] and not a.mats[owner[0], np.clip(a.ids[owner[1]], 0, 2)].any()
        else:
            assert np.nonzero(changed)[0].tolist() == [owner[1]], name
    count, offsets, partial, owner = cases["rows that are not a number where no valid (offset, count) reaches"]
    assert np.isnan(partial).any(axis=1).sum() == want["count"][owner] and count[owner] == 0


def test_the_cases_tell_mutated_projections_and_gathers_apart():
    a = cc.full_case(cc.KEY_HW, cc.KEY_VIEWS)
    iso = gr.isotropic(np.random.default_rng(1).uniform(0.05, 0.4, a.n), a.n)             # what every raw GPU test had before
    project = lambda fn, cov: fn(a.xyz, cov, a.opacity, a.ids, a.mats, a.cam, a.hw)
    keys = ("uv", "conic", "depth", "rect", "count")
    swaps = {"sxy <-> sxz": ("(0, 1): cov[:, 1], (0, 2): cov[:, 2]", "(0, 1): cov[:, 2], (0, 2): cov[:, 1]"),
             "sxz <-> syz": ("(0, 2): cov[:, 2], (1, 1): cov[:, 3], (1, 2): cov[:, 4]", "(0, 2): cov[:, 4], (1, 1): cov[:, 3], (1, 2): cov[:, 2]"),
             "v0[1] reads sxz for syz": ("T0[1] * S(1, k)) + T0[2] * S(2, k)", "T0[1] * S(1, k)) + T0[2] * S(2, k if k != 1 else 0)")}
    for name, (old, new) in swaps.items():
        mutant = _mutant(gr.project, old, new, gr)
        right, wrong = project(gr.project, a.cov), project(mutant, a.cov)
        differ = {k: int((right[k] != wrong[k]).sum()) for k in keys}
        blind = project(gr.project, iso), project(mutant, iso)
        print(f"A projection with {name}: elements that differ on full covariances {differ}; on isotropic ones "
              f"{sum(int((blind[0][k] != blind[1][k]).sum()) for k in keys)}")
        assert differ["conic"] > a.n and differ["rect"] > 0, name
        assert all(np.array_equal(blind[0][k], blind[1][k]) for k in keys), name         # the gap this file closes
    count, offsets, partial, _ = cc.gather_cases()["clean"]
    gather = lambda fn, t=(count, offsets, partial): fn(a.xyz, a.cov, a.ids, a.mats, a.cam, a.hw, *t)
    clean = gather(gb.project_bwd)
    for name, (old, new) in dict(swaps, **{"a factor 2 dropped from an off-diagonal gradient": ("da2 * (T0[r] * T0[k])", "da * (T0[r] * T0[k])")}).items():
        wrong = gather(_mutant(gb.project_bwd, old, new, gb))
        differ = {k: int((x != y).sum()) for k, x, y in zip(GRADS, clean, wrong)}
        print(f"A backward with {name}: elements that differ {differ}")
        assert differ["d_cov"] > a.n // 2, name
    guards = {"offset -1": "(off >= 0) & ", "offset E - count + 1": "(off <= E - cnt) & ", "a count that says drawn where zc is out of range": "(zc > znear) & "}
    for name, term in guards.items():
        mutant = _mutant(gb.project_bwd, term, "", gb)
        apart = _told_apart(lambda t: gather(gb.project_bwd, t[:3]), lambda t: gather(mutant, t[:3]), cc.gather_cases())
        print(f"F without `{term[1:-4]}`: told apart by {apart}")
        assert apart == [name]
    # `cnt > 0` is implied: a count <= 0 adds no rows and a chain rule of zeros adds +0.  `zc < zfar`: the next test.


def test_a_zfar_that_is_a_drawn_gaussians_depth_silences_every_pair_at_or_beyond_it():
    a = cc.full_case(cc.KEY_HW, cc.KEY_VIEWS)
    want = cc.full_definition((cc.KEY_HW, cc.KEY_VIEWS))
    zfar, g = cc.gather_zfar()
    clean, got = cc.gather_definition("clean"), cc.gather_definition("clean", zfar)
    drawn = want["count"] > 0
    beyond = drawn & (want["depth"] >= zfar)
    assert want["depth"][0, g] == zfar and beyond[0, g] and (drawn & ~beyond).any() and all(np.isfinite(x).all() for x in got)
    changed = np.zeros(a.n, bool)
    for x, w in zip(got, clean):
        changed |= (x.reshape(a.n, -1) != w.reshape(a.n, -1)).any(axis=1)
    print(f"F zfar = {float(zfar)!r}, the depth of Gaussian {g} in view 0: {int(beyond.sum())} of {int(drawn.sum())} drawn pairs at or beyond it, "
          f"{int(changed.sum())} Gaussians' gradients change")
    assert changed[g] and not changed[~beyond.any(axis=0)].any() and changed.sum() > 20
    count, offsets, partial, _ = cc.gather_cases()["clean"]
    mutant = _mutant(gb.project_bwd, " & (zc < zfar)", "", gb)
    blind = mutant(a.xyz, a.cov, a.ids, a.mats, a.cam, a.hw, count, offsets, partial, zfar=zfar)
    assert _same(blind, clean) and not _same(blind, got)                               # without the term: as if zfar were 200
    equal = _mutant(gb.project_bwd, "(zc < zfar)", "(zc <= zfar)", gb)(a.xyz, a.cov, a.ids, a.mats, a.cam, a.hw, count, offsets, partial, zfar=zfar)
    assert not np.array_equal(equal[0][g], got[0][g])                                  # zc == zfar is refused: `<=` is told apart at Gaussian g
