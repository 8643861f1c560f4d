"""The two harmonics kernels of csrc/gaussians_sh.hip and the three `_views` blends, raw, on the hand-made cases of
tests/gaussians_sh_cases.py (tests/test_gaussians_sh_cases_cpu.py shows that each case reaches the clause it names): cloud sizes whose
last block ends in one, two and three single floats, every active degree, workgroups a view draws nothing of, ids clamped and absent,
the clamp at zero, count and offsets that falsify each guard of with_partials, and one tile at the blends' batch edges.

Every input sits in a NaN-filled (integers: sentinel-filled) allocation and is compared with itself after each call; every output sits in
a sentinel-filled allocation of exactly its size.  Every comparison is torch.equal on the bits with no element left out: the definition
(tests/gaussians_sh_reference.py) performs the kernels' rounded fp32 operations in the kernels' order.  Each call is made twice and must
give the same bits."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gaussians_sh_cases as sc
import gaussians_sh_reference as gs
from sentinel_buffers import Flat

pytestmark = pytest.mark.gpu
F = np.float32
I32, I64, F32 = torch.int32, torch.int64, torch.float32
SH_OUTS = ("d_colour", "d_sh", "d_xyz_dir")


def _t(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


def _lib():
    from mudg_amd import hip
    return hip.lib()


def _put(a, dev, dtype):
    t = _t(a).reshape(-1)
    return Flat(t.numel(), dtype, nan=dtype == F32).put(t, dev)


def _bits(t):
    return t.view(I32) if t.dtype == F32 else t


def _same(got, want, what):
    got, want = got.reshape(-1), _t(want).reshape(-1)
    assert got.dtype == want.dtype == F32 and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    differ = int((_bits(got) != _bits(want)).sum())
    assert differ == 0 and torch.equal(_bits(got), _bits(want)), f"{what}: {differ} of {got.numel()} elements differ"


def _plus_zero(got, what):
    assert torch.equal(_bits(got.reshape(-1)), torch.zeros(got.numel(), dtype=I32)), f"{what}: not +0 everywhere"


def _twice(dev, call, ins, sizes, names):
    """call(pointers of fresh blank outputs) twice; the inputs unchanged after each; the same bits; the first run's outputs."""
    runs = []
    for _ in range(2):
        outs = [Flat(size, F32).blank(dev) for size in sizes]
        assert call(*[o.ptr for o in outs], None) == 0, _lib().mudg_last_error()
        torch.cuda.synchronize()
        for k, b in ins.items():
            b.unchanged(k)
        runs.append([o.read(name) for o, name in zip(outs, names)])
    for a, b, name in zip(*runs, names):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: a repeat run differs"
    return runs[0]


# ------------------------------------------------------------------------------------------------ the two harmonics entry points
def _harmonics(cuda, c):
    """mudg_gauss_sh_colour and mudg_gauss_sh_bwd on a case: colours and the three gradients, flat, on the CPU."""
    lib = _lib()
    ins = dict(pts=_put(c.pts, cuda, I32), mats=_put(c.mats, cuda, F32), count=_put(c.count, cuda, I32), offsets=_put(c.offsets, cuda, I64),
               partial=_put(c.partial, cuda, F32), colour=_put(c.colour, cuda, F32), sh=_put(c.sh, cuda, F32))
    if c.ids is not None:
        ins["ids"] = _put(c.ids, cuda, I32)
    ids = ins["ids"].ptr if c.ids is not None else None
    head = (ins["pts"].ptr, ids, c.n, ins["mats"].ptr, c.V, c.nmat, ins["count"].ptr)
    rule = (ins["colour"].ptr, ins["sh"].ptr, c.L, c.active)
    out = SimpleNamespace()
    out.colours, = _twice(cuda, lambda *o: lib.mudg_gauss_sh_colour(*head, *rule, *o), ins, [c.V * c.n * 3], ["colours"])
    sizes = [c.n * 3, c.n * sc.row_floats(c.L), c.n * 3]
    got = _twice(cuda, lambda *o: lib.mudg_gauss_sh_bwd(*head, ins["offsets"].ptr, ins["partial"].ptr, c.E, *rule, *o), ins, sizes, SH_OUTS)
    for name, g in zip(SH_OUTS, got):
        setattr(out, name, g)
    return out


def _is_the_definition(got, want, what):
    for k in vars(got):
        _same(getattr(got, k), getattr(want, k), f"{what}: {k}")


@pytest.mark.parametrize("n", sc.SIZES)
@pytest.mark.parametrize("L", sc.DEGREES)
def test_sizes_whose_last_block_ends_in_whole_pieces_and_in_single_floats(cuda, L, n):
    c = sc.size_case(L, n)
    _is_the_definition(_harmonics(cuda, c), sc.definition(c), f"L = {L}, n = {n}, last block {sc.last_block(L, n)}")


@pytest.mark.parametrize("L,active", sc.ACTIVE)
def test_every_active_degree_reads_and_writes_its_coefficients_only(cuda, L, active):
    c = sc.active_case(L, active)
    got = _harmonics(cuda, c)
    _is_the_definition(got, sc.definition(c), f"L = {L}, active = {active}")
    Ka = gs.terms(active)
    _plus_zero(got.d_sh.reshape(c.n, -1, 3)[:, Ka - 1:], "d_sh at and above Ka")       # written (no sentinel left), the sign bit clear


def test_a_view_that_draws_nothing_of_a_workgroup_and_a_call_that_draws_nothing(cuda):
    a, b = sc.undrawn_cases()
    got = _harmonics(cuda, a)
    _is_the_definition(got, sc.definition(a), "view 1 draws nothing of Gaussians 256 .. 511")
    _plus_zero(got.colours.reshape(a.V, a.n, 3)[1, 256:512], "the colours of the workgroup that is not drawn")
    nothing = _harmonics(cuda, b)
    _is_the_definition(nothing, sc.definition(b), "every count 0")
    for k in ("colours",) + SH_OUTS:
        _plus_zero(getattr(nothing, k), f"every count 0: {k}")


def test_ids_are_clamped_and_may_be_absent_with_one_matrix(cuda):
    wild, clipped, null = sc.ids_cases()
    a, b = _harmonics(cuda, wild), _harmonics(cuda, clipped)
    _is_the_definition(a, sc.definition(wild), "ids from {-3, 0, 1, 2, 7}")
    for k in vars(a):
        _same(getattr(a, k), getattr(b, k), f"ids clipped by the caller: {k}")
    _is_the_definition(_harmonics(cuda, null), sc.definition(null), "one matrix, no ids")


def test_the_clamp_at_zero_minus_zero_and_just_below(cuda):
    c = sc.clamp_case()
    _is_the_definition(_harmonics(cuda, c), sc.definition(c), "the clamp's edge")


@pytest.mark.parametrize("guard", ("clean",) + sc.GUARDS)
def test_count_and_offsets_that_falsify_one_guard_are_not_followed(cuda, guard):
    clean, spoiled = sc.spoiled_cases()
    c = clean if guard == "clean" else spoiled[guard][0]
    _is_the_definition(_harmonics(cuda, c), sc.definition(c), guard)


# ------------------------------------------------------------------------------------------------ the three `_views` blends
BLEND_OUTS = ("rgb", "depth", "alpha", "state", "partial")


def _blends(cuda, t, colour, tables=None):
    """The training blend, the inference blend and the backward on a tile case, raw.  colour (n, 3): mudg_gauss_blend_train and
    mudg_gauss_blend_bwd; colour (V, n, 3): the three `_views` entry points.  tables: values, order, ranges (the case's own)."""
    lib = _lib()
    views = colour.ndim == 3
    values, order, ranges = tables or (t.values, t.order, t.ranges)
    H, W = t.hw
    ins = dict(colour=_put(colour, cuda, F32), uv=_put(t.proj["uv"], cuda, F32), conic=_put(t.proj["conic"], cuda, F32),
               depth=_put(t.proj["depth"], cuda, F32), values=_put(values, cuda, I32), order=_put(order, cuda, I64), ranges=_put(ranges, cuda, I32))
    ins.update({f"up{k}": _put(u, cuda, F32) for k, u in enumerate(t.ups)})
    head = tuple(ins[k].ptr for k in ("colour", "uv", "conic", "depth", "values"))
    size = (t.n, t.E, t.V, H, W)
    images = [t.V * 3 * H * W, t.V * H * W, t.V * H * W]
    train = lib.mudg_gauss_blend_train_views if views else lib.mudg_gauss_blend_train
    rgb, depth, alpha, state = _twice(cuda, lambda *o: train(*head, ins["ranges"].ptr, *size, *o), ins, images + [t.V * 5 * H * W], BLEND_OUTS[:4])
    if views:
        plain = _twice(cuda, lambda *o: lib.mudg_gauss_blend_views(*head, ins["ranges"].ptr, *size, *o), ins, images, BLEND_OUTS[:3])
        for a, b, name in zip(plain, (rgb, depth, alpha), BLEND_OUTS):
            _same(a, b, f"mudg_gauss_blend_views against the training blend: {name}")
    ins["state"] = _put(state, cuda, F32)
    ups = [ins[f"up{k}"].ptr for k in range(3)]
    bwd = lib.mudg_gauss_blend_bwd_views if views else lib.mudg_gauss_blend_bwd
    partial, = _twice(cuda, lambda *o: bwd(*head, ins["order"].ptr, ins["ranges"].ptr, *size, ins["state"].ptr, *ups, *o), ins, [t.E * 10], ["partial"])
    return SimpleNamespace(rgb=rgb, depth=depth, alpha=alpha, state=state, partial=partial)


@pytest.mark.parametrize("n", sc.TILE_SIZES)
def test_the_views_blends_with_one_colour_for_both_views_are_the_plain_blends(cuda, n):
    t = sc.tile_case(n)
    views, plain = _blends(cuda, t, t.same), _blends(cuda, t, t.colour)
    for k in BLEND_OUTS:
        _same(getattr(views, k), getattr(plain, k), f"{n} entries on the tile: {k}")
    assert plain.partial.any() and plain.rgb.any()


def test_the_views_blends_take_each_views_own_colours(cuda):
    t = sc.tile_case(257)
    want = sc.blend_definition(t, t.colours, t.values, t.order, t.ranges)
    got, same = _blends(cuda, t, t.colours), _blends(cuda, t, t.same)
    for k in BLEND_OUTS:
        _same(getattr(got, k), getattr(want, k), f"colours that differ between the views: {k}")
    half = got.rgb.numel() // 2
    assert torch.equal(got.rgb[:half], same.rgb[:half]) and not torch.equal(got.rgb[half:], same.rgb[half:])   # a stride of 0 fails here
    assert torch.equal(got.partial[:2570], same.partial[:2570]) and not torch.equal(_bits(got.partial[2570:]), _bits(same.partial[2570:]))


def test_the_views_blends_do_not_follow_spoiled_values_order_or_ranges(cuda):
    t = sc.tile_case(257)
    want = sc.blend_definition(t, t.colours, *t.spoiled)
    got = _blends(cuda, t, t.colours, t.spoiled)
    for k in BLEND_OUTS:
        _same(getattr(got, k), getattr(want, k), f"spoiled tables: {k}")
