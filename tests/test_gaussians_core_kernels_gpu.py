"""The seven core entry points of the Gaussian splat renderer (mudg_gauss_project, _keys, _ranges, _blend, _blend_train, _blend_bwd,
_project_bwd), raw, on the hand-made cases of tests/gaussians_core_cases.py (tests/test_gaussians_core_cases_cpu.py shows that each case
reaches the clause it names and tells a mutated definition apart): full covariances, one Gaussian per drop clause, rect / count / offsets
that falsify each guard of the keys, sorted keys with tiles outside the grid, hand-made blend tables that take every branch of the blend
step at the batch edges with spoiled values and ranges, and count / offsets / partial rows that falsify the gather's guards.

Every input sits in a NaN-filled (integers: sentinel-filled) allocation and is compared with itself after each call; every output sits in
a sentinel-filled allocation of exactly its size.  Every comparison is torch.equal on the bits with no element left out: the definitions
perform the kernels' rounded fp32 operations in the kernels' order.  Each call is made twice and must give the same bits.  Each stage is
fed the definition's tables, so that one wrong stage fails alone; `chained` runs feed each kernel the previous kernel's output.  Every
test runs twice: with every base pointer 1 KiB-aligned, and with each operand at the least alignment its entry point asks for (16 bytes
for points, conic and rect, 8 for uv and the int64 tables, 4 for everything else)."""
import numpy as np
import pytest
import torch

import gaussians_core_cases as cc
import gaussians_reference as gr
from sentinel_buffers import Flat

pytestmark = pytest.mark.gpu
F = np.float32
I32, I64, F32 = torch.int32, torch.int64, torch.float32
GRADS = ("d_xyz", "d_cov", "d_opacity", "d_colour")
PROJ = ("uv", "conic", "depth", "rect", "count")
IMAGES = ("rgb", "depth_out", "alpha")
# elements past a 1 KiB boundary when `shift` is set: 16 bytes, 8 bytes, or an odd number of 4-byte elements
SHIFT = dict(pts=4, conic=4, rect=4, uv=2, offsets=1, order=1, keys=1, cov=1, opacity=3, ids=1, mats=3, depth=1, count=3, values=3, ranges=1, colour=3,
             state=1, d_rgb=1, d_depth=3, d_alpha=1, partial=3, rgb=1, depth_out=3, alpha=1, walked=3, d_xyz=1, d_cov=3, d_opacity=1, d_colour=3)
SENTINEL = {I64: Flat(1, I64).cpu[0].clone(), I32: Flat(1, I32).cpu[0].clone()}


def _t(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


def _bits(t):
    return t.view(I32) if t.dtype == F32 else t


def _same(got, want, what):
    got, want = got.reshape(-1), _t(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    differ = int((_bits(got) != _bits(want)).sum())
    assert differ == 0 and torch.equal(_bits(got), _bits(want)), f"{what}: {differ} of {got.numel()} elements differ"


class Bench:
    """Where the operands and results of a test live: on `dev`, in Flat buffers, shifted or not."""

    def __init__(self, dev, shift):
        from mudg_amd import hip
        self.dev, self.shift, self.hip, self.lib = dev, shift, hip, hip.lib()

    def off(self, name):
        return SHIFT[name] if self.shift else 0

    def put(self, name, a):
        t = _t(a).reshape(-1)
        return Flat(t.numel(), t.dtype, off=self.off(name), nan=t.dtype == F32).put(t, self.dev)

    def twice(self, what, call, ins, outs):
        """call(pointers of fresh blank outputs) twice; the inputs unchanged after each; the same bits; the first run's outputs.
        outs: (name, elements, dtype) each."""
        runs = []
        for _ in range(2):
            bufs = [Flat(size, dtype, off=self.off(name)).blank(self.dev) for name, size, dtype in outs]
            self.hip.check(call(*[b.ptr for b in bufs]), what)
            torch.cuda.synchronize()
            for k, b in ins.items():
                b.unchanged(f"{what}: {k}")
            runs.append([b.read(f"{what}: {name}") for b, (name, _, _) in zip(bufs, outs)])
        for a, b, (name, _, _) in zip(*runs, outs):
            assert torch.equal(_bits(a), _bits(b)), f"{what}: {name}: a repeat run differs"
        return runs[0]

    # ---------------------------------------------------------------------------------------------- the seven entry points
    def project(self, c):
        ins = dict(pts=self.put("pts", c.pts), cov=self.put("cov", c.cov), opacity=self.put("opacity", c.opacity), mats=self.put("mats", c.mats))
        if c.ids is not None:
            ins["ids"] = self.put("ids", c.ids)
        ids = ins["ids"].ptr if c.ids is not None else None
        H, W = c.hw
        m = c.V * c.n
        call = lambda *o: self.lib.mudg_gauss_project(ins["pts"].ptr, ins["cov"].ptr, ins["opacity"].ptr, ids, c.n, ins["mats"].ptr, c.V, c.nmat, H, W,
                                                      *[float(x) for x in c.cam], gr.ZNEAR, gr.ZFAR, *o, None)
        got = self.twice("project", call, ins, [("uv", 2 * m, F32), ("conic", 4 * m, F32), ("depth", m, F32), ("rect", 4 * m, I32), ("count", m, I32)])
        return dict(zip(PROJ, got))

    def keys(self, depth, rect, count, offsets, n, V, hw, E):
        ins = dict(depth=self.put("depth", depth), rect=self.put("rect", _t(rect).to(I32)), count=self.put("count", count), offsets=self.put("offsets", offsets))
        call = lambda *o: self.lib.mudg_gauss_keys(ins["depth"].ptr, ins["rect"].ptr, ins["count"].ptr, ins["offsets"].ptr, n, V, hw[0], hw[1], E, *o, None)
        return self.twice("keys", call, ins, [("keys", E, I64), ("values", E, I32)])

    def ranges(self, keys_sorted, E, tiles):
        ins = dict(keys=self.put("keys", keys_sorted))
        call = lambda *o: self.lib.mudg_gauss_ranges(ins["keys"].ptr, E, tiles, *o, None)
        return self.twice("ranges", call, ins, [("ranges", 2 * tiles, I32)])[0]

    def _tables(self, proj, values, ranges):
        return dict(uv=self.put("uv", proj["uv"]), conic=self.put("conic", proj["conic"]), depth=self.put("depth", proj["depth"]),
                    values=self.put("values", values), ranges=self.put("ranges", ranges))

    def blend(self, pts, proj, values, ranges, n, V, hw, with_walked):
        ins = dict(self._tables(proj, values, ranges), pts=self.put("pts", pts))
        H, W = hw
        E, tiles = len(values), len(np.asarray(ranges).reshape(-1, 2))
        head = tuple(ins[k].ptr for k in ("pts", "uv", "conic", "depth", "values", "ranges"))
        outs = [("rgb", 3 * V * H * W, F32), ("depth_out", V * H * W, F32), ("alpha", V * H * W, F32)]
        if with_walked:
            return self.twice("blend", lambda *o: self.lib.mudg_gauss_blend(*head, n, E, V, H, W, *o, None), ins, outs + [("walked", tiles, I32)])
        return self.twice("blend", lambda *o: self.lib.mudg_gauss_blend(*head, n, E, V, H, W, *o, None, None), ins, outs)

    def blend_train(self, colour, proj, values, ranges, n, V, hw):
        ins = dict(self._tables(proj, values, ranges), colour=self.put("colour", colour))
        H, W = hw
        head = tuple(ins[k].ptr for k in ("colour", "uv", "conic", "depth", "values", "ranges"))
        outs = [("rgb", 3 * V * H * W, F32), ("depth_out", V * H * W, F32), ("alpha", V * H * W, F32), ("state", 5 * V * H * W, F32)]
        return self.twice("blend_train", lambda *o: self.lib.mudg_gauss_blend_train(*head, n, len(values), V, H, W, *o, None), ins, outs)

    def blend_bwd(self, colour, proj, values, order, ranges, n, V, hw, state, ups):
        ins = dict(self._tables(proj, values, ranges), colour=self.put("colour", colour), order=self.put("order", order), state=self.put("state", state),
                   d_rgb=self.put("d_rgb", ups[0]), d_depth=self.put("d_depth", ups[1]), d_alpha=self.put("d_alpha", ups[2]))
        H, W = hw
        E = len(values)
        head = tuple(ins[k].ptr for k in ("colour", "uv", "conic", "depth", "values", "order", "ranges"))
        tail = tuple(ins[k].ptr for k in ("state", "d_rgb", "d_depth", "d_alpha"))
        return self.twice("blend_bwd", lambda *o: self.lib.mudg_gauss_blend_bwd(*head, n, E, V, H, W, *tail, *o, None), ins, [("partial", 10 * E, F32)])[0]

    def project_bwd(self, c, count, offsets, partial, zfar=gr.ZFAR):
        ins = dict(pts=self.put("pts", c.pts), cov=self.put("cov", c.cov), mats=self.put("mats", c.mats), count=self.put("count", count),
                   offsets=self.put("offsets", offsets), partial=self.put("partial", partial))
        if c.ids is not None:
            ins["ids"] = self.put("ids", c.ids)
        ids = ins["ids"].ptr if c.ids is not None else None
        H, W = c.hw
        E = _t(partial).numel() // 10
        call = lambda *o: self.lib.mudg_gauss_project_bwd(ins["pts"].ptr, ins["cov"].ptr, ids, c.n, ins["mats"].ptr, c.V, c.nmat, H, W, *[float(x) for x in c.cam],
                                                          gr.ZNEAR, float(zfar), ins["count"].ptr, ins["offsets"].ptr, ins["partial"].ptr, E, *o, None)
        got = self.twice("project_bwd", call, ins, [("d_xyz", 3 * c.n, F32), ("d_cov", 6 * c.n, F32), ("d_opacity", c.n, F32), ("d_colour", 3 * c.n, F32)])
        return dict(zip(GRADS, got))


@pytest.fixture(params=[False, True], ids=["aligned", "shifted"])
def bench(cuda, request):
    return Bench(cuda, request.param)


def _full(key):
    return (cc.flat_full_case() if key == "flat" else cc.full_case(*key)), cc.full_definition(key)


FULL_KEYS = cc.FULL_SHAPES + ("flat",)
FULL_IDS = [k if k == "flat" else f"{k[0][0]}x{k[0][1]}-{k[1]}views" for k in FULL_KEYS]


def _sorted(keys, values):
    """The host's step between mudg_gauss_keys and mudg_gauss_ranges, as the product makes it."""
    keys, order = torch.sort(keys, stable=True)
    return keys, values[order], order


# ------------------------------------------------------------------------------------------------ A: full covariances
@pytest.mark.parametrize("key", FULL_KEYS, ids=FULL_IDS)
def test_full_covariances_through_every_entry_point_each_fed_the_definitions_tables(bench, key):
    c, want = _full(key)
    E, hw, V, n = want["E"], c.hw, c.V, c.n
    tiles = len(want["ranges"])
    got = bench.project(c)
    for k in PROJ:
        _same(got[k], want[k].astype(np.int32) if k == "rect" else want[k], f"project: {k}")
    keys, values = bench.keys(want["depth"], want["rect"], want["count"], want["offsets"], n, V, hw, E)
    raw = cc.keys_raw(want["depth"], want["rect"], want["count"], want["offsets"], n, V, hw, E)
    assert raw[2].all()
    _same(keys, raw[0], "keys")
    _same(values, raw[1], "values")
    k_sorted, v_sorted, order = _sorted(keys, values)
    _same(k_sorted, want["keys"], "sorted keys")
    _same(v_sorted, want["values"], "sorted values")
    _same(order, want["order"], "the sort's permutation")
    _same(bench.ranges(want["keys"], E, tiles), want["ranges"], "ranges")
    proj = want["proj"]
    for with_walked in (False, True):
        out = bench.blend(c.pts, proj, want["values"], want["ranges"], n, V, hw, with_walked)
        for o, k in zip(out, ("rgb8", "depth8", "alpha8", "walked8")):
            _same(o, want[k], f"blend: {k}")
    out = bench.blend_train(c.colour, proj, want["values"], want["ranges"], n, V, hw)
    for o, k in zip(out, ("rgb", "depth_image", "alpha", "state")):
        _same(o, want[k], f"blend_train: {k}")
    _same(bench.blend_bwd(c.colour, proj, want["values"], want["order"], want["ranges"], n, V, hw, want["state"], c.ups), want["partial"], "partial")
    grads = bench.project_bwd(c, want["count"], want["offsets"], want["partial"])
    for k in GRADS:
        _same(grads[k], want[k], k)
    print(f"A {key}: {E} entries; elements that differ: 0 of every output of the seven entry points")


@pytest.mark.parametrize("key", FULL_KEYS, ids=FULL_IDS)
def test_full_covariances_chained_each_kernel_fed_the_previous_kernels_output(bench, key):
    c, want = _full(key)
    hw, V, n = c.hw, c.V, c.n
    got = bench.project(c)
    count = got["count"].to(I64)
    ends = torch.cumsum(count, 0)
    offsets, E = ends - count, int(ends[-1])
    assert E == want["E"]
    keys, values = bench.keys(got["depth"], got["rect"], got["count"], offsets, n, V, hw, E)
    k_sorted, v_sorted, order = _sorted(keys, values)
    ranges = bench.ranges(k_sorted, E, len(want["ranges"]))
    proj = {k: got[k] for k in ("uv", "conic", "depth")}
    for o, k in zip(bench.blend(c.pts, proj, v_sorted, ranges, n, V, hw, True), ("rgb8", "depth8", "alpha8", "walked8")):
        _same(o, want[k], f"chained blend: {k}")
    rgb, depth, alpha, state = bench.blend_train(c.colour, proj, v_sorted, ranges, n, V, hw)
    for o, k in zip((rgb, depth, alpha, state), ("rgb", "depth_image", "alpha", "state")):
        _same(o, want[k], f"chained blend_train: {k}")
    partial = bench.blend_bwd(c.colour, proj, v_sorted, order, ranges, n, V, hw, state, c.ups)
    _same(partial, want["partial"], "chained partial")
    grads = bench.project_bwd(c, got["count"], offsets, partial)
    for k in GRADS:
        _same(grads[k], want[k], f"chained {k}")


@pytest.mark.parametrize("key", FULL_KEYS, ids=FULL_IDS)
def test_full_covariances_through_the_products_wrappers(cuda, key):
    from mudg_amd import gaussians, render
    c, want = _full(key)
    d = lambda a: None if a is None else _t(a).to(cuda)
    g = gaussians.Gaussians(render.PointCloud(d(c.pts)), d(c.cov), d(c.opacity), d(c.ids))
    stats = {}
    out = gaussians.render(g, d(c.mats), c.cam, c.hw, stats=stats)
    for k, w in (("rgb", "rgb8"), ("depth", "depth8"), ("alpha", "alpha8")):
        _same(out[k].cpu(), want[w], f"render: {k}")
    _same(stats["values"].cpu(), want["values"], "render: sorted values")
    _same(stats["ranges"].cpu(), want["ranges"], "render: ranges")
    leaves = [d(a).requires_grad_(True) for a in (c.xyz, c.colour, c.cov, c.opacity)]
    images = gaussians.render_differentiable(*leaves, d(c.mats), c.cam, c.hw, ids=d(c.ids))
    for o, k in zip(images, ("rgb", "depth_image", "alpha")):
        _same(o.detach().cpu(), want[k], f"render_differentiable: {k}")
    torch.autograd.backward(images, [d(u) for u in c.ups])
    for leaf, k in zip(leaves, ("d_xyz", "d_colour", "d_cov", "d_opacity")):
        _same(leaf.grad.cpu(), want[k], f"render_differentiable: {k}")


# ------------------------------------------------------------------------------------------------ B: what the projection drops
@pytest.mark.parametrize("hw", [(16, 16), (40, 56)])
def test_one_gaussian_per_drop_clause(bench, hw):
    c = cc.drop_case(hw)
    want = cc.project_case(c)
    got = bench.project(c)
    count = got["count"].tolist()
    for i, clause in enumerate(c.clauses):
        assert (count[i] > 0) == bool(c.drawn[i]), clause
    for k in PROJ:
        _same(got[k], want[k].astype(np.int32) if k == "rect" else want[k], f"project: {k}")
        assert not got[k].reshape(c.n, -1)[_t(~c.drawn)].any(), k                     # +0 and 0 where dropped: written, nothing stale


# ------------------------------------------------------------------------------------------------ C: the guards of the keys
def test_rect_count_and_offsets_that_falsify_a_guard_of_the_keys_write_nothing(bench):
    clean, cases = cc.key_cases()
    tables = dict({"clean": (clean, None)}, **cases)
    for name, (c, owner) in tables.items():
        keys, values, written = cc.keys_definition(c)
        want_keys = torch.where(_t(written), _t(keys), SENTINEL[I64])
        want_values = torch.where(_t(written), _t(values), SENTINEL[I32])
        got_keys, got_values = bench.keys(c.depth, c.rect, c.count, c.offsets, c.n, c.V, c.hw, c.E)
        _same(got_keys, want_keys, f"{name}: keys, the sentinel where nothing is written")
        _same(got_values, want_values, f"{name}: values, the sentinel where nothing is written")
        a, b = _sorted(got_keys, got_values), _sorted(want_keys, want_values)
        _same(a[0], b[0], f"{name}: sorted keys")
        _same(a[1], b[1], f"{name}: sorted values")
        print(f"C {name}: owner {owner}, {int((~written).sum())} of {c.E} entries left at the sentinel")


# ------------------------------------------------------------------------------------------------ D: sorted keys
def test_ranges_of_one_entry_one_tile_distant_tiles_and_tiles_outside_the_grid(bench):
    for name, (keys, E, tiles) in cc.range_cases().items():
        _same(bench.ranges(keys, E, tiles), cc.ranges_raw(keys, E, tiles), name)


# ------------------------------------------------------------------------------------------------ E: hand-made blend tables
@pytest.mark.parametrize("spoiled", [False, True], ids=["clean", "spoiled"])
@pytest.mark.parametrize("hw,n", [((16, 16), n) for n in cc.TILE_SIZES] + [((17, 33), 60)])
def test_hand_made_tables_through_the_three_blends(bench, hw, n, spoiled):
    t, want = cc.table_case(hw, n), cc.table_definition(hw, n, spoiled)
    values, order, ranges = t.spoiled if spoiled else (t.values, t.order, t.ranges)
    out = bench.blend(t.pts, t.proj, values, ranges, t.n, 1, hw, False)
    for o, k in zip(out, ("rgb8", "depth8", "alpha8")):
        _same(o, getattr(want, k), f"blend without walked: {k}")
    out = bench.blend(t.pts, t.proj, values, ranges, t.n, 1, hw, True)
    for o, k in zip(out, ("rgb8", "depth8", "alpha8", "walked8")):
        _same(o, getattr(want, k), f"blend: {k}")
    out = bench.blend_train(t.colour, t.proj, values, ranges, t.n, 1, hw)
    for o, k in zip(out, ("rgb", "depth", "alpha", "state")):
        _same(o, getattr(want, k), f"blend_train: {k}")
    _same(bench.blend_bwd(t.colour, t.proj, values, order, ranges, t.n, 1, hw, want.state, t.ups), want.partial, "partial")


# ------------------------------------------------------------------------------------------------ F: the guards of the gather
def test_count_offsets_and_rows_that_falsify_a_guard_of_the_gather_add_nothing(bench):
    c = cc.full_case(cc.KEY_HW, cc.KEY_VIEWS)
    for name, (count, offsets, partial, owner) in cc.gather_cases().items():
        want = cc.gather_definition(name)
        got = bench.project_bwd(c, count, offsets, partial)
        for k, w in zip(GRADS, want):
            _same(got[k], w, f"{name}: {k}")
            assert not torch.isnan(got[k]).any(), f"{name}: {k}"
        print(f"F {name}: owner {owner}")
    zfar, g = cc.gather_zfar()                                                         # the clean tables, a zfar that is Gaussian g's zc in view 0
    count, offsets, partial, _ = cc.gather_cases()["clean"]
    got = bench.project_bwd(c, count, offsets, partial, zfar=zfar)
    for k, w in zip(GRADS, cc.gather_definition("clean", zfar)):
        _same(got[k], w, f"zfar = {float(zfar)!r}: {k}")
