"""tests/gemm_reference.py against the textbook torch ops in fp64 (needs no GPU), and the conditions the GPU file's cases rest on:
the exactness condition of every exact case, the constructors' properties, and the head-room of the bounded tests' flip cap."""
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_reference as R
import test_gemm_kernels_gpu as T
from backward_reference import operand_planes

F64 = torch.float64
TOL = 1e-12


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def close(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------ mode 0
def test_gemm_is_linear_with_the_epilogue_in_the_stated_order():
    x, w, b = rnd(2, 37, 24, seed=1), rnd(2, 10, 24, seed=2), rnd(10, seed=3)
    gb, r = rnd(5, 10, seed=4), rnd(2, 37, 10, seed=5)
    want = torch.stack([F.linear(x[z], w[z]) for z in range(2)])
    close(R.gemm(x, w), want)
    close(R.gemm(x, w, alpha=0.0), want)                                                       # alpha = 0 means 1
    grp = torch.arange(37) // 8
    close(R.gemm(x, w, alpha=0.5, bias=b, gbias=gb, rows_per_group=8, r=r), 0.5 * want + b + gb[grp] + r)
    close(R.gemm(x, w, alpha=2.0, bias=b, act=True, r=r), F.gelu(2.0 * want + b) + r)
    # two sources split at csplit; a shared X (sX = 0)
    close(R.gemm(x[..., :8], w, x2=x[..., 8:], csplit=8), want)
    close(R.gemm(x[:1], w), torch.stack([F.linear(x[0], w[z]) for z in range(2)]))


def test_gemm_strided_views_state_the_vt_form():
    """X = the projection's rows shared by every batch (sX = 0), W = a batch's tokens, Y = V^T [channels][tokens] with a padded ldy."""
    wv, ctx = rnd(16, 24, seed=1), rnd(3, 7, 24, seed=2)
    flat_w = torch.zeros(5 + 3 * 7 * 32, dtype=F64)
    R.strided(flat_w, 5, 32, 7, 24, 3, 7 * 32).copy_(ctx)
    y = R.gemm(wv[None], R.strided(flat_w, 5, 32, 7, 24, 3, 7 * 32))
    flat_y = torch.full((3 + 3 * 16 * 12,), float("nan"), dtype=F64)
    R.strided(flat_y, 3, 12, 16, 7, 3, 16 * 12).copy_(y)
    for z in range(3):
        close(R.strided(flat_y, 3, 12, 16, 7, 3, 16 * 12)[z], F.linear(ctx[z], wv).t())
    assert int(torch.isnan(flat_y).sum()) == flat_y.numel() - 3 * 16 * 7


def test_gelu_and_geglu_packing():
    g = torch.linspace(-10, 10, 4001, dtype=F64)
    close(R.gelu_erf(g), F.gelu(g))
    x, w, b = rnd(1, 9, 16, seed=1), rnd(1, 128, 16, seed=2), rnd(128, seed=3)
    # the packing of mudg_amd.engine.packing.geglu: blocks of 32 value rows followed by their 32 gate rows
    idx = torch.arange(64).reshape(-1, 32)
    order = torch.cat([idx, idx + 64], 1).reshape(-1)
    h = F.linear(x[0], w[0], b)
    want = h[:, :64] * F.gelu(h[:, 64:])
    close(R.gemm(x, w[:, order], bias=b[order], geglu=True)[0], want)


# ------------------------------------------------------------------------------------------------ mode 1
def nchw(x_rows, frames, h, w):
    return x_rows.reshape(frames, h, w, -1).permute(0, 3, 1, 2)


def rows_of(y):
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def pack_taps(w4):
    """(Cout, Cin, 3, 3) -> [Cout][tap][Cin] flattened (korder 0)."""
    return w4.permute(0, 2, 3, 1).reshape(w4.shape[0], -1)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 2), (2, 1), (5, 7), (8, 6)])
@pytest.mark.parametrize("stride,pad,up", [(1, 1, 0), (2, 1, 0), (2, 0, 0), (1, 1, 1)])
def test_conv3x3_is_conv2d(h, w, stride, pad, up):
    if pad == 0 and (h < 2 or w < 2):
        return                                                                                 # no output pixel
    frames, cin, n = 3, 8, 5
    x, w4, b = rnd(frames * h * w, cin, seed=1), rnd(n, cin, 3, 3, seed=2), rnd(n, seed=3)
    img = nchw(x, frames, h, w)
    if up:
        img = F.interpolate(img, scale_factor=2, mode="nearest")
    if pad == 0:
        want = F.conv2d(F.pad(img, (0, 1, 0, 1)), w4, b, stride=stride)
    else:
        want = F.conv2d(img, w4, b, stride=stride, padding=1)
    got = R.conv3x3(x[None], pack_taps(w4)[None], frames=frames, hin=h, win=w, cin=cin, stride=stride, pad=pad, upsample=up, bias=b)
    assert (want.shape[2], want.shape[3]) == R.conv_out_size(h, w, stride, pad, up)
    close(got[0], rows_of(want))


def test_conv3x3_two_sources_and_slab_major_twin():
    frames, h, w, cin, n = 2, 4, 5, 128, 6
    x, w4 = rnd(frames * h * w, cin, seed=1), rnd(n, cin, 3, 3, seed=2)
    want = rows_of(F.conv2d(nchw(x, frames, h, w), w4, padding=1))
    wk = pack_taps(w4)
    geo = dict(frames=frames, hin=h, win=w, cin=cin)
    close(R.conv3x3(x[None, :, :64], wk[None], x2=x[None, :, 64:], csplit=64, **geo)[0], want)
    close(R.conv3x3(x[None], R.slab_major(wk, 9, cin)[None], korder=1, **geo)[0], want)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (5, 8)])
def test_subpixel_form_is_upsample_then_conv3x3(h, w, monkeypatch):
    from mudg_amd.engine import packing
    monkeypatch.setattr(packing, "_need_cuda", lambda p, what: None)                          # layout work only: runs on CPU tensors too
    frames, cin, n = 2, 64, 5
    conv = torch.nn.Conv2d(cin, n, 3, padding=1)
    with torch.no_grad():                                                                      # small integers: the 16-bit cast of the packed sums is exact
        conv.weight.copy_(torch.randint(-3, 4, conv.weight.shape, generator=torch.Generator().manual_seed(1)).float())
    w4 = packing.conv3x3_subpixel(conv).to(F64).reshape(4, n, 4 * cin)
    x, b = rnd(frames * h * w, cin, seed=2), rnd(n, seed=3)
    want = F.conv2d(F.interpolate(nchw(x, frames, h, w), scale_factor=2, mode="nearest"), conv.weight.detach().to(F64), b, padding=1)
    close(R.conv3x3_subpixel(x[None], w4, frames=frames, hin=h, win=w, cin=cin, bias=b)[0], rows_of(want))
    close(R.conv3x3(x[None], pack_taps(conv.weight.detach().to(F64))[None], frames=frames, hin=h, win=w, cin=cin, upsample=1, bias=b)[0], rows_of(want))


# ------------------------------------------------------------------------------------------------ mode 2
@pytest.mark.parametrize("t", [1, 2, 3, 16, 17])
def test_tconv3_is_conv3d(t):
    clips, hw, cin, n = 2, 5, 64, 6
    x, w5, b = rnd(clips * t * hw, cin, seed=1), rnd(n, cin, 3, 1, 1, seed=2), rnd(n, seed=3)
    vol = x.reshape(clips, t, hw, 1, cin).permute(0, 4, 1, 2, 3)
    want = F.conv3d(vol, w5, b, padding=(1, 0, 0)).permute(0, 2, 3, 4, 1).reshape(clips * t * hw, n)
    wk = w5[:, :, :, 0, 0].permute(0, 2, 1).reshape(n, 3 * cin)
    close(R.tconv3(x[None], wk[None], clips=clips, t=t, hw=hw, cin=cin, bias=b)[0], want)
    close(R.tconv3(x[None], R.slab_major(wk, 3, cin)[None], clips=clips, t=t, hw=hw, cin=cin, korder=1, bias=b)[0], want)
    close(R.tconv3(x[None, :, :8], wk[None], x2=x[None, :, 8:], csplit=8, clips=clips, t=t, hw=hw, cin=cin, bias=b)[0], want)


# ------------------------------------------------------------------------------------------------ storage, stats, pieces, fp8
def test_store_stats_split_kept_and_mxfp8():
    v = rnd(70, 64, seed=1) * 300
    assert torch.equal(R.store(v, R.KIND_F32), v.float().double())
    assert torch.equal(R.store(v, R.KIND_F16), v.float().half().double())
    assert torch.equal(R.store(torch.tensor([1e6, -1e6], dtype=F64), R.KIND_F16), torch.tensor([65504.0, -65504.0], dtype=F64))
    assert torch.equal(R.store(v, R.KIND_OPERAND, torch.bfloat16, 1), v.float().bfloat16().double())
    for planes, bits in ((2, 16), (3, 24)):
        err = (R.store(v, R.KIND_OPERAND, torch.bfloat16, planes) - v.float().double()).abs()
        assert bool((err <= v.abs() * 2.0 ** -bits).all())
    st = R.stats(v, 32)
    assert st.shape == (3, 64, 2)
    close(st[2, :, 0], v[64:].sum(0))
    close(st[1, :, 1], (v[32:64] ** 2).sum(0))
    # the kept pairs: all products of the pieces minus the dropped ones
    for planes, dropped in ((1, []), (2, [(1, 1)]), (3, [(1, 2), (2, 1), (2, 2)])):
        xs, ws = [rnd(1, 9, 8, seed=10 + p) for p in range(planes)], [rnd(1, 5, 8, seed=20 + p) for p in range(planes)]
        full = R.contract_gemm(sum(xs), sum(ws))
        close(R.split_kept(R.contract_gemm, xs, ws, planes), full - sum(R.contract_gemm(xs[p], ws[q]) for p, q in dropped))
        assert len(R.KEPT[planes]) == planes * planes - len(dropped)
    # MX-fp8: definition of the header, element by element
    y = (rnd(5, 64, seed=3) * torch.tensor([1e-3, 1.0, 37.0, 0.0, 448.0], dtype=F64)[:, None]).float().bfloat16().double()
    y8, s8 = R.mxfp8(y)
    for r in range(5):
        for blk in range(2):
            seg = y[r, 32 * blk:32 * blk + 32]
            amax = float(seg.abs().max())
            e = (math.floor(math.log2(amax)) - 8) if amax > 0 else 0
            assert int(s8[r, blk]) == e + 127
            want = (seg / 2.0 ** e).clamp(-448, 448).float().to(torch.float8_e4m3fn)
            assert torch.equal(y8[r, 32 * blk:32 * blk + 32], want.view(torch.uint8))


# ------------------------------------------------------------------------------------------------ the GPU file's cases
@pytest.mark.parametrize("planes", [1, 2, 3])
@pytest.mark.parametrize("c", T.EXACT_CASES, ids=lambda c: c["name"])
def test_every_exact_case_meets_its_exactness_condition(c, planes):
    bits, unit = T.exactness(c, planes)
    assert math.log2(unit) == int(math.log2(unit))
    assert bits < 2 ** 24, (c["name"], planes, bits)


@pytest.mark.parametrize("c", [c for c in T.EXACT_CASES if T.geometry(c)[1] * c["N"] * T.geometry(c)[2] <= 3e7], ids=lambda c: c["name"])
def test_exact_cases_have_fp32_representable_results_within_the_bound(c):
    """The expected values of the small cases, built as the GPU file builds them: integers (multiples of the unit) that fp32 holds, inside
    the case's bound; operands exact in both 16-bit operand types."""
    for planes in (1, 3):
        xs, ws, bias, gb, res = T.exact_operands(c, planes, 1)
        for t in xs + ws:
            assert torch.equal(t.bfloat16().float(), t) and torch.equal(t.half().float(), t)
        want = T.exact_value(c, xs, ws, bias, gb, res, planes)
        bits, unit = T.exactness(c, planes)
        assert bool((want.float().double() == want).all())
        assert bool(((want / unit) == torch.round(want / unit)).all())
        assert float(want.abs().max()) <= bits * unit


@pytest.mark.parametrize("c", T.STATS_CASES, ids=lambda c: c["name"])
def test_stats_cases_have_exact_sums_of_squares(c):
    """`stats` of the exact cases: the sums of squares of the stored values over a block, in units of the square of their granularity, stay
    below 2^24 — exact in fp32 in any order — for every block height the library may report, operand type and piece count."""
    for dt, planes in ((torch.bfloat16, 1), (torch.float16, 1), (torch.bfloat16, 2), (torch.bfloat16, 3)):
        if planes > 1 and c["name"] == "stats_rounding_operand":
            continue                                                                           # a 16-bit-operand case (see the table)
        xs, ws, bias, gb, res = T.exact_operands(c, planes, 1)
        stored = R.store(T.exact_value(c, xs, ws, bias, gb, res, planes), c["out"], dt, planes)[0]
        for rows in (128, 160, 288):
            assert T.stats_exact_bits(stored, rows) < 2 ** 24, (c["name"], dt, planes, rows)


def test_alpha_cases_are_exact():
    for alpha in (1.0, 0.5, 2.0, 0.0):
        for planes in (1, 2, 3):
            assert T.exactness(T.G("a", 130, 72, 128, "", alpha=alpha, bias=True, res=T.F32K, out=T.F32K), planes)[0] < 2 ** 24


def test_constructors():
    x = T.onehot_x(300, 64)
    assert bool((x.sum(1) == 1).all()) and bool(((x == 0) | (x == 1)).all())
    assert len(set(x.argmax(1).tolist())) == 64                                                # every channel is named
    assert not torch.equal(T.onehot_x(300, 64, 1), x)
    w = T.asym_w(136, 576)
    assert float(w.min()) == -3 and float(w.max()) == 3
    assert not bool((w[:, 1:] == w[:, :-1]).any()) and not bool((w[1:] == w[:-1]).all(1).any())
    assert not torch.equal(w, w.flip(1)) and not torch.equal(T.asym_w(136, 576, 1), w)
    f, y, xx = T.conv_coords(3, 5, 7)
    p = T.position_x((f, y, xx), 8)
    assert torch.equal(p[:, 0], (f % 7 - 3).float()) and torch.equal(p[:, 1], (y % 7 - 3).float()) and torch.equal(p[:, 2], (xx % 7 - 3).float())
    assert torch.equal(p[:, 3], p[:, 0]) and float(p.abs().max()) <= 3
    # two horizontally / vertically adjacent pixels and two frames never carry the same code
    img = p.reshape(3, 5, 7, 8)
    assert not bool((img[:, :, 1:] == img[:, :, :-1]).all(-1).any()) and not bool((img[:, 1:] == img[:, :-1]).all(-1).any())
    assert not bool((img[1:] == img[:-1]).all(-1).any())
    fine, shift = T.gate_sweep()
    for v in fine + shift:                                                                     # 8 significand bits: exact in bf16 and fp16
        t = torch.tensor([v])
        assert torch.equal(t.bfloat16().float(), t) and torch.equal(t.half().float(), t)


def test_phi_table_interpolation_bound():
    """h^2 / 8 max|Phi''| at h = 1/64 is what linear interpolation of Phi between its nodes costs: measured on a fine grid in fp64."""
    x = torch.linspace(-8, 8, 1024 * 64 + 1, dtype=F64)
    phi = lambda t: 0.5 * torch.erfc(-t / math.sqrt(2.0))
    lo = torch.floor(x * 64) / 64
    f = (x - lo) * 64
    err = (phi(lo) + f * (phi(lo + 1 / 64) - phi(lo)) - phi(x)).abs().max()
    assert float(err) <= (1 / 64) ** 2 / 8 * 0.24197072451914337 <= 7.4e-6


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("c", T.BOUNDED_CASES, ids=lambda c: c["name"])
def test_flip_cap_leaves_head_room_over_plain_fp32(c, dt):
    """The cap of the bounded 16-bit tests is a condition on the inputs: the same formula in plain fp32 torch, stored the same way, stays under
    a quarter of it in every 32 x 64 block, at every shape and seed the GPU file uses, for both 16-bit operand types and both 16-bit kinds."""
    xs, ws, bias, res = T.random_operands(c, T.bounded_seed(c), dt, 1)
    want = T.value_of(c, xs, ws, bias, res, F64)
    plain = T.value_of(c, xs, ws, bias, res, torch.float32)
    for kdt in (dt, torch.float16):
        ok, mean, worst = T.flip_share(plain.float().to(kdt), want)
        assert bool(ok.all())
        assert worst <= T.FLIP_CAP / 4, (c["name"], kdt, worst)


@pytest.mark.parametrize("planes", [2, 3], ids=["bf16x3", "bf16x6"])
@pytest.mark.parametrize("c", T.BOUNDED_CASES, ids=lambda c: c["name"])
def test_flip_cap_leaves_head_room_in_the_split_builds(c, planes):
    """fp16 storage in the split builds: the pairs of canonical pieces a split build keeps (gemm_reference.split_kept, everything else in
    fp64) — bf16x3 drops (1,1) by design — and plain fp32 on the same operands each stay under a quarter of the cap in every block."""
    xs, ws, bias, res = T.random_operands(c, T.bounded_seed(c), torch.bfloat16, planes)
    want = T.value_of(c, xs, ws, bias, res, F64)
    for emu in (T.value_of(c, xs, ws, bias, res, F64, kept=planes), T.value_of(c, xs, ws, bias, res, torch.float32)):
        ok, mean, worst = T.flip_share(emu.float().half(), want)
        assert bool(ok.all())
        assert worst <= T.FLIP_CAP / 4, (c["name"], planes, worst)
