"""Every backward kernel of the training step (csrc/wgrad.hip, attention_bwd.hip, train.hip, optim.hip) called through its own C-ABI entry
and held to the plain fp64 definition in tests/backward_reference.py — evaluated on the very operands the kernel reads (made on the
CPU, rounded to the operand type once, the same values widened to fp64 for the reference), at shapes read off each kernel's dispatch
and tiling code.  What reaches what in csrc/rows_shared.h, the steps train.hip shares with norm.hip and misc.hip: fold4 through
group_colsum_kernel and gn_bwd_partial_kernel, block_sum4 through softmax_bwd_kernel and mse_partial_kernel, softmax_row_walk through
softmax_f32_kernel, store_mean_rstd through gn_stat_f32_kernel, gn_bwd_dz / silu_grad through gn_bwd_partial_kernel and gn_bwd_apply_kernel.

  exact      small-integer operands (-3 .. 3) make every product and every partial sum an integer below 2^24, which fp32 holds
             exactly: torch.equal, so one misplaced, dropped or doubled term fails.  Each test asserts its magnitude condition.
  fp32       the kernels whose inputs are fp32 see the reference's numbers; bound = max(TOL_F32 = 2e-5 — accumulation order only, as in
             test_kernels_gpu.py — , 4 x the rel-L2 error plain fp32 torch makes on the same formula on the CPU): cancellation is the
             operation's property, not the kernel's.  Whole tensor, every 64-row block and every 64-column block.
  attention  mudg_attention_bwd rounds P and dS to the operand type before its MFMAs; bound = 3 x the rel-L2 distance from fp64 of an fp64
             evaluation that rounds exactly those two matrices.  Whole tensor and every 32-row block.
Every figure is printed next to its bound (lines with "rel-L2")."""
import ctypes as C
import math

import pytest
import torch

import backward_reference as R
from mudg_amd import hip, ops
from mudg_amd.train import functions as F
from mudg_amd.train import kernels as K

pytestmark = pytest.mark.gpu

TOL_F32 = 2e-5            # tests/test_kernels_gpu.py: fp32 results on identical inputs differ by accumulation order only
NAN = float("nan")
SPLIT = hip.planes() > 1
ONLY16 = pytest.mark.skipif(SPLIT, reason="mudg_wgrad / mudg_attention_bwd belong to the 16-bit operand builds; the split builds take "
                                          "transposed copies + mudg_gemm (tested here through wgrad_gemm) and recompute P explicitly")


def _s():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed=0, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=gen(seed), dtype=torch.float32) * scale + shift


def ints(*shape, seed=0):
    """Integers in -3 .. 3 as fp32: exact in bf16 and fp16, and so is every product and every sum of fewer than 2^24 / 9 of them."""
    return torch.randint(-3, 4, shape, generator=gen(seed)).to(torch.float32)


def rounded(x):
    """fp32 values that the operand type of the loaded library holds exactly."""
    return x.to(hip.operand_dtype()).to(torch.float32)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _block_errors(d2, w2, block):
    """rel-L2 of every block of `block` consecutive entries of two vectors of squared sums."""
    n = (d2.numel() + block - 1) // block * block
    pad = lambda v: torch.cat([v, v.new_zeros(n - v.numel())]).reshape(-1, block).sum(1)
    return torch.sqrt(pad(d2)) / torch.sqrt(pad(w2)).clamp_min(1e-300)


def check(name, got, want, bound, base=None, rb=64, cb=64):
    """got against want (2-D): whole tensor, every block of rb rows and every block of cb columns within `bound`; printed."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
    got, want = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    d2, w2 = (got - want) ** 2, want ** 2
    whole = float(torch.sqrt(d2.sum()) / torch.sqrt(w2.sum()).clamp_min(1e-300))
    rows = _block_errors(d2.sum(1), w2.sum(1), rb)
    cols = _block_errors(d2.sum(0), w2.sum(0), cb) if cb else rows[:1] * 0
    wr, wc = float(rows.max()), float(cols.max())
    print(f"[backward {hip.operand_name()}] {name}: rel-L2 {whole:.3e}, worst {rb}-row block {wr:.3e} (#{int(rows.argmax())}), worst "
          f"{cb}-column block {wc:.3e} (#{int(cols.argmax())}), bound {bound:.3e}" + (f" (cpu fp32 {base:.3e})" if base is not None else ""))
    assert whole <= bound, (name, "whole tensor", whole, bound)
    assert wr <= bound, (name, f"rows {int(rows.argmax()) * rb}..", wr, bound)
    assert wc <= bound, (name, f"columns {int(cols.argmax()) * cb}..", wc, bound)
    return whole


def check_f32(name, got, ref_fn, **blocks):
    """A kernel with fp32 inputs against ref_fn(dtype): fp64 is the yardstick, the same formula in fp32 on the CPU sets the bound."""
    want, plain = ref_fn(torch.float64), ref_fn(torch.float32)
    if not isinstance(want, (tuple, list)):
        got, want, plain = [got], [want], [plain]
    for i, (g, w, p) in enumerate(zip(got, want, plain)):
        base = rel_l2(p, w)
        check(f"{name}[{i}]" if len(want) > 1 else name, g, w, max(TOL_F32, 4.0 * base), base, **blocks)


def gapped(x, ld, dev, dtype=None, guard=0):
    """x [rows][cols] on the device as a view of a NaN-filled [guard + rows + guard][ld] tensor: the gap columns and the guard rows
    are never data."""
    rows, cols = x.shape
    big = torch.full((rows + 2 * guard, ld), NAN, dtype=dtype or x.dtype)
    big[guard:guard + rows, :cols] = x.to(big.dtype)
    return big.to(dev)[guard:guard + rows, :cols]


def base_of(t):
    return t if t._base is None else t._base


def filled_operand(rows, cols, dev, fill):
    """An operand matrix [rows][cols] (every piece of a split build) filled with `fill`."""
    out = ops.empty_rows(rows, cols, ops.H16(), dev)
    base_of(out).fill_(fill)
    return out


def pieces_of(t):
    """The pieces of an operand matrix, each [rows][cols], on the CPU."""
    base, planes = base_of(t), hip.planes()
    if planes == 1:
        return [t.cpu()]
    w = base.shape[1] // planes
    return [base[:t.shape[0], pl * w:pl * w + t.shape[1]].cpu() for pl in range(planes)]


def check_operand(name, out, want32, written, fill):
    """Operand matrix `out` holds want32 [rows][written] (fp32) piece by piece, bit for bit; the pieces add up to the value to the
    precision their count carries; columns from `written` on keep `fill`."""
    want = R.operand_planes(want32, hip.operand_dtype(), hip.planes())
    got = pieces_of(out)
    for pl, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g[:, :written], w), (name, "piece", pl, int((g[:, :written] != w).sum()))
        assert bool((g[:, written:] == fill).all()), (name, "piece", pl, "columns beyond the padded width were written")
    back = sum(g[:, :written].double() for g in got)
    bits = (11 if hip.operand_name() == "fp16" else 8) * hip.planes()
    err = (back - want32.double()).abs()
    slack = 2.0 ** -24 if hip.operand_name() == "fp16" else 1e-37          # fp16 goes subnormal below 6e-5: absolute steps of 2^-24
    assert bool((err <= want32.double().abs() * 2.0 ** -bits + slack).all()), (name, "the pieces do not add up to the value", float(err.max()))


# ================================================================================================ exact: weight gradients
def call_wgrad(a, b, P, M, Cc, taps, mode, geo, slices, chunk):
    """mudg_wgrad itself, with the slicing given: fp32 slabs [slices][M][taps C], pre-filled with NaN."""
    slabs = torch.full((slices, M, taps * Cc), NAN, dtype=torch.float32, device=a.device)
    g = dict(Hin=0, Win=0, Hout=0, Wout=0, stride=1, pad=1, T=0, HW=0)
    g.update(geo or {})
    d = hip.WgradDesc()
    d.A, d.B, d.out = a.data_ptr(), b.data_ptr(), slabs.data_ptr()
    d.lda, d.ldb, d.P = a.stride(0), b.stride(0), P
    d.M, d.C, d.taps, d.mode = M, Cc, taps, mode
    d.Hin, d.Win, d.Hout, d.Wout, d.stride, d.pad, d.T, d.HW = g["Hin"], g["Win"], g["Hout"], g["Wout"], g["stride"], g["pad"], g["T"], g["HW"]
    d.slices, d.chunk = slices, chunk
    hip.check(hip.lib().mudg_wgrad(C.byref(d), _s()), "mudg_wgrad")
    return slabs


def conv_geo(h, w, stride):
    return dict(Hin=h, Win=w, Hout=(h - 1) // stride + 1, Wout=(w - 1) // stride + 1, stride=stride, pad=1)


def expected_path(mode, geo):
    """The geometry path mudg_wgrad takes (csrc/wgrad.hip, `gm`), restated from its dispatch conditions."""
    if mode == 0:
        return 0
    if mode == 1:
        hw = geo["Hout"] * geo["Wout"]
        same = geo["stride"] == 1 and geo["Hin"] == geo["Hout"] and geo["Win"] == geo["Wout"]
        return 1 if same and hw % 64 == 0 and (geo["Wout"] % 64 == 0 or 64 % geo["Wout"] == 0) else 3
    return 2 if geo["HW"] % 64 == 0 else 3


# (path, mode, geometry, frames or clips, M, C, chunk, lda - M, ldb - C)
WGRAD_CASES = [
    # path 0: linear layers.  One slice; three slices with a ragged last K-step (1000 = 384 + 384 + 232, 232 = 3 * 64 + 40); four slices
    (0, 0, None, 1000, 8, 64, 1024, 0, 0),
    (0, 0, None, 1000, 136, 192, 384, 8, 64),
    (0, 0, None, 4100, 328, 320, 1088, 24, 8),
    # path 1: same-size 3x3 conv, (H W) % 64 == 0 and W % 64 == 0 or 64 % W == 0: W = 16 (four image rows per K-step), 64, 128
    (1, 1, conv_geo(8, 16, 1), 5, 72, 128, 640, 0, 0),
    (1, 1, conv_geo(3, 64, 1), 4, 136, 64, 320, 8, 8),
    (1, 1, conv_geo(2, 128, 1), 3, 8, 192, 256, 16, 0),
    # path 2: temporal taps, HW % 64 == 0
    (2, 2, dict(T=5, HW=64), 2, 72, 64, 640, 0, 8),
    (2, 2, dict(T=3, HW=128), 3, 328, 128, 448, 8, 0),
    # path 3: everything else.  Stride 2 on odd grids; W = 40 ((H W) % 64 == 0 but neither W condition); H W % 64 != 0; temporal HW = 7
    (3, 1, conv_geo(9, 7, 2), 7, 136, 64, 192, 0, 0),
    (3, 1, conv_geo(17, 15, 2), 5, 72, 192, 128, 8, 8),
    (3, 1, conv_geo(8, 40, 1), 3, 72, 320, 512, 0, 24),
    (3, 1, conv_geo(5, 16, 1), 5, 8, 128, 192, 8, 0),
    (3, 2, dict(T=5, HW=7), 3, 72, 192, 64, 8, 8),
]


def wgrad_problem(mode, geo, n, M, Cc, seed):
    """Integer operands of a weight gradient: (P, rows of B, taps, a [P][M], b [rows][C])."""
    if mode == 0:
        P, brows, taps = n, n, 1
    elif mode == 1:
        P, brows, taps = n * geo["Hout"] * geo["Wout"], n * geo["Hin"] * geo["Win"], 9
    else:
        P, brows, taps = n * geo["T"] * geo["HW"], n * geo["T"] * geo["HW"], 3
    return P, brows, taps, ints(P, M, seed=seed), ints(brows, Cc, seed=seed + 1)


@ONLY16
@pytest.mark.parametrize("case", range(len(WGRAD_CASES)))
def test_wgrad_is_exact_on_integer_operands_on_every_geometry_path(cuda, case):
    path, mode, geo, n, M, Cc, chunk, gap_a, gap_b = WGRAD_CASES[case]
    assert expected_path(mode, geo) == path
    P, brows, taps, a, b = wgrad_problem(mode, geo, n, M, Cc, 100 + case)
    # |a b| <= 9 per term: every partial sum is an integer of magnitude <= 9 P < 2^24, exact in the fp32 accumulators
    assert 9 * P < 2 ** 24 and P <= 10 ** 5
    slices = (P + chunk - 1) // chunk
    a16 = gapped(a, M + gap_a, cuda, hip.operand_dtype(), guard=2)            # NaN in the gap columns and in the rows around the operand
    b16 = gapped(b, Cc + gap_b, cuda, hip.operand_dtype(), guard=2)
    slabs = call_wgrad(a16, b16, P, M, Cc, taps, mode, geo, slices, chunk).cpu()
    for s in range(slices):
        p0, p1 = s * chunk, min(P, (s + 1) * chunk)
        want = R.wgrad(a, b, P, M, Cc, taps, mode, geo, p_range=(p0, p1))
        assert float(want.abs().max()) < 2 ** 24
        bad = slabs[s].double() != want
        assert not bool(bad.any()), (f"path {path} slice {s} (positions {p0}..{p1}): {int(bad.sum())} wrong elements, first at "
                                     f"{bad.nonzero()[0].tolist()} (row m, column tap C + c), got {slabs[s][bad][0]}, want {want[bad][0]}")
    print(f"[backward {hip.operand_name()}] mudg_wgrad path {path} P={P} M={M} C={Cc} taps={taps} slices={slices}: exact")


@ONLY16
@pytest.mark.parametrize("which", ["mdm512 level-0 conv 16 x 40 x 64, 320 -> 320", "1280-wide linear"])
def test_wgrad_is_exact_at_shapes_of_the_real_network(cuda, which):
    """Through kernels.wgrad — its slicing rule and the slab sum included."""
    if which.startswith("mdm512"):
        mode, geo, n, M, Cc = 1, conv_geo(40, 64, 1), 16, 320, 320
        assert expected_path(mode, geo) == 1
    else:
        mode, geo, n, M, Cc = 0, None, 4100, 1280, 1280
    P, brows, taps, a, b = wgrad_problem(mode, geo, n, M, Cc, 300)
    assert 9 * P < 2 ** 24 and P <= 10 ** 5
    a16, b16 = a.to(hip.operand_dtype()).to(cuda), b.to(hip.operand_dtype()).to(cuda)
    got = K.wgrad(a16, b16, positions=P, m=M, c=Cc, taps=taps, mode=mode, geo=geo).cpu()
    want = R.wgrad(a, b, P, M, Cc, taps, mode, geo)
    assert float(want.abs().max()) < 2 ** 24
    bad = got.double() != want
    assert not bool(bad.any()), (which, int(bad.sum()), bad.nonzero()[0].tolist())
    print(f"[backward {hip.operand_name()}] kernels.wgrad {which}: P={P}, exact")


@pytest.mark.parametrize("kind", ["linear", "conv stride 2 odd grid", "conv 8 x 16 K-slices", "temporal"])
def test_wgrad_gemm_over_transposed_operands_is_exact_on_integer_operands(cuda, kind):
    """The route of the split builds (and of widths mudg_wgrad does not take): transposed, tap-gathered operand copies contracted by
    mudg_gemm in K-slices — the project's own packing (functions.transposed / transposed_taps) on the same integer operands."""
    mode, geo, n, M, Cc = {"linear": (0, None, 1100, 72, 192), "conv stride 2 odd grid": (1, conv_geo(9, 7, 2), 4, 72, 64),
                           "conv 8 x 16 K-slices": (1, conv_geo(8, 16, 1), 10, 72, 64), "temporal": (2, dict(T=5, HW=64), 2, 136, 72)}[kind]
    P, brows, taps, a, b = wgrad_problem(mode, geo, n, M, Cc, 400)
    assert 9 * P < 2 ** 24 and P <= 10 ** 5
    dy, x = a.to(cuda), b.to(cuda)
    at = F.transposed(dy, M, taps * Cc)
    if mode == 0:
        bt = F.transposed(x, M, Cc)
    else:
        offs = [R.tap_offsets(mode, t) for t in range(taps)]
        bt = F.transposed_taps(x, M, Cc, P, offs, mode, geo)
    got = F.wgrad_gemm(at, bt, M, taps * Cc, P).cpu()
    want = R.wgrad(a, b, P, M, Cc, taps, mode, geo)
    assert float(want.abs().max()) < 2 ** 24
    bad = got.double() != want
    assert not bool(bad.any()), (kind, int(bad.sum()), bad.nonzero()[0].tolist())
    print(f"[backward {hip.operand_name()}] wgrad_gemm {kind}: P={P} K-slices={F._splits(M, taps * Cc, P)}, exact")


# ================================================================================================ exact: transposes, sums, resampling
@pytest.mark.parametrize("kind", ["plain", "conv tap stride 2", "conv tap same size", "temporal tap", "batched"])
def test_transpose_gather_writes_the_cast_the_zero_padding_and_nothing_else(cuda, kind):
    Cc, fill = 72, 7.0
    if kind == "plain":
        mode, geo, P, srows, taps = 0, None, 203, 203, [{}]
    elif kind == "conv tap stride 2":
        mode, geo = 1, conv_geo(9, 7, 2)
        P, srows, taps = 3 * 20, 3 * 63, [dict(dy=t // 3, dx=t % 3) for t in range(9)]
    elif kind == "conv tap same size":
        mode, geo = 1, conv_geo(5, 13, 1)
        P, srows, taps = 2 * 65, 2 * 65, [dict(dy=t // 3, dx=t % 3) for t in (0, 2, 4, 6, 8)]
    elif kind == "temporal tap":
        mode, geo, P, srows, taps = 2, dict(T=5, HW=7), 70, 70, [dict(dt=t) for t in range(3)]
    else:
        mode, geo, P, srows, taps = 0, None, 77, 3 * 77, [{}]
    src = rnd(srows, Cc, seed=500)
    dsrc = gapped(src, Cc + 4, cuda)
    width = R.ceil8(P) + 16
    for tap in taps:
        if kind == "batched":
            out = filled_operand(3 * Cc, width, cuda, fill)
            K.transpose_gather(dsrc, P=P, out=out, batch=3, src_batch_rows=P, dst_batch_rows=Cc)
            want = torch.cat([R.transpose_gather(src[z * P:(z + 1) * P], P) for z in range(3)]).float()
        else:
            out = filled_operand(Cc, width, cuda, fill)
            K.transpose_gather(dsrc, P=P, mode=mode, geo=dict(geo or {}, **tap), out=out)
            want = R.transpose_gather(src, P, mode, geo, **tap).float()
        assert want.shape[1] == R.ceil8(P) and not bool(want[:, P:].any())
        check_operand(f"transpose_gather {kind} {tap}", out, want, R.ceil8(P), fill)
    print(f"[backward {hip.operand_name()}] mudg_transpose_gather {kind}: {len(taps)} taps, bit-equal, padding zero, fill kept")


@pytest.mark.parametrize("P,Cc", [(203, 72), (64, 64), (1, 4), (130, 260)])
def test_transpose_cast_sum_writes_all_three_forms(cuda, P, Cc):
    fill = 7.0
    width = R.ceil8(P) + 16
    # (a) any fp32 values: the transposed copy and the row copy are the operand cast, bit for bit
    src = rnd(P, Cc, seed=600)
    dsrc = gapped(src, Cc + 4, cuda)
    out = filled_operand(Cc, width, cuda, fill)
    rows, _ = K.transpose_cast_sum(dsrc, out, rows=True, sums=False)
    want_t, want_r, _ = R.transpose_cast_sum(src)
    check_operand("transpose_cast_sum dst", out, want_t.float(), R.ceil8(P), fill)
    check_operand("transpose_cast_sum rows", rows, want_r.float(), Cc, fill)
    # (b) integers: the per-64-row column sums are exact (|sum| <= 3 * 64 < 2^24), with and without the other outputs
    src = ints(P, Cc, seed=601)
    assert 3 * 64 < 2 ** 24
    dsrc = gapped(src, Cc + 4, cuda)
    want_t, want_r, want_p = R.transpose_cast_sum(src)
    for with_dst in (True, False):
        out = filled_operand(Cc, width, cuda, fill) if with_dst else None
        part = torch.full(((P + 63) // 64, Cc), NAN, dtype=torch.float32, device=cuda)
        hip.check(hip.lib().mudg_transpose_cast_sum(dsrc.data_ptr(), dsrc.stride(0), None if out is None else out.data_ptr(),
                                                    0 if out is None else out.stride(0), None, 0, part.data_ptr(), P, Cc, _s()), "mudg_transpose_cast_sum")
        assert torch.equal(part.cpu().double(), want_p), ("part", with_dst)
        if with_dst:
            check_operand("transpose_cast_sum dst (integers)", out, want_t.float(), R.ceil8(P), fill)
    _, total = K.transpose_cast_sum(dsrc, None, rows=False, sums=True)
    assert 3 * P < 2 ** 24 and torch.equal(total.cpu().double(), src.double().sum(0))
    print(f"[backward {hip.operand_name()}] mudg_transpose_cast_sum P={P} C={Cc}: bit-equal casts, exact tile sums")


@pytest.mark.parametrize("rows,cols,rpg,with_b", [(21, 70, 7, False), (21, 70, 7, True), (1030, 64, 1030, True), (6, 200, 1, False),
                                                  (4 * 2049, 33, 2049, True), (9 * 1024, 65, 3072, False)])
def test_group_colsum_is_exact_on_integers(cuda, rows, cols, rpg, with_b):
    a, b = ints(rows, cols, seed=700), (ints(rows, cols, seed=701) if with_b else None)
    assert 9 * rpg < 2 ** 24                                   # |a b| <= 9: every group sum is an exact fp32 integer
    da, db = gapped(a, cols + 3, cuda), (gapped(b, cols + 5, cuda) if with_b else None)
    want = R.group_colsum(a, b, rpg)
    got = K._colsum_once(da, db, rpg).cpu().double()
    assert torch.equal(got, want), int((got != want).sum())
    assert torch.equal(K.group_colsum(da, db, rows_per_group=rpg).cpu().double(), want)           # two launches where a group is long
    print(f"[backward {hip.operand_name()}] mudg_group_colsum rows={rows} cols={cols} rows_per_group={rpg} b={with_b}: exact")


@pytest.mark.parametrize("frames,hi,wi,Cc", [(2, 9, 7, 5), (3, 8, 6, 64), (1, 1, 1, 3), (2, 5, 12, 70)])
def test_dilate2x_and_upsample2x_adjoint_are_exact_on_integers(cuda, frames, hi, wi, Cc):
    ho, wo = (hi - 1) // 2 + 1, (wi - 1) // 2 + 1
    dy = ints(frames * ho * wo, Cc, seed=800)
    got = K.dilate2x(dy.to(cuda), frames, ho, wo, hi, wi).cpu()
    assert torch.equal(got, R.dilate2x(dy, frames, ho, wo, hi, wi))
    g = ints(frames * 4 * hi * wi, Cc, seed=801)                # the adjoint at the odd size hi x wi: sums of four, |sum| <= 12 < 2^24
    assert 4 * 3 < 2 ** 24
    got = K.upsample2x(g.to(cuda), frames, hi, wi, adjoint=True).cpu().double()
    assert torch.equal(got, R.upsample2x(g, frames, hi, wi, adjoint=True))
    x = rnd(frames * hi * wi, Cc, seed=802)
    assert torch.equal(K.upsample2x(x.to(cuda), frames, hi, wi).cpu().double(), R.upsample2x(x, frames, hi, wi))
    print(f"[backward {hip.operand_name()}] mudg_dilate2x / mudg_upsample2x {frames} x {hi} x {wi} x {Cc}: exact")


# ================================================================================================ fp32 kernels: norms
def gn_bwd_raw(x, dy, gamma, beta, stat, samples, rows, groups, silu, dres):
    """mudg_groupnorm_bwd itself: (dX, AB [samples][C][2])."""
    c = x.shape[1]
    dx = torch.full((samples * rows, c), NAN, dtype=torch.float32, device=x.device)
    ab = torch.full((samples, c, 2), NAN, dtype=torch.float32, device=x.device)
    ws = torch.empty(hip.lib().mudg_groupnorm_bwd_ws_floats(samples, rows, c, groups), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().mudg_groupnorm_bwd(x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), gamma.data_ptr(), beta.data_ptr(),
                                           stat.data_ptr(), samples, rows, c, groups, int(silu), dx.data_ptr(), dx.stride(0), ab.data_ptr(),
                                           ws.data_ptr(), None if dres is None else dres.data_ptr(), 0 if dres is None else dres.stride(0),
                                           _s()), "mudg_groupnorm_bwd")
    return dx, ab


# (C, rows, samples, SiLU, dres, ldx - C, mean of x / its spread).  32 groups: 2 .. 80 channels per group; rows / 256 chunks: 50, 255 -> 1,
# 256, 257 -> 1, 513 -> 2 (257 + 256 rows), 70 000 -> 273 clamped to 256 (274 rows each, the last 130)
GN_CASES = [
    (64, 70000, 1, True, False, 0, 0.0),
    (320, 50, 3, True, True, 0, 0.0),
    (320, 513, 2, False, False, 8, 0.0),
    (960, 255, 2, True, False, 0, 0.0),
    (1280, 256, 1, False, True, 4, 0.0),
    (1280, 257, 2, True, False, 0, 50.0),
    (1920, 257, 2, True, False, 0, 0.0),
    (2560, 513, 1, True, True, 0, 0.0),
    (2560, 50, 3, False, False, 16, 0.0),
    (320, 70000, 1, False, True, 0, 0.0),
]


@pytest.mark.parametrize("case", range(len(GN_CASES)))
def test_groupnorm_stats_and_backward(cuda, case):
    c, rows, samples, silu, with_res, gap, shift = GN_CASES[case]
    groups, eps = 32, 1e-5
    x = rnd(samples * rows, c, seed=900 + case, scale=1.3, shift=shift * 1.3)
    dy = rnd(samples * rows, c, seed=920 + case)
    gamma, beta = rnd(c, seed=940 + case, shift=1.0, scale=0.3), rnd(c, seed=960 + case, scale=0.3)
    dres = rnd(samples * rows, c, seed=980 + case) if with_res else None
    dx_, ddy, dres_ = gapped(x, c + gap, cuda), gapped(dy, c + 8, cuda), (None if dres is None else gapped(dres, c + 4, cuda))
    tag = f"C={c} rows={rows} samples={samples} silu={int(silu)} dres={int(with_res)} ldx={c + gap} mean={shift:g} sigma"
    # the statistics: fp32 rows in, (mean, rstd) out
    stat = K.groupnorm_stats(dx_, samples, rows, groups, eps)
    check_f32(f"mudg_groupnorm_stats {tag}", stat, lambda dt: R.groupnorm_stats(x, samples, rows, groups, eps, dtype=dt), cb=1)   # mean | rstd
    # the backward pass on the statistics the reference itself computed (rounded to fp32 once: what both sides read)
    st = R.groupnorm_stats(x, samples, rows, groups, eps).float()
    got = gn_bwd_raw(dx_, ddy, gamma.to(cuda), beta.to(cuda), st.to(cuda), samples, rows, groups, silu, dres_)
    want, plain = (R.groupnorm_bwd(x, dy, gamma, beta, st, samples, rows, groups, silu, dres, dtype=dt) for dt in (torch.float64, torch.float32))
    base = rel_l2(plain[0], want[0])
    check(f"mudg_groupnorm_bwd dX {tag}", got[0], want[0], max(TOL_F32, 4 * base), base)
    for j, nm in enumerate(("sum dz", "sum dz xhat")):           # AB[s][c][j]: one row per sample, 64-channel blocks
        w, p = want[1][..., j], plain[1][..., j]
        base = rel_l2(p, w)
        check(f"mudg_groupnorm_bwd AB {nm} {tag}", got[1][..., j], w, max(TOL_F32, 4 * base), base, rb=1)


def ln_bwd_raw(x, dy, gamma, eps, dres):
    rows, c = x.shape
    dx = torch.full((rows, c), NAN, dtype=torch.float32, device=x.device)
    chunks = hip.lib().mudg_layernorm_bwd_chunks(rows)
    part = torch.full((chunks, 2, c), NAN, dtype=torch.float32, device=x.device)
    hip.check(hip.lib().mudg_layernorm_bwd(x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), gamma.data_ptr(), dx.data_ptr(), dx.stride(0),
                                           part.data_ptr(), rows, c, eps, None if dres is None else dres.data_ptr(),
                                           0 if dres is None else dres.stride(0), _s()), "mudg_layernorm_bwd")
    return dx, part


# (C, rows, dres): 64-column register blocks with C % 64 != 0 tails (72, 1276), the widest the kernel takes (1280 = 64 * 20), 64-row chunks
# with one row, one short, exactly one, one more, and 4100 = 64 * 64 + 4
LN_CASES = [(64, 1, False), (72, 63, True), (320, 64, False), (1024, 65, True), (1276, 4100, False), (1280, 65, False), (1280, 4100, True),
            (72, 4100, False), (1276, 1, True)]


@pytest.mark.parametrize("c,rows,with_res", LN_CASES)
def test_layernorm_backward(cuda, c, rows, with_res):
    eps = 1e-5
    x, dy = rnd(rows, c, seed=1000 + c + rows, scale=1.5, shift=0.3), rnd(rows, c, seed=1001 + c + rows)
    gamma = rnd(c, seed=1002 + c, shift=1.0, scale=0.3)
    dres = rnd(rows, c, seed=1003 + c) if with_res else None
    got = ln_bwd_raw(gapped(x, c + 4, cuda), gapped(dy, c + 12, cuda), gamma.to(cuda), eps, None if dres is None else gapped(dres, c + 8, cuda))
    assert got[1].shape[0] == (rows + 63) // 64
    tag = f"C={c} rows={rows} dres={int(with_res)}"
    want, plain = (R.layernorm_bwd(x, dy, gamma, eps, dres, dtype=dt) for dt in (torch.float64, torch.float32))
    base = rel_l2(plain[0], want[0])
    check(f"mudg_layernorm_bwd dX {tag}", got[0], want[0], max(TOL_F32, 4 * base), base)
    for j, nm in enumerate(("sum dy xhat", "sum dy")):           # part[chunk][j][C]: one row per 64-row chunk, 64-column blocks
        base = rel_l2(plain[1][:, j], want[1][:, j])
        check(f"mudg_layernorm_bwd part {nm} {tag}", got[1][:, j], want[1][:, j], max(TOL_F32, 4 * base), base, rb=1)


# ================================================================================================ fp32 kernels: softmax, temporal attention
@pytest.mark.parametrize("cols", [1, 77, 255, 256, 257, 1100])
@pytest.mark.parametrize("magnitude", [1.0, 80.0])
def test_softmax_and_softmax_backward(cuda, cols, magnitude):
    rows, scale = 130, 0.125
    s = (torch.rand(rows, cols, generator=gen(1100 + cols)) * 2 - 1) * magnitude          # scores in [-magnitude, magnitude]
    ld = cols + 5
    ds_ = gapped(s, ld, cuda)
    K.softmax_f32(ds_, cols)                                                            # in place over the first `cols` columns
    assert bool(torch.isnan(base_of(ds_)[:, cols:]).all()), "softmax wrote beyond `cols`"
    tag = f"rows={rows} cols={cols} |s|<={magnitude:g}"
    check_f32(f"mudg_softmax_f32 {tag}", ds_, lambda dt: R.softmax(s, dtype=dt))
    p = R.softmax(s).float()                                                            # the probabilities both sides read
    dp = rnd(rows, cols, seed=1101 + cols)
    out = torch.full((rows, ld), NAN, dtype=torch.float32, device=cuda)
    K.softmax_bwd(gapped(p, cols + 3, cuda), gapped(dp, cols + 9, cuda), out[:, :cols], cols, scale)
    assert bool(torch.isnan(out[:, cols:]).all())
    check_f32(f"mudg_softmax_bwd {tag}", out[:, :cols], lambda dt: R.softmax_bwd(p, dp, scale, dtype=dt))


@pytest.mark.parametrize("t,hw,heads,clips", [(1, 7, 1, 2), (5, 64, 5, 1), (16, 7, 5, 2), (17, 64, 1, 1), (20, 7, 5, 1), (32, 64, 1, 2),
                                              (32, 7, 5, 1), (16, 64, 1, 1)])
def test_temporal_attention_backward(cuda, t, hw, heads, clips):
    """tattn_bwd_kernel<16> serves T <= 16, <32> T <= 32: 1, 5, 16 | 17, 20, 32."""
    c, scale = heads * 64, 0.125
    qkv, do = rnd(clips * t * hw, 3 * c, seed=1200 + t), rnd(clips * t * hw, c, seed=1201 + t)
    got = K.temporal_attention_bwd(gapped(qkv, 3 * c + 4, cuda), gapped(do, c + 8, cuda), clips, t, hw, heads, scale)
    check_f32(f"mudg_temporal_attention_bwd T={t} HW={hw} heads={heads} clips={clips}", got,
              lambda dt: R.temporal_attention_bwd(qkv, do, clips=clips, t=t, hw=hw, heads=heads, scale=scale, dtype=dt))


# ================================================================================================ fp32 kernels: GEGLU, dropout, loss, clipping
@pytest.mark.parametrize("m,n", [(130, 100), (67, 324), (1, 4)])
def test_geglu_and_geglu_dropout(cuda, m, n):
    h, dy = rnd(m, 2 * n, seed=1300 + n, scale=1.5), rnd(m, n, seed=1301 + n)
    dh_, ddy = gapped(h, 2 * n + 4, cuda), gapped(dy, n + 8, cuda)
    check_f32(f"mudg_geglu M={m} N={n}", K.geglu(dh_), lambda dt: R.geglu(h, dtype=dt))
    check_f32(f"mudg_geglu backward M={m} N={n}", K.geglu(dh_, ddy), lambda dt: R.geglu(h, dy, dtype=dt))
    for p, seed in ((0.0, 5), (0.1, 77), (0.5, 2 ** 40 + 3)):
        keep = R.keep_mask(seed, m * n, p).reshape(m, n)
        # the mask itself, through mudg_dropout_rows on ones and on data (the element index is m C + c whatever the row strides)
        y, y16 = K.dropout_rows(gapped(torch.ones(m, n), n + 4, cuda), p, seed, operand=True)
        assert torch.equal(y.cpu() != 0, keep), "the keep mask is not the documented one"
        check_operand("dropout_rows operand rows", y16, y.cpu(), n, 0.0)
        y, _ = K.dropout_rows(ddy, p, seed)
        assert torch.equal(y.cpu() != 0, keep & (dy != 0))
        check_f32(f"mudg_dropout_rows M={m} N={n} p={p}", y, lambda dt: R.dropout_rows(dy, keep, p, dtype=dt))
        out, o16 = K.geglu_dropout(dh_, p, seed, operand=True)
        check_f32(f"mudg_geglu_dropout M={m} N={n} p={p}", out, lambda dt: R.geglu_dropout(h, keep, p, dtype=dt))
        check_operand("geglu_dropout operand rows", o16, out.cpu(), n, 0.0)
        assert bool((out.cpu()[~keep] == 0).all()), "a dropped element is not zero"
        check_f32(f"mudg_geglu_dropout backward M={m} N={n} p={p}", K.geglu_dropout(dh_, p, seed, dy=ddy),
                  lambda dt: R.geglu_dropout(h, keep, p, dy, dtype=dt))


@pytest.mark.parametrize("shape", [(3, 4, 5, 7, 9), (2, 100003), (1, 1), (5, 4, 16, 40, 64)])
def test_weighted_mse_and_its_gradient(cuda, shape):
    pred, target = rnd(*shape, seed=1400), rnd(*shape, seed=1401)
    w = rnd(shape[0], seed=1402).abs() + 0.1
    loss, grad = K.mse(pred.to(cuda), target.to(cuda), w.to(cuda), want_grad=True)
    flat = lambda v: v.reshape(shape[0], -1)
    for dt_name, g, f in (("loss", loss[None], lambda dt: R.mse(pred, target, w, dtype=dt)[0][None]),
                          ("gradient", flat(grad), lambda dt: flat(R.mse(pred, target, w, dtype=dt)[1]))):
        want, plain = f(torch.float64), f(torch.float32)
        base = rel_l2(plain, want)
        check(f"mudg_mse {dt_name} {shape}", g, want, max(TOL_F32, 4 * base), base, rb=1 if dt_name == "gradient" else 64)
    loss_only, none = K.mse(pred.to(cuda), target.to(cuda))
    assert none is None and torch.equal(loss_only, loss)


@pytest.mark.parametrize("max_norm", [0.5, 1e6])
def test_clip_grad_norm(cuda, max_norm):
    chunk = hip.lib().mudg_clip_chunk()
    sizes = [(5, 3), (chunk,), (chunk + 1,), (3 * chunk + 17,), (1,), (320, 77)]           # chunk tails of 15, full, 1, 17, 1 values
    grads = [rnd(*s, seed=1500 + i, scale=0.01 * (i + 1)) for i, s in enumerate(sizes)]
    dev = [g.to(cuda) for g in grads]
    table, n = K.chunk_table([(g,) for g in dev])
    partial = torch.empty(n, dtype=torch.float64, device=cuda)
    out = torch.full((2,), NAN, dtype=torch.float32, device=cuda)
    hip.check(hip.lib().mudg_clip_grad_norm(table.data_ptr(), n, partial.data_ptr(), max_norm, out.data_ptr(), _s()), "mudg_clip_grad_norm")
    ref = lambda dt: R.clip_grad_norm(grads, max_norm, dtype=dt)
    want, plain = ref(torch.float64), ref(torch.float32)
    for j, nm in enumerate(("norm", "coefficient")):
        base = rel_l2(plain[j], want[j])
        check(f"mudg_clip_grad_norm {nm} max_norm={max_norm:g}", out[j].reshape(1, 1), want[j].reshape(1, 1), max(TOL_F32, 4 * base), base)
    for i, (g, w, p) in enumerate(zip(dev, want[2], plain[2])):
        if max_norm > 1.0:
            assert torch.equal(g.cpu(), grads[i]), "a coefficient of 1 leaves the gradients untouched"
        base = rel_l2(p, w)
        check(f"mudg_clip_grad_norm tensor {i} {sizes[i]} max_norm={max_norm:g}", g.reshape(1, -1), w.reshape(1, -1), max(TOL_F32, 4 * base), base,
              cb=4096)


def test_multi_tensor_optimiser_kernels_against_their_definitions(cuda):
    """mudg_adamw_multi = mudg_adamw per element, bit for bit, and AdamW in fp64 within the fp32 bound; mudg_ema_multi is LitEma's
    update with every operation rounded on its own; mudg_adamw_ema_multi is the two in a row; mudg_swap_multi exchanges."""
    chunk = hip.lib().mudg_clip_chunk()
    sizes = [7, chunk, chunk + 3, 2 * chunk + 1, 12]
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))                  # the C-ABI takes the hyperparameters as fp32
    hp = dict(lr=f32(1e-3), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(0.01))
    mk = lambda seed, scale=1.0, positive=False: [(rnd(n, seed=seed + i, scale=scale).abs() if positive else rnd(n, seed=seed + i, scale=scale))
                                                   for i, n in enumerate(sizes)]
    p0, g0, m0, v0, sh0 = mk(1600), mk(1610, 0.1), mk(1620, 0.05), mk(1630, 0.01, True), mk(1640)
    step, omd = 3, 0.0123
    dev = lambda ts: [t.to(cuda) for t in ts]
    # one tensor at a time
    p1, g1, m1, v1 = dev(p0), dev(g0), dev(m0), dev(v0)
    for t in zip(p1, g1, m1, v1):
        K.adamw_(*t, step=step, **hp)
    # all in one launch
    p2, g2, m2, v2 = dev(p0), dev(g0), dev(m0), dev(v0)
    table, n = K.chunk_table(list(zip(p2, g2, m2, v2)))
    K.adamw_multi_(table, n, step=step, **hp)
    for a, b in zip(p1 + m1 + v1, p2 + m2 + v2):
        assert torch.equal(a, b)
    for i in range(len(sizes)):                                  # AdamW (decoupled decay, bias correction) in fp64
        def adamw(dt):
            p, g, m, v = (t[i].to(dt) for t in (p0, g0, m0, v0))
            m_ = hp["betas"][0] * m + (1 - hp["betas"][0]) * g
            v_ = hp["betas"][1] * v + (1 - hp["betas"][1]) * g * g
            p_ = p * (1 - hp["lr"] * hp["weight_decay"])
            den = torch.sqrt(v_) / math.sqrt(1 - hp["betas"][1] ** step) + hp["eps"]
            return (p_ - hp["lr"] / (1 - hp["betas"][0] ** step) * m_ / den)[None], m_[None], v_[None]
        check_f32(f"mudg_adamw_multi tensor {i} n={sizes[i]}", (p2[i][None], m2[i][None], v2[i][None]), adamw)
    # EMA: shadow - omd * (shadow - param), each operation rounded to fp32 (bit-equal to the fp32 expression on the CPU)
    sh2 = dev(sh0)
    table, n = K.chunk_table(list(zip(sh2, p2)))
    K.ema_multi_(table, n, omd)
    for s_dev, s_cpu, p_dev in zip(sh2, sh0, p2):
        want = s_cpu - torch.tensor(omd, dtype=torch.float32) * (s_cpu - p_dev.cpu())
        assert torch.equal(s_dev.cpu(), want)
    # both in one launch
    p3, g3, m3, v3, sh3 = dev(p0), dev(g0), dev(m0), dev(v0), dev(sh0)
    table, n = K.chunk_table(list(zip(p3, g3, m3, v3, sh3)))
    K.adamw_ema_multi_(table, n, step=step, one_minus_decay=omd, **hp)
    for a, b in zip(p3 + m3 + v3 + sh3, p2 + m2 + v2 + sh2):
        assert torch.equal(a, b)
    # swap
    a, b = dev(p0), dev(sh0)
    table, n = K.chunk_table(list(zip(a, b)))
    K.swap_multi_(table, n)
    for x, y, x0, y0 in zip(a, b, p0, sh0):
        assert torch.equal(x.cpu(), y0) and torch.equal(y.cpu(), x0)
    print(f"[backward {hip.operand_name()}] multi-tensor optimiser kernels: bit-equal to the single-tensor kernels and to their definitions")


def test_the_multi_tensor_walk_at_its_edges_aligned_and_off_by_one_float(cuda):
    """Every kernel on csrc/optim.hip's multi_walk, at the sizes where the walk changes course (a piece = 256 lanes x 4 floats, two
    pieces per pass): 3 has no vector part; 1024 fills exactly the first piece and leaves the second empty; 1203 = 300 vectors + 3
    has lanes 0..43 live in the second piece; 2053 = 513 vectors + 1 runs a second pass with one live lane.  Every tensor is a
    view into its own sentinel-filled flat buffer: 16 bytes in (the vector branch), one float in (the scalar loop), and with the
    gradient alone one float in (one unaligned operand turns the whole row scalar).  The four AdamW forms equal mudg_adamw per
    tensor bit for bit — the scaled ones at scale 1 and coefficient 1, where (g * 1) * 1 is g —, the shadows equal the fp32
    expression on the CPU, mudg_swap_multi exchanges bits, a set overflow flag leaves parameters and moments alone and moves the
    shadows, and no sentinel changes.
    The step is 1: the scaled forms take b^n from powf on the device, the others from powf on the host, and b^1 = b is the
    exponent at which the two cannot differ."""
    sizes, sentinel = [3, 1024, 1203, 2053], -12345.0
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    hp = dict(lr=f32(1e-3), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(0.01))
    omd = 0.0123
    mk = lambda seed, scale=1.0: [rnd(n, seed=seed + i, scale=scale) for i, n in enumerate(sizes)]
    p0, g0, m0, v0, sh0 = mk(1700), mk(1710, 0.1), mk(1720, 0.05), [t.abs() for t in mk(1730, 0.01)], mk(1740)
    ref = [[t.to(cuda) for t in ts] for ts in (p0, g0, m0, v0)]                   # the yardstick: one tensor at a time, once
    for t in zip(*ref):
        K.adamw_(*t, step=1, **hp)
    p1, _, m1, v1 = [[t.cpu() for t in ts] for ts in ref]
    ema_of = lambda shadows, params: [s - torch.tensor(omd, dtype=torch.float32) * (s - p) for s, p in zip(shadows, params)]
    stat = torch.tensor([0.25, 1.0], dtype=torch.float32).to(cuda)              # [norm, clip coefficient]
    record = lambda flag: torch.tensor([0x3F800000, 0, flag, 0], dtype=torch.int32).to(cuda)      # scale 1.0, no step taken yet

    def lay(operands, off_of):
        """views[k][i]: tensor i of operand k, off_of(k) floats into a flat buffer of sentinels; and the check that they are intact."""
        flats, views = [], []
        for k, ts in enumerate(operands):
            off = off_of(k)
            row = []
            for t in ts:
                flat = torch.full((t.numel() + 8,), sentinel)
                flat[off:off + t.numel()] = t
                flats.append((flat.to(cuda), off, t.numel()))
                row.append(flats[-1][0][off:off + t.numel()])
                assert row[-1].data_ptr() % 16 == 4 * off % 16
            views.append(row)

        def intact():
            for flat, off, n in flats:
                flat = flat.cpu()
                assert bool((flat[:off] == sentinel).all()) and bool((flat[off + n:] == sentinel).all()), "a sentinel was overwritten"
        return views, intact

    def run(what, off_of, launch, want, shadow=False):
        views, intact = lay([p0, g0, m0, v0] + ([sh0] if shadow else []), off_of)
        table, n = K.chunk_table(list(zip(*views)))
        launch(table, n)
        for k, (got, exp) in enumerate(zip(views, want)):
            for i, (a, b) in enumerate(zip(got, exp)):
                assert torch.equal(a.cpu(), b), (what, f"operand {k}", sizes[i])
        intact()

    for where, off_of in (("aligned", lambda k: 4), ("one float off", lambda k: 1), ("gradient alone off", lambda k: 1 if k == 1 else 4)):
        run(f"mudg_adamw_multi, {where}", off_of, lambda t, n: K.adamw_multi_(t, n, step=1, **hp), (p1, g0, m1, v1))
        run(f"mudg_adamw_ema_multi, {where}", off_of, lambda t, n: K.adamw_ema_multi_(t, n, step=1, one_minus_decay=omd, **hp),
            (p1, g0, m1, v1, ema_of(sh0, p1)), shadow=True)
        for flag, (p, m, v) in ((0, (p1, m1, v1)), (1, (p0, m0, v0))):
            rec = record(flag)
            run(f"mudg_adamw_scaled_multi, flag {flag}, {where}", off_of, lambda t, n: K.adamw_scaled_multi_(t, n, rec, stat, **hp), (p, g0, m, v))
            moved = ema_of(sh0, p)
            assert not any(torch.equal(a, b) for a, b in zip(moved, sh0))
            run(f"mudg_adamw_scaled_ema_multi, flag {flag}, {where}", off_of,
                lambda t, n: K.adamw_scaled_ema_multi_(t, n, rec, stat, one_minus_decay=omd, **hp), (p, g0, m, v, moved), shadow=True)
            assert rec.cpu().tolist() == [0x3F800000, 0, flag, 0]
        views, intact = lay([p0, sh0], off_of)
        table, n = K.chunk_table(list(zip(*views)))
        K.swap_multi_(table, n)
        for a, b, a0, b0 in zip(*views, p0, sh0):
            assert torch.equal(a.cpu(), b0) and torch.equal(b.cpu(), a0), ("mudg_swap_multi", where)
        intact()
    print(f"[backward {hip.operand_name()}] the multi-tensor walk at sizes {sizes}, aligned and off by one float: bit-equal, sentinels intact")


# ================================================================================================ refusals
def test_what_a_kernel_cannot_do_is_refused_before_any_launch(cuda):
    """Every call below fails a MUDG_REQUIRE that returns before the launch; the tensors have the sizes the call names all the same."""
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=cuda)
    with pytest.raises(hip.MudgError, match="above 1280"):
        ln_bwd_raw(z(4, 1344), z(4, 1344), z(1344), 1e-5, None)
    with pytest.raises(hip.MudgError):
        K.temporal_attention_bwd(z(33 * 2, 192), z(33 * 2, 64), 1, 33, 2, 1, 0.125)
    with pytest.raises(hip.MudgError, match="shape"):
        gn_bwd_raw(z(8, 514), z(8, 514), z(514), z(514), z(2, 2), 1, 8, 2, False, None)             # 257 channels per group
    h = lambda r, c: torch.zeros((r, c), dtype=hip.operand_dtype(), device=cuda)
    if SPLIT:
        with pytest.raises(hip.MudgError, match="16-bit operand builds"):
            call_wgrad(h(64, 64), h(64, 64), 64, 64, 64, 1, 0, None, 1, 64)
        with pytest.raises(hip.MudgError, match="16-bit operand builds"):
            K.attention_bwd(h(8, 64), h(8, 64), h(8, 64), h(8, 64), frames=1, heads=1, nq=8, nk=8, kv_div=1, scale=0.125)
    else:
        with pytest.raises(hip.MudgError, match="multiple of 8"):
            call_wgrad(h(64, 16), h(64, 64), 64, 12, 64, 1, 0, None, 1, 64)
        with pytest.raises(hip.MudgError, match="multiple of 8"):
            call_wgrad(h(64, 64), h(64, 96), 64, 64, 96, 1, 0, None, 1, 64)


# ================================================================================================ attention backward
ATTN_SHAPES = [(40, 40, 1, 3), (333, 333, 1, 2), (576, 576, 1, 1), (520, 300, 1, 2), (200, 150, 2, 4), (2304, 77, 4, 4)]     # nq, nk, kv_div, frames


def check_attn(name, got, want, bounds):
    worst = 0.0
    for g, w, b, nm in zip(got, want, bounds, ("dQ", "dK", "dV")):
        worst = max(worst, check(f"{name} {nm}", g, w, b, rb=32, cb=64))
    return worst


@ONLY16
@pytest.mark.parametrize("heads", [1, 5])
@pytest.mark.parametrize("nq,nk,kv_div,frames", ATTN_SHAPES)
def test_attention_backward(cuda, nq, nk, kv_div, frames, heads):
    c, scale = heads * 64, 0.125
    dt16 = hip.operand_dtype()
    mk = lambda rows, seed: rounded(rnd(rows, c, seed=seed))
    q, k, v, do = mk(frames * nq, 1700), mk(frames // kv_div * nk, 1701), mk(frames // kv_div * nk, 1702), mk(frames * nq, 1703)
    kw = dict(frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div, scale=scale)
    want = R.attention_bwd(q, k, v, do, **kw)
    emu = R.attention_bwd(q, k, v, do, round_to=dt16, **kw)              # fp64 throughout, except P and dS through the operand type
    dist = [rel_l2(e, w) for e, w in zip(emu, want)]
    bounds = [3.0 * d for d in dist]
    tag = f"Nq={nq} Nk={nk} kv_div={kv_div} frames={frames} heads={heads}"
    print(f"[backward {hip.operand_name()}] mudg_attention_bwd {tag}: rel-L2 of the P / dS-rounding emulation from fp64 "
          f"dQ {dist[0]:.3e} dK {dist[1]:.3e} dV {dist[2]:.3e}; bound = 3 x")
    dev16 = lambda t, gap=0: gapped(t, t.shape[1] + gap, cuda, dt16)
    q16, k16, v16, do16 = dev16(q), dev16(k, 8), dev16(v, 16), dev16(do, 8)
    # (1) statistics from the kernel's own pass
    stats = K.attention_bwd(q16, k16, v16, do16, **kw)
    check_attn(f"mudg_attention_bwd {tag} stats pass", stats, want, bounds)
    # (2) statistics from the forward pass (o, lse)
    vt, ldv = F._vt(v.to(cuda), frames // kv_div, nk)
    o = ops.empty_rows(frames * nq, c, ops.H16(), cuda)
    lse = torch.empty((frames * nq, heads), dtype=torch.float32, device=cuda)
    ops.attention(q16, k16, vt, o, frames=frames, heads=heads, nq=nq, nk=nk, ldvt=ldv, svt=c * ldv, kv_div=kv_div, scale=scale, lse=lse)
    fwd = K.attention_bwd(q16, k16, v16, do16, o=o, lse=lse, **kw)
    check_attn(f"mudg_attention_bwd {tag} forward statistics", fwd, want, bounds)
    check_attn(f"mudg_attention_bwd {tag} forward statistics vs stats pass", fwd, [t.cpu() for t in stats], bounds)
    if nq == nk and kv_div == 1:
        # (3) the packed projection [q | k | v] read through column views (row stride 3 C), dq / dk / dv written into the column blocks
        # of one packed gradient whose other entries must stay as they were
        qkv16 = gapped(torch.cat([q, k, v], 1), 3 * c + 8, cuda, dt16)
        dqkv = torch.full((frames * nq, 3 * c + 4), NAN, dtype=torch.float32, device=cuda)
        for form, extra in (("stats pass", {}), ("forward statistics", dict(o=o, lse=lse))):
            dqkv.fill_(NAN)
            K.attention_bwd(qkv16[:, :c], qkv16[:, c:2 * c], qkv16[:, 2 * c:], do16, out=(dqkv[:, :c], dqkv[:, c:2 * c], dqkv[:, 2 * c:3 * c]),
                            **extra, **kw)
            assert bool(torch.isnan(dqkv[:, 3 * c:]).all()), "columns beyond the packed gradient were written"
            packed = (dqkv[:, :c], dqkv[:, c:2 * c], dqkv[:, 2 * c:3 * c])
            check_attn(f"mudg_attention_bwd {tag} packed views, {form}", packed, want, bounds)
            for g, s in zip(packed, stats if not extra else fwd):                      # the layout changes nothing
                assert torch.equal(g, s), f"packed views, {form}: not bit-equal to the separate tensors"


@ONLY16
def test_attention_backward_of_two_key_value_sets(cuda):
    """Text + image cross-attention: two key / value sets with their own softmax, O = O1 + O2; dQ is the sum of the two calls'."""
    frames, heads, nq, scale = 4, 5, 200, 0.125
    nk, kv_div, nk2, kv_div2 = 77, 4, 150, 1
    c, dt16 = heads * 64, hip.operand_dtype()
    mk = lambda rows, seed: rounded(rnd(rows, c, seed=seed))
    q, do = mk(frames * nq, 1800), mk(frames * nq, 1801)
    k, v, k2, v2 = mk(nk, 1802), mk(nk, 1803), mk(frames * nk2, 1804), mk(frames * nk2, 1805)
    args = dict(frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div, nk2=nk2, kv_div2=kv_div2, scale=scale)
    want = R.attention_bwd_two_sets(q, k, v, k2, v2, do, **args)
    one = dict(frames=frames, heads=heads, nq=nq, scale=scale)
    e1 = R.attention_bwd(q, k, v, do, nk=nk, kv_div=kv_div, round_to=dt16, **one)
    e2 = R.attention_bwd(q, k2, v2, do, nk=nk2, kv_div=kv_div2, round_to=dt16, **one)
    emu = (e1[0] + e2[0], e1[1], e1[2], e2[1], e2[2])
    d16 = lambda t: t.to(dt16).to(cuda)
    g1 = K.attention_bwd(d16(q), d16(k), d16(v), d16(do), nk=nk, kv_div=kv_div, **one)
    g2 = K.attention_bwd(d16(q), d16(k2), d16(v2), d16(do), nk=nk2, kv_div=kv_div2, **one)
    got = (g1[0] + g2[0], g1[1], g1[2], g2[1], g2[2])
    for g, w, e, nm in zip(got, want, emu, ("dQ", "dK", "dV", "dK2", "dV2")):
        dist = rel_l2(e, w)
        print(f"[backward {hip.operand_name()}] two sets {nm}: emulation rel-L2 {dist:.3e}")
        check(f"mudg_attention_bwd two sets {nm}", g, w, 3.0 * dist, rb=32, cb=64)
