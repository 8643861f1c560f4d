"""Every autograd Function of the training step (mudg_amd/train/functions.py, the resampler's Gelu) on its own, against torch autograd
of the textbook op on the CPU in fp64 — the layer between the backward kernels (tests/test_backward_kernels_gpu.py) and the whole UNet
(tests/test_training_gpu.py), where the indexing decisions are made in Python: filter rotation, channel padding, dilation, the choice
of weight-gradient route, the slicing rules, the needs_input_grad branches, the operand caches, the two-output *Skip Functions.

  A  exact    Linear, Conv3x3, TConv3 on integers -3 .. 3 (tests/train_functions_cases.py; the magnitude condition is checked on the CPU
              in tests/test_train_functions_cpu.py): the forward value and every gradient torch.equal to fp64, for every non-empty
              needs-grad subset of (x, w, b), then the residual alone and the group bias alone; what was not asked for is None, what was
              asked for never is.  backward() is called on the node itself, so what it RETURNS is seen, not what autograd keeps of it;
              the all-required run also goes through torch.autograd.grad.  Add, ToRows, FromRows, Upsample2x on integers.
  B  bounded  Gaussian operands; whole tensor, every 64-row block, every 64-column block (32 rows for attention).  No constant of this
              file's own: fp32-input backward passes take check_f32's rule (max(TOL_F32, 4 x the error of the same formula in fp32 on
              the CPU)); forward values that pass through operand storage one operand rounding of the mode (EPS of test_towers_gpu.py);
              Linear / Conv3x3 / TConv3 3 x the distance from fp64 of the fp64 evaluation on operand-rounded x, w, dy (bound_of);
              attention 3 x the distance of the P / dS-rounding evaluation (backward_reference.attention_bwd(round_to=...)).
  C  glue     a gradient does not depend on which others were asked for (bit for bit); op() and the attached operand (identity, bit
              equality, refusal after an in-place change, survival of eviction); transposed() and its cache; *Skip with a zero dy, and
              with only the second output used; every case run twice gives the same bits.
Every figure is printed next to its bound (lines with "rel-L2"); the default build's are kept in profiles/train_functions_tests/."""
import gc

import pytest
import torch
import torch.nn.functional as TF

import backward_reference as R
import train_functions_cases as C
from attention_reference import through
from mudg_amd import hip, ops
from mudg_amd.train import functions as Fn
from mudg_amd.train import kernels as K
from mudg_amd.train.resampler import Gelu
from test_backward_kernels_gpu import (ONLY16, SPLIT, base_of, check, check_f32, conv_geo, expected_path, ints, pieces_of, rel_l2, rnd,
                                       rounded)
from test_towers_gpu import EPS, bound_of

pytestmark = pytest.mark.gpu
MODE = hip.operand_name()
RT = (hip.operand_dtype(), hip.planes())
EPS_GN = 1e-5           # the epsilon of the norms (an argument of the op, not a tolerance)


# ------------------------------------------------------------------------------------------------ running a Function
def launch(cls, call, tensors, needs, dys, dev):
    """Forward of `call` on GPU copies of `tensors` (those named in `needs` require gradients), then cls.backward on the node itself:
    (outputs, what backward returned per input position, the GPU leaves)."""
    g = {k: v.to(dev).requires_grad_(k in needs) for k, v in tensors.items()}
    out = call(g)
    outs = out if isinstance(out, tuple) else (out,)
    with torch.no_grad():
        raw = cls.backward(outs[0].grad_fn, *[None if d is None else d.to(dev) for d in dys])
    return outs, (raw if isinstance(raw, tuple) else (raw,)), g


def same_bits(what, a, b):
    for i, (p, q) in enumerate(zip(a, b)):
        assert (p is None) == (q is None), (what, i)
        if p is not None:
            assert torch.equal(p, q), (what, i, "two runs of the same case differ")


def assert_equal(what, got, want):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong, first at {bad.nonzero()[0].tolist()}: got "
                                 f"{float(got[bad][0])}, want {float(want[bad][0])}")


def spy(monkeypatch):
    """Records which weight-gradient route and which column-sum chunking a backward pass takes."""
    seen = dict(wgrad=[], wgrad_gemm=[], colsum=[])
    lib = hip.lib()
    real_wgrad, real_gemm, real_colsum = lib.mudg_wgrad, Fn.wgrad_gemm, K._colsum_once

    def wgrad(desc, stream):
        d = desc._obj
        seen["wgrad"].append((d.P, d.slices, d.chunk))
        return real_wgrad(desc, stream)

    def wgrad_gemm(at, bt, m, n, p):
        seen["wgrad_gemm"].append((m, n, p, Fn._splits(m, n, p)))
        return real_gemm(at, bt, m, n, p)

    def colsum(a, b, rpg):
        seen["colsum"].append((a.shape[0], rpg))
        return real_colsum(a, b, rpg)
    monkeypatch.setattr(lib, "mudg_wgrad", wgrad)
    monkeypatch.setattr(Fn, "wgrad_gemm", wgrad_gemm)
    monkeypatch.setattr(K, "_colsum_once", colsum)
    return seen


def family(fam):
    cases, problem, ref_of, apply, cls_name, positions, tied = C.FAMILIES[fam]
    return cases, problem, ref_of, (lambda case: (lambda g: apply(Fn, case, g))), getattr(Fn, cls_name), positions, tied


def widths(fam, case):
    """(Cout, Cin, positions of the weight-gradient contraction)."""
    if fam == "linear":
        return case[2], case[1], case[0]
    if fam == "conv3x3":
        ho, wo = C.conv_out(case[1], case[2], case[3])
        return case[5], case[4], case[0] * ho * wo
    return case[4], case[3], case[0] * case[1] * case[2]


def wanted(name, tensors, tied, needs):
    return name is not None and name in tensors and tied.get(name, name) in needs


# ================================================================================================ A. exact
@pytest.mark.parametrize("fam,i", C.EXACT_IDS)
def test_linear_conv_tconv_are_exact_on_integers_for_every_needs_grad_subset(cuda, fam, i, monkeypatch):
    cases, problem, ref_of, call_of, cls, positions, tied = family(fam)
    case = cases[i]
    tensors, dy = problem(case, C.int_make)
    y_ref, g_ref = C.reference(ref_of(case), tensors, dy)
    assert all(C.is_integer_valued(t, 2 ** 24) for t in (y_ref, *g_ref.values()))          # tests/test_train_functions_cpu.py
    seen = spy(monkeypatch)
    co, ci, p = widths(fam, case)
    direct = Fn.rows_wgrad_ok(co, ci)
    assert direct == (not SPLIT and ci % 64 == 0 and co % 8 == 0)
    subsets = C.needs_subsets(tensors, tied)
    first = None
    for n, needs in enumerate(subsets):
        for k in seen:
            seen[k].clear()
        (y,), raw, g = launch(cls, call_of(case), tensors, needs, [dy], cuda)
        tag = f"{fam} {case} needs {sorted(needs)}"
        assert_equal(f"{tag} forward", y, y_ref)
        assert len(raw) == len(positions)
        for pos, name in enumerate(positions):
            if not wanted(name, tensors, tied, needs):
                assert raw[pos] is None, (tag, f"a gradient nobody asked for was returned at position {pos} ({name})")
            else:
                assert raw[pos] is not None, (tag, f"the gradient of {name} is missing")
                assert_equal(f"{tag} d{name}", raw[pos], g_ref[name])
        # the route the table names
        if "w" in needs:
            assert bool(seen["wgrad"]) == direct and bool(seen["wgrad_gemm"]) == (not direct), (tag, seen)
            if direct:
                assert seen["wgrad"][0][0] == p, (tag, seen["wgrad"])
        else:
            assert not seen["wgrad"] and not seen["wgrad_gemm"], (tag, "a weight gradient was computed for a frozen weight")
        if n == 0:
            first = (y.detach(), *raw)
            again = launch(cls, call_of(case), tensors, needs, [dy], cuda)
            same_bits(tag, first, (again[0][0].detach(), *again[1]))
            # and through the autograd engine: what arrives at the leaves (a tied residual adds to its source)
            leaves = [k for k in tensors if k not in tied]
            got = torch.autograd.grad(y, [g[k] for k in leaves], dy.to(cuda))
            for k, gr in zip(leaves, got):
                assert_equal(f"{tag} autograd d{k}", gr, g_ref[k] + sum(g_ref[t] for t, src in tied.items() if src == k and t in tensors))
            if (fam, i) == ("linear", 5) and direct:
                assert seen["wgrad"][0] == (4100, 4, 1088), seen["wgrad"]                  # kernels.wgrad's cost model, by hand
            if (fam, i) == ("linear", 6):
                assert seen["wgrad_gemm"] and seen["wgrad_gemm"][0][3] > 1, seen
            if (fam, i) == ("conv3x3", 6):
                assert (6144, 1024) in seen["colsum"] and (6, 6) in seen["colsum"], seen["colsum"]         # the chunk ladder
            if (fam, i) == ("conv3x3", 5) and direct:
                assert expected_path(1, conv_geo(case[1], case[2], case[3])) == 1 and seen["wgrad"][0][0] == 4 * 24 * 32
    print(f"[functions {MODE}] {fam} {case}: {len(subsets)} needs-grad subsets, forward and every gradient exact "
          f"({'mudg_wgrad' if direct else 'transposed copies'})")


def test_add_and_the_layout_functions_are_exact_on_integers(cuda):
    b, c, t, h, w = shape = (2, 5, 3, 4, 7)
    a5, g5 = ints(*shape, seed=11), ints(*shape, seed=12)
    rows = b * t * h * w
    ar, gr = ints(rows, c, seed=13), ints(rows, c, seed=14)
    to_rows = lambda v: v.permute(0, 2, 3, 4, 1).reshape(rows, c)
    from_rows = lambda v: v.reshape(b, t, h, w, c).permute(0, 4, 1, 2, 3)
    (y,), raw, _ = launch(Fn.ToRows, lambda g: Fn.ToRows.apply(g["x"]), dict(x=a5), {"x"}, [gr], cuda)
    assert_equal("ToRows", y, to_rows(a5).double())
    assert_equal("ToRows dx", raw[0], from_rows(gr).double())
    assert y.is_contiguous() and raw[0].is_contiguous()
    (y,), raw, _ = launch(Fn.FromRows, lambda g: Fn.FromRows.apply(g["y"], shape), dict(y=ar), {"y"}, [g5], cuda)
    assert_equal("FromRows", y, from_rows(ar).double())
    assert_equal("FromRows dy", raw[0], to_rows(g5).double())
    assert raw[1] is None and y.is_contiguous() and raw[0].is_contiguous()
    (y,), raw, g = launch(Fn.Add, lambda g: Fn.Add.apply(g["a"], g["b"]), dict(a=ar, b=gr), {"a", "b"}, [ar], cuda)
    assert_equal("Add", y, (ar + gr).double())
    assert_equal("Add da", raw[0], ar.double())
    assert_equal("Add db", raw[1], ar.double())
    assert torch.equal(g["a"].detach().cpu(), ar) and torch.equal(g["b"].detach().cpu(), gr), "Add changed an input"
    # nearest 2x: the adjoint sums four integers
    f, hh, ww, cc = 2, 3, 5, 16
    x, dy = ints(f * hh * ww, cc, seed=15), ints(f * 4 * hh * ww, cc, seed=16)
    xr = x.double().requires_grad_(True)
    yr = TF.interpolate(xr.reshape(f, hh, ww, cc).permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1).reshape(-1, cc)
    (dxr,) = torch.autograd.grad(yr, xr, dy.double())
    for rep in range(2):
        (y,), raw, _ = launch(Fn.Upsample2x, lambda g: Fn.Upsample2x.apply(g["x"], (f, hh, ww)), dict(x=x), {"x"}, [dy], cuda)
        assert_equal("Upsample2x", y, yr.detach())
        assert_equal("Upsample2x dx", raw[0], dxr)
        assert raw[1] is None
    print(f"[functions {MODE}] Add, ToRows, FromRows {shape}, Upsample2x ({f}, {hh}, {ww}) x {cc}: exact")


# ================================================================================================ B. bounded: fp32-input backward passes
def norm_operands(rows, c, seed):
    return dict(x=rnd(rows, c, seed=seed) * 2 + 0.5, g=1 + 0.2 * rnd(c, seed=seed + 1), b=0.2 * rnd(c, seed=seed + 2)), rnd(rows, c, seed=seed + 3)


def run_twice(cls, call, tensors, dys, dev):
    outs, raw, g = launch(cls, call, tensors, set(tensors), dys, dev)
    outs2, raw2, _ = launch(cls, call, tensors, set(tensors), dys, dev)
    same_bits(cls.__name__, [o.detach() for o in outs] + list(raw), [o.detach() for o in outs2] + list(raw2))
    return outs, raw, g


@pytest.mark.parametrize("kind", ["GroupNorm", "GroupNormSkip + dskip", "GroupNormSkip"])
@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("samples,rows,c", C.GN_CASES)
def test_groupnorm_functions(cuda, samples, rows, c, silu, kind):
    cls = Fn.GroupNorm if kind == "GroupNorm" else Fn.GroupNormSkip
    t, dy = norm_operands(samples * rows, c, 2000 + c)
    dskip = rnd(samples * rows, c, seed=2010 + c) if "dskip" in kind else None
    dys = [dy] if cls is Fn.GroupNorm else [dy, dskip]
    outs, raw, _ = run_twice(cls, lambda g: cls.apply(g["x"], g["g"], g["b"], samples, rows, EPS_GN, silu, 32), t, dys, cuda)
    tag = f"{kind} samples={samples} rows={rows} C={c} silu={int(silu)}"
    want = C.groupnorm_ref(samples, rows, c, silu, 32, EPS_GN)(*(t[k].double() for k in "xgb"))
    check(f"{tag} forward", outs[0], want, EPS)
    if cls is Fn.GroupNormSkip:
        assert torch.equal(outs[1].detach().cpu(), t["x"]), "the skip output is not x"
    assert all(r is None for r in raw[3:]) and len(raw) == 8

    def ref(dt):
        st = R.groupnorm_stats(t["x"], samples, rows, 32, EPS_GN, dtype=dt)
        dx, ab = R.groupnorm_bwd(t["x"], dy, t["g"], t["b"], st, samples, rows, 32, silu, dskip, dtype=dt)
        return dx, ab[..., 1].sum(0), ab[..., 0].sum(0)
    check_f32(f"{tag} backward (dx, dgamma, dbeta)", raw[:3], ref)


@pytest.mark.parametrize("kind", ["LayerNorm", "LayerNormSkip + dskip", "LayerNormSkip"])
@pytest.mark.parametrize("rows,c", C.LN_CASES)
def test_layernorm_functions(cuda, rows, c, kind):
    cls = Fn.LayerNorm if kind == "LayerNorm" else Fn.LayerNormSkip
    t, dy = norm_operands(rows, c, 2100 + c)
    dskip = rnd(rows, c, seed=2110 + c) if "dskip" in kind else None
    dys = [dy] if cls is Fn.LayerNorm else [dy, dskip]
    outs, raw, _ = run_twice(cls, lambda g: cls.apply(g["x"], g["g"], g["b"], EPS_GN), t, dys, cuda)
    tag = f"{kind} rows={rows} C={c}"
    check(f"{tag} forward", outs[0], TF.layer_norm(t["x"].double(), (c,), t["g"].double(), t["b"].double(), EPS_GN), EPS)
    if cls is Fn.LayerNormSkip:
        assert torch.equal(outs[1].detach().cpu(), t["x"]), "the skip output is not x"
    assert raw[3] is None and len(raw) == 4

    def ref(dt):
        dx, part = R.layernorm_bwd(t["x"], dy, t["g"], EPS_GN, dskip, dtype=dt)
        return dx, part[:, 0].sum(0), part[:, 1].sum(0)
    check_f32(f"{tag} backward (dx, dgamma, dbeta)", raw[:3], ref)


@pytest.mark.parametrize("cls", [Fn.GroupNormSkip, Fn.LayerNormSkip])
def test_skip_functions_hand_dskip_through_exactly(cuda, cls):
    """A zero dy leaves dx = dskip bit for bit and dgamma = dbeta = 0; with only the second output used the gradient of x is dskip."""
    samples, rows, c = 3, 50, 64
    t, _ = norm_operands(samples * rows, c, 2200)
    dskip = ints(samples * rows, c, seed=2201)
    call = (lambda g: cls.apply(g["x"], g["g"], g["b"], samples, rows, EPS_GN, True, 32)) if cls is Fn.GroupNormSkip else \
           (lambda g: cls.apply(g["x"], g["g"], g["b"], EPS_GN))
    outs, raw, g = launch(cls, call, t, set(t), [torch.zeros_like(dskip), dskip], cuda)
    assert_equal(f"{cls.__name__} dx under a zero dy", raw[0], dskip.double())
    assert not bool(raw[1].any()) and not bool(raw[2].any()), "dgamma / dbeta of a zero dy are not zero"
    outs, raw, g = launch(cls, call, t, set(t), [None, dskip], cuda)
    assert_equal(f"{cls.__name__} dx, second output only (backward itself)", raw[0], dskip.double())
    assert all(r is None for r in raw[1:])
    (dx,) = torch.autograd.grad(outs[1], g["x"], dskip.to(cuda))
    assert_equal(f"{cls.__name__} dx, second output only (autograd)", dx, dskip.double())
    print(f"[functions {MODE}] {cls.__name__}: dskip arrives bit for bit")


def elementwise(cuda, name, cls, x, dy, fn):
    """An elementwise Function with fp32 inputs against `fn` (torch, any dtype): forward and backward by check_f32's rule."""
    outs, raw, _ = run_twice(cls, lambda g: cls.apply(g["x"]), dict(x=x), [dy], cuda)

    def ref(dt):
        xr = x.to(dt).requires_grad_(True)
        y = fn(xr)
        return y.detach(), torch.autograd.grad(y, xr, dy.to(dt))[0]
    check_f32(f"{name} (forward, backward)", (outs[0], raw[0]), ref)


@pytest.mark.parametrize("m,n", C.GEGLU_CASES)
def test_geglu_function(cuda, m, n):
    elementwise(cuda, f"Geglu M={m} N={n}", Fn.Geglu, rnd(m, 2 * n, seed=2300 + n, scale=1.5), rnd(m, n, seed=2301 + n),
                lambda h: h[:, :n] * TF.gelu(h[:, n:]))


def test_silu_and_gelu_functions(cuda):
    elementwise(cuda, "Silu 40 x 8", Fn.Silu, rnd(40, 8, seed=2400, scale=2.0), rnd(40, 8, seed=2401), TF.silu)
    elementwise(cuda, "Gelu 60 x 256", Gelu, rnd(60, 256, seed=2402, scale=2.0), rnd(60, 256, seed=2403), TF.gelu)


def test_temporal_attention_function(cuda):
    clips, t, hw, heads = 2, 6, 10, 2
    c = heads * 64
    qkv, do = rounded(rnd(clips * t * hw, 3 * c, seed=2500)), rnd(clips * t * hw, c, seed=2501)
    geo = (clips, t, hw, heads, C.SCALE)
    outs, raw, _ = run_twice(Fn.TemporalAttention, lambda g: Fn.TemporalAttention.apply(g["qkv"], geo), dict(qkv=qkv), [do], cuda)
    check("TemporalAttention forward", outs[0], C.temporal_attention_ref(qkv.double(), clips, t, hw, heads, C.SCALE), EPS, rb=32)
    assert raw[1] is None
    check_f32("TemporalAttention backward", raw[0],
              lambda dt: R.temporal_attention_bwd(qkv, do, clips=clips, t=t, hw=hw, heads=heads, scale=C.SCALE, dtype=dt), rb=32)


def test_weighted_mse_function(cuda):
    shape = (3, 4, 2, 5, 5)
    pred, target, w = rnd(*shape, seed=2600), rnd(*shape, seed=2601), torch.tensor([0.5, 0.2, 0.3])
    up = torch.tensor(2.0)
    outs, raw, _ = launch(Fn.WeightedMSE, lambda g: Fn.WeightedMSE.apply(g["pred"], target.to(cuda), w.to(cuda)), dict(pred=pred), {"pred"},
                          [up, None], cuda)
    outs2, raw2, _ = launch(Fn.WeightedMSE, lambda g: Fn.WeightedMSE.apply(g["pred"], target.to(cuda), w.to(cuda)), dict(pred=pred), {"pred"},
                            [up, None], cuda)
    same_bits("WeightedMSE", [o.detach() for o in outs] + [raw[0]], [o.detach() for o in outs2] + [raw2[0]])
    assert raw[1] is None and raw[2] is None

    def ref(dt):
        loss_b, grad = R.mse(pred, target, w, dtype=dt)
        return (w.to(dt) * loss_b).sum().reshape(1, 1), loss_b.reshape(1, -1), (grad * up.to(dt)).reshape(shape[0], -1)
    check_f32("WeightedMSE (loss, per sample, gradient)", (outs[0].reshape(1, 1), outs[1].reshape(1, -1), raw[0].reshape(shape[0], -1)), ref, rb=1)


# ================================================================================================ B / C.1: Gaussian Linear, Conv3x3, TConv3
@pytest.mark.parametrize("fam", list(C.GAUSS))
def test_gaussian_linear_conv_tconv_within_the_operand_rounding_and_independent_of_what_was_asked_for(cuda, fam):
    _, problem, ref_of, call_of, cls, positions, tied = family(fam)
    case = C.GAUSS[fam]
    tensors, dy = problem(case, C.gauss_make, seed=3000)
    ref = ref_of(case)
    want, emu, plain = C.reference(ref, tensors, dy), C.reference(ref, tensors, dy, rt=through(RT)), C.reference(ref, tensors, dy, torch.float32)
    subsets = C.needs_subsets(tensors, tied)
    (y,), full, _ = launch(cls, call_of(case), tensors, subsets[0], [dy], cuda)
    tag = f"{fam} {case}"
    check(f"{tag} forward", y, want[0], bound_of(f"{tag} forward", emu[0], plain[0], want[0]))
    for pos, name in enumerate(positions):
        if name in tensors:
            check(f"{tag} d{name}", full[pos], want[1][name], bound_of(f"{tag} d{name}", emu[1][name], plain[1][name], want[1][name]))
    # C.1: every form of dy is one round-to-nearest of the same fp32 values and every kernel sums in a fixed order, so a gradient
    # is the same bits whichever others were asked for; C.6: and the same bits when the case is run again
    for needs in subsets:
        (y2,), raw, _ = launch(cls, call_of(case), tensors, needs, [dy], cuda)
        assert torch.equal(y2, y), (tag, sorted(needs), "forward")
        for pos, name in enumerate(positions):
            if wanted(name, tensors, tied, needs):
                assert raw[pos] is not None, (tag, sorted(needs), name)
                diff = int((raw[pos] != full[pos]).sum())
                assert diff == 0, (f"{tag}: d{name} asked for with {sorted(needs)} differs from the all-required run in {diff} of "
                                   f"{raw[pos].numel()} elements (rel-L2 {rel_l2(raw[pos], full[pos]):.3e})")
            else:
                assert raw[pos] is None, (tag, sorted(needs), pos)
    print(f"[functions {MODE}] {tag}: every gradient bit-equal over {len(subsets)} needs-grad subsets and two runs")


# ================================================================================================ B: attention
def attn_operands(case, seed):
    frames, heads, nq, nk, kv_div, nk2, kv_div2 = case
    c = heads * 64
    mk = lambda rows, s: rounded(rnd(rows, c, seed=seed + s))            # operand-rounded: both sides read the same numbers
    t = dict(q=mk(frames * nq, 0), k=mk(frames // kv_div * nk, 1), v=mk(frames // kv_div * nk, 2))
    if nk2:
        t.update(k2=mk(frames // kv_div2 * nk2, 3), v2=mk(frames // kv_div2 * nk2, 4))
    return t, mk(frames * nq, 5)


def attn_gradients(t, do, case, round_to=None):
    frames, heads, nq, nk, kv_div, nk2, kv_div2 = case
    one = dict(frames=frames, heads=heads, nq=nq, scale=C.SCALE, round_to=round_to)
    g1 = R.attention_bwd(t["q"], t["k"], t["v"], do, nk=nk, kv_div=kv_div, **one)
    if not nk2:
        return g1
    g2 = R.attention_bwd(t["q"], t["k2"], t["v2"], do, nk=nk2, kv_div=kv_div2, **one)
    return g1[0] + g2[0], g1[1], g1[2], g2[1], g2[2]


@pytest.mark.parametrize("i", range(len(C.ATTN_CASES)))
def test_attention_function(cuda, i):
    case = frames, heads, nq, nk, kv_div, nk2, kv_div2 = C.ATTN_CASES[i]
    t, do = attn_operands(case, 4000 + 10 * i)
    geo = (frames, heads, nq, nk, kv_div, nk2, kv_div2, C.SCALE)
    outs, raw, _ = run_twice(Fn.Attention, lambda g: Fn.Attention.apply(g["q"], g["k"], g["v"], g.get("k2"), g.get("v2"), geo), t, [do], cuda)
    tag = f"Attention frames={frames} heads={heads} Nq={nq} Nk={nk} kv_div={kv_div} Nk2={nk2}"
    d = {k: v.double() for k, v in t.items()}
    want_o = C.attention_ref(d["q"], d["k"], d["v"], frames, heads, nq, nk, kv_div, C.SCALE)
    if nk2:
        want_o = want_o + C.attention_ref(d["q"], d["k2"], d["v2"], frames, heads, nq, nk2, kv_div2, C.SCALE)
    check(f"{tag} forward", outs[0], want_o, EPS, rb=32)
    want = attn_gradients(t, do, case)
    if nk2:
        two = R.attention_bwd_two_sets(t["q"], t["k"], t["v"], t["k2"], t["v2"], do, frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div,
                                       nk2=nk2, kv_div2=kv_div2, scale=C.SCALE)
        assert all(torch.equal(a, b) for a, b in zip(want, two))
    emu = attn_gradients(t, do, case, round_to=RT if SPLIT else RT[0])
    assert raw[5] is None and len(raw) == 6 and all((r is None) == (nk2 == 0) for r in raw[3:5])
    for g, w, e, nm in zip(raw, want, emu, ("dq", "dk", "dv", "dk2", "dv2")):
        check(f"{tag} {nm}", g, w, 3.0 * rel_l2(e, w), rb=32)


@ONLY16
def test_packed_self_attention_function(cuda):
    frames, heads, n = 2, 2, 40
    c = heads * 64
    qkv, do = rounded(rnd(frames * n, 3 * c, seed=4100)), rounded(rnd(frames * n, c, seed=4101))
    geo = (frames, heads, n, C.SCALE)
    outs, raw, _ = run_twice(Fn.SelfAttention, lambda g: Fn.SelfAttention.apply(g["qkv"], geo), dict(qkv=qkv), [do], cuda)
    q, k, v = qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:]
    check("SelfAttention forward", outs[0], C.attention_ref(q.double(), k.double(), v.double(), frames, heads, n, n, 1, C.SCALE), EPS, rb=32)
    kw = dict(frames=frames, heads=heads, nq=n, nk=n, kv_div=1, scale=C.SCALE)
    want, emu = R.attention_bwd(q, k, v, do, **kw), R.attention_bwd(q, k, v, do, round_to=RT[0], **kw)
    assert raw[1] is None and raw[0].shape == (frames * n, 3 * c)
    for j, nm in enumerate(("dq", "dk", "dv")):
        check(f"SelfAttention {nm}", raw[0][:, j * c:(j + 1) * c], want[j], 3.0 * rel_l2(emu[j], want[j]), rb=32)


# ================================================================================================ C.2: op() and the attached operand
def same_pieces(what, a, b):
    for pl, (p, q) in enumerate(zip(pieces_of(a), pieces_of(b))):
        assert torch.equal(p, q), (what, "piece", pl, int((p != q).sum()))


def producers(dev):
    """name -> (a call that makes a fresh tagged output, whether the fp32 tensor is the primary result)."""
    c = 128
    x = rnd(120, c, seed=5000).to(dev)
    gam, bet = (1 + 0.2 * rnd(c, seed=5001)).to(dev), (0.2 * rnd(c, seed=5002)).to(dev)
    h = rnd(120, 2 * c, seed=5003).to(dev)
    q, k, v = (rounded(rnd(2 * 40, c, seed=5004 + j)).to(dev) for j in range(3))
    qkv = rnd(2 * 40, 3 * c, seed=5008).to(dev)
    out = {
        "GroupNorm": (lambda: Fn.GroupNorm.apply(x, gam, bet, 3, 40, EPS_GN, True, 32), False),
        "GroupNormSkip": (lambda: Fn.GroupNormSkip.apply(x, gam, bet, 3, 40, EPS_GN, False, 32)[0], False),
        "LayerNorm": (lambda: Fn.LayerNorm.apply(x, gam, bet, EPS_GN), False),
        "LayerNormSkip": (lambda: Fn.LayerNormSkip.apply(x, gam, bet, EPS_GN)[0], False),
        "GegluDropout p=0": (lambda: Fn.GegluDropout.apply(h, 0.0, 0), True),
        "GegluDropout p=0.25": (lambda: Fn.GegluDropout.apply(h, 0.25, 1234), True),
        "Dropout rows": (lambda: Fn.Dropout.apply(x, 0.25, 77), True),
        "Attention": (lambda: Fn.Attention.apply(q, k, v, None, None, (2, 2, 40, 40, 1, 0, 1, C.SCALE)), False),
        "TemporalAttention": (lambda: Fn.TemporalAttention.apply(qkv, (2, 4, 10, 2, C.SCALE)), False),
    }
    if not SPLIT:
        out["SelfAttention"] = (lambda: Fn.SelfAttention.apply(qkv, (2, 2, 40, C.SCALE)), False)
    return out


def test_op_takes_the_attached_operand_while_it_is_valid_and_a_fresh_cast_otherwise(cuda):
    made = producers(cuda)
    filler = made["LayerNorm"][0]
    for name, (make, fp32_primary) in made.items():
        y = make()
        tag = getattr(y, "_mudg_operand", None)
        assert tag is not None, (name, "no operand attached")
        attached = tag[1]()
        assert attached is not None and Fn.op(y) is attached, (name, "op() does not return the attached operand")
        fresh = ops.cast_bf16(y.clone())
        if fp32_primary:
            same_pieces(f"{name}: attached operand against a cast of the fp32 result", attached, fresh)
        else:
            assert torch.equal(ops.to_f32(attached), y), (name, "the fp32 result is not the attached operand widened")
            if not SPLIT:       # (a kernel's own split of a value into pieces need not be the one the cast of the pieces' sum makes)
                same_pieces(f"{name}: attached operand against a cast of its own fp32 copy", attached, fresh)
        if not SPLIT:
            # a consumer sees the same numbers through the attached operand and through a cast of a copy
            w = rnd(72, y.shape[1], seed=5100, scale=0.1)
            dz = rnd(y.shape[0], 72, seed=5101)
            res = []
            for src in (y, y.clone()):
                (z,), raw, _ = launch(Fn.Linear, lambda g: Fn.Linear.apply(src, g["w"], None, None), dict(w=w), {"w"}, [dz], cuda)
                res.append((z.detach(), raw[1]))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (name, "Linear differs on the tagged tensor")
        # an in-place change makes the attached operand stale
        y.mul_(1.0)
        got = Fn.op(y)
        assert got is not attached, (name, "op() returned a stale operand after an in-place change")
        same_pieces(f"{name}: op() after an in-place change", got, ops.cast_bf16(y.clone()))
        # eviction: the last few operands stay alive, older ones are freed, and op() casts afresh
        y = make()
        weak = y._mudg_operand[1]
        del attached, got, tag, fresh
        keep = [filler() for _ in range(5)]
        gc.collect()
        assert weak() is None, (name, "the attached operand outlived five further producers")
        same_pieces(f"{name}: op() after eviction", Fn.op(y), ops.cast_bf16(y.clone()))
        del keep
    print(f"[functions {MODE}] op(): {len(made)} producers, attached operand taken, refused when stale, recast when evicted")


# ================================================================================================ C.3: transposed()
@pytest.mark.parametrize("p,c", [(203, 72), (203, 6)])
def test_transposed_contents_and_cache(cuda, p, c):
    """72 columns: mudg_transpose_cast_sum; 6 columns (rows not 16-byte aligned): mudg_transpose_gather."""
    src32 = rnd(p, c, seed=6000 + c)
    src = src32.to(cuda)
    m, n = 72, 64
    t1 = Fn.transposed(src, m, n)
    assert Fn.transposed(src, m, n) is t1, "a second call made a new copy"
    width = Fn._width(m, n, p)
    want = R.operand_planes(R.transpose_gather(src32, p).float(), *RT)
    for pl, (g, w) in enumerate(zip(pieces_of(t1), want)):
        assert g.shape == (c, width) and torch.equal(g[:, :R.ceil8(p)], w), ("piece", pl)
        assert not bool(g[:, R.ceil8(p):].any()), "columns beyond the rows are not zero"
    src.add_(0)
    t2 = Fn.transposed(src, m, n)
    assert t2 is not t1, "the copy of a changed tensor was reused"
    same_pieces("transposed after add_(0)", t2, t1)


def test_transposed_does_not_reuse_a_copy_of_another_width(cuda):
    p, c = 4100, 8
    src32 = rnd(p, c, seed=6100)
    src = src32.to(cuda)
    (m1, n1), (m2, n2) = (72, 96), (2048, 2048)
    w1, w2 = Fn._width(m1, n1, p), Fn._width(m2, n2, p)
    assert w1 != w2 and Fn._splits(m1, n1, p) > 1 and Fn._splits(m2, n2, p) > 1
    t1 = Fn.transposed(src, m1, n1)
    t2 = Fn.transposed(src, m2, n2)
    assert t2 is not t1 and t1.shape == (c, w1) and t2.shape == (c, w2)
    want = R.operand_planes(R.transpose_gather(src32, p).float(), *RT)
    for t, width in ((t1, w1), (t2, w2)):
        for g, w in zip(pieces_of(t), want):
            assert torch.equal(g[:, :R.ceil8(p)], w) and not bool(g[:, R.ceil8(p):].any())
    assert Fn.transposed(src, m2, n2) is t2
