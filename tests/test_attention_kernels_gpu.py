"""Every forward attention kernel of csrc/attention.hip, reached through mudg_attention / mudg_temporal_attention by the shipped
dispatch rule, and held to tests/attention_reference.py — in every operand mode: the file runs in bf16 directly and in fp16, bf16x3
and bf16x6 in the mode children (tests/test_precision_modes_gpu.py), and under the dispatcher's A/B switches in the variant children
(tests/test_gemm_variants_gpu.py).  Operands are made by the library's own cast and read back, so references see what the kernels read.

  gather     Q row i is the +-4 code of key pi(i): softmax puts 1 - 2^-40 or more on that key (asserted on the CPU), so O = V[pi(i)]
             bit for bit.  A wrong key order against V^T, a mis-masked last key, a wrong row / frame / head mapping each move whole rows.
             With prescaled Q the first-tile form stays inside the lean softmax's range and the full-range form forces its fallback.
  uniform    K = 0: every key weighs 1 / Nk, V is constant over keys, O = that constant, Lse = log2 Nk.
  random     Gaussian operands against the fp64 definition: whole tensor within 2 x TOL_OP of the mode (test_operand_modes_gpu.py),
             every 32-row block (one wave's queries) and every 64-column block (one head) within 3 x the rel-L2 distance from fp64 of
             the emulation that rounds P and O to the operand storage.  bf16x6 alone takes max(that, 4 x the distance of the same
             formula in fp32 on the CPU): its pieces carry fp32's own 24 bits, so the emulation sits at 3.6e-8 from fp64 while any
             fp32-accumulating softmax sits at 3e-7 .. 5e-7 (CPU) — the kernel measures 1.5e-7 .. 7.5e-7.  Both distances are printed.
  exact      torch.equal in the 16-bit builds.  In the split builds each element within one operand rounding of the mode (the eps table of
             test_cast_round_trip_is_exact_to_the_modes_precision); in bf16x6 alone uniform outputs get 2^-23, the two fp32 roundings
             of (sum V) * (1 / Nk), which 16 or 17 stored bits hide and 24 do not.
  Lse        fp32, against fp64 lse2: max(2e-5, 4 x the error of the same formula in fp32 on the CPU), as tests/test_backward_kernels_gpu.py."""
import math
import os

import pytest
import torch

import attention_reference as A
from mudg_amd import hip, ops
from test_backward_kernels_gpu import NAN, base_of, check, filled_operand, gapped, rel_l2
from test_operand_modes_gpu import MODE, TOL_OP, _vt, operand, value

pytestmark = pytest.mark.gpu

SPLIT = hip.planes() > 1
RT = (hip.operand_dtype(), hip.planes())                       # the operand storage P and O pass through
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "bf16x3": 2.0 ** -17, "bf16x6": 2.0 ** -24}[MODE]
TOL_LSE = 2e-5
SCALE = 0.125
CL2 = SCALE * A.LOG2E
_env = os.environ.get
VARIANT = _env("MUDG_DEBUG_VARIANTS") == "1"
# the fp8 score path lives in attn64d_kernel<true, true>: 16-bit builds, and not where a variant child turns that kernel off
FP8 = not SPLIT and not (VARIANT and (_env("MUDG_ATTN_Q") == "32" or _env("MUDG_ATTN_DMA") == "0"))


# ------------------------------------------------------------------------------------------------ the shipped rule, restated
def shipped_path(frames, heads, nq, nk, nk2=0, prescaled=False, fp8=False):
    """The kernel mudg_attention launches in the 16-bit builds with no variant switch set (csrc/attention.hip, mudg_attention)."""
    nqt = (nq + 127) // 128
    if not nk2 and nq >= 512 and nk >= 256:
        if nk % 64:
            return "attn64q"
        return "attn64d<1,1>" if fp8 else ("attn64d<1,0>" if prescaled else "attn64d<0,0>")
    xq = min(8, nqt * frames * heads // 1024)
    if xq >= 2 and nk <= 128 and nk2 <= 64:
        return "xattn<1>" if nk2 else "xattn<0>"
    return "attn<1>" if nk2 else "attn<0>"


PATHS = {"few tiles, ragged keys": "attn<0>", "Nk > 128, short queries": "attn<0>", "Nq 511": "attn<0>", "Nk 255": "attn<0>",
         "many query tiles, ragged last": "xattn<0>", "long, ragged keys": "attn64q", "long, Nq 512 Nk 256": "attn64d<0,0>",
         "long, Nq 513 Nk 320": "attn64d<0,0>", "long, shared keys": "attn64d<0,0>", "long, 2304 tokens": "attn64d<0,0>",
         "text + image, few tiles": "attn<1>", "text + ragged second set": "attn<1>", "text + image, many query tiles": "xattn<1>"}
LONG = [s for s in A.SHAPES if PATHS[s[0]].startswith("attn64d")]
SELF = [s for s in A.SHAPES if s[3] == s[4] and s[5] == 1]                  # nq == nk, kv_div == 1: what a packed [q | k] matrix serves
IDS = lambda shapes: [s[0] for s in shapes]


def test_attention_shapes_reach_every_kernel_under_the_shipped_rule():
    for name, frames, heads, nq, nk, kv_div, *second in A.SHAPES + A.TWO_SET_SHAPES:
        assert shipped_path(frames, heads, nq, nk, second[0] if second else 0) == PATHS[name], name
        assert frames > 1 and heads > 1
    assert {shipped_path(s[1], s[2], s[3], s[4], prescaled=True) for s in LONG} == {"attn64d<1,0>"}
    assert set(PATHS.values()) == {"attn<0>", "attn<1>", "xattn<0>", "xattn<1>", "attn64q", "attn64d<0,0>"}
    assert any(s[5] > 1 for s in LONG) and any(s[3] % 32 for s in LONG) and len(SELF) >= 3
    assert {PATHS[s[0]] for s in SELF} == {"attn<0>", "attn64q", "attn64d<0,0>"}


# ------------------------------------------------------------------------------------------------ helpers
def nan_out(rows, c, dev, gap=0, guard=0):
    """An output operand matrix [rows][c] whose every piece is NaN: a view with row stride c + gap, `guard` NaN rows around it."""
    big = filled_operand(rows + 2 * guard, c + gap, dev, NAN)
    return big[guard:guard + rows, :c]


def nan_operand(x32, ld, dev):
    """fp32 values [rows][cols] as an operand view of a NaN-filled matrix of row width ld: the gap columns are never data.  The 16-bit
    builds take gapped(...) on values the type holds; the split builds cast into the view.  A dense operand to compare with must be
    cast from the same fp32 values: a value whose low piece is half a unit of the high one has two splits (the one made from the
    24-bit number it came from, and the one made from the value itself), and a kernel that drops low x low (bf16x3) tells them apart."""
    rows, cols = x32.shape
    if not SPLIT:
        assert torch.equal(x32.to(hip.operand_dtype()).float(), x32.float())
        return gapped(x32, ld, dev, hip.operand_dtype())
    out = filled_operand(rows, ld, dev, NAN)[:, :cols]
    return ops.cast_rows(x32.float().contiguous().to(dev), out)


def gaps_are_nan(view, guard=0):
    base, (rows, cols) = base_of(view), view.shape
    ld = base.shape[1] // hip.planes()
    ok = all(bool(torch.isnan(base[:, p * ld + cols:(p + 1) * ld]).all()) for p in range(hip.planes()))
    return ok and (guard == 0 or bool(torch.isnan(base[:guard]).all() and torch.isnan(base[-guard:]).all()))


def problem(q32, k32, v32, frames, heads, nk, kv_div, dev):
    """Operands of one key / value set and the values they hold: (q, qv, k, kv, vt, vv)."""
    c = heads * 64
    q, qv = operand(q32, dev) if q32 is not None else (None, None)
    k, kv = operand(k32, dev)
    _, vv = operand(v32, dev)
    return q, qv, k, kv, _vt(vv, frames // kv_div, nk, c, dev), vv


def run(q, k, vt, frames, heads, nq, nk, kv_div, dev, out=None, **kw):
    out = nan_out(frames * nq, heads * 64, dev) if out is None else out
    ops.attention(q, k, vt, out, frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div, **kw)
    return out


def fp8_of(q, k, heads):
    """MX-fp8 copies of Q and K for the score MFMA, and the values they dequantise to (OCP MX: e4m3 x 2^E per 32 columns)."""
    out, deq = [], []
    for t in (q, k):
        y8, s8 = ops.quantize_mxfp8(t)
        e = s8.cpu().double() - 127.0
        deq.append((y8.cpu().view(torch.float8_e4m3fn).double().reshape(t.shape[0], -1, 32) * torch.pow(2.0, e)[..., None]).reshape(t.shape[0], -1))
        out += [y8, s8]
    return tuple(out), deq[0], deq[1]


def assert_exact(name, out, want, tol=None, pi=None, v=None, geo=None, slack=None):
    """out == want: bit for bit in the 16-bit builds, within `tol` (one operand rounding) relative in the split builds.  On failure
    the first wrong element, its 32-row block and — for a gather — the key whose value row came out instead are named."""
    got, want = value(out), want.double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), f"{name}: shape / non-finite output"
    tol = (EPS if SPLIT else 0.0) if tol is None else tol
    bad = (got - want).abs() > tol * want.abs() + (0.0 if slack is None else slack.double())
    if bool(bad.any()):
        r, col = bad.nonzero()[0].tolist()
        msg = (f"{name}: {int(bad.sum())} wrong elements in {int(bad.any(1).sum())} rows; first at row {r} (32-row block #{r // 32}) column {col} "
               f"(head {col // 64}): got {float(got[r, col])!r}, want {float(want[r, col])!r}")
        if pi is not None:
            frames, heads, nq, nk, kv_div = geo
            f, h = r // nq, col // 64
            keys = v.double()[(f // kv_div) * nk:(f // kv_div + 1) * nk, 64 * h:64 * h + 64]
            hits = (keys == got[r, 64 * h:64 * h + 64]).all(1).nonzero().flatten().tolist()
            msg += f"; frame {f} row {r % nq} wants key {int(pi[f, h, r % nq])}, the output is the value row of key(s) {hits or 'none'}"
        raise AssertionError(msg)
    print(f"[attention {MODE}] {name}: {'bit-equal' if tol == 0.0 else f'within {tol:.1e}'}")


def check_random(name, out, want, emu, plain):
    """Whole tensor within 2 x TOL_OP; every 32-row and every 64-column block within 3 x emulation (bf16x6: or 4 x fp32; module text)."""
    d_emu, d_f32 = rel_l2(emu, want), rel_l2(plain, want)
    bound = max(3.0 * d_emu, 4.0 * d_f32) if MODE == "bf16x6" else 3.0 * d_emu
    print(f"[attention {MODE}] {name}: rel-L2 from fp64 of the P / O-rounding emulation {d_emu:.3e}, of fp32 {d_f32:.3e}; block bound {bound:.3e}, "
          f"whole-tensor bound {2 * TOL_OP:.3e}")
    whole = check(name, value(out), want, bound, rb=32, cb=64)
    assert whole <= 2 * TOL_OP, (name, whole)


def check_lse(name, lse, ref_fn):
    want, plain = ref_fn(torch.float64), ref_fn(torch.float32)
    base = rel_l2(plain, want)
    check(name, lse, want, max(TOL_LSE, 4.0 * base), base, rb=32, cb=1)


def rnd(*shape, seed):
    return torch.randn(*shape, generator=A.gen(seed))


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("name,frames,heads,nq,nk,kv_div", A.SHAPES, ids=IDS(A.SHAPES))
def test_attention_gathers_the_value_row_of_the_one_matching_key(cuda, name, frames, heads, nq, nk, kv_div):
    geo = (frames, heads, nq, nk, kv_div)
    for first_tile in (False, True):
        q32, k32, v32, pi, want = A.gather_problem(frames, heads, nq, nk, kv_div, seed=7, first_tile=first_tile)
        form = "first tile" if first_tile else "full range"
        q, qv, k, kv, vt, vv = problem(q32, k32, v32, frames, heads, nk, kv_div, cuda)
        assert torch.equal(qv, q32.double()) and torch.equal(kv, k32.double()) and torch.equal(vv, v32.double())
        if not first_tile:
            out = run(q, k, vt, *geo, cuda, scale=SCALE)
            assert_exact(f"gather {name} ({PATHS[name]})", out, want, pi=pi, v=v32, geo=geo)
        # prescaled Q: first tile = the lean softmax proper where the shape has one; full range = its fallback (every block overflows)
        qp, _ = operand(q32 * CL2, cuda)
        out = run(qp, k, vt, *geo, cuda, q_prescaled=True)
        assert_exact(f"gather {name} prescaled, {form} ({shipped_path(frames, heads, nq, nk, prescaled=True)})", out, want, pi=pi, v=v32, geo=geo)
        if FP8 and PATHS[name].startswith("attn64d"):
            f8, qd, kd = fp8_of(qp, k, heads)
            assert qd.abs().unique().numel() == 1 and torch.equal(kd, k32.double())           # +-one value, +-4: still a code
            out = run(qp, k, vt, *geo, cuda, q_prescaled=True, fp8=f8)
            assert_exact(f"gather {name} prescaled, fp8 scores, {form} (attn64d<1,1>)", out, want, pi=pi, v=v32, geo=geo)


@pytest.mark.parametrize("name,frames,heads,nq,nk,kv_div,nk2,kv_div2", A.TWO_SET_SHAPES, ids=IDS(A.TWO_SET_SHAPES))
def test_attention_gathers_through_either_of_two_key_value_sets(cuda, name, frames, heads, nq, nk, kv_div, nk2, kv_div2):
    """The gather through one set while the other is uniform (K = 0, V constant): O = V[pi] + that constant.  Through the second set it
    checks that set's last-key mask and its kv_div2 mapping row by row.  Bit-equal in the 16-bit builds.  The split builds add, to the
    one operand rounding, what fp32 does to the sum: the uniform set's (sum V) * (1 / Nk), two roundings of the constant, and the
    addition of the two sets, one rounding of O."""
    geo = (frames, heads, nq, nk, kv_div)
    for second in (False, True):
        q32, k32, v32, k2_32, v2_32, pi, want, const = A.gather_two_set_problem(*geo, nk2, kv_div2, seed=7, second=second)
        q, qv, k, kv, vt, vv = problem(q32, k32, v32, frames, heads, nk, kv_div, cuda)
        _, _, k2, k2v, vt2, v2v = problem(None, k2_32, v2_32, frames, heads, nk2, kv_div2, cuda)
        assert all(torch.equal(a, b.double()) for a, b in ((qv, q32), (kv, k32), (vv, v32), (k2v, k2_32), (v2v, v2_32)))
        kw = dict(k2=k2, vt2=vt2, nk2=nk2, kv_div2=kv_div2)
        slack = (2.0 ** -23 * const.abs() + 2.0 ** -24 * want.abs()) if SPLIT else None
        tag = f"gather through the {'second' if second else 'first'} of two sets, {name} ({PATHS[name]})"
        assert_exact(tag, run(q, k, vt, *geo, cuda, scale=SCALE, **kw), want, slack=slack)
        qp, _ = operand(q32 * CL2, cuda)
        assert_exact(tag + " prescaled", run(qp, k, vt, *geo, cuda, q_prescaled=True, **kw), want, slack=slack)


# ------------------------------------------------------------------------------------------------ uniform
@pytest.mark.parametrize("case", range(len(A.SHAPES) + len(A.TWO_SET_SHAPES)), ids=IDS(A.SHAPES + A.TWO_SET_SHAPES))
def test_attention_over_zero_keys_returns_the_constant_value_and_log2_nk(cuda, case):
    name, frames, heads, nq, nk, kv_div, *second = (A.SHAPES + A.TWO_SET_SHAPES)[case]
    nk2, kv_div2 = second or (0, 1)
    geo = (frames, heads, nq, nk, kv_div)
    q32, k32, v32, k2_32, v2_32, want, lse2 = A.uniform_problem(*geo, seed=9, nk2=nk2, kv_div2=kv_div2)
    q, qv, k, kv, vt, vv = problem(q32, k32, v32, frames, heads, nk, kv_div, cuda)
    kw = {}
    if nk2:
        _, _, k2, _, vt2, _ = problem(None, k2_32, v2_32, frames, heads, nk2, kv_div2, cuda)
        kw = dict(k2=k2, vt2=vt2, nk2=nk2, kv_div2=kv_div2)
    tol = 2.0 ** -23 if MODE == "bf16x6" else None                # (sum V) * (1 / Nk): two fp32 roundings, seen by 24 stored bits only
    for prescaled in (False, True):
        out = run(q, k, vt, *geo, cuda, scale=SCALE, q_prescaled=prescaled, **kw)
        assert_exact(f"uniform {name} prescaled={int(prescaled)} ({shipped_path(frames, heads, nq, nk, nk2, prescaled)})", out, want, tol=tol)
    if FP8 and not nk2 and PATHS[name].startswith("attn64d"):
        f8, qd, kd = fp8_of(q, k, heads)
        assert not bool(kd.any())
        assert_exact(f"uniform {name} fp8 scores", run(q, k, vt, *geo, cuda, q_prescaled=True, fp8=f8), want, tol=tol)
    if not SPLIT and not nk2:
        lse = torch.full((frames * nq, heads), NAN, dtype=torch.float32, device=cuda)
        with_lse = run(q, k, vt, *geo, cuda, scale=SCALE, lse=lse)
        assert torch.equal(value(with_lse), value(out))
        check_lse(f"uniform {name} Lse ({PATHS[name]})", lse, lambda dt: torch.log2(torch.full((frames * nq, heads), float(nk), dtype=dt)))


# ------------------------------------------------------------------------------------------------ random operands
@pytest.mark.parametrize("name,frames,heads,nq,nk,kv_div", A.SHAPES, ids=IDS(A.SHAPES))
def test_attention_on_random_operands_block_by_block(cuda, name, frames, heads, nq, nk, kv_div):
    c, geo = heads * 64, (frames, heads, nq, nk, kv_div)
    kwr = dict(frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div)
    q, qv, k, kv, vt, vv = problem(rnd(frames * nq, c, seed=1), rnd(frames // kv_div * nk, c, seed=2), rnd(frames // kv_div * nk, c, seed=3),
                                   frames, heads, nk, kv_div, cuda)
    ref = lambda **kw: A.attention(qv, kv, vv, scale=SCALE, **kwr, **kw)
    want, lse2 = ref()
    plain = ref(dtype=torch.float32)[0]
    tag = f"random {name} ({PATHS[name]})"
    out = run(q, k, vt, *geo, cuda, scale=SCALE)
    check_random(tag, out, want, ref(round_to=RT)[0], plain)
    # accumulate: O += onto operand values already there, rounded once
    o0, o0v = operand(rnd(frames * nq, c, seed=4), cuda)
    acc = run(q, k, vt, *geo, cuda, out=o0, scale=SCALE, accumulate=True)
    check_random(tag + " accumulate", acc, want + o0v, ref(round_to=RT, add=o0v)[0], plain + o0v.float())
    # prescaled Q: its own operand rounding, so its own reference
    qp, qpv = operand(qv.float() * CL2, cuda)
    refp = lambda **kw: A.attention(qpv, kv, vv, base2=True, **kwr, **kw)
    wantp = refp()[0]
    check_random(f"random {name} prescaled ({shipped_path(frames, heads, nq, nk, prescaled=True)})", run(qp, k, vt, *geo, cuda, q_prescaled=True),
                 wantp, refp(round_to=RT)[0], refp(dtype=torch.float32)[0])
    if FP8 and PATHS[name].startswith("attn64d"):
        f8, qd, kd = fp8_of(qp, k, heads)
        ref8 = lambda **kw: A.attention(qd, kd, vv, base2=True, **kwr, **kw)
        check_random(f"random {name} fp8 scores (attn64d<1,1>)", run(qp, k, vt, *geo, cuda, q_prescaled=True, fp8=f8), ref8()[0],
                     ref8(round_to=RT)[0], ref8(dtype=torch.float32)[0])
    if not SPLIT:
        lse = torch.full((frames * nq, heads), NAN, dtype=torch.float32, device=cuda)
        with_lse = run(q, k, vt, *geo, cuda, scale=SCALE, lse=lse)
        assert torch.equal(value(with_lse), value(out)), "asking for Lse changed O"
        check_lse(tag + " Lse", lse, lambda dt: A.attention(qv, kv, vv, scale=SCALE, dtype=dt, **kwr)[1])


@pytest.mark.parametrize("name,frames,heads,nq,nk,kv_div,nk2,kv_div2", A.TWO_SET_SHAPES, ids=IDS(A.TWO_SET_SHAPES))
def test_attention_with_two_key_value_sets_on_random_operands_block_by_block(cuda, name, frames, heads, nq, nk, kv_div, nk2, kv_div2):
    c, geo = heads * 64, (frames, heads, nq, nk, kv_div)
    q, qv, k, kv, vt, vv = problem(rnd(frames * nq, c, seed=1), rnd(frames // kv_div * nk, c, seed=2), rnd(frames // kv_div * nk, c, seed=3),
                                   frames, heads, nk, kv_div, cuda)
    _, _, k2, k2v, vt2, v2v = problem(None, rnd(frames // kv_div2 * nk2, c, seed=4), rnd(frames // kv_div2 * nk2, c, seed=5), frames, heads, nk2,
                                      kv_div2, cuda)
    kwr = dict(frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div, k2=k2v, v2=v2v, nk2=nk2, kv_div2=kv_div2)
    kwl = dict(k2=k2, vt2=vt2, nk2=nk2, kv_div2=kv_div2)
    ref = lambda **kw: A.attention(qv, kv, vv, scale=SCALE, **kwr, **kw)[0]
    check_random(f"random {name} ({PATHS[name]})", run(q, k, vt, *geo, cuda, scale=SCALE, **kwl), ref(), ref(round_to=RT), ref(dtype=torch.float32))
    qp, qpv = operand(qv.float() * CL2, cuda)
    refp = lambda **kw: A.attention(qpv, kv, vv, base2=True, **kwr, **kw)[0]
    check_random(f"random {name} prescaled ({PATHS[name]})", run(qp, k, vt, *geo, cuda, q_prescaled=True, **kwl), refp(), refp(round_to=RT),
                 refp(dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ the engine's calling convention
@pytest.mark.parametrize("name,frames,heads,nq,nk,kv_div", SELF, ids=IDS(SELF))
def test_attention_through_packed_views_is_bit_equal_and_leaves_the_gaps_alone(cuda, name, frames, heads, nq, nk, kv_div):
    """Q and K as column views of one packed [q | k] matrix, O a view with ldo > c, V^T with its row stride padded beyond ceil8(Nk):
    every gap column (and two guard rows around O) is NaN inside the same allocation."""
    c, geo = heads * 64, (frames, heads, nq, nk, kv_div)
    q, qv, k, kv, vt, vv = problem(rnd(frames * nq, c, seed=11), rnd(frames * nk, c, seed=12), rnd(frames * nk, c, seed=13), frames, heads, nk, 1, cuda)
    q, k = operand(qv.float(), cuda)[0], operand(kv.float(), cuda)[0]            # dense and packed: both cast from the values (nan_operand)
    packed = nan_operand(torch.cat([qv, kv], 1).float(), 2 * c + 8, cuda)
    vt32 = vv.float().reshape(frames, nk, c).transpose(1, 2).reshape(frames * c, nk).contiguous()
    vtg = nan_operand(vt32, (nk + 7) // 8 * 8 + 8, cuda)
    assert torch.equal(value(packed), torch.cat([qv, kv], 1)) and torch.equal(value(vtg), vt32.double())
    assert torch.equal(value(q), qv) and torch.equal(value(k), kv)
    for prescaled in (False, True):
        kw = dict(scale=SCALE, q_prescaled=prescaled)
        plain = run(q, k, vt, *geo, cuda, **kw)
        out = nan_out(frames * nq, c, cuda, gap=8, guard=2)
        run(packed[:, :c], packed[:, c:], vtg, *geo, cuda, out=out, **kw)
        got = value(out)
        assert bool(torch.isfinite(got).all()), "a gap value reached the output"
        assert torch.equal(got, value(plain)), f"{name} prescaled={int(prescaled)}: the packed call is not bit-equal to the contiguous one"
        assert gaps_are_nan(out, guard=2), "columns beyond c or rows around O were written"
        assert gaps_are_nan(packed) and gaps_are_nan(vtg)
    print(f"[attention {MODE}] packed views {name} ({PATHS[name]}): bit-equal, gaps and guard rows untouched")


# ------------------------------------------------------------------------------------------------ temporal attention
@pytest.mark.parametrize("clips,t,hw,heads", A.TEMPORAL_SHAPES)
def test_temporal_attention_on_random_operands_block_by_block(cuda, clips, t, hw, heads):
    """T <= 16 and 17 .. 32 are different kernels; clips hw heads is no multiple of the (pixel, head) items of a workgroup (4 or 16)."""
    c, rows = heads * 64, clips * t * hw
    assert (clips * hw * heads) % 4 != 0
    _, v = operand(rnd(rows, 3 * c, seed=20 + t), cuda)
    qkv = nan_operand(v.float(), 3 * c + 8, cuda)
    out = nan_out(rows, c, cuda, gap=8, guard=2)
    ops.temporal_attention(qkv, out, clips=clips, t=t, hw=hw, heads=heads, scale=SCALE)
    ref = lambda **kw: A.temporal_attention(v, clips=clips, t=t, hw=hw, heads=heads, scale=SCALE, **kw)
    check_random(f"temporal attention T={t} HW={hw} heads={heads} clips={clips}", out, ref(), ref(round_to=RT), ref(dtype=torch.float32))
    assert gaps_are_nan(out, guard=2) and gaps_are_nan(qkv)
    dense = nan_out(rows, c, cuda)
    ops.temporal_attention(operand(v.float(), cuda)[0], dense, clips=clips, t=t, hw=hw, heads=heads, scale=SCALE)
    assert torch.equal(value(dense), value(out)), "the row strides changed the result"


# ------------------------------------------------------------------------------------------------ refusals
def test_attention_refuses_what_no_kernel_serves_before_any_launch(cuda):
    """Every call fails a MUDG_REQUIRE that returns before the launch: the NaN-filled output is still NaN afterwards."""
    frames, heads, nq, nk = 2, 2, 640, 640
    c, geo = heads * 64, (2, 2, 640, 640, 1)
    z = lambda rows, cols=c: operand(torch.zeros(rows, cols), cuda)[0]
    q, k, vt, k2, vt2 = z(frames * nq), z(frames * nk), z(frames * c, nk), z(frames * 16), z(frames * c, 16)
    lse = torch.full((frames * nq, heads), NAN, dtype=torch.float32, device=cuda)
    out = nan_out(frames * nq, c, cuda)
    two = dict(k2=k2, vt2=vt2, nk2=16)
    refused = [("Lse with a second set", dict(lse=lse, **two)), ("Lse with prescaled Q", dict(lse=lse, q_prescaled=True)),
               ("Lse with accumulate", dict(lse=lse, accumulate=True)), ("accumulate with a second set", dict(accumulate=True, **two)),
               ("ldvt < Nk", dict(ldvt=(nk - 8) * hip.planes(), svt=c * nk * hip.planes()))]
    if SPLIT:
        refused.append(("Lse in a split build", dict(lse=lse)))
    for what, kw in refused:
        with pytest.raises(hip.MudgError):
            run(q, k, vt, *geo, cuda, out=out, scale=SCALE, **kw)
        assert bool(torch.isnan(base_of(out)).all()) and bool(torch.isnan(lse).all()), what
    if not SPLIT:
        f8, _, _ = fp8_of(q, k, heads)
        for what, g, kw in [("fp8 on a short sequence", (2, 2, 200, 200, 1), dict(q_prescaled=True)), ("fp8 with accumulate", geo, dict(q_prescaled=True, accumulate=True)),
                            ("fp8 without prescaled Q", geo, {})]:
            with pytest.raises(hip.MudgError):
                run(q, k, vt, *g, cuda, out=out, fp8=f8, **kw)
            assert bool(torch.isnan(base_of(out)).all()), what
    else:
        with pytest.raises(hip.MudgError):
            ops.quantize_mxfp8(q)
    for t in (0, 33):
        qkv, o = z(max(t, 1) * 4, 3 * c), nan_out(max(t, 1) * 4, c, cuda)
        with pytest.raises(hip.MudgError):
            ops.temporal_attention(qkv, o, clips=1, t=t, hw=4, heads=heads, scale=SCALE)
        assert bool(torch.isnan(base_of(o)).all()), f"T = {t}"
