"""mudg_temporal_self_attention (csrc/attention.hip, tsattn_fused_kernel): the q | k | v projection and the attention over T in one
launch, held to the two launches it replaces (ops.gemm with the stacked weight, then ops.temporal_attention) and to fp64.

  exact      x and W are small integers, so every q, k, v value is an integer of magnitude <= 8 (the issue allows 256) — exact in bf16 and fp16, no
             rounding in the projection whatever its accumulation order — and the fused result must be bit-equal to
             ops.temporal_attention on that q | k | v.  Every (clip, pixel, frame, head) slice of q | k | v is a distinct pattern
             (asserted), so a wrong row gather or head packing cannot pass.
  random     Gaussian operands against the fp64 definition: qkv = x W^T rounded to the operand type, then
             attention_reference.temporal_attention(round_to = operand).  The fused and the two-launch path differ only in the fp32
             accumulation order of the projection, which can flip single roundings of q, k, v: the two-launch path's error against
             the same reference on the same inputs is measured (whole tensor, worst 32-row block, worst 64-column block: the blocks of
             test_temporal_attention_on_random_operands_block_by_block) and the fused path is allowed twice each.
             Measured (bf16, MI355X): whole-tensor rel-L2 2.63e-3 .. 2.68e-3, worst block 2.91e-3, for BOTH paths — the results were
             bit-identical at all four shapes (profiles/temporal_fused/test_errors.txt).
  shapes     (clips, HW, C): (1, 8, 64) one tile, one head, one K stage; (2, 24, 128) several tiles, the clip boundary inside the
             grid; (1, 40, 320) five heads, K no multiple of 128; (3, 16, 1280) twenty heads, long K, the reference driver's batch.
             One case with ldx, ldw, ldo > C inside NaN-filled allocations (sentinel_buffers.Buf): the gaps must be untouched.
"""
import pytest
import torch

import attention_reference as A
from helpers import golden, rel_l2, seeded_sd, unet_inputs
from mudg_amd import hip, ops
from sentinel_buffers import NAN, Buf

pytestmark = pytest.mark.gpu

SPLIT = hip.planes() > 1
DT = hip.operand_dtype()
RT = (DT, hip.planes())
SCALE = 0.125
T = 16
SHAPES = [(1, 8, 64), (2, 24, 128), (1, 40, 320), (3, 16, 1280)]        # (clips, hw, c)
sixteen_bit = pytest.mark.skipif(SPLIT, reason="the fused kernel belongs to the 16-bit operand builds (the query test covers the refusal)")


def filled_operand(rows, cols, dev, fill):
    return torch.full((rows, cols), fill, dtype=DT, device=dev)


def head_packed(w, heads):
    """[3C][C] rows [to_q | to_k | to_v] -> rows [q_h | k_h | v_h] per head: row 192 h + 64 j + d = row C j + 64 h + d."""
    c = w.shape[1]
    idx = torch.tensor([c * j + 64 * h + d for h in range(heads) for j in range(3) for d in range(64)])
    return w[idx].contiguous()


def integer_problem(clips, hw, c, seed):
    """x in {-1, 0, 1}; four +-1 entries per q / k weight row, eight per v row: |q|, |k| <= 4, |v| <= 8.  Small q and k keep the scaled
    scores at a few units, so the softmax is no one-hot and the bit-equality bites on the exponentials and P V as well."""
    g = A.gen(seed)
    rows = clips * T * hw
    x = torch.randint(-1, 2, (rows, c), generator=g).double()
    w = torch.zeros(3 * c, c, dtype=torch.float64)
    for r in range(3 * c):
        n = 4 if r < 2 * c else 8
        cols = torch.randperm(c, generator=g)[:n]
        w[r, cols] = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return x, w


def random_problem(clips, hw, c, seed):
    g = A.gen(seed)
    x = torch.randn(clips * T * hw, c, generator=g).to(DT).double()
    w = (torch.randn(3 * c, c, generator=g) / c ** 0.5).to(DT).double()
    return x, w


def two_launches(x, w, clips, hw, heads, dev):
    qkv = ops.gemm(x.to(DT).to(dev), w.to(DT).to(dev), frame_rows=hw)
    out = filled_operand(x.shape[0], heads * 64, dev, NAN)
    ops.temporal_attention(qkv, out, clips=clips, t=T, hw=hw, heads=heads, scale=SCALE)
    return qkv, out


def fused(x, w, clips, hw, heads, dev, out=None, xd=None):
    xd = x.to(DT).to(dev) if xd is None else xd
    out = filled_operand(x.shape[0], heads * 64, dev, NAN) if out is None else out
    ops.temporal_self_attention(xd, head_packed(w, heads).to(DT).to(dev), out, clips=clips, t=T, hw=hw, heads=heads, scale=SCALE)
    return out


def block_errors(got, want):
    """(whole, worst 32-row block, worst 64-column block) rel-L2 of got against want."""
    got, want = got.double().cpu(), want.double().cpu()
    d2, w2 = (got - want) ** 2, want ** 2
    rows, cols = d2.shape
    assert rows % 32 == 0 and cols % 64 == 0
    rb = torch.sqrt(d2.reshape(rows // 32, -1).sum(1) / w2.reshape(rows // 32, -1).sum(1))
    cb = torch.sqrt(d2.reshape(rows, cols // 64, 64).sum((0, 2)) / w2.reshape(rows, cols // 64, 64).sum((0, 2)))
    return float(torch.sqrt(d2.sum() / w2.sum())), float(rb.max()), float(cb.max())


@sixteen_bit
@pytest.mark.parametrize("clips,hw,c", SHAPES)
def test_fused_is_bit_equal_to_the_attention_of_the_exact_projection(cuda, clips, hw, c):
    heads = c // 64
    x, w = integer_problem(clips, hw, c, seed=100 + c)
    qkv64 = x @ w.t()
    assert float(qkv64.abs().max()) <= 256 and torch.equal(qkv64.to(DT).double(), qkv64) and torch.equal(x.to(DT).double(), x)
    slices = qkv64.reshape(-1, 3, heads, 64).permute(0, 2, 1, 3).reshape(-1, 192)          # one per (clip, frame, pixel, head)
    assert torch.unique(slices, dim=0).shape[0] == slices.shape[0], "two (row, head) slices carry the same pattern"
    qkv, want = two_launches(x, w, clips, hw, heads, cuda)
    assert torch.equal(qkv.double().cpu(), qkv64), "the projection of integer operands is not exact"
    got = fused(x, w, clips, hw, heads, cuda)
    assert bool(torch.isfinite(got.float()).all()), "output elements were not written"
    bad = (got != want).any(1).nonzero().flatten()
    assert bad.numel() == 0, (f"{int(bad.numel())} rows differ from ops.temporal_attention on the exact q | k | v; first row {int(bad[0])} "
                              f"(clip {int(bad[0]) // (T * hw)}, frame {int(bad[0]) // hw % T}, pixel {int(bad[0]) % hw})")
    assert torch.equal(fused(x, w, clips, hw, heads, cuda), got), "a repeated call changed the bits"


@sixteen_bit
@pytest.mark.parametrize("clips,hw,c", SHAPES)
def test_fused_on_random_operands_within_twice_the_two_launch_error(cuda, clips, hw, c):
    heads = c // 64
    x, w = random_problem(clips, hw, c, seed=200 + c)
    want = A.temporal_attention(A.through(RT)(x @ w.t()), clips=clips, t=T, hw=hw, heads=heads, scale=SCALE, round_to=RT)
    _, two = two_launches(x, w, clips, hw, heads, cuda)
    got = fused(x, w, clips, hw, heads, cuda)
    assert bool(torch.isfinite(got.float()).all())
    e_two, e_fused = block_errors(two, want), block_errors(got, want)
    msg = (f"clips {clips} HW {hw} C {c} rel-L2 from fp64 (whole, worst 32-row block, worst 64-column block): two launches "
           f"{e_two[0]:.3e} {e_two[1]:.3e} {e_two[2]:.3e}, fused {e_fused[0]:.3e} {e_fused[1]:.3e} {e_fused[2]:.3e}")
    print("[temporal fused] " + msg)
    assert all(f <= 2.0 * t for f, t in zip(e_fused, e_two)), msg
    assert torch.equal(fused(x, w, clips, hw, heads, cuda), got), "a repeated call changed the bits"


@sixteen_bit
def test_fused_with_padded_rows_is_bit_equal_and_leaves_the_gaps_alone(cuda):
    clips, hw, c = 2, 24, 128
    heads = c // 64
    x, w = random_problem(clips, hw, c, seed=31)
    rows = x.shape[0]
    dense = fused(x, w, clips, hw, heads, cuda)
    xb = Buf(1, rows, c, c + 8, DT).put([x[None]], cuda)
    wb = Buf(1, 3 * c, c, c + 16, DT).put([head_packed(w, heads)[None]], cuda)
    ob = Buf(1, rows, c, c + 24, DT).blank(cuda)
    ops.temporal_self_attention(xb.view(xb.dev)[0], wb.view(wb.dev)[0], ob.view(ob.dev)[0], clips=clips, t=T, hw=hw, heads=heads, scale=SCALE)
    out = ob.read("O")[0][0]            # asserts that the gap columns and the rows around O still hold NaN
    assert bool(torch.isfinite(out.float()).all()), "a gap value reached the output, or output elements were not written"
    assert torch.equal(out, dense.cpu()), "the row strides changed the result"
    xb.read("x")
    wb.read("W")


@sixteen_bit
def test_fused_does_not_depend_on_the_batch(cuda):
    clips, hw, c = 3, 16, 320
    heads = c // 64
    x, w = random_problem(clips, hw, c, seed=41)
    got = fused(x, w, clips, hw, heads, cuda)
    n = T * hw
    for b in range(clips):
        one = fused(x[b * n:(b + 1) * n], w, 1, hw, heads, cuda)
        assert torch.equal(one, got[b * n:(b + 1) * n]), f"clip {b} alone differs from the stacked call"


def test_query_refuses_what_the_fused_kernel_does_not_serve(cuda):
    ok = ops.temporal_self_attention_ok
    assert ok(16, 24, 5, 320) == (not SPLIT)
    for what, args in [("T = 4", (4, 24, 5, 320)), ("HW = 6", (16, 6, 5, 320)), ("head width 32", (16, 24, 10, 320)),
                       ("head width 128", (16, 24, 5, 640)), ("C no multiple of 64", (16, 24, 5, 328)), ("no heads", (16, 24, 0, 0))]:
        assert not ok(*args), what
    assert not ok(16, 24, 5, 320, ldx=324) and not ok(16, 24, 5, 320, ldo=312) and not ok(16, 24, 5, 320, ldw=316)
    x = filled_operand(4 * 24, 320, cuda, 0.0)
    wh = filled_operand(960, 320, cuda, 0.0)
    out = filled_operand(4 * 24, 320, cuda, NAN)
    with pytest.raises(hip.MudgError):          # refused before any launch
        ops.temporal_self_attention(x, wh, out, clips=1, t=4, hw=24, heads=5, scale=SCALE)
    assert bool(torch.isnan(out).all())
    with pytest.raises(hip.MudgError):          # rows that are not clips * t * hw
        ops.temporal_self_attention(filled_operand(16 * 24, 320, cuda, 0.0), wh, filled_operand(16 * 24, 320, cuda, NAN), clips=2, t=16, hw=24,
                                    heads=5, scale=SCALE)


def test_unet_a_agrees_with_the_switch_off_and_on(cuda, monkeypatch):
    """UNET_A (T = 16, C 64 / 128 / 256 / 256 at HW 384 / 96 / 24 / 6): with the switch on every temporal self-attention of the three
    fine levels is ONE fused call and only the 6-pixel level keeps the two launches; both settings within the golden test's bound of
    the reference and of each other."""
    from mudg_amd.engine import unet as engine
    from test_unet_gpu import TOL_UNET, build_unet
    g = golden("unet_a.pt")
    net = build_unet(g["cfg"], seeded_sd(g["param_shapes"], g["seed"], g["checksum"]), cuda)
    x, ctx = unet_inputs(g["cfg"], g["shape"], g["seed"])
    case = g["cases"][0]
    calls = []
    for name in ("temporal_attention", "temporal_self_attention"):
        def recorded(*a, _f=getattr(ops, name), _n=name, **kw):
            calls.append((_n, kw["hw"]))
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, recorded)
    outs, seen = {}, {}
    for on in (False, True):
        monkeypatch.setattr(engine, "_TSATTN_FUSED", on)
        del calls[:]
        outs[on] = net(x.to(cuda), case["t"].to(cuda), c_label=case["c_label"].to(cuda), context=ctx.to(cuda), fs=case["fs"].to(cuda))
        seen[on] = list(calls)
    e_off, e_on, e_pair = rel_l2(outs[False], case["y"]), rel_l2(outs[True], case["y"]), rel_l2(outs[True], outs[False])
    two = {on: sorted(hw for n, hw in seen[on] if n == "temporal_attention") for on in seen}
    one = {on: sorted(hw for n, hw in seen[on] if n == "temporal_self_attention") for on in seen}
    print(f"[temporal fused] unet_a rel-L2 vs reference: switch off {e_off:.3e}, on {e_on:.3e}; on vs off {e_pair:.3e}; switch on: "
          f"{len(one[True])} fused calls, {len(two[True])} two-launch calls; off: {len(two[False])} two-launch calls")
    assert e_off < TOL_UNET and e_on < TOL_UNET and e_pair < TOL_UNET
    assert one[False] == [] and set(two[False]) == {384, 96, 24, 6}
    if SPLIT:
        assert one[True] == [] and two[True] == two[False] and torch.equal(outs[True], outs[False])
    else:       # a quiet fallback at any fine level fails here
        assert set(two[True]) == {6} and one[True] == [hw for hw in two[False] if hw != 6]
