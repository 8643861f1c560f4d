"""tests/attention_reference.py before a GPU is involved: the fp64 definitions against torch's scaled_dot_product_attention in
fp64 (bound 1e-12: fp64 round-off), and the condition every input constructor relies on, asserted at every shape
tests/test_attention_kernels_gpu.py uses and printed (lines with "gather" / "uniform").  The conditions are properties of the
inputs — 128 nats on the target, at least 48 nats to any other key — not tolerances."""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_reference as A

TOL = 1e-12
CL2 = 0.125 * A.LOG2E


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=A.gen(seed), dtype=torch.float64)


def sdpa(q, k, v, frames, heads, nq, nk, kv_div, scale):
    """torch's own attention on the (frame, head, row, 64) view, key / value batches repeated for the frames that share them."""
    qh = q.reshape(frames, nq, heads, 64).permute(0, 2, 1, 3)
    kh = k.reshape(frames // kv_div, nk, heads, 64).permute(0, 2, 1, 3).repeat_interleave(kv_div, 0)
    vh = v.reshape(frames // kv_div, nk, heads, 64).permute(0, 2, 1, 3).repeat_interleave(kv_div, 0)
    o = F.scaled_dot_product_attention(qh, kh, vh, scale=scale)
    lse = torch.logsumexp(scale * (qh @ kh.transpose(-1, -2)), dim=-1)                      # [f][h][nq]
    return o.permute(0, 2, 1, 3).reshape(frames * nq, heads * 64), lse.permute(0, 2, 1).reshape(frames * nq, heads)


@pytest.mark.parametrize("frames,heads,nq,nk,kv_div", [(2, 2, 50, 50, 1), (4, 3, 70, 33, 2), (6, 1, 129, 200, 3)])
def test_attention_is_torch_sdpa_in_fp64_and_lse2_is_logsumexp_over_ln2(frames, heads, nq, nk, kv_div):
    c = heads * 64
    q, k, v = rnd(frames * nq, c, seed=1), rnd(frames // kv_div * nk, c, seed=2), rnd(frames // kv_div * nk, c, seed=3)
    kw = dict(frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div)
    o, lse2 = A.attention(q, k, v, scale=0.125, **kw)
    want, lse = sdpa(q, k, v, frames, heads, nq, nk, kv_div, 0.125)
    assert rel(o, want) <= TOL and rel(lse2, lse / math.log(2.0)) <= TOL
    # base 2: Q carrying scale log2(e) gives the same softmax, and the same statistics
    o2, lse2b = A.attention(q * CL2, k, v, base2=True, **kw)
    assert rel(o2, want) <= TOL and rel(lse2b, lse2) <= TOL
    # with no rounding asked for, the emulation is the definition; with one, it moves by about that type's rounding and no more
    for dt, eps in ((torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11), ((torch.bfloat16, 2), 2.0 ** -16)):
        d = rel(A.attention(q, k, v, scale=0.125, round_to=dt, **kw)[0], want)
        assert 0.0 < d < 2 * eps, (dt, d)


def test_two_key_value_sets_are_two_softmaxes_summed():
    frames, heads, nq, nk, kv_div, nk2, kv_div2 = 4, 2, 60, 77, 4, 16, 2
    c = heads * 64
    q, k, v = rnd(frames * nq, c, seed=1), rnd(nk, c, seed=2), rnd(nk, c, seed=3)
    k2, v2 = rnd(2 * nk2, c, seed=4), rnd(2 * nk2, c, seed=5)
    o, lse2 = A.attention(q, k, v, frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div, scale=0.125, k2=k2, v2=v2, nk2=nk2, kv_div2=kv_div2)
    w1, lse = sdpa(q, k, v, frames, heads, nq, nk, kv_div, 0.125)
    w2, _ = sdpa(q, k2, v2, frames, heads, nq, nk2, kv_div2, 0.125)
    assert rel(o, w1 + w2) <= TOL and rel(lse2, lse / math.log(2.0)) <= TOL


@pytest.mark.parametrize("clips,t,hw,heads", [(2, 5, 7, 3), (1, 17, 4, 1)])
def test_temporal_attention_is_torch_sdpa_over_the_frames_of_a_pixel(clips, t, hw, heads):
    c = heads * 64
    qkv = rnd(clips * t * hw, 3 * c + 8, seed=1)                                              # a wider row: the tail is not data
    x = qkv[:, :3 * c].reshape(clips, t, hw, 3, heads, 64).permute(3, 0, 2, 4, 1, 5)
    want = F.scaled_dot_product_attention(x[0], x[1], x[2], scale=0.125).permute(0, 3, 1, 2, 4).reshape(clips * t * hw, c)
    assert rel(A.temporal_attention(qkv, clips=clips, t=t, hw=hw, heads=heads, scale=0.125), want) <= TOL


def _as_stored(x, dt):
    return x.to(dt).to(torch.float64)


@pytest.mark.parametrize("name,frames,heads,nq,nk,kv_div", A.SHAPES)
@pytest.mark.parametrize("first_tile", [False, True])
def test_gather_conditions_at_every_gpu_shape(name, frames, heads, nq, nk, kv_div, first_tile):
    q, k, v, pi, want = A.gather_problem(frames, heads, nq, nk, kv_div, seed=7, first_tile=first_tile)
    kw = dict(frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div)
    for dt in (torch.bfloat16, torch.float16):                            # every input is held exactly by both operand types
        for t in (q, k, v, want):
            assert torch.equal(t.to(dt).float(), t)
    span = min(nk, 64) if first_tile else nk
    hit = torch.zeros(span, dtype=torch.bool)
    hit[pi.flatten()] = True
    assert int(pi.max()) == span - 1 and int(pi[0, 0, nq - 1]) == span - 1
    assert bool(hit.all()) or frames * nq < span, "some key is nobody's target"
    # scaled scores (scale 0.125): the definition itself returns V[pi] to fp64 round-off
    target, gap, miss, _ = A.gather_margins(q, k, pi, c2=CL2, **kw)
    assert float((target - 128.0).abs().max()) < 1e-9 and float(gap.min()) >= 48.0 - 1e-9 and float(miss.max()) < 2.0 ** -40
    o = A.attention(q, k, v, scale=0.125, **kw)[0]
    assert rel(o, want) < 1e-15
    # ... element by element too: what the other keys leave behind is 2^-40 of the value or less, far inside half a unit of any operand
    # type.  A zero in V would fail here: the exact output next to it is ~1e-36, not 0, and a correct kernel returns that
    assert float(v.abs().min()) >= 0.125 and bool(((o - want).abs() <= 2.0 ** -40 * want.abs()).all())
    # prescaled Q as each 16-bit type stores it (scores in base 2): the same margins to within the rounding of 4 scale log2(e) ...
    for dt in (torch.bfloat16, torch.float16):
        _, gap2, miss2, tile = A.gather_margins(_as_stored(q * CL2, dt), k, pi, c2=1.0, **kw)
        assert float(gap2.min()) >= 47.0 and float(miss2.max()) < 2.0 ** -40
        # ... and the lean softmax's range: its reference is the row maximum over the first 64 keys
        worst = tile.reshape(frames, nq, heads).permute(0, 2, 1)                                  # [f][h][nq]
        if first_tile:
            assert float(worst.max()) <= min(A.LEAN_LIMIT_LOG2, 15), "a row leaves the lean range"
        elif nk > 64:
            pad = (-nq) % 128
            blocks = torch.cat([worst, worst.new_full((frames, heads, pad), -math.inf)], 2).reshape(frames, heads, -1, 128).max(3).values
            assert float(blocks.min()) > A.LEAN_LIMIT_LOG2, "a 128-query block would stay on the lean path"
    print(f"[gather {'first tile' if first_tile else 'full range'}] {name} Nq={nq} Nk={nk}: target {float(target.min()):.1f} nats, smallest gap "
          f"{float(gap.min()):.1f} nats, 1 - p_target <= {float(miss.max()):.3e}, prescaled: gap {float(gap2.min()):.1f} nats, largest tile "
          f"sum over the first tile's maximum 2^{float(tile.max()):.1f}")


@pytest.mark.parametrize("name,frames,heads,nq,nk,kv_div,nk2,kv_div2", A.TWO_SET_SHAPES)
@pytest.mark.parametrize("second", [False, True])
def test_two_set_gather_conditions_at_every_gpu_shape(name, frames, heads, nq, nk, kv_div, nk2, kv_div2, second):
    q, k, v, k2, v2, pi, want, const = A.gather_two_set_problem(frames, heads, nq, nk, kv_div, nk2, kv_div2, seed=7, second=second)
    for dt in (torch.bfloat16, torch.float16):
        for t in (q, k, v, k2, v2, want):
            assert torch.equal(t.to(dt).float(), t)
    gk, gdiv, kg = (nk2, kv_div2, k2) if second else (nk, kv_div, k)
    assert int(pi.max()) == gk - 1 and int(pi[0, 0, nq - 1]) == gk - 1 and pi.unique().numel() == gk
    assert not bool((k2 if not second else k).any()) and float(want.min()) >= 8.25 and float(want.max()) <= 30.0
    kw = dict(frames=frames, heads=heads, nq=nq, nk=gk, kv_div=gdiv)
    target, gap, miss, _ = A.gather_margins(q, kg, pi, c2=CL2, **kw)
    assert float((target - 128.0).abs().max()) < 1e-9 and float(gap.min()) >= 48.0 - 1e-9 and float(miss.max()) < 2.0 ** -40
    for dt in (torch.bfloat16, torch.float16):
        _, gap2, miss2, _ = A.gather_margins(_as_stored(q * CL2, dt), kg, pi, c2=1.0, **kw)
        assert float(gap2.min()) >= 47.0 and float(miss2.max()) < 2.0 ** -40
    o = A.attention(q, k, v, frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div, scale=0.125, k2=k2, v2=v2, nk2=nk2, kv_div2=kv_div2)[0]
    assert bool(((o - want).abs() <= 2.0 ** -40 * want.abs()).all())
    print(f"[gather through the {'second' if second else 'first'} of two sets] {name}: {gk} keys, smallest gap {float(gap.min()):.1f} nats, "
          f"1 - p_target <= {float(miss.max()):.3e}, O in [{float(want.min()):g}, {float(want.max()):g}]")


@pytest.mark.parametrize("case", range(len(A.SHAPES) + len(A.TWO_SET_SHAPES)))
def test_uniform_outputs_are_exact_in_both_16_bit_types(case):
    name, frames, heads, nq, nk, kv_div, *second = (A.SHAPES + A.TWO_SET_SHAPES)[case]
    nk2, kv_div2 = second or (0, 1)
    q, k, v, k2, v2, want, lse2 = A.uniform_problem(frames, heads, nq, nk, kv_div, seed=9, nk2=nk2, kv_div2=kv_div2)
    for dt in (torch.bfloat16, torch.float16):
        for t in (k, v, want) + ((k2, v2) if nk2 else ()):
            assert torch.equal(t.to(dt).float(), t)
    assert float(want.abs().min()) > 0.0 or not nk2                        # two sets never cancel: a sum of two roundings stays exact
    per_batch = want.reshape(frames, nq, heads * 64)[:, 0]
    assert per_batch[::max(kv_div, kv_div2)].unique(dim=0).shape[0] == frames // max(kv_div, kv_div2), "two batches share their values"
    assert all(per_batch[f].unique().numel() >= 40 for f in range(frames)), "channels / heads are not told apart"
    o, l2 = A.attention(q, k, v, frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div, scale=0.125, k2=k2, v2=v2, nk2=nk2, kv_div2=kv_div2)
    assert float((o - want).abs().max()) < 1e-13 and float((l2 - lse2).abs().max()) < 1e-13
    print(f"[uniform] {name}: |O| in [{float(want.abs().min()):g}, {float(want.abs().max()):g}], lse2 = log2 {nk} = {math.log2(nk):.6f}")
