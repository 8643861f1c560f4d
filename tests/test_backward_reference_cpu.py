"""tests/backward_reference.py against torch.autograd of the textbook forward, in fp64 on the CPU: the yardstick the backward
kernels are held to (tests/test_backward_kernels_gpu.py) is checked before a GPU is involved.  Bound: 1e-10, fp64 round-off."""
import pytest
import torch
import torch.nn.functional as F

import backward_reference as R

TOL = 1e-10


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def close(got, want, what):
    e = rel(got, want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert e <= TOL, (what, e)


# ------------------------------------------------------------------------------------------------ weight gradients, transposes
def test_wgrad_linear_is_the_gradient_of_f_linear():
    p, m, c = 37, 8, 64
    x, dy = rnd(p, c, seed=1), rnd(p, m, seed=2)
    w = rnd(m, c, seed=3).requires_grad_()
    (dw,) = torch.autograd.grad(F.linear(x, w), w, dy)
    close(R.wgrad(dy, x, p, m, c), dw, "linear")
    # slices of the contraction add up to the whole
    parts = sum(R.wgrad(dy, x, p, m, c, p_range=r) for r in ((0, 16), (16, 32), (32, 37)))
    close(parts, dw, "linear slices")


@pytest.mark.parametrize("frames,h,wd,stride", [(2, 5, 7, 1), (2, 5, 7, 2), (1, 8, 8, 2), (3, 4, 16, 1)])
def test_wgrad_conv3x3_is_the_gradient_of_f_conv2d(frames, h, wd, stride):
    m, c = 8, 6
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    x = rnd(frames, c, h, wd, seed=4)
    w = rnd(m, c, 3, 3, seed=5).requires_grad_()
    dy = rnd(frames, m, ho, wo, seed=6)
    (dw,) = torch.autograd.grad(F.conv2d(x, w, stride=stride, padding=1), w, dy)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    geo = dict(Hin=h, Win=wd, Hout=ho, Wout=wo, stride=stride, pad=1)
    got = R.wgrad(rows(dy), rows(x), frames * ho * wo, m, c, taps=9, mode=1, geo=geo)
    close(got, dw.permute(0, 2, 3, 1).reshape(m, 9 * c), "conv3x3")


def test_wgrad_temporal_is_the_gradient_of_f_conv3d():
    clips, t, hw, m, c = 2, 5, 6, 8, 4
    x = rnd(clips, c, t, hw, 1, seed=7)
    w = rnd(m, c, 3, 1, 1, seed=8).requires_grad_()
    dy = rnd(clips, m, t, hw, 1, seed=9)
    (dw,) = torch.autograd.grad(F.conv3d(x, w, padding=(1, 0, 0)), w, dy)
    rows = lambda v: v[..., 0].permute(0, 2, 3, 1).reshape(-1, v.shape[1])
    got = R.wgrad(rows(dy), rows(x), clips * t * hw, m, c, taps=3, mode=2, geo=dict(T=t, HW=hw))
    close(got, dw[:, :, :, 0, 0].permute(0, 2, 1).reshape(m, 3 * c), "tconv3")


def test_transpose_gather_is_unfold_and_pads_with_zeros():
    frames, h, wd, c, stride = 2, 5, 7, 3, 2
    ho, wo = (h - 1) // stride + 1, (wd - 1) // stride + 1
    x = rnd(frames, c, h, wd, seed=10)
    cols = F.unfold(x, 3, padding=1, stride=stride).reshape(frames, c, 9, ho * wo)          # [f][c][tap][pos]
    rows = x.permute(0, 2, 3, 1).reshape(-1, c)
    p = frames * ho * wo
    geo = dict(Hin=h, Win=wd, Hout=ho, Wout=wo, stride=stride, pad=1)
    for tap in range(9):
        got = R.transpose_gather(rows, p, 1, geo, dy=tap // 3, dx=tap % 3)
        assert got.shape == (c, R.ceil8(p))
        assert torch.equal(got[:, :p], cols[:, :, tap].permute(1, 0, 2).reshape(c, p))
        assert torch.equal(got[:, p:], torch.zeros(c, R.ceil8(p) - p, dtype=torch.float64))
    # temporal taps: the neighbouring frame of the same clip, zero outside it
    clips, t, hw = 2, 3, 5
    y = rnd(clips * t * hw, c, seed=11)
    for dt in range(3):
        got = R.transpose_gather(y, clips * t * hw, 2, dict(T=t, HW=hw), dt=dt)[:, :clips * t * hw].t().reshape(clips, t, hw, c)
        want = torch.zeros(clips, t, hw, c, dtype=torch.float64)
        src = y.reshape(clips, t, hw, c)
        lo, hi = max(0, 1 - dt), min(t, t + 1 - dt)
        want[:, lo:hi] = src[:, lo + dt - 1:hi + dt - 1]
        assert torch.equal(got, want)


def test_transpose_cast_sum_and_operand_planes():
    src = rnd(130, 12, seed=12)
    dst, rows, part = R.transpose_cast_sum(src)
    assert dst.shape == (12, 136) and torch.equal(dst[:, :130], src.t()) and not dst[:, 130:].any()
    assert torch.equal(rows, src)
    assert part.shape == (3, 12)
    close(part[0], src[:64].sum(0), "tile 0")
    close(part[2], src[128:].sum(0), "ragged tile")
    close(part.sum(0), src.sum(0), "bias gradient")
    x = rnd(1000, seed=13).float()
    for dt in (torch.bfloat16, torch.float16):
        one = R.operand_planes(x, dt, 1)
        assert len(one) == 1 and torch.equal(one[0], x.to(dt))
    for planes in (2, 3):                                       # bf16x3 / bf16x6: every piece carries 8 significand bits of what was left
        pieces = R.operand_planes(x, torch.bfloat16, planes)
        assert len(pieces) == planes and torch.equal(pieces[0], x.to(torch.bfloat16))
        back = sum(p.double() for p in pieces)
        assert bool(((back - x.double()).abs() <= x.double().abs() * 2.0 ** (-8 * planes)).all())


def test_group_colsum():
    a, b = rnd(24, 5, seed=14), rnd(24, 5, seed=15)
    close(R.group_colsum(a), a.sum(0, keepdim=True), "one group")
    close(R.group_colsum(a, b, 6), (a * b).reshape(4, 6, 5).sum(1), "groups with b")


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("frames,heads,nq,nk,kv_div", [(2, 2, 9, 9, 1), (4, 1, 7, 5, 2), (4, 2, 6, 3, 4)])
def test_attention_bwd_is_the_gradient_of_softmax_attention(frames, heads, nq, nk, kv_div):
    c, scale = heads * 64, 0.2
    q = rnd(frames * nq, c, seed=16).requires_grad_()
    k = rnd(frames // kv_div * nk, c, seed=17).requires_grad_()
    v = rnd(frames // kv_div * nk, c, seed=18).requires_grad_()
    do = rnd(frames * nq, c, seed=19)

    def forward(q, k, v, nk, kv_div):
        qh = q.reshape(frames, nq, heads, 64).permute(0, 2, 1, 3)
        kh = k.reshape(frames // kv_div, nk, heads, 64).permute(0, 2, 1, 3).repeat_interleave(kv_div, 0)
        vh = v.reshape(frames // kv_div, nk, heads, 64).permute(0, 2, 1, 3).repeat_interleave(kv_div, 0)
        return (torch.softmax(scale * qh @ kh.transpose(-1, -2), -1) @ vh).permute(0, 2, 1, 3).reshape(frames * nq, c)

    want = torch.autograd.grad(forward(q, k, v, nk, kv_div), (q, k, v), do)
    got = R.attention_bwd(q.detach(), k.detach(), v.detach(), do, frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div, scale=scale)
    for g, w, name in zip(got, want, "qkv"):
        close(g, w, "d" + name)
    # two key / value sets, each with its own softmax
    nk2, kv_div2 = 4, frames
    k2, v2 = rnd(nk2, c, seed=20).requires_grad_(), rnd(nk2, c, seed=21).requires_grad_()
    out = forward(q, k, v, nk, kv_div) + forward(q, k2, v2, nk2, kv_div2)
    want = torch.autograd.grad(out, (q, k, v, k2, v2), do)
    got = R.attention_bwd_two_sets(q.detach(), k.detach(), v.detach(), k2.detach(), v2.detach(), do, frames=frames, heads=heads, nq=nq,
                                   nk=nk, kv_div=kv_div, nk2=nk2, kv_div2=kv_div2, scale=scale)
    for g, w, name in zip(got, want, ("q", "k", "v", "k2", "v2")):
        close(g, w, "two sets d" + name)
    # rounding P and dS to 16 bits moves the gradients by about the unit roundoff of that type, and by nothing more
    exact = R.attention_bwd(q.detach(), k.detach(), v.detach(), do, frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div, scale=scale)
    for dt, eps in ((torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)):
        em = R.attention_bwd(q.detach(), k.detach(), v.detach(), do, frames=frames, heads=heads, nq=nq, nk=nk, kv_div=kv_div, scale=scale,
                             round_to=dt)
        for g, w in zip(em, exact):
            assert 0.0 < rel(g, w) < eps


def test_temporal_attention_bwd_is_the_gradient_of_attention_over_frames():
    clips, t, hw, heads, scale = 2, 5, 3, 2, 0.125
    c = heads * 64
    qkv = rnd(clips * t * hw, 3 * c, seed=22).requires_grad_()
    do = rnd(clips * t * hw, c, seed=23)
    x = qkv.reshape(clips, t, hw, 3, heads, 64).permute(3, 0, 2, 4, 1, 5)
    o = torch.softmax(scale * x[0] @ x[1].transpose(-1, -2), -1) @ x[2]                         # [b][s][h][t][64]
    out = o.permute(0, 3, 1, 2, 4).reshape(clips * t * hw, c)
    (want,) = torch.autograd.grad(out, qkv, do)
    close(R.temporal_attention_bwd(qkv.detach(), do, clips=clips, t=t, hw=hw, heads=heads, scale=scale), want, "dqkv")


# ------------------------------------------------------------------------------------------------ norms, softmax
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_groupnorm_stats_and_bwd_are_the_gradient_of_f_group_norm(silu, with_res):
    samples, rows, c, groups, eps = 3, 10, 24, 4, 1e-5
    x = (rnd(samples * rows, c, seed=24) * 1.7 + 0.4).requires_grad_()
    gamma, beta = rnd(c, seed=25).requires_grad_(), rnd(c, seed=26).requires_grad_()
    dy = rnd(samples * rows, c, seed=27)
    xs = x.reshape(samples, rows, c).permute(0, 2, 1)
    y = F.group_norm(xs, groups, gamma, beta, eps)
    if silu:
        y = F.silu(y)
    y = y.permute(0, 2, 1).reshape(samples * rows, c)
    if with_res:
        y = y + x
    dx, dgamma, dbeta = torch.autograd.grad(y, (x, gamma, beta), dy)
    stat = R.groupnorm_stats(x.detach(), samples, rows, groups, eps)
    v = x.detach().reshape(samples, rows, groups, c // groups).permute(0, 2, 1, 3).reshape(samples * groups, -1)
    close(stat[:, 0], v.mean(1), "mean")
    close(stat[:, 1], 1 / torch.sqrt(v.var(1, unbiased=False) + eps), "rstd")
    got_dx, ab = R.groupnorm_bwd(x.detach(), dy, gamma.detach(), beta.detach(), stat, samples, rows, groups, silu, dres=dy if with_res else None)
    assert ab.shape == (samples, c, 2)
    close(got_dx, dx, "dx")
    close(ab[..., 0].sum(0), dbeta, "dbeta")
    close(ab[..., 1].sum(0), dgamma, "dgamma")


@pytest.mark.parametrize("rows,c,with_res", [(1, 8, False), (70, 24, True), (64, 5, False)])
def test_layernorm_bwd_is_the_gradient_of_f_layer_norm(rows, c, with_res):
    eps = 1e-5
    x = rnd(rows, c, seed=28).requires_grad_()
    gamma, beta = rnd(c, seed=29).requires_grad_(), rnd(c, seed=30).requires_grad_()
    dy = rnd(rows, c, seed=31)
    y = F.layer_norm(x, (c,), gamma, beta, eps)
    if with_res:
        y = y + x
    dx, dgamma, dbeta = torch.autograd.grad(y, (x, gamma, beta), dy)
    got_dx, part = R.layernorm_bwd(x.detach(), dy, gamma.detach(), eps, dres=dy if with_res else None)
    assert part.shape == ((rows + 63) // 64, 2, c)
    close(got_dx, dx, "dx")
    close(part[:, 0].sum(0), dgamma, "dgamma")
    close(part[:, 1].sum(0), dbeta, "dbeta")
    if rows > 64:
        close(part[1, 1], dy[64:].sum(0), "second chunk")


def test_softmax_and_its_backward():
    s = (rnd(6, 11, seed=32) * 30).requires_grad_()
    dp = rnd(6, 11, seed=33)
    p = torch.softmax(s * 0.3, 1)
    (ds,) = torch.autograd.grad(p, s, dp)
    close(R.softmax(s.detach() * 0.3), p.detach(), "softmax")
    close(R.softmax_bwd(p.detach(), dp, 0.3), ds, "softmax backward")


# ------------------------------------------------------------------------------------------------ elementwise, resampling
def test_geglu_and_geglu_dropout():
    m, n, p = 7, 12, 0.25
    h = rnd(m, 2 * n, seed=34).requires_grad_()
    dy = rnd(m, n, seed=35)
    y = h[:, :n] * F.gelu(h[:, n:])
    (dh,) = torch.autograd.grad(y, h, dy)
    close(R.geglu(h.detach()), y.detach(), "geglu")
    close(R.geglu(h.detach(), dy), dh, "geglu backward")
    keep = R.keep_mask(1234, m * n, p).reshape(m, n)
    assert 0.5 < float(keep.double().mean()) < 0.95
    assert torch.equal(keep, R.keep_mask(1234, m * n, p).reshape(m, n)) and not torch.equal(keep, R.keep_mask(1235, m * n, p).reshape(m, n))
    yd = y * keep.double() / (1 - p)
    (dhd,) = torch.autograd.grad(h[:, :n] * F.gelu(h[:, n:]) * keep.double() / (1 - p), h, dy)
    close(R.geglu_dropout(h.detach(), keep, p), yd.detach(), "geglu + dropout")
    close(R.geglu_dropout(h.detach(), keep, p, dy), dhd, "geglu + dropout backward")
    assert bool(R.keep_mask(7, 1000, 0.0).all())
    frac = float(R.keep_mask(99, 200000, 0.1).double().mean())
    assert abs(frac - 0.9) < 5e-3


@pytest.mark.parametrize("h,wd", [(5, 7), (4, 6), (1, 3)])
def test_dilate2x_and_upsample_adjoint_are_adjoints_of_their_forwards(h, wd):
    frames, c = 2, 3
    # dilate2x is the adjoint of taking every second pixel (the positions a stride-2 conv's output sits on)
    ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    x = rnd(frames * h * wd, c, seed=36).requires_grad_()
    dy = rnd(frames * ho * wo, c, seed=37)
    sub = x.reshape(frames, h, wd, c)[:, ::2, ::2].reshape(-1, c)
    (want,) = torch.autograd.grad(sub, x, dy)
    assert torch.equal(R.dilate2x(dy, frames, ho, wo, h, wd), want)
    # the adjoint of nearest-2x
    z = rnd(frames * h * wd, c, seed=38).requires_grad_()
    up = F.interpolate(z.reshape(frames, h, wd, c).permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1).reshape(-1, c)
    close(R.upsample2x(z.detach(), frames, h, wd), up.detach(), "upsample")
    g = rnd(frames * 4 * h * wd, c, seed=39)
    (want,) = torch.autograd.grad(up, z, g)
    close(R.upsample2x(g, frames, h, wd, adjoint=True), want, "upsample adjoint")


# ------------------------------------------------------------------------------------------------ reductions
def test_weighted_mse_and_its_gradient():
    pred = rnd(3, 4, 2, 5, seed=40).requires_grad_()
    target, w = rnd(3, 4, 2, 5, seed=41), rnd(3, seed=42).abs()
    loss = F.mse_loss(pred, target, reduction="none").mean((1, 2, 3))
    (grad,) = torch.autograd.grad((loss * w).sum(), pred)
    got_loss, got_grad = R.mse(pred.detach(), target, w)
    close(got_loss, loss.detach(), "loss")
    close(got_grad, grad, "gradient")
    assert R.mse(pred.detach(), target)[1] is None


@pytest.mark.parametrize("max_norm", [0.5, 1e6])
def test_clip_grad_norm_is_torch_clip_grad_norm(max_norm):
    ps = [torch.nn.Parameter(rnd(*s, seed=43 + i)) for i, s in enumerate([(5, 3), (17,), (2, 2, 2)])]
    for i, p in enumerate(ps):
        p.grad = rnd(*p.shape, seed=50 + i)
    before = [p.grad.clone() for p in ps]
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    got_norm, coef, scaled = R.clip_grad_norm(before, max_norm)
    close(got_norm, norm, "norm")
    for s, p in zip(scaled, ps):
        close(s, p.grad, "scaled gradient")
    assert (float(coef) == 1.0) == (max_norm > 1.0)
