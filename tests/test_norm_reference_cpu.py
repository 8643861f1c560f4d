"""tests/norm_reference.py against the textbook torch ops and the formulas of lvdm/ in fp64 (needs no GPU), and the conditions the cases of
tests/test_norm_kernels_gpu.py rest on: the exactness of every exact case, and that every row of its case tables reaches the clause
written next to it under the host rules restated in the reference."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_reference as R
import norm_reference as N
import test_norm_kernels_gpu as T

F64, F32 = torch.float64, torch.float32
TOL = 1e-12


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=N.gen(seed), dtype=F64)


def close(a, b, tol=TOL):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------ definitions
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_is_torch_group_norm_on_channels_last_rows(silu):
    s, rows, c, g, eps = 3, 10, 24, 4, 1e-5
    x, gamma, beta = rnd(s * rows, c, seed=1) * 2 + 3, rnd(c, seed=2), rnd(c, seed=3)
    y, mean, rstd = N.groupnorm(x, gamma, beta, s, rows, g, eps, silu)
    want = F.group_norm(x.reshape(s, rows, c).permute(0, 2, 1), g, gamma, beta, eps)
    want = (F.silu(want) if silu else want).permute(0, 2, 1).reshape(s * rows, c)
    close(y, want)
    xg = x.reshape(s, rows, g, c // g).permute(0, 2, 1, 3).reshape(s, g, -1)
    close(mean, xg.mean(2))
    close(rstd, 1.0 / torch.sqrt(xg.var(2, unbiased=False) + eps))
    # two sources are the channel axis cut at csplit
    close(N.groupnorm(R.sources(x[:, :8], x[:, 8:], 8), gamma, beta, s, rows, g, eps, silu)[0], want)


def test_groupnorm_from_partials_of_x_is_groupnorm_and_a_negative_variance_is_clamped():
    s, rows, c, g, eps = 2, 576, 16, 4, 1e-5
    x, gamma, beta = rnd(s * rows, c, seed=4) + 2, rnd(c, seed=5), rnd(c, seed=6)
    want = N.groupnorm(x, gamma, beta, s, rows, g, eps, True)
    for h1, h2 in ((128, 128), (288, 128), (288, 288)):
        if rows % h1 or rows % h2:
            continue
        p1, p2 = R.stats(x[:, :8], h1), R.stats(x[:, 8:], h2)
        for got, w in zip(N.groupnorm_from_partials(p1, p2, x, gamma, beta, s, rows, g, eps, True), want):
            close(got, w, 1e-9)                                            # the one-pass variance in fp64
    p1, p2 = N.exact_partials(2, 256, 64, 24, 32, 128, 128, seed=1, clamp=True)
    mean, rstd = N.partial_statistics(p1, p2, 2, 256, 32, 16.0)
    assert torch.equal(rstd, torch.full((2, 32), 0.25, dtype=F64))
    assert torch.equal(mean, torch.tensor([[N.exact_mean(a, b) for b in range(32)] for a in range(2)], dtype=F64))


def test_layernorm_and_softmax_are_the_torch_ops():
    x, gamma, beta = rnd(7, 40, seed=7) * 3 - 5, rnd(40, seed=8), rnd(40, seed=9)
    close(N.layernorm(x, gamma, beta, 1e-5), F.layer_norm(x, (40,), gamma, beta, 1e-5))
    s = rnd(5, 33, seed=10) * 20
    s[2, ::3] = -math.inf
    close(N.softmax(s), F.softmax(s, 1))
    assert bool((N.softmax(s)[2, ::3] == 0).all())


@pytest.mark.parametrize("dim", [2, 3, 7, 320, 321])
def test_timestep_embedding_is_the_formula_of_lvdm(dim):
    """lvdm/models/utils_diffusion.py (and ops.sinusoid_freqs for the table): args = t[:, None].float() * freqs[None];
    cat([cos(args), sin(args)]), one zero column when dim is odd."""
    from mudg_amd.ops import sinusoid_freqs
    t = torch.tensor([0, 1, 500, 999])
    freqs = sinusoid_freqs(dim, 10000, torch.device("cpu"))
    args = (t[:, None].float() * freqs[None]).double()
    want = torch.cat([torch.cos(args), torch.sin(args)], -1)
    if dim % 2:
        want = torch.cat([want, torch.zeros_like(want[:, :1])], -1)
    close(N.timestep_embedding(t, freqs, dim), want)


def test_small_linear_is_linear_with_silu_before_and_after():
    x, w, b, y0 = rnd(3, 17, seed=11), rnd(5, 17, seed=12), rnd(5, seed=13), rnd(3, 5, seed=14)
    close(N.small_linear(x, w), F.linear(x, w))
    close(N.small_linear(x, w, b, True, True), F.silu(F.linear(F.silu(x), w, b)))
    close(N.small_linear(x, w, b, False, True, into=y0), y0 + F.silu(F.linear(x, w, b)))
    assert bool((N.small_linear_magnitude(x, w) >= F.linear(x, w).abs()).all())


def test_layout_conversions_are_permutations_of_a_frame_window():
    v = rnd(2, 3, 5, 4, 6, seed=15)
    rows = N.ncthw_to_rows(v, 1, 3)
    close(rows, v[:, :, 1:4].permute(0, 2, 3, 4, 1).reshape(2 * 3 * 24, 3))
    close(N.rows_to_ncthw(rows, 2, 3, 3, 4, 6, 0.5), 0.5 * v[:, :, 1:4])


def test_cast_rounds_once_and_the_fp16_stream_saturates():
    v = torch.tensor([[1.0 + 2.0 ** -12, 7.0e4, -7.0e4, 65520.0, math.inf, -math.inf, 1e30, 65504.0]], dtype=F64)
    assert N.cast(v, N.KIND_F16)[0].tolist() == [[1.0, 65504.0, -65504.0, 65504.0, 65504.0, -65504.0, 65504.0, 65504.0]]
    assert torch.equal(N.cast(v, N.KIND_F32)[0], v.float())
    x = rnd(4, 9, seed=16)
    for dt, planes in ((torch.bfloat16, 1), (torch.float16, 1), (torch.bfloat16, 2), (torch.bfloat16, 3)):
        pieces = N.cast(x, N.KIND_OPERAND, dt, planes)
        assert len(pieces) == planes and torch.equal(pieces[0], x.float().to(dt))
        assert float((sum(p.double() for p in pieces) - x).abs().max()) <= 2.0 ** (-8 * planes if dt == torch.bfloat16 else -11) * float(x.abs().max())


def test_gaussian_sample_lincomb_axpy():
    mom, nz = rnd(2, 6, 3, 4, seed=17) * 25, rnd(2, 3, 3, 4, seed=18)
    mean, lv = mom[:, :3], mom[:, 3:].clamp(-30, 20)
    close(N.gaussian_sample(mom, nz, 0.18215), 0.18215 * (mean + torch.exp(0.5 * lv) * nz))          # DiagonalGaussianDistribution.sample
    close(N.gaussian_sample(mom, None, 2.0), 2.0 * mean)
    x, y = rnd(3, 2, 5, seed=19), rnd(3, 2, 5, seed=20)
    ca, cb = torch.tensor([1.0, 2.0, -3.0]), torch.tensor([0.5, 0.0, 4.0])
    close(N.lincomb(x, y, ca, cb), torch.stack([ca[i] * x[i] + cb[i] * y[i] for i in range(3)]))
    close(N.axpy(y, x, -2.5), y - 2.5 * x)


@pytest.mark.parametrize("ways,phi,noise", list(itertools.product((1, 2, 3), (0.0, 0.7), (False, True))))
def test_ddim_step_is_p_sample_ddim_of_lvdm(ways, phi, noise):
    """v-prediction against oracle/ddim.py (the restatement of lvdm/models/samplers/ddim.py, ddim_multiplecond.py and rescale_noise_cfg);
    eps-prediction against the formulas of ddim.py:247-268 written out."""
    from oracle import ddim as O
    b, n = 3, 50
    x, e_c, e_u, e_m, nz = (rnd(b, n, seed=21 + i) for i in range(5))
    coef = [7.5, phi, 0.6, 0.8, 0.95, 0.7, 0.55, 0.3, 1.5, 0.0]
    k = dict(zip(N.COEF, [float(torch.tensor(v, dtype=F32)) for v in coef]))
    oc = {key: torch.tensor([k[key]], dtype=F64) for key in ("sqrt_ac", "sqrt_1mac", "sqrt_a_prev", "dir_coef", "sigma", "rescale")}
    got = N.ddim_step(x, e_c, e_u if ways > 1 else None, e_m if ways > 2 else None, nz if noise else None, coef)
    want = O.p_sample_ddim(x, e_c, e_u if ways > 1 else None, nz if noise else None, oc, k["cfg"], k["phi"], e_img=e_m if ways > 2 else None,
                           cfg_img=k["cfg_img"])
    close(got[0], want[0])
    close(got[1], want[1])
    assert bool((got[3] >= got[1].abs() * (1 - 1e-12)).all()) and bool((got[4] >= got[0].abs() * (1 - 1e-12)).all())
    # eps-prediction: e_t = the guided prediction, pred_x0 = (x - sqrt(1 - a_t) e_t) / sqrt(a_t)
    coef[9] = 1.0
    got = N.ddim_step(x, e_c, e_u if ways > 1 else None, e_m if ways > 2 else None, nz if noise else None, coef)
    v = e_c
    if ways == 2:
        v = e_u + k["cfg"] * (e_c - e_u)
    if ways == 3:
        v = e_u + k["cfg_img"] * (e_m - e_u) + k["cfg"] * (e_c - e_m)
    if phi > 0 and ways > 1:
        v = O.rescale_noise_cfg(v, e_c, k["phi"])
    x0 = (x - k["sqrt_1mac"] * v) / k["sqrt_ac"] * k["rescale"]
    close(got[1], x0)
    close(got[0], k["sqrt_a_prev"] * x0 + k["dir_coef"] * v + (k["sigma"] * nz if noise else 0.0))
    if phi > 0 and ways > 1:
        close(got[2], e_c.std(1) / (got[2] * 0 + (e_u + k["cfg"] * (e_c - e_u) if ways == 2 else
                                                  e_u + k["cfg_img"] * (e_m - e_u) + k["cfg"] * (e_c - e_m)).std(1)))


def test_the_emulations_follow_the_definitions():
    s, rows, c, g = 2, 40, 48, 8
    x, gamma, beta = rnd(s * rows, c, seed=30) + 1, rnd(c, seed=31), rnd(c, seed=32)
    y, mean, rstd = N.groupnorm(x.float(), gamma.float(), beta.float(), s, rows, g, 1e-5, True)
    m_e, r_e = N.gn_stats_emulated(x, s, rows, g, 1e-5)
    close(m_e.double(), mean, 1e-6)
    close(r_e.double(), rstd, 1e-5)
    close(N.gn_apply_emulated(x, m_e, r_e, gamma, beta, s, rows, g, True).double(), y, 1e-5)
    close(N.layernorm_emulated(x, gamma, beta, 1e-5).double(), N.layernorm(x.float(), gamma.float(), beta.float(), 1e-5), 1e-5)
    close(N.softmax_emulated(x).double(), N.softmax(x.float()), 1e-6)


# ------------------------------------------------------------------------------------------------ exactness of the exact cases
@pytest.mark.parametrize("case", T.GN_EXACT, ids=[c["name"] for c in T.GN_EXACT])
def test_exact_groupnorm_cases_are_exact(case):
    """Every partial sum the statistics pass can form, in any order, is an integer below 2^24 (the sums of squares are sums of positive
    integers: a chunk's total bounds every partial); mean, variance + eps and rstd are the stated integers and powers of two; sc, sh and the
    fma are exact (multiples of 2^-4 below 2^24 of them) and every expected output fits the 8 significand bits of bf16."""
    c = case
    s, rows, ch, g = c["s"], c["rows"], c["c"], c["g"]
    cpg = ch // g
    assert (rows * cpg) % 4 == 0
    x = N.exact_groupnorm_input(s, rows, ch, g, seed=11)
    gamma, beta = N.exact_affine(ch, seed=12)
    assert torch.equal(x, x.round()) and float(x.abs().max()) <= 27
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(x.to(dt).float(), x)
    rpc = N.gn_chunk_rows(rows)
    xg = x.double().reshape(s, rows, g, cpg)
    worst = max(float((xg[:, r0:r0 + rpc] ** 2).sum((1, 3)).max()) for r0 in range(0, rows, rpc))
    assert worst < 2 ** 24, worst
    y, mean, rstd = N.groupnorm(x, gamma, beta, s, rows, g, N.EXACT_EPS, False)
    assert torch.equal(mean, torch.tensor([[N.exact_mean(a, b) for b in range(g)] for a in range(s)], dtype=F64))
    assert torch.equal(rstd, torch.tensor([N.exact_rstd(b) for b in range(g)], dtype=F64).expand(s, g))
    assert {float(v) for v in rstd.unique()} <= {0.25, 0.125, 0.0625}
    # the device's fp32 steps, each exact: sc = rstd gamma, mean sc, sh = beta - mean sc, x sc + sh
    m_e, r_e = N.gn_stats_emulated(x, s, rows, g, N.EXACT_EPS)
    assert torch.equal(m_e.double(), mean) and torch.equal(r_e.double(), rstd)
    assert torch.equal(N.gn_apply_emulated(x, m_e, r_e, gamma, beta, s, rows, g, False).double(), y)
    assert torch.equal(y * 16, (y * 16).round()) and float(y.abs().max()) * 16 <= 256
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(R.store(y, N.KIND_OPERAND, dt, 1), y)


@pytest.mark.parametrize("case", T.GN_PARTIALS, ids=[c["name"] for c in T.GN_PARTIALS])
def test_exact_partial_cases_are_exact(case):
    c = case
    s, rows, ch, g, csplit = c["s"], c["rows"], c["c"], c["g"], c["csplit"]
    clamp = c.get("clamp", False)
    eps = 16.0 if clamp else N.EXACT_EPS
    assert rows % c["h1"] == 0 and rows % c["h2"] == 0 and csplit % 8 == 0
    p1, p2 = N.exact_partials(s, rows, ch, csplit, g, c["h1"], c["h2"], seed=23, clamp=clamp)
    assert (p2 is None) == (csplit == ch)
    per = [p.reshape(s, -1, p.shape[1], 2).abs().sum(1) for p in (p1, p2) if p is not None]
    total = torch.cat(per, 1).reshape(s, g, ch // g, 2).sum(2)
    assert float(total.max()) < 2 ** 24, float(total.max())                  # the sum of the magnitudes bounds every partial sum
    for p in (p1, p2):
        if p is not None:
            assert torch.equal(p, p.round()) and torch.equal(p.float().double(), p)
    mean, rstd = N.partial_statistics(p1, p2, s, rows, g, eps)
    assert torch.equal(mean, torch.tensor([[N.exact_mean(a, b) for b in range(g)] for a in range(s)], dtype=F64))
    want_rstd = torch.full((s, g), 0.25, dtype=F64) if clamp else torch.tensor([N.exact_rstd(b) for b in range(g)], dtype=F64).expand(s, g)
    assert torch.equal(rstd, want_rstd)
    x = T.ints(s * rows, ch, seed=21)
    gamma, beta = N.exact_affine(ch, seed=22)
    y = N.groupnorm(x, gamma, beta, s, rows, g, eps, False, stats=(mean, rstd))[0]
    assert torch.equal(y * 16, (y * 16).round()) and float(y.abs().max()) * 16 <= 256
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(R.store(y, N.KIND_OPERAND, dt, 1), y)
    assert torch.equal(N.gn_apply_emulated(x, mean.float(), rstd.float(), gamma, beta, s, rows, g, False).double(), y)
    assert T.partial_where(c) == c["where"]


def test_the_clamp_case_rounds_below_the_square_of_the_mean():
    x = torch.tensor(4097.0)
    assert float(x * x) == 16785408.0 and 4097 ** 2 == 16785409
    m_e, r_e = N.gn_stats_emulated(torch.full((2, 64), 4097.0), 2, 1, 32, 16.0)
    assert bool((m_e == 4097.0).all()) and bool((r_e == 0.25).all())
    assert abs(1.0 / math.sqrt(15.0) - 0.25) > 0.008                         # what rstd would be without the clamp


def test_exact_layernorm_and_softmax_and_misc_inputs():
    for c in T.LN_WIDTHS:
        x, gamma, beta = T.ln_inputs("balanced", 3, c, seed=5)
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(x.to(dt).float(), x)
        assert {float(v) for v in x.double().mean(1)} <= {N.exact_mean(r, 0) for r in range(3)}
    assert 0.0 < math.exp(-40.0) < 2.0 ** -57 and float(torch.exp(torch.tensor(-120.0))) == 0.0
    # the layout tests' integers survive every storage, the halved ones too
    for dt in (torch.bfloat16, torch.float16):
        v = torch.arange(-101, 102, dtype=F32)
        assert torch.equal(v.to(dt).float(), v) and torch.equal((0.5 * v).to(dt).float(), 0.5 * v)


# ------------------------------------------------------------------------------------------------ the tables reach their clauses
def test_groupnorm_tables_reach_the_clauses_written_next_to_them():
    for c in T.GN_EXACT:
        geo = T.gn_geometry(c)
        for key, want in c["hits"].items():
            assert geo[key] == want, (c["name"], key, geo[key], want)
    every = [T.gn_geometry(c) for c in T.GN_EXACT]
    assert {g["cpg"] for g in every} >= {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 30, 80, 257}
    assert {c["rows"] for c in T.GN_EXACT} >= {1, 16, 17, 33, 50, 1000, 2047, 2048, 2100, 70000}
    assert {c["c"] for c in T.GN_EXACT} >= {32, 64, 96, 128, 160, 192, 224, 256, 320, 960, 1328, 1920, 2048, 2056, 2560, 4088, 4096}
    assert {g["nvp"] for g in every} >= {1, 7, 40, 80, 120, 240, 256} and any(g["SRP"] == 1 and g["nvp"] == 240 for g in every)
    assert {g["empty"] for g in every} >= {0, 3, 6, 9} and any(g["chunks"] == 1024 for g in every) and any(64 < g["chunks"] < 1024 for g in every)
    assert {c["s"] for c in T.GN_EXACT} == {1, 3}
    for kernel in ("reg", "lds"):
        assert {c["kind"] for c, g in zip(T.GN_EXACT, every) if g["kernel"] == kernel} == set(T.KINDS), kernel
    assert any(c.get("goff") and g["kernel"] == "lds" and g["CS"] // 8 <= 256 for c, g in zip(T.GN_EXACT, every))
    assert any(g["CS"] // 8 > 256 for g in every)
    # ragged last pass of the register kernel: rows % (RP * GN_UNROLL) in {1, RP * GN_UNROLL - 1}
    lasts = {(g["last"], g["RP"] * N.GN_UNROLL) for g in every if g["kernel"] == "reg"}
    assert any(l == 1 for l, rb in lasts) and any(l == rb - 1 for l, rb in lasts)
    # both branches of the group lookup: cpg < 8, cpg >= 8 a multiple of 8 and not
    cpgs = {g["cpg"] for g in every if g["kernel"] == "reg"}
    assert any(v < 8 for v in cpgs) and any(v >= 8 and v % 8 for v in cpgs) and any(v >= 8 and v % 8 == 0 for v in cpgs)
    two = [(c, g) for c, g in zip(T.GN_EXACT, every) if c.get("csplit")]
    assert any(g["straddle"] for _, g in two) and all(c["gap"] + c["csplit"] != c["gap2"] + c["c"] - c["csplit"] for c, _ in two)
    # all -> every MUDG_GN_REG=0 child case is the LDS-table kernel
    assert all(N.gn_apply(c["c"], True, reg=False)[1] == "lds" for c in T.GN_EXACT)
    # partials: heights, more than 256 blocks, samples
    assert {(c["h1"], c["h2"]) for c in T.GN_PARTIALS if c["csplit"] < c["c"]} >= {(128, 128), (288, 128), (160, 288), (128, 160)}
    assert any(c["rows"] // c["h1"] > 256 for c in T.GN_PARTIALS) and any(c["s"] > 1 for c in T.GN_PARTIALS)
    assert set().union(*(c["where"] for c in T.GN_PARTIALS)) == {1, 2, "both"}
    # bounded: the ratios of GN_CASES, a constant group, both eps, SiLU on and off, the LDS-table kernel
    assert {c["ratio"] for c in T.GN_BOUNDED} == {0.0, 50.0} and {c["eps"] for c in T.GN_BOUNDED} == {1e-5, 1e-6}
    assert {c["silu"] for c in T.GN_BOUNDED} == {True, False} and any("const" in c for c in T.GN_BOUNDED)
    assert {c["kind"] for c in T.GN_BOUNDED} == set(T.KINDS) and any(N.gn_apply(c["c"])[1] == "lds" for c in T.GN_BOUNDED)


def test_layernorm_table_reaches_every_kernel_and_its_dead_rows():
    assert T.LN_WIDTHS == [8, 64, 320, 328, 512, 640, 1024, 1280, 1536, 1544, 2048, 4096]
    for c in T.LN_WIDTHS:
        assert N.ln_kernel(c) == T.LN_HITS[c], c
        kernel, rpb = N.ln_kernel(c)
        rows = T.ln_row_counts(c)
        assert rows == ([1, 3, 4, 5] if kernel.startswith("ln<") else [1, rpb - 1, rpb, rpb + 1])
        assert N.ln_kernel(c, rows_switch=False)[0] == ("ln<3>" if c <= 1536 else "ln<8>")
    assert {T.LN_HITS[c][0] for c in T.LN_WIDTHS} == {"ln<3>", "ln<8>", "ln_rows<8,5>", "ln_rows<16,4>", "ln_rows<16,5>", "ln_rows<32,4>", "ln_rows<32,5>"}
    assert {T.LN_HITS[c][1] for c in (320, 512, 1024)} == {32, 16, 8}
    assert N.ln_kernel(1536)[0] == "ln<3>" and N.ln_kernel(1544)[0] == "ln<8>"


def test_cast_forms_take_the_stated_path_in_every_build():
    for planes, (form, cols, sgap, dgap, soff, doff), sk, dk in itertools.product((1, 2, 3), T.CAST_FORMS, T.KINDS, T.KINDS):
        lds = (planes if sk == N.KIND_OPERAND else 1) * (cols + sgap)
        ldd = (planes if dk == N.KIND_OPERAND else 1) * (cols + dgap)
        assert N.rows_vec(cols, lds, ldd, sk, dk, soff, doff, planes) == T.CAST_VEC[form], (planes, form, sk, dk)
    assert set(T.CAST_VEC.values()) == {True, False}
    assert T.SOFTMAX_COLS == [1, 63, 64, 77, 255, 256, 257, 1100] and T.DDIM_N == [2, 63, 64, 65, 9216]
