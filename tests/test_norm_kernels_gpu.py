"""Every kernel of csrc/norm.hip and csrc/misc.hip, called through the C-ABI (hip.lib(), raw pointers, the test's own strides, gaps and
base offsets) and held to the plain fp64 definitions of tests/norm_reference.py.  Every operand and result is a sentinel_buffers.Buf view
inside a NaN-filled allocation (gap columns, guard rows); all views are in bounds and everything outside them must still be NaN after the
call.  Operand inputs are made by the library's own cast and read back, so the references see what the kernels read.  The file runs in
bf16 directly, in fp16 / bf16x3 / bf16x6 in the mode children (tests/test_precision_modes_gpu.py) and under MUDG_GN_REG=0 / MUDG_LN_ROWS=0 in
the variant children (tests/test_gemm_variants_gpu.py, VARIANTS_NORM).  tests/test_norm_reference_cpu.py proves, without a GPU, that the
exact cases are exact and that every row of the case tables reaches the clause written next to it.

What reaches what (norm.hip; the steps its kernels share with misc.hip and train.hip — the storage kinds Kind<h16 | float | StreamH>, the
host's with_kind dispatch, pin_requests, fold4 / block_sum4 / block_max4, store_mean_rstd, gn_affine_act, load_affine8, ln_apply1 / 8,
softmax_row_walk — are written once in csrc/rows_shared.h and are reached through every kernel below that uses them):
  gn_stats_kernel<h16 | float | StreamH>   test_groupnorm_exact: GN_EXACT (kind column): empty trailing chunks r1000 / r2047, the 1024-chunk
                                           clamp r70000, idle row classes nvp 40 / 80 / 120 (c320, c2560, c960), nvp 1 (c2056), nvp 240 with
                                           one row class (c1920), nvp 7 (c4088), two sources x2_*; ragged shapes in all three kinds.
  gn_finalize_kernel                       the same cases: lanes loop over > 64 chunks at r2047 (127) and r70000 (1024);
                                           test_groupnorm_clamps_a_negative_variance (var < 0 -> 0, exactly); one-pass formula at mean = 50
                                           spreads and a constant group: test_groupnorm_bounded.
  gn_finalize_ch_kernel                    test_groupnorm_from_partials_exact: hand-made partials that are NOT the sums of X; block heights
                                           (128, 128), (288, 128), (160, 288), (128, 160); groups in source 1, in source 2 and across csplit;
                                           257 blocks per sample; 3 samples; the clamp.
  gn_apply_reg_kernel                      GN_EXACT: cpg 1 .. 7 (the per-channel branch), 8 / 10 / 12 / 30 / 60 / 64 / 80 / 128 / 166 / 511
                                           (the two-group shortcut; its last group in every case), ragged last pass r33 / r63 / r65.
  gn_apply_kernel (LDS table)              c2056 (nvec 257: dr = 0 carries), *_goff (gamma / beta one float off 16 bytes); every case in the
                                           MUDG_GN_REG=0 child.
  ln_kernel<3 | 8>                         test_layernorm: C 8, 64, 328, 1536 | 1544, 2048, 4096, rows 1, 3, 4, 5; the five UNet widths in
                                           the MUDG_LN_ROWS=0 child.
  ln_rows_kernel<8,5 | 16,4 | 16,5 | 32,4 | 32,5>   test_layernorm: C 320, 512, 640, 1024, 1280 with 1, RPB - 1, RPB, RPB + 1 rows (dead rows of
                                           the last wave); all three input kinds with gapped ldx / ldy.
  softmax_rows_kernel                      test_softmax_rows.
misc.hip:
  temb_kernel test_timestep_embedding; small_linear_kernel<float | h16> test_small_linear*; ncthw_to_rows_kernel<float | h16>,
  rows_to_ncthw_kernel<3 sources x 2 destinations> test_layout_conversions; cast_rows_kernel<3 x 3 x {VEC, scalar}> test_cast_rows;
  copy_rows_kernel test_copy_rows; cast_kernel test_cast_f32_bf16; zero_channels_kernel test_zero_channels; axpy_kernel, lincomb_kernel
  test_axpy_and_lincomb; gaussian_sample_kernel test_gaussian_sample; ddim_stats_kernel, ddim_update_kernel test_ddim_step.

Bounds.  EPS = one rounding of the mode's operand storage (2^-8 bf16, 2^-11 fp16, 2^-17 bf16x3, 2^-24 bf16x6); U = 2^-24.
  exact       torch.equal with the ONE rounding of the exactly known value (16-bit builds, fp32 and fp16 results); operand results of the
              split builds within EPS relative.  Statistics within one fp32 ulp.
  statistics  bounded GroupNorm, per (sample, group) against fp64: |mean - ref| <= max(4 E_mean, 2^-22 (|mean| + std)), and relative
              |rstd / ref - 1| <= max(4 E_rstd, 2^-22 (1 + mean^2 / (var + eps))), E = the largest error over the case's pairs of the CPU
              emulation of the one-pass formula (fp32 partials per chunk, fp64 fold).  The rstd floor is the propagation of eight fp32
              roundings of E[x^2] (size mean^2 + var) through rstd = (var + eps)^-1/2: half the variance's relative error.
  elementwise |y - ref| <= 2 EPS |ref| + 8 U (|x| + |mean|) |rstd gamma|: the four fp32 roundings of sc, sh and the fma plus the roundings of
              the two statistics, doubled.  LayerNorm: against fp64 outright, per element and per row (the norms of both sides), mean
              and rstd being the row's.  GroupNorm: see the first addition below.
  blocks      GroupNorm: rel-L2 of every (sample, group) block against fp64 within 3 x the distance of the emulation (which rounds to the
              operand storage) for that block, never below the case's median block; bf16x6: max(that, 4 x the distance of the fp32
              formula).  softmax rows: the same per row.
Every bound that rests on an emulation prints the emulation's distance and the kernel's (-s).

Additions to the bounds the issue states, each from the number formats or the formula, none from a kernel's output:
  GroupNorm, elementwise   ref is the fp64 formula evaluated at the statistics the kernel reported, which the statistics check holds to
              fp64: the error that check admits is not charged twice.  The two bounds of the issue do not compose otherwise: the
              statistics may be off by 2^-22 (|mean| + std), the elementwise budget allots them 8 U |mean|.  At mean = 50 spreads the
              one-pass formula (design) leaves rstd 1e-4 .. 5e-4 off (the emulation reproduces the kernel's figure to three digits), ten
              times the budget; at mean = 0 the mean's error scales with the spread, not with |mean|: against fp64 outright bf16x6 misses
              at one element of c1920_r257_silu (error 3.25e-10, bound 3.21e-10, y = -1.6e-4), every other mode and case passes.
  mean = 50 spreads, blocks        a block's distance is ONE draw of that variance error, shared by all its elements, so a multiple of the
              emulation's draw for the same block bounds nothing: the floor is the emulation's worst block of the case instead of its median.
  rstd floor  2^-22 (1 + mean^2 / (var + eps)), relative, where the issue gives one floor 2^-22 (|mean| + std) for both statistics: that
              unit is the mean's.  Eight fp32 roundings of E[x^2] (size mean^2 + var) pass through rstd = (var + eps)^-1/2 at half the
              variance's relative error.  At the constant group (var = 0, eps 1e-5) it is loose, so rstd sqrt(eps) = 1 is asserted to 2^-22.
  LayerNorm rows   no emulation-based row bound (the issue asks for the two-term bound only): at +-30 spreads one fp32 rounding of the
              mean moves a whole row by 2e-6 of its norm, one draw again.  Both distances are printed.
  SiLU        1.1 x the two-term bound (|silu'| <= 1.1) + 4 U (1 + |a|) |ref|: exp, 1 +, the division and the product at the affine value
              a; the fast exp of the 16-bit builds rounds its argument a log2 e, which is the |a| U.  The issue gives no SiLU term.
  fp16 build  + 2^-24 absolute: results below 2^-14 are subnormal in fp16 storage, spaced 2^-24 (half of it, doubled as the EPS term is).
  softmax     a row's emulation distance is floored at EPS / 8: a (nearly) one-hot row rounds to itself on the CPU, distance 0, while the
              kernel's exp may sit one storage step away on a small entry.  One-hot by 40: the entries are e^-40 = 4e-18, which bf16
              and the split builds hold, so "exactly 0" holds in fp16 only; elsewhere they are held to e^-40 within 2 EPS + 64 U (the
              fast exp forms 40 log2 e = 57.7 in fp32: 57.7 ln 2 U = 40 U of relative error, + the storage rounding), and a row one-hot
              by 120, where fp32's exp underflows, is held to exactly 0 in every build.
  small_linear   sum |x w| includes |bias| and the accumulated-into value: they are terms of the same fp32 sum.

Mutation check (by hand, on scratch copies of the bf16 library, each run under this file and under tests/test_kernels_gpu.py -k "norm or
softmax or ddim or cast or linear or timestep or layout"):
  every statistics chunk drops its last row (r1 - 1)      39 tests here fail (all of test_groupnorm_exact, the clamp, all of
                                     test_groupnorm_bounded); the older file fails 11 (this form is coarse: it moves every mean)
  only each sample's last chunk drops the last row         the same 39 here; older file 7
  mb = st[gq] in the two-group shortcut                    14 here (test_groupnorm_exact r50_c320, c96_g8, c960, c1920, c4088_g8, c1328_g8,
                                     c1328_g16_f32, x2_c320_csplit168; from_partials h128_128, h288_128, h128_160; three bounded); older file 6
  blocks_per_sample <-> blocks_per_sample2                 3 here (from_partials h288_128, h160_288, h128_160: NaN guard blocks are read, in
                                     bounds); the older file's same-height groupnorm tests (13) stay green, its mixed-height ones were not
                                     run: they would read past their partial tensors
  dn for dn - 1 in var_c only                              5 here (test_ddim_step at every n); older file 2.  In both variances the ratio is
                                     unchanged: equivalent mutant, 102 here and 35 there pass
  f16_sat dropped from store8_f16                          3 here (test_cast_rows operand / fp32 / fp16 -> fp16); the older file stays green
  the `live` return before ln_rows_kernel's store dropped  equivalent mutant: dead lanes were redirected to row rows - 1 and store that row's
                                     own values again; 102 here and 35 there pass"""
import ctypes as C
import itertools
import math
import os

import pytest
import torch

import gemm_reference as R
import norm_reference as N
from mudg_amd import hip
from sentinel_buffers import Buf

pytestmark = pytest.mark.gpu

NAN = float("nan")
F64, F32 = torch.float64, torch.float32
MODE = hip.operand_name()
PLANES = hip.planes()
SPLIT = PLANES > 1
OPD = hip.operand_dtype()
OPER, F32K, F16K = R.KIND_OPERAND, R.KIND_F32, R.KIND_F16
KINDS = (OPER, F32K, F16K)
KNAME = {OPER: "operand", F32K: "fp32", F16K: "fp16"}
EPS = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "bf16x3": 2.0 ** -17, "bf16x6": 2.0 ** -24}[MODE]
U = 2.0 ** -24
STORE_ABS = 2.0 ** -24 if MODE == "fp16" else 0.0          # fp16 storage is subnormal below 2^-14: half its spacing of 2^-24, doubled as the relative term is
EINVAL, EUNSUPPORTED = -1, -3
_env = os.environ.get
VARIANT = _env("MUDG_DEBUG_VARIANTS") == "1"
GN_REG = not (VARIANT and _env("MUDG_GN_REG") == "0")
LN_ROWS = not (VARIANT and _env("MUDG_LN_ROWS") == "0")


def _s():
    return torch.cuda.current_stream().cuda_stream


def L():
    return hip.lib()


def ok(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, (what, rc, L().mudg_last_error())


def rnd(*shape, seed, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=N.gen(seed), dtype=F32) * scale + shift


def ints(*shape, seed, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=N.gen(seed)).to(F32)


def kind_dtype(kind):
    return {OPER: OPD, F32K: F32, F16K: torch.float16}[kind]


def kplanes(kind):
    return PLANES if kind == OPER else 1


# ================================================================================================ buffers
def blank(rows, cols, kind, dev, gap=0, off=0):
    """A NaN-filled result [rows][cols] of storage `kind`: row stride planes * (cols + gap), base `off` elements past an aligned address."""
    p = kplanes(kind)
    return Buf(1, rows, cols, p * (cols + gap), kind_dtype(kind), off=off, planes=p).blank(dev)


def holding(pieces, kind, dev, gap=0, off=0, tail_rows=2):
    rows, cols = pieces[0].shape
    p = kplanes(kind)
    return Buf(1, rows, cols, p * (cols + gap), kind_dtype(kind), off=off, planes=p, tail_rows=tail_rows).put([t[None] for t in pieces], dev)


def value(buf, name):
    """The values a buffer holds (the sum of its pieces, fp64) after asserting that nothing outside its view was written."""
    return sum(p[0].to(F64) for p in buf.read(name))


def rows_in(x32, kind, dev, gap=0):
    """fp32 values [rows][cols] as an input of storage `kind` -> (Buf, the values it holds).  Operand storage is written by the library's
    own cast (mudg_cast_rows) into the gapped view and read back."""
    rows, cols = x32.shape
    if kind != OPER:
        held = x32.to(kind_dtype(kind))
        return holding([held], kind, dev, gap), held.to(F64)
    buf = blank(rows, cols, OPER, dev, gap)
    src = x32.to(F32).contiguous().to(dev)
    ok(L().mudg_cast_rows(src.data_ptr(), F32K, cols, buf.ptr, OPER, buf.ld, rows, cols, _s()), "operand cast")
    return buf, value(buf, "operand cast")


def vec_f32(t, dev, off=0):
    """A flat fp32 vector (gamma, beta, coefficients) in a sentinel buffer, `off` floats past a 16-byte boundary."""
    t = t.reshape(1, 1, -1).to(F32)
    return Buf(1, 1, t.shape[-1], t.shape[-1], F32, off=off).put([t], dev)


def flat_blank(n, dtype, dev, off=0):
    return Buf(1, 1, n, n, dtype, off=off).blank(dev)


def assert_stored(name, buf, want64, kind, tol=None):
    """The buffer holds the one rounding of want64: piece by piece bit for bit (16-bit builds, fp32 and fp16 storage), within EPS relative
    for operand storage of the split builds.  Names the first wrong element."""
    got_pieces = [p[0] for p in buf.read(name)]
    if kind == OPER and SPLIT:
        got = sum(p.to(F64) for p in got_pieces)
        bad = ~((got - want64).abs() <= (EPS if tol is None else tol) * want64.abs())
    else:
        want = R.store_pieces(want64, kind, OPD, 1)[0]
        bad = ~((got_pieces[0] == want) | (torch.isnan(want) & torch.isnan(got_pieces[0])))
        got = got_pieces[0].to(F64)
    if bool(bad.any()):
        r, c = bad.nonzero()[0].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())} wrong elements in {int(bad.any(1).sum())} rows, {int(bad.any(0).sum())} columns; first at "
                             f"row {r} column {c}: got {float(got[r, c])!r}, want {float(want64[r, c])!r}")


def block_bound(d_emu, d_f32, pick):
    """Per-block rel-L2 bounds from the emulation's per-block distances: 3 x max(a block's own, pick(all blocks)); bf16x6: or 4 x the same
    of the fp32 formula (module text)."""
    b = 3.0 * torch.maximum(d_emu, pick(d_emu))
    return torch.maximum(b, 4.0 * torch.maximum(d_f32, pick(d_f32))) if MODE == "bf16x6" else b


def block_rel(got, want, blocks):
    """rel-L2 of got against want over the trailing axes of a [blocks][...] reshape given by `blocks` (a callable)."""
    g, w = blocks(got.to(F64)), blocks(want.to(F64))
    return torch.sqrt(((g - w) ** 2).sum(1)) / torch.sqrt((w ** 2).sum(1)).clamp_min(1e-300)


# ================================================================================================ GroupNorm: case tables
def GN(name, s, rows, c, g, kind=OPER, hits=None, **kw):
    return dict(name=name, s=s, rows=rows, c=c, g=g, kind=kind, hits=hits or {}, **kw)


# hits: chunks / empty (statistics chunks, and how many start past the last row), cpg, nvp (vectors per statistics sweep), CS (apply
# slab), kernel (shipped apply kernel), RP (register kernel: rows per pass), last (rows % (RP * GN_UNROLL)), straddle (csplit inside a group)
GN_EXACT = [
    GN("r1_c128", 1, 1, 128, 32, OPER, dict(chunks=1, empty=0, cpg=4, kernel="reg", RP=16, last=1)),
    GN("r16_c64_f32", 3, 16, 64, 32, F32K, dict(chunks=1, cpg=2)),
    GN("r17_c128_f16", 1, 17, 128, 32, F16K, dict(chunks=1, cpg=4, last=17)),
    GN("r33_c256", 3, 33, 256, 32, OPER, dict(chunks=2, cpg=8, RP=8, last=1)),
    GN("r63_c256_f16", 1, 63, 256, 32, F16K, dict(chunks=3, RP=8, last=31)),
    GN("r65_c128_f32", 1, 65, 128, 32, F32K, dict(chunks=4, RP=16, last=1)),
    GN("r50_c320", 3, 50, 320, 32, OPER, dict(chunks=3, cpg=10, nvp=40, CS=320, kernel="reg", RP=6)),
    GN("r50_c320_goff", 1, 50, 320, 32, OPER, dict(kernel="lds"), goff=1),
    GN("r16_c64_goff_f16", 3, 16, 64, 32, F16K, dict(kernel="lds"), goff=1),
    GN("r1000_c64", 1, 1000, 64, 32, OPER, dict(chunks=62, empty=3)),
    GN("r2047_c128_f32", 1, 2047, 128, 32, F32K, dict(chunks=127, empty=6)),
    GN("r2048_c32", 1, 2048, 32, 32, OPER, dict(chunks=32, empty=0, cpg=1)),
    GN("r2100_c96_f16", 1, 2100, 96, 32, F16K, dict(chunks=32, empty=0, cpg=3)),
    GN("r70000_c32", 1, 70000, 32, 32, OPER, dict(chunks=1024, empty=9, cpg=1)),
    GN("c160", 3, 20, 160, 32, OPER, dict(cpg=5)),
    GN("c192_f32", 1, 18, 192, 32, F32K, dict(cpg=6)),
    GN("c224_f16", 1, 12, 224, 32, F16K, dict(cpg=7)),
    GN("c96_g8", 3, 5, 96, 8, OPER, dict(cpg=12)),
    GN("c960", 1, 34, 960, 32, OPER, dict(cpg=30, nvp=120, CS=320)),
    GN("c2560", 3, 9, 2560, 32, OPER, dict(cpg=80, nvp=80, CS=640)),
    GN("c2056_g8", 1, 8, 2056, 8, OPER, dict(cpg=257, nvp=1, CS=2056, kernel="lds")),
    GN("c2056_g8_f32", 3, 8, 2056, 8, F32K, dict(cpg=257, nvp=1, kernel="lds")),
    GN("c1920", 1, 6, 1920, 32, OPER, dict(cpg=60, nvp=240, SRP=1, CS=640)),
    GN("c2048_f16", 1, 5, 2048, 32, F16K, dict(cpg=64, nvp=256, CS=512)),
    GN("c4088_g8", 1, 4, 4088, 8, OPER, dict(cpg=511, nvp=7, CS=584)),
    GN("c4096", 3, 3, 4096, 32, OPER, dict(cpg=128, nvp=256, CS=512, kernel="reg")),
    GN("c1328_g8", 1, 6, 1328, 8, OPER, dict(cpg=166, CS=1328, RP=1, kernel="reg")),
    GN("c1328_g16_f32", 1, 4, 1328, 16, F32K, dict(cpg=83, CS=1328, RP=1)),
    GN("x2_c320_csplit168", 3, 50, 320, 32, OPER, dict(straddle=True, cpg=10), csplit=168, gap=8, gap2=16),
    GN("x2_c64_csplit8_f32", 1, 16, 64, 32, F32K, dict(straddle=False), csplit=8, gap=4, gap2=0),
    GN("x2_c2056_csplit1032_f16", 1, 8, 2056, 8, F16K, dict(straddle=True, kernel="lds"), csplit=1032, gap=0, gap2=16),
]


def gn_geometry(c):
    """What the host rules of csrc/norm.hip make of a case (shipped build, no variant switch)."""
    cs, kernel, rb = N.gn_apply(c["c"], aligned=not c.get("goff"))
    nvp = N.gn_stats_sweep(c["c"] // 8)
    out = dict(chunks=N.gn_chunks(c["rows"]), empty=N.gn_empty_chunks(c["rows"]), cpg=c["c"] // c["g"], nvp=nvp, SRP=256 // nvp, CS=cs,
               kernel=kernel, RP=rb // N.GN_UNROLL if kernel == "reg" else None, last=c["rows"] % rb,
               straddle=bool(c.get("csplit", 0) % (c["c"] // c["g"])))
    return out


def PT(name, s, rows, c, g, csplit, h1, h2, where, kind=OPER, **kw):
    return dict(name=name, s=s, rows=rows, c=c, g=g, csplit=csplit, h1=h1, h2=h2, where=where, kind=kind, **kw)


# where: the set of {1, 2, "both"} a case's groups lie in (source 1, source 2, across csplit)
GN_PARTIALS = [
    PT("h128_one_source", 3, 256, 64, 32, 64, 128, 128, {1}),
    PT("h128_128", 3, 128, 96, 8, 40, 128, 128, {1, 2, "both"}, kind=F32K),
    PT("h288_128", 1, 1152, 80, 8, 24, 288, 128, {1, 2, "both"}),
    PT("h160_288", 3, 1440, 64, 32, 32, 160, 288, {1, 2}, kind=F16K),
    PT("h128_160", 1, 640, 320, 32, 168, 128, 160, {1, 2, "both"}),
    PT("h288_one_source", 1, 576, 32, 32, 32, 288, 288, {1}),
    PT("257_blocks", 1, 257 * 128, 32, 32, 32, 128, 128, {1}),
    PT("clamp", 3, 256, 64, 32, 24, 128, 128, {1, 2}, clamp=True),
]


def partial_where(c):
    cpg = c["c"] // c["g"]
    out = set()
    for g in range(c["g"]):
        lo, hi = g * cpg, (g + 1) * cpg
        out.add(1 if hi <= c["csplit"] else (2 if lo >= c["csplit"] else "both"))
    return out


def BD(name, s, rows, c, g, kind, silu, eps, ratio, **kw):
    return dict(name=name, s=s, rows=rows, c=c, g=g, kind=kind, silu=silu, eps=eps, ratio=ratio, **kw)


# ratio: mean / spread of the inputs (0 and 50: GN_CASES of tests/test_backward_kernels_gpu.py); const: (sample, group) held at 2.0
GN_BOUNDED = [
    BD("c320_r50_silu", 3, 50, 320, 32, OPER, True, 1e-5, 0.0, const=(1, 5)),
    BD("c1280_r257_mean50", 2, 257, 1280, 32, OPER, False, 1e-5, 50.0),
    BD("c32_r17_f32_silu", 3, 17, 32, 32, F32K, True, 1e-6, 0.0),
    BD("c320_r513_f16", 2, 513, 320, 32, F16K, False, 1e-6, 0.0, gap=8, const=(0, 31)),
    BD("c96_r33_x2_f32_mean50", 3, 33, 96, 32, F32K, True, 1e-5, 50.0, csplit=40, gap=4, gap2=8),
    BD("c2056_r7_mean50", 1, 7, 2056, 8, F16K, True, 1e-5, 50.0),
    BD("c1920_r257_silu", 2, 257, 1920, 32, OPER, True, 1e-5, 0.0),
]


# ================================================================================================ GroupNorm: running a case
def gn_sources(xv32, c, dev):
    """The input buffers of a case: one source, or two cut at csplit with their own row strides.  Returns (bufs, the values held)."""
    kind, csplit = c["kind"], c.get("csplit", 0)
    if not csplit:
        b, v = rows_in(xv32, kind, dev, c.get("gap", 0))
        return (b, None), v
    b1, v1 = rows_in(xv32[:, :csplit].contiguous(), kind, dev, c.get("gap", 0))
    b2, v2 = rows_in(xv32[:, csplit:].contiguous(), kind, dev, c.get("gap2", 0))
    return (b1, b2), R.sources(v1, v2, csplit)


def gn_call(c, bufs, gamma, beta, eps, silu, dev, partials=None):
    """mudg_groupnorm (or, with partials = (P1 Buf, h1, P2 Buf | None, h2), mudg_groupnorm_fused_rows) on a case.
    Returns (y Buf, statistics [samples][groups][2] read back from the tail of ws)."""
    s, rows, ch, g = c["s"], c["rows"], c["c"], c["g"]
    b1, b2 = bufs
    gb, bb = vec_f32(gamma, dev, c.get("goff", 0)), vec_f32(beta, dev, c.get("goff", 0))
    y = blank(s * rows, ch, OPER, dev, gap=c.get("ygap", 8))
    if partials is None:
        n = L().mudg_groupnorm_ws_floats(s, g, rows)
        assert n == s * g * 2 * (N.gn_chunks(rows) + 1)
        ws = flat_blank(n, F32, dev)
        rc = L().mudg_groupnorm(b1.ptr, b2.ptr if b2 else None, c.get("csplit", 0), b1.ld, b2.ld if b2 else 0, c["kind"], gb.ptr, bb.ptr, y.ptr, y.ld,
                                s, rows, ch, g, eps, int(silu), ws.ptr, _s())
    else:
        p1, h1, p2, h2 = partials
        ws = flat_blank(2 * s * g, F32, dev)
        rc = L().mudg_groupnorm_fused_rows(b1.ptr, b2.ptr if b2 else None, c["csplit"] if b2 else 0, b1.ld, b2.ld if b2 else 0, c["kind"], gb.ptr, bb.ptr,
                                           y.ptr, y.ld, s, rows, ch, g, eps, int(silu), p1.ptr, h1, p2.ptr if p2 else None, h2, ws.ptr, _s())
    ok(rc, c["name"])
    for b in (b1, b2, gb, bb):
        if b is not None:
            b.read(c["name"] + ": an input")
    w = ws.read(c["name"] + ": ws")[0].reshape(-1)
    assert bool(torch.isfinite(w).all()), f"{c['name']}: the kernels left part of ws unwritten"
    return y, w[-2 * s * g:].reshape(s, g, 2).to(F64)


def assert_stats_exact(name, stat, mean, rstd):
    """Within one fp32 ulp (2^-23 relative, 2^-149 at zero) of the exactly known statistics; names the first wrong (sample, group)."""
    for j, (what, want) in enumerate((("mean", mean), ("rstd", rstd))):
        bad = (stat[..., j] - want).abs() > 2.0 ** -23 * want.abs()
        if bool(bad.any()):
            s, g = bad.nonzero()[0].tolist()
            raise AssertionError(f"{name}: {what} of {int(bad.sum())} (sample, group) pairs; first sample {s} group {g}: got {float(stat[s, g, j])!r}, "
                                 f"want {float(want[s, g])!r}")


@pytest.mark.parametrize("case", GN_EXACT, ids=[c["name"] for c in GN_EXACT])
def test_groupnorm_exact(cuda, case):
    c = case
    s, rows, ch, g = c["s"], c["rows"], c["c"], c["g"]
    x = N.exact_groupnorm_input(s, rows, ch, g, seed=11)
    gamma, beta = N.exact_affine(ch, seed=12)
    bufs, xv = gn_sources(x, c, cuda)
    assert torch.equal(xv, x.to(F64))                                       # integers below 2^8: every storage holds them
    y, stat = gn_call(c, bufs, gamma, beta, N.EXACT_EPS, False, cuda)
    want, mean, rstd = N.groupnorm(xv, gamma, beta, s, rows, g, N.EXACT_EPS, False)
    assert_stats_exact(c["name"], stat, mean, rstd)
    assert_stored(f"groupnorm {c['name']} ({KNAME[c['kind']]}, {N.gn_apply(ch, not c.get('goff'), GN_REG)[1]} apply)", y, want, OPER)


def test_groupnorm_clamps_a_negative_variance(cuda):
    """One row of 4097.0 in fp32: q = fmaf(x, x, 0) rounds 4097^2 = 16785409 to 16785408 (a tie at spacing 2, to even), the group's sum of
    two such is exact, so E[x^2] - mean^2 = -1 whatever the order: the clamp makes var 0 and, with eps = 16, rstd = 1 / 4 (without it
    1 / sqrt(15)); y = fmaf(4097, rstd gamma, beta - 4097 rstd gamma) = beta exactly."""
    c = GN("clamp_4097", 2, 1, 64, 32, F32K)
    x = torch.full((2, 64), 4097.0)
    gamma, beta = N.exact_affine(64, seed=13)
    bufs, xv = gn_sources(x, c, cuda)
    y, stat = gn_call(c, bufs, gamma, beta, 16.0, False, cuda)
    assert_stats_exact(c["name"], stat, torch.full((2, 32), 4097.0, dtype=F64), torch.full((2, 32), 0.25, dtype=F64))
    assert_stored("groupnorm clamp", y, beta.to(F64).expand(2, 64), OPER)


@pytest.mark.parametrize("case", GN_PARTIALS, ids=[c["name"] for c in GN_PARTIALS])
def test_groupnorm_from_partials_exact(cuda, case):
    c = case
    s, rows, ch, g, csplit = c["s"], c["rows"], c["c"], c["g"], c["csplit"]
    clamp = c.get("clamp", False)
    eps = 16.0 if clamp else N.EXACT_EPS
    x = ints(s * rows, ch, seed=21)
    gamma, beta = N.exact_affine(ch, seed=22)
    p1, p2 = N.exact_partials(s, rows, ch, csplit, g, c["h1"], c["h2"], seed=23, clamp=clamp)
    two = dict(c, csplit=csplit if csplit < ch else 0, gap=8, gap2=16)
    bufs, xv = gn_sources(x, two, cuda)
    assert torch.equal(xv, x.to(F64))
    # NaN guard blocks behind each source's partials, as many as the other source has: mixed-up block heights read NaN, in bounds
    guard = s * max(rows // c["h1"], rows // c["h2"])
    pb1 = holding([p1.reshape(p1.shape[0], -1).to(F32)], F32K, cuda, tail_rows=guard)
    pb2 = holding([p2.reshape(p2.shape[0], -1).to(F32)], F32K, cuda, tail_rows=guard) if p2 is not None else None
    y, stat = gn_call(two, bufs, gamma, beta, eps, False, cuda, partials=(pb1, c["h1"], pb2, c["h2"]))
    want, mean, rstd = N.groupnorm_from_partials(p1, p2, xv, gamma, beta, s, rows, g, eps, False)
    # the partials are not the sums of X: statistics taken from a pass over X would be these instead
    _, _, rstd_x = N.groupnorm(xv, gamma, beta, s, rows, g, eps, False)
    assert float((rstd - rstd_x).abs().min()) > 0.01
    for b in (pb1, pb2):
        if b is not None:
            b.read(c["name"] + ": partials")
    assert_stats_exact(c["name"], stat, mean, rstd)
    assert_stored(f"groupnorm from partials {c['name']}", y, want, OPER)


def elementwise_bound(ref, xv, mean_e, rstd_gamma, a=None):
    """The two-term bound of the module text; with the affine value `a` given, its SiLU form."""
    b = 8.0 * U * (xv.abs() + mean_e.abs()) * rstd_gamma.abs()
    if a is None:
        return 2.0 * EPS * ref.abs() + STORE_ABS + b
    return 2.0 * EPS * ref.abs() + STORE_ABS + 1.1 * b + 4.0 * U * (1.0 + a.abs()) * ref.abs()


def assert_elementwise(name, got, ref, bound):
    bad = ~((got - ref).abs() <= bound)
    worst = float(((got - ref).abs() / bound.clamp_min(1e-300)).max())
    print(f"[norm {MODE}] {name}: largest |error| / bound {worst:.3f}")
    if bool(bad.any()):
        r, col = bad.nonzero()[0].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())} elements beyond the bound in {int(bad.any(1).sum())} rows; first at row {r} column {col}: got "
                             f"{float(got[r, col])!r}, want {float(ref[r, col])!r}, bound {float(bound[r, col]):.3e}")


@pytest.mark.parametrize("case", GN_BOUNDED, ids=[c["name"] for c in GN_BOUNDED])
def test_groupnorm_bounded(cuda, case):
    c = case
    s, rows, ch, g, eps, silu = c["s"], c["rows"], c["c"], c["g"], c["eps"], c["silu"]
    cpg = ch // g
    x = rnd(s * rows, ch, seed=31, scale=1.3, shift=1.3 * c["ratio"])
    if "const" in c:
        cs_, cg = c["const"]
        x[cs_ * rows:(cs_ + 1) * rows, cg * cpg:(cg + 1) * cpg] = 2.0
    gamma, beta = rnd(ch, seed=32, scale=0.3, shift=1.0), rnd(ch, seed=33, scale=0.3)
    bufs, xv = gn_sources(x, c, cuda)
    y, stat = gn_call(c, bufs, gamma, beta, eps, silu, cuda)
    got = value(y, c["name"])
    want, mean, rstd = N.groupnorm(xv, gamma, beta, s, rows, g, eps, silu)
    blocks = lambda t: t.reshape(s, rows, g, cpg).permute(0, 2, 1, 3).reshape(s * g, rows * cpg)
    var = blocks(xv).var(1, unbiased=False).reshape(s, g)
    # ---- statistics per (sample, group)
    m_e, r_e = N.gn_stats_emulated(xv, s, rows, g, eps)
    e_mean, e_rstd = float((m_e.to(F64) - mean).abs().max()), float((r_e.to(F64) / rstd - 1).abs().max())
    k_mean, k_rstd = (stat[..., 0] - mean).abs(), (stat[..., 1] / rstd - 1).abs()
    b_mean = torch.maximum(torch.tensor(4.0 * e_mean, dtype=F64), 2.0 ** -22 * (mean.abs() + var.clamp_min(0).sqrt()))
    b_rstd = torch.maximum(torch.tensor(4.0 * e_rstd, dtype=F64), 2.0 ** -22 * (1.0 + mean ** 2 / (var + eps)))
    print(f"[norm {MODE}] groupnorm {c['name']}: statistics, largest error of the emulation: mean {e_mean:.3e}, rstd (relative) {e_rstd:.3e}; "
          f"of the kernel: mean {float(k_mean.max()):.3e}, rstd {float(k_rstd.max()):.3e}")
    assert bool((k_mean <= b_mean).all()), (c["name"], "mean", (k_mean > b_mean).nonzero()[0].tolist(), float(k_mean.max()))
    assert bool((k_rstd <= b_rstd).all()), (c["name"], "rstd", (k_rstd > b_rstd).nonzero()[0].tolist(), float(k_rstd.max()))
    if "const" in c:
        cs_, cg = c["const"]
        assert float(var[cs_, cg]) == 0.0 and abs(float(stat[cs_, cg, 1]) * math.sqrt(eps) - 1.0) <= 2.0 ** -22      # var -> 0: rstd = eps^-1/2
    # ---- every element, at the reported statistics (module text)
    at, _, _ = N.groupnorm(xv, gamma, beta, s, rows, g, eps, False, stats=(stat[..., 0], stat[..., 1]))
    per = lambda t: t.reshape(s, 1, g, 1).expand(s, rows, g, cpg).reshape(s * rows, ch)
    rg = per(stat[..., 1]) * gamma.to(F64).repeat(s * rows, 1)
    ref = at * torch.sigmoid(at) if silu else at
    assert_elementwise(f"groupnorm {c['name']} elementwise", got, ref, elementwise_bound(ref, xv, per(stat[..., 0]), rg, at if silu else None))
    # ---- every (sample, group) block against pure fp64
    emu32 = N.gn_apply_emulated(xv, m_e, r_e, gamma, beta, s, rows, g, silu)
    emu = R.store(emu32.to(F64), OPER, OPD, PLANES)
    d_emu, d_f32, d_k = block_rel(emu, want, blocks), block_rel(emu32, want, blocks), block_rel(got, want, blocks)
    bound = block_bound(d_emu, d_f32, torch.max if c["ratio"] else torch.median)
    print(f"[norm {MODE}] groupnorm {c['name']}: (sample, group) blocks, rel-L2 from fp64: emulation {float(d_emu.max()):.3e} (fp32 formula "
          f"{float(d_f32.max()):.3e}), kernel {float(d_k.max()):.3e}; worst kernel / bound {float((d_k / bound).max()):.3f}")
    assert bool((d_k <= bound).all()), (c["name"], "block", int((d_k / bound).argmax()), float(d_k.max()))


# ================================================================================================ LayerNorm
LN_WIDTHS = [8, 64, 320, 328, 512, 640, 1024, 1280, 1536, 1544, 2048, 4096]
# the kernel a width gets in the shipped build, and the rows a workgroup of it takes
LN_HITS = {8: ("ln<3>", 4), 64: ("ln<3>", 4), 320: ("ln_rows<8,5>", 32), 328: ("ln<3>", 4), 512: ("ln_rows<16,4>", 16), 640: ("ln_rows<16,5>", 16),
           1024: ("ln_rows<32,4>", 8), 1280: ("ln_rows<32,5>", 8), 1536: ("ln<3>", 4), 1544: ("ln<8>", 4), 2048: ("ln<8>", 4), 4096: ("ln<8>", 4)}


def ln_row_counts(c, rows_switch=True):
    kernel, rpb = N.ln_kernel(c, rows_switch)
    return [1, 3, 4, 5] if kernel.startswith("ln<") else [1, rpb - 1, rpb, rpb + 1]


def ln_inputs(form, rows, c, seed):
    """gauss: rows of spread 1.5 around +-30 spreads; balanced: row r holds m_r + {+-p, +-q} in equal counts in a seeded order of its own
    (the output names its row and channel)."""
    if form == "gauss":
        sign = torch.tensor([1.0 if r % 2 == 0 else -1.0 for r in range(rows)])[:, None]
        return rnd(rows, c, seed=seed, scale=1.5) + 45.0 * sign, rnd(c, seed=seed + 1, scale=0.3, shift=1.0), rnd(c, seed=seed + 2, scale=0.3)
    return (N.exact_groupnorm_input(rows, 1, c, 1, seed=seed),) + N.exact_affine(c, seed + 1)


@pytest.mark.parametrize("c", LN_WIDTHS)
def test_layernorm(cuda, c):
    eps = 1e-5
    kernel = N.ln_kernel(c, LN_ROWS)[0]
    for rows, kind, form in itertools.product(ln_row_counts(c, LN_ROWS), KINDS, ("gauss", "balanced")):
        name = f"layernorm C={c} rows={rows} {KNAME[kind]} {form} ({kernel})"
        x, gamma, beta = ln_inputs(form, rows, c, seed=41 + rows)
        xb, xv = rows_in(x, kind, cuda, gap=8 if kind != F32K else 4)
        gb, bb = vec_f32(gamma, cuda), vec_f32(beta, cuda)
        y = blank(rows, c, OPER, cuda, gap=16)
        ok(L().mudg_layernorm(xb.ptr, xb.ld, kind, gb.ptr, bb.ptr, y.ptr, y.ld, rows, c, eps, _s()), name)
        xb.read(name + ": x")
        got = value(y, name)
        want = N.layernorm(xv, gamma, beta, eps)
        mean = xv.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((xv - mean) ** 2).mean(1, keepdim=True) + eps)
        bound = elementwise_bound(want, xv, mean.expand_as(xv), rstd * gamma.to(F64))
        assert_elementwise(name, got, want, bound)
        row_err, row_bound = (got - want).norm(dim=1), bound.norm(dim=1)
        assert bool((row_err <= row_bound).all()), (name, "row", int((row_err / row_bound).argmax()))
        if form == "gauss":                                                   # for the record: no bound rests on these
            ident = lambda t: t
            emu32 = N.layernorm_emulated(xv, gamma, beta, eps)
            d_emu, d_k = block_rel(R.store(emu32.to(F64), OPER, OPD, PLANES), want, ident), block_rel(got, want, ident)
            print(f"[norm {MODE}] {name}: rows, rel-L2 from fp64: emulation {float(d_emu.max()):.3e}, kernel {float(d_k.max()):.3e}")


# ================================================================================================ softmax_rows
SOFTMAX_COLS = [1, 63, 64, 77, 255, 256, 257, 1100]


@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_rows(cuda, cols):
    """Rows: 0 one-hot (one entry 40 above the rest), 1 one-hot by 120 (exp underflows in fp32: exactly 0 in every storage), 2 constant,
    3 .. 6 Gaussian of magnitude 1, 1, 80, 80, the last two of them with -inf entries (not all)."""
    g_ = N.gen(50 + cols)
    s = torch.zeros((7, cols), dtype=F32)
    hot = [int(torch.randint(0, cols, (1,), generator=g_)) for _ in range(2)]
    s[0], s[1], s[2] = -3.0, -100.0, 1.75
    s[0, hot[0]], s[1, hot[1]] = 37.0, 20.0
    s[3:5] = rnd(2, cols, seed=51)
    s[5:7] = rnd(2, cols, seed=52, scale=80.0)
    if cols > 1:
        for r in (4, 6):
            drop = torch.randperm(cols, generator=g_)[:max(1, cols // 3)]
            s[r, drop] = -math.inf
    sb = holding([s], F32K, cuda, gap=3)
    p = blank(7, cols, OPER, cuda, gap=5)
    ok(L().mudg_softmax_rows(sb.ptr, sb.ld, p.ptr, p.ld, 7, cols, _s()), "softmax_rows")
    sb.read("softmax: scores")
    pieces = [t[0] for t in p.read(f"softmax cols={cols}")]
    got = sum(t.to(F64) for t in pieces)
    want = N.softmax(s)
    name = f"softmax_rows cols={cols}"
    # one-hot rows: exactly 1; the rest exactly 0 where exp underflows (row 1), and e^-40 to the storage's precision (row 0)
    for r in (0, 1):
        assert float(got[r, hot[r]]) == 1.0, (name, "hot entry", float(got[r, hot[r]]))
    rest = torch.ones(cols, dtype=torch.bool)
    rest[hot[1]] = False
    assert bool((got[1][rest] == 0).all()), (name, "entries 120 below the maximum are not exactly 0")
    rest[:] = True
    rest[hot[0]] = False
    tiny = math.exp(-40.0)
    if MODE == "fp16":
        assert bool((got[0][rest] == 0).all()), (name, "e^-40 is below fp16's range: exactly 0")
    else:
        assert bool(((got[0][rest] - tiny).abs() <= (2 * EPS + 64 * U) * tiny).all()), (name, "entries 40 below the maximum")
    # constant row: the rounding of 1 / cols (exp(0) = 1, the sum is the integer cols, one IEEE division)
    inv = torch.full((cols,), 1.0, dtype=F32) / torch.tensor(float(cols), dtype=F32)
    for pl, w in enumerate(R.store_pieces(inv.to(F64), OPER, OPD, PLANES)):
        assert torch.equal(pieces[pl][2], w), (name, "constant row, piece", pl)
    # -inf entries: exactly 0
    assert bool((got[s == -math.inf] == 0).all()), (name, "-inf entries")
    # random rows against the three-pass emulation; row sums
    emu32 = N.softmax_emulated(s)
    emu = R.store(emu32.to(F64), OPER, OPD, PLANES)
    ident = lambda t: t[3:]
    d_emu, d_f32, d_k = block_rel(emu, want, ident), block_rel(emu32, want, ident), block_rel(got, want, ident)
    floor = torch.full_like(d_emu, EPS / 8)                      # a row that is (nearly) one-hot rounds to itself: not below a fraction of EPS
    bound = block_bound(torch.maximum(d_emu, floor), d_f32, torch.median)
    print(f"[norm {MODE}] {name}: rows, rel-L2 from fp64: emulation {[f'{v:.2e}' for v in d_emu.tolist()]}, kernel {[f'{v:.2e}' for v in d_k.tolist()]}")
    assert bool((d_k <= bound).all()), (name, d_k.tolist(), bound.tolist())
    assert bool(((got.sum(1) - 1.0).abs() <= cols * EPS).all()), (name, "row sums", got.sum(1).tolist())


# ================================================================================================ misc.hip
@pytest.mark.parametrize("dim", [2, 3, 7, 320, 321])
def test_timestep_embedding(cuda, dim):
    half = dim // 2
    t = torch.tensor([0, 1, 999], dtype=torch.int64)
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F32) / half)
    tb = t.to(cuda)
    fb, out = vec_f32(freqs, cuda), blank(3, dim, F32K, cuda)
    ok(L().mudg_timestep_embedding(tb.data_ptr(), fb.ptr, out.ptr, 3, dim, _s()), "timestep_embedding")
    got, want = value(out, f"timestep_embedding dim={dim}"), N.timestep_embedding(t, freqs, dim)
    err = float((got - want).abs().max())
    print(f"[norm {MODE}] timestep_embedding dim={dim}: largest |error| {err:.3e} (bound 2^-22 = {2.0 ** -22:.3e})")
    assert err <= 2.0 ** -22
    assert torch.equal(got[0, :half], torch.ones(half, dtype=F64)) and torch.equal(got[0, half:], torch.zeros(dim - half, dtype=F64))     # t = 0
    if dim % 2:
        assert bool((got[:, -1] == 0).all())


def small_linear_case(dev, m, n, k, w16, bias, act_in, act_out, accumulate, integer, seed):
    make = (lambda *sh, seed: ints(*sh, seed=seed, lo=-3, hi=3)) if integer else rnd
    x, w, b, y0 = make(m, k, seed=seed), make(n, k, seed=seed + 1), make(n, seed=seed + 2), make(m, n, seed=seed + 3)
    w = w.to(OPD) if w16 else w                                              # 16-bit weights: one plane of the operand type
    xb, bb = holding([x], F32K, dev), vec_f32(b, dev)
    wb = Buf(1, n, k, k, w.dtype).put([w[None]], dev)
    yb = holding([y0], F32K, dev) if accumulate else blank(m, n, F32K, dev)
    ok(L().mudg_small_linear(xb.ptr, wb.ptr, int(w16), bb.ptr if bias else None, yb.ptr, m, n, k, int(act_in), int(act_out), int(accumulate), _s()),
       "small_linear")
    name = f"small_linear M={m} N={n} K={k} {'16-bit' if w16 else 'fp32'} W bias={int(bias)} act_in={int(act_in)} act_out={int(act_out)} acc={int(accumulate)}"
    got = value(yb, name)
    want = N.small_linear(x, w, b if bias else None, act_in, act_out, y0 if accumulate else None)
    if integer and not act_in and not act_out:
        assert torch.equal(got, want), (name, int((got != want).sum()))
        return
    mag = N.small_linear_magnitude(x, w, act_in) + (b.to(F64).abs() if bias else 0.0) + (y0.to(F64).abs() if accumulate else 0.0)
    ratio = float(((got - want).abs() / (4.0 * U * mag).clamp_min(1e-300)).max())
    assert ratio <= 1.0, (name, "largest |error| / (4 U sum |x w|)", ratio)


@pytest.mark.parametrize("w16", [False, True], ids=["w_fp32", "w_16bit"])
def test_small_linear_shapes(cuda, w16):
    for i, (m, n, k) in enumerate(itertools.product([1, 3], [1, 5, 1280], [1, 63, 64, 65, 320])):
        small_linear_case(cuda, m, n, k, w16, True, False, False, False, True, 60 + i)            # integers: exact
        small_linear_case(cuda, m, n, k, w16, i % 2 == 0, False, False, False, False, 160 + i)    # Gaussian: bounded


@pytest.mark.parametrize("w16", [False, True], ids=["w_fp32", "w_16bit"])
def test_small_linear_every_epilogue_combination(cuda, w16):
    for i, (bias, act_in, act_out, acc) in enumerate(itertools.product([False, True], repeat=4)):
        small_linear_case(cuda, 1, 1, 1, w16, bias, act_in, act_out, acc, False, 260 + i)
        small_linear_case(cuda, 3, 5, 65, w16, bias, act_in, act_out, acc, False, 360 + i)
        small_linear_case(cuda, 1, 1, 1, w16, bias, False, False, acc, True, 460 + i)


def test_layout_conversions(cuda):
    """ncthw_to_rows: fp32 and 16-bit sources into channels [coff, coff + C) of an operand rows matrix, frame window [t0, t0 + T) of Ttot;
    rows_to_ncthw: all three row kinds into fp32 and 16-bit tensors, the frames outside the window untouched (NaN), scale 0.5.
    HW = 5 x 59 = 295 (no multiple of 256, more than one block)."""
    b, c, ttot, t0, t, h, w, coff = 2, 3, 5, 1, 3, 5, 59, 2
    hw, rows = h * w, 2 * 3 * 5 * 59
    vals = ints(b, c, ttot, h, w, seed=70, lo=-100, hi=100)                  # integers below 2^8 in magnitude: every storage holds them
    for src_f32 in (1, 0):
        src = Buf(1, 1, vals.numel(), vals.numel(), F32 if src_f32 else OPD).put([vals.reshape(1, 1, -1)], cuda)
        dst = blank(rows, coff + c + 1, OPER, cuda, gap=3)
        keep = rnd(rows, coff + c + 1, seed=71).to(OPD)
        for p in range(PLANES):
            dst.view(dst.cpu, p).copy_(keep[None])
        dst.blank(cuda)
        ok(L().mudg_ncthw_to_rows(src.ptr, src_f32, dst.ptr, b, c, t, hw, dst.ld, coff, ttot, t0, _s()), "ncthw_to_rows")
        name = f"ncthw_to_rows {'fp32' if src_f32 else '16-bit'} source"
        pieces = [x[0] for x in dst.read(name)]
        want = N.ncthw_to_rows(vals, t0, t)
        for pl, wp in enumerate(R.store_pieces(want, OPER, OPD, PLANES)):
            assert torch.equal(pieces[pl][:, coff:coff + c], wp), (name, "piece", pl)
            assert torch.equal(pieces[pl][:, :coff], keep[:, :coff]) and torch.equal(pieces[pl][:, coff + c:], keep[:, coff + c:]), (name, "neighbouring channels")
    rvals = ints(b * t * hw, coff + c + 1, seed=72, lo=-101, hi=101)         # odd values too: x 0.5 is still exact
    for kind, dst_f32 in itertools.product(KINDS, (1, 0)):
        rb, rv = rows_in(rvals, kind, cuda, gap=8)
        out = flat_blank(b * c * ttot * hw, F32 if dst_f32 else OPD, cuda)
        ok(L().mudg_rows_to_ncthw(rb.ptr, kind, rb.ld, coff, out.ptr, dst_f32, b, c, t, hw, 0.5, ttot, t0, _s()), "rows_to_ncthw")
        name = f"rows_to_ncthw {KNAME[kind]} -> {'fp32' if dst_f32 else '16-bit'}"
        got = out.read(name)[0].reshape(b, c, ttot, h, w)
        want = N.rows_to_ncthw(rv[:, coff:coff + c], b, c, t, h, w, 0.5)
        assert torch.equal(got[:, :, t0:t0 + t].to(F64), want.to(F32 if dst_f32 else OPD).to(F64)), name
        assert bool(torch.isnan(got[:, :, :t0].float()).all() and torch.isnan(got[:, :, t0 + t:].float()).all()), (name, "frames outside the window")


# (name, cols, source gap, destination gap, source offset, destination offset): the clause of launch_cast_rows that decides VEC
CAST_FORMS = [("vec", 24, 8, 16, 0, 0), ("cols % 8", 21, 8, 8, 0, 0), ("source base + 1", 24, 8, 8, 1, 0), ("destination base + 1", 24, 8, 8, 0, 1),
              ("ld % 8", 24, 3, 8, 0, 0)]
CAST_VEC = {"vec": True, "cols % 8": False, "source base + 1": False, "destination base + 1": False, "ld % 8": False}
BIG = [7.0e4, -7.0e4, 65504.0, -65504.0, 65520.0, 1.0e30, -1.0e30, math.inf, -math.inf]


def cast_source(kind, rows, cols, to_f16, seed):
    """The pieces a source of storage `kind` holds: Gaussian values; towards the fp16 stream also values beyond +-65504 and +-inf wherever
    the source storage can hold them (operand pieces of a split build cannot hold an infinity: 1e30 stands in)."""
    x = rnd(rows, cols, seed=seed, scale=3.0)
    if to_f16:
        big = torch.tensor([v for v in BIG if not (kind == OPER and SPLIT and math.isinf(v))], dtype=F32)
        x[1, :min(cols, big.numel())] = big[:cols]
        x[rows - 1, -1] = 1.0e5
    return [x.to(torch.float16)] if kind == F16K else R.store_pieces(x.to(F64), kind, OPD, PLANES)       # an fp16 source holds +-inf


@pytest.mark.parametrize("src_kind,dst_kind", list(itertools.product(KINDS, KINDS)), ids=lambda k: KNAME[k])
def test_cast_rows(cuda, src_kind, dst_kind):
    rows = 5
    for form, cols, sgap, dgap, soff, doff in CAST_FORMS:
        pieces = cast_source(src_kind, rows, cols, dst_kind == F16K, seed=80 + cols + sgap)
        src = holding(pieces, src_kind, cuda, gap=sgap, off=soff)
        dst = blank(rows, cols, dst_kind, cuda, gap=dgap, off=doff)
        vec = N.rows_vec(cols, src.ld, dst.ld, src_kind, dst_kind, soff, doff, PLANES)
        ok(L().mudg_cast_rows(src.ptr, src_kind, src.ld, dst.ptr, dst_kind, dst.ld, rows, cols, _s()), "cast_rows")
        name = f"cast_rows {KNAME[src_kind]} -> {KNAME[dst_kind]}, {form} ({'VEC' if vec else 'scalar'})"
        src.read(name + ": source")
        held = sum(p.to(F32) for p in pieces)                                 # the fp32 sum of the pieces, as the kernels form it
        got = [p[0] for p in dst.read(name)]
        want = N.cast(held.to(F64), dst_kind, OPD, PLANES)
        for pl, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), (name, "piece", pl, int((g != w).sum()), "elements differ")


def test_copy_rows(cuda):
    rows = 5
    for form, cols, sgap, dgap, soff, doff in CAST_FORMS:
        pieces = [rnd(rows, cols, seed=90 + p).to(OPD) for p in range(PLANES)]                    # independent planes: a copy moves bits
        src = holding(pieces, OPER, cuda, gap=sgap, off=soff)
        dst = blank(rows, cols, OPER, cuda, gap=dgap, off=doff)
        ok(L().mudg_copy_rows(src.ptr, src.ld, dst.ptr, dst.ld, rows, cols, _s()), "copy_rows")
        name = f"copy_rows {form} ({'VEC' if N.rows_vec(cols, src.ld, dst.ld, OPER, OPER, soff, doff, PLANES) else 'scalar'})"
        for pl, g in enumerate(dst.read(name)):
            assert torch.equal(g[0], pieces[pl]), (name, "piece", pl)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1003])
def test_cast_f32_bf16(cuda, n):
    x = rnd(n, seed=100 + n, scale=3.0)
    src, dst = vec_f32(x, cuda), flat_blank(n, OPD, cuda)
    rc = L().mudg_cast_f32_bf16(src.ptr, dst.ptr, n, _s())
    torch.cuda.synchronize()
    got = dst.read(f"cast_f32_bf16 n={n}")[0].reshape(-1)
    if SPLIT:
        assert rc == EUNSUPPORTED and bool(torch.isnan(got.float()).all()), "the flat cast is refused in the split builds, nothing written"
    else:
        assert rc == 0 and torch.equal(got, x.to(OPD))


def test_zero_channels(cuda):
    rows, cols, c0, c1 = 300, 11, 3, 8
    pieces = [rnd(rows, cols, seed=110 + p).to(OPD) + 4.0 for p in range(PLANES)]
    buf = holding(pieces, OPER, cuda, gap=2)
    ok(L().mudg_zero_channels(buf.ptr, rows, buf.ld, c0, c1, _s()), "zero_channels")
    for pl, g in enumerate(buf.read("zero_channels")):
        assert bool((g[0][:, c0:c1] == 0).all()), ("plane", pl, "not zeroed")
        assert torch.equal(g[0][:, :c0], pieces[pl][:, :c0]) and torch.equal(g[0][:, c1:], pieces[pl][:, c1:]), ("plane", pl, "neighbouring channels")


def test_axpy_and_lincomb(cuda):
    for n in (1, 255, 257, 1000):
        x, y = ints(n, seed=120), ints(n, seed=121)
        xb, yb = vec_f32(x, cuda), vec_f32(y, cuda)
        ok(L().mudg_axpy_f32(yb.ptr, xb.ptr, n, -2.5, _s()), "axpy")
        assert torch.equal(value(yb, f"axpy n={n}").reshape(-1), N.axpy(y, x, -2.5))
    for b, n in ((3, 1024 * 256 + 5), (3, 1), (2, 300)):
        x, y = ints(b, n, seed=122), ints(b, n, seed=123)
        ca, cb = torch.tensor([2.0, -3.0, 0.5][:b]), torch.tensor([-1.0, 4.0, 8.0][:b])
        xb, yb, ab, bb = holding([x], F32K, cuda), holding([y], F32K, cuda), vec_f32(ca, cuda), vec_f32(cb, cuda)
        out = blank(b, n, F32K, cuda)
        ok(L().mudg_lincomb(out.ptr, xb.ptr, yb.ptr, ab.ptr, bb.ptr, b, n, _s()), "lincomb")
        got, want = value(out, f"lincomb B={b} n={n}"), N.lincomb(x, y, ca, cb)
        assert torch.equal(got, want), (b, n, int((got != want).sum()))


@pytest.mark.parametrize("noise", [True, False], ids=["sample", "mode"])
def test_gaussian_sample(cuda, noise):
    n, c, h, w, scale = 2, 3, 5, 59, 0.18215
    mom = rnd(n, 2 * c, h, w, seed=130)
    lv = torch.tensor([-40.0, 0.0, 30.0, -30.0, 20.0, 1.5])
    mom[:, c:] = lv[torch.randint(0, 6, (n, c, h, w), generator=N.gen(131))]
    nz = rnd(n, c, h, w, seed=132) if noise else None
    mb = vec_f32(mom, cuda)
    nb = vec_f32(nz, cuda) if noise else None
    out = flat_blank(n * c * h * w, F32, cuda)
    ok(L().mudg_gaussian_sample(mb.ptr, nb.ptr if noise else None, out.ptr, n, c, h * w, scale, _s()), "gaussian_sample")
    got = out.read("gaussian_sample")[0].reshape(n, c, h, w).to(F64)
    sc32 = float(torch.tensor(scale, dtype=F32))
    want = N.gaussian_sample(mom, nz, sc32)
    mag = sc32 * (mom[:, :c].to(F64).abs() + (torch.exp(0.5 * mom[:, c:].to(F64).clamp(-30, 20)) * nz.to(F64).abs() if noise else 0.0))
    ratio = float(((got - want).abs() / (4.0 * 2.0 ** -23 * mag).clamp_min(1e-300)).max())
    print(f"[norm {MODE}] gaussian_sample noise={int(noise)}: largest |error| in units of 4 ulp {ratio:.3f}")
    assert ratio <= 1.0


DDIM_N = [2, 63, 64, 65, 4 * 16 * 9 * 16]


@pytest.mark.parametrize("n", DDIM_N)
def test_ddim_step(cuda, n):
    """B = 3 samples whose predictions differ by 4 x in scale (a ratio taken from another sample's partials is off by 4 or 16); both
    prediction forms, no guidance, two- and three-way guidance, phi 0 and 0.7, with and without noise.  pred_x0 within 1e-6 of the size of
    its terms (the ratio rests on fp64 partials), x_prev within 8 U sum |terms|."""
    bsz = 3
    scale = torch.tensor([1.0, 4.0, 16.0])[:, None]
    x, e_c, e_u, e_m, nz = (rnd(bsz, n, seed=140 + i) for i in range(5))
    e_c, e_u, e_m = e_c * scale, (e_c * 0.8 + 0.3 * e_u) * scale, (e_c * 0.9 + 0.2 * e_m) * scale
    bufs = {k: holding([v], F32K, cuda) for k, v in dict(x=x, e_c=e_c, e_u=e_u, e_m=e_m, nz=nz).items()}
    ws_n = L().mudg_ddim_ws_doubles(bsz)
    worst0 = worst = 0.0
    for eps_form, ways, phi, noise in itertools.product((0.0, 1.0), (1, 2, 3), (0.0, 0.7), (False, True)):
        coef = [7.5, phi, 0.6, 0.8, 0.95, 0.7, 0.55, 0.3, 1.5, eps_form]
        ws = flat_blank(ws_n, F64, cuda)
        xp, x0 = blank(bsz, n, F32K, cuda), blank(bsz, n, F32K, cuda)
        arr = (C.c_float * 10)(*coef)
        ok(L().mudg_ddim_step(bufs["x"].ptr, bufs["e_c"].ptr, bufs["e_u"].ptr if ways > 1 else None, bufs["e_m"].ptr if ways > 2 else None,
                              bufs["nz"].ptr if noise else None, xp.ptr, x0.ptr, bsz, n, arr, ws.ptr, _s()), "ddim_step")
        name = f"ddim_step n={n} {'eps' if eps_form else 'v'}-prediction {ways}-way phi={phi} noise={int(noise)}"
        w_prev, w_x0, ratio, mag0, mag = N.ddim_step(x, e_c, e_u if ways > 1 else None, e_m if ways > 2 else None, nz if noise else None, coef)
        ws.read(name + ": ws")
        g_prev, g_x0 = value(xp, name + " x_prev"), value(x0, name + " pred_x0")
        r0 = float(((g_x0 - w_x0).abs() / (1e-6 * mag0)).max())
        r1 = float(((g_prev - w_prev).abs() / (8.0 * U * mag)).max())
        worst0, worst = max(worst0, r0), max(worst, r1)
        assert r0 <= 1.0, (name, "pred_x0: largest |error| / (1e-6 sum |terms|)", r0, "ratios", ratio.tolist())
        assert r1 <= 1.0, (name, "x_prev: largest |error| / (8 U sum |terms|)", r1)
    for b in bufs.values():
        b.read("ddim_step: an input")
    print(f"[norm {MODE}] ddim_step n={n}: largest |error| / bound: pred_x0 {worst0:.3f}, x_prev {worst:.3f}")


# ================================================================================================ refusals
def test_refusals_write_nothing(cuda):
    """Every MUDG_REQUIRE of these entry points that no other test triggers: MUDG_EINVAL, and the result buffers still hold NaN."""
    lib = L()
    x, xv = rows_in(rnd(8, 64, seed=150), OPER, cuda)
    xf = holding([rnd(8, 64, seed=151)], F32K, cuda)
    gam, bet = vec_f32(torch.ones(4096), cuda), vec_f32(torch.zeros(4096), cuda)
    gam1 = vec_f32(torch.ones(64), cuda, off=1)
    y = blank(8, 64, OPER, cuda)
    ws = flat_blank(4096, F32, cuda)
    pf = holding([torch.zeros(8, 128)], F32K, cuda)
    outf = blank(8, 64, F32K, cuda)
    i64 = torch.zeros(3, dtype=torch.int64, device=cuda)
    wsd = flat_blank(lib.mudg_ddim_ws_doubles(1), F64, cuda)
    coef = (C.c_float * 10)(*([1.0] * 10))
    s, P = _s(), PLANES
    gn = lambda **k: lib.mudg_groupnorm(*[k.get(n_, d) for n_, d in (("X", x.ptr), ("X2", None), ("csplit", 0), ("ldx", x.ld), ("ldx2", 0), ("kind", 0),
                                        ("gamma", gam.ptr), ("beta", bet.ptr), ("Y", y.ptr), ("ldy", y.ld), ("samples", 1), ("rows", 8), ("C", 64),
                                        ("groups", 32), ("eps", 1e-5), ("silu", 0), ("ws", ws.ptr), ("s", s))])
    fr = lambda **k: lib.mudg_groupnorm_fused_rows(*[k.get(n_, d) for n_, d in (("X", x.ptr), ("X2", None), ("csplit", 0), ("ldx", x.ld), ("ldx2", 0),
                                                   ("kind", 0), ("gamma", gam.ptr), ("beta", bet.ptr), ("Y", y.ptr), ("ldy", y.ld), ("samples", 1),
                                                   ("rows", 128), ("C", 64), ("groups", 32), ("eps", 1e-5), ("silu", 0), ("P1", pf.ptr), ("h1", 128),
                                                   ("P2", None), ("h2", 128), ("ws", ws.ptr), ("s", s))])
    ln = lambda **k: lib.mudg_layernorm(*[k.get(n_, d) for n_, d in (("X", x.ptr), ("ldx", x.ld), ("kind", 0), ("gamma", gam.ptr), ("beta", bet.ptr),
                                        ("Y", y.ptr), ("ldy", y.ld), ("rows", 8), ("C", 64), ("eps", 1e-5), ("s", s))])
    calls = {
        "groupnorm: null ws": lambda: gn(ws=None),
        "groupnorm: rows 0": lambda: gn(rows=0),
        "groupnorm: C % groups": lambda: gn(groups=24),
        "groupnorm: C % 8": lambda: gn(C=60, groups=4),
        "groupnorm: C > 4096": lambda: gn(C=4104, groups=8),
        "groupnorm: groups > 256": lambda: gn(C=4096, groups=512),
        "groupnorm: kind 3": lambda: gn(kind=3),
        "groupnorm: ldx % 8": lambda: gn(ldx=x.ld + P),
        "groupnorm: ldy % 8": lambda: gn(ldy=y.ld + P),
        "groupnorm: X off 16 bytes": lambda: gn(X=x.ptr + 2),
        "groupnorm: ldy < C": lambda: gn(ldy=56 * P),
        "groupnorm: samples > 65535": lambda: gn(samples=65536),
        "groupnorm: csplit % 8": lambda: gn(X2=x.ptr, csplit=12, ldx2=x.ld),
        "groupnorm: csplit = C": lambda: gn(X2=x.ptr, csplit=64, ldx2=x.ld),
        "groupnorm_fused_rows: null P1": lambda: fr(P1=None),
        "groupnorm_fused_rows: block height 100": lambda: fr(h1=100),
        "groupnorm_fused_rows: second block height 64": lambda: fr(X2=x.ptr, csplit=32, ldx2=x.ld, P2=pf.ptr, h2=64),
        "groupnorm_fused_rows: rows % height": lambda: fr(rows=192),
        "groupnorm_fused_rows: X2 without P2": lambda: fr(X2=x.ptr, csplit=32, ldx2=x.ld),
        "groupnorm_fused_rows: kind 3": lambda: fr(kind=3),
        "layernorm: null beta": lambda: ln(beta=None),
        "layernorm: C % 8": lambda: ln(C=60),
        "layernorm: C > 4096": lambda: ln(C=4104),
        "layernorm: kind -1": lambda: ln(kind=-1),
        "layernorm: gamma off 16 bytes": lambda: ln(gamma=gam1.ptr),
        "layernorm: ldy < C": lambda: ln(ldy=56 * P),
        "layernorm: ldx % 8": lambda: ln(ldx=x.ld + P),
        "softmax_rows: ldp < cols": lambda: lib.mudg_softmax_rows(xf.ptr, 64, y.ptr, 56 * P, 8, 64, s),
        "softmax_rows: cols 0": lambda: lib.mudg_softmax_rows(xf.ptr, 64, y.ptr, y.ld, 8, 0, s),
        "timestep_embedding: dim 1": lambda: lib.mudg_timestep_embedding(i64.data_ptr(), gam.ptr, outf.ptr, 3, 1, s),
        "small_linear: K 0": lambda: lib.mudg_small_linear(xf.ptr, xf.ptr, 0, None, outf.ptr, 1, 8, 0, 0, 0, 0, s),
        "small_linear: M > 65535": lambda: lib.mudg_small_linear(xf.ptr, xf.ptr, 0, None, outf.ptr, 65536, 8, 8, 0, 0, 0, s),
        "ncthw_to_rows: coff + C > ld": lambda: lib.mudg_ncthw_to_rows(xf.ptr, 1, y.ptr, 1, 8, 1, 8, y.ld, 60, 0, 0, s),
        "ncthw_to_rows: window outside": lambda: lib.mudg_ncthw_to_rows(xf.ptr, 1, y.ptr, 1, 8, 2, 4, y.ld, 0, 3, 2, s),
        "rows_to_ncthw: window outside": lambda: lib.mudg_rows_to_ncthw(x.ptr, 0, x.ld, 0, outf.ptr, 1, 1, 8, 2, 4, 1.0, 3, -1, s),
        "rows_to_ncthw: coff + C > ld": lambda: lib.mudg_rows_to_ncthw(x.ptr, 0, x.ld, 60, outf.ptr, 1, 1, 8, 1, 8, 1.0, 0, 0, s),
        "zero_channels: c1 <= c0": lambda: lib.mudg_zero_channels(y.ptr, 8, y.ld, 8, 8, s),
        "zero_channels: c1 > ld": lambda: lib.mudg_zero_channels(y.ptr, 8, y.ld, 0, 80, s),
        "cast_rows: kind 3": lambda: lib.mudg_cast_rows(xf.ptr, 3, 64, y.ptr, 0, y.ld, 8, 64, s),
        "cast_rows: lds < cols": lambda: lib.mudg_cast_rows(xf.ptr, 1, 56, y.ptr, 0, y.ld, 8, 64, s),
        "cast_rows: ldd < cols": lambda: lib.mudg_cast_rows(xf.ptr, 1, 64, outf.ptr, 1, 56, 8, 64, s),
        "copy_rows: ldd < cols": lambda: lib.mudg_copy_rows(x.ptr, x.ld, y.ptr, 56 * P, 8, 64, s),
        "cast_f32_bf16: source off 16 bytes": lambda: lib.mudg_cast_f32_bf16(xf.ptr + 4, y.ptr, 64, s),
        "axpy: n 0": lambda: lib.mudg_axpy_f32(outf.ptr, xf.ptr, 0, 1.0, s),
        "lincomb: B 0": lambda: lib.mudg_lincomb(outf.ptr, xf.ptr, xf.ptr, gam.ptr, bet.ptr, 0, 8, s),
        "gaussian_sample: HW 0": lambda: lib.mudg_gaussian_sample(xf.ptr, None, outf.ptr, 1, 4, 0, 1.0, s),
        "ddim_step: n 1": lambda: lib.mudg_ddim_step(xf.ptr, xf.ptr, None, None, None, outf.ptr, outf.ptr, 1, 1, coef, wsd.ptr, s),
        "ddim_step: e_m without e_u": lambda: lib.mudg_ddim_step(xf.ptr, xf.ptr, None, xf.ptr, None, outf.ptr, outf.ptr, 1, 64, coef, wsd.ptr, s),
        "ddim_step: null ws": lambda: lib.mudg_ddim_step(xf.ptr, xf.ptr, None, None, None, outf.ptr, outf.ptr, 1, 64, coef, None, s),
    }
    for name, call in calls.items():
        rc = call()
        assert rc == EINVAL, (name, rc)
        assert lib.mudg_last_error(), name
    torch.cuda.synchronize()
    for name, b in (("Y", y), ("ws", ws), ("fp32 out", outf), ("ddim ws", wsd)):
        got = b.read("refusals: " + name)
        assert all(bool(torch.isnan(t.float()).all()) for t in got), f"a refused call wrote to {name}"
