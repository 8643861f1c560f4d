"""The stream kernel (csrc/sgemm.hip: K = 320 and N = 320 or 640, W resident in registers, rows streamed through LDS by persistent workgroups) through
the C-ABI, with the descriptors, buffers and fp64 definitions of tests/test_gemm_kernels_gpu.py and tests/gemm_reference.py.

Which kernel runs a launch is asked of the library (mudg_gemm_stream_ok) and asserted, case by case.  Three processes:

  this one      the shipped bf16 library: the selection rule (a 288-row frame hint with K = 320 and N = 320 or 640 runs the kernel, within the bound the
                bounded K-loop tests of test_gemm_kernels_gpu.py apply; a problem with `stats` and one with N = 960 do not, and give the
                bits the debug-variants library gives with MUDG_GEMM_STREAM=0).
  child "dbg"   the debug-variants library, where MUDG_GEMM_STREAM is read at every call: = 2 for ragged M (exact against fp64, nothing
                written outside the result), = 1 against = 0 for the bit-identity with wgemm_kernel, batch independence, repeatability.
  child "fp16"  the shipped fp16 library: exact cases and bit-identity at M = 288 x 7 by the rule; the 288-row tile's side of the comparison
                is the same problem with `stats` asked for, which the rule leaves on wgemm_kernel.

TR is the kernel's tile height (csrc/gemm_shared.h, SBM) and CU its grid: one workgroup per compute unit, whole XCDs."""
import ctypes as C
import os
import sys

import pytest
import torch

import gemm_reference as R
from mudg_amd import hip
from sentinel_buffers import Buf
from test_gemm_kernels_gpu import (Call, G, assert_same, check_16bit, exact_operands, exact_value, exactness, kind_dtype, random_operands,
                                   value_of)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLE = os.environ.get("MUDG_STREAM_CHILD", "")
THIS = "tests/test_gemm_stream_gpu.py"
F64 = torch.float64
OPER, F16K = R.KIND_OPERAND, R.KIND_F16
TR = 64

# every epilogue the kernel has: bias or none, a residual of either 16-bit kind or none, both kinds of Y
EPILOGUES = {
    "plain_operand": dict(out=OPER),
    "bias_stream": dict(bias=True, out=F16K),
    "bias_res16_operand": dict(bias=True, res=F16K, out=OPER),
    "bias_res16_stream": dict(bias=True, res=F16K, out=F16K),
    "resoperand_stream": dict(res=OPER, out=F16K),
}
# row strides wider than the logical width (column slices of wider matrices are what the UNet passes), 16-byte rows
WIDE = dict(xgap=320, ypad=648, rpad=328)


def cu_count():
    n = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return max(n, 8) & ~7


def ragged_ms():
    cu = cu_count()
    return {"one_row": 1, "tile_minus_1": TR - 1, "tile_plus_1": TR + 1, "m288": 288, "m288_plus_17": 288 + 17,
            "one_workgroup_idle": TR * (cu - 1), "uneven_ranges": TR * (cu + 3), "two_tiles_each_plus_5": TR * 2 * cu + 5,
            "five_tiles_each_plus_3": TR * 5 * cu + 3}       # (the last: every slot of the three-tile ring is used twice)


def case(name, m, epi, hint=0, n=320, **kw):
    """K = 320; N = 320, or 640: two column slices, each with its own workgroups."""
    return G(name, m, n, 320, "stream kernel", hint=hint, **dict(WIDE, **EPILOGUES[epi], **kw))


def stream_runs(call):
    return hip.lib().mudg_gemm_stream_ok(C.byref(call.d))


def raw(buf):
    """Every byte of a 16-bit buffer, sentinel included."""
    return buf.dev.cpu().view(torch.int16)


def exact_call(c, dev, seed=1):
    bits, unit = exactness(c, 1, seed)
    assert bits < 2 ** 24, (c["name"], bits)
    xs, ws, bias, gb, res = exact_operands(c, 1, seed)
    want = exact_value(c, xs, ws, bias, gb, res, 1)
    return Call(c, xs, ws, bias, gb, res, dev), want


def check_exact(c, call, want):
    got = call.run()                                    # (asserts that nothing outside the view of Y was written)
    for g, w in zip(got, R.store_pieces(want, c["out"], hip.operand_dtype(), 1)):
        assert_same(c, "Y", g, w)


if ROLE == "dbg":
    def switch(v):
        os.environ["MUDG_GEMM_STREAM"] = str(v)

    @pytest.mark.parametrize("epi", list(EPILOGUES))
    @pytest.mark.parametrize("mname", ["one_row", "tile_minus_1", "tile_plus_1", "m288", "m288_plus_17", "one_workgroup_idle", "uneven_ranges",
                                       "two_tiles_each_plus_5", "five_tiles_each_plus_3"])
    def test_stream_exact_at_ragged_m(cuda, mname, epi):
        """Small-integer operands, weights, bias and residual (|sum| <= 9 x 320 + 12: exact in fp32 in any order): the result is the ONE
        rounding of the fp64 value.  No frame hint: only MUDG_GEMM_STREAM=2 sends these to the kernel."""
        switch(2)
        c = case(f"{mname}_{epi}", ragged_ms()[mname], epi)
        call, want = exact_call(c, cuda, seed=3)
        assert stream_runs(call) == 1
        check_exact(c, call, want)

    @pytest.mark.parametrize("epi", ["plain_operand", "bias_res16_stream"])
    @pytest.mark.parametrize("mname", ["one_row", "tile_plus_1", "m288_plus_17", "one_workgroup_idle", "uneven_ranges", "five_tiles_each_plus_3"])
    def test_stream_exact_at_ragged_m_two_slices(cuda, mname, epi):
        """N = 640: half the workgroups per slice, so the same M give other ranges (and idle workgroups in both slices)."""
        switch(2)
        m = {"one_workgroup_idle": TR * (cu_count() // 2 - 1), "uneven_ranges": TR * (cu_count() // 2 + 3)}.get(mname) or ragged_ms()[mname]
        c = case(f"n640_{mname}_{epi}", m, epi, n=640)
        call, want = exact_call(c, cuda, seed=6)
        assert stream_runs(call) == 1
        check_exact(c, call, want)

    @pytest.mark.parametrize("mname", ["one_row", "tile_minus_1", "tile_plus_1", "m288_plus_17", "uneven_ranges", "two_tiles_each_plus_5"])
    def test_stream_writes_nothing_outside_the_result(cuda, mname):
        """Y as a view inside a NaN-filled buffer: row stride > N, and more than two whole tiles of rows behind row M - 1 (the rows a ragged
        last tile, and the tiles requested ahead of a range's end, would touch)."""
        switch(2)
        c = case(f"sentinel_{mname}", ragged_ms()[mname], "bias_res16_stream")
        call, want = exact_call(c, cuda, seed=4)
        call.y = Buf(1, c["M"], 320, 968, kind_dtype(c["out"]), tail_rows=2 * TR + 9).blank(cuda)
        call.d.Y, call.d.ldy = call.y.ptr, 968
        assert stream_runs(call) == 1
        check_exact(c, call, want)

    @pytest.fixture(scope="module")
    def random_by_m():
        made = {}

        def get(m, n=320):
            if (m, n) not in made:
                made[m, n] = random_operands(case("r", m, "bias_res16_stream", n=n), seed=500 + m % 97 + n)
            return made[m, n]
        return get

    def random_call(c, ops, dev):
        xs, ws, bias, res = ops
        if c.get("res") == OPER:
            res = [res[0].to(hip.operand_dtype()).float()]
        return Call(c, xs, ws, bias if c.get("bias") else None, None, res if c.get("res") is not None else None, dev)

    @pytest.mark.parametrize("n,epi", [(320, e) for e in EPILOGUES] + [(640, "plain_operand"), (640, "bias_res16_stream")])
    @pytest.mark.parametrize("tiles", ["1", "7", "cu_plus_3"])
    def test_stream_is_bit_identical_to_the_288_row_tile(cuda, random_by_m, tiles, n, epi):
        """Random operands, the frame hint 288: MUDG_GEMM_STREAM=1 (the rule: this kernel) against = 0 (wgemm_kernel), every byte of Y's buffer."""
        m = 288 * (cu_count() + 3 if tiles == "cu_plus_3" else int(tiles))
        c = case(f"bits_m{m}_n{n}_{epi}", m, epi, hint=288, n=n)
        out = []
        for sw, ran in ((1, 1), (0, 0)):
            switch(sw)
            call = random_call(c, random_by_m(m, n), cuda)
            assert stream_runs(call) == ran
            call.run()
            out.append(raw(call.y))
        assert torch.equal(out[0], out[1]), (c["name"], int((out[0] != out[1]).sum()))

    def test_stream_rows_do_not_depend_on_the_batch(cuda, random_by_m):
        """Two problems of 288 x 4 rows in one launch and one by one."""
        switch(1)
        m = 288 * 4
        xs, ws, bias, res = random_by_m(2 * m)
        c2 = case("stacked", 2 * m, "bias_res16_stream", hint=288)
        both = random_call(c2, (xs, ws, bias, res), cuda)
        assert stream_runs(both) == 1
        y2 = both.run()[0]
        for h in range(2):
            part = ([x[:, h * m:(h + 1) * m] for x in xs], ws, bias, [r[:, h * m:(h + 1) * m] for r in res])
            one = random_call(case(f"half{h}", m, "bias_res16_stream", hint=288), part, cuda)
            assert stream_runs(one) == 1
            assert torch.equal(one.run()[0].view(torch.int16), y2[:, h * m:(h + 1) * m].contiguous().view(torch.int16)), h

    def test_stream_is_repeatable(cuda, random_by_m):
        """The same launch five times (four to five tiles per workgroup: counted waits, ring slots and the residual area reused)."""
        switch(1)
        m = 288 * (cu_count() + 3)
        call = random_call(case("repeat", m, "bias_res16_operand", hint=288), random_by_m(m), cuda)
        assert stream_runs(call) == 1
        first = None
        for i in range(5):
            call.run()
            bits = raw(call.y)
            first = bits if first is None else first
            assert torch.equal(bits, first), i

    def test_dump_what_the_rule_leaves_alone(cuda):
        """For this module's own process (MUDG_STREAM_DUMP): the problems the rule does not take, as MUDG_GEMM_STREAM=0 computes them."""
        switch(0)
        for name, call in rule_leaves_alone(cuda).items():
            assert stream_runs(call) == 0
            call.run()
            torch.save({"y": raw(call.y), "stats": None if call.stats is None else call.stats.dev.cpu()},
                       os.path.join(os.environ["MUDG_STREAM_DUMP"], name + ".pt"))


def rule_leaves_alone(dev):
    """A problem with GroupNorm partials and one with N = 960, both with the 288-row frame hint and K = 320."""
    calls = {}
    for name, c in (("stats", case("rule_stats", 288 * 3, "bias_res16_stream", hint=288, stats=True)),
                    ("n960", G("rule_n960", 288 * 3, 960, 320, "three column tiles", hint=288, bias=True, res=F16K, out=OPER, **WIDE))):
        xs, ws, bias, res = random_operands(c, seed=77)
        calls[name] = Call(c, xs, ws, bias, None, res, dev)
    return calls


if ROLE == "fp16":
    FP16_CASES = [(320, e) for e in EPILOGUES] + [(640, "plain_operand")]

    @pytest.mark.parametrize("n,epi", FP16_CASES)
    def test_stream_exact_in_the_fp16_build(cuda, n, epi):
        c = case(f"fp16_exact_n{n}_{epi}", 288 * 7, epi, hint=288, n=n)
        call, want = exact_call(c, cuda, seed=5)
        assert stream_runs(call) == 1
        check_exact(c, call, want)

    @pytest.mark.parametrize("n,epi", FP16_CASES)
    def test_stream_is_bit_identical_to_the_288_row_tile_in_the_fp16_build(cuda, n, epi):
        """The shipped library has no switch: the same problem with `stats` asked for stays on wgemm_kernel."""
        ops = random_operands(case("r", 288 * 7, "bias_res16_stream", n=n), seed=600)
        out = []
        for stats, ran in ((False, 1), (True, 0)):
            c = case(f"fp16_bits_n{n}_{epi}", 288 * 7, epi, hint=288, n=n, stats=stats)
            xs, ws, bias, res = ops
            if c.get("res") == OPER:
                res = [res[0].to(hip.operand_dtype()).float()]
            call = Call(c, xs, ws, bias if c.get("bias") else None, None, res if c.get("res") is not None else None, cuda)
            assert stream_runs(call) == ran
            call.run()
            out.append(raw(call.y))
        assert torch.equal(out[0], out[1]), (epi, int((out[0] != out[1]).sum()))


if ROLE == "" and hip.planes() == 1:                # (the kernel belongs to the 16-bit builds)
    @pytest.fixture(scope="module")
    def children(tmp_path_factory):
        from helpers import ChildRuns
        dump = str(tmp_path_factory.mktemp("stream_dump"))
        runs = ChildRuns(workers=2)
        cmd = [sys.executable, "-m", "pytest", THIS, "-m", "gpu", "-q", "-p", "no:cacheprovider"]
        env = {k: v for k, v in os.environ.items() if not k.startswith("MUDG_GEMM_")}
        runs.submit("dbg", cmd, ROOT, dict(env, MUDG_STREAM_CHILD="dbg", MUDG_DEBUG_VARIANTS="1", MUDG_OPERAND="bf16", MUDG_STREAM_DUMP=dump), 900)
        runs.submit("fp16", cmd, ROOT, dict(env, MUDG_STREAM_CHILD="fp16", MUDG_OPERAND="fp16"), 900)
        runs.dump = dump
        yield runs
        runs.shutdown()

    def _child(children, key):
        rc, stdout = children.result(key)
        print("\n".join(l for l in stdout.splitlines() if "passed" in l or "failed" in l or l.startswith("[child")))
        assert rc == 0, stdout[-6000:]

    def test_stream_kernel_in_the_debug_variants_library(cuda, children):
        """Exact at ragged M, nothing written outside Y, bit-identity with wgemm_kernel, batch independence, repeatability (child "dbg")."""
        _child(children, "dbg")

    def test_stream_kernel_in_the_fp16_build(cuda, children):
        _child(children, "fp16")

    def test_rule_runs_the_stream_kernel_on_whole_frames(cuda):
        """The shipped library, a 288-row frame hint, N = K = 320: the kernel runs, and random operands come out within the bound of the
        bounded linear cases of test_gemm_kernels_gpu.py (check_16bit: every element on a storage neighbour of the fp64 value, at most
        FLIP_CAP of a 32 x 64 block off the nearest) — for both kinds of Y."""
        for n, epi in ((320, "bias_res16_operand"), (320, "bias_res16_stream"), (640, "bias_res16_stream")):
            c = case(f"rule_n{n}_{epi}", 288 * 3, epi, hint=288, n=n)
            xs, ws, bias, res = random_operands(c, seed=78)
            call = Call(c, xs, ws, bias, None, res, cuda)
            assert stream_runs(call) == 1
            check_16bit(c["name"], call.run()[0], value_of(c, xs, ws, bias, res, F64))
        assert stream_runs(exact_call(case("rule_no_hint", 288 * 3, "plain_operand"), cuda)[0]) == 0          # no frame hint: not the rule's

    def test_rule_leaves_stats_and_other_widths_where_they_were(cuda, children):
        """A problem with `stats` and one with N = 960 do not run the kernel and give, bit for bit, what the debug-variants library gives
        with MUDG_GEMM_STREAM=0."""
        _child(children, "dbg")
        for name, call in rule_leaves_alone(cuda).items():
            assert stream_runs(call) == 0
            call.run()
            want = torch.load(os.path.join(children.dump, name + ".pt"))
            assert torch.equal(raw(call.y), want["y"]), name
            if want["stats"] is not None:
                assert torch.equal(call.stats.dev.cpu().view(torch.int32), want["stats"].view(torch.int32)), name
