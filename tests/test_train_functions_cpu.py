"""The condition the exact cases of tests/test_train_functions_gpu.py rest on, checked before a GPU is involved: every operand of
every exact case is an integer of magnitude <= 3 (exact in bf16 and fp16, one piece of a split operand), and every reference value and
gradient is an integer below 2^24, which the fp32 accumulators and every fp32 partial sum hold exactly.  Also: the tables reach the
branches of mudg_amd/train/functions.py they name (the parts of that decided without a GPU)."""
import pytest
import torch

import train_functions_cases as C
from mudg_amd.train import functions as Fn

LIMIT = 2 ** 24


@pytest.fixture(scope="module")
def largest():
    return {}


@pytest.mark.parametrize("fam,i", C.EXACT_IDS)
def test_exact_cases_have_integer_operands_and_integer_results_below_2_to_24(fam, i, largest):
    cases, problem, ref_of, _, _, positions, tied = C.FAMILIES[fam]
    tensors, dy = problem(cases[i], C.int_make)
    for name, t in {**tensors, "dy": dy}.items():
        assert t.dtype == torch.float32 and C.is_integer_valued(t, 3.5), (fam, i, name)
    assert set(tensors) <= {p for p in positions if p}
    y, grads = C.reference(ref_of(cases[i]), tensors, dy)
    assert set(grads) == set(tensors)
    for name, t in {"y": y, **grads}.items():
        assert C.is_integer_valued(t, LIMIT), (fam, i, name, float(t.abs().max()))
        assert t.shape == (y.shape if name == "y" else tensors[name].shape)
    largest[(fam, i)] = max(float(t.abs().max()) for t in (y, *grads.values()))
    print(f"{fam} case {i}: largest magnitude {largest[(fam, i)]:.0f}")
    subsets = C.needs_subsets(tensors, tied)
    main = [k for k in C.MAIN if k in tensors]
    side = [k for k in C.SIDE if k in tensors and k not in tied]
    assert len(subsets) == 2 ** len(main) - 1 + len(side) and subsets[0] == frozenset(main) | frozenset(side)


def test_no_exact_case_exceeds_the_bound_derived_by_hand():
    """9 per product, 6144 positions in the longest contraction (the 48 x 64 conv over two frames)."""
    worst = 0.0
    for fam, i in C.EXACT_IDS:
        cases, problem, ref_of = C.FAMILIES[fam][:3]
        tensors, dy = problem(cases[i], C.int_make)
        y, grads = C.reference(ref_of(cases[i]), tensors, dy)
        worst = max(worst, *(float(t.abs().max()) for t in (y, *grads.values())))
    assert worst <= 9 * 6144 < LIMIT


def test_the_tables_reach_the_slicing_rules_they_name():
    m, k, n = C.LINEAR_CASES[6][:3]
    assert Fn._splits(n, k, m) > 1 and k % 64                                  # K-slices on the transposed route
    assert Fn._splits(C.LINEAR_CASES[2][2], C.LINEAR_CASES[2][1], C.LINEAR_CASES[2][0]) == 1
    assert Fn._width(n, k, m) % (Fn._splits(n, k, m) * 64) == 0 and Fn._width(n, k, m) >= m
    assert all(case[1] % 8 == 0 for case in C.LINEAR_CASES)
    assert C.LINEAR_CASES[3][2] % 8 and C.CONV_CASES[3][5] % 8 and C.CONV_CASES[0][4] % 8          # padded dy, padded Cout, padded Cin
    assert C.conv_rows_per_group(C.CONV_CASES[6]) == 6144 == 1024 * 6 and C.conv_rows_per_group(C.CONV_CASES[5]) == 1536
    assert C.LINEAR_CASES[4][0] == 16 * 64 + 6
    assert C.TCONV_CASES[2][1] == 1
