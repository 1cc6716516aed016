"""The exact MLP problems of tests/test_mlp_exact_gpu.py, checked without a GPU: every shape that file uses must satisfy the
conditions that make an exact comparison meaningful (tests/mlp_exact_cases.py: exactness in bf16 and fp16, the 2^24 sum
bound, every batch row and every 16x16 tile counts, no all-zero output row) and must tell the classic kernel mistakes apart
from the right answer; a deliberately bad recipe must be rejected by those same checks."""
import numpy as np
import pytest

import mlp_exact_cases as cases


def _group(key):
    out = {}
    for c in cases.all_mlp_cases():
        out.setdefault(key(c), []).append(c)
    return out


_BY_NET = _group(lambda c: (c[1], c[2]))


@pytest.mark.parametrize("hidden,nhm", sorted(_BY_NET))
def test_every_gpu_shape_meets_the_conditions(hidden, nhm):
    for args in _BY_NET[(hidden, nhm)]:
        c = cases.get_case(*args)  # (asserts check_conditions)
        assert c.B == args[3] and (c.in_dim, c.hidden, c.nhm) == (args[0], hidden, nhm)
        cases.check_discrimination(c)
        assert max(np.abs(t).max() for t in c.compared().values()) <= cases.VALUE_LIMIT


def test_gpu_file_uses_only_listed_shapes():
    """The GPU file takes its problems from get_case with the lists of mlp_exact_cases: the batches that depend on the CU
    count are periodic, so the conditions of one CU count are those of any other except the sum bound, which get_case asserts
    again on the device's own count."""
    for cus in (64, 256, 304):
        i, h, n, B = cases.stride_cases(cus)["wide_lds_forward"]
        assert B > 256 * cus
        cases.get_case(i, h, n, B, cases.ACT_RELU)


def test_gemm_chain_problem_keeps_weight_gradients_in_16_bits():
    """The library-GEMM chain's autograd stores dW in the element type: its problem must keep every dW a bf16 integer."""
    i, o, h, layers, B = cases.MODULE_CHAIN
    c = cases.get_case(i, h, layers - 1, B, cases.ACT_RELU, o)
    assert np.abs(c.flat_dW()).max() <= cases.VALUE_LIMIT


def test_periodic_batches_reach_the_second_grid_stride_iteration():
    s = cases.stride_cases()
    assert s["narrow_backward"][3] > 512 * 128 and s["narrow_forward"][3] > 2048 * 256 and s["wide"][3] > 4096 * 256
    for i, h, n, B in s.values():
        c = cases.get_case(i, h, n, B, cases.ACT_RELU)
        assert c.P == cases.PERIOD and c.B == B and np.gcd(cases.PERIOD, 256) == 1
        assert c.cnt.sum() == B and c.cnt.min() >= B // cases.PERIOD


def test_bad_recipe_is_rejected():
    """Signed sparse hidden matrices in a 14-deep ReLU net: half of the surviving units die in every layer, the net is all
    zero long before its output, and the condition checks must say so."""
    c = cases.build_case(48, 64, 14, 65, cases.ACT_RELU, recipe="signed_sparse_hidden")
    assert not np.any(c.y) and not np.any(c.fb[-1])
    with pytest.raises(AssertionError, match="every batch row counts|every tile counts"):
        cases.check_conditions(c)
    # the same shape with the recipe of the GPU file passes
    cases.check_conditions(cases.build_case(48, 64, 14, 65, cases.ACT_RELU))


def test_conditions_catch_inexact_and_oversized_problems():
    c = cases.build_case(32, 64, 1, 65, cases.ACT_RELU)
    cases.check_conditions(c)
    big = cases.build_case(32, 64, 1, 65, cases.ACT_RELU, lo=-40, hi=40)
    with pytest.raises(AssertionError, match="exactness"):
        cases.check_conditions(big)
    c.cnt = c.cnt * 2.0 ** 20  # the same rows a million times over: sums of |terms| past 2^24
    with pytest.raises(AssertionError, match="dW sum bound"):
        cases.check_conditions(c)


@pytest.mark.parametrize("B", (cases.WGRAD_B,) + cases.WGRAD_EDGE_BATCHES)
def test_wgrad_problems_meet_the_conditions(B):
    c = cases.get_wgrad_case(B)  # (asserts its conditions for every (M, N) the GPU file uses at this batch)
    assert np.abs(c.dW).max() < cases.SUM_LIMIT and np.array_equal(c.dW, np.round(c.dW))
