"""The premises of the exact cases of tests/test_gpu_eval.py, on the CPU.  The argument is that of
tests/test_gpu_num_diff.py::test_exact_dyadic_accumulate, restated for ROWS: with data, x and h = 2^-6 all multiples of 1/8 (1/64),
every product, partial sum and difference of the linear bodies is a dyadic rational of fewer than 24 bits, so it is exact in fp32
and in fp64, the order of the additions does not matter, a fused multiply-add rounds nothing that a multiply and an add would
not, and the device's rows must equal exact rational arithmetic bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_reference as er  # noqa: E402
import num_diff_reference as nd  # noqa: E402


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,kR,items", er.SHAPES)
def test_rows_of_the_exact_cases_are_exact_in_the_test_dtype(n, kR, items, dtype):
    data, x = er.dyadic_case(n, kR, items)
    for squared, fwd in ((False, None), (True, None), (True, er.H6)):
        r, J, units = er.linear_rows_exact(data, x, n, squared, fwd)
        assert units < 2 ** 24, "a partial sum leaves 24 bits"
        # float64 arithmetic is the exact arithmetic (what the GPU tests compare with), and so is the test dtype's
        r64, J64 = er.linear_rows(data, x, n, np.float64, squared, fwd)
        assert np.array_equal(r64, er.as_dtype(r, np.float64)) and np.array_equal(J64, er.as_dtype(J, np.float64))
        rt, Jt = er.linear_rows(data, x, n, dtype, squared, fwd)
        assert rt.dtype == dtype and Jt.dtype == dtype
        assert np.array_equal(rt, er.as_dtype(r, dtype)) and np.array_equal(Jt, er.as_dtype(J, dtype))
        assert np.array_equal(rt.astype(np.float64), r64) and np.array_equal(Jt.astype(np.float64), J64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,kR,items", er.SHAPES)
def test_finite_differences_of_the_exact_cases_are_exact(n, kR, items, dtype):
    """NumEval restated in the test dtype (num_diff_reference) reads the exact Jacobian off the linear body with central and fast
    central differences, and J + h in column 0 of the squared variant with forward differences."""
    data, x = er.dyadic_case(n, kR, items)
    for method, squared, fwd in ((nd.CENTRAL, False, None), (nd.FAST_CENTRAL, False, None), (nd.FORWARD, True, er.H6)):
        r, J, _ = er.linear_rows_exact(data, x, n, squared, fwd)
        rn, Jn = er.numeric_rows(data, x, n, dtype, method, squared)
        assert rn.dtype == dtype and Jn.dtype == dtype
        assert np.array_equal(rn, er.as_dtype(r, dtype)) and np.array_equal(Jn, er.as_dtype(J, dtype))


def test_the_batch_scale_cases_are_exact():
    """P = 5 000 x 5 items at n = 3, one problem of 20 000 items at n = 6, and the shapes of
    test_waves_run_several_units_and_several_super_steps as they come out on 256 compute units: float64 rows cast to fp32 lose
    nothing (the generator and the bounds do not depend on P or on the number of items)."""
    for n, items, P in ((3, 5, 5000), (6, 20000, 1), (3, 5, 18435), (3, 64 * 18432 + 3, 1), (6, 761, 8193), (3, 130, 32773)):
        data, x = er.dyadic_case(n, 1, items, P=P)
        r64, J64 = er.linear_rows(data, x, n, np.float64)
        r32, J32 = er.linear_rows(data, x, n, np.float32)
        assert np.array_equal(r32.astype(np.float64), r64) and np.array_equal(J32.astype(np.float64), J64)
        assert np.abs(r64).max() * 64 < 2 ** 24 and (r64 * 64 == np.rint(r64 * 64)).all()
