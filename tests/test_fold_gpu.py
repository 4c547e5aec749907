"""The fixed-order float64 fold of csrc/gsr_fold.h, bit for bit against tests/fold_model.py, through the
private hook gsr_debug_fold: block_fold_store<3, 4, tree> and k_fold_partials<64 or 256> and nothing else.  Every registration
method's sums pass through these two functions; their own tests pin only that two runs agree."""
import numpy as np
import pytest

import fold_model as F

pytestmark = pytest.mark.gpu


def _bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def _device_fold(hip_lib, x, order, final_threads):
    x = np.ascontiguousarray(x, np.float64)
    out = np.full(3, 123.0)
    rc = hip_lib.gsr_debug_fold(x.ctypes.data, len(x), order, final_threads, out.ctypes.data, 0)
    assert rc == 0, hip_lib.gsr_last_error()
    return out


CASES = [(n, 64) for n in F.SIZES] + [(n, 256) for n in F.SIZES_256]


@pytest.mark.parametrize("order", [F.XOR, F.ROWS], ids=["xor", "rows"])
@pytest.mark.parametrize("n,final_threads", CASES)
def test_fold_has_the_bits_of_the_model(hip_lib, n, final_threads, order):
    x = F.seeded_rows(n)
    assert np.array_equal(_bits(_device_fold(hip_lib, x, order, final_threads)), _bits(F.fold(x, order, final_threads)))


@pytest.mark.parametrize("order", [F.XOR, F.ROWS], ids=["xor", "rows"])
@pytest.mark.parametrize("final_threads", [64, 256])
def test_fold_of_minus_zero_and_of_a_nan_row(hip_lib, final_threads, order):
    for n in (64, 256, 300):                # a wave and a block of -0.0 alone; a block with +0.0 rows past n beside them
        x = np.full((n, 3), -0.0)
        assert np.array_equal(_bits(_device_fold(hip_lib, x, order, final_threads)), _bits(F.fold(x, order, final_threads)))
    x = F.seeded_rows(700)
    x[333] = np.nan                         # one payload only: whichever operand's NaN an addition keeps, the bits are these
    got = _device_fold(hip_lib, x, order, final_threads)
    assert np.isnan(got).all()
    assert np.array_equal(_bits(got), _bits(F.fold(x, order, final_threads)))
