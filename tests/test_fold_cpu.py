"""The inputs of tests/test_fold_gpu.py tell the orders apart (conditions on the inputs, checked in the NumPy model alone): on the
seeded rows the two wave trees of csrc/gsr_fold.h give different bits -- a caller that swapped its tree would not pass -- and both
differ from NumPy's own pairwise sum, so a kernel that summed in some other reasonable order would not pass either."""
import numpy as np
import pytest

import fold_model as F


def _bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


@pytest.mark.parametrize("final_threads", [64, 256])
@pytest.mark.parametrize("n", [n for n in F.SIZES_256 if n >= 63])
def test_the_two_trees_give_different_bits_on_the_seeded_rows(n, final_threads):
    x = F.seeded_rows(n)
    assert not np.array_equal(_bits(F.fold(x, F.XOR, final_threads)), _bits(F.fold(x, F.ROWS, final_threads)))


@pytest.mark.parametrize("final_threads", [64, 256])
@pytest.mark.parametrize("n", [n for n in F.SIZES_256 if n >= 64])
def test_both_trees_differ_from_numpy_sum_on_the_seeded_rows(n, final_threads):
    x = F.seeded_rows(n)
    for order in (F.XOR, F.ROWS):
        assert not np.array_equal(_bits(F.fold(x, order, final_threads)), _bits(x.sum(0)))


def test_the_model_is_a_sum_and_keeps_special_values():
    x = F.seeded_rows(1000)
    for order in (F.XOR, F.ROWS):
        for T in (64, 256):
            assert np.allclose(F.fold(x, order, T), x.sum(0), rtol=0, atol=1000 * 2.0 ** -52 * np.abs(x).sum(0).max())
            # one row: the value itself; a full block of -0.0 stays -0.0 through both trees, and +0.0 comes out of the second
            # stage, whose lanes start at +0.0
            assert np.array_equal(_bits(F.fold(x[:1], order, T)), _bits(x[0]))
            assert np.array_equal(_bits(F.fold(np.full((256, 3), -0.0), order, T)), _bits(np.zeros(3)))
            nan = x[:300].copy()
            nan[77, 1] = np.nan
            got = F.fold(nan, order, T)
            assert np.isnan(got[1]) and np.isfinite(got[[0, 2]]).all()
