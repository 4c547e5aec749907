"""Float64 NumPy model of the fixed-order fold of csrc/gsr_fold.h; NumPy's addition is IEEE, so the model
gives the bits the kernels must give.  x is [n][3]: thread t of block b holds row 256 b + t, rows past n are +0.0."""
import numpy as np

XOR, ROWS = 0, 1
TREES = {XOR: (32, 16, 8, 4, 2, 1), ROWS: (8, 4, 2, 1, 16, 32)}
# the sizes the tests use: a lane, a wave and a block with one row less, exact and one row more; 64 blocks + 1 (one lane of the
# second stage takes two partials); 129 blocks, the last one short; 258 blocks (a thread of a 256-thread second stage takes two)
SIZES = (1, 63, 64, 65, 255, 256, 257, 64 * 256 + 1, 129 * 256 - 5)
SIZES_256 = SIZES + (257 * 256 + 3,)


def seeded_rows(n, seed=7):
    """n rows with a wide exponent range: where the order of the additions changes the rounding"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 3)) * 2.0 ** rng.integers(-20, 21, (n, 3))


def wave_sum(v, order):
    """v [..., 64, k] -> [..., k]: the butterfly over lanes l ^ o for o in TREES[order] (every lane ends with the same bits)"""
    lanes = np.arange(64)
    for o in TREES[order]:
        v = v + v[..., lanes ^ o, :]
    return v[..., 0, :]


def waves_in_order(w):
    """w [..., 4, k] -> ((w0 + w1) + w2) + w3"""
    return ((w[..., 0, :] + w[..., 1, :]) + w[..., 2, :]) + w[..., 3, :]


def fold(x, order, final_threads):
    x = np.asarray(x, np.float64)
    nb = (len(x) + 255) // 256
    rows = np.zeros((nb * 256, 3))
    rows[:len(x)] = x
    partials = waves_in_order(wave_sum(rows.reshape(nb, 4, 64, 3), order))           # block_fold_store: [nb][3]
    s = np.zeros((final_threads, 3))                                                 # k_fold_partials: thread t takes t, t + T, ...
    for b0 in range(0, nb, final_threads):
        part = partials[b0:b0 + final_threads]
        s[:len(part)] += part
    w = wave_sum(s.reshape(final_threads // 64, 64, 3), XOR)
    return w[0] if final_threads == 64 else waves_in_order(w)
