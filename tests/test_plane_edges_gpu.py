"""The RANSAC plane search (k_plane_score, k_plane_mask, gsr_plane_score in csrc/model.hip; fit_planes) against the float64 model of
tests/plane_model.py, where the kernels can go wrong: more candidates than one LDS chunk holds, ties between chunks, point counts around
a wave and a block and past one grid-stride trip, points exactly on both thresholds, non-finite and degenerate rows and candidates,
host against device placement, and the driver plane by plane.  The inputs are plane_model's; tests/test_planes_cpu.py holds the
conditions on them (how many pairs each case may leave undecided: at most 1 in 10^5, none on the lattice)."""
import ctypes as C

import numpy as np
import pytest
import torch

import plane_model as M

pytestmark = pytest.mark.gpu
SENTINEL = 0xAB


class _PC:
    def __init__(self, points, normals):
        self.points, self.normals = points, normals


def _score(p, q, c, thr, nthr, on_device=False):
    """gsr_plane_score on host arrays or on CUDA tensors -> counts, best, mask (pre-filled with SENTINEL), return code"""
    from gaussiansplattingregistration_amd import _lib
    L = _lib.load(require_device=True)
    n, P = len(p), len(c)
    p, q, c = (np.ascontiguousarray(a, np.float32) for a in (p, q, c))
    counts = np.full(max(P, 1), 0xFFFFFFFF, np.uint32)
    best = C.c_int32(12345)
    if on_device:
        tp, tq = torch.tensor(p, device="cuda"), torch.tensor(q, device="cuda")
        tm = torch.full((max(n, 1),), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.current_stream().synchronize()
        rc = L.gsr_plane_score(tp.data_ptr(), tq.data_ptr(), n, c.ctypes.data, P, thr, nthr, counts.ctypes.data, tm.data_ptr(), C.byref(best), 1, 0,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
        mask = tm.cpu().numpy()
    else:
        mask = np.full(max(n, 1), SENTINEL, np.uint8)
        rc = L.gsr_plane_score(p.ctypes.data, q.ctypes.data, n, c.ctypes.data, P, thr, nthr, counts.ctypes.data, mask.ctypes.data, C.byref(best), 0, 0, None)
    return counts[:P], best.value, mask[:n], rc


def _check(p, q, c, thr=M.THR, nthr=M.NTHR, exact=False, on_device=False):
    """The four properties of a case; -> counts, best, mask, sure_in."""
    counts, best, mask, rc = _score(p, q, c, thr, nthr, on_device)
    assert rc == 0
    s_in, und = M.score(p, q, c, thr, nthr, exact=exact)
    lo = s_in.sum(1)
    hi = lo + und.sum(1)
    print(f"n {len(p)} P {len(c)}: undecided {int(und.sum())} of {und.size}, counts off the sure ones by at most {int(np.abs(counts.astype(np.int64) - lo).max())}")
    bad = np.flatnonzero((counts < lo) | (counts > hi))
    assert len(bad) == 0, (bad[:8], counts[bad[:8]], lo[bad[:8]], hi[bad[:8]])
    assert best == M.best(counts)
    if best < 0:
        assert (mask == SENTINEL).all()
        return counts, best, mask, s_in
    assert set(np.unique(mask)) <= {0, 1}
    decided = ~und[best]
    assert np.array_equal(mask[decided].astype(bool), s_in[best][decided])
    assert int(mask.sum()) == int(counts[best])                       # the score kernel and the mask kernel agree to the unit
    return counts, best, mask, s_in


@pytest.mark.parametrize("P", M.CHUNK_P)
def test_candidate_chunks(P):
    """P around PLANE_CHUNK = 256 and up to the reference's default of 1000 iterations: every further chunk re-zeroes the LDS counters
    and adds into counts[p0 + ...]."""
    counts, best, _, s_in = _check(*M.chunk_case(P))
    assert counts.max() > 0
    if P == 513:
        assert best == 512                                            # the winner is the only candidate of the third chunk


def test_ties_across_chunks():
    counts, best, _, s_in = _check(*M.tie_case())
    assert best == 7 and counts[7] == counts[300] == counts[599] == s_in[7].sum() == counts.max()


@pytest.mark.parametrize("n", M.POINT_N)
def test_point_counts_around_a_wave_and_a_block(n):
    counts, _, _, _ = _check(*M.points_case(n))
    assert n == 1 or counts.sum() > 0


def test_second_grid_stride_trip():
    """n = 2048 * 256 + 257: the grid is capped at 2048 blocks, so blocks 0 and 1 take a second trip, block 1's with a single live lane:
    63 lanes of its first wave and its three other waves are kept alive for the ballot only."""
    counts, _, _, _ = _check(*M.big_case())
    assert counts.min() > 50000


def test_points_on_the_thresholds():
    """The lattice: no rounding anywhere, points on |dist| == thr and |al| == nthr (both out) and one lattice step inside (in), in the
    first, a middle and the last wave of a block, lanes 0 and 63, and in the partial tail wave.  Counts and mask equal the model."""
    p, q, c, planted = M.lattice_case()
    counts, best, mask, s_in = _check(p, q, c, M.L_THR, M.L_NTHR, exact=True)
    assert np.array_equal(counts, s_in.sum(1)) and np.array_equal(mask.astype(bool), s_in[best])
    for k in (0, 1):                                                  # each candidate's own mask
        _, b, m, _ = _check(p, q, c[k:k + 1], M.L_THR, M.L_NTHR, exact=True)
        assert b == 0 and np.array_equal(m.astype(bool), s_in[k])
        for i, cand, inl in planted:
            assert cand != k or bool(m[i]) == inl, (i, cand)


def test_non_finite_and_degenerate_input():
    """Rows with a NaN coordinate, an Inf coordinate, a NaN normal and a zero normal, a NaN candidate (what collinear samples give) and a
    candidate with nn = 0: they score nothing, never win and change no other count."""
    (p, q, c), (po, qo, co), rows, cands = M.odd_case()
    counts0, best0, mask0, _ = _check(p, q, c)
    counts1, best1, mask1, _ = _check(po, qo, co)
    assert counts0.min() > 0
    assert np.array_equal(counts1[cands], counts0) and (counts1[M.ODD_AT_CAND] == 0).all()
    assert best1 == cands[best0]
    assert np.array_equal(mask1[rows], mask0) and (mask1[M.ODD_AT_ROW] == 0).all()
    # the odd candidates alone, among ordinary and odd rows: nothing wins, the mask is not written
    for cc in (M.ODD_CANDS[:1], M.ODD_CANDS, np.repeat(M.ODD_CANDS[:1], 300, 0)):
        for on_device in (False, True):
            counts, best, mask, rc = _score(po, qo, cc, M.THR, M.NTHR, on_device)
            assert rc == 0 and best == -1 and (counts == 0).all() and (mask == SENTINEL).all()
    # thresholds that admit nothing
    for on_device in (False, True):
        counts, best, mask, rc = _score(p, q, c, 1e-9, 0.999999, on_device)
        assert rc == 0 and best == -1 and (counts == 0).all() and (mask == SENTINEL).all()


def test_empty_input():
    p, q, c = M.points_case(64)
    for pp, qq, cc in ((p[:0], q[:0], c), (p, q, c[:0]), (p[:0], q[:0], c[:0])):
        for on_device in (False, True):
            counts, best, mask, rc = _score(pp, qq, cc, M.THR, M.NTHR, on_device)
            assert rc == 0 and best == -1 and (mask == SENTINEL).all()


@pytest.mark.parametrize("case", ["chunks", "lattice", "odd"])
def test_placement_and_reproducibility(case):
    """Host arrays and device tensors (on_device = 1), and two runs of each: the same counts, winner and mask bytes."""
    p, q, c = {"chunks": lambda: M.chunk_case(513), "lattice": lambda: M.lattice_case()[:3], "odd": lambda: M.odd_case()[1]}[case]()
    thr, nthr = (M.L_THR, M.L_NTHR) if case == "lattice" else (M.THR, M.NTHR)
    runs = [_score(p, q, c, thr, nthr, on_device) for on_device in (False, True, False, True)]
    for counts, best, mask, rc in runs[1:]:
        assert rc == 0 and best == runs[0][1] >= 0
        assert counts.tobytes() == runs[0][0].tobytes() and mask.tobytes() == runs[0][2].tobytes()


@pytest.mark.parametrize("compat", [False, True])
def test_driver_against_the_serial_model(compat, monkeypatch):
    """fit_planes, three planes of 300 candidates (two chunks) each, the shrinking point set kept on the device, against
    fit_planes_model fed the very candidates fit_planes drew: the same planes bit for bit, the same inliers in original indices."""
    from gaussiansplattingregistration_amd.utils import plane_fitting_util as pf
    p, q = M.small_scene()
    drawn, real = [], pf._candidate

    def recording(points_tensor, sampled):
        drawn.append(real(points_tensor, sampled))
        return drawn[-1]
    monkeypatch.setattr(pf, "_candidate", recording)
    torch.manual_seed(M.DRIVER_SEED)
    planes, inliers = pf.fit_planes(_PC(p, q), M.DRIVER_PLANES, M.DRIVER_ITERS, M.THR, M.NTHR, M.MSD, reference_compat=compat)
    assert len(drawn) == len(planes) * M.DRIVER_ITERS
    searches = [drawn[k:k + M.DRIVER_ITERS] for k in range(0, len(drawn), M.DRIVER_ITERS)]
    want = M.fit_planes_model(p, q, M.DRIVER_PLANES, [([pl for pl, _ in s], np.stack([cd for _, cd in s])) for s in searches], M.THR, M.NTHR,
                              reference_compat=compat)
    assert len(planes) == len(want) == 3
    for k, w in enumerate(want):
        assert len(w["undecided"]) == 0 and not w["contested"], k         # tests/test_planes_cpu.py holds this for the seed
        assert np.asarray(planes[k]).tobytes() == np.asarray(w["plane"]).tobytes(), k
        assert inliers[k].dtype == torch.int64 and np.array_equal(inliers[k].numpy(), w["inliers"]), k
    allidx = torch.cat(inliers).numpy()
    assert len(np.unique(allidx)) == len(allidx)


def test_driver_ends_when_every_candidate_is_collinear():
    """After its plane the line scene has only collinear points left: every candidate of the second search is NaN, nothing wins, and
    fit_planes returns the one plane it found."""
    from gaussiansplattingregistration_amd.utils import plane_fitting_util as pf
    p, q = M.line_scene()
    torch.manual_seed(11)
    planes, inliers = pf.fit_planes(_PC(p, q), 3, 40, M.THR, M.NTHR, 0.25)
    assert len(planes) == len(inliers) == 1 and np.isfinite(planes[0]).all()
    assert np.array_equal(inliers[0].numpy(), np.flatnonzero(p[:, 2] == 0))
