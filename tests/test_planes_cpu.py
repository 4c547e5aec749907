"""The float64 plane-search model (tests/plane_model.py) checked without a GPU: against the reference's own recorded inlier sets, on its
exact mode and its winner rule, and -- as conditions on the generated cases, not measurements -- the share of pairs each case of
tests/test_plane_edges_gpu.py leaves undecided.  A GPU test can therefore never pass by leaving pairs out."""
import os

import numpy as np
import pytest
import torch

import plane_model as M
from conftest import GOLDEN


def _cand_of_plane(plane):
    """the 8 kernel constants of a recorded winning plane, as plane_fitting_util._candidate derives them from its normal"""
    plane = np.asarray(plane, np.float32)
    n2 = torch.tensor([plane[0], plane[1], plane[2]], dtype=torch.float32)
    n2 = n2 / n2.norm()
    return np.float32([n2[0], n2[1], n2[2], plane[3], plane[0], plane[1], plane[2], n2.norm()])


@pytest.mark.parametrize("case", [0, 1])
def test_model_reproduces_the_reference_inliers(case):
    g = np.load(os.path.join(GOLDEN, "planes.npz"))
    _, thr, nthr, _, _ = g[f"params_{case}"]
    s_in, und = M.score(g[f"points_{case}"], g[f"normals_{case}"], _cand_of_plane(g[f"plane_{case}"])[None], thr, nthr)
    assert und.sum() == 0
    assert np.array_equal(np.flatnonzero(s_in[0]), g[f"inliers_{case}"])


def test_model_reproduces_the_reference_compat_planes():
    g = np.load(os.path.join(GOLDEN, "planes2.npz"))
    _, _, thr, nthr, _, _ = g["params"]
    cands = [([g[f"plane_{k}"]], _cand_of_plane(g[f"plane_{k}"])[None]) for k in range(3)]
    got = M.fit_planes_model(g["points"], g["normals"], 3, cands, thr, nthr, reference_compat=True)
    assert len(got) == 3
    for k in range(3):
        assert len(got[k]["undecided"]) == 0, k
        assert np.array_equal(got[k]["inliers"], g[f"inliers_{k}"]), k
    # the default filters the normals with the points: the first plane is the same, the second search sees other pairs
    dflt = M.fit_planes_model(g["points"], g["normals"], 2, cands[:2], thr, nthr)
    assert np.array_equal(dflt[0]["inliers"], got[0]["inliers"]) and not np.array_equal(dflt[1]["inliers"], got[1]["inliers"])


def test_exact_mode_refuses_inexact_arithmetic():
    p, q, c, _ = M.lattice_case()
    M.score(p, q, c, M.L_THR, M.L_NTHR, exact=True)                       # the lattice is exact
    p = p.copy()
    p[17, 0] = np.float32(0.1)                                          # 0.1f * 0.5 is a float32, 0.1f / 2 - y / 4 + z + 1/8 is not
    with pytest.raises(AssertionError, match="exact=True"):
        M.score(p, q, c, M.L_THR, M.L_NTHR, exact=True)
    c = M.L_CANDS.copy()
    c[1, 7] = 3                                                         # a quotient by 3
    with pytest.raises(AssertionError, match="exact=True"):
        M.score(*M.lattice_case()[:2], c, M.L_THR, M.L_NTHR, exact=True)


def test_best_is_the_first_strict_maximum():
    assert M.best([0, 0, 0]) == -1 and M.best([]) == -1
    assert M.best([0, 5, 5, 3]) == 1 and M.best([5, 0, 5]) == 0 and M.best([1, 2, 3, 3]) == 2
    assert M.best(np.uint32([0, 0, 1])) == 2 and M.best(np.uint32([4000000000, 1])) == 0


def test_non_finite_pairs_are_sure_out():
    (p, q, c), (po, qo, co), rows, cands = M.odd_case()
    s0, u0 = M.score(p, q, c, M.THR, M.NTHR)
    s1, u1 = M.score(po, qo, co, M.THR, M.NTHR)
    assert np.array_equal(s1[np.ix_(cands, rows)], s0) and np.array_equal(u1[np.ix_(cands, rows)], u0)
    assert not s1[M.ODD_AT_CAND].any() and not u1[M.ODD_AT_CAND].any()
    assert not s1[:, M.ODD_AT_ROW].any() and not u1[:, M.ODD_AT_ROW].any()
    assert s0.sum(1).min() > 0                                            # every ordinary candidate has inliers to lose


def _share(case):
    p, q, c = case[:3]
    s_in, und = M.score(p, q, c, M.THR, M.NTHR)
    return und.sum(), und.size, s_in


@pytest.mark.parametrize("P", M.CHUNK_P)
def test_undecided_cap_chunk_cases(P):
    und, pairs, s_in = _share(M.chunk_case(P))
    assert pairs == P * M.N_SMALL and und <= M.UNDECIDED_CAP * pairs, (und, pairs)
    if P == 513:                                                          # the winner sits alone in the third chunk, unrivalled
        lo = s_in.sum(1)
        assert M.best(lo) == 512 and lo[512] > lo[:512].max() + und


def test_undecided_cap_tie_case():
    und, pairs, s_in = _share(M.tie_case())
    lo = s_in.sum(1)
    assert und <= M.UNDECIDED_CAP * pairs
    _, u = M.score(*M.small_scene(), M.DOMINANT[None], M.THR, M.NTHR)
    assert u.sum() == 0                                                   # the tied candidate's count is known to the unit
    others = np.setdiff1d(np.arange(600), [7, 300, 599])
    assert lo[7] == lo[300] == lo[599] > lo[others].max() + und


@pytest.mark.parametrize("n", M.POINT_N + [M.N_BIG])
def test_undecided_cap_point_count_cases(n):
    case = M.big_case() if n == M.N_BIG else M.points_case(n)
    assert len(case[0]) == n
    und, pairs, s_in = _share(case)
    assert pairs == 3 * n and und <= M.UNDECIDED_CAP * pairs, (und, pairs)
    assert s_in[:, 0].any()                   # point 0 is an inlier: it is the point a dead tail lane reads, so counting one shows
    assert n == 1 or s_in.sum(1).min() > 0
    if n == M.N_BIG:
        assert s_in.sum(1).min() > 50000


def test_lattice_case_is_exact_and_planted():
    p, q, c, planted = M.lattice_case()
    s_in, und = M.score(p, q, c, M.L_THR, M.L_NTHR, exact=True)
    assert und.sum() == 0
    assert len(planted) == 32 and sum(inl for _, _, inl in planted) == 8
    for i, cand, inl in planted:
        assert s_in[cand, i] == inl, (i, cand)
    # on the thresholds themselves: the pairs a `<=` or a `>=` would take in
    p64, q64, c64 = p.astype(np.float64), q.astype(np.float64), c.astype(np.float64)
    dist = (p64 @ c64[:, :3].T + c64[:, 3]) / c64[:, 7]
    al = q64 @ c64[:, 4:7].T
    on_d = (np.abs(dist) == M.L_THR) & (np.abs(al) > M.L_NTHR)
    on_a = (np.abs(al) == M.L_NTHR) & (np.abs(dist) < M.L_THR)
    assert on_d.sum(0).min() >= 4 and on_a.sum(0).min() >= 4 and not s_in.T[on_d | on_a].any()
    assert s_in.sum(1).min() >= 4


def test_odd_case_caps():
    (p, q, c), (po, qo, co), _, _ = M.odd_case()
    for case in ((p, q, c), (po, qo, co)):
        assert _share(case)[0] == 0
    # thresholds that admit nothing: not one pair could be counted in, whatever the rounding
    s_in, und = M.score(p, q, c, 1e-9, 0.999999)
    assert s_in.sum() + und.sum() == 0


@pytest.mark.parametrize("compat", [False, True])
def test_driver_case_is_decided(compat):
    from gaussiansplattingregistration_amd.utils import plane_fitting_util as pf
    p, q = M.small_scene()
    torch.manual_seed(M.DRIVER_SEED)
    got = M.fit_planes_model(p, q, M.DRIVER_PLANES, lambda pts: M.draw(pf, torch.from_numpy(pts.copy()), M.DRIVER_ITERS, M.MSD), M.THR, M.NTHR,
                             reference_compat=compat)
    assert len(got) == 3
    for k, r in enumerate(got):
        assert len(r["undecided"]) == 0 and not r["contested"], k
    allidx = np.concatenate([r["inliers"] for r in got])
    assert len(np.unique(allidx)) == len(allidx)


def test_line_scene_runs_out_of_planes():
    """Once the plane is gone, three samples of the line are collinear: every candidate is NaN and the search ends with one plane."""
    from gaussiansplattingregistration_amd.utils import plane_fitting_util as pf
    p, q = M.line_scene()
    torch.manual_seed(11)
    seen = []

    def cands(pts):
        seen.append(M.draw(pf, torch.from_numpy(pts.copy()), 40, 0.25)[1])
        return [None] * 40, seen[-1]
    got = M.fit_planes_model(p, q, 3, cands, M.THR, M.NTHR)
    assert len(got) == 1 and len(seen) == 2 and len(got[0]["inliers"]) == 400 and len(got[0]["undecided"]) == 0
    assert np.isnan(seen[1]).all() and np.isnan(seen[0]).all(1).any()
