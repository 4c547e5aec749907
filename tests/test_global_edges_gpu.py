"""The three stages of csrc/features.hip (FPFH, feature matching, RANSAC over correspondences) on the MI355X at the shapes where a
kernel goes wrong and a workload-sized test does not look: degenerate Darboux frames, one to three points, sizes on either side of a
block, a tile and a chunk, ragged batches, and the second trip of every grid-stride loop (n = 524 288 + 300).  Every expectation is
the float64 restatement's (tests/global_model.py) or derived by hand; the inputs come from tests/global_edge_cases.py, and
tests/test_global_model_cpu.py shows for each, without a GPU, that the restatement decides it.  The tolerances are those of
tests/test_global_registration_gpu.py, with no allowance for rows at bin edges: no input here has any.

    FPFH rows                                                                 < 1e-9, every row
    match indices, correspondences, used_mutual                               exact
    best_index, exit_index, n_evaluated, n_valid, fitness                     exact
    inlier_rmse                                                               < 1e-12
    transformation                                                            < 1e-9

Left out, because the restatement does not decide them (never held to a looser bar instead):
  * FPFH on the 6 x 6 x 6 lattice with normals +-z by index parity at radius 1.5 and 2.0: every row has a pair with antiparallel normals,
    phi = atan2(+-0, -1), where the sign of a zero picks bin 0 or bin 10.  Radius 1.0 is in.
  * FPFH on that lattice with the x, y, z axis as normal by index mod 3: every row has alpha = +-1, on the outer bin edge.
  * A NaN row among the TARGET rows of a feature match, which includes a NaN source row under `mutual` (the search back runs against
    the source): the restatement's argmin selects a NaN row, k_fm_nn never does, and nothing in the project says which is right.  The
    NaN source row is planted without `mutual` only, where it must match row 0.
  * NaN coordinates or normals in fpfh: (int)floor(NaN) is undefined in the kernel and the restatement alike.
"""
import numpy as np
import pytest
import torch

import global_edge_cases as E
import global_model as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F(hip_lib):
    from gaussiansplattingregistration_amd import features
    return features


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()             # (a copy: the shared inputs are read-only)


# ---- FPFH ---------------------------------------------------------------------------------------------------------------------
def test_fpfh_two_point_parallel_pair_known_answer(F):
    """Two points (0, 0, 0) and (0, 0, 1), both normals (0, 0, 1), radius 2, max_nn 10.  Each point has k = 2, hence one pair, and its
    p2 - p1 is parallel to the frame normal: the pair feature is Open3D's zero vector, bins 5 / 5 / 5 (11 * 0.5 = 5.5 in each third).
    One pair: the increment is 100 / (k - 1) = 100, SPFH = 100 in bins 5, 16 and 27.  d2 = 1: each third of the neighbour sum is 100,
    its scale 100 / 100 = 1.  FPFH = 100 + SPFH = 200 in bins 5, 16 and 27 and 0 elsewhere, both rows, exact in float64."""
    got = F.fpfh(*E.TWO_POINTS)
    assert np.array_equal(got, E.TWO_POINTS_FPFH), got


@pytest.mark.parametrize("name", sorted(E.FPFH_CASES))
def test_fpfh_edge_input_equals_restatement(F, name):
    """plusz / checker / parity: p2 - p1 exactly parallel to the frame normal (v_norm == 0) without and through the swap; zero: every
    normal the zero vector; dup64: every pair coincident, every d2 skipped (FPFH = SPFH); n1 .. n3: fewer points than any max_nn, k = 1
    rows all zero; uniform127 .. 129: around one k_spfh block of 128."""
    xyz, nrm, radius, max_nn = E.fpfh_input(name)
    _, _, want = E.fpfh_want(name)
    got = F.fpfh(xyz, nrm, radius, max_nn)
    assert got.shape == want.shape == (len(xyz), 33)
    err = np.abs(got - want).max(1)
    print(name, "rows", len(xyz), "rows off", int((err >= 1e-9).sum()), "max |got - want|", err.max())
    assert np.all(err < 1e-9), (np.flatnonzero(err >= 1e-9)[:10], err.max())
    dev = F.fpfh(_dev(xyz), _dev(nrm), radius, max_nn)
    assert torch.equal(dev.cpu(), torch.from_numpy(got))


def test_fpfh_second_trip_of_the_grid_stride_loops(F):
    """n = 524 288 + 300 > 4096 x 128 = 2048 x 256: k_spfh (whose LDS histogram is zeroed again inside the loop) and k_fpfh go round
    twice.  The first 524 288 points are alone within the radius: rows of exact zeros.  The last 300 see only each other, in input
    order, so their rows are the restatement's on those 300 alone."""
    xyz, nrm = E.two_trip_cloud()
    got = F.fpfh(_dev(xyz), _dev(nrm), E.TWO_TRIP_RADIUS, E.TWO_TRIP_NN)
    assert got.is_cuda and tuple(got.shape) == (E.TRIP + E.TAIL, 33)
    assert int(torch.count_nonzero(got[:E.TRIP])) == 0
    _, want = G.spfh_fpfh(xyz[E.TRIP:], nrm[E.TRIP:], E.TWO_TRIP_RADIUS, E.TWO_TRIP_NN)
    err = np.abs(got[E.TRIP:].cpu().numpy() - want).max(1)
    print("tail rows off", int((err >= 1e-9).sum()), "max |got - want|", err.max())
    assert np.all(err < 1e-9), (np.flatnonzero(err >= 1e-9)[:10], err.max())


# ---- feature matching ---------------------------------------------------------------------------------------------------------
def _match_equals_restatement(F, fs, ft, mutual):
    c, um, nst, nts = F.feature_match(fs, ft, mutual=mutual, return_nn=True)
    wc, wum, wst, wts = G.feature_match(fs, ft, mutual)
    assert np.array_equal(nst, wst), np.flatnonzero(nst != wst)[:10]
    if mutual:
        assert np.array_equal(nts, wts), np.flatnonzero(nts != wts)[:10]
    assert um == wum and np.array_equal(c, wc)
    dc, dum = F.feature_match(_dev(fs), _dev(ft), mutual=mutual)
    assert torch.equal(dc.cpu(), torch.from_numpy(c.astype(np.int32))) and dum == um
    return nst


@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("na,nb", E.FM_SHAPES)
def test_feature_match_edge_shapes(F, na, nb, mutual):
    """nb below a tile (32), on either side of a tile and of a chunk (512); na on either side of FM_BLOCK (256)."""
    _match_equals_restatement(F, *E.fm_input(na, nb), mutual)


@pytest.mark.parametrize("mutual", [False, True])
@pytest.mark.parametrize("na,nb", E.FM_PLANTED)
def test_feature_match_ties_across_chunks(F, na, nb, mutual):
    """nn_rows splits the target into nch = min(ceil(2048 / ceil(na / 256)), ceil(nb / 512)) chunks of ceil(nb / nch) rows: 2 x 257 at
    (300, 513), 3 x 342 at (70, 1025).  Target row 3 (chunk 0) is repeated as the last row (last chunk) and as a source row: both
    chunks report d = 0 and the strict `<` of k_fm_merge must keep the lower index.  Another source row equals target row nb - 2: a
    strict minimum in the last chunk.  Without `mutual`, a source row of NaN matches row 0."""
    nst = _match_equals_restatement(F, *E.fm_planted(na, nb, not mutual), mutual)
    assert nst[E.FM_TIE_SRC] == E.FM_TIE_TGT and nst[E.FM_LAST_SRC] == nb - 2
    if not mutual:
        assert nst[E.FM_NAN_SRC] == 0


def test_feature_match_second_trip_of_the_merge(F):
    """na = 524 288 + 300 > 2048 x 256: k_fm_merge goes round twice.  The first 2 000 and the last 300 rows against the restatement."""
    na, nb = E.FM_TWO_TRIP
    rng = np.random.default_rng(17)
    fs, ft = rng.random((na, 33)) * 50, rng.random((nb, 33)) * 50
    c, um, nst, nts = F.feature_match(_dev(fs), _dev(ft), mutual=False, return_nn=True)
    assert not um and nts is None and tuple(c.shape) == (na, 2)
    c, nst = c.cpu().numpy(), nst.cpu().numpy()
    assert np.array_equal(c[:, 0], np.arange(na)) and np.array_equal(c[:, 1], nst)
    for rows in (slice(0, 2000), slice(na - E.TAIL, na)):
        assert np.array_equal(nst[rows], G.nn_rows(fs[rows], ft))


# ---- RANSAC -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(E.RANSAC_CASES))
def test_ransac_edge_case_equals_serial_restatement(F, name):
    """m3 .. m257: m below, at and above one k_ransac_eval block (256), where most threads carry a zero sum into the tree; -b250:
    max_iteration 1001 in batches of 250 (the last batch is 1: neither a multiple of RANSAC_HB = 4 nor of the 64 of k_ransac_hyp);
    -b1: 7 batches of 1; -conf1: confidence 1.0, never an early exit; -it1: a single hypothesis; m257-checkers: the three checkers;
    plane-m6 / -m70: point-to-plane at m = ransac_n and above, one batch of 203; gather-two-trips: m = 524 288 + 300 rows, twice
    round k_ransac_gather."""
    args, kw = E.ransac_input(name)
    want, _ = E.ransac_want(name)
    got = F.ransac_correspondence(*args, **kw)
    print(name, {k: (got[k], want[k]) for k in ("best_index", "exit_index", "n_evaluated", "n_valid", "fitness", "inlier_rmse")},
          "max |T - T_want|", np.abs(got["transformation"] - want["transformation"]).max())
    for k in ("best_index", "exit_index", "n_evaluated", "n_valid"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["fitness"] == want["fitness"]
    assert abs(got["inlier_rmse"] - want["inlier_rmse"]) < 1e-12
    assert np.abs(got["transformation"] - want["transformation"]).max() < 1e-9
    if kw["confidence"] == 1.0:
        assert got["exit_index"] == got["n_evaluated"] == kw["max_iteration"]
    if name == "gather-two-trips":           # device in: the rows are gathered from the caller's arrays
        src, tgt, corres, max_corr = args
        again = F.ransac_correspondence(_dev(src), _dev(tgt), _dev(corres), max_corr, **kw)
        assert all(np.array_equal(np.asarray(got[k]), np.asarray(again[k])) for k in got)
