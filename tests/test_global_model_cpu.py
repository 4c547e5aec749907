"""Global registration without a GPU: the C ABI of the new entry points, the RANSAC sampler of the library against the NumPy
restatement (tests/global_model.py), sanity of the restatement itself, and the proof that the restatement decides every edge-shape
input (tests/global_edge_cases.py) that tests/test_global_edges_gpu.py puts to the kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import global_edge_cases as E
import global_model as G
from conftest import ROOT

NEW = ["gsr_hybrid_search", "gsr_fpfh", "gsr_feature_match", "gsr_ransac_correspondence"]


def test_global_entry_points_in_header_and_bindings(hip_lib):
    from gaussiansplattingregistration_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(hip_lib, name)
    assert "gsr_debug_ransac_sample" in _lib.TEST_HOOKS
    assert C.sizeof(_lib.RansacParams) == 96 and C.sizeof(_lib.RansacResult) == 176


def test_sampler_hook_equals_numpy(hip_lib):
    for seed, k0, m, n in ((0, 0, 1000, 3), (123456789, 77777, 3, 4), ((1 << 64) - 1, 1 << 40, 2 ** 31 - 1, 5)):
        count = 100000 // n
        out = np.empty((count, n), np.int32)
        assert hip_lib.gsr_debug_ransac_sample(seed, k0, count, m, n, out.ctypes.data) == 0
        want = G.ransac_sample(seed, k0, count, m, n)
        assert np.array_equal(out.astype(np.int64), want)
        assert want.min() >= 0 and want.max() < m
    # roughly uniform
    out = G.ransac_sample(5, 0, 100000, 10, 1)
    assert np.all(np.abs(np.bincount(out[:, 0], minlength=10) - 10000) < 500)


def _cloud(n=3000, seed=3):
    sc = G.make_scene(n, seed)
    return sc["xyz"], sc["normals"]


def test_spfh_thirds_sum_to_100():
    xyz, nrm = _cloud()
    spfh, fpfh = G.spfh_fpfh(xyz, nrm, 0.15, 100)
    has = spfh.sum(1) > 0
    assert has.mean() > 0.95
    for q in range(3):
        assert np.allclose(spfh[has, 11 * q:11 * q + 11].sum(1), 100.0, atol=1e-9)
        assert np.allclose(fpfh[has, 11 * q:11 * q + 11].sum(1), 200.0, atol=1e-9)


def test_fpfh_invariant_under_rigid_motion():
    """A quarter turn about z maps float32 coordinates exactly, so every d2 and neighbour list is the same.  The histograms may then
    differ only where phi = atan2(+-0, -1) = +-pi (antiparallel normals): bin 0 <-> bin 10 of the first third, the one place where
    the angle wraps.  Everything else is equal to rounding."""
    xyz, nrm = _cloud(2000, 4)
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    xyz2 = (xyz.astype(np.float64) @ R.T).astype(np.float32)
    assert np.array_equal(xyz2[:, 0], -xyz[:, 1]) and np.array_equal(xyz2[:, 1], xyz[:, 0])
    s1, f1 = G.spfh_fpfh(xyz, nrm, 0.15, 100)
    s2, f2 = G.spfh_fpfh(xyz2, nrm @ R.T, 0.15, 100)
    d = np.abs(s1 - s2)
    d[:, [0, 10]] = 0.0
    assert d.max() < 1e-9
    assert np.allclose(s1[:, 0] + s1[:, 10], s2[:, 0] + s2[:, 10], atol=1e-9)
    assert np.allclose(f1[:, 11:], f2[:, 11:], atol=1e-9)          # alpha and theta thirds of FPFH: unchanged
    same = np.all(np.abs(f1 - f2) < 1e-9, axis=1)
    assert same.mean() > 0.5


def test_serial_ransac_recovers_T_gt():
    sc = G.make_scene(3000, 5)
    T = G.make_T()
    src = sc["xyz"]
    tgt = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    rng = np.random.default_rng(0)
    m = 600
    i = rng.choice(len(src), m, replace=False)
    j = i.copy()
    bad = rng.random(m) < 0.7                      # 70 % wrong correspondences
    j[bad] = rng.integers(0, len(src), bad.sum())
    corres = np.stack([i, j], 1).astype(np.int32)
    r = G.ransac(src, tgt, corres, 0.02, checkers=[(G.EDGE, 0.9), (G.DIST, 0.02)], max_iteration=5000, confidence=0.999, seed=1)
    assert r["best_index"] >= 0 and r["exit_index"] < 5000
    assert np.abs(r["transformation"] - T).max() < 1e-4
    assert r["fitness"] >= 0.29
    # degenerate inputs: Open3D's empty result
    for kw in ({"ransac_n": 2}, {"max_corr": 0.0}):
        args = dict(max_corr=0.02, ransac_n=3)
        args.update(kw)
        e = G.ransac(src, tgt, corres[:10], args["max_corr"], ransac_n=args["ransac_n"])
        assert e["best_index"] == -1 and np.array_equal(e["transformation"], np.eye(4)) and e["fitness"] == 0.0


# ---- the edge-shape inputs of tests/test_global_edges_gpu.py: the restatement decides each one before a GPU sees it -----------
def test_two_point_parallel_pair_known_answer():
    """Two points (0, 0, 0) and (0, 0, 1), both normals (0, 0, 1), radius 2, max_nn 10, by hand and without the restatement:
    each point has k = 2 neighbours (itself and the other), hence one pair, and that pair's p2 - p1 is parallel to the frame normal:
    v = dp x n = 0, so the pair feature is Open3D's zero vector, which falls into bin 5 of each third (11 * (0 + pi) / 2 pi = 11 *
    (0 + 1) / 2 = 5.5).  With one pair the increment is 100 / (k - 1) = 100: SPFH = 100 in bins 5, 16 and 27.  d2 = 1, so the
    neighbour's SPFH enters with weight 1, each third sums to 100 and its scale is 100 / 100 = 1: FPFH = 100 * 1 + SPFH = 200 in
    bins 5, 16 and 27 and 0 elsewhere, for both rows, exactly in float64."""
    spfh, fpfh = G.spfh_fpfh(*E.TWO_POINTS)
    assert np.array_equal(spfh, E.TWO_POINTS_FPFH / 2) and np.array_equal(fpfh, E.TWO_POINTS_FPFH)


def test_small_clouds_are_those_of_the_grid_tests():
    import test_grid_gpu
    for name in ("n1", "n2", "n3", "dup64"):
        assert np.array_equal(E._small(name), test_grid_gpu.cloud(name))


@pytest.mark.parametrize("name", sorted(E.FPFH_CASES))
def test_edge_fpfh_inputs_are_decided(name):
    """No pair feature of the input lies within 1e-9 of a bin edge (or at phi = +-pi): two correct implementations agree on every row."""
    xyz, nrm, radius, max_nn = E.fpfh_input(name)
    nbrs, spfh, fpfh = E.fpfh_want(name)
    assert not G._near_edge_rows(xyz, nrm, nbrs).any()
    k = np.array([len(x) for x in nbrs])
    head = name.split("-")[0]
    if head in ("plusz", "checker", "parity"):
        # the input reaches what it is there for: a pair with len != 0 and v_norm == 0 in every row ...
        P, N = xyz.astype(np.float64), nrm
        for i, x in enumerate(nbrs):
            dp = P[x[1:]] - P[i]
            a1 = np.abs(dp @ N[i]) / np.linalg.norm(dp, axis=1)
            a2 = np.abs((dp * N[x[1:]]).sum(1)) / np.linalg.norm(dp, axis=1)
            par1, par2 = a1 == 1.0, (a2 == 1.0) & (a2 > a1)
            # ... without the swap (the point's own normal is the frame's) or through it (the neighbour's is)
            assert par2.any() if head == "checker" and (xyz[i].sum() % 2) == 0 else par1.any(), i
    elif head == "zero":
        assert np.array_equal(fpfh[:, [5, 16, 27]], np.full((len(xyz), 3), 200.0)) and np.count_nonzero(fpfh) == 3 * len(xyz)
    elif head == "dup64":
        assert np.all(k == 64) and np.array_equal(fpfh, spfh) and np.array_equal(fpfh[:, [5, 16, 27]], np.full((64, 3), 100.0))
    elif head == "n1" or name.endswith("-nn1"):
        assert np.all(k == 1) and not fpfh.any()
    elif head in ("n2", "n3"):
        assert np.all(k == min(len(xyz), max_nn)) and fpfh.any()
    else:
        assert k.min() >= 2 and k.max() < max_nn


@pytest.mark.parametrize("name", sorted(E.FPFH_UNDECIDED))
def test_edge_fpfh_inputs_left_out_are_the_undecided_ones(name):
    """+-z by index parity at radius 1.5 and 2.0: the diagonal neighbours' normals are antiparallel, phi = atan2(+-0, -1), and the sign
    of a zero picks bin 0 or 10.  The three axes by index mod 3: alpha = +-1 sits on the outer edge of its bins, where one ulp of the
    normalisation moves it.  Every row is touched, at every radius: nothing of these inputs can be held to 1e-9."""
    xyz, nrm, radius, max_nn = E.fpfh_input(name)
    assert G._near_edge_rows(xyz, nrm, E.fpfh_want(name)[0]).all()


def test_edge_fpfh_two_trip_cloud_is_decided():
    xyz, nrm = E.two_trip_cloud()
    assert len(xyz) == E.TRIP + E.TAIL > 4096 * 128 and E.TRIP == 2048 * 256
    head, tail = xyz[:E.TRIP].astype(np.float64), xyz[E.TRIP:].astype(np.float64)
    assert np.array_equal(head, np.round(head)) and len(np.unique(head, axis=0)) == E.TRIP      # distinct integer points: 1 apart
    assert np.linalg.norm(tail - np.round(tail), axis=1).min() > 0.5 > 2 * E.TWO_TRIP_RADIUS - 0.01
    nbrs = G.hybrid_search(xyz[E.TRIP:], E.TWO_TRIP_RADIUS, E.TWO_TRIP_NN)
    assert not G._near_edge_rows(xyz[E.TRIP:], nrm[E.TRIP:], nbrs).any()
    assert max(len(x) for x in nbrs) == E.TWO_TRIP_NN              # the cut at max_nn is taken


@pytest.mark.parametrize("na,nb", E.FM_PLANTED)
def test_edge_feature_match_plants_straddle_the_chunks(na, nb):
    nch, chunk = E.fm_chunks(na, nb)
    assert nch >= 2 and E.FM_TIE_TGT // chunk == 0 and (nb - 1) // chunk == (nb - 2) // chunk == nch - 1
    fs, ft = E.fm_planted(na, nb, True)
    _, _, nst, _ = G.feature_match(fs, ft, False)
    assert nst[E.FM_TIE_SRC] == E.FM_TIE_TGT and nst[E.FM_LAST_SRC] == nb - 2 and nst[E.FM_NAN_SRC] == 0
    # why the NaN row is planted only without `mutual`: in the search back, the restatement's argmin picks the NaN row for every target row
    assert np.all(G.nn_rows(ft, fs) == E.FM_NAN_SRC)
    # without it, every minimum of either direction is strict, or an exact tie between the two equal target rows (equal operands in
    # the same order: the same d on either side), which the lowest index wins
    fs, ft = E.fm_planted(na, nb, False)
    for a, b in ((fs, ft), (ft, fs)):
        d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(2)
        two = np.sort(d, axis=1)[:, :2]
        gap = two[:, 1] - two[:, 0]
        assert np.all((gap == 0.0) | (gap > 1e-9))
        assert np.all(np.argmin(d, axis=1)[gap == 0.0] == E.FM_TIE_TGT) and ((gap == 0.0).any() == (b is ft))


def test_edge_feature_match_shapes_sit_on_the_kernel_edges():
    chunks = {s: E.fm_chunks(*s) for s in E.FM_SHAPES}
    assert chunks[(300, 512)] == (1, 512) and chunks[(300, 513)] == (2, 257) and chunks[(70, 1025)] == (3, 342)
    assert E.fm_chunks(*E.FM_TWO_TRIP) == (1, 40) and E.FM_TWO_TRIP[0] > 2048 * 256
    # random rows: every nearest row is nearest by far more than a rounding error (and the kernel's sum is the restatement's, term by term)
    for na, nb in E.FM_SHAPES:
        fs, ft = E.fm_input(na, nb)
        for a, b in ((fs, ft), (ft, fs)):
            if len(b) > 1:
                two = np.sort(((a[:, None, :] - b[None, :, :]) ** 2).sum(2), axis=1)[:, :2]
                assert np.all(two[:, 1] - two[:, 0] > 1e-9)


@pytest.mark.parametrize("name", sorted(E.RANSAC_CASES))
def test_edge_ransac_cases_are_decided(name):
    """The restatement finds a best hypothesis (an empty result would test nothing), no d2 of a valid hypothesis lies within
    1e-6 max_corr^2 of max_corr^2, and the best hypothesis' own system is well conditioned."""
    assert E.ransac_undecided(name) == []
    want, _ = E.ransac_want(name)
    c = E.RANSAC_CASES[name]
    if c["confidence"] == 1.0:
        assert want["exit_index"] == want["n_evaluated"] == c["max_iteration"]
