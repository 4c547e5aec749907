"""Compatibility-graph global registration without a GPU: the NumPy model (tests/sc2_model.py) against a brute force and on planted
correspondences, the claim it is built on (RANSAC's cubic law), the C ABI of the entry point, and the Python layers."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import global_model as G
import sc2_model as M
from conftest import ROOT


# ---------------------------------------------------------------------------------------------------------------- the model
def _brute(src, tgt, corres, d_thr, seed_ratio, k1, k2):
    """steps 1 to 4 of include/gsr_hip.h in plain loops"""
    P = src.astype(np.float64)[corres[:, 0]]
    Q = tgt.astype(np.float64)[corres[:, 1]]
    m = len(corres)

    def ln(X, i, j):
        dx, dy, dz = X[i, 0] - X[j, 0], X[i, 1] - X[j, 1], X[i, 2] - X[j, 2]
        return math.sqrt((dx * dx + dy * dy) + dz * dz)
    Cm = [[1 if i != j and abs(ln(P, i, j) - ln(Q, i, j)) < d_thr else 0 for j in range(m)] for i in range(m)]
    deg = [sum(Cm[i]) for i in range(m)]
    n_seeds = min(math.ceil(seed_ratio * m), m)
    seeds = sorted(range(m), key=lambda i: (-deg[i], i))[:n_seeds]
    rows, K1, K2 = [], [], []
    for s in seeds:
        r = [0] * m
        for j in range(m):
            if Cm[s][j]:
                for k in range(m):
                    r[j] += Cm[s][k] * Cm[k][j]
        rows.append(r)
        a = [s] + sorted([j for j in range(m) if Cm[s][j]], key=lambda j: (-r[j], j))[: k1 - 1]
        l = {j: sum(Cm[j][k] for k in a) for j in a}
        b = [s] + sorted(a[1:], key=lambda j: (-l[j], j))[: k2 - 1]
        K1.append(a + [-1] * (M.KMAX - len(a)))
        K2.append(b + [-1] * (M.KMAX - len(b)))
    return np.array(Cm), np.array(deg), np.array(seeds), np.array(rows), np.array(K1), np.array(K2)


@pytest.mark.parametrize("kw", [dict(seed_ratio=0.2, k1=30, k2=20), dict(seed_ratio=1.0, k1=5, k2=3), dict(seed_ratio=0.5, k1=64, k2=64)])
def test_model_equals_a_brute_force(kw):
    src, tgt, corres, _ = M.planted(40, 0.5, seed=40)
    # lattice-like ties as well: a few repeated and a few exactly translated pairs
    corres[7] = corres[3]
    got = M.sc2(src, tgt, corres, 0.2, **kw)
    Cm, deg, seeds, rows, K1, K2 = _brute(src, tgt, corres, 0.2, kw["seed_ratio"], kw["k1"], kw["k2"])
    assert np.array_equal(got["C"], Cm) and np.array_equal(got["C"], got["C"].T) and not got["C"].diagonal().any()
    for name, want in (("deg", deg), ("seeds", seeds), ("rows", rows), ("K1", K1), ("K2", K2)):
        assert np.array_equal(got[name], want), name
    assert got["n_edges"] == Cm.sum() // 2 and got["n_seeds"] == len(seeds)
    assert (np.diff(deg[seeds]) <= 0).all() and rows.max() <= 40


@pytest.mark.parametrize("m,share,seed", [(257, 0.30, 1), (1000, 0.10, 2), (1000, 0.05, 3)])
def test_model_recovers_the_planted_pose(m, share, seed):
    src, tgt, corres, inl = M.planted(m, share, seed)
    r = M.sc2(src, tgt, corres, M.D_THR)
    rot, tr = M.pose_error(r["transformation"], M.T_PLANTED)
    print("m %d share %.2f: rotation error %.3f deg, translation error %.4f, fitness %.4f, winner rank %d, smallest s2/s1 %.3f" %
          (m, share, rot, tr, r["fitness"], r["best_seed"], r["sigma_ratio"][r["valid"]].min()))
    assert rot < 1.0 and tr < M.D_THR
    assert r["decided"] and len(r["undecided_seeds"]) == 0
    assert abs(r["fitness"] - share) < 0.01 and r["host_waits"] == 1 + r["refine_steps"] + (r["refine_steps"] < 20)
    # the model on its own terms
    d2 = M.d2_of(r["transformation"], src.astype(np.float64)[corres[:, 0]], tgt.astype(np.float64)[corres[:, 1]])
    assert r["fitness"] == (d2 < M.D_THR ** 2).sum() / m


def test_ransac_with_2000_hypotheses_fails_where_the_model_succeeds():
    """At 5 % inliers an all-inlier triple has probability 1.25e-4: 2000 hypotheses expect 0.25 of them."""
    src, tgt, corres, _ = M.planted(1000, 0.05, 3)
    r = G.ransac(src, tgt, corres, M.D_THR, max_iteration=2000, confidence=1.0)
    rot, tr = M.pose_error(r["transformation"], M.T_PLANTED)
    assert r["n_evaluated"] == 2000 and not (rot < 1.0 and tr < M.D_THR)
    assert r["fitness"] < 0.02


def test_model_empty_results():
    src, tgt, corres, _ = M.planted(40, 0.5, seed=1)
    for r in (M.sc2(src, tgt, corres[:2], 0.05), M.sc2(src, tgt, corres, 0.0), M.sc2(src, tgt, corres, -1.0)):
        assert np.array_equal(r["transformation"], np.eye(4)) and r["best_seed"] == -1 and r["best_index"] == -1 and r["fitness"] == 0.0
    far = M.sc2(src, tgt + np.float32(0), corres, 1e-9)          # nothing is compatible: no valid seed
    assert far["n_valid"] == 0 and far["best_seed"] == -1 and far["n_seeds"] == 8 and far["host_waits"] == 1


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _call(hip_lib, src, tgt, corres, m=None, ns=None, params=True, result=True, **kw):
    from gaussiansplattingregistration_amd import _lib, features
    d = dict(d_thr=0.05, seed_ratio=0.2, max_seeds=4096, k1=30, k2=20, refine_iters=20)
    d.update(kw)
    P = features._sc2_params(**d)
    R = _lib.Sc2Result()
    R.fitness, R.best_seed = 5.0, 7                              # the call must overwrite them
    p = lambda a: a.ctypes.data
    code = hip_lib.gsr_sc2_correspondence(p(src), len(src) if ns is None else ns, p(tgt), len(tgt), p(corres), len(corres) if m is None else m,
                                          C.byref(P) if params else None, C.byref(R) if result else None, 0, 0, None)
    return code, R


def test_entry_point_in_header_and_bindings(hip_lib):
    from gaussiansplattingregistration_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr_hip.h")).read(), flags=re.S)
    assert re.search(r"\bgsr_sc2_correspondence\s*\(", text) and "gsr_sc2_params" in text and "gsr_sc2_result" in text
    assert "gsr_sc2_correspondence" in _lib.SIGNATURES and hasattr(hip_lib, "gsr_sc2_correspondence")
    for hook in ("gsr_test_i8_gemm_nt", "gsr_test_sc2_stages"):
        assert hook in _lib.TEST_HOOKS and hook not in text and hasattr(hip_lib, hook)
    assert C.sizeof(_lib.Sc2Params) == 32 and C.sizeof(_lib.Sc2Result) == 192
    assert re.search(r"#define\s+GSR_SC2_MAX_CORRES\s+32768", text) and _lib.GSR_SC2_MAX_CORRES == 32768 and _lib.GSR_SC2_MAX_K == 64


def test_bad_arguments_are_invalid_and_degenerate_inputs_are_empty(hip_lib):
    """All of it is decided before the device is opened: the same with and without a GPU."""
    from gaussiansplattingregistration_amd import _lib
    src, tgt, corres, _ = M.planted(40, 0.5, seed=1)
    bad_row = corres.copy()
    bad_row[5, 1] = len(tgt)
    neg_row = corres.copy()
    neg_row[0, 0] = -1
    many = np.zeros((_lib.GSR_SC2_MAX_CORRES + 1, 2), np.int32)
    cases = [dict(params=False), dict(result=False), dict(m=-1), dict(ns=-1), dict(corres=bad_row), dict(corres=neg_row), dict(corres=many),
             dict(seed_ratio=0.0), dict(seed_ratio=1.5), dict(seed_ratio=float("nan")), dict(max_seeds=0), dict(k2=2), dict(k1=19, k2=20),
             dict(k1=65), dict(refine_iters=-1)]
    for kw in cases:
        args = dict(src=src, tgt=tgt, corres=corres)
        args.update(kw)
        code, R = _call(hip_lib, **args)
        assert code == _lib.GSR_E_INVALID, kw
        assert b"gsr_sc2_correspondence" in hip_lib.gsr_last_error(), kw
        if kw.get("result", True) and kw.get("params", True) and "m" not in kw and "ns" not in kw:
            assert R.best_seed == -1 and R.fitness == 0.0, kw      # the empty result stands behind an error
    # a parameter error wins over an empty input
    assert _call(hip_lib, src, tgt, corres, m=2, k2=2)[0] == _lib.GSR_E_INVALID
    for kw in (dict(m=2), dict(m=0), dict(d_thr=0.0), dict(d_thr=-1.0), dict(d_thr=float("nan"))):
        code, R = _call(hip_lib, src, tgt, corres, **kw)
        assert code == _lib.GSR_OK, kw
        assert np.array_equal(np.array(R.T[:]).reshape(4, 4), np.eye(4)) and R.fitness == 0.0 and R.inlier_rmse == 0.0
        assert (R.best_seed, R.best_index, R.n_seeds, R.n_valid, R.n_edges, R.refine_steps, R.host_waits) == (-1, -1, 0, 0, 0, 0, 0)


def test_a_real_call_needs_a_device(hip_lib):
    from gaussiansplattingregistration_amd import _lib
    src, tgt, corres, _ = M.planted(40, 0.5, seed=1)
    code, R = _call(hip_lib, src, tgt, corres)
    if hip_lib.gsr_device_count() <= 0:
        msg = hip_lib.gsr_last_error()
        assert code == _lib.GSR_E_NO_DEVICE and b"no HIP device" in msg and b"gsr_sc2_correspondence" in msg
        assert R.best_seed == -1 and R.fitness == 0.0
    else:
        assert code == _lib.GSR_OK and R.n_seeds == 8


# ---------------------------------------------------------------------------------------------------------------- the Python layers
def test_params_enum_and_shims():
    from gaussiansplattingregistration_amd import features
    from gaussiansplattingregistration_amd.controllers.registration_controller import RegistrationController
    from gaussiansplattingregistration_amd.params.registration_parameters import SC2RegistrationParams
    from gaussiansplattingregistration_amd.utils import global_registration_util as U
    from gaussiansplattingregistration_amd.workers.registrators import SC2Registrator
    p = SC2RegistrationParams()
    want = dict(voxel_size=0.05, mutual_filter=True, max_correspondence=0.075, seed_ratio=0.2, max_seeds=4096, k1=30, k2=20, refine_iterations=20)
    for k, v in want.items():
        assert getattr(p, k) == v and type(getattr(p, k)) is type(v), k
    assert list(p.__dataclass_fields__) == list(want)
    T = U.GlobalRegistrationType
    assert (T.RANSAC.value, T.FGR.value, T.SC2.value) == (0, 1, 2) and T.SC2.instance_name == "SC2" and len(T) == 3
    o = U.SC2Option()
    assert (o.seed_ratio, o.max_seeds, o.k1, o.k2, o.refine_iterations) == (0.2, 4096, 30, 20, 20)
    for f in (U.registration_sc2_based_on_correspondence, U.registration_sc2_based_on_feature_matching, U.do_sc2_registration,
              features.sc2_correspondence, RegistrationController.execute_sc2_registration_normal, SC2Registrator.run):
        assert callable(f)
    assert "sc2_correspondence" in features.__all__
    # a non-positive threshold is the empty result before anything is matched
    r = U.registration_sc2_based_on_feature_matching(None, None, None, None, True, 0.0)
    assert np.array_equal(r.transformation, np.eye(4)) and r.fitness == 0.0


def test_command_line_flags_are_declared():
    for name in ("register_ply.py", "register_many.py"):
        text = open(os.path.join(ROOT, "scripts", name)).read()
        assert re.search(r'method\.add_argument\("--global-sc2"', text), name
    assert "refused with --with-scaling" in open(os.path.join(ROOT, "scripts", "register_ply.py")).read()
