"""Consistent normal orientation without a GPU: the two CPU models against each other and against SciPy, the conditions the GPU
tests rest on, the C ABI's argument checks, and the host self-test of the round logic under the sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import orient_model as M
from conftest import ROOT

CASES = ["torus", "sheets", "chain", "junk", "sphere", "tiny1", "tiny2", "tiny3"]


@pytest.mark.parametrize("name", CASES)
def test_models_agree(name):
    c = M.gpu_cases()[name]
    a = M.kruskal_dfs(c["xyz"], c["normals"], c["nbr"], c["count"], c["reference"])
    b = M.expected(name)
    assert np.array_equal(a["flip"], b["flip"]) and np.array_equal(a["component"], b["component"])
    for k in ("n", "n_components", "n_flipped", "n_not_live"):
        assert a[k] == b[k], k
    assert b["rounds"] <= 31
    live = np.isfinite(c["normals"]).all(1)
    assert not a["flip"][~live].any()
    assert np.array_equal(a["component"][~live], np.flatnonzero(~live))
    # every vertex carries the lowest index of its component
    assert (a["component"] <= np.arange(a["n"])).all() and np.array_equal(a["component"][a["component"]], a["component"])


def test_models_agree_on_larger_tori():
    for n in (6000, 20000):
        c = M.torus_case(n, seed=n)
        a = M.kruskal_dfs(c["xyz"], c["normals"], c["nbr"], c["count"], c["reference"])
        b = M.boruvka(c["xyz"], c["normals"], c["nbr"], c["count"], c["reference"])
        assert np.array_equal(a["flip"], b["flip"]) and np.array_equal(a["component"], b["component"])


def test_rounds_and_components_of_the_cases():
    assert [M.expected(k)["rounds"] for k in ("torus", "sheets", "chain")] == [6, 5, 1]
    assert M.expected("torus")["n_components"] == 1 and M.expected("chain")["n_components"] == 1
    r = M.expected("sheets")
    assert sorted(np.unique(r["component"], return_counts=True)[1].tolist()) == [1, 1, 1599, 1600]
    c = M.gpu_cases()["sheets"]
    live = np.isfinite(c["normals"]).all(1)
    for s in (0, 1):                                                  # every weight ties at 0, and each sheet still has one sign
        assert np.unique(r["normals"][live & (c["sheet"] == s), 2]).size == 1
    assert M.expected("tiny1")["n_flipped"] == 1                      # a singleton follows the centroid rule
    assert M.expected("tiny2")["flip"].tolist() == [False, True]      # no reference: vertex 0 keeps its sign


def test_torus_is_oriented_exactly():
    """A condition on the input, asserted on the model: against the noiseless normals the result is all-outward or all-inward."""
    c, r = M.gpu_cases()["torus"], M.expected("torus")
    s = (r["normals"] * c["outward"]).sum(1)
    assert (s > 0).all() or (s < 0).all()


def test_centroid_rule_splits_the_torus():
    """Why the feature exists: the centroid rule alone puts at least 30 % of a torus's normals on each side."""
    c = M.gpu_cases()["torus"]
    p = c["xyz"].astype(np.float64)
    towards = ((c["reference"] - p) * c["outward"]).sum(1) > 0         # the outward normal already looks at the centroid
    assert 0.3 <= towards.mean() <= 0.7, towards.mean()


@pytest.mark.parametrize("name", ["torus", "sheets", "junk", "tiny3"])
def test_labels_are_scipy_connected_components(name):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    c, r = M.gpu_cases()[name], M.expected(name)
    n = r["n"]
    _, lo, hi, _, _ = M.edges_from_lists(c["normals"], c["nbr"], c["count"])
    k, lab = connected_components(coo_matrix((np.ones(lo.size), (lo, hi)), shape=(n, n)), directed=False)
    assert k == r["n_components"]
    pairs = np.unique(np.stack([lab, r["component"]], 1), axis=0)      # equal up to renaming: a bijection between the label sets
    assert pairs.shape[0] == k and np.unique(pairs[:, 0]).size == k and np.unique(pairs[:, 1]).size == k


def test_sphere_vote_is_not_near_a_tie():
    c = M.gpu_cases()["sphere"]
    r = M.boruvka(c["xyz"], c["normals"], c["nbr"], c["count"], None)
    assert r["n_components"] == 1
    t = ((c["reference"] - c["xyz"].astype(np.float64)) * r["normals"]).sum(1)
    toward, away = int((t > 0).sum()), int((t < 0).sum())
    assert abs(toward - away) > 0.1 * (toward + away), (toward, away)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def _args(n=8):
    rng = np.random.default_rng(0)
    a = {"xyz": rng.random((n, 3)).astype(np.float32), "nrm": np.tile([0.0, 0.0, 1.0], (n, 1)), "nbr": np.zeros((n, 2), np.int32),
         "cnt": np.full(n, 2, np.int32), "ref": np.array([0.5, 0.5, 0.5]), "comp": np.zeros(n, np.int32)}
    return a, (lambda x: None if x is None else x.ctypes.data)


def _graph(L, a, p, R, n=8, stride=2, **over):
    g = dict(a, **over)
    return L.gsr_orient_normals_graph(p(g["xyz"]), p(g["nrm"]), n, p(g["nbr"]), stride, p(g["cnt"]), p(g["ref"]), p(g["comp"]), C.addressof(R), 0, 0, None)


def _search(L, a, p, R, n=8, radius=0.5, max_nn=4, **over):
    g = dict(a, **over)
    return L.gsr_orient_normals(p(g["xyz"]), p(g["nrm"]), n, radius, max_nn, p(g["ref"]), p(g["comp"]), C.addressof(R), 0, 0, None)


def test_abi_symbols_and_no_device(hip_lib):
    from gaussiansplattingregistration_amd import _lib
    assert hasattr(hip_lib, "gsr_orient_normals_graph") and hasattr(hip_lib, "gsr_orient_normals")
    assert C.sizeof(_lib.OrientReport) == 64
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    a, p = _args()
    R = _lib.OrientReport()
    for name, call in (("gsr_orient_normals_graph", _graph), ("gsr_orient_normals", _search)):
        assert call(hip_lib, a, p, R) == _lib.GSR_E_NO_DEVICE
        msg = hip_lib.gsr_last_error()
        assert b"no HIP device" in msg and name.encode() in msg, msg
    from gaussiansplattingregistration_amd import orient
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        orient.orient_normals(a["xyz"], a["nrm"], 0.5, 4)


def test_abi_invalid_arguments(hip_lib):
    """Every argument check judges on the host and runs before the device check: the codes are the same with and without a GPU."""
    from gaussiansplattingregistration_amd import _lib
    a, p = _args()
    R = _lib.OrientReport()
    nan_ref, inf_ref = np.array([0.0, np.nan, 0.0]), np.array([np.inf, 0.0, 0.0])
    bad_graph = [dict(n=-1), dict(n=2 ** 31), dict(stride=0), dict(stride=-3), dict(nrm=None), dict(nbr=None), dict(cnt=None), dict(xyz=None),
                 dict(ref=nan_ref), dict(ref=inf_ref), dict(n=2 ** 29, stride=2)]
    for kw in bad_graph:
        assert _graph(hip_lib, a, p, R, **kw) == _lib.GSR_E_INVALID, kw
        assert b"gsr_orient_normals_graph" in hip_lib.gsr_last_error()
    bad_search = [dict(n=-1), dict(n=2 ** 31), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
                  dict(max_nn=0), dict(max_nn=1025), dict(max_nn=513), dict(nrm=None), dict(xyz=None), dict(xyz=None, ref=None), dict(ref=nan_ref)]
    for kw in bad_search:
        assert _search(hip_lib, a, p, R, **kw) == _lib.GSR_E_INVALID, kw
        assert b"gsr_orient_normals:" in hip_lib.gsr_last_error()
    # an empty cloud is valid and needs no device: GSR_OK and a zero report
    R.n, R.n_components, R.rounds = 5, 5, 5
    assert _graph(hip_lib, a, p, R, n=0) == _lib.GSR_OK and (R.n, R.n_components, R.n_flipped, R.n_not_live, R.rounds) == (0, 0, 0, 0, 0)
    assert _search(hip_lib, a, p, R, n=0) == _lib.GSR_OK
    assert hip_lib.gsr_orient_normals_graph(None, None, 0, None, 1, None, None, None, None, 0, 0, None) == _lib.GSR_OK


def test_python_surface_without_a_gpu():
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.utils import global_registration_util as U
    a, _ = _args()
    with pytest.raises(ValueError, match="finite radius"):
        PointCloud(xyz32=a["xyz"], normals=a["nrm"]).orient_normals_consistent_tangent_plane(8)
    with pytest.raises(RuntimeError, match="No normals"):
        PointCloud(xyz32=a["xyz"]).orient_normals_consistent_tangent_plane(8, radius=0.5)
    with pytest.raises(ValueError, match="orient must be"):
        U.preprocess_point_cloud(PointCloud(xyz32=a["xyz"]), 0.1, orient="camera")


def test_selftest_is_clean_under_the_host_sanitizers(tmp_path):
    """scripts/orient_selftest.cpp: the steps of csrc/gsr_orient.h run serially against Kruskal + DFS on random graphs with ties,
    duplicates, self entries, entries out of range and deep chains, built with AddressSanitizer and UBSan."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "orient_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "scripts", "orient_selftest.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
