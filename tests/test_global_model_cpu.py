"""Global registration without a GPU: the C ABI of the new entry points, the RANSAC sampler of the library against the NumPy
restatement (tests/global_model.py), and sanity of the restatement itself."""
import ctypes as C
import os
import re

import numpy as np

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
