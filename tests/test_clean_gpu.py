"""Floater removal on the GPU against the float64 model of tests/clean_model.py: the mask EXACTLY the model's, the mean distances
within (k + 2) 2^-52 relative (one ulp per sqrt were the device's not correctly rounded, half an ulp per addition on either side),
the counts and the report exact; row selection bit-equal to NumPy boolean indexing."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import clean_model as M
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(hip_lib):
    assert torch.cuda.is_available()
    return torch


def _params(kw):
    from gaussiansplattingregistration_amd.params.clean_parameters import CleanParams
    return CleanParams(nb_neighbors=kw.get("nb_neighbors", 20), std_ratio=kw.get("std_ratio", 2.0), radius=kw.get("radius", 0.0),
                       nb_points=kw.get("nb_points", 16))


def _run(name, on_device=False, torch=None):
    """the library's answer for a case of clean_model.gpu_cases(): host arrays, or tensors on cuda:0"""
    from gaussiansplattingregistration_amd import clean
    xyz, kw, _ = M.gpu_cases()[name]
    P = _params(kw)
    op, sc = kw.get("raw_opacity"), kw.get("scaling")
    if name == "gates":
        g = M.gates_case()
        P.min_opacity, P.max_extent = g["min_opacity"], g["max_extent"]
        assert P.min_raw_opacity == kw["min_raw_opacity"] and P.max_log_scale == kw["max_log_scale"]
    if on_device:
        dev = lambda a: None if a is None else torch.as_tensor(a, device="cuda:0")
        xyz, op, sc = dev(xyz), dev(op), dev(sc)
    mask, info = clean.outlier_mask(xyz, P, raw_opacity=op, scaling=sc, with_mean_dist=True, with_count=True)
    if on_device:
        mask, info["mean_dist"], info["count"] = mask.cpu().numpy(), info["mean_dist"].cpu().numpy(), info["count"].cpu().numpy()
    return mask, info


def _check(name, mask, info):
    xyz, kw, _ = M.gpu_cases()[name]
    want = M.model_of(name)
    k = kw.get("nb_neighbors", 20)
    assert mask.dtype == np.uint8 and np.array_equal(mask, want["mask"]), (name, np.flatnonzero(mask != want["mask"])[:10])
    for key in ("n_nonfinite", "n_gate_opacity", "n_gate_scale", "n_statistical", "n_radius", "n_kept"):
        assert info[key] == want[key], (name, key, info[key], want[key])
    assert info["n"] == len(xyz)
    got, ref = info["mean_dist"], want["mean_dist"]
    assert np.array_equal(got == -1, ref == -1)
    reached = ref >= 0
    err = float(np.max(np.abs(got[reached] - ref[reached]) / np.maximum(ref[reached], 1e-300))) if reached.any() and k >= 1 else 0.0
    print(f"clean[{name}]: n {len(xyz)} kept {info['n_kept']} deferred {info['deferred_queries']} max relative mean_dist error {err:.3g} "
          f"(bound {(k + 2) * 2.0 ** -52:.3g}) threshold {info['threshold']!r} model {want['threshold']!r}")
    assert err <= (k + 2) * 2.0 ** -52
    assert np.array_equal(info["count"], want["count"])
    if k >= 1 and math.isfinite(want["threshold"]):
        assert abs(info["threshold"] - want["threshold"]) <= 1e-12 * want["threshold"]
        assert abs(info["cloud_mean"] - want["cloud_mean"]) <= 1e-12 * want["cloud_mean"]
    elif k >= 1:
        assert math.isnan(info["threshold"])


def test_base(gpu):
    """exact mask; host arrays and device tensors give the same bits; two runs give the same bits"""
    mask, info = _run("base")
    _check("base", mask, info)
    assert mask[:M.N_CORE].all() and not mask[M.N_CORE:].any()
    mask_d, info_d = _run("base", on_device=True, torch=gpu)
    mask_2, info_2 = _run("base")
    for m, i in ((mask_d, info_d), (mask_2, info_2)):
        assert np.array_equal(m, mask)
        assert i["mean_dist"].tobytes() == info["mean_dist"].tobytes() and np.array_equal(i["count"], info["count"])
        for key in ("cloud_mean", "std_dev", "threshold"):
            assert np.float64(i[key]).tobytes() == np.float64(info[key]).tobytes(), key


def test_far(gpu):
    """floaters at 10^6 box radii: queries that leave the lane-per-query walk; the workspace does not depend on how many"""
    mask, info = _run("far")
    _check("far", mask, info)
    assert info["deferred_queries"] > 0
    _, base = _run("base")
    assert info["workspace_bytes"] == base["workspace_bytes"]


@pytest.mark.parametrize("name", ["clustered", "lattice_1", "lattice_next", "nonfinite", "gates", "base_radius"] + [f"small_{n}" for n in M.SMALL_N] +
                         [f"duplicates_{k}" for k in M.DUP_K])
def test_case(gpu, name):
    mask, info = _run(name)
    _check(name, mask, info)
    if name == "lattice_1":
        assert info["n_kept"] == 0
    if name == "lattice_next":
        assert info["n_kept"] == 64
    if name == "small_1":
        assert info["n_kept"] == 0 and math.isnan(info["threshold"])
    if name == "nonfinite":
        assert info["n_nonfinite"] == len(M.nonfinite_case()["rows"])
    if name == "gates":
        assert mask[M.gates_case()["p_row"]] == 0                            # gated rows are not neighbours
    if name.startswith("duplicates"):
        assert not mask[2000:2040].any() and (info["mean_dist"][2000:2040] == 0).all()


def test_clustered_on_device_tensors(gpu):
    mask, info = _run("clustered", on_device=True, torch=gpu)
    _check("clustered", mask, info)


def _random_view(n, K, sr, seed):
    rng = np.random.default_rng(seed)
    width = {"xyz": 3, "cov6": 6, "dc": 3, "sh": 3 * K, "opacity": 1, "scaling": 3, "rot": 4}
    arrays = {}
    for name, w in width.items():
        if w == 0 or (name in ("scaling", "rot") and not sr):
            continue
        a = rng.normal(size=(n, w)).astype(np.float32)
        a.view(np.uint32)[rng.integers(0, n, 20), rng.integers(0, w, 20)] = rng.integers(0, 2 ** 32, 20, dtype=np.uint64).astype(np.uint32)   # any bit pattern, NaNs included
        arrays[name] = a if w > 1 else a.reshape(n)
    return arrays


@pytest.mark.parametrize("K", [0, 15])
@pytest.mark.parametrize("sr", [False, True])
def test_select(gpu, K, sr):
    from gaussiansplattingregistration_amd import clean
    n = 1000
    arrays = _random_view(n, K, sr, seed=K + sr)
    rng = np.random.default_rng(3)
    for mask in (rng.integers(0, 2, n).astype(np.uint8), np.zeros(n, np.uint8), np.ones(n, np.uint8), (rng.integers(0, 2, n) * 255).astype(np.uint8)):
        for on_device in (False, True):
            if on_device:
                sel, index = clean.select_rows({k: gpu.as_tensor(v, device="cuda:0") for k, v in arrays.items()}, gpu.as_tensor(mask, device="cuda:0"))
                sel, index = {k: v.cpu().numpy() for k, v in sel.items()}, index.cpu().numpy()
            else:
                sel, index = clean.select_rows(arrays, mask)
            keep = mask != 0
            assert index.dtype == np.int32 and np.array_equal(index, np.flatnonzero(keep))
            assert sorted(sel) == sorted(arrays)
            for name, a in arrays.items():
                assert sel[name].shape == a[keep].shape
                assert sel[name].tobytes() == a[keep].tobytes(), name           # bit for bit


def test_select_capacity(gpu, hip_lib):
    """more kept rows than the output holds: GSR_E_INVALID, n_out says how many, nothing behind the capacity is written"""
    import ctypes as C
    from gaussiansplattingregistration_amd import _lib
    n, cap = 100, 10
    xyz = np.random.default_rng(0).random((n, 3)).astype(np.float32)
    out = np.full((cap + 5, 3), -7.0, np.float32)
    mask = np.ones(n, np.uint8)
    vin, vout = _lib.ModelView(), _lib.ModelView()
    vin.n, vin.xyz, vout.n, vout.xyz = n, xyz.ctypes.data, cap, out.ctypes.data
    n_out = C.c_int64(0)
    rc = hip_lib.gsr_model_select(C.addressof(vin), 0, mask.ctypes.data, C.addressof(vout), None, C.byref(n_out), 0, 0, None)
    assert rc == _lib.GSR_E_INVALID and n_out.value == n and (out == -7.0).all()
    mask[cap:] = 0
    rc = hip_lib.gsr_model_select(C.addressof(vin), 0, mask.ctypes.data, C.addressof(vout), None, C.byref(n_out), 0, 0, None)
    assert rc == 0 and n_out.value == cap and vout.n == cap and np.array_equal(out[:cap], xyz[:cap]) and (out[cap:] == -7.0).all()


def _floater_model(torch, n=3000, n_float=30, device="cuda:0"):
    """synth.make_cloud(3000) + 30 floaters at 5 - 50 box radii, as a GaussianModel with scaling / rotation"""
    from gaussiansplattingregistration_amd import synth
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    c = synth.make_cloud(n, seed=4, sh_degree=3)
    rng = np.random.default_rng(9)
    xyz = c["xyz"].copy()
    lo, hi = xyz.min(0), xyz.max(0)
    ctr, rad = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    dirs = rng.normal(size=(n_float, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rows = rng.choice(n, n_float, replace=False)
    xyz[rows] = (ctr + dirs * rng.uniform(5, 50, (n_float, 1)) * rad).astype(np.float32)
    m = GaussianModel(device).from_arrays(xyz, c["color"], c["opacity"], c["cov6"], c["sh"], 3)
    m._scaling = torch.as_tensor(rng.normal(-3.0, 0.5, (n, 3)).astype(np.float32), device=device)
    q = rng.normal(size=(n, 4)).astype(np.float32)
    m._rotation = torch.as_tensor(q / np.linalg.norm(q, axis=1, keepdims=True), device=device)
    return m, rows


_NAMES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_covariance")


def test_model(gpu):
    from gaussiansplattingregistration_amd.params.clean_parameters import CleanParams
    m, rows = _floater_model(gpu)
    P = CleanParams(nb_neighbors=20, std_ratio=2.0)
    cleaned, info = m.remove_floaters(P)
    want = M.outlier_model(m._xyz.cpu().numpy(), nb_neighbors=20, std_ratio=2.0)
    assert want["margin_stat"] >= 1e-9
    assert info["n_kept"] == want["n_kept"] == len(cleaned) and not want["mask"][rows].any()
    ref = m.select_by_mask(gpu.as_tensor(want["mask"], device="cuda:0"))
    keep = want["mask"] != 0
    assert cleaned.sh_degree == m.sh_degree == ref.sh_degree
    for name in _NAMES:
        a, b, src = getattr(cleaned, name), getattr(ref, name), getattr(m, name)
        assert a.is_cuda and a.shape == b.shape == (int(keep.sum()),) + tuple(src.shape[1:]), name
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == src.cpu().numpy()[keep].tobytes(), name
    assert len(m) == 3000                                                       # the model itself is left as it was


def test_point_cloud_methods(gpu):
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    xyz, kw, _ = M.gpu_cases()["base"]
    want = M.model_of("base")
    nrm = np.random.default_rng(2).normal(size=(len(xyz), 3))
    for dev in (False, True):
        pc = PointCloud(gpu.as_tensor(xyz, device="cuda:0") if dev else xyz, normals=gpu.as_tensor(nrm, device="cuda:0") if dev else nrm)
        out, index = pc.remove_statistical_outlier(20, 2.0)
        host = lambda a: a.cpu().numpy() if dev else a
        assert (gpu.is_tensor(out.xyz32) and out.xyz32.is_cuda) == dev
        assert np.array_equal(host(index), np.flatnonzero(want["mask"])) and np.array_equal(host(out.xyz32), xyz[want["mask"] != 0])
        assert np.array_equal(host(out.normals), nrm[want["mask"] != 0])
        inv = pc.select_by_index(index, invert=True)
        assert np.array_equal(host(inv.xyz32), xyz[want["mask"] == 0])
    wr = M.model_of("lattice_next")
    out, index = PointCloud(M.lattice_cloud()).remove_radius_outlier(6, float(np.nextafter(1.0, 2.0)))
    assert np.array_equal(index, np.flatnonzero(wr["mask"])) and len(out) == 64


def test_cli(gpu, tmp_path):
    """scripts/clean_ply.py: the output reads back with n_kept rows, bit-equal to the selection"""
    from gaussiansplattingregistration_amd.utils import ply_io
    m, rows = _floater_model(gpu, device="cpu")
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    m.save_ply(src)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "clean_ply.py"), src, "--out", dst, "--clean-knn", "20", "--clean-std", "2.0"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = ply_io.load_gaussian_arrays(src), ply_io.load_gaussian_arrays(dst)
    want = M.outlier_model(a["xyz"], nb_neighbors=20, std_ratio=2.0)
    keep = want["mask"] != 0
    assert f"{len(keep)} -> {int(keep.sum())} splats" in r.stdout, r.stdout
    assert not keep[rows].any()
    for name in ("xyz", "color", "opacity", "sh", "scale", "rot"):
        assert b[name].shape[0] == keep.sum() and b[name].tobytes() == a[name][keep].tobytes(), name
