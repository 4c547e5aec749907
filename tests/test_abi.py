"""The C-ABI library: loads without a GPU, exports every symbol include/gsr_hip.h declares, and the
product path fails loudly (no CPU fallback) when no device is visible."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _declared_symbols(path=("include", "gsr_hip.h")):
    text = open(os.path.join(ROOT, *path)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)) - {"gsr_allreduce_fn"})


def test_header_symbols_all_exported(hip_lib):
    from gaussiansplattingregistration_amd import _lib
    syms = _declared_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(hip_lib, s), f"{s} declared in include/gsr_hip.h but not exported"
    # and the Python binding table covers exactly the header
    assert sorted(_lib.SIGNATURES) == syms
    # the private test hooks live in their own header and binding table
    assert not any(s.startswith("gsr_debug") for s in syms)
    hooks = _declared_symbols(("gaussiansplattingregistration_amd", "csrc", "gsr_test_hooks.h"))
    assert sorted(_lib.TEST_HOOKS) == hooks
    for s in hooks:
        assert hasattr(hip_lib, s)


def test_version_and_no_device_behaviour(hip_lib):
    assert b"gfx950" in hip_lib.gsr_version()
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    assert hip_lib.gsr_device_count() == 0
    h = C.c_void_p()
    assert hip_lib.gsr_hem_create(C.byref(h), 0, None) == -3          # GSR_E_NO_DEVICE
    assert b"no HIP device" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_icp_create(C.byref(h), 0, None) == -3
    from gaussiansplattingregistration_amd import hem, icp
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hem.HemMixture()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        icp.IcpContext()
    with pytest.raises(RuntimeError):
        icp.normals_from_cov(np.zeros((3, 6), np.float32))


def _one_shot_calls():
    """name -> call(L) of every stateless entry point, with small valid non-empty host arrays (device 0, null stream)"""
    from gaussiansplattingregistration_amd import _lib
    n = 8
    rng = np.random.default_rng(0)
    xyz = rng.random((n, 3)).astype(np.float32)
    nrm32 = np.tile(np.float32([0, 0, 1]), (n, 1))
    nrm64 = nrm32.astype(np.float64)
    cov32 = np.tile(np.float32([1, 0, 0, 1, 0, 1]), (n, 1))
    feat = rng.random((n, 33))
    p = lambda a: a.ctypes.data
    keep = []                                   # the output arrays, alive as long as the calls

    def zeros(dtype):
        def make(*shape):
            keep.append(np.zeros(shape, dtype))
            return p(keep[-1])
        return make
    f32, f64, i32 = zeros(np.float32), zeros(np.float64), zeros(np.int32)
    cands = np.tile(np.float32([0, 0, 1, 0, 0, 0, 1, 1]), (2, 1))
    best, nv, nc, um, h = C.c_int32(-1), C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_void_p()
    offsets = (C.c_int32 * 15)(*[4 * i for i in range(15)])
    corres = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    P, R = _lib.RansacParams(), _lib.RansacResult()
    P.kind, P.ransac_n, P.max_corr, P.max_iteration, P.confidence, P.batch = 0, 3, 0.5, 10, 0.999, 8
    return {
        "gsr_plane_score": lambda L: L.gsr_plane_score(p(xyz), p(nrm32), n, p(cands), 2, 0.1, 0.5, i32(2), i32(n), C.byref(best), 0, 0, None),
        "gsr_decompose_cov": lambda L: L.gsr_decompose_cov(p(cov32), n, _lib.GSR_DECOMP_EXACT, f32(n, 3), f32(n, 4), f32(n, 9), 0, 0, None),
        "gsr_ply_unpack": lambda L: L.gsr_ply_unpack(f32(n, 15), n, 60, offsets, 0, f32(n, 3), f32(n, 3), None, f32(n), f32(n, 3), f32(n, 4),
                                                     f32(n, 6), 0, None),
        "gsr_normals_from_cov": lambda L: L.gsr_normals_from_cov(p(cov32), n, f64(n, 3), 0, 0, None),
        "gsr_cov_from_normals": lambda L: L.gsr_cov_from_normals(p(nrm64), n, 1e-3, f64(n, 6), 0, 0, None),
        "gsr_normals_knn": lambda L: L.gsr_normals_knn(p(xyz), n, 5, f64(n, 3), 0, 0, None),
        "gsr_voxel_down_sample": lambda L: L.gsr_voxel_down_sample(0, None, p(xyz), None, None, n, 0.25, 0, C.byref(h), C.byref(nv)),
        "gsr_hybrid_search": lambda L: L.gsr_hybrid_search(p(xyz), n, 0.5, 4, i32(n, 4), i32(n), 0, 0, None),
        "gsr_fpfh": lambda L: L.gsr_fpfh(p(xyz), p(nrm64), n, 0.5, 4, f64(n, 33), 0, 0, None),
        "gsr_feature_match": lambda L: L.gsr_feature_match(p(feat), n, p(feat), n, 0, 3, i32(n, 2), C.byref(nc), C.byref(um), None, None, 0, 0, None),
        "gsr_ransac_correspondence": lambda L: L.gsr_ransac_correspondence(p(xyz), n, p(xyz), n, None, None, p(corres), n, C.byref(P), C.byref(R),
                                                                           0, 0, None),
    }


ONE_SHOT_ENTRY_POINTS = ["gsr_plane_score", "gsr_decompose_cov", "gsr_ply_unpack", "gsr_normals_from_cov", "gsr_cov_from_normals", "gsr_normals_knn",
                         "gsr_voxel_down_sample", "gsr_hybrid_search", "gsr_fpfh", "gsr_feature_match", "gsr_ransac_correspondence"]


@pytest.mark.parametrize("name", ONE_SHOT_ENTRY_POINTS)
def test_one_shot_entry_points_without_a_device(hip_lib, name):
    """Every stateless entry point goes through the same device check: valid host arrays and no visible device give
    GSR_E_NO_DEVICE and a message that names the function."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    calls = _one_shot_calls()
    assert sorted(calls) == sorted(ONE_SHOT_ENTRY_POINTS)
    assert calls[name](hip_lib) == -3                                  # GSR_E_NO_DEVICE
    msg = hip_lib.gsr_last_error()
    assert b"no HIP device" in msg and name.encode() in msg, msg


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: no module of the product package may reference it."""
    pkg = os.path.join(ROOT, "gaussiansplattingregistration_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(d, f)).read()
                assert "from oracle" not in text and "import oracle" not in text and "libgsr_oracle" not in text, f


def test_host_solve_matches_oracle_umeyama(hip_lib, oracle):
    """gsr_icp_solve is pure host code: feed it exact sums and compare with the oracle's one-iteration update."""
    rng = np.random.default_rng(0)
    p = rng.normal(size=(500, 3))
    from gaussiansplattingregistration_amd.synth import rigid_transform
    T = rigid_transform(7.0, (0.2, 1.0, -0.4), (0.03, -0.02, 0.05))
    q = p @ T[:3, :3].T + T[:3, 3]
    ctr = np.array([0.1, -0.2, 0.3])
    acc = np.zeros(32)
    a, b = p - ctr, q - ctr
    acc[0] = len(p)
    acc[2:5], acc[5:8] = a.sum(0), b.sum(0)
    acc[8:17] = (a[:, :, None] * b[:, None, :]).sum(0).reshape(-1)
    upd = np.zeros((4, 4))
    assert hip_lib.gsr_icp_solve(acc.ctypes.data, 0, ctr.ctypes.data, upd.ctypes.data) == 0
    assert np.linalg.norm(upd - T) < 1e-12
    # point-to-plane: exact normal equations of a small known motion
    n = rng.normal(size=(500, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    r = ((p - q) * n).sum(1)
    J = np.hstack([np.cross(p, n), n])
    JTJ, JTr = J.T @ J, J.T @ r
    acc = np.zeros(32)
    acc[0] = len(p)
    acc[2:23] = JTJ[np.triu_indices(6)]
    acc[23:29] = JTr
    assert hip_lib.gsr_icp_solve(acc.ctypes.data, 1, None, upd.ctypes.data) == 0
    x = np.linalg.solve(JTJ, -JTr)
    assert np.allclose(upd[:3, 3], x[3:], atol=1e-12)
    assert abs(np.linalg.det(upd[:3, :3]) - 1) < 1e-12


def test_wrong_rccl_library_is_an_error_not_a_crash(hip_lib):
    """a dlopen candidate that fails must yield GSR_E_HIP with dlopen's message (it used to assign a
    std::string from the NULL a second dlerror() returns).  Fresh process: the library handle is cached per process."""
    import subprocess
    import sys
    code = (
        "import ctypes as C, sys\n"
        "sys.path.insert(0, %r)\n"
        "from gaussiansplattingregistration_amd import _lib\n"
        "lib = _lib.load()\n"
        "buf = (C.c_char * 128)()\n"
        "rc = lib.gsr_comm_get_unique_id(buf)\n"
        "msg = lib.gsr_last_error()\n"
        "assert rc == -2, rc\n"                                   # GSR_E_HIP
        "assert b'not available' in msg and b'no_such_rccl' in msg, msg\n"
        "h = C.c_void_p()\n"
        "rc = lib.gsr_comm_create(C.byref(h), buf, 0, 1, 0)\n"
        "assert rc == -2 and not h.value, rc\n"
        "print('ok')\n" % ROOT)
    env = dict(os.environ, GSR_RCCL_LIB="/tmp/no_such_rccl.so")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
