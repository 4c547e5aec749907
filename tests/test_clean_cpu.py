"""Floater removal without a GPU: the cases the GPU tests run are far from any decision rounding could turn, the model has the
properties the feature is for, and the two entry points check their arguments before they look for a device."""
import ctypes as C
import math

import numpy as np
import pytest

import clean_model as M

CASES = sorted(M.gpu_cases())


@pytest.mark.parametrize("name", CASES)
def test_gpu_cases_are_unambiguous(name):
    """The device reduces the two moments in another order than NumPy: two float64 summation orders of ~4000 positive terms differ
    by ~1e-15 relative, so a margin of 1e-9 between every mean distance and the threshold is six orders above what could turn a
    verdict.  d2 itself is computed identically on both sides (float64, left to right, no contraction), so the radius stage has no
    rounding to be ambiguous about; its margin is asserted wherever the coordinates are not integers (the lattice sits ON radius^2 on
    purpose: integer coordinates make every d2 exact).  An ambiguous case gets another seed, it is never excluded."""
    xyz, kw, exact = M.gpu_cases()[name]
    r = M.model_of(name)
    print(f"{name}: n {len(xyz)} kept {r['n_kept']} threshold {r['threshold']:.6g} margin_stat {r['margin_stat']:.3g} margin_radius {r['margin_radius']:.3g}")
    assert r["margin_stat"] >= 1e-9
    if exact:
        assert np.array_equal(xyz, np.round(xyz)) and np.abs(xyz).max() < 1024
    else:
        assert r["margin_radius"] >= 1e-9


def test_base_floaters_are_all_dropped():
    r = M.model_of("base")
    assert r["mask"][:M.N_CORE].all() and not r["mask"][M.N_CORE:].any()
    assert abs(r["threshold"] - 5.3236) < 1e-4 and r["margin_stat"] > 1e-2
    r = M.model_of("far")
    assert r["mask"][:M.N_CORE].all() and not r["mask"][M.N_CORE:].any()
    r = M.model_of("clustered")
    assert r["mask"][:3000].all() and not r["mask"][3000:].any() and r["margin_stat"] > 0.29


def test_lattice_strictness():
    r1, r2 = M.model_of("lattice_1"), M.model_of("lattice_next")
    assert r1["n_kept"] == 0 and (r1["count"] == 1).all()                       # strict: the six unit neighbours sit ON the radius
    assert r2["n_kept"] == 64 and np.bincount(r2["count"]).tolist() == [0, 0, 0, 0, 8, 48, 96, 64]      # > nb_points = 6: only the interior


def test_second_call_is_not_the_identity():
    """Cleaning is not idempotent: the survivors have a smaller mean and deviation, so a second identical call drops rows the first
    one kept.  (Iterated cleaning is out of scope; this documents why a caller must not expect a fixed point.)"""
    xyz, kw, _ = M.gpu_cases()["base"]
    r = M.model_of("base")
    kept = xyz[r["mask"] != 0]
    r2 = M.outlier_model(kept, **kw)
    assert r2["n_kept"] < len(kept)
    assert r2["threshold"] < r["threshold"]


def test_permutation_invariance():
    xyz, kw, _ = M.gpu_cases()["base"]
    r = M.model_of("base")
    perm = np.random.default_rng(5).permutation(len(xyz))
    rp = M.outlier_model(xyz[perm], **kw)
    assert np.array_equal(rp["mask"], r["mask"][perm])
    assert np.array_equal(rp["mean_dist"], r["mean_dist"][perm])              # the k' smallest d2 in ascending order: no index enters


def test_stage_order_in_the_model():
    g = M.gates_case()
    xyz, kw, _ = M.gpu_cases()["gates"]
    r = M.model_of("gates")
    assert r["stage"][g["p_row"]] == 4                                          # its only near neighbours are gated out: isolated
    assert (r["stage"][g["p_row"] + 1:] == 2).all()
    assert (r["stage"][0:10] == 2).all() and r["stage"][5] == 2                 # row 5 fails both gates: the first one counts it
    assert (r["stage"][10:30] != 2).all() and (r["stage"][10:30] != 3).all()
    assert (r["stage"][30:40] == 3).all() and r["stage"][40] == 2 and r["stage"][41] == 3
    assert (r["mean_dist"][r["stage"] == 2] == -1).all() and (r["mean_dist"][r["stage"] == 3] == -1).all()
    ungated = M.outlier_model(xyz, **dict(kw, min_raw_opacity=-math.inf))
    assert ungated["mask"][g["p_row"]] == 1
    r = M.model_of("duplicates_20")
    assert (r["mean_dist"][2000:2040] == 0).all() and not r["mask"][2000:2040].any()
    r = M.model_of("nonfinite")
    assert r["n_nonfinite"] == len(M.nonfinite_case()["rows"]) and not r["mask"][M.nonfinite_case()["rows"]].any()


def test_clean_params_validation():
    from gaussiansplattingregistration_amd.params.clean_parameters import CleanParams
    p = CleanParams()
    assert (p.min_opacity, p.max_extent, p.nb_neighbors, p.std_ratio, p.radius, p.nb_points) == (0.0, math.inf, 20, 2.0, 0.0, 16)
    assert p.min_raw_opacity == -math.inf and p.max_log_scale == math.inf
    assert CleanParams(min_opacity=0.1).min_raw_opacity == M.logit(0.1) and CleanParams(max_extent=0.5).max_log_scale == math.log(0.5)
    for bad in (dict(nb_neighbors=33), dict(nb_neighbors=-1), dict(std_ratio=0.0), dict(std_ratio=-1.0), dict(std_ratio=math.nan), dict(min_opacity=1.0),
                dict(min_opacity=-0.1), dict(max_extent=0.0), dict(radius=-1.0), dict(radius=math.inf), dict(nb_points=-1), dict(nb_neighbors=2.5)):
        with pytest.raises(ValueError):
            CleanParams(**bad)
    CleanParams(nb_neighbors=0, std_ratio=0.0)                                  # the stage is off: its ratio is not looked at


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------

def _params(_lib, **kw):
    d = dict(min_raw_opacity=-math.inf, max_log_scale=math.inf, nb_neighbors=20, std_ratio=2.0, radius=0.0, nb_points=16)
    d.update(kw)
    return _lib.CleanParams(d["min_raw_opacity"], d["max_log_scale"], d["nb_neighbors"], 0, d["std_ratio"], d["radius"], d["nb_points"], 0)


def _mask_call(L, _lib, n=8, opacity=False, scaling=False, **kw):
    xyz = np.random.default_rng(0).random((n, 3)).astype(np.float32)
    op = np.zeros(n, np.float32) if opacity else None
    sc = np.zeros((n, 3), np.float32) if scaling else None
    mask = np.zeros(n, np.uint8)
    P, R = _params(_lib, **kw), _lib.CleanReport()
    rc = L.gsr_outlier_mask(xyz.ctypes.data, op.ctypes.data if opacity else None, sc.ctypes.data if scaling else None, n, C.addressof(P),
                            mask.ctypes.data, None, None, C.addressof(R), 0, 0, None)
    return rc, L.gsr_last_error()


def test_struct_layouts(hip_lib):
    from gaussiansplattingregistration_amd import _lib
    assert C.sizeof(_lib.CleanParams) == 48 and _lib.CleanParams.std_ratio.offset == 24 and _lib.CleanParams.nb_points.offset == 40
    assert C.sizeof(_lib.CleanReport) == 12 * 8 + 16 and _lib.CleanReport.phase_ms.offset == 96
    assert "gsr_outlier_mask" in _lib.SIGNATURES and "gsr_model_select" in _lib.SIGNATURES
    assert hasattr(hip_lib, "gsr_outlier_mask") and hasattr(hip_lib, "gsr_model_select")


@pytest.mark.parametrize("kw, word", [(dict(nb_neighbors=33), b"nb_neighbors"), (dict(nb_neighbors=-1), b"nb_neighbors"),
                                      (dict(std_ratio=0.0), b"std_ratio"), (dict(std_ratio=-2.0), b"std_ratio"), (dict(std_ratio=math.nan), b"std_ratio"),
                                      (dict(min_raw_opacity=-2.0), b"raw_opacity"), (dict(max_log_scale=1.0), b"scaling")])
def test_outlier_mask_argument_errors(hip_lib, kw, word):
    """checked before the device is looked for: the same answer with and without a GPU"""
    from gaussiansplattingregistration_amd import _lib
    rc, msg = _mask_call(hip_lib, _lib, **kw)
    assert rc == _lib.GSR_E_INVALID, (rc, msg)
    assert b"gsr_outlier_mask" in msg and word in msg, msg


def _views(_lib, n, K, sr, cap=None):
    rng = np.random.default_rng(1)
    width = {"xyz": 3, "cov6": 6, "dc": 3, "sh": 3 * K, "opacity": 1, "scaling": 3, "rot": 4}
    vin, vout, keep = _lib.ModelView(), _lib.ModelView(), []
    cap = n if cap is None else cap
    vin.n, vout.n = n, cap
    for name, w in width.items():
        if w == 0 or (name in ("scaling", "rot") and not sr):
            continue
        a, o = rng.random((n, w)).astype(np.float32), np.zeros((max(cap, 1), w), np.float32)
        keep += [a, o]
        setattr(vin, name, a.ctypes.data)
        setattr(vout, name, o.ctypes.data)
    return vin, vout, keep


def test_select_argument_errors(hip_lib):
    from gaussiansplattingregistration_amd import _lib
    L, n = hip_lib, 16
    mask = np.ones(n, np.uint8)
    n_out = C.c_int64(0)
    call = lambda vin, K, vout, m=mask, idx=None: L.gsr_model_select(C.addressof(vin), K, m.ctypes.data, C.addressof(vout), idx, C.byref(n_out), 0, 0, None)
    for K in (1, 2, 16, -1):
        vin, vout, keep = _views(_lib, n, 3, True)
        assert call(vin, K, vout) == _lib.GSR_E_INVALID and b"K must be" in L.gsr_last_error()
    vin, vout, keep = _views(_lib, n, 3, True)
    vout.xyz = vin.xyz                                                           # in place
    assert call(vin, 3, vout) == _lib.GSR_E_INVALID and b"overlaps" in L.gsr_last_error()
    vin, vout, keep = _views(_lib, n, 3, True)
    vout.cov6 = vin.xyz + 4 * 3 * (n - 1)                                        # the output's first bytes on the input's last row
    assert call(vin, 3, vout) == _lib.GSR_E_INVALID and b"overlaps" in L.gsr_last_error()
    vin, vout, keep = _views(_lib, n, 0, False)
    vout.dc = vout.xyz                                                           # two outputs on one buffer
    assert call(vin, 0, vout) == _lib.GSR_E_INVALID and b"overlaps" in L.gsr_last_error()
    vin, vout, keep = _views(_lib, n, 0, False)
    assert call(vin, 0, vout, idx=vout.xyz) == _lib.GSR_E_INVALID and b"overlaps" in L.gsr_last_error()
    vin, vout, keep = _views(_lib, n, 0, True)
    vin.rot = None                                                               # scaling without rot
    assert call(vin, 0, vout) == _lib.GSR_E_INVALID and b"scaling and rot" in L.gsr_last_error()
    vin, vout, keep = _views(_lib, n, 0, False)
    vin.n = 1 << 31
    assert call(vin, 0, vout) == _lib.GSR_E_INVALID
    for m in (L.gsr_last_error(),):
        assert b"gsr_model_select" in m


@pytest.mark.parametrize("name", ["gsr_outlier_mask", "gsr_model_select"])
def test_no_device_names_the_function(hip_lib, name):
    """valid host arrays and no visible device: GSR_E_NO_DEVICE through open_device, with the function's name"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    from gaussiansplattingregistration_amd import _lib
    if name == "gsr_outlier_mask":
        rc, msg = _mask_call(hip_lib, _lib)
    else:
        vin, vout, keep = _views(_lib, 8, 3, True)
        mask, n_out = np.ones(8, np.uint8), C.c_int64(0)
        rc = hip_lib.gsr_model_select(C.addressof(vin), 3, mask.ctypes.data, C.addressof(vout), None, C.byref(n_out), 0, 0, None)
        msg = hip_lib.gsr_last_error()
    assert rc == _lib.GSR_E_NO_DEVICE
    assert b"no HIP device" in msg and name.encode() in msg, msg


def test_python_front_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    from gaussiansplattingregistration_amd import clean
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.params.clean_parameters import CleanParams
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clean.outlier_mask(M.small_cloud(5), CleanParams())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PointCloud(M.small_cloud(5)).remove_statistical_outlier(20, 2.0)
