"""The covariance build and its derivative without a GPU: the analytic NumPy model (tests/cov_grad_model.py) against central
differences of its float64 forward, the two invariances of the map (it ignores the quaternion's norm), the recorded float32 cost that
tests/test_cov_grad_gpu.py multiplies by four, the two new C-ABI entries without a device and the fine-tuner's argument checks.

Finite differences.  Rows are independent, so every row is a test of its own: ``L_r = sum_j g6[r, j] cov6[r, j]`` in float64, all rows
moved at once along ``d`` (log-scales by ``h d``, quaternion entries by ``h |q_r| d``), ``FD(h) = (L_r(+h) - L_r(-h)) / 2h`` with h = 2^-17
and h / 2.  The analytic value must lie within ``4 |FD(h) - FD(h/2)| + 8 eps A_r / h`` of ``FD(h/2)``: Richardson's estimate of the truncation
error plus the round-off floor of evaluating ``L_r``, whose terms sum to ``A_r = sum_j |g6[r, j]| scale(cov6)[r, j]`` in absolute value
(eps = 2^-52) -- the two-step-size criterion of tests/test_raster_grad_cpu.py.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cov_grad_model as M
from conftest import GOLDEN

TOLERANCE = os.path.join(GOLDEN, "cov_grad_tolerance.json")
H_STEP = 2.0 ** -17
EPS = 2.0 ** -52


def _row_losses(m, s, q):
    return (m["grad_cov6"].astype(np.float64) * M.chain(s, q)["cov6"]).sum(1)


def _fd_rows(m, ds, dq):
    """-> (FD(h), FD(h/2)) per row along (ds, dq)"""
    s, q = m["scaling"].astype(np.float64), m["rotation"].astype(np.float64)
    out = []
    for h in (H_STEP, H_STEP / 2):
        out.append((_row_losses(m, s + h * ds, q + h * dq) - _row_losses(m, s - h * ds, q - h * dq)) / (2 * h))
    return out


def _assert_rows(what, m, ds, dq):
    ana = (m["ref"]["scaling"] * ds).sum(1) + (m["ref"]["rotation"] * dq).sum(1)
    fd_h, fd_h2 = _fd_rows(m, ds, dq)
    floor = (np.abs(m["grad_cov6"].astype(np.float64)) * m["scale"]["cov6"]).sum(1)
    allowed = 4 * np.abs(fd_h - fd_h2) + 8 * EPS * floor / H_STEP
    err = np.abs(ana - fd_h2)
    bad = np.nonzero(~(err <= allowed))[0]
    assert bad.size == 0, (what, bad[:5], err[bad[:5]], allowed[bad[:5]])
    return float((err / (np.abs(ana) + M.TINY)).max())


@pytest.mark.parametrize("name", M.SCENES)
def test_analytic_backward_matches_central_differences_along_random_directions(name):
    """16 directions over both inputs at once, every row judged on its own"""
    m = M.scene_models(name)
    n = len(m["scaling"])
    rng = np.random.default_rng(5)
    qn = np.linalg.norm(m["rotation"].astype(np.float64), axis=1, keepdims=True)
    worst = 0.0
    for trial in range(16):
        ds = rng.integers(-4, 5, (n, 3)) / 4.0
        dq = qn * rng.integers(-4, 5, (n, 4)) / 4.0
        worst = max(worst, _assert_rows((name, trial), m, ds, dq))
    print(f"{name}: largest |analytic - FD(h/2)| / |analytic| over the rows {worst:.3e}")


@pytest.mark.parametrize("name", M.SCENES)
def test_analytic_backward_matches_central_differences_on_every_coordinate(name):
    m = M.scene_models(name)
    n = len(m["scaling"])
    qn = np.linalg.norm(m["rotation"].astype(np.float64), axis=1)
    for col in range(7):
        ds, dq = np.zeros((n, 3)), np.zeros((n, 4))
        if col < 3:
            ds[:, col] = 1.0
        else:
            dq[:, col - 3] = qn
        _assert_rows((name, col), m, ds, dq)


@pytest.mark.parametrize("name", M.SCENES)
def test_gradient_of_the_quaternion_is_orthogonal_to_it(name):
    """the map does not depend on |q|: q . dL/dq = 0 to the rounding of the four products, read against sum |q_c| scale_c"""
    m = M.scene_models(name)
    q = m["rotation"].astype(np.float64)
    dot = (q * m["ref"]["rotation"]).sum(1)
    mag = (np.abs(q) * m["scale"]["rotation"]).sum(1)
    assert (np.abs(dot) <= 64 * EPS * mag).all(), float((np.abs(dot) / (mag + M.TINY)).max())
    assert (mag > 0).sum() >= len(mag) - 16          # (the identity has mag = 0: every term of the dot product is an exact zero)


@pytest.mark.parametrize("name", M.SCENES)
def test_scaling_a_quaternion_leaves_cov_and_grad_scaling_and_divides_grad_rotation(name):
    m = M.scene_models(name)
    for c in (0.5, 3.0, 128.0):                          # (powers of two scale exactly; 3.0 does not)
        got = M.chain(m["scaling"], m["rotation"].astype(np.float64) * c, m["grad_cov6"])
        for k in ("cov6", "scaling"):
            assert (np.abs(got[k] - m["ref"][k]) <= 64 * EPS * m["scale"][k]).all(), (name, c, k)
        assert (np.abs(got["rotation"] * c - m["ref"]["rotation"]) <= 64 * EPS * m["scale"]["rotation"]).all(), (name, c)


def test_scenes_hold_what_they_were_built_for():
    s, q, g = M.make("generic")
    assert s.min() >= -6 and s.max() <= 1 and len(s) <= 300
    nq = np.linalg.norm(q.astype(np.float64), axis=1)
    assert nq.min() < 0.2 and nq.max() > 5 and nq.min() >= 0.0999 and nq.max() <= 10.001
    assert not g[-8:].any() and g[:-8].any(1).all()
    s, q, g = M.make("needles_discs")
    ratio = np.exp(s.max(1).astype(np.float64) - s.min(1))
    assert ratio.max() > 9000 and ratio.max() < 1.3e4 and ratio.min() > 8
    s, q, g = M.make("special_rotations")
    unit = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    assert any(np.allclose(u, (1, 0, 0, 0)) for u in unit)
    for k in (1, 2, 3):
        assert any(np.allclose(u, np.eye(4)[k]) for u in unit)               # the half-turns: w = 0
    for k in range(4):
        assert ((q[:, k] == 0) & ((q != 0).sum(1) == 3)).sum() >= 12           # exactly one zero component
    s, q, g = M.make("norms")
    nq = np.linalg.norm(q.astype(np.float64), axis=1)
    assert np.allclose(nq[0::2], 1e-3, rtol=1e-6) and np.allclose(nq[1::2], 1e3, rtol=1e-6)
    # the gradient of the quaternion scales with 1 / |q|: six orders of magnitude between the two halves
    m = M.scene_models("norms")
    gr = np.abs(m["ref"]["rotation"]).max(1)
    assert np.median(gr[0::2]) > 1e5 * np.median(gr[1::2])
    for name in M.SCENES:
        assert len(M.make(name)[0]) <= 300
        assert all(np.isfinite(M.scene_models(name)["ref"][k]).all() for k in M.OUTPUTS)


def test_zero_gradient_rows_are_exact_zeros_whatever_the_scale():
    s = np.float32([[100.0, 100.0, 100.0], [0.0, 0.0, 0.0]])
    q = np.float32([[1.0, 2.0, 3.0, 4.0], [1.0, 0.0, 0.0, 0.0]])
    g = np.zeros((2, 6), np.float32)
    for dtype in (np.float64, np.float32):
        got = M.chain(s, q, g, dtype)
        assert not got["scaling"].any() and not got["rotation"].any() and not np.signbit(got["scaling"]).any() and not np.signbit(got["rotation"]).any()


def test_recorded_float32_cost():
    """writes tests/golden/cov_grad_tolerance.json when it is missing, checks it otherwise: per scene and output, max |float32 model -
    float64 model| / scale.  Every figure is some float32 roundings (2^-24 each, relative to the scale) of a chain of at most 64
    operations: below 64 x 2^-24 = 3.8e-6."""
    got = {name: M.float32_cost(name) for name in M.SCENES}
    for name in M.SCENES:
        print(f"{name}: float32 model against float64 model {got[name]}")
    if not os.path.exists(TOLERANCE):
        with open(TOLERANCE, "w") as out:
            json.dump(got, out, indent=1, sort_keys=True)
            out.write("\n")
    want = json.load(open(TOLERANCE))
    assert sorted(want) == sorted(M.SCENES)
    for name in M.SCENES:
        for k in M.OUTPUTS:
            assert got[name][k] == pytest.approx(want[name][k], rel=1e-6, abs=1e-12), (name, k)
            assert 0 < got[name][k] < 64 * 2.0 ** -24, (name, k)


def test_cov_entry_points_without_a_device(hip_lib):
    """argument checks need no device; valid host arrays and no visible device give GSR_E_NO_DEVICE and a message that names the function"""
    import torch
    n = 8
    s, q, g = (np.zeros((n, 3), np.float32), np.tile(np.float32([1, 0, 0, 0]), (n, 1)), np.ones((n, 6), np.float32))
    cov, gs, gq = np.zeros((n, 6), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32)
    p = lambda a: a.ctypes.data
    assert hip_lib.gsr_cov_build(p(s), p(q), -1, p(cov), 0, 0, None) == -1                       # GSR_E_INVALID
    assert b"gsr_cov_build" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_cov_build(p(s), None, n, p(cov), 0, 0, None) == -1
    assert b"gsr_cov_build: rotation" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_cov_build(p(s), p(q), n, None, 0, 0, None) == -1
    assert b"gsr_cov_build: cov6" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_cov_build_backward(p(s), p(q), p(g), -1, p(gs), p(gq), 0, 0, None) == -1
    assert b"gsr_cov_build_backward" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_cov_build_backward(p(s), p(q), None, n, p(gs), p(gq), 0, 0, None) == -1
    assert b"gsr_cov_build_backward: grad_cov6" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_cov_build_backward(p(s), p(q), p(g), n, None, None, 0, 0, None) == -1
    assert b"both NULL" in hip_lib.gsr_last_error()
    if torch.cuda.is_available():                  # the rest is about a machine without one
        return
    assert hip_lib.gsr_cov_build(p(s), p(q), n, p(cov), 0, 0, None) == -3                        # GSR_E_NO_DEVICE
    msg = hip_lib.gsr_last_error()
    assert b"no HIP device" in msg and b"gsr_cov_build" in msg, msg
    assert hip_lib.gsr_cov_build_backward(p(s), p(q), p(g), n, p(gs), p(gq), 0, 0, None) == -3
    msg = hip_lib.gsr_last_error()
    assert b"no HIP device" in msg and b"gsr_cov_build_backward" in msg, msg
    assert not cov.any() and not gs.any() and not gq.any()
    from gaussiansplattingregistration_amd import covariance
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        covariance.build_covariance(s, q)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        covariance.build_covariance_backward(s, q, g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        covariance.covariance_from_scale_rotation(torch.zeros(1, 3), torch.ones(1, 4))


def test_finetuner_accepts_scaling_and_rotation():
    from gaussiansplattingregistration_amd import covariance
    from gaussiansplattingregistration_amd.finetune import TUNABLE, FinetuneParams, FinetuneResult, ModelFinetuner
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    p = FinetuneParams()
    assert TUNABLE == ("dc", "sh_rest", "opacity", "xyz", "scaling", "rotation")
    assert (p.params, p.lr_scaling, p.lr_rotation, p.geometry_rtol) == (("dc", "sh_rest", "opacity"), 5e-3, 1e-3, 1e-3)
    assert FinetuneResult().geometry_source is None
    # the new fields are keyword-only: positional construction is what it was
    old = FinetuneParams(5, ("dc",), 1.0, 2.0, 3.0, 4.0, "l1", (1.0, 1.0, 1.0), 0.3)
    assert (old.iterations, old.lr_xyz, old.loss, old.background, old.lambda_dssim, old.lr_scaling) == (5, 4.0, "l1", (1.0, 1.0, 1.0), 0.3, 5e-3)
    with pytest.raises(TypeError):
        FinetuneParams(5, ("dc",), 1.0, 2.0, 3.0, 4.0, "l1", (1.0, 1.0, 1.0), 0.3, 5e-3)
    model = GaussianModel("cpu").from_arrays(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32), np.zeros(2, np.float32),
                                             np.tile(np.float32([1, 0, 0, 1, 0, 1]), (2, 1)), np.zeros((2, 0), np.float32), 0)
    with pytest.raises(ValueError, match="unknown tensor 'cov6'"):
        ModelFinetuner(model, [], [], FinetuneParams(params=("scaling", "cov6")))
    with pytest.raises(ValueError, match="unknown tensor 'scale'"):
        ModelFinetuner(model, [], [], FinetuneParams(params=("scale",)))
    # the two names pass the argument check: what stops a model on the host is the device, as for every other tensor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ModelFinetuner(model, [], [], FinetuneParams(params=("scaling", "rotation")))
    with pytest.raises(ValueError, match="unknown output"):
        covariance.build_covariance_backward(np.zeros((1, 3)), np.ones((1, 4)), np.zeros((1, 6)), wants=("cov6",))
    with pytest.raises(ValueError, match="no output"):
        covariance.build_covariance_backward(np.zeros((1, 3)), np.ones((1, 4)), np.zeros((1, 6)), wants=())
