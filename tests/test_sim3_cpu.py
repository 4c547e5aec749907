"""Similarity (scaled) registration, the parts that need no GPU: the host solve gsr_icp_solve with
GSR_ICP_POINT_TO_POINT_SCALED (kind 4), utils/similarity_util.py, and the error paths of the new ABI surface.

The solve is compared with the float64 NumPy Umeyama of tests/sim3_model.py.  Its bound is not a chosen number: kind 0 goes through
the same comparison on the same inputs (against NumPy's rigid Umeyama) and the bound is 4 x its worst deviation -- the margin
covers Jacobi versus LAPACK on a matrix scaled by c.  Measured on the cases below: kind 0 worst 5.0e-15, so the bound is 2.0e-14;
kind 4 worst 7.7e-15.
"""
import ctypes as C

import numpy as np
import pytest

import sim3_model as M

SIZES = (3, 50, 1000)
SCALES = (0.5, 1.0, 2.5)
CENTRES = ((0.0, 0.0, 0.0), (0.7, -1.3, 2.1))
INVALID = -1


def _pairs(n, c, seed):
    """p (moved source) and q (target): q = c R p + t, with 1 % noise once there are more pairs than unknowns"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3)) + np.array([0.4, -0.2, 0.1])
    T = M.similarity(c, 23.0, (0.3, -1.0, 0.5), (0.2, -0.1, 0.3))
    q = p @ T[:3, :3].T + T[:3, 3]
    if n > 3:
        q = q + 0.01 * rng.normal(size=(n, 3))
    return p, q


def _solve(lib, acc, kind, centre):
    upd = np.zeros(16)
    ctr = np.asarray(centre, np.float64)
    assert lib.gsr_icp_solve(acc.ctypes.data, kind, ctr.ctypes.data, upd.ctypes.data) == 0, lib.gsr_last_error()
    return upd.reshape(4, 4)


def _cases():
    return [(n, c, ctr) for n in SIZES for c in SCALES for ctr in CENTRES]


def _deviation(lib, kind):
    """worst max|library - model| over the cases, per case printed"""
    worst = 0.0
    for i, (n, c, ctr) in enumerate(_cases()):
        p, q = _pairs(n, c, 100 + i)
        acc = M.accumulators(p, q, np.asarray(ctr), scaled=kind == 4)
        d = float(np.abs(_solve(lib, acc, kind, ctr) - M.umeyama(p, q, with_scaling=kind == 4)).max())
        print(f"kind {kind} n {n} c {c} centre {ctr}: deviation {d:.3e}")
        worst = max(worst, d)
    return worst


@pytest.fixture(scope="module")
def bound(hip_lib):
    b0 = _deviation(hip_lib, 0)
    print(f"kind 0 worst deviation {b0:.3e} -> bound {4 * b0:.3e}")
    assert 0.0 < b0 < 1e-12                 # float64 round-off of a 3x3 problem: anything else and the yardstick itself is broken
    return 4.0 * b0


def test_scaled_solve_matches_the_model(hip_lib, bound):
    """gsr_icp_solve(kind 4) on accumulators built in NumPy from 3, 50 and 1000 pairs, c in {0.5, 1, 2.5}, centre zero and
    non-zero, against Eigen's Umeyama with scaling restated in NumPy.  Bound: 4 x kind 0's worst deviation from the rigid
    Umeyama on the same inputs (measured 5.0e-15 -> 2.0e-14; kind 4 measured 7.7e-15).  Refused (unknown kind) before kind 4."""
    d4 = _deviation(hip_lib, 4)
    print(f"kind 4 worst deviation {d4:.3e}, bound {bound:.3e}")
    assert d4 <= bound
    for i, (n, c, ctr) in enumerate(_cases()):          # and the scale itself comes back (noise-free at n = 3)
        if n == 3:
            p, q = _pairs(n, c, 100 + i)
            T = _solve(hip_lib, M.accumulators(p, q, np.asarray(ctr), True), 4, ctr)
            assert abs(M.scale_of(T) - c) <= 1e-12 * c


def test_unit_scale_agrees_with_the_rigid_kind(hip_lib, bound):
    """c = 1 inputs without noise: rotation and translation of kinds 0 and 4 agree to the bound, and |c - 1| stays within it."""
    for n in SIZES:
        rng = np.random.default_rng(7 + n)
        p = rng.normal(size=(n, 3))
        T = M.similarity(1.0, 31.0, (1.0, 0.2, -0.4), (0.1, 0.2, -0.3))
        q = p @ T[:3, :3].T + T[:3, 3]
        for ctr in CENTRES:
            T0 = _solve(hip_lib, M.accumulators(p, q, np.asarray(ctr), False), 0, ctr)
            T4 = _solve(hip_lib, M.accumulators(p, q, np.asarray(ctr), True), 4, ctr)
            c = M.scale_of(T4)
            print(f"n {n} centre {ctr}: |T4 - T0| {np.abs(T4 - T0).max():.3e}  |c - 1| {abs(c - 1):.3e}")
            assert np.abs(T4 - T0).max() <= bound and abs(c - 1.0) <= bound


def test_degenerate_inputs_give_the_identity(hip_lib):
    """Where Eigen divides by zero the update is the identity: one correspondence; all sources equal."""
    one = M.accumulators(np.array([[0.3, 0.2, 0.1]]), np.array([[1.0, 2.0, 3.0]]), np.zeros(3), True)
    assert np.array_equal(_solve(hip_lib, one, 4, (0, 0, 0)), np.eye(4))
    p = np.tile(np.array([[0.5, -0.25, 2.0]]), (20, 1))            # exactly representable: the variance is exactly zero
    q = np.random.default_rng(0).normal(size=(20, 3))
    same = M.accumulators(p, q, np.zeros(3), True)
    assert np.array_equal(_solve(hip_lib, same, 4, (0, 0, 0)), np.eye(4))
    assert np.array_equal(M.umeyama(p, q, True), np.eye(4))
    none = np.zeros(32)
    assert np.array_equal(_solve(hip_lib, none, 4, (0, 0, 0)), np.eye(4))


def test_split_similarity():
    from gaussiansplattingregistration_amd.utils.similarity_util import split_similarity
    for c in (1e-3, 0.5, 1.0, 2.5, 400.0):
        T = M.similarity(c, 77.0, (0.2, 0.5, -1.0), (1.0, -2.0, 3.0))
        cc, R, t = split_similarity(T)
        assert abs(cc - c) <= 1e-12 * c and np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and np.array_equal(t, T[:3, 3])
        assert np.allclose(cc * R, T[:3, :3], rtol=0, atol=1e-12 * c)
    refl = M.similarity(1.3, 10.0, (0, 0, 1), (0, 0, 0))
    refl[:3, 0] *= -1
    shear = M.similarity(1.3, 10.0, (0, 0, 1), (0, 0, 0))
    shear[:3, :3] = shear[:3, :3] @ np.array([[1, 1e-2, 0], [0, 1, 0], [0, 0, 1.0]])
    zero = np.eye(4)
    zero[:3, :3] = 0.0
    for bad in (refl, shear, zero):
        with pytest.raises(ValueError):
            split_similarity(bad)


def test_initial_similarity_gives_the_exact_scale():
    from gaussiansplattingregistration_amd.utils.similarity_util import initial_similarity, split_similarity
    rng = np.random.default_rng(3)
    src = rng.normal(size=(500, 3)) * np.array([1.0, 2.0, 0.5])
    for c in (0.25, 1.0, 3.0):
        shift = np.array([4.0, -1.0, 2.5])
        tgt = c * src + shift
        T = initial_similarity(src, tgt)
        cc, R, t = split_similarity(T)
        assert abs(cc - c) <= 1e-12 * c and np.abs(R - np.eye(3)).max() <= 4e-16      # c I / cbrt(c^3): one rounding
        assert np.abs(src @ T[:3, :3].T + T[:3, 3] - tgt).max() <= 1e-12 * (1 + c)       # a pure scale + shift is recovered whole


# ------------------------------------------------------------------------------------------------ error paths, raw ABI
def _msg(lib):
    return lib.gsr_last_error().decode()


def test_scaled_kind_with_a_loss_is_refused(hip_lib):
    """Robust losses do not apply to the scaled kind: GSR_E_INVALID and a message, checked on the arguments alone."""
    T, acc = np.eye(4), np.zeros(32)
    out, f, r, it = np.zeros(16), C.c_double(), C.c_double(), C.c_int32()
    for loss in (1, 2, 3, 4):
        assert hip_lib.gsr_icp_accumulate(None, T.ctypes.data, 4, loss, 0.1, acc.ctypes.data) == INVALID
        assert "no robust loss" in _msg(hip_lib) and "gsr_icp_accumulate" in _msg(hip_lib)
        assert hip_lib.gsr_icp_register(None, T.ctypes.data, 4, loss, 0.1, 1e-6, 1e-6, 5, out.ctypes.data, C.byref(f), C.byref(r), C.byref(it)) == INVALID
        assert "no robust loss" in _msg(hip_lib)
        assert hip_lib.gsr_icp_register_clouds(None, None, 0, None, None, 0, 0, 0.1, T.ctypes.data, 4, loss, 0.1, 1e-6, 1e-6, 5, out.ctypes.data,
                                               C.byref(f), C.byref(r), C.byref(it)) == INVALID
        assert "no robust loss" in _msg(hip_lib)
    # without a loss the arguments pass and the NULL context is what is refused
    assert hip_lib.gsr_icp_accumulate(None, T.ctypes.data, 4, 0, 0.0, acc.ctypes.data) == INVALID
    assert "NULL" in _msg(hip_lib)


@pytest.mark.parametrize("kind", [5, 6, 7])
def test_scaling_with_another_estimator_is_refused(hip_lib, kind):
    """The with_scaling bit on point-to-plane (5), generalized (6) or colored (7): GSR_E_INVALID with a message."""
    acc, upd, T = np.zeros(32), np.zeros(16), np.eye(4)
    acc[0] = 10
    assert hip_lib.gsr_icp_solve(acc.ctypes.data, kind, None, upd.ctypes.data) == INVALID
    assert "point-to-point estimation only" in _msg(hip_lib)
    assert hip_lib.gsr_icp_accumulate(None, T.ctypes.data, kind, 0, 0.0, acc.ctypes.data) == INVALID
    assert "point-to-point estimation only" in _msg(hip_lib)
    from gaussiansplattingregistration_amd import _lib
    P, R = _lib.RansacParams(), _lib.RansacResult()
    P.kind, P.ransac_n, P.max_corr, P.max_iteration, P.confidence, P.batch = kind, 3, 0.5, 10, 0.999, 8
    assert hip_lib.gsr_ransac_correspondence(None, 0, None, 0, None, None, None, 0, C.byref(P), C.byref(R), 0, 0, None) == INVALID
    assert "not supported" in _msg(hip_lib)
    assert hip_lib.gsr_icp_solve(acc.ctypes.data, 8, None, upd.ctypes.data) == INVALID and "unknown kind" in _msg(hip_lib)


def test_model_similarity_bad_arguments(hip_lib):
    n = 4
    T = M.similarity(1.5, 20.0, (0, 1, 0), (0.1, 0.2, 0.3))
    xyz, cov, rot, scl = (np.zeros((n, k), np.float32) for k in (3, 6, 4, 3))
    ox, oc, oq, ol = (np.zeros((n, k), np.float32) for k in (3, 6, 4, 3))
    p = lambda a: a.ctypes.data
    call = hip_lib.gsr_model_similarity
    assert call(None, n, 0, 0, p(xyz), p(cov), p(rot), None, p(scl), p(ox), p(oc), p(oq), None, p(ol), 0, 0, None) == INVALID
    assert "gsr_model_similarity" in _msg(hip_lib)
    assert call(p(T), n, 0, 0, None, p(cov), p(rot), None, p(scl), p(ox), p(oc), p(oq), None, p(ol), 0, 0, None) == INVALID
    assert "NULL array" in _msg(hip_lib)
    assert call(p(T), n, 0, 0, p(xyz), p(cov), p(rot), None, p(scl), p(ox), p(oc), p(oq), None, None, 0, 0, None) == INVALID      # scaling without scaling_out
    assert "NULL array" in _msg(hip_lib)
    assert call(p(T), n, 3, 0, p(xyz), p(cov), p(rot), None, p(scl), p(ox), p(oc), p(oq), None, p(ol), 0, 0, None) == INVALID      # K = 3 without sh
    assert call(p(T), n, 4, 0, p(xyz), p(cov), p(rot), None, p(scl), p(ox), p(oc), p(oq), None, p(ol), 0, 0, None) == INVALID      # K not 0 / 3 / 8 / 15
    assert call(p(T), -1, 0, 0, p(xyz), p(cov), p(rot), None, p(scl), p(ox), p(oc), p(oq), None, p(ol), 0, 0, None) == INVALID
    # the gate, in front of any device work: a reflection, a shear, a scale outside [1e-6, 1e6]; in place
    refl = T.copy()
    refl[:3, 0] *= -1
    shear = T.copy()
    shear[:3, :3] = shear[:3, :3] @ np.array([[1, 1e-2, 0], [0, 1, 0], [0, 0, 1.0]])
    tiny = M.similarity(1e-7, 20.0, (0, 1, 0), (0, 0, 0))
    for bad in (refl, shear, tiny):
        assert call(p(bad), n, 0, 0, p(xyz), p(cov), p(rot), None, p(scl), p(ox), p(oc), p(oq), None, p(ol), 0, 0, None) == INVALID
        assert "not c R" in _msg(hip_lib)
    assert call(p(T), n, 0, 0, p(xyz), p(cov), p(rot), None, p(scl), p(ox), p(oc), p(oq), None, p(scl), 0, 0, None) == INVALID
    assert "overlaps" in _msg(hip_lib)
    # and the rigid entry keeps refusing a scaled matrix
    assert hip_lib.gsr_model_transform(p(T), n, 0, 0, p(xyz), p(cov), p(rot), None, p(ox), p(oc), p(oq), None, 0, 0, None) == INVALID
    assert "not a rotation" in _msg(hip_lib)


def test_python_surface_refuses_scaling_off_point_to_point():
    from gaussiansplattingregistration_amd import icp
    from gaussiansplattingregistration_amd.utils import global_registration_util as G
    from gaussiansplattingregistration_amd.utils import local_registration_util as L
    assert L.get_estimation(L.LocalRegistrationType.ICP_Point_To_Point, None, with_scaling=True).kind == icp.KIND_POINT_TO_POINT_SCALED == 4
    assert L.get_estimation(L.LocalRegistrationType.ICP_Point_To_Point, None).kind == 0
    for rt in (L.LocalRegistrationType.ICP_Point_To_Plane, L.LocalRegistrationType.ICP_Color, L.LocalRegistrationType.ICP_General):
        with pytest.raises(RuntimeError, match="with_scaling"):
            L.get_estimation(rt, None, with_scaling=True)
        with pytest.raises(RuntimeError, match="with_scaling"):
            L.do_icp_registration(None, None, np.eye(4), rt, 0.1, 1e-6, 1e-6, 5, L.KernelLossFunctionType.Loss_None, 0.0, with_scaling=True)
    assert G.TransformationEstimationPointToPoint().kind == 0 and G.TransformationEstimationPointToPoint(with_scaling=True).kind == 4
