"""Non-rigid refinement without a GPU: the float64 model (tests/warp_model.py) against its own definitions,
the host solver ``gsr_warp_solve`` against the model's dense solve, and the stand-alone sanitiser self-test.  The device side is
tests/test_warp_gpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import warp_model as M
from conftest import ROOT
from gaussiansplattingregistration_amd import warp as W

EPS = 2.0 ** -52


def _random_sums(dims, n, rng, cells=None, planar=False):
    """sums of n random correspondences (points uniform in the unit box over the lattice [0, 1]^3; `cells`: only those inside that
    cell index survive; planar: every normal is e_z and every point lies on one plane)"""
    lo, hi = np.zeros(3), np.ones(3)
    p = rng.random((n, 3))
    if planar:
        p[:, 2] = 0.37
    c, f, _, _ = M.locate(lo, hi, dims, p)
    cell = M.cell_index(dims, c)
    if cells is not None:
        keep = np.isin(cell, cells)
        p, c, f, cell = p[keep], c[keep], f[keep], cell[keep]
    nr = rng.normal(size=(len(p), 3))
    if planar:
        nr = np.tile([0.0, 0.0, 1.0], (len(p), 1))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    r0 = 0.05 * rng.normal(size=len(p))
    g = (M.weights(f)[:, :, None] * nr[:, None, :]).reshape(-1, 24)
    return M.cell_sums(dims, cell, np.concatenate([g, r0[:, None]], 1))[0]


# ------------------------------------------------------------------------------------------------ 1. partition of unity
@pytest.mark.parametrize("dims", [(2, 2, 2), (2, 3, 5), (5, 5, 5)])
def test_affine_nodes_give_an_affine_field(dims):
    rng = np.random.default_rng(1)
    lo, hi = np.array([-1.0, 0.5, 2.0]), np.array([1.5, 1.0, 4.0])
    A, t = 0.1 * rng.normal(size=(3, 3)), rng.normal(size=3)
    U = M.node_positions(lo, hi, dims) @ A.T + t
    p = lo + (hi - lo) * (0.001 + 0.998 * rng.random((500, 3)))
    d = M.displacement(lo, hi, dims, U, p)
    assert np.abs(d - (p @ A.T + t)).max() < 1e-13 * (1 + np.abs(U).max())
    F = M.deformation(lo, hi, dims, U, p)
    assert np.abs(F - (np.eye(3) + A)).max() < 1e-12
    assert np.abs(M.weights(M.locate(lo, hi, dims, p)[1]).sum(1) - 1).max() < 1e-15
    # the library's host evaluation (what the prolongation uses) is the same field
    fld = W.WarpField(W.WarpLattice(lo, hi, dims), U)
    assert np.array_equal(fld.displacement(p), d)


def test_gradient_of_the_weights():
    """the analytic grad w against central differences inside cells; zero on clamped axes and on the outer faces"""
    rng = np.random.default_rng(2)
    dims, lo, hi = (3, 4, 2), np.zeros(3), np.array([1.0, 2.0, 0.5])
    U = rng.normal(size=(24, 3))
    h = M.spacing(lo, hi, dims)
    cc = np.stack([rng.integers(0, dims[a] - 1, 200) for a in range(3)], 1)
    p = lo + (cc + 0.05 + 0.9 * rng.random((200, 3))) * h          # at least 5 % of a cell away from every lattice plane
    F = M.deformation(lo, hi, dims, U, p)
    e = 1e-6
    for a in range(3):
        dp = np.zeros(3)
        dp[a] = e
        num = (M.displacement(lo, hi, dims, U, p + dp) - M.displacement(lo, hi, dims, U, p - dp)) / (2 * e)
        assert np.abs(F[:, :, a] - (np.eye(3)[:, a] + num)).max() < 1e-8
    out = np.array([[-0.3, 1.0, 0.2], [0.5, 2.5, 0.2], [0.5, 1.0, 0.9], [0.0, 1.0, 0.2], [0.5, 1.0, 0.5]])       # x<lo, y>hi, z>hi, x on lo, z on hi
    for row, axis in zip(out, (0, 1, 2, 0, 2)):
        c, f, act, hh = M.locate(lo, hi, dims, row[None])
        assert not act[0, axis]
        assert np.all(M.grad_weights(f, act, hh)[0, :, axis] == 0.0)
        assert np.all(M.deformation(lo, hi, dims, U, row[None])[0, :, axis] == np.eye(3)[:, axis])


# ------------------------------------------------------------------------------------------------ 2. prolongation
def test_prolongation_is_exact():
    rng = np.random.default_rng(3)
    lo, hi = np.array([-2.0, -1.0, 0.0]), np.array([1.0, 3.0, 0.7])
    p = lo + (hi - lo) * rng.random((2000, 3))
    U2 = rng.normal(size=(8, 3))
    f2 = W.WarpField(W.WarpLattice(lo, hi, (2, 2, 2)), U2)
    f3 = f2.prolong((3, 3, 3))
    f5 = f3.prolong((5, 5, 5))
    assert np.array_equal(f3.U, M.prolong(lo, hi, (2, 2, 2), U2, (3, 3, 3)))
    d2 = M.displacement(lo, hi, (2, 2, 2), U2, p)
    for fld in (f3, f5):
        d = M.displacement(lo, hi, tuple(fld.lattice.dims), fld.U, p)
        assert np.abs(d - d2).max() <= 1e-14 * np.abs(d2).max()
    # and a 3^3 field with its own content survives 3^3 -> 5^3
    U3 = rng.normal(size=(27, 3))
    g5 = W.WarpField(W.WarpLattice(lo, hi, (3, 3, 3)), U3).prolong((5, 5, 5))
    d3 = M.displacement(lo, hi, (3, 3, 3), U3, p)
    assert np.abs(M.displacement(lo, hi, (5, 5, 5), g5.U, p) - d3).max() <= 1e-14 * np.abs(d3).max()


def test_default_box_and_field_file(tmp_path):
    pts = np.array([[0.0, 0.0, 0.0], [2.0, 1.0, 0.0], [np.nan, 5.0, 5.0]], np.float32)       # flat in z; the NaN row does not count
    for lo, hi in (W.default_box(pts), M.default_box(pts)):
        assert np.allclose(hi - lo, [2.0 + 4e-6, 1.0 + 4e-6, 2e-3 + 4e-6], rtol=0, atol=1e-12)
        assert np.allclose(lo + hi, [2.0, 1.0, 0.0], atol=1e-12)
    assert all(np.array_equal(a, b) for a, b in zip(W.default_box(pts), M.default_box(pts)))
    fld = W.WarpField(W.WarpLattice(*W.default_box(pts), (2, 3, 5)), np.random.default_rng(0).normal(size=(30, 3)))
    fld.save(tmp_path / "f.npz")
    back = W.WarpField.load(tmp_path / "f.npz")
    assert np.array_equal(back.U, fld.U) and np.array_equal(back.lattice.lo, fld.lattice.lo) and np.array_equal(back.lattice.dims, fld.lattice.dims)
    with pytest.raises(ValueError):
        W.WarpLattice([0, 0, 0], [1, 1, 1], (1, 2, 2))
    with pytest.raises(ValueError):
        W.WarpLattice([0, 0, 0], [1, 1, 1], (2, 18, 2))


# ------------------------------------------------------------------------------------------------ 3. gradient of E
def test_normal_equations_are_half_the_gradient_of_E():
    rng = np.random.default_rng(4)
    dims = (2, 3, 5)
    sums = _random_sums(dims, 600, rng)
    H, b = M.assemble(dims, sums, 0.01, 1e-6)
    U = 0.1 * rng.normal(size=(30, 3))
    g = H @ U.reshape(-1) + b
    e = 1e-5
    num = np.empty(90)
    for i in range(90):
        d = np.zeros(90)
        d[i] = e
        num[i] = (M.energy(dims, sums, 0.01, 1e-6, U + d.reshape(30, 3)) - M.energy(dims, sums, 0.01, 1e-6, U - d.reshape(30, 3))) / (2 * e)
    assert np.abs(g - 0.5 * num).max() < 1e-8 * (1 + np.abs(g).max())


# ------------------------------------------------------------------------------------------------ 4. the host solver
def _cases():
    rng = np.random.default_rng(5)
    return {
        "2x2x2": ((2, 2, 2), _random_sums((2, 2, 2), 300, rng)),
        "2x3x5": ((2, 3, 5), _random_sums((2, 3, 5), 800, rng)),
        "5x5x5_one_cell": ((5, 5, 5), _random_sums((5, 5, 5), 20000, rng, cells=[21])),
        "planar": ((3, 3, 3), _random_sums((3, 3, 3), 500, rng, planar=True)),
    }


@pytest.mark.parametrize("name", ["2x2x2", "2x3x5", "5x5x5_one_cell", "planar"])
def test_solver_against_the_dense_solve(hip_lib, name):
    """|U_library - U_model| <= cond(H) 2^-52 |U_model| (max norms), cond(H) computed by the model"""
    dims, sums = _cases()[name]
    assert sums[:, 325].sum() > 50
    Um, cond = M.solve_dense(dims, sums, 0.01, 1e-6)
    U0 = 0.01 * np.random.default_rng(6).normal(size=Um.shape)
    U, rep = W.solve(dims, sums, 0.01, 1e-6, U0)
    err, margin = np.abs(U - Um).max(), cond * EPS * np.abs(Um).max()
    print(f"{name}: cond {cond:.3e}, |U| {np.abs(Um).max():.3e}, error {err:.3e}, margin {margin:.3e}, E {rep['E_before']:.6g} -> {rep['E_after']:.6g}")
    assert err <= margin
    assert rep["n_corr"] == int(sums[:, 325].sum()) and rep["n_unknowns"] == Um.size
    assert abs(rep["E_before"] - M.energy(dims, sums, 0.01, 1e-6, U0)) <= 1e-12 * abs(rep["E_before"])
    assert abs(rep["E_after"] - M.energy(dims, sums, 0.01, 1e-6, Um)) <= 1e-9 * abs(rep["E_after"])
    assert rep["E_after"] <= rep["E_before"]


def test_solver_without_a_correspondence_gives_zero(hip_lib):
    for dims in ((2, 2, 2), (3, 3, 3)):
        ncells = int(np.prod(np.array(dims) - 1))
        U, rep = W.solve(dims, np.zeros((ncells, 326)), 0.01, 1e-6, np.full((int(np.prod(dims)), 3), 0.5))
        assert not U.any() and rep["n_corr"] == 0 and rep["E_after"] == 0.0


def test_solver_refusals(hip_lib):
    dims, sums = _cases()["2x3x5"]
    def refused(match, d, s, lam=0.01, lam0=1e-6, U=None):
        with pytest.raises(RuntimeError, match=match):
            W.solve(d, s, lam, lam0, U)

    refused("outside", (1, 3, 5), sums)
    refused("outside", (2, 18, 5), sums)
    refused("negative regularisation", dims, sums, lam=-1.0)
    refused("negative regularisation", dims, sums, lam0=-1e-9)
    refused("non-finite", dims, sums, lam=float("nan"))
    refused("non-finite", dims, sums, lam0=float("inf"))
    s = sums.copy(); s[3, 17] = np.nan
    refused("non-finite sum", dims, s)
    s = sums.copy(); s[0, 310] = np.inf
    refused("non-finite sum", dims, s)
    U = np.zeros((30, 3)); U[4, 1] = np.nan
    refused("non-finite displacement", dims, sums, U=U)
    s = sums.copy(); s[2, 0] = -1.0
    refused("negative diagonal", dims, s)
    s = sums.copy(); s[2, 1] = 10.0 * (s[2, 0] + s[2, 24] + 1.0)          # an off-diagonal entry far beyond Cauchy-Schwarz
    refused("positive semi-definite", dims, s)
    s = sums.copy(); s[2, 300:324] *= 1e3                                # b no longer inside the span of A and S_rr
    refused("positive semi-definite", dims, s)
    s = sums.copy(); s[1, 325] = 2.5
    refused("not a non-negative integer", dims, s)
    d5, s5 = _cases()["5x5x5_one_cell"]
    refused("not positive definite", d5, s5, lam=0.0, lam0=0.0)


# ------------------------------------------------------------------------------------------------ 5. the sanitiser self-test
def test_selftest_is_clean_under_the_host_sanitizers(tmp_path):
    """scripts/warp_selftest.cpp: csrc/gsr_warp.h alone, its refusals and one small solve, built with AddressSanitizer and UBSan"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "warp_selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "scripts", "warp_selftest.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ 9 (model). the drift scene
@pytest.fixture(scope="module")
def scene():
    return M.drift_scene()


def test_model_loop_removes_the_drift(scene):
    """The loop on a case a matrix cannot solve, in the model: the RMS of p + d(p) minus the undrifted position falls below ONE THIRD
    of its value before the warp (a float64 prototype reached 0.22: 0.0315 -> 0.0070).  tests/test_warp_gpu.py holds the library to
    the same third."""
    r = M.refine(scene["src"], scene["tgt"], scene["nrm"], 0.1)
    src = scene["src"].astype(np.float64)
    before = M.rms(src - scene["clean"])
    after = M.rms(src + M.displacement(r["lo"], r["hi"], r["dims"], r["U"], src) - scene["clean"])
    print(f"drift RMS {before:.5f} -> {after:.5f} (ratio {after / before:.3f}); point-to-plane RMSE {r['rmse_before']:.5f} -> {r['rmse_after']:.5f}; "
          f"{len(r['log'])} solves, {r['n_corr']} correspondences")
    assert after < before / 3.0


def test_model_loop_null_case(scene):
    """the undrifted sample against the same target: the RMS displacement stays below the jitter, 0.002 (the prototype: 0.0005)"""
    r = M.refine(scene["null"], scene["tgt"], scene["nrm"], 0.1)
    p = scene["null"].astype(np.float64)
    moved = M.rms(M.displacement(r["lo"], r["hi"], r["dims"], r["U"], p))
    print(f"null case: RMS displacement {moved:.5f}; point-to-plane RMSE {r['rmse_before']:.5f} -> {r['rmse_after']:.5f}")
    assert moved < 0.002
