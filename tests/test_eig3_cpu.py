"""The references of tests/eig3_model.py decide: every condition tests/test_eig3_gpu.py relies on, checked on the CPU oracle and numpy alone.

E_f, the oracle's worst e / max|lambda| per family (eig3_model.excess), is printed (pytest -s shows it); the GPU test recomputes it and allows
the kernel 16 times as much."""
import numpy as np
import pytest

import eig3_model as M


def oracle_normals(oracle, c6):
    return oracle.normals_from_cov(M.cov33(c6))


@pytest.mark.parametrize("name", M.NORMAL_FAMILIES)
def test_oracle_normals_are_smallest_eigenvectors(oracle, name):
    c6 = M.family(name)
    lam, V = M.eig(c6)
    v = oracle_normals(oracle, c6)
    assert np.isfinite(v).all()
    unit = float(np.abs(M.norm_ld(v) - 1).max())
    E = M.excess(c6, v, lam).max()
    d = M.decided(lam)
    ang = M.angle_to(v[d], V[d, :, 0]).max() if d.any() else 0.0
    print(f"\n{name:10s} rows {len(c6)}  decided {int(d.sum())}  E_f {E:.2e}  | |v| - 1 | {unit:.1e}  angle to LAPACK on decided rows {ang:.1e}")
    # the normalisation is c / sqrt(c . c), or the cross product of two such vectors: a handful of roundings of 2^-53 each
    assert unit <= 2.0 ** -49
    assert E <= 1.7e-15
    # on decided rows the oracle IS the eigenvector: that is what lets the GPU test compare vectors at 1e-9
    assert ang <= 1e-10


def test_families_are_what_they_claim():
    lam = {f: M.eig(M.family(f))[0] for f in set(M.NORMAL_FAMILIES + M.DECOMP_FAMILIES)}
    mx = {f: np.abs(l).max(1) for f, l in lam.items()}
    assert M.decided(lam["flat"]).all() and (lam["flat"][:, 0] < 1e-4 / 0.3 * 1.01 * mx["flat"]).all()
    assert (lam["flat"][:, 0] < 0).mean() > 0.02 and (lam["rank1"][:, 0] < 0).mean() > 0.5      # float32 rounding leaves them indefinite
    assert not M.decided(lam["needle_eq"]).any() and not M.decided(lam["rank1"]).any() and not M.decided(lam["iso_rot"]).any()
    assert (lam["disc_eq"][:, 2] - lam["disc_eq"][:, 1] < 1e-6 * mx["disc_eq"]).all()
    assert (np.abs(lam["rank2"][:, 0]) < 1e-6 * mx["rank2"]).all()
    assert (M.family("diag")[:, [1, 2, 4]] == 0).all() and (M.family("iso_rot")[:, [1, 2, 4]] != 0).any()
    s = M.family("symmetric")
    assert np.array_equal(s[:, 1], s[:, 2]) and np.array_equal(s[:, 3], s[:, 5]) and (lam["symmetric"][:, 0] > 0).all()
    assert mx["tiny30"].max() < 2e-30 and mx["huge30"].max() > 1e29 and np.isfinite(M.family("huge30")).all()
    for f in M.DECOMP_FAMILIES:                           # nothing the documented clamp would have to reproduce
        assert (lam[f][:, 2] > 1e3 * M.CLAMP).all(), f


def test_hand_rows_follow_open3ds_rule(oracle):
    got = oracle_normals(oracle, M.HAND_COV6)
    for (name, _, want), g in zip(M.HAND, got):
        assert tuple(g) == tuple(float(w) for w in want), (name, g)


def test_nonfinite_rows_get_the_fallback_normal(oracle):
    """NaN, +Inf or -Inf anywhere in a covariance: (0, 0, 1).  Before the finiteness test a NaN off the diagonal was dropped by the max that
    scales the matrix and the row left through the diagonal branch as (1, 0, 0): [1, NaN, 0, 2, 0, 3] is among these rows."""
    rows = M.nonfinite_rows()
    assert rows.shape == (18, 6) and (~np.isfinite(rows)).sum() == 18
    assert np.array_equal(rows[1], np.array([1, np.nan, 0, 2, 0, 3], np.float32), equal_nan=True)
    got = oracle_normals(oracle, rows)
    assert np.array_equal(got, np.tile([[0.0, 0.0, 1.0]], (18, 1))), got


def test_every_shepperd_branch_is_populated():
    _, R = M.exact_rotation(M.family("generic"))
    branch, q, margin = M.shepperd(R)
    counts = np.bincount(branch, minlength=4)
    clear = np.bincount(branch[margin > 1e-3], minlength=4)
    print("\nShepperd branches (w x y z) of generic:", counts.tolist(), " with margin > 1e-3:", clear.tolist())
    assert (counts >= 100).all() and (clear >= 100).all()
    # where the margin is positive the branch is the class of the quaternion
    assert np.array_equal(np.abs(q).argmax(1)[margin > 1e-3], branch[margin > 1e-3])
    assert np.abs(M.quat_to_rot(q) - R).max() < 1e-14 and (q[:, 0] >= 0).all()


@pytest.mark.parametrize("name", M.DECOMP_FAMILIES + ("hand",))
def test_exact_model_reproduces_the_covariance(name):
    """eigh, s = float32(ln max(lambda, 1e-30) / 2), the quaternion rounded to float32: within 1e-5 max|A| of A -- the bar is reachable"""
    c6 = M.HAND_COV6[M.HAND_PSD] if name == "hand" else M.family(name)
    s, q = M.exact_model(c6)
    err = M.recon_error(c6, s, q).max()
    print(f"\n{name:10s} float64 model of EXACT mode: worst |R diag(exp 2s) R^T - A| / max|A| = {err:.2e}")
    assert err <= 1e-5
    lam = np.linalg.eigvalsh(M.cov33(c6))
    assert (np.abs(np.sort(np.exp(2 * s.astype(np.float64)), 1) - lam).max(1) <= 1e-5 * np.abs(lam).max(1)).all()


def test_cov_from_normals_model_against_the_oracle(oracle):
    nrm, eps = M.cfn_normals(), 1e-3
    want, mag = M.cfn_model(nrm, eps)
    got = oracle.cov_from_normals(nrm, eps)[:, M.I6[0], M.I6[1]]
    fin = np.isfinite(nrm).all(1)
    assert fin.sum() == len(nrm) - 1 and np.isnan(got[~fin]).all() and np.isnan(np.asarray(want[~fin], np.float64)).all()
    diff = np.abs(got[fin] - want[fin])
    ratio = M.cfn_worst_ratio(diff, mag[fin])
    print(f"\ncov_from_normals: oracle against the long double model, worst |diff| / sum|terms| = {ratio:.2e} (bound {M.CFN_BOUND:.2e})")
    assert (diff <= M.CFN_BOUND * mag[fin]).all()
    # both sides of the branch are there, at -0.99 itself and at its two float64 neighbours
    side = M.cfn_identity_side(nrm)
    x = nrm[:, 0]
    assert side[x == np.nextafter(-0.99, -1.0)].all() and not side[x == -0.99].any() and not side[x == np.nextafter(-0.99, 0.0)].any()
    assert (x == -0.99).sum() >= 8 and (x == np.nextafter(-0.99, -1.0)).sum() >= 8
    ident = np.array([eps, 0, 0, 1, 0, 1])
    assert (np.asarray(want[side], np.float64) == ident).all() and (got[side] == ident).all()
    assert (np.abs(got[fin & ~side & (np.abs(nrm[:, 1:]).max(1) > 0)] - ident).max(1) > 0).all()
    zero = len(nrm) - 3
    assert not nrm[zero].any() and np.array_equal(got[zero], ident)
