"""The float64 model of the ICP accumulators (tests/icp_acc_model.py) is checked before it judges the kernels (test_icp_acc_gpu.py):
its weights against its losses, its Jacobians against its residuals, its update against the library's host solve, the scenes against
the caps under which the comparison on the GPU is decided by arithmetic and not by a tie, and the tolerance file against a
recomputation.  Nothing here needs a GPU.
"""
import math

import numpy as np
import pytest

import icp_acc_model as A

EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("loss", A.LOSSES)
def test_weight_is_the_derivative_of_the_loss(loss):
    """w(r) r against the central difference of rho at r / s in {+-0.1 .. +-10} on both sides of the switch (s = k, for GM
    sqrt(k), for L2 1), and w(0) against the second difference of rho at 0.  Step h = 1e-4 s; no grid point lies within 10 h of
    the switch, so rho is smooth across every stencil.  The scale of rho' is s w(0) (w(0) = 1, for GM 1 / k): truncation
    h^2 rho''' / 6 ~ 1e-8 of it, rounding 2^-52 rho / h ~ 1e-12 of it.  Allowed 1e-7 s w(0) (1e-6 relative for the second
    difference)."""
    k = A.K[loss] if loss != A.L2 else 0.0
    s = {A.L2: 1.0, A.GM: math.sqrt(A.K[A.GM])}.get(loss, k)
    h = 1e-4 * s
    scale = s * float(A.weight(loss, k, 0.0))
    worst = 0.0
    for u in (0.1, 0.5, 0.9, 0.999, 1.001, 1.1, 2.0, 10.0):
        for sign in (1.0, -1.0):
            r = sign * u * s
            fd = (A.rho(loss, k, r + h) - A.rho(loss, k, r - h)) / (2 * h)
            err = abs(float(A.weight(loss, k, r)) * r - float(fd))
            worst = max(worst, err / scale)
            assert err <= 1e-7 * scale, (A.LOSS_NAME[loss], r, err)
    fd2 = float(A.rho(loss, k, h) - 2 * A.rho(loss, k, 0.0) + A.rho(loss, k, -h)) / (h * h)
    w0 = float(A.weight(loss, k, 0.0))
    print(f"{A.LOSS_NAME[loss]}: worst |w r - d rho| / (s w(0)) = {worst:.2e}; w(0) = {w0!r}, second difference {fd2!r}")
    assert abs(w0 - fd2) <= 1e-6 * abs(w0)
    if loss in A.SWITCHED:                 # the branch decides something on this grid
        assert float(A.weight(loss, k, 2 * k)) < 0.6 and float(A.weight(loss, k, 0.1 * k)) > 0.9


# ----------------------------------------------------------------------------------------------------------------- Jacobians
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_jacobian_is_the_derivative_of_the_residual(kind):
    """Each row of J against the central difference of the row's residual under T <- rigid_from_euler6(x) T at x = 0 (Rz(x2) Ry(x1)
    Rx(x0), translation x3..5), on the first 50 matched pairs of the 257-point scene; the pair and, for the generalized kind, W
    stay fixed, as the linearisation has them.  h = 1e-5: truncation h^2 |g| |p| / 6 ~ 2e-11, rounding 2^-52 / h ~ 2e-11 per unit
    of the residual's operands; allowed 1e-8 max(1, |g|) (1 + |p|)."""
    sc = A.scene(257, 0.03)
    res = A.scene_model(sc, kind, A.L2)
    rows = np.nonzero(res["matched"])[0][:50]
    assert len(rows) == 50
    T = sc["T"]
    src, tgt = sc["src"][rows].astype(np.float64), sc["tgt"].astype(np.float64)
    jm = res["j"][rows]
    q = tgt[jm]
    kw = dict(normals=sc["normals"], src_cov=sc["src_cov"], tgt_cov=sc["tgt_cov"], src_int=sc["src_int"], tgt_int=sc["tgt_int"],
              tgt_grad=sc["grad"], lambda_geometric=A.LAMBDA)
    p = src @ T[:3, :3].T + T[:3, 3]
    g, r0, _ = A.residual_rows(kind, T, p, q, jm, rows, **kw)
    J = A.jacobian(p, g)
    h = 1e-5
    worst = 0.0
    for a in range(6):
        rr = []
        for sign in (1.0, -1.0):
            x = np.zeros(6)
            x[a] = sign * h
            Tx = A.euler6(x) @ T
            rr.append(A.residual_rows(kind, T, src @ Tx[:3, :3].T + Tx[:3, 3], q, jm, rows, **kw)[1])
        fd = (rr[0] - rr[1]) / (2 * h)
        scale = np.maximum(1.0, np.linalg.norm(g, axis=2)) * (1.0 + np.linalg.norm(p, axis=1))[:, None]
        err = np.abs(fd - J[:, :, a]) / scale
        worst = max(worst, float(err.max()))
        assert (err <= 1e-8).all(), (kind, a, float(err.max()))
    assert np.abs(J).max() > 0.1            # (the rows are not trivially zero)
    print(f"kind {kind}: {J.shape[0]} pairs x {J.shape[1]} rows, worst |J - finite difference| / scale = {worst:.2e}")


# --------------------------------------------------------------------------------------------------------------------- solve
def _lib_solve(lib, acc, kind, centre):
    upd = np.zeros(16)
    ctr = np.asarray(centre, np.float64)
    assert lib.gsr_icp_solve(np.ascontiguousarray(acc).ctypes.data, kind, ctr.ctypes.data, upd.ctypes.data) == 0, lib.gsr_last_error()
    return upd.reshape(4, 4)


@pytest.mark.parametrize("kind", A.KINDS)
def test_update_agrees_with_the_host_solve(hip_lib, kind):
    """The model's update (Umeyama by numpy.linalg.svd; numpy.linalg.solve and the Euler matrix) against gsr_icp_solve, both fed
    with the model's slots of every scene and loss.  Only well-conditioned systems are asserted (cond(JTJ) < 1e8; for Umeyama at
    least three pairs and sigma_2 + sigma_3 > 1e-8 sigma_1); the others are documented behaviour and are printed.
    Bound, kinds 1..3: two backward-stable 6 x 6 solves, each with a forward error of at most n^2 2^-53 cond |x|, and a rotation
    entry moves by at most sqrt(3) |dx|: 72 sqrt(3) 2^-53 cond |x| + 8 2^-53.  Kinds 0 / 4: two 3 x 3 SVDs of the same Sigma, each
    backward stable to n^2 2^-53 |Sigma|; the rotation is Sigma's polar factor, which moves by at most 2 |dSigma| / (sigma_2 +
    sigma_3): dR = 72 2^-53 sigma_1 / (sigma_2 + sigma_3), the translation by dR |ma + ctr|_1 plus 16 2^-53 (1 + |mb + ctr|)."""
    ctr = np.array([0.5, 0.49, 0.51])
    asserted, worst = 0, 0.0
    for s in A.SCENES:
        sc = A.scene(*s)
        for loss in (A.LOSSES if kind in (1, 2, 3) else (A.L2,)):
            res = A.scene_model(sc, kind, loss, centre=ctr)
            acc = res["acc"]
            if kind in (1, 2, 3) and not np.linalg.cond(A.normal_equations(acc)[0]) < 1e8:
                print(f"{sc['name']} kind {kind} {A.LOSS_NAME[loss]}: cond(JTJ) not below 1e8, not asserted")
                continue
            want, got = A.update(acc, kind, ctr), _lib_solve(hip_lib, acc, kind, ctr)
            tol = np.zeros((4, 4))
            if kind in (0, 4):
                n = acc[0]
                ma, mb = acc[2:5] / n, acc[5:8] / n
                sv = np.linalg.svd(acc[8:17].reshape(3, 3).T / n - np.outer(mb, ma), compute_uv=False)
                if n < 3 or not sv[1] + sv[2] > 1e-8 * sv[0]:
                    print(f"{sc['name']} kind {kind}: degenerate ({n:.0f} pairs), not asserted")
                    continue
                c = abs(np.cbrt(np.linalg.det(want[:3, :3])))
                dR = 72 * A.EPS53 * sv[0] / (sv[1] + sv[2]) * max(c, 1.0)
                tol[:3, :3] = dR
                tol[:3, 3] = dR * np.abs(ma + ctr).sum() + 16 * A.EPS53 * (1 + np.abs(mb + ctr).max())
            else:
                Am, b = A.normal_equations(acc)
                cond = np.linalg.cond(Am)
                dx = 72 * A.EPS53 * cond * np.linalg.norm(np.linalg.solve(Am, b))
                tol[:3, :3] = math.sqrt(3.0) * dx + 8 * A.EPS53
                tol[:3, 3] = dx + 8 * A.EPS53
            d = np.abs(got - want)
            ratio = float((d[:3] / tol[:3]).max())
            worst = max(worst, ratio)
            asserted += 1
            assert (d <= tol).all(), (sc["name"], kind, loss, ratio)
    print(f"kind {kind}: {asserted} systems asserted, worst |library - model| / bound = {worst:.3f}")
    assert asserted >= (6 if kind in (0, 4) else 30)


# ------------------------------------------------------------------------------------------------- the scenes stay within their caps
@pytest.mark.parametrize("ns,max_corr", A.SCENES)
def test_scene_within_caps(ns, max_corr):
    """What makes a scene decidable: matched fraction in [0.4, 0.7] (ns >= 63), no nearest-neighbour tie and no pair on the
    max_corr sphere to 1e-9 relative, no row on the switch of Huber / Tukey to 1e-9 k, at least 20 % of the rows on each side of k
    (ns >= 63: the single pair of ns = 1 has one point-to-plane row and cannot lie on both sides), every Ct + R Cs R^T conditioned
    below 1e4.  The coloured kind runs with the stand-in gradient here; test_icp_acc_gpu.py asserts the same margins again with the
    gradient the library computed."""
    sc = A.scene(ns, max_corr)
    assert sc["src"].dtype == np.float32 and sc["src"].shape == (ns, 3) and sc["tgt"].shape == (A.NT, 3)
    for kind in A.KINDS:
        for loss in (A.LOSSES if kind in (1, 2, 3) else (A.L2,)):
            res = A.scene_model(sc, kind, loss)
            frac = res["matched"].mean()
            if ns >= 63:
                assert 0.4 <= frac <= 0.7, frac
            assert res["margin_tie"] >= 1e-9 and res["margin_corr"] >= 1e-9
            assert res["cond"] < 1e4
            if kind in (1, 2, 3) and loss in A.SWITCHED:
                assert res["margin_k"] >= 1e-9, (kind, loss, res["margin_k"])
                if ns >= 63:
                    assert 0.2 <= res["below_k"] <= 0.8, (kind, loss, res["below_k"])
            if kind == 2 and loss == A.HUBER:
                print(f"{sc['name']}: matched {100 * frac:.1f} %, tie margin {res['margin_tie']:.1e}, max_corr margin {res['margin_corr']:.1e}, "
                      f"largest cond(Ct + R Cs R^T) {res['cond']:.0f}")
            if kind in (1, 2, 3) and loss == A.HUBER:
                print(f"  kind {kind}: {len(res['r'])} rows, {100 * res['below_k']:.0f} % below k, k margin {res['margin_k']:.1e}")


def test_layout_and_empty():
    """Slots at and past NACC are zero, the count is the number of matched pairs, and a source with nothing in reach gives zeros."""
    sc = A.scene(63, 0.03)
    for kind in A.KINDS:
        res = A.scene_model(sc, kind, A.L2)
        assert res["acc"][0] == res["matched"].sum() and not res["acc"][A.NACC[kind]:].any() and not res["abs"][A.NACC[kind]:].any()
        assert (res["terms"][2:A.NACC[kind]] == res["matched"].sum() * max(1, A.ROWS[kind])).all()
        far = A.model(sc["src"] + np.float32(50.0), sc["tgt"], np.eye(4), 0.03, kind, A.L2, 0.0, normals=sc["normals"], src_cov=sc["src_cov"],
                      tgt_cov=sc["tgt_cov"], src_int=sc["src_int"], tgt_int=sc["tgt_int"], tgt_grad=sc["grad"])
        assert not far["acc"].any() and np.array_equal(A.update(far["acc"], kind), np.eye(4))


# ------------------------------------------------------------------------------------------------------------ the tolerance file
def test_tolerance_file_is_current():
    """tests/golden/icp_acc_tolerance.json against a recomputation (50-digit mpmath on the first 300 matched pairs): equal to 10 %,
    zero for kinds 0 and 4, and of the order of float64 round-off everywhere."""
    stored, now = A.load_tolerances(), A.tolerances()
    assert sorted(stored) == sorted(now) and len(now) == len(A.SCENES) * len(A.KINDS)
    for key in sorted(now):
        print(f"{key}: stored {stored[key]:.3e} recomputed {now[key]:.3e}")
        assert abs(now[key] - stored[key]) <= 0.1 * stored[key], key
        if key.endswith(("kind0", "kind4")):
            assert stored[key] == 0.0
        else:
            assert 0.0 < stored[key] < 1e-12
