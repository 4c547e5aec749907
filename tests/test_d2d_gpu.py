"""Mixture-to-mixture registration on the device: ``gsr_d2d_accumulate`` against ``d2d_model`` on all 32 sums, the
rows and pairs that must not count, its bits from run to run and from host or device arrays, ``gsr_d2d_register`` against the model's
loop, and the front ends.

The tolerance of a float sum is derived (the derivation of tests/test_photo_gpu.py, restated): kernel and model form every pair's
``m`` and ``M`` in float64 from the same float32 inputs with the same operations in the same order, without fused multiply-add, so
a term differs only by the last place of the two ``exp`` implementations (one ulp each: glibc documents exp within 1 ulp, the AMD
device library's double-precision exp is within 1 ulp), and the sums differ by the ORDER of the summation.  Two orders of N terms are
within N 2^-52 sum|term| of each other; the two ``exp`` add 2 2^-52 sum|term|: (n_pairs + 2) 2^-52 sum|term_k|, with sum|term_k| what
the model returns beside each sum (for H and g: the magnitudes carried through the per-row expansion, see ``d2d_model.accumulate``).
The counts in slots 29..31 are exact."""
import functools

import numpy as np
import pytest

import d2d_model as M

pytestmark = pytest.mark.gpu

T_CASE = M.rigid(23.0, (0.3, -1.0, 0.5), (0.2, -0.1, 0.15))       # a rotation about a skew axis plus a shift
R_ALL = 4.0                                                       # more than the diameter of the clouds: every pair counts
SCALE, FLOOR = 1.25, 1e-5


def _cov(rng, n, size):
    L = rng.normal(size=(n, 3, 3)) * size
    Cm = L @ np.transpose(L, (0, 2, 1)) + (0.05 * size) ** 2 * np.eye(3)
    return np.stack([Cm[:, 0, 0], Cm[:, 0, 1], Cm[:, 0, 2], Cm[:, 1, 1], Cm[:, 1, 2], Cm[:, 2, 2]], -1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _clouds(ns, nt):
    """uniform points in the unit cube on the target's side; the source is such points moved by T_CASE^-1.  Weights in [0.5, 1.5]."""
    rng = np.random.default_rng(1000 * ns + nt)
    spacing = (1.0 / max(nt, 2)) ** (1.0 / 3.0)
    tx = rng.random((nt, 3)).astype(np.float32)
    Ti = np.linalg.inv(T_CASE)
    sx = (rng.random((ns, 3)) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    src = (sx, _cov(rng, ns, 0.5 * spacing), rng.uniform(0.5, 1.5, ns).astype(np.float32))
    tgt = (tx, _cov(rng, nt, 0.5 * spacing), rng.uniform(0.5, 1.5, nt).astype(np.float32))
    for a in src + tgt:
        a.setflags(write=False)
    return src, tgt, spacing


@functools.lru_cache(maxsize=None)
def _model(ns, nt, radius_kind, weighted):
    """the model's sums of a case, computed once and left unchanged"""
    src, tgt, spacing = _clouds(ns, nt)
    radius = R_ALL if radius_kind == "all" else 1.2 * spacing
    if not weighted:
        src, tgt = (src[0], src[1], None), (tgt[0], tgt[1], None)
    sums, asum = M.accumulate(src, tgt, T_CASE, radius, SCALE, FLOOR)
    sums.setflags(write=False)
    asum.setflags(write=False)
    return src, tgt, radius, sums, asum


def _dev(c):
    import torch
    return tuple(None if a is None else torch.as_tensor(np.array(a), device="cuda:0") for a in c)


def _kernel(src, tgt, T, radius, scale=1.0, floor=0.0, on_device=False):
    from gaussiansplattingregistration_amd import d2d
    if on_device:
        src, tgt = _dev(src), _dev(tgt)
    with d2d.D2DContext(0) as ctx:
        ctx.set_target(*tgt, radius)
        ctx.set_source(*src)
        return ctx.accumulate(T, scale, floor)


def _check(got, sums, asum, name):
    n_pairs = sums[29]
    tol = (n_pairs + 2) * 2.0 ** -52 * asum
    err = np.abs(got - sums)
    print(f"{name}: pairs {sums[29]:.0f} rows {sums[30]:.0f} singular {sums[31]:.0f}; largest |kernel - model| / ((n + 2) 2^-52 sum|term|) = "
          f"{np.max(err[:29] / np.maximum(tol[:29], 1e-300)):.3g}; largest relative error {np.max(err[:29] / np.maximum(np.abs(sums[:29]), 1e-300)):.3g}")
    assert np.array_equal(got[29:], sums[29:]), (name, got[29:], sums[29:])
    worst = int(np.argmax(err[:29] - tol[:29]))
    assert np.all(err[:29] <= tol[:29]), (name, worst, got[worst], sums[worst], tol[worst])


@pytest.mark.parametrize("nt", [1, 64, 300])
@pytest.mark.parametrize("ns", [0, 1, 63, 64, 65, 257])
def test_sums_against_the_model(ns, nt):
    """both radii (every pair; 1.2 mean spacings of the target), with and without weights, host arrays and device arrays"""
    bits = {}
    for radius_kind in ("all", "spacing"):
        for weighted in (True, False):
            src, tgt, radius, sums, asum = _model(ns, nt, radius_kind, weighted)
            if radius_kind == "all":
                assert sums[29] == ns * nt and sums[30] == ns
            for on_device in (False, True):
                got = _kernel(src, tgt, T_CASE, radius, SCALE, FLOOR, on_device)
                _check(got, sums, asum, f"{ns} x {nt} {radius_kind} weights={weighted} device={on_device}")
                if ns == 0:
                    assert not got.any() and not np.signbit(got).any()
                key = (radius_kind, weighted)
                assert np.array_equal(bits.setdefault(key, got), got)           # host arrays or device arrays: the same bits


def test_a_radius_near_the_spacing_pairs_some_and_not_all():
    """the second radius does what it is there for: rows with several pairs, rows with none"""
    _, _, _, sums, _ = _model(257, 300, "spacing", True)
    assert 257 < sums[29] < 257 * 300 / 4 and 0 < sums[30] <= 257


def test_reproducible():
    src, tgt, radius, sums, asum = _model(257, 300, "spacing", True)
    a = _kernel(src, tgt, T_CASE, radius, SCALE, FLOOR)
    b = _kernel(src, tgt, T_CASE, radius, SCALE, FLOOR)
    assert a.tobytes() == b.tobytes()
    from gaussiansplattingregistration_amd import d2d
    with d2d.D2DContext(0) as ctx:                   # and within one context, with another evaluation in between
        ctx.set_target(*tgt, radius)
        ctx.set_source(*src)
        c = ctx.accumulate(T_CASE, SCALE, FLOOR)
        ctx.accumulate(np.eye(4), 1.0, 0.0)
        d = ctx.accumulate(T_CASE, SCALE, FLOOR)
    assert a.tobytes() == c.tobytes() == d.tobytes()


# ------------------------------------------------------------------------------------------------ rows and pairs that must not count
def _edge_base():
    src, tgt, spacing = _clouds(65, 64)
    return tuple(np.array(a) for a in src), tuple(np.array(a) for a in tgt), 2.0 * spacing


@pytest.mark.parametrize("what", ["source_xyz", "target_xyz", "source_cov", "target_cov", "source_weight", "target_weight", "source_inf", "target_cov_inf"])
def test_a_non_finite_row_takes_part_in_nothing(what):
    """the sums with the poisoned row are the sums without it: against the model with the row poisoned, and against the kernel on the
    clouds with the row REMOVED (counts and score)"""
    src, tgt, radius = _edge_base()
    side, row = (src, 7) if what.startswith("source") else (tgt, 11)
    bad = np.inf if what.endswith("inf") else np.nan
    if "xyz" in what or what == "source_inf":
        side[0][row, 1] = bad
    elif "cov" in what:
        side[1][row, 4] = bad
    else:
        side[2][row] = bad
    sums, asum = M.accumulate(src, tgt, T_CASE, radius, SCALE, FLOOR)
    got = _kernel(src, tgt, T_CASE, radius, SCALE, FLOOR)
    assert np.isfinite(got).all()
    _check(got, sums, asum, what)
    cut = lambda c: tuple(np.delete(a, row, axis=0) for a in c)
    src2, tgt2 = (cut(src), tgt) if side is src else (src, cut(tgt))
    ref = _kernel(src2, tgt2, T_CASE, radius, SCALE, FLOOR)
    assert np.array_equal(got[29:], ref[29:]) and abs(got[27] - ref[27]) <= (ref[29] + 2) * 2.0 ** -52 * ref[27]
    clean_src, clean_tgt, _ = _edge_base()
    assert M.accumulate(clean_src, clean_tgt, T_CASE, radius, SCALE, FLOOR)[0][29] > sums[29]      # (the row had pairs to lose)


def test_zero_covariances_are_singular_without_a_floor_and_count_with_one():
    z6 = np.zeros((1, 6), np.float32)
    src = (np.float32([[0.25, 0.5, -0.125]]), z6, None)
    tgt = (np.float32([[0.5, 0.5, -0.125], [0.25, 0.75, 0.0]]), np.concatenate([z6, np.float32([[1e-2, 0, 0, 1e-2, 0, 1e-2]])]), None)
    got = _kernel(src, tgt, np.eye(4), 1.0)
    sums, asum = M.accumulate(src, tgt, np.eye(4), 1.0)
    assert tuple(got[29:]) == (1.0, 1.0, 1.0) == tuple(sums[29:])        # the regular pair counts, the singular one is counted apart
    _check(got, sums, asum, "singular, no floor")
    floor = 0.0625
    got = _kernel(src, tgt, np.eye(4), 1.0, 1.0, floor)
    sums, asum = M.accumulate(src, tgt, np.eye(4), 1.0, 1.0, floor)
    assert tuple(got[29:]) == (2.0, 1.0, 0.0)
    _check(got, sums, asum, "singular, floor")
    only = _kernel(src, (tgt[0][:1], tgt[1][:1], None), np.eye(4), 1.0, 1.0, floor)
    assert only[29] == 1.0 and abs(only[27] - np.exp(-0.5)) <= 2 * 2.0 ** -52       # M = I / floor exactly (powers of two), m = |r|^2 / floor = 1
    alone = _kernel(src, (tgt[0][:1], tgt[1][:1], None), np.eye(4), 1.0)
    assert tuple(alone[29:]) == (0.0, 0.0, 1.0) and not alone[:29].any()


def test_a_source_row_beyond_the_targets_box():
    src, tgt, radius = _edge_base()
    Ti = np.linalg.inv(T_CASE)
    src[0][3] = (np.array([1.0 + 1.5 * radius, 0.5, 0.5]) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)      # beyond the box by more than the radius
    src[0][4] = (np.array([0.5, -40.0, 0.5]) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)                  # and far beyond it
    sums, asum = M.accumulate(src, tgt, T_CASE, radius, SCALE, FLOOR)
    t = M.pair_terms(src, tgt, T_CASE, radius, SCALE, FLOOR)
    assert 3 not in t["i"] and 4 not in t["i"]
    _check(_kernel(src, tgt, T_CASE, radius, SCALE, FLOOR), sums, asum, "outside the box")
    far = np.eye(4)
    far[:3, 3] = 50.0
    assert not _kernel(src, tgt, far @ T_CASE, radius, SCALE, FLOOR).any()                                    # every row: thirty-two zeros


def test_every_point_in_one_cell():
    """a target whose points all coincide (a box without extent: one cell), and one inside a cube far smaller than the radius"""
    src, tgt, _ = _edge_base()
    for spread in (0.0, 1e-4):
        rng = np.random.default_rng(5)
        tx = (np.float32([0.5, 0.5, 0.5]) + spread * rng.random((64, 3))).astype(np.float32)
        t2 = (tx, tgt[1], tgt[2])
        for radius in (0.3, 3.0):
            sums, asum = M.accumulate(src, t2, T_CASE, radius, SCALE, FLOOR)
            assert sums[29] > 0 and sums[29] % 64 == 0
            _check(_kernel(src, t2, T_CASE, radius, SCALE, FLOOR), sums, asum, f"one cell, spread {spread}, radius {radius}")


def test_a_pair_at_exactly_max_corr_does_not_count():
    c6 = np.float32([[1e-2, 0, 0, 1e-2, 0, 1e-2]])
    src = (np.float32([[0.0, 0.0, 0.0]]), c6, None)
    tgt = (np.float32([[0.5, 0.0, 0.0], [0.0, -0.5, 0.0], [0.0, 0.0, np.nextafter(np.float32(0.5), np.float32(0))], [0.25, 0.25, 0.25]]), np.repeat(c6, 4, 0), None)
    got = _kernel(src, tgt, np.eye(4), 0.5)
    sums, asum = M.accumulate(src, tgt, np.eye(4), 0.5)
    assert sums[29] == 2                                             # the one just inside and the one well inside; d^2 == max_corr^2 is out
    _check(got, sums, asum, "exactly max_corr")
    shift = np.eye(4)
    shift[:3, 3] = (0.25, 0.0, 0.0)                                  # dyadic: p' and every d^2 stay exact
    got = _kernel(src, tgt, shift, 0.25)
    sums, asum = M.accumulate(src, tgt, shift, 0.25)
    assert sums[29] == 0 and not got.any()                           # |(0.25, 0, 0) - (0.5, 0, 0)| = 0.25 exactly: out; the others are farther


# ------------------------------------------------------------------------------------------------ the registration
@functools.lru_cache(maxsize=None)
def _scene300():
    sc = M.scene(300, 0)
    r = M.register(sc["src"], sc["tgt"], np.eye(4), 0.2)
    return sc, r


def test_registration_against_the_model():
    """the prototype's scene at 300 components a side: the final T within 1e-9 (Frobenius) of the model's, the same iteration count"""
    from gaussiansplattingregistration_amd import d2d
    sc, want = _scene300()
    assert want["status"] == "converged" and 3 < want["iterations"] < 30
    with d2d.D2DContext(0) as ctx:
        ctx.set_target(*sc["tgt"], 0.2)
        ctx.set_source(*sc["src"])
        got = ctx.register(np.eye(4), 1.0, 0.0, 1e-6, 30)
    e0, e1 = M.pose_error(np.eye(4), sc["truth"]), M.pose_error(got["transformation"], sc["truth"])
    print(f"iterations {got['iterations']} / {want['iterations']}; |T - T_model| = {np.linalg.norm(got['transformation'] - want['T']):.3g}; "
          f"pose error {e0[0]:.3f} deg / {e0[1]:.4f} -> {e1[0]:.4f} deg / {e1[1]:.2g}; score {got['score']:.6f}")
    assert got["iterations"] == want["iterations"] and got["status"] == want["status"]
    assert np.linalg.norm(got["transformation"] - want["T"]) < 1e-9
    assert abs(got["score"] - want["score"]) <= 1e-9 * want["score"]
    assert abs(got["fitness"] - want["fitness"]) == 0 and abs(got["mahalanobis_rmse"] - want["mahalanobis_rmse"]) <= 1e-9
    assert got["n_pairs"] == want["sums"][29] and got["n_singular"] == 0


def test_registration_stops():
    from gaussiansplattingregistration_amd import d2d
    sc, _ = _scene300()
    far = np.eye(4)
    far[:3, 3] = 30.0
    with d2d.D2DContext(0) as ctx:
        ctx.set_target(*sc["tgt"], 0.2)
        ctx.set_source(*sc["src"])
        r = ctx.register(far)
        assert r["status"] == "no_pairs" and r["iterations"] == 0 and np.array_equal(r["transformation"], far) and r["score"] == 0.0
        r = ctx.register(np.eye(4), max_iteration=2)
        want = M.register(sc["src"], sc["tgt"], np.eye(4), 0.2, max_iter=2)
        assert r["status"] == "max_iteration" and r["iterations"] == 2 and np.linalg.norm(r["transformation"] - want["T"]) < 1e-9
        assert abs(r["score"] - want["score"]) <= 1e-9 * want["score"]          # the report is taken at the final T
        r = ctx.register(np.eye(4), max_iteration=0)
        assert r["iterations"] == 0 and np.array_equal(r["transformation"], np.eye(4)) and r["score"] > 0


# ------------------------------------------------------------------------------------------------ the front ends
def test_do_mixture_registration_through_the_point_cloud_record():
    import torch
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.params import MixtureRegistrationParams
    from gaussiansplattingregistration_amd.utils.local_registration_util import do_mixture_registration
    sc, want = _scene300()
    P = MixtureRegistrationParams(max_correspondence=0.2)
    for dev in (False, True):
        f = (lambda a: torch.as_tensor(np.array(a), device="cuda:0")) if dev else np.array
        res = do_mixture_registration(PointCloud(xyz32=f(sc["src"][0]), cov6=f(sc["src"][1])), PointCloud(xyz32=f(sc["tgt"][0]), cov6=f(sc["tgt"][1])), np.eye(4), P)
        assert np.linalg.norm(res.transformation - want["T"]) < 1e-9 and res.iterations == want["iterations"]
        assert res.score > 0 and res.status == "converged" and res.fitness == want["fitness"] and res.inlier_rmse == res.mahalanobis_rmse
    # weights reach the kernel: the model with the same weights
    rng = np.random.default_rng(1)
    w, v = rng.uniform(0.2, 2.0, 300).astype(np.float32), rng.uniform(0.2, 2.0, 300).astype(np.float32)
    res = do_mixture_registration(PointCloud(xyz32=sc["src"][0], cov6=sc["src"][1]), PointCloud(xyz32=sc["tgt"][0], cov6=sc["tgt"][1]), np.eye(4), P,
                                  source_weights=w, target_weights=v)
    ww = M.register((sc["src"][0], sc["src"][1], w), (sc["tgt"][0], sc["tgt"][1], v), np.eye(4), 0.2)
    assert np.linalg.norm(res.transformation - ww["T"]) < 1e-9 and res.iterations == ww["iterations"]
    assert np.linalg.norm(ww["T"] - want["T"]) > 1e-7
    with pytest.raises(RuntimeError, match="covariances"):
        do_mixture_registration(PointCloud(xyz32=sc["src"][0]), PointCloud(xyz32=sc["tgt"][0], cov6=sc["tgt"][1]), np.eye(4), P)


def test_coarse_to_fine_driver_over_two_two_level_lists():
    """two levels a side (fine: 300 components; coarse: 100 components with nine times the covariance, carrying weights as a HEM level
    does), from 12 degrees off: entry by entry the model's loop, and the controller's entry point on top"""
    from gaussiansplattingregistration_amd.controllers.registration_controller import RegistrationController
    from gaussiansplattingregistration_amd.workers.registrators import MixtureToMixtureRegistrator
    truth = M.rigid(12.0, (1, 1, 1), (0.1, -0.1, 0.05))
    fine, coarse = M.scene(300, 3, truth), M.scene(100, 4, truth)
    rng = np.random.default_rng(2)
    level = lambda c, w: {"xyz": c[0], "cov6": c[1]} if w is None else {"xyz": c[0], "cov6": (9.0 * c[1]).astype(np.float32), "weight": w}
    ws, wt = rng.uniform(1.0, 5.0, 100).astype(np.float32), rng.uniform(1.0, 5.0, 100).astype(np.float32)
    l1, l2 = [level(fine["src"], None), level(coarse["src"], ws)], [level(fine["tgt"], None), level(coarse["tgt"], wt)]
    corr, scale, iters = [0.6, 0.2], [2.0, 1.0], [30, 30]
    m0 = M.register((l1[1]["xyz"], l1[1]["cov6"], ws), (l2[1]["xyz"], l2[1]["cov6"], wt), np.eye(4), corr[0], scale[0], max_iter=iters[0])
    m1 = M.register(fine["src"], fine["tgt"], m0["T"], corr[1], scale[1], max_iter=iters[1])
    worker = MixtureToMixtureRegistrator(l1, l2, np.eye(4), corr, scale, iters)
    out = worker.run()
    assert out is not None and not worker.errors and len(worker.level_results) == 2
    r0, r1 = worker.level_results
    e = M.pose_error(r1.transformation, truth)
    print(f"coarse: {r0.iterations} / {m0['iterations']} iterations, fine: {r1.iterations} / {m1['iterations']}; |T - T_model| = "
          f"{np.linalg.norm(r0.transformation - m0['T']):.3g}, {np.linalg.norm(r1.transformation - m1['T']):.3g}; pose error {e[0]:.4f} deg / {e[1]:.2g}")
    assert r0.iterations == m0["iterations"] and np.linalg.norm(r0.transformation - m0["T"]) < 1e-9
    assert r1.iterations == m1["iterations"] and np.linalg.norm(r1.transformation - m1["T"]) < 1e-9
    assert out.result is r1 and out.registration_data.result_transformation is r1.transformation
    assert e[1] < 0.25 * M.pose_error(np.eye(4), truth)[1]
    bad = MixtureToMixtureRegistrator(l1, l2[:1], np.eye(4), corr, scale, iters)
    assert bad.run() is None and bad.errors

    class Repo:
        pc_open3d_list_first, pc_open3d_list_second, current_index = [], [], 0

    class Ui:
        transformation_matrix = np.eye(4)

    rc = RegistrationController(Repo(), Ui())
    res = rc.execute_mixture_registration(corr, scale, iters, levels=(l1, l2))
    assert res is not None and np.array_equal(rc.ui_repository.transformation_matrix, r1.transformation)


def test_register_ply_mixture_refine(tmp_path):
    """scripts/register_ply.py --mixture-refine as a child process on the scene's two samplings written as .ply files (scales and
    quaternions from the eigen-decomposition of the disc covariances): the printed transform is the model's on the same files, started
    from the ICP result the script prints.  Both matrices are printed to six decimals (5e-7 each) and the loop stops within its own
    1e-6, so entries may differ by 2e-6; the covariances the script rebuilds from scales and quaternions are the model's to float32."""
    import os
    import re
    import subprocess
    import sys
    from scipy.spatial.transform import Rotation
    from conftest import ROOT
    from gaussiansplattingregistration_amd import synth
    from gaussiansplattingregistration_amd.utils import ply_io
    sc, _ = _scene300()
    paths, clouds = [], []
    for name, c in (("a.ply", sc["src"]), ("b.ply", sc["tgt"])):
        lam, V = np.linalg.eigh(M._full(c[1].astype(np.float64)))
        V[:, :, 0] *= np.sign(np.linalg.det(V))[:, None]                    # proper rotations
        q = Rotation.from_matrix(V).as_quat()[:, [3, 0, 1, 2]].astype(np.float32)
        s = (0.5 * np.log(lam)).astype(np.float32)
        R = synth._quat_to_rot(q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True))
        L = R * np.exp(s.astype(np.float64))[:, None, :]
        C = L @ L.transpose(0, 2, 1)
        cov6 = C[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]].astype(np.float32)
        assert np.abs(cov6 - c[1]).max() < 1e-6 * np.abs(c[1]).max() * 10
        n = len(c[0])
        paths.append(str(tmp_path / name))
        ply_io.save_gaussian_ply(paths[-1], c[0], np.full((n, 3), 0.5, np.float32), np.zeros((n, 9), np.float32), np.zeros((n, 1), np.float32), s, q)
        clouds.append((c[0], cov6, None))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "register_ply.py"), paths[0], paths[1], "--voxel", "--type", "point", "--max-corr", "0.3",
                        "--iters", "30", "--mixture-refine", "0.2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    num = r"[-+]?\d+\.?\d*(?:e[-+]?\d+)?"

    def matrix(after):
        text = r.stdout[r.stdout.index(after) + len(after):]
        return np.array([float(x) for x in re.findall(num, text)[:16]]).reshape(4, 4)

    T_icp = matrix("transformation (first -> second):")
    T_mix = matrix("transformation after the mixture-to-mixture refinement (first -> second):")
    want = M.register(clouds[0], clouds[1], T_icp, 0.2)
    e_icp, e_mix = M.pose_error(T_icp, sc["truth"]), M.pose_error(T_mix, sc["truth"])
    print(f"ICP {e_icp[0]:.4f} deg / {e_icp[1]:.3g} -> mixture-to-mixture {e_mix[0]:.4f} deg / {e_mix[1]:.3g}; largest |T - T_model| entry "
          f"{np.abs(T_mix - want['T']).max():.3g}")
    assert re.search(r"mixture-to-mixture refinement: score .* iterations \(converged\)", r.stdout), r.stdout
    assert np.abs(T_mix - want["T"]).max() <= 2e-6
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "register_ply.py"), paths[0], paths[1], "--with-scaling", "--mixture-refine", "0.2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "refused with --with-scaling" in r.stderr
