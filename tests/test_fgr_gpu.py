"""Fast Global Registration on the MI355X (csrc/fgr.hip) against the NumPy restatement (tests/fgr_model.py)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fgr_model as M
import global_model as G

pytestmark = pytest.mark.gpu

POSES = [(120.0, (1.0, 2.0, 0.7)), (45.0, (-0.3, 0.2, 1.0))]
VOXEL = 0.05


def _pose_ok(T, T_gt, voxel):
    return G.rotation_error_deg(T, T_gt) < 3.0 and np.linalg.norm(T[:3, 3] - T_gt[:3, 3]) < 2 * voxel


@pytest.fixture(scope="module")
def F(hip_lib):
    from gaussiansplattingregistration_amd import features
    return features


@pytest.fixture(scope="module", params=POSES, ids=["120deg", "45deg"])
def scene(request, F):
    """Two independent samplings of the scene, the second moved by T; FPFH and the reciprocal matches from the library (both tested
    against the restatement in test_global_registration_gpu.py)."""
    deg, axis = request.param
    T = G.make_T(deg, axis)
    xs, ns = M.down(60000, 1, VOXEL)
    xt, nt = M.down(60000, 2, VOXEL, T=T)
    fs, ft = F.fpfh(xs, ns, 5 * VOXEL, 100), F.fpfh(xt, nt, 5 * VOXEL, 100)
    corres, used_mutual, nst, nts = F.feature_match(fs, ft, mutual=True, ransac_n=0, return_nn=True)
    i = np.arange(len(xs))
    keep = nts[nst] == i
    assert used_mutual and np.array_equal(corres, np.stack([i[keep], nst[keep]], 1))        # the reciprocal set, no fall-back
    return {"T": T, "xs": xs, "ns": ns, "xt": xt, "nt": nt, "fs": fs, "ft": ft, "corres": np.ascontiguousarray(corres, dtype=np.int32)}


def _place(where, *arrays):
    if where == "host":
        return arrays
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


@pytest.mark.parametrize("where", ["host", "cuda"])
@pytest.mark.parametrize("batch", [256, 0])
def test_tuple_test_equals_restatement(F, scene, batch, where):
    xs, xt, corres = scene["xs"], scene["xt"], scene["corres"]
    dxs, dxt, dcor = _place(where, xs, xt, corres)
    # the count is reached (1000 triples long before 100 m trials)
    want, n_trials = M.tuple_test(xs, xt, corres, 0.95, 1000, seed=0)
    got, nt = F.fgr_tuple_test(dxs, dxt, dcor, 0.95, 1000, seed=0, batch=batch)
    assert isinstance(got, torch.Tensor) == (where == "cuda")
    assert want.shape == (3000, 2) and n_trials < 100 * len(corres)
    assert nt == n_trials and np.array_equal(_np(got).astype(np.int64), want)
    # another seed and scale, a count that is not a multiple of anything
    want, n_trials = M.tuple_test(xs, xt, corres, 0.9, 777, seed=12345)
    got, nt = F.fgr_tuple_test(dxs, dxt, dcor, 0.9, 777, seed=12345, batch=batch)
    assert nt == n_trials and np.array_equal(_np(got).astype(np.int64), want)
    # the count is not reached: every one of the 100 m trials is visited
    few = np.ascontiguousarray(corres[:60])
    want, n_trials = M.tuple_test(xs, xt, few, 0.95, 100000, seed=4)
    got, nt = F.fgr_tuple_test(dxs, dxt, _place(where, few)[0], 0.95, 100000, seed=4, batch=batch)
    assert n_trials == 6000 and 0 < len(want) < 300000
    assert nt == n_trials and np.array_equal(_np(got).astype(np.int64), want)


def test_tuple_test_degenerate_and_errors(F, scene):
    xs, xt, corres = scene["xs"], scene["xt"], scene["corres"]
    got, nt = F.fgr_tuple_test(xs, xt, corres[:0])
    assert got.shape == (0, 2) and nt == 0
    got, nt = F.fgr_tuple_test(xs, xt, corres, maximum_tuple_count=0)
    assert got.shape == (0, 2) and nt == 0
    one = np.repeat(corres[:1], 5, 0)                    # every edge is zero: no trial passes
    got, nt = F.fgr_tuple_test(xs, xt, one)
    assert got.shape == (0, 2) and nt == 500
    bad = torch.from_numpy(corres.copy()).cuda()
    bad[3, 0] = len(xs)                                   # a device array: the kernel finds the row, nothing is read out of bounds
    with pytest.raises(RuntimeError, match="gsr_fgr_tuple_test"):
        F.fgr_tuple_test(torch.from_numpy(xs).cuda(), torch.from_numpy(xt).cuda(), bad)
    with pytest.raises(RuntimeError, match="gsr_fgr_optimize"):
        F.fgr_optimize(torch.from_numpy(xs).cuda(), torch.from_numpy(xt).cuda(), bad)


@pytest.mark.parametrize("decrease_mu,use_absolute_scale,full", list(itertools.product([False, True], [False, True], [False, True])))
def test_optimize_equals_restatement(F, scene, decrease_mu, use_absolute_scale, full):
    """T within 1e-9 of the restatement (float64 both sides; only the order of the sums over the pairs differs), the iteration count
    and scale_global equal; over the tuple list (<= 3000 pairs) and the whole reciprocal set."""
    xs, xt, corres = scene["xs"], scene["xt"], scene["corres"]
    used = corres if full else M.tuple_test(xs, xt, corres, 0.95, 1000, seed=0)[0].astype(np.int32)
    assert len(used) == (len(corres) if full else 3000)
    kw = dict(division_factor=1.4, use_absolute_scale=use_absolute_scale, decrease_mu=decrease_mu,
              maximum_correspondence_distance=1.5 * VOXEL, iteration_number=64)
    want = M.optimize(xs, xt, used, **kw)
    got = F.fgr_optimize(xs, xt, used, **kw)
    err = np.abs(got["transformation"] - want["transformation"]).max()
    print("max |T - T_restatement| = %.3e, iterations %d / %d, scale_global %r / %r" %
          (err, got["iterations"], want["iterations"], got["scale_global"], want["scale_global"]))
    assert err < 1e-9
    assert got["iterations"] == want["iterations"] == 64
    assert got["scale_global"] == want["scale_global"] and (got["scale_global"] == 1.0) == use_absolute_scale
    assert got["n_corres"] == len(used) and got["host_waits"] == 1
    # the same inputs give the same bits, from host arrays and from device tensors
    again = F.fgr_optimize(xs, xt, used, **kw)
    dev = F.fgr_optimize(*_place("cuda", xs, xt, used), **kw)
    assert np.array_equal(again["transformation"], got["transformation"]) and np.array_equal(dev["transformation"], got["transformation"])


def test_optimize_small_and_degenerate(F, scene):
    xs, xt, corres = scene["xs"], scene["xt"], scene["corres"]
    r = F.fgr_optimize(xs, xt, corres[:9])
    assert np.array_equal(r["transformation"], np.eye(4)) and r["iterations"] == 0 and r["n_corres"] == 9 and r["host_waits"] == 1
    assert r["scale_global"] == M.optimize(xs, xt, corres[:9])["scale_global"]
    r = F.fgr_optimize(xs, xt, corres[:10], iteration_number=7)
    w = M.optimize(xs, xt, corres[:10], iteration_number=7)
    assert r["iterations"] == w["iterations"] == 7 and np.abs(r["transformation"] - w["transformation"]).max() < 1e-9
    # every point of a cloud at one place: the scale is 0, the normalised coordinates are 0 / 0, the first solve is not finite and
    # the loop ends with the transform reached so far (the identity in normalised units: the translation between the two means)
    src, tgt = np.tile(np.float32([1, 2, 3]), (20, 1)), np.tile(np.float32([4, 6, 8]), (20, 1))
    ident = np.stack([np.arange(12), np.arange(12)], 1).astype(np.int32)
    r, w = F.fgr_optimize(src, tgt, ident), M.optimize(src, tgt, ident)
    assert r["iterations"] == w["iterations"] == 0 and r["scale_global"] == w["scale_global"] == 0.0
    want = np.eye(4)
    want[:3, 3] = [3, 4, 5]
    assert np.array_equal(r["transformation"], want) and np.array_equal(w["transformation"], want)


def _clouds(scene):
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    return PointCloud(xyz32=scene["xs"], normals=scene["ns"]), PointCloud(xyz32=scene["xt"], normals=scene["nt"])


def test_evaluation_equals_brute_force(F, scene):
    """fitness / inlier_rmse / correspondence_set of the shim against a brute-force float64 nearest-neighbour evaluation."""
    from gaussiansplattingregistration_amd.utils import global_registration_util as U
    a, b = _clouds(scene)
    T = scene["T"]
    for Tq, mc in ((T, 1.5 * VOXEL), (T @ G.make_T(2.0, (0.0, 1.0, 0.0), (0.01, 0.0, 0.0)), 0.6 * VOXEL), (np.eye(4), 1.5 * VOXEL)):
        fit, rmse, cs = M.evaluate(scene["xs"], scene["xt"], mc, Tq)
        r = U.evaluate_registration(a, b, mc, Tq)
        assert r.fitness == fit and abs(r.inlier_rmse - rmse) < 1e-12
        assert np.array_equal(np.asarray(r.correspondence_set, np.int64), cs)
    assert 0.9 < U.evaluate_registration(a, b, 1.5 * VOXEL, T).fitness <= 1.0
    e = U.evaluate_registration(a, b, 0.0, T)
    assert e.fitness == 0.0 and e.inlier_rmse == 0.0 and len(e.correspondence_set) == 0


def test_shims_recover_the_pose(F, scene):
    """FPFH -> reciprocal matches -> tuple test -> optimisation -> evaluation through the Open3D-named shims, the other options
    at their defaults; and the same against the restatement run on the same matches."""
    from gaussiansplattingregistration_amd.utils import global_registration_util as U
    a, b = _clouds(scene)
    T = scene["T"]
    fa = U.compute_fpfh_feature(a, U.KDTreeSearchParamHybrid(5 * VOXEL, 100))
    fb = U.compute_fpfh_feature(b, U.KDTreeSearchParamHybrid(5 * VOXEL, 100))
    opt = U.FastGlobalRegistrationOption(maximum_correspondence_distance=1.5 * VOXEL)
    r = U.registration_fgr_based_on_feature_matching(a, b, fa, fb, opt)
    print("rotation error %.3f deg, translation error %.4f, fitness %.4f" %
          (G.rotation_error_deg(r.transformation, T), np.linalg.norm(r.transformation[:3, 3] - T[:3, 3]), r.fitness))
    assert _pose_ok(r.transformation, T, VOXEL)
    w = M.fgr(scene["xs"], scene["xt"], scene["corres"], maximum_correspondence_distance=1.5 * VOXEL)
    assert np.abs(r.transformation - w["transformation"]).max() < 1e-9
    for k in ("n_corres", "n_reciprocal", "n_trials", "n_tuples", "iterations", "scale_global"):
        assert r.info[k] == w[k], k
    assert r.info["host_waits"] == 1
    fit, rmse, cs = M.evaluate(scene["xs"], scene["xt"], 1.5 * VOXEL, r.transformation)
    assert r.fitness == fit and abs(r.inlier_rmse - rmse) < 1e-12 and np.array_equal(np.asarray(r.correspondence_set, np.int64), cs)
    # without the tuple test the optimiser runs on every reciprocal pair
    r2 = U.registration_fgr_based_on_feature_matching(
        a, b, fa, fb, U.FastGlobalRegistrationOption(1.4, False, True, 1.5 * VOXEL, 64, 0.95, 1000, False))
    assert _pose_ok(r2.transformation, T, VOXEL) and r2.info["n_corres"] == len(scene["corres"]) and r2.info["n_trials"] == 0
    # another seed draws other triples and lands within the same bound
    r3 = U.registration_fgr_based_on_feature_matching(a, b, fa, fb, U.FastGlobalRegistrationOption(maximum_correspondence_distance=1.5 * VOXEL, seed=2))
    assert _pose_ok(r3.transformation, T, VOXEL) and not np.array_equal(r3.transformation, r.transformation)


def _load_pair(tmp_path, T, n=60000):
    """Two independent samplings of the scene written as 3DGS .ply files (the second moved by T), loaded as the reference does:
    GaussianModel.from_ply -> convert_gs_to_open3d_pc (device-resident records)."""
    from gaussiansplattingregistration_amd.models.data_repository import DataRepository, UIStateRepository
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.utils.point_cloud_converter import convert_gs_to_open3d_pc
    pa, pb = tmp_path / "first.ply", tmp_path / "second.ply"
    G.save_scene_ply(str(pa), G.make_scene(n, 1))
    G.save_scene_ply(str(pb), G.transform_scene(G.make_scene(n, 2), T))
    repo, ui = DataRepository(), UIStateRepository()
    for path, gl, ol in ((pa, repo.pc_gaussian_list_first, repo.pc_open3d_list_first), (pb, repo.pc_gaussian_list_second, repo.pc_open3d_list_second)):
        gm = GaussianModel("cuda:0").from_ply(str(path))
        gl.append(gm)
        ol.append(convert_gs_to_open3d_pc(gm))
    assert repo.pc_open3d_list_first[0].xyz32.is_cuda and repo.pc_open3d_list_first[0].cov6.is_cuda
    return repo, ui, pa, pb


@pytest.mark.parametrize("deg,axis", [(120.0, (1.0, 2.0, 0.7)), (60.0, (-0.3, 0.2, 1.0))])
def test_fgr_then_mixture_icp_recovers_T_gt(hip_lib, tmp_path, deg, axis):
    """The Global tab's FGR on device-resident clouds from .ply files, started from a non-identity current pose: do_fgr_registration
    through the worker and the controller lands within 3 degrees and 2 voxels of T_gt; the mixture multiscale ICP from there reaches
    T_gt within 1e-3; the same ICP from the identity does not."""
    from gaussiansplattingregistration_amd import mixture_bind
    from gaussiansplattingregistration_amd.controllers.downsampler_controller import DownsamplerController
    from gaussiansplattingregistration_amd.controllers.registration_controller import RegistrationController
    from gaussiansplattingregistration_amd.params import GaussianMixtureParams
    from gaussiansplattingregistration_amd.params.registration_parameters import FGRRegistrationParams
    from gaussiansplattingregistration_amd.utils.local_registration_util import KernelLossFunctionType, LocalRegistrationType
    from gaussiansplattingregistration_amd.workers.registrators import FGRRegistrator
    T_gt = G.make_T(deg, axis)
    v = VOXEL
    repo, ui, _, _ = _load_pair(tmp_path, T_gt)
    T_ui = G.make_T(10.0, (0.0, 0.3, 1.0), (0.02, 0.01, 0.0))
    ui.transformation_matrix = T_ui.copy()
    params = FGRRegistrationParams(voxel_size=v, maximum_correspondence=1.5 * v)
    # the worker registers the first cloud moved by the current pose, and leaves the clouds it was given alone
    before = repo.pc_open3d_list_first[0].xyz32.clone()
    w = FGRRegistrator(repo.pc_open3d_list_first[0], repo.pc_open3d_list_second[0], T_ui, params).run()
    assert torch.equal(repo.pc_open3d_list_first[0].xyz32, before)
    assert _pose_ok(w.transformation @ T_ui, T_gt, v) and w.info["n_tuples"] == 1000 and w.info["iterations"] == 64
    assert w.fitness > 0.5 and len(w.correspondence_set) > 0
    rc = RegistrationController(repo, ui)
    res = rc.execute_fgr_registration_normal(params)
    assert np.array_equal(res.transformation, w.transformation)                  # deterministic for a given seed
    assert np.allclose(ui.transformation_matrix, res.transformation @ T_ui)
    T_global = ui.transformation_matrix.copy()
    assert _pose_ok(T_global, T_gt, v), (G.rotation_error_deg(T_global, T_gt), T_global, T_gt)
    mixture_bind.reset_rng()
    DownsamplerController(repo).create_mixture(GaussianMixtureParams(cluster_level=2))
    icp = (False, "", "", LocalRegistrationType.ICP_Point_To_Plane, 1e-7, 1e-7, [0.3, 0.15, 0.08], [40, 30, 20],
           KernelLossFunctionType.Loss_None, 0.0, True)
    out = rc.execute_multiscale_registration(*icp)
    assert out is not None, rc.errors
    T = out.result.transformation
    assert np.linalg.norm(T - T_gt) < 1e-3, (np.linalg.norm(T - T_gt), T, T_gt)
    # without the global step: the same ICP from the identity
    ui.transformation_matrix = np.eye(4)
    out0 = rc.execute_multiscale_registration(*icp)
    T0 = out0.result.transformation if out0 is not None else np.eye(4)
    assert np.linalg.norm(T0 - T_gt) > 0.1, T0


def test_register_ply_global_fgr(hip_lib, tmp_path):
    """scripts/register_ply.py --global-fgr on a real .ply pair: the global step runs on device-resident clouds, then the ICP; the
    two global methods exclude each other."""
    from conftest import ROOT
    T_gt = G.make_T()
    pa, pb = tmp_path / "first.ply", tmp_path / "second.ply"
    G.save_scene_ply(str(pa), G.make_scene(40000, 1))
    G.save_scene_ply(str(pb), G.transform_scene(G.make_scene(40000, 2), T_gt))
    script = os.path.join(ROOT, "scripts", "register_ply.py")
    r = subprocess.run([sys.executable, script, str(pa), str(pb), "--global-fgr", "0.05", "--levels", "2", "--max-corr", "0.3", "0.15", "0.08",
                        "--iters", "40", "30", "20"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "global FGR" in r.stdout
    rows = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("[") or ln.strip().startswith("[[")]
    T = np.array([[float(x) for x in ln.replace("[", " ").replace("]", " ").split()] for ln in rows[:4]])
    assert T.shape == (4, 4) and np.linalg.norm(T - T_gt) < 1e-3, (T, T_gt)
    r = subprocess.run([sys.executable, script, str(pa), str(pb), "--global-fgr", "0.05", "--global-ransac", "0.05"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "not allowed with" in r.stderr
