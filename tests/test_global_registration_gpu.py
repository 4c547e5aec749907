"""Global registration on the MI355X (csrc/features.hip) against the NumPy restatement (tests/global_model.py), at workload-like
shapes.  The small, lattice and degenerate inputs, the sizes on either side of each kernel's tile, chunk and block, and the second
trips of the grid-stride loops live in tests/test_global_edges_gpu.py."""
import numpy as np
import pytest
import torch

import global_model as G
from global_model import _near_edge_rows, _ransac_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F(hip_lib):
    from gaussiansplattingregistration_amd import features
    return features


def _down(n, seed, voxel, T=None, orient=None):
    sc = G.make_scene(n, seed)
    if T is not None:
        sc = G.transform_scene(sc, T)
    P, C = G.voxel_down(sc["xyz"], sc["cov6"], voxel)
    N = G.normals_from_cov(C)
    if orient is not None:
        N = np.where(((orient - P) * N).sum(1, keepdims=True) < 0, -N, N)
    return P.astype(np.float32), N


def _with_specials(xyz, nrm):
    """an isolated point and a clump of 150 coincident-ish points (more than 100 neighbours)"""
    far = np.array([[50.0, 50.0, 50.0]], np.float32)
    c = xyz[len(xyz) // 2] + (np.random.default_rng(0).normal(size=(150, 3)) * 1e-3).astype(np.float32)
    x = np.vstack([xyz, far, c]).astype(np.float32)
    n = np.vstack([nrm, [[0.0, 0.0, 1.0]], np.repeat(nrm[len(xyz) // 2][None], 150, 0)])
    return x, n


def test_hybrid_search_equals_restatement(F):
    xyz, nrm = _with_specials(*_down(20000, 1, 0.03))
    nbr, cnt = F.hybrid_search(xyz, 0.1, 100)
    want = G.hybrid_search(xyz, 0.1, 100)
    assert cnt[len(xyz) - 151] == 1 and cnt.max() == 100
    for i in range(len(xyz)):
        assert cnt[i] == len(want[i]) and np.array_equal(nbr[i, :cnt[i]], want[i]), i


# splat counts and voxels that give about 1 k, 20 k and 100 k points after down-sampling (plus the 151 special points)
@pytest.mark.parametrize("n,voxel", [(20000, 0.09), (200000, 0.02), (600000, 0.009)])
def test_fpfh_equals_restatement(F, n, voxel):
    xyz, nrm = _with_specials(*_down(n, 2, voxel))
    r = 5 * voxel
    got = F.fpfh(xyz, nrm, r, 100)
    nbrs = G.hybrid_search(xyz, r, 100)
    spfh, want = G.spfh_fpfh(xyz, nrm, r, 100, nbrs)
    assert got.shape == (len(xyz), 33)
    print("points", len(xyz))
    assert np.all(got[len(xyz) - 151] == 0.0)                      # the isolated point
    assert max(len(x) for x in nbrs) == 100                        # the clump: more than 100 within the radius
    ok = np.all(np.abs(got - want) < 1e-9, axis=1)
    assert ok.mean() >= 0.999, (len(xyz), ok.mean())
    # every other row is explained by a pair feature at a bin edge of the row's own SPFH or a neighbour's
    assert np.all(_near_edge_rows(xyz, nrm, nbrs)[~ok]), np.flatnonzero(~ok)[:10]
    # device in, device out: the same values
    dev = F.fpfh(torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda(), r, 100)
    assert torch.equal(dev.cpu(), torch.from_numpy(got))


def test_feature_match_equals_restatement(F):
    rng = np.random.default_rng(3)
    fs = rng.random((3000, 33)) * 50
    ft = rng.random((2500, 33)) * 50
    ft[100] = ft[7]                                                 # duplicated rows: ties go to the lowest index
    fs[5] = ft[100]
    for mutual in (False, True):
        c, um, nst, nts = F.feature_match(fs, ft, mutual=mutual, return_nn=True)
        wc, wum, wst, wts = G.feature_match(fs, ft, mutual)
        assert np.array_equal(nst, wst) and um == wum and np.array_equal(c, wc)
        if mutual:
            assert np.array_equal(nts, wts)
        assert nst[5] == 7
        dc, dum = F.feature_match(torch.from_numpy(fs).cuda(), torch.from_numpy(ft).cuda(), mutual=mutual)
        assert torch.equal(dc.cpu(), torch.from_numpy(c.astype(np.int32))) and dum == um
    # the fall-back: too few mutual pairs for ransac_n = 3000 -> the one-way set
    c, um = F.feature_match(fs, ft, mutual=True, ransac_n=3000)
    assert not um and len(c) == len(fs)


CHECKS = {"none": [], "edge": [(0, 0.9)], "dist": [(1, 0.03)], "normal": [(2, 0.5)], "all": [(0, 0.9), (1, 0.03), (2, 0.5)]}


@pytest.mark.parametrize("checks", sorted(CHECKS))
def test_ransac_equals_serial_restatement(F, checks):
    src, tgt, ns, nt, corres, T = _ransac_case()
    kw = dict(ransac_n=3, checkers=CHECKS[checks], max_iteration=3000, confidence=0.999, seed=11)
    got = F.ransac_correspondence(src, tgt, corres, 0.02, src_normals=ns, tgt_normals=nt, batch=256, **kw)
    want = G.ransac(src, tgt, corres, 0.02, src_normals=ns, tgt_normals=nt, **kw)
    for k in ("best_index", "exit_index", "n_evaluated", "n_valid"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["fitness"] == want["fitness"]
    assert abs(got["inlier_rmse"] - want["inlier_rmse"]) < 1e-12
    assert np.abs(got["transformation"] - want["transformation"]).max() < 1e-9
    assert np.abs(got["transformation"] - T).max() < 1e-4
    # the batch size is a speed knob only, and runs repeat to the bit
    for b in (8192, 256):
        again = F.ransac_correspondence(src, tgt, corres, 0.02, src_normals=ns, tgt_normals=nt, batch=b, **kw)
        assert all(np.array_equal(np.asarray(got[k]), np.asarray(again[k])) for k in got)


def test_ransac_point_to_plane(F):
    # point-to-plane is Open3D's linearised step: a small motion, as in the ICP that uses it
    T0 = np.eye(4)
    T0[:3, :3] = G.rot((0.2, 1.0, 0.3), 2.0)
    T0[:3, 3] = (0.01, -0.004, 0.006)
    src, tgt, ns, nt, corres, T = _ransac_case(m=600, inlier=0.7, curved=True, T=T0)
    kw = dict(kind=F.KIND_POINT_TO_PLANE, ransac_n=6, max_iteration=2000, confidence=0.99, seed=3)
    got = F.ransac_correspondence(src, tgt, corres, 0.02, tgt_normals=nt, **kw)
    want = G.ransac(src, tgt, corres, 0.02, tgt_normals=nt, **kw)
    assert got["best_index"] == want["best_index"] and got["fitness"] == want["fitness"]
    assert got["n_evaluated"] == want["n_evaluated"]
    assert np.abs(got["transformation"] - want["transformation"]).max() < 1e-9


def test_ransac_degenerate_and_errors(F):
    src, tgt, ns, nt, corres, T = _ransac_case(m=50)
    for kw in ({"ransac_n": 2}, {"max_corr": 0.0}, {"corres": corres[:2]}):
        args = dict(corres=corres, max_corr=0.02, ransac_n=3)
        args.update(kw)
        r = F.ransac_correspondence(src, tgt, args["corres"], args["max_corr"], ransac_n=args["ransac_n"])
        assert r["best_index"] == -1 and r["fitness"] == 0.0 and r["inlier_rmse"] == 0.0
        assert np.array_equal(r["transformation"], np.eye(4))
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.utils import global_registration_util as U
    a, b = PointCloud(xyz32=src), PointCloud(xyz32=tgt)
    for e in (U.RANSACEstimationMethod.TransformationEstimationForGeneralizedICP, U.RANSACEstimationMethod.TransformationEstimationForColoredICP):
        with pytest.raises(RuntimeError):
            U.registration_ransac_based_on_correspondence(a, b, corres, 0.02, U.get_estimation_method_from_enum(e))
    with pytest.raises(RuntimeError):
        F.ransac_correspondence(src, tgt, corres, 0.02, kind=F.KIND_POINT_TO_PLANE)      # no target normals


@pytest.mark.parametrize("deg,axis", [(120.0, (1.0, 2.0, 0.7)), (45.0, (-0.3, 0.2, 1.0))])
def test_feature_matching_registration_recovers_pose(F, deg, axis):
    """FPFH -> matching -> RANSAC on two independent samplings of the scene, the second moved by T_gt, through the Open3D-named shims
    (normals from the covariances, turned towards each cloud's centroid as preprocess_point_cloud does)."""
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.utils import global_registration_util as U
    T = G.make_T(deg, axis)
    v = 0.05
    xs, ns = _down(60000, 1, v)
    xt, nt = _down(60000, 2, v, T=T)
    a = U.orient_normals_towards_centroid(PointCloud(xyz32=xs, normals=ns))
    b = U.orient_normals_towards_centroid(PointCloud(xyz32=xt, normals=nt))
    fa = U.compute_fpfh_feature(a, U.KDTreeSearchParamHybrid(5 * v, 100))
    fb = U.compute_fpfh_feature(b, U.KDTreeSearchParamHybrid(5 * v, 100))
    assert fa.data.shape == (33, len(xs)) and fa.dimension() == 33 and fa.num() == len(xs)
    r = U.registration_ransac_based_on_feature_matching(a, b, fa, fb, True, 1.5 * v, U.TransformationEstimationPointToPoint(), 3,
                                                        [U.CorrespondenceCheckerBasedOnEdgeLength(0.9), U.CorrespondenceCheckerBasedOnDistance(1.5 * v)],
                                                        U.RANSACConvergenceCriteria(100000, 0.999))
    assert G.rotation_error_deg(r.transformation, T) < 3.0
    assert np.linalg.norm(r.transformation[:3, 3] - T[:3, 3]) < 2 * v


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


def _pose_ok(T, T_gt, voxel):
    return G.rotation_error_deg(T, T_gt) < 3.0 and np.linalg.norm(T[:3, 3] - T_gt[:3, 3]) < 2 * voxel


@pytest.mark.parametrize("deg,axis", [(120.0, (1.0, 2.0, 0.7)), (60.0, (-0.3, 0.2, 1.0))])
def test_global_then_mixture_icp_recovers_T_gt(hip_lib, tmp_path, deg, axis):
    """The Global tab on device-resident clouds from .ply files, started from a non-identity current pose: do_ransac_registration
    through the controller lands within 3 degrees and 2 voxels of T_gt; the mixture multiscale ICP from there reaches T_gt within
    1e-3; the same ICP from the identity does not."""
    from gaussiansplattingregistration_amd import mixture_bind
    from gaussiansplattingregistration_amd.controllers.downsampler_controller import DownsamplerController
    from gaussiansplattingregistration_amd.controllers.registration_controller import RegistrationController
    from gaussiansplattingregistration_amd.params import GaussianMixtureParams
    from gaussiansplattingregistration_amd.params.registration_parameters import RANSACRegistrationParams
    from gaussiansplattingregistration_amd.utils.local_registration_util import KernelLossFunctionType, LocalRegistrationType
    from gaussiansplattingregistration_amd.utils import global_registration_util as U
    T_gt = G.make_T(deg, axis)
    v = 0.05
    repo, ui, _, _ = _load_pair(tmp_path, T_gt)
    T_ui = G.make_T(10.0, (0.0, 0.3, 1.0), (0.02, 0.01, 0.0))
    ui.transformation_matrix = T_ui.copy()
    rc = RegistrationController(repo, ui)
    params = RANSACRegistrationParams(voxel_size=v, mutual_filter=True, max_correspondence=1.5 * v,
                                      checkers=[U.CorrespondenceCheckerBasedOnEdgeLength(0.9), U.CorrespondenceCheckerBasedOnDistance(1.5 * v)])
    res = rc.execute_ransac_registration_normal(params)
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


def test_worker_moves_points_normals_and_covariances(hip_lib):
    """RANSACRegistrator moves the first cloud by the current pose first: with the covariances rotated too, a source handed over in
    another frame gives the same composed pose as the same source already in that frame."""
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.params.registration_parameters import RANSACRegistrationParams
    from gaussiansplattingregistration_amd.workers.registrators import RANSACRegistrator
    T_gt = G.make_T()
    v = 0.05
    a, b = G.make_scene(60000, 1), G.transform_scene(G.make_scene(60000, 2), T_gt)
    T_ui = G.make_T(35.0, (1.0, 0.0, 0.2), (0.1, 0.0, 0.0))
    a_ui = G.transform_scene(a, np.linalg.inv(T_ui))                # the source as handed over: T_ui brings it back
    tgt = PointCloud(xyz32=torch.from_numpy(b["xyz"]).cuda(), cov6=torch.from_numpy(b["cov6"]).cuda())
    p = RANSACRegistrationParams(voxel_size=v, mutual_filter=True, max_correspondence=1.5 * v)
    r1 = RANSACRegistrator(PointCloud(xyz32=torch.from_numpy(a_ui["xyz"]).cuda(), cov6=torch.from_numpy(a_ui["cov6"]).cuda()), tgt, T_ui, p).run()
    r0 = RANSACRegistrator(PointCloud(xyz32=torch.from_numpy(a["xyz"]).cuda(), cov6=torch.from_numpy(a["cov6"]).cuda()), tgt, np.eye(4), p).run()
    # the worker registers the MOVED source: its result is the pose of the source once moved, and the controller composes it with T_ui
    T1, T0 = r1.transformation, r0.transformation
    assert _pose_ok(T0, T_gt, v) and _pose_ok(T1, T_gt, v), (G.rotation_error_deg(T0, T_gt), G.rotation_error_deg(T1, T_gt))
    # (the two frames voxelise the source on different grids, so the two runs see different down-sampled clouds: they agree to RANSAC's
    # accuracy, not to the bit; unrotated covariances give normals of the wrong frame and fail the line above by tens of degrees)
    assert G.rotation_error_deg(T0, T1) < 2.0
    assert _pose_ok(T1 @ T_ui, T_gt @ T_ui, v)                      # = the pose of the source as handed over


def test_register_ply_global_ransac(hip_lib, tmp_path):
    """scripts/register_ply.py --global-ransac on a real .ply pair: the global step runs on device-resident clouds, then the ICP."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    T_gt = G.make_T()
    pa, pb = tmp_path / "first.ply", tmp_path / "second.ply"
    G.save_scene_ply(str(pa), G.make_scene(40000, 1))
    G.save_scene_ply(str(pb), G.transform_scene(G.make_scene(40000, 2), T_gt))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "register_ply.py"), str(pa), str(pb), "--global-ransac", "0.05",
                        "--ransac-iters", "20000", "--levels", "2", "--max-corr", "0.3", "0.15", "0.08", "--iters", "40", "30", "20"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "global RANSAC" in r.stdout
    rows = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("[") or ln.strip().startswith("[[")]
    T = np.array([[float(x) for x in ln.replace("[", " ").replace("]", " ").split()] for ln in rows[:4]])
    assert T.shape == (4, 4) and np.linalg.norm(T - T_gt) < 1e-3, (T, T_gt)
