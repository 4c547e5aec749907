"""Multiway registration on the GPU: the information-matrix kernel (gsr_icp_information) against tests/posegraph_model.py, the
driver (workers/multiway.py) on four overlapping fragments of one scene, the N-way merge and scripts/register_many.py.
Open3D is absent: parity with get_information_matrix_from_point_clouds / global_optimization is unpinned; the model is the reference.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import posegraph_model as M
import test_model_transform_gpu as MT
from gaussiansplattingregistration_amd import icp, synth
from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
from gaussiansplattingregistration_amd.params.registration_parameters import LocalRegistrationParams
from gaussiansplattingregistration_amd.utils import pose_graph as PG
from gaussiansplattingregistration_amd.utils.local_registration_util import (LocalRegistrationType, do_icp_registration,
                                                                             get_information_matrix_from_point_clouds)
from gaussiansplattingregistration_amd.workers.multiway import MultiwayRegistrator, initial_poses

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------- information matrix
def _pair(ns, tgt, T_gt, seed, angle=4.0, spare=0, max_corr=0.03):
    """ns source points, each a target point (+ 1e-3 noise) seen through inv(T_gt); T = T_gt turned by `angle` degrees, which leaves
    about a third of them without a target point within 0.03 (measured with the model: 33-35 % at 4 degrees on the 2000-point
    target).  spare > 0: that many more are drawn and the points whose squared distance lies within 1e-7 of the gate are left out
    before the first ns are taken (among 400 000 points some land within 1e-9 of it by chance, where two float64 evaluations of the
    distance may disagree about the strict <)."""
    rng = np.random.default_rng(seed)
    moved = tgt[rng.integers(0, len(tgt), ns + spare)].astype(np.float64) + 1e-3 * rng.normal(size=(ns + spare, 3))
    Ti = np.linalg.inv(T_gt)
    src = (moved @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    T = synth.rigid_transform(angle, (0.3, 1.0, -0.5)) @ T_gt
    if spare:
        _, d2 = M.correspondences(src, tgt, T, max_corr)
        src = src[np.abs(d2 - max_corr * max_corr) >= 1e-7]
        assert len(src) >= ns
    return np.ascontiguousarray(src[:ns]), T


def _check_information(src, tgt, T, max_corr, lo, hi):
    j, d2 = M.correspondences(src, tgt, T, max_corr)
    margin = np.abs(d2 - max_corr * max_corr).min()
    want, n_want = M.information_from_points(tgt.astype(np.float64)[j[j >= 0]]), int((j >= 0).sum())
    frac = 1.0 - n_want / len(src)
    with icp.IcpContext(device=0) as ctx:
        ctx.set_target(tgt, None, max_corr)
        ctx.set_source(src)
        got, n = ctx.information(T)
        again, n2 = ctx.information(T)
        far = T.copy()
        far[:3, 3] += 100.0
        zero, n0 = ctx.information(far)
    err = np.abs(got - want).max() / np.abs(want).max() if n_want else np.abs(got).max()
    print(f"ns {len(src)}: {n} correspondences (model {n_want}), {100 * frac:.1f} % without, gate margin {margin:.2e}, relative error {err:.2e}")
    assert margin > 1e-9                                    # the strict < cannot flip between float64 evaluations
    assert lo <= frac <= hi
    assert n == n_want and got[5, 5] == n_want
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    assert np.array_equal(got, got.T)
    assert got.tobytes() == again.tobytes() and n == n2
    assert n0 == 0 and not zero.any()
    return got


@pytest.fixture(scope="module")
def pair2000():
    _, tgt, T_gt = synth.make_pair(2000, seed=0)
    return tgt["xyz"], T_gt


@pytest.mark.parametrize("ns", [1, 63, 257, 3001])
def test_information_against_model(pair2000, ns):
    """One lane, less than a wave, a block and a lane, several blocks with a ragged tail.  n_corr exact, the matrix within
    1e-10 max|Lambda| (n 2^-52 at the largest n: a reordered float64 sum), two calls bit-identical, nothing in reach -> zero."""
    tgt, T_gt = pair2000
    src, T = _pair(ns, tgt, T_gt, 100 + ns)
    _check_information(src, tgt, T, 0.03, 0.0 if ns == 1 else 0.25, 1.0 if ns == 1 else 0.45)


def test_information_search_kernel_path():
    """400 037 source points (above the 400 000 of nn_mode(): k_icp_nn + the streaming pass) against a 50 000-point target"""
    _, tgt, T_gt = synth.make_pair(50000, seed=1)
    tgt = tgt["xyz"]
    src, T = _pair(400037, tgt, T_gt, 7, angle=1.4, spare=200)
    _check_information(src, tgt, T, 0.03, 0.2, 0.5)


def test_information_agrees_with_correspondences(pair2000):
    tgt, T_gt = pair2000
    src, T = _pair(3001, tgt, T_gt, 5)
    with icp.IcpContext(device=0) as ctx:
        ctx.set_target(tgt, None, 0.03)
        ctx.set_source(src)
        got, n = ctx.information(T)
        idx, _ = ctx.correspondences(T)
        ctx.set_allreduce(lambda acc: None, len(src))
        with pytest.raises(RuntimeError, match="gsr_icp_information"):
            ctx.information(T)
        ctx.set_allreduce(None, 0)
        assert ctx.information(T)[0].tobytes() == got.tobytes()
    want = M.information_from_points(tgt.astype(np.float64)[idx[idx >= 0]])
    assert n == int((idx >= 0).sum())
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    shim = get_information_matrix_from_point_clouds(PointCloud(xyz32=src), PointCloud(xyz32=tgt), 0.03, T)
    assert shim.tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------------------- four fragments
EDGES = [(0, 1), (1, 2), (2, 3), (0, 2), (1, 3)]
MAX_CORR = 0.05


def make_fragments(pose_size):
    """synth.make_cloud(12000, seed=0, sh_degree=0) cut into four slabs along x, slab i over [i/6, i/6 + 1/2] of the width, each
    moved into a frame of its own: frame_i = inv(P_i) world.  -> (cloud, list of index arrays, list of P_i, list of float32 xyz in frame i)"""
    cloud = synth.make_cloud(12000, seed=0, sh_degree=0)
    x, h = cloud["xyz"][:, 0].astype(np.float64), cloud["h"]
    u = (x + h) / (2 * h)
    rng = np.random.default_rng(42)
    idx, poses, frames = [], [], []
    for i in range(4):
        sel = np.nonzero((u >= i / 6) & (u <= i / 6 + 0.5))[0]
        P = np.eye(4) if i == 0 else M.pose(rng.normal(size=3) * pose_size, rng.normal(size=3) * pose_size)
        Pi = M.inv(P)
        idx.append(sel)
        poses.append(P)
        frames.append((cloud["xyz"][sel].astype(np.float64) @ Pi[:3, :3].T + Pi[:3, 3]).astype(np.float32))
    return cloud, idx, poses, frames


def edge_truth(poses, s, t):
    return M.inv(poses[t]) @ poses[s]


@pytest.fixture(scope="module")
def fragments():
    cloud, idx, poses, frames = make_fragments(0.15)
    rng = np.random.default_rng(9)
    init = {(s, t): M.pose(rng.normal(size=3) * 0.006, rng.normal(size=3) * 0.006) @ edge_truth(poses, s, t) for s, t in EDGES}     # ~0.01 rad / 0.01 units
    clouds = [PointCloud(xyz32=f) for f in frames]
    params = LocalRegistrationParams(registration_type=LocalRegistrationType.ICP_Point_To_Point, max_correspondence=MAX_CORR, max_iteration=30)
    worker = MultiwayRegistrator(clouds, params, edges=EDGES, init=init)
    res = worker.run()
    assert res is not None, worker.errors
    return {"poses": poses, "clouds": clouds, "params": params, "init": init, "res": res}


def _bound(reports, poses):
    errs = [np.linalg.norm(r["transformation"] - edge_truth(poses, r["source"], r["target"])) for r in reports]
    return (len(poses) - 1) * max(errs), errs


def test_four_fragments(fragments):
    f = fragments
    res, poses = f["res"], f["poses"]
    assert [len(c) for c in f["clouds"]] == pytest.approx([6000] * 4, rel=0.05)
    bound, errs = _bound(res.edge_reports, poses)
    got = [np.linalg.norm(X - P) for X, P in zip(res.poses, poses)]
    print("fitness", [round(r["fitness"], 3) for r in res.edge_reports], "iterations", [r["iterations"] for r in res.edge_reports])
    print("pairwise errors", [f"{e:.2e}" for e in errs], "pose errors", [f"{e:.2e}" for e in got], f"bound {bound:.2e}")
    print("line process", res.optimization.line_process, res.optimization)
    assert all(r["fitness"] > 0.2 for r in res.edge_reports)
    assert max(got) <= bound
    assert not res.optimization.pruned.any() and (res.optimization.line_process >= 0.9).all()
    assert len(res.pose_graph.edges) == len(EDGES)
    assert [r["uncertain"] for r in res.edge_reports] == [False, False, False, True, True]
    # one false edge (0, 3) through the API: a wrong transform with the information matrix of edge (0, 1)
    g = PG.PoseGraph()
    g.nodes = [PG.PoseGraphNode(n.pose) for n in res.pose_graph.nodes]
    g.edges = [PG.PoseGraphEdge(e.source_node_id, e.target_node_id, e.transformation, e.information, e.uncertain) for e in res.pose_graph.edges]
    wrong = M.pose([0.3, -0.35, 0.25], [0.4, -0.3, 0.33]) @ edge_truth(poses, 0, 3)
    g.edges.append(PG.PoseGraphEdge(0, 3, wrong, res.edge_reports[0]["information"], True))
    rep = PG.global_optimization(g, None, PG.GlobalOptimizationOption(max_correspondence_distance=MAX_CORR))
    got = [np.linalg.norm(n.pose - P) for n, P in zip(g.nodes, poses)]
    print("with the false edge: line process", rep.line_process, "pose errors", [f"{e:.2e}" for e in got])
    assert list(rep.pruned) == [False] * len(EDGES) + [True]
    assert (rep.line_process[:-1] >= 0.9).all() and rep.line_process[-1] < 0.25
    assert max(got) <= bound


def test_driver_is_the_composition_of_its_parts(fragments):
    f = fragments
    g = PG.PoseGraph()
    for s, t in EDGES:
        r = do_icp_registration(f["clouds"][s], f["clouds"][t], f["init"][(s, t)], f["params"])
        with icp.IcpContext(device=0) as ctx:
            ctx.set_target(f["clouds"][t].xyz32, None, MAX_CORR)
            ctx.set_source(f["clouds"][s].xyz32)
            info, _ = ctx.information(r.transformation)
        g.edges.append(PG.PoseGraphEdge(s, t, r.transformation, info, t != s + 1))
    X = [np.eye(4)]
    for i in range(3):
        X.append(X[i] @ np.linalg.inv(g.edges[i].transformation))            # chained odometry
    assert all(np.array_equal(a, b) for a, b in zip(X, initial_poses(4, [(e.source_node_id, e.target_node_id, e.transformation, e.uncertain) for e in g.edges])))
    g.nodes = [PG.PoseGraphNode(P) for P in X]
    rep = PG.global_optimization(g, None, PG.GlobalOptimizationOption(max_correspondence_distance=MAX_CORR))
    res = f["res"]
    assert len(g.edges) == len(res.pose_graph.edges)
    for a, b in zip(g.edges, res.pose_graph.edges):
        assert (a.source_node_id, a.target_node_id, a.uncertain) == (b.source_node_id, b.target_node_id, b.uncertain)
        assert a.transformation.tobytes() == b.transformation.tobytes() and a.information.tobytes() == b.information.tobytes()
        assert a.confidence == b.confidence
    for a, b in zip(g.nodes, res.pose_graph.nodes):
        assert a.pose.tobytes() == b.pose.tobytes()
    assert rep.line_process.tobytes() == res.optimization.line_process.tobytes()


# ------------------------------------------------------------------------------------------------------------- N-way merge
NAMES = ("_xyz", "_rotation", "_scaling", "_features_dc", "_features_rest", "_opacity", "_covariance")


@pytest.mark.parametrize("rotate_sh", [False, True])
def test_merge_multi(rotate_sh):
    """Three models, SH degree 1: slice i is bit for bit transform_gaussian_model(poses[i]) of model i alone; the model with the
    identity pose is bit for bit its input; the inputs are left as they were."""
    models = [MT.make_model(n, 1, seed)[0] for n, seed in ((300, 1), (257, 2), (1000, 3))]
    poses = [np.eye(4), synth.rigid_transform(25.0, (0.2, 1.0, -0.4), (0.3, -0.1, 0.2)), synth.rigid_transform(-70.0, (1.0, 0.1, 0.3), (-0.5, 0.4, 0.1))]
    before = [{k: getattr(m, k).clone() for k in NAMES} for m in models]
    merged = GaussianModel.get_merged_gaussian_point_clouds_multi(models, poses, rotate_sh=rotate_sh)
    assert len(merged) == 300 + 257 + 1000 and merged.sh_degree == 1
    off = 0
    for i, (m, T) in enumerate(zip(models, poses)):
        alone = m.clone_gaussian()
        if i > 0:
            alone.transform_gaussian_model(T, rotate_sh=rotate_sh)
        for k in NAMES:
            a, b = getattr(merged, k)[off:off + len(m)], getattr(alone, k)
            assert a.shape == b.shape and torch.equal(a, b), (i, k)
            assert torch.equal(getattr(m, k), before[i][k]), (i, k)
        if i > 0:
            assert not torch.equal(merged._xyz[off:off + len(m)], m._xyz)
            assert torch.equal(merged._features_rest[off:off + len(m)], m._features_rest) != rotate_sh
        off += len(m)
    with pytest.raises(ValueError):
        GaussianModel.get_merged_gaussian_point_clouds_multi(models, poses[:2])


# ------------------------------------------------------------------------------------------------------------- command line
def test_register_many_command_line(tmp_path):
    """scripts/register_many.py as a child process on three fragments (SH degree 0) whose frames differ by about 0.01 rad / 0.01
    units, so the identity start of the script lies within reach of a 0.05 correspondence distance: merged.ply has every row, and
    the poses of poses.json lie within test_four_fragments' bound, computed from the edges the file reports."""
    from conftest import ROOT
    from gaussiansplattingregistration_amd.utils import ply_io
    cloud, idx, poses, frames = make_fragments(0.006)
    paths = []
    for i in range(3):
        sel = idx[i]
        m = GaussianModel("cuda:0").from_arrays(frames[i], cloud["color"][sel], cloud["opacity"][sel], cloud["cov6"][sel], cloud["sh"][sel], 0)
        m._scaling = torch.full((len(sel), 3), -2.5, device="cuda:0")
        m._rotation = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device="cuda:0").repeat(len(sel), 1)
        paths.append(str(tmp_path / f"fragment{i}.ply"))
        m.save_ply(paths[-1])
    out, pj = str(tmp_path / "merged.ply"), str(tmp_path / "poses.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "register_many.py"), *paths, "--edges", "all", "--type", "point", "--max-corr", "0.05",
                        "--out", out, "--poses-out", pj], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    assert len(ply_io.load_gaussian_arrays(out)["xyz"]) == sum(len(idx[i]) for i in range(3))
    doc = json.load(open(pj))
    assert [(e["source"], e["target"]) for e in doc["edges"]] == [(0, 1), (0, 2), (1, 2)] and doc["pruned"] == []
    assert all("line_process" in e for e in doc["edges"])
    errs = [np.linalg.norm(np.array(e["transformation"]) - edge_truth(poses, e["source"], e["target"])) for e in doc["edges"]]
    got = [np.linalg.norm(np.array(X) - P) for X, P in zip(doc["poses"], poses)]
    print("pairwise errors", errs, "pose errors", got)
    assert max(got) <= 2 * max(errs)                       # (N - 1) max_e |T_e - T_gt,e| with N = 3
