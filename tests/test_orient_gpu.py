"""Consistent normal orientation on the GPU (csrc/orient.hip) against the CPU models of tests/orient_model.py: exact, since the
definition has no floating-point sum whose order could differ."""
import numpy as np
import pytest
import torch

import orient_model as M

pytestmark = pytest.mark.gpu

CASES = ["torus", "sheets", "chain", "junk", "sphere", "tiny1", "tiny2", "tiny3"]
COUNTS = ("n", "n_components", "n_flipped", "n_not_live", "rounds")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _check(case, want, out, info):
    """the flip set, the labels and the report are the model's; every row is +- its input bit for bit, dead rows untouched"""
    nrm = np.asarray(case["normals"], np.float64)
    out = out.cpu().numpy() if torch.is_tensor(out) else out
    comp = info["component"].cpu().numpy() if torch.is_tensor(info["component"]) else info["component"]
    same = (_bits(out) == _bits(nrm)).all(1)
    negated = (_bits(out) == _bits(-nrm)).all(1)
    live = np.isfinite(nrm).all(1)
    assert (same | negated).all()
    assert same[~live].all()
    flipped = negated & ~same                                         # (a zero normal equals its negation nowhere: -0.0 has other bits)
    got = {k: info[k] for k in COUNTS}
    print({k: (got[k], want[k]) for k in COUNTS}, "flip mismatches", int((flipped != want["flip"]).sum()), "label mismatches",
          int((comp != want["component"]).sum()))
    assert np.array_equal(flipped, want["flip"])
    assert np.array_equal(comp, want["component"])
    assert got == {k: want[k] for k in COUNTS}
    assert info["rounds"] <= 31


@pytest.mark.parametrize("name", CASES)
def test_graph_matches_the_model_host_arrays(hip_lib, name):
    from gaussiansplattingregistration_amd import orient
    c = M.gpu_cases()[name]
    out, info = orient.orient_normals_graph(c["xyz"], c["normals"], c["nbr"], c["count"], c["reference"])
    assert isinstance(out, np.ndarray) and isinstance(info["component"], np.ndarray)
    _check(c, M.expected(name), out, info)


@pytest.mark.parametrize("name", CASES)
def test_graph_matches_the_model_device_tensors(hip_lib, name):
    from gaussiansplattingregistration_amd import orient
    c = M.gpu_cases()[name]
    t = {k: torch.from_numpy(np.array(c[k])).cuda() for k in ("xyz", "normals", "nbr", "count")}
    before = t["normals"].clone()
    out, info = orient.orient_normals_graph(t["xyz"], t["normals"], t["nbr"], t["count"], c["reference"])
    assert out.is_cuda and info["component"].is_cuda
    assert torch.equal(before.view(torch.int64), t["normals"].view(torch.int64))      # the input is not written
    _check(c, M.expected(name), out, info)


def test_two_runs_give_the_same_bytes(hip_lib):
    from gaussiansplattingregistration_amd import orient
    c = M.gpu_cases()["torus"]
    a, ia = orient.orient_normals_graph(c["xyz"], c["normals"], c["nbr"], c["count"], c["reference"])
    b, ib = orient.orient_normals_graph(c["xyz"], c["normals"], c["nbr"], c["count"], c["reference"])
    assert a.tobytes() == b.tobytes() and ia["component"].tobytes() == ib["component"].tobytes()
    assert {k: ia[k] for k in COUNTS} == {k: ib[k] for k in COUNTS}


def test_sphere_looks_at_its_centroid_and_moves_with_the_cloud(hip_lib):
    from gaussiansplattingregistration_amd import orient, synth
    c = M.gpu_cases()["sphere"]
    p = c["xyz"].astype(np.float64)
    # on the model first: the vote is not within 10 % of a tie
    free = M.boruvka(c["xyz"], c["normals"], c["nbr"], c["count"], None)
    t = ((c["reference"] - p) * free["normals"]).sum(1)
    toward, away = int((t > 0).sum()), int((t < 0).sum())
    assert abs(toward - away) > 0.1 * (toward + away)
    out, info = orient.orient_normals_graph(c["xyz"], c["normals"], c["nbr"], c["count"], c["reference"])
    assert info["n_components"] == 1
    assert (((c["reference"] - p) * out).sum(1) >= 0).all()           # the convention of orient_normals_towards_centroid
    flips = (_bits(out) != _bits(c["normals"])).any(1)
    # the same cloud moved rigidly, its normals rotated, over the same lists: the same flip set
    T = synth.rigid_transform(40.0, (0.3, -1.0, 0.5), (0.7, -0.2, 1.1))
    xyz2 = (p @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    nrm2 = np.asarray(c["normals"]) @ T[:3, :3].T
    want2 = M.boruvka(xyz2, nrm2, c["nbr"], c["count"], M.centroid(xyz2))
    out2, _ = orient.orient_normals_graph(xyz2, nrm2, c["nbr"], c["count"], M.centroid(xyz2))
    flips2 = (_bits(out2) != _bits(nrm2)).any(1)
    assert np.array_equal(flips2, want2["flip"])
    assert np.array_equal(flips2, flips)


@pytest.mark.parametrize("name", ["torus", "junk", "sheets"])
def test_without_reference_the_lowest_vertex_keeps_its_sign(hip_lib, name):
    from gaussiansplattingregistration_amd import orient
    c = M.gpu_cases()[name]
    want = M.boruvka(c["xyz"], c["normals"], c["nbr"], c["count"], None)
    out, info = orient.orient_normals_graph(None, c["normals"], c["nbr"], c["count"], None)      # xyz may be missing without a reference
    flips = (_bits(out) != _bits(c["normals"])).any(1)
    assert np.array_equal(flips, want["flip"]) and np.array_equal(info["component"], want["component"])
    lowest = np.unique(info["component"])
    assert not flips[lowest].any()


@pytest.mark.parametrize("name,radius,max_nn", [("torus", 0.12, 9), ("sheets", 0.15, 7), ("junk", 0.4, 5)])
def test_search_entry_equals_graph_entry_on_the_same_lists(hip_lib, name, radius, max_nn):
    """gsr_orient_normals = gsr_hybrid_search + gsr_orient_normals_graph; the model runs on those lists too, so the tie order of a
    k-d tree never enters."""
    from gaussiansplattingregistration_amd import features, orient
    c = M.gpu_cases()[name]
    nbr, cnt = features.hybrid_search(c["xyz"], radius, max_nn)
    ref = M.centroid(c["xyz"])
    want = M.boruvka(c["xyz"], c["normals"], nbr, cnt, ref)
    a, ia = orient.orient_normals(c["xyz"], c["normals"], radius, max_nn, ref)
    b, ib = orient.orient_normals_graph(c["xyz"], c["normals"], nbr, cnt, ref)
    assert a.tobytes() == b.tobytes() and np.array_equal(ia["component"], ib["component"])
    assert {k: ia[k] for k in COUNTS} == {k: ib[k] for k in COUNTS} == {k: want[k] for k in COUNTS}
    assert np.array_equal((_bits(a) != _bits(c["normals"])).any(1), want["flip"])
    assert np.array_equal(ia["component"], want["component"])
    assert all(v >= 0.0 for v in ia["phase_ms"].values()) and ia["workspace_bytes"] > 0


def test_point_cloud_method(hip_lib):
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    c = M.gpu_cases()["torus"]
    nrm = np.array(c["normals"])
    host = PointCloud(xyz32=np.array(c["xyz"]), normals=nrm.copy())
    assert host.orient_normals_consistent_tangent_plane(8, radius=0.3) is host
    assert isinstance(host.normals, np.ndarray) and host.normals.dtype == np.float64
    s = (host.normals * c["outward"]).sum(1)
    assert (s > 0).all() or (s < 0).all()                             # what the centroid rule cannot do (test_orient_cpu.py)
    dev = PointCloud(xyz32=torch.from_numpy(np.array(c["xyz"])).cuda(), normals=torch.from_numpy(nrm.copy()).cuda())
    dev.orient_normals_consistent_tangent_plane(8, radius=0.3)
    assert torch.is_tensor(dev.normals) and dev.normals.is_cuda and dev.normals.dtype == torch.float64
    assert np.array_equal(_bits(dev.normals.cpu().numpy()), _bits(host.normals))
    explicit = PointCloud(xyz32=np.array(c["xyz"]), normals=nrm.copy()).orient_normals_consistent_tangent_plane(8, radius=0.3, reference=(0.0, 0.0, 9.0))
    free = PointCloud(xyz32=np.array(c["xyz"]), normals=nrm.copy()).orient_normals_consistent_tangent_plane(8, radius=0.3, reference=None)
    assert np.array_equal(_bits(free.normals[0]), _bits(nrm[0]))
    for other in (explicit, free):                                    # one component: the same signs or all of them turned
        same = (_bits(other.normals) == _bits(host.normals)).all(1)
        assert same.all() or not same.any()
    with pytest.raises(ValueError, match="finite radius"):
        PointCloud(xyz32=np.array(c["xyz"]), normals=nrm.copy()).orient_normals_consistent_tangent_plane(8)
    with pytest.raises(RuntimeError, match="No normals"):
        PointCloud(xyz32=np.array(c["xyz"])).orient_normals_consistent_tangent_plane(8, radius=0.3)


def test_preprocess_default_is_unchanged_and_consistent_differs_by_sign_only(hip_lib):
    import global_model as G
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.utils import global_registration_util as U
    scene = G.make_scene(20000, 1)
    v = 0.05
    make = lambda: PointCloud(xyz32=scene["xyz"].astype(np.float32), cov6=scene["cov6"].astype(np.float32))
    a, fa = U.preprocess_point_cloud(make(), v)
    b, fb = U.preprocess_point_cloud(make(), v, orient="centroid")
    assert np.array_equal(np.asarray(a.xyz32), np.asarray(b.xyz32)) and np.array_equal(_bits(a.normals), _bits(b.normals))
    assert np.array_equal(_bits(fa.rows), _bits(fb.rows))
    k, fk = U.preprocess_point_cloud(make(), v, orient="consistent")
    assert np.array_equal(np.asarray(a.xyz32), np.asarray(k.xyz32))
    same, negated = (_bits(k.normals) == _bits(a.normals)).all(1), (_bits(k.normals) == _bits(-np.asarray(a.normals))).all(1)
    assert (same | negated).all()
    assert fk.rows.shape == fa.rows.shape and k.orient_info["n"] == len(k)
    # the helper the keyword calls, on its own
    ns = PointCloud(xyz32=np.asarray(a.xyz32), normals=np.asarray(a.normals).copy())
    assert U.orient_normals_consistent(ns, 2 * v) is ns and ns.orient_info["n_components"] == k.orient_info["n_components"]
