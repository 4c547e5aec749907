"""The pose-graph optimiser (gsr_posegraph_optimize: host code, no device) against tests/posegraph_model.py, the independent
NumPy / SciPy model of the contract (Open3D is absent: parity with its global_optimization is unpinned).

The graph of the noisy cases: 6 nodes, scene scale 2, five odometry edges with 1e-3 noise, four loop closures with 2e-4 noise, one
false loop closure about 30 degrees / 0.6 units off, 2000 correspondences per edge, max_correspondence_distance 0.05 (mu = 5).
"""
import ctypes as C

import numpy as np
import pytest

import posegraph_model as M
from gaussiansplattingregistration_amd import _lib
from gaussiansplattingregistration_amd.utils import pose_graph as PG

D = 0.05
TIGHT = dict(max_iteration=1000, min_relative_increment=1e-12, min_relative_residual_increment=1e-12, min_right_term=0.0, min_residual=0.0)


def _graph(poses, edges, certain=False):
    g = PG.PoseGraph()
    g.nodes = [PG.PoseGraphNode(X) for X in poses]
    g.edges = [PG.PoseGraphEdge(e.s, e.t, e.T, e.info, e.uncertain and not certain) for e in edges]
    return g


def _poses(g):
    return [n.pose for n in g.nodes]


def _option(**kw):
    return PG.GlobalOptimizationOption(max_correspondence_distance=D, **kw)


@pytest.fixture(scope="module")
def noisy():
    """the graph without the false edge, the model's two solutions of it and their spread"""
    gt, edges, _ = M.make_graph(seed=0, false_edge=False)
    start = M.chain_odometry(len(gt), edges)
    a = M.global_optimization(start, edges, D, method="trf")
    b = M.global_optimization(start, edges, D, method="lm")
    spread = max(np.linalg.norm(x - y) for x, y in zip(a["poses"], b["poses"]))
    return {"gt": gt, "edges": edges, "start": start, "model": a, "spread": spread}


@pytest.fixture(scope="module")
def false_edge():
    gt, edges, k = M.make_graph(seed=0, false_edge=True)
    start = M.chain_odometry(len(gt), edges)
    a = M.global_optimization(start, edges, D, method="trf")
    b = M.global_optimization(start, edges, D, method="lm")
    spread = max(np.linalg.norm(x - y) for x, y in zip(a["poses"], b["poses"]))
    return {"gt": gt, "edges": edges, "start": start, "model": a, "spread": spread, "k": k}


def test_consistent_graph(hip_lib):
    """Exact edges, a start 0.05 rad / 0.05 units off: every pose returns to ground truth within 1e-8 (Frobenius).  E = 0 at the
    solution, so Gauss-Newton converges quadratically; the default thresholds (1e-6 on E itself) would stop it at ~1e-5, so the
    test asks for the tight ones."""
    gt, edges, _ = M.make_graph(seed=1, false_edge=False, exact=True)
    rng = np.random.default_rng(5)
    start = [gt[0]] + [M.pose(rng.normal(size=3) * 0.03, rng.normal(size=3) * 0.03) @ X for X in gt[1:]]
    g = _graph(start, edges)
    rep = PG.global_optimization(g, PG.GlobalOptimizationConvergenceCriteria(**TIGHT), _option())
    err = M.pose_error(_poses(g), gt)
    print(f"start error {M.pose_error(start, gt):.3e}, final {err:.3e}, E {rep.E_initial:.3e} -> {rep.E_final:.3e}, iterations {rep.iterations}")
    assert M.pose_error(start, gt) > 0.03
    assert err <= 1e-8
    assert rep.E_final <= 1e-12 * rep.E_initial
    assert rep.iterations[0] <= 12                      # quadratic: 0.05 -> 1e-8 takes a handful of steps, not hundreds
    assert rep.n_pruned == 0 and len(g.edges) == len(edges)


def test_noisy_graph(hip_lib, noisy):
    g = _graph(noisy["start"], noisy["edges"])
    rep = PG.global_optimization(g, PG.GlobalOptimizationConvergenceCriteria(**TIGHT), _option())
    E_model = noisy["model"]["E"]
    diff = max(np.linalg.norm(a - b) for a, b in zip(_poses(g), noisy["model"]["poses"]))
    e_chain, e_opt = M.pose_error(noisy["start"], noisy["gt"]), M.pose_error(_poses(g), noisy["gt"])
    print(f"E library {rep.E_final!r} model {E_model!r}; poses differ by {diff:.3e}, model's solvers by {noisy['spread']:.3e}; "
          f"error chained {e_chain:.3e} optimised {e_opt:.3e}; iterations {rep.iterations}")
    assert rep.E_final <= E_model * (1 + 1e-9)
    assert abs(M.objective(_poses(g), noisy["edges"], rep.mu) - rep.E_final) <= 1e-9 * rep.E_final      # E is the contract's E
    assert diff <= 100 * noisy["spread"]
    assert e_opt < e_chain
    assert rep.n_pruned == 0 and (rep.line_process >= 0.9).all()


def test_false_edge(hip_lib, false_edge):
    f = false_edge
    g = _graph(f["start"], f["edges"])
    rep = PG.global_optimization(g, PG.GlobalOptimizationConvergenceCriteria(**TIGHT), _option())
    want = np.zeros(len(f["edges"]), bool)
    want[f["k"]] = True
    diff = max(np.linalg.norm(a - b) for a, b in zip(_poses(g), f["model"]["poses"]))
    e_opt = M.pose_error(_poses(g), f["gt"])
    print(f"line process {np.round(rep.line_process, 5)}; poses differ from the model by {diff:.3e} (its solvers: {f['spread']:.3e}); error {e_opt:.3e}")
    assert (rep.pruned == want).all() and (f["model"]["pruned"] == want).all()
    loops = np.array([e.uncertain for e in f["edges"]]) & ~want
    assert (rep.line_process[loops] >= 0.9).all()
    assert rep.line_process[f["k"]] < 0.25
    assert len(g.edges) == len(f["edges"]) - 1 and all((e.source_node_id, e.target_node_id) != (1, 3) for e in g.edges)
    assert rep.E_final <= f["model"]["E"] * (1 + 1e-9)
    assert diff <= 100 * f["spread"]
    # the same graph with every edge certain: the false edge drags the poses away -- the line process is what saved them
    gc = _graph(f["start"], f["edges"], certain=True)
    PG.global_optimization(gc, PG.GlobalOptimizationConvergenceCriteria(**TIGHT), _option())
    e_certain = M.pose_error(_poses(gc), f["gt"])
    print(f"all edges certain: error {e_certain:.3e}")
    assert e_certain > 10 * e_opt


def test_mu_and_line_process(hip_lib, noisy, false_edge):
    for case in (noisy, false_edge):
        g = _graph(case["start"], case["edges"])
        rep = PG.global_optimization(g, None, _option(preference_loop_closure=0.7))
        assert rep.mu_first == pytest.approx(M.mu_of(case["edges"], D, 0.7), rel=1e-14)
        rest = [e for e, gone in zip(case["edges"], rep.pruned) if not gone]
        assert rep.mu == pytest.approx(M.mu_of(rest, D, 0.7), rel=1e-14)
        l = M.line_process(_poses(g), rest, rep.mu)
        assert np.abs(rep.line_process[~rep.pruned] - l).max() <= 1e-12
        assert [e.confidence for e in g.edges] == list(rep.line_process[~rep.pruned])


def test_first_order_property():
    """chi = r^T Lambda r is, to first order in D, the sum over the correspondences of |D q - q|^2"""
    rng = np.random.default_rng(3)
    q = (rng.random((500, 3)) - 0.5) * 2.0 + np.array([0.3, -0.2, 0.5])
    L = M.information_from_points(q)
    Xs, Xt = M.pose([0.2, -0.1, 0.4], [0.5, 0.1, -0.3]), M.pose([-0.3, 0.2, 0.1], [0.0, 0.4, 0.2])
    Dm = M.pose(rng.normal(size=3) * 1e-4, rng.normal(size=3) * 1e-4)
    T = M.inv(Dm) @ M.inv(Xt) @ Xs                       # D = X_t^-1 X_s T^-1 = Dm
    r = PG.edge_residual(Xs, Xt, T)
    chi = float(r @ L @ r)
    direct = float((((q @ Dm[:3, :3].T + Dm[:3, 3]) - q) ** 2).sum())
    print(f"chi {chi!r} direct {direct!r}")
    assert abs(chi - direct) <= 1e-3 * direct


@pytest.mark.parametrize("k", [0, 2, 5])
def test_gauge(hip_lib, noisy, k):
    start = [X.copy() for X in noisy["start"]]
    start[k] = M.pose([0.1, 0.2, -0.3], [0.7, -0.1, 0.2]) @ start[k]          # not where the other poses want it
    g = _graph(start, noisy["edges"])
    PG.global_optimization(g, None, _option(reference_node=k))
    assert g.nodes[k].pose.tobytes() == start[k].tobytes()
    assert any(not np.array_equal(g.nodes[i].pose, start[i]) for i in range(len(start)) if i != k)


def _raw(n_nodes, poses, edges, option=None):
    arr = (_lib.PoseEdge * max(1, len(edges)))()
    for i, (s, t, T, info, u) in enumerate(edges):
        arr[i].source, arr[i].target, arr[i].uncertain = s, t, u
        arr[i].T[:] = np.asarray(T, np.float64).reshape(16).tolist()
        arr[i].information[:] = np.asarray(info, np.float64).reshape(36).tolist()
    P = np.ascontiguousarray(poses, dtype=np.float64)
    L = _lib.load()
    rc = L.gsr_posegraph_optimize(n_nodes, P.ctypes.data, len(edges), C.cast(arr, C.c_void_p), C.cast(C.pointer(option), C.c_void_p) if option else None,
                                  None, None, None)
    return rc, L.gsr_last_error().decode()


def _default_option():
    o = _lib.PoseGraphOption()
    o.max_correspondence_distance, o.edge_prune_threshold, o.preference_loop_closure = 0.075, 0.25, 1.0
    o.reference_node, o.max_iteration, o.max_iteration_lm = 0, 100, 20
    o.min_relative_increment = o.min_relative_residual_increment = o.min_right_term = o.min_residual = 1e-6
    return o


def test_errors(hip_lib):
    I4, I6 = np.eye(4), np.eye(6) * 10
    three = np.stack([I4] * 3)
    ok = [(0, 1, I4, I6, 0), (1, 2, I4, I6, 0)]
    assert _raw(3, three, ok)[0] == 0
    assert _raw(3, three, ok, _default_option())[0] == 0
    asym = I6.copy()
    asym[0, 1] = 1.0
    indefinite = I6.copy()
    indefinite[0, 1] = indefinite[1, 0] = 20.0
    nan_pose = three.copy()
    nan_pose[2, 0, 3] = np.nan
    nan_T = I4.copy()
    nan_T[1, 1] = np.inf
    bad_threshold = _default_option()
    bad_threshold.edge_prune_threshold = -0.1
    bad_ref = _default_option()
    bad_ref.reference_node = 3
    cases = {
        "unreachable node": (3, three, [(0, 1, I4, I6, 0)], None, "cannot be reached"),
        "index out of range": (3, three, [(0, 1, I4, I6, 0), (1, 3, I4, I6, 0)], None, "out of range"),
        "negative index": (3, three, [(0, 1, I4, I6, 0), (-1, 2, I4, I6, 0)], None, "out of range"),
        "s == t": (3, three, ok + [(2, 2, I4, I6, 1)], None, "source == target"),
        "NaN pose": (3, nan_pose, ok, None, "not finite"),
        "inf transform": (3, three, [(0, 1, nan_T, I6, 0), (1, 2, I4, I6, 0)], None, "not finite"),
        "asymmetric information": (3, three, [(0, 1, I4, asym, 0), (1, 2, I4, I6, 0)], None, "not symmetric"),
        "indefinite information": (3, three, [(0, 1, I4, indefinite, 0), (1, 2, I4, I6, 0)], None, "semi-definite"),
        "negative threshold": (3, three, ok, bad_threshold, "edge_prune_threshold"),
        "reference out of range": (3, three, ok, bad_ref, "reference_node"),
    }
    for name, (n, poses, edges, opt, word) in cases.items():
        rc, msg = _raw(n, poses, edges, opt)
        assert rc == _lib.GSR_E_INVALID, name
        assert "gsr_posegraph_optimize" in msg and word in msg, (name, msg)
    # and from Python
    g = PG.PoseGraph()
    g.nodes = [PG.PoseGraphNode() for _ in range(3)]
    g.edges = [PG.PoseGraphEdge(0, 1, I4, I6)]
    with pytest.raises((RuntimeError, ValueError), match="cannot be reached"):
        PG.global_optimization(g)
    g.edges.append(PG.PoseGraphEdge(1, 2, I4, asym))
    with pytest.raises((RuntimeError, ValueError), match="not symmetric"):
        PG.global_optimization(g)
    g.edges[1].information = I6
    with pytest.raises((RuntimeError, ValueError), match="edge_prune_threshold"):
        PG.global_optimization(g, None, PG.GlobalOptimizationOption(edge_prune_threshold=-1.0))
    # a zero information matrix (a pair without correspondences) is semi-definite: accepted
    g.edges[1].information = np.zeros((6, 6))
    PG.global_optimization(g)


def test_information_symbol_is_bound(hip_lib):
    """gsr_icp_information needs a context, and without a device none can be created (tests/test_abi.py): here only that the
    symbol is exported and bound, and that the Python surface exists."""
    from gaussiansplattingregistration_amd import icp
    from gaussiansplattingregistration_amd.utils import local_registration_util as U
    assert "gsr_icp_information" in _lib.SIGNATURES and hasattr(hip_lib, "gsr_icp_information")
    assert hip_lib.gsr_icp_information(None, None, None, None) == _lib.GSR_E_INVALID
    assert b"gsr_icp_information" in hip_lib.gsr_last_error()
    assert callable(icp.IcpContext.information) and callable(U.get_information_matrix_from_point_clouds)
