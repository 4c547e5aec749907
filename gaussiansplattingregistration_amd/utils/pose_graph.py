"""Pose graphs for multiway registration: Open3D's ``PoseGraph`` / ``PoseGraphNode`` / ``PoseGraphEdge``,
``GlobalOptimizationOption``, ``GlobalOptimizationConvergenceCriteria`` and ``global_optimization`` on the library's host
optimiser (``gsr_posegraph_optimize``, ``csrc/gsr_posegraph.h``).  No device is involved.

Frames: a node's ``pose`` maps the node's frame into the global one; an edge's ``transformation`` maps the source node's frame
into the target node's -- what ``do_icp_registration(source, target, ...)`` returns -- so a consistent graph has
``pose[t] @ transformation == pose[s]``.  The residual of an edge is ``D = pose[t]^-1 pose[s] transformation^-1`` as
``[log_SO3(R_D); t_D]``, weighted by the edge's ``information`` (``IcpContext.information``).  Open3D composes the residual on
the other side and writes the rotation in Euler angles; the two agree to first order in the residual.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib

__all__ = ["PoseGraphNode", "PoseGraphEdge", "PoseGraph", "GlobalOptimizationOption", "GlobalOptimizationConvergenceCriteria",
           "GlobalOptimizationReport", "global_optimization", "edge_residual"]


class PoseGraphNode:
    def __init__(self, pose=None):
        self.pose = np.eye(4) if pose is None else np.array(pose, dtype=np.float64).reshape(4, 4)

    def __repr__(self):
        return "PoseGraphNode"


class PoseGraphEdge:
    def __init__(self, source_node_id=-1, target_node_id=-1, transformation=None, information=None, uncertain=False, confidence=1.0):
        self.source_node_id = int(source_node_id)
        self.target_node_id = int(target_node_id)
        self.transformation = np.eye(4) if transformation is None else np.array(transformation, dtype=np.float64).reshape(4, 4)
        self.information = np.eye(6) if information is None else np.array(information, dtype=np.float64).reshape(6, 6)
        self.uncertain = bool(uncertain)
        self.confidence = float(confidence)          # the line process value l of the last global_optimization

    def __repr__(self):
        return f"PoseGraphEdge from nodes {self.source_node_id} to {self.target_node_id}{' (uncertain)' if self.uncertain else ''}"


class PoseGraph:
    def __init__(self):
        self.nodes = []
        self.edges = []

    def __repr__(self):
        return f"PoseGraph with {len(self.nodes)} nodes and {len(self.edges)} edges."


class GlobalOptimizationOption:
    def __init__(self, max_correspondence_distance=0.075, edge_prune_threshold=0.25, preference_loop_closure=1.0, reference_node=0):
        self.max_correspondence_distance = max_correspondence_distance
        self.edge_prune_threshold = edge_prune_threshold
        self.preference_loop_closure = preference_loop_closure
        self.reference_node = reference_node


class GlobalOptimizationConvergenceCriteria:
    def __init__(self, max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6, min_right_term=1e-6,
                 min_residual=1e-6, max_iteration_lm=20):
        self.max_iteration = max_iteration
        self.min_relative_increment = min_relative_increment
        self.min_relative_residual_increment = min_relative_residual_increment
        self.min_right_term = min_right_term
        self.min_residual = min_residual
        self.max_iteration_lm = max_iteration_lm


class GlobalOptimizationReport:
    """What ``global_optimization`` did: ``line_process`` (one value per INPUT edge, 1.0 for a certain one), ``pruned`` (bool per
    input edge), and the library's result fields."""

    def __init__(self, line_process, pruned, result):
        self.line_process = line_process
        self.pruned = pruned
        self.iterations = (int(result.iterations[0]), int(result.iterations[1]))
        self.n_pruned = int(result.n_pruned)
        self.E_initial, self.E_final = float(result.E_initial), float(result.E_final)
        self.mu, self.mu_first = float(result.mu), float(result.mu_first)

    def __repr__(self):
        return (f"GlobalOptimizationReport: E {self.E_initial:.6g} -> {self.E_final:.6g}, iterations {self.iterations}, mu {self.mu:.6g}, "
                f"{self.n_pruned} edge(s) pruned")


def global_optimization(pose_graph, criteria=None, option=None):
    """Open3D's ``global_optimization(pose_graph, GlobalOptimizationLevenbergMarquardt(), criteria, option)``: optimises the node
    poses in place, drops the pruned edges from ``pose_graph.edges`` (as Open3D does) and stores each remaining edge's line process
    value in its ``confidence``.  Returns a ``GlobalOptimizationReport`` indexed by the edges as they were on entry.
    ``ValueError``: a graph the library refuses (its message says why)."""
    criteria = criteria or GlobalOptimizationConvergenceCriteria()
    option = option or GlobalOptimizationOption()
    L = _lib.load()
    n, m = len(pose_graph.nodes), len(pose_graph.edges)
    poses = np.ascontiguousarray(np.stack([np.asarray(nd.pose, dtype=np.float64).reshape(4, 4) for nd in pose_graph.nodes])) if n else np.zeros((0, 4, 4))
    edges = (_lib.PoseEdge * max(1, m))()
    for k, e in enumerate(pose_graph.edges):
        edges[k].source, edges[k].target, edges[k].uncertain = int(e.source_node_id), int(e.target_node_id), 1 if e.uncertain else 0
        edges[k].T[:] = np.asarray(e.transformation, dtype=np.float64).reshape(16).tolist()
        edges[k].information[:] = np.asarray(e.information, dtype=np.float64).reshape(36).tolist()
    o = _lib.PoseGraphOption()
    o.max_correspondence_distance = float(option.max_correspondence_distance)
    o.edge_prune_threshold = float(option.edge_prune_threshold)
    o.preference_loop_closure = float(option.preference_loop_closure)
    o.reference_node = int(option.reference_node)
    o.max_iteration, o.max_iteration_lm = int(criteria.max_iteration), int(criteria.max_iteration_lm)
    o.min_relative_increment = float(criteria.min_relative_increment)
    o.min_relative_residual_increment = float(criteria.min_relative_residual_increment)
    o.min_right_term, o.min_residual = float(criteria.min_right_term), float(criteria.min_residual)
    lp = np.ones(max(1, m), np.float64)
    pr = np.zeros(max(1, m), np.int32)
    res = _lib.PoseGraphResult()
    rc = L.gsr_posegraph_optimize(n, poses.ctypes.data, m, C.cast(edges, C.c_void_p), C.cast(C.pointer(o), C.c_void_p), lp.ctypes.data, pr.ctypes.data,
                                  C.cast(C.pointer(res), C.c_void_p))
    if rc != _lib.GSR_OK:
        msg = L.gsr_last_error()
        raise ValueError(f"global_optimization failed ({rc}): {msg.decode('utf-8', 'replace') if msg else ''}")
    for nd, P in zip(pose_graph.nodes, poses):
        nd.pose = P.copy()
    lp, pr = lp[:m], pr[:m].astype(bool)
    kept = []
    for e, l, gone in zip(pose_graph.edges, lp, pr):
        e.confidence = float(l)
        if not gone:
            kept.append(e)
    pose_graph.edges[:] = kept
    return GlobalOptimizationReport(lp, pr, res)


def _so3_log(R):
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(v), min(1.0, max(-1.0, 0.5 * (np.trace(R) - 1.0)))
    th = np.arctan2(s, c)
    return v * (1.0 + th * th / 6.0) if th < 1e-6 else v * (th / s)


def edge_residual(pose_source, pose_target, transformation):
    """``r = [log_SO3(R_D); t_D]`` of ``D = pose_target^-1 pose_source transformation^-1`` (6,): what an edge's information matrix
    weighs (``chi = r @ information @ r``).  For rotations well below pi."""
    D = np.linalg.inv(pose_target) @ pose_source @ np.linalg.inv(transformation)
    return np.concatenate([_so3_log(D[:3, :3]), D[:3, 3]])
