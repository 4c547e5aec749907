"""Headless multiway registration: N scenes into one frame (Open3D's multiway registration recipe:
``registration_icp`` per pair, ``get_information_matrix_from_point_clouds``, ``PoseGraph``, ``global_optimization``).

Per edge ``(s, t)``: one ``do_icp_registration(clouds[s], clouds[t], init, params)`` -- its transformation maps ``s``'s frame into
``t``'s --, then the pair's information matrix at that transformation and ``params.max_correspondence`` (``IcpContext.information``,
the ``gsr_icp_information`` kernel).  Edges with ``t == s + 1`` are certain ("odometry"), all others uncertain (loop closures under
the line process).  Node poses start from chaining the odometry edges from the reference node (a breadth-first walk over all edges
reaches what the odometry does not), then ``global_optimization`` (``utils/pose_graph.py``).  Errors are collected as strings, as in
the other workers; ``cancel()`` takes effect between edges.
"""
from __future__ import annotations

import numpy as np

from .. import icp as _icp
from ..utils.local_registration_util import do_icp_registration, get_information_matrix_from_point_clouds
from ..utils.pose_graph import (GlobalOptimizationConvergenceCriteria, GlobalOptimizationOption, PoseGraph, PoseGraphEdge, PoseGraphNode,
                                global_optimization)


def edge_list(n, edges):
    """``"sequential"`` -> (i, i + 1); ``"all"`` -> every pair s < t; or the list of (s, t) given."""
    if isinstance(edges, str):
        if edges == "sequential":
            return [(i, i + 1) for i in range(n - 1)]
        if edges == "all":
            return [(s, t) for s in range(n) for t in range(s + 1, n)]
        raise ValueError(f"edges: 'sequential', 'all' or a list of (source, target), not {edges!r}")
    out = [(int(s), int(t)) for s, t in edges]
    for s, t in out:
        if not (0 <= s < n and 0 <= t < n) or s == t:
            raise ValueError(f"edge ({s}, {t}) of {n} clouds")
    return out


def initial_poses(n, edges, reference_node=0):
    """Node poses from the edges ``[(s, t, T, uncertain), ...]``: the certain edges are chained from the reference node
    (``X_s = X_t T``, ``X_t = X_s T^-1``), then a breadth-first walk over all edges places what they did not reach.  A node no edge
    path reaches keeps the identity (``global_optimization`` refuses such a graph)."""
    poses = [None] * n
    poses[reference_node] = np.eye(4)
    for only_certain in (True, False):
        queue = [i for i in range(n) if poses[i] is not None]
        while queue:
            k = queue.pop(0)
            for s, t, T, uncertain in edges:
                if only_certain and uncertain:
                    continue
                if s == k and poses[t] is None:
                    poses[t] = poses[s] @ np.linalg.inv(T)
                    queue.append(t)
                elif t == k and poses[s] is None:
                    poses[s] = poses[t] @ T
                    queue.append(s)
    return [np.eye(4) if X is None else X for X in poses]


class MultiwayRegistrator:
    class ResultData:
        def __init__(self, poses, pose_graph, edge_reports, optimization):
            self.poses = poses                      # list of 4x4: cloud i's frame -> the reference node's
            self.pose_graph = pose_graph            # the optimised graph (pruned edges dropped)
            self.edge_reports = edge_reports        # one dict per requested edge
            self.optimization = optimization        # GlobalOptimizationReport

    def __init__(self, clouds, params, edges="sequential", init=None, option=None, criteria=None, progress=None, fuse=None, match_colors=None,
                 match_colors_gate=None):
        """``clouds``: the ``PointCloud`` records; ``params``: ``LocalRegistrationParams`` of every pairwise ICP; ``init``: ``None``
        (identity), ``{(s, t): T}`` (missing pairs: identity) or ``callable(s, t, cloud_s, cloud_t) -> T`` (e.g. a global
        registration); ``option`` (``GlobalOptimizationOption``): default ``max_correspondence_distance = params.max_correspondence``;
        ``fuse`` (``FuseOverlapParams`` or ``None``): what ``merge`` hands to ``get_merged_gaussian_point_clouds_multi``;
        ``match_colors`` (``ColorMatchParams`` or ``None``) and ``match_colors_gate`` (``FuseOverlapParams``, needed without ``fuse``)
        likewise: ``merge`` harmonises the colours of the scenes between the move and the concatenation or fusion."""
        self.clouds, self.params = list(clouds), params
        self.edges = edge_list(len(self.clouds), edges)
        self.init = init
        self.option = option or GlobalOptimizationOption(max_correspondence_distance=params.max_correspondence)
        self.criteria = criteria or GlobalOptimizationConvergenceCriteria()
        self.errors = []
        self.signal_cancel = False
        self._progress = progress
        self.timing = {}
        self.fuse = fuse                    # FuseOverlapParams or None: the merge stores a surface that k scenes share once
        self.fuse_info = None               # the report of the last merge with `fuse`
        self.match_colors, self.match_colors_gate = match_colors, match_colors_gate
        self.color_info = None              # (transforms, info) of the last merge with `match_colors`

    def merge(self, models, result, rotate_sh=False):
        """The ``GaussianModel`` s of the clouds, each moved by its pose of ``result`` (what ``run`` returned), in one model:
        concatenated, or -- with ``fuse`` -- with the overlaps fused (``GaussianModel.fuse_overlap_multi``; the report goes to
        ``fuse_info``)."""
        from ..models.gaussian_model import GaussianModel
        if self.match_colors is not None:
            gate = self.fuse if self.fuse is not None else self.match_colors_gate
            moved, self.color_info = GaussianModel.move_and_match_colors_multi(models, result.poses, rotate_sh, self.match_colors, gate,
                                                                                         reference=self.option.reference_node)
            if self.fuse is None:
                return GaussianModel.get_merged_gaussian_point_clouds_multi(moved, [np.eye(4)] * len(moved))
            merged, self.fuse_info = GaussianModel.fuse_overlap_multi(moved, self.fuse)
            return merged
        if self.fuse is None:
            return GaussianModel.get_merged_gaussian_point_clouds_multi(models, result.poses, rotate_sh=rotate_sh)
        merged, self.fuse_info = GaussianModel.get_merged_gaussian_point_clouds_fused_multi(models, result.poses, self.fuse, rotate_sh=rotate_sh)
        return merged

    def cancel(self):
        self.signal_cancel = True

    def _init_for(self, s, t):
        if self.init is None:
            return np.eye(4)
        if callable(self.init):
            return np.asarray(self.init(s, t, self.clouds[s], self.clouds[t]), dtype=np.float64).reshape(4, 4)
        return np.asarray(self.init.get((s, t), np.eye(4)), dtype=np.float64).reshape(4, 4)

    def run(self):
        import time
        graph, reports = PoseGraph(), []
        t_icp = t_info = 0.0
        ctx = None
        try:
            for k, (s, t) in enumerate(self.edges):
                if self.signal_cancel:
                    return None
                src, tgt = self.clouds[s], self.clouds[t]
                t0 = time.perf_counter()
                try:
                    T0 = self._init_for(s, t)
                    res = do_icp_registration(src, tgt, T0, self.params)
                    t1 = time.perf_counter()
                    if ctx is None:
                        ctx = _icp.IcpContext(device=getattr(tgt, "device_index", 0))
                    info = get_information_matrix_from_point_clouds(src, tgt, self.params.max_correspondence, res.transformation, ctx=ctx)
                except RuntimeError as e:
                    self.errors.append(f"{e}\nSource: \"{src}\" (cloud {s})\nTarget: \"{tgt}\" (cloud {t})")
                    return None
                t_icp += t1 - t0
                t_info += time.perf_counter() - t1
                uncertain = t != s + 1
                graph.edges.append(PoseGraphEdge(s, t, res.transformation, info, uncertain))
                reports.append({"source": s, "target": t, "uncertain": uncertain, "initial_transformation": T0, "transformation": res.transformation,
                                "fitness": res.fitness, "inlier_rmse": res.inlier_rmse, "iterations": getattr(res, "iterations", 0),
                                "n_correspondences": int(info[5, 5]), "information": info})
                if self._progress:
                    self._progress(int((k + 1) / (len(self.edges) + 1) * 100))
        finally:
            if ctx is not None:
                ctx.close()
        if self.signal_cancel:
            return None
        t2 = time.perf_counter()
        start = initial_poses(len(self.clouds), [(e.source_node_id, e.target_node_id, e.transformation, e.uncertain) for e in graph.edges],
                              self.option.reference_node)
        graph.nodes = [PoseGraphNode(X) for X in start]
        try:
            opt = global_optimization(graph, self.criteria, self.option)
        except ValueError as e:
            self.errors.append(str(e))
            return None
        for r, l, gone in zip(reports, opt.line_process, opt.pruned):
            r["line_process"], r["pruned"] = float(l), bool(gone)
        self.timing = {"pairwise_s": t_icp, "information_s": t_info, "optimization_s": time.perf_counter() - t2}
        if self._progress:
            self._progress(100)
        return MultiwayRegistrator.ResultData([n.pose for n in graph.nodes], graph, reports, opt)
