"""Global registration: the reference's ``src/utils/global_registration_util.py`` on the GPU (``features.py``,
``csrc/features.hip``, ``csrc/fgr.hip``, ``csrc/sc2.hip``), with Open3D-named shims for what it reaches through open3d==0.16.0.

``preprocess_point_cloud`` follows the project's conventions: ``PointCloud.voxel_down_sample`` then ``estimate_normals()`` (the
averaged covariances of a splat cloud, KNN-30 without covariances -- so the reference's normal radius ``2 * voxel`` is inert, as
for the voxel multiscale path), then every normal is turned towards the cloud's centroid, then FPFH at (5 * voxel, 100).  The
orientation is a deviation from the reference, whose normals keep the eigen-solver's arbitrary sign: FPFH is not invariant under a
normal's sign, and with arbitrary signs only ~7 % of the mutual feature matches of the project's test scene are right (57 % oriented,
DESIGN.md section 12).  The centroid moves with the cloud, so the orientation is the same for a cloud and its rigidly moved copy.
``orient="consistent"`` propagates the signs along the neighbour graph instead (``orient_normals_consistent``).
Both methods of the reference's tab are here: ``do_ransac_registration`` and ``do_fgr_registration`` (Fast Global Registration;
its tuple test draws with the library's counter-based sampler, so it is deterministic for a given ``seed``).  A third method, which the
reference does not have, stands beside them: ``do_sc2_registration``, the compatibility-graph method of ``csrc/sc2.hip`` (DESIGN.md
section 33) -- rigid, deterministic, without sampling.
"""
from __future__ import annotations

from enum import Enum

import numpy as np

from .. import features as _F
from .. import icp as _icp

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


class GlobalRegistrationType(Enum):
    def __new__(cls, *args, **kwds):
        value = len(cls.__members__)
        obj = object.__new__(cls)
        obj._value_ = value
        return obj

    def __init__(self, name):
        self.instance_name = name

    RANSAC = "RANSAC"
    FGR = "FGR"
    SC2 = "SC2"              # the compatibility-graph method (not in the reference): appended, so the two above keep their values


class RANSACEstimationMethod(Enum):
    def __new__(cls, *args, **kwds):
        value = len(cls.__members__)
        obj = object.__new__(cls)
        obj._value_ = value
        return obj

    def __init__(self, name):
        self.instance_name = name

    TransformationEstimationPointToPoint = "Point-To-Point"
    TransformationEstimationPointToPlane = "Point-To-Plane"
    TransformationEstimationForGeneralizedICP = "For GICP"
    TransformationEstimationForColoredICP = "For CICP"


class TransformationEstimationPointToPoint:
    """``with_scaling=True``: Umeyama with scaling, the hypotheses are similarities ``[c R | t]``.  The edge-length checker compares
    lengths of the two clouds as they are (Open3D's behaviour, kept): leave it out when the clouds' relative scale is unknown."""

    kind = _F.KIND_POINT_TO_POINT

    def __init__(self, with_scaling=False):
        self.with_scaling = bool(with_scaling)
        self.kind = _F.KIND_POINT_TO_POINT_SCALED if self.with_scaling else _F.KIND_POINT_TO_POINT


class TransformationEstimationPointToPlane:
    kind = _F.KIND_POINT_TO_PLANE


class _Unsupported:
    kind = -1

    def __init__(self, name):
        self.name = name


def get_estimation_method_from_enum(estimation_method):
    """The estimator of each enum value.  GICP / CICP are not valid RANSAC estimators (the reference even swaps the two,
    ``global_registration_util.py:44-47``); they give an object that ``registration_ransac_*`` rejects with RuntimeError."""
    if estimation_method == RANSACEstimationMethod.TransformationEstimationPointToPoint:
        return TransformationEstimationPointToPoint()
    if estimation_method == RANSACEstimationMethod.TransformationEstimationPointToPlane:
        return TransformationEstimationPointToPlane()
    if estimation_method == RANSACEstimationMethod.TransformationEstimationForGeneralizedICP:
        return _Unsupported("TransformationEstimationForGeneralizedICP")
    if estimation_method == RANSACEstimationMethod.TransformationEstimationForColoredICP:
        return _Unsupported("TransformationEstimationForColoredICP")
    raise ValueError(f"unknown estimation method {estimation_method!r}")


class Feature:
    """``o3d.pipelines.registration.Feature``: ``data`` is (33, n) like Open3D's; ``rows`` the (n, 33) array the library wrote."""

    def __init__(self, rows):
        self.rows = rows

    @property
    def data(self):
        return self.rows.T

    def dimension(self):
        return int(self.rows.shape[1])

    def num(self):
        return int(self.rows.shape[0])


class KDTreeSearchParamHybrid:
    def __init__(self, radius, max_nn):
        self.radius, self.max_nn = float(radius), int(max_nn)


class RANSACConvergenceCriteria:
    def __init__(self, max_iteration=100000, confidence=0.999):
        self.max_iteration, self.confidence = int(max_iteration), float(confidence)


class CorrespondenceCheckerBasedOnEdgeLength:
    code = _F.CHECK_EDGE_LENGTH

    def __init__(self, similarity_threshold=0.9):
        self.similarity_threshold = float(similarity_threshold)

    @property
    def param(self):
        return self.similarity_threshold


class CorrespondenceCheckerBasedOnDistance:
    code = _F.CHECK_DISTANCE

    def __init__(self, distance_threshold):
        self.distance_threshold = float(distance_threshold)

    @property
    def param(self):
        return self.distance_threshold


class CorrespondenceCheckerBasedOnNormal:
    code = _F.CHECK_NORMAL

    def __init__(self, normal_angle_threshold):
        self.normal_angle_threshold = float(normal_angle_threshold)

    @property
    def param(self):
        return self.normal_angle_threshold


class RegistrationResult:
    def __init__(self, transformation=None, fitness=0.0, inlier_rmse=0.0, correspondence_set=None, info=None):
        self.transformation = np.eye(4) if transformation is None else np.asarray(transformation, dtype=np.float64)
        self.fitness, self.inlier_rmse = float(fitness), float(inlier_rmse)
        self.correspondence_set = correspondence_set if correspondence_set is not None else np.zeros((0, 2), np.int32)
        self.info = info or {}

    def __repr__(self):
        return f"RegistrationResult with fitness={self.fitness:e}, inlier_rmse={self.inlier_rmse:e}"


def compute_fpfh_feature(pcd, search_param):
    """``o3d.pipelines.registration.compute_fpfh_feature`` on a ``PointCloud`` record with normals."""
    if not pcd.has_normals():
        raise RuntimeError("[Open3D Error] Failed because input point cloud has no normal.")
    return Feature(_F.fpfh(pcd.xyz32, pcd.normals, search_param.radius, search_param.max_nn, device=pcd.device_index))


def _estimation_kind(estimation_method):
    kind = getattr(estimation_method, "kind", -1)
    if kind not in (_F.KIND_POINT_TO_POINT, _F.KIND_POINT_TO_PLANE, _F.KIND_POINT_TO_POINT_SCALED):
        raise RuntimeError(f"{getattr(estimation_method, 'name', estimation_method)} is not a RANSAC estimation method of this backend "
                           "(point-to-point or point-to-plane)")
    return kind


def _checker_list(checkers):
    return [(c.code, c.param) for c in (checkers or [])]


def registration_ransac_based_on_correspondence(source, target, corres, max_correspondence_distance, estimation_method=None,
                                                ransac_n=3, checkers=None, criteria=None, seed=0, batch=8192):
    """``o3d.pipelines.registration.registration_ransac_based_on_correspondence``, deterministic for a given ``seed``."""
    estimation_method = estimation_method or TransformationEstimationPointToPoint()
    kind = _estimation_kind(estimation_method)
    criteria = criteria or RANSACConvergenceCriteria()
    if kind == _F.KIND_POINT_TO_PLANE and not target.has_normals():
        raise RuntimeError("[Open3D Error] TransformationEstimationPointToPlane requires pre-computed normal vectors for target PointCloud.")
    nrm = source.has_normals() and target.has_normals()
    r = _F.ransac_correspondence(source.xyz32, target.xyz32, corres, max_correspondence_distance, kind=kind, ransac_n=ransac_n,
                                 checkers=_checker_list(checkers), max_iteration=criteria.max_iteration, confidence=criteria.confidence,
                                 seed=seed, batch=batch, src_normals=source.normals if nrm else None,
                                 tgt_normals=target.normals if (nrm or kind == _F.KIND_POINT_TO_PLANE) else None,
                                 device=source.device_index)
    info = {k: r[k] for k in ("best_index", "n_evaluated", "n_valid", "exit_index")}
    return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], info=info)


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, mutual_filter,
                                                  max_correspondence_distance, estimation_method=None, ransac_n=3, checkers=None,
                                                  criteria=None, seed=0, batch=8192):
    """``o3d.pipelines.registration.registration_ransac_based_on_feature_matching`` (Open3D 0.16): exact feature 1-NN,
    optional mutual filter (falls back to the one-way set below 3 * ransac_n pairs), then RANSAC over the correspondences."""
    _estimation_kind(estimation_method or TransformationEstimationPointToPoint())
    if ransac_n < 3 or not (max_correspondence_distance > 0.0):
        return RegistrationResult()
    corres, used_mutual = _F.feature_match(source_feature.rows, target_feature.rows, mutual=bool(mutual_filter), ransac_n=ransac_n,
                                           device=source.device_index)
    res = registration_ransac_based_on_correspondence(source, target, corres, max_correspondence_distance, estimation_method, ransac_n,
                                                      checkers, criteria, seed=seed, batch=batch)
    res.info["used_mutual"] = used_mutual
    res.info["n_corres"] = int(corres.shape[0])
    return res


def orient_normals_towards_centroid(pcd):
    """Flip every normal n of ``pcd`` with n . (centroid - p) < 0 (Open3D's orient_normals_towards_camera_location with the camera at
    the cloud's centroid).  Keeps the normals' placement."""
    x, nrm = pcd.xyz32, pcd.normals
    if torch is not None and isinstance(nrm, torch.Tensor):
        p = x.detach().double() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, np.float64), device=nrm.device)
        c = p.mean(0)
        flip = ((c[None] - p) * nrm).sum(1) < 0
        pcd.normals = torch.where(flip[:, None], -nrm, nrm)
    else:
        p = np.asarray(pcd.points, np.float64)
        c = p.mean(0)
        nrm = np.asarray(nrm, np.float64)
        flip = ((c[None] - p) * nrm).sum(1) < 0
        pcd.normals = np.where(flip[:, None], -nrm, nrm)
    return pcd


def orient_normals_consistent(pcd, radius, max_nn=30):
    """Propagate the normals' signs along the minimum spanning forest of the hybrid ``(radius, max_nn)`` neighbour graph and let
    every connected piece look towards the cloud's centroid by majority (``orient.orient_normals``).  Right
    for shapes the centroid rule splits (a torus, the far side of a wall, two objects); a single point still follows the centroid
    rule.  Keeps the normals' placement."""
    if not pcd.has_normals():
        raise RuntimeError("[Open3D Error] No normals in the PointCloud. Call estimate_normals() first.")
    return pcd.orient_normals_consistent_tangent_plane(int(max_nn) - 1, radius=radius, reference="centroid")


ORIENT_MODES = ("centroid", "consistent")


def preprocess_point_cloud(pcd, voxel_size, orient="centroid"):
    """``orient``: ``"centroid"`` (the default: every normal towards the cloud's centroid) or ``"consistent"`` (the centroid-voted
    propagation over the hybrid lists of ``radius = 2 * voxel_size, max_nn = 30``)."""
    if orient not in ORIENT_MODES:
        raise ValueError(f"orient must be one of {ORIENT_MODES} (got {orient!r})")
    pcd_down = pcd.voxel_down_sample(voxel_size)
    pcd_down.estimate_normals()
    if orient == "consistent":
        orient_normals_consistent(pcd_down, radius=2 * voxel_size, max_nn=30)
    else:
        orient_normals_towards_centroid(pcd_down)
    radius_feature = voxel_size * 5
    pcd_fpfh = compute_fpfh_feature(pcd_down, KDTreeSearchParamHybrid(radius=radius_feature, max_nn=100))
    return pcd_down, pcd_fpfh


def do_ransac_registration(point_cloud_first, point_cloud_second, params):
    source_down, source_fpfh = preprocess_point_cloud(point_cloud_first, params.voxel_size, orient=getattr(params, "orient_normals", "centroid"))
    target_down, target_fpfh = preprocess_point_cloud(point_cloud_second, params.voxel_size, orient=getattr(params, "orient_normals", "centroid"))
    real_estimation_method = get_estimation_method_from_enum(params.estimation_method)
    result = registration_ransac_based_on_feature_matching(
        source_down, target_down, source_fpfh, target_fpfh, params.mutual_filter,
        params.max_correspondence,
        real_estimation_method,
        params.ransac_n,
        params.checkers,
        RANSACConvergenceCriteria(params.max_iteration, params.confidence),
        seed=getattr(params, "seed", 0))
    return result


class FastGlobalRegistrationOption:
    """``o3d.pipelines.registration.FastGlobalRegistrationOption`` (Open3D 0.16): its eight fields in its positional order, plus the
    keywords ``seed`` (of the tuple test's counter-based draws) and ``batch`` (trials per device batch, a speed knob only)."""

    def __init__(self, division_factor=1.4, use_absolute_scale=False, decrease_mu=False, maximum_correspondence_distance=0.025,
                 iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000, tuple_test=True, *, seed=0, batch=0):
        self.division_factor, self.use_absolute_scale, self.decrease_mu = float(division_factor), bool(use_absolute_scale), bool(decrease_mu)
        self.maximum_correspondence_distance, self.iteration_number = float(maximum_correspondence_distance), int(iteration_number)
        self.tuple_scale, self.maximum_tuple_count, self.tuple_test = float(tuple_scale), int(maximum_tuple_count), bool(tuple_test)
        self.seed, self.batch = int(seed), int(batch)


def evaluate_registration(source, target, max_correspondence_distance, transformation):
    """``o3d.pipelines.registration.evaluate_registration``: the nearest target point of every transformed source point through the
    ICP context's search; a pair is an inlier iff its squared distance is below ``max_correspondence_distance ** 2`` (the ICP's
    rule).  ``fitness = inliers / |source|``, ``inlier_rmse``, ``correspondence_set`` (source row, target row) in source order."""
    T = np.asarray(transformation, np.float64).reshape(4, 4)
    ns = int(source.xyz32.shape[0])
    if ns == 0 or int(target.xyz32.shape[0]) == 0 or not (max_correspondence_distance > 0.0):
        return RegistrationResult(T)
    with _icp.IcpContext(device=source.device_index) as c:
        c.set_target(target.xyz32, None, max_correspondence_distance)
        c.set_source(source.xyz32)
        idx, d2 = c.correspondences(T)
    inl = idx >= 0
    good = int(inl.sum())
    rmse = float(np.sqrt(d2[inl].sum() / good)) if good else 0.0
    cs = np.stack([np.flatnonzero(inl), idx[inl]], axis=1).astype(np.int32)
    return RegistrationResult(T, good / ns, rmse, cs)


def registration_fgr_based_on_correspondence(source, target, corres, option=None):
    """Fast Global Registration over given correspondences ``(m, 2)`` (source row, target row): the tuple test (when
    ``option.tuple_test``), the optimisation, then ``evaluate_registration`` at ``option.maximum_correspondence_distance``."""
    o = option or FastGlobalRegistrationOption()
    dev = source.device_index
    n_trials, n_tuples = 0, 0
    used = corres
    if o.tuple_test:
        used, n_trials = _F.fgr_tuple_test(source.xyz32, target.xyz32, corres, o.tuple_scale, o.maximum_tuple_count, seed=o.seed,
                                           batch=o.batch, device=dev)
        n_tuples = int(used.shape[0]) // 3
    r = _F.fgr_optimize(source.xyz32, target.xyz32, used, o.division_factor, o.use_absolute_scale, o.decrease_mu,
                        o.maximum_correspondence_distance, o.iteration_number, device=dev)
    res = evaluate_registration(source, target, o.maximum_correspondence_distance, r["transformation"])
    res.info = {"n_corres": r["n_corres"], "n_reciprocal": int(corres.shape[0]), "n_trials": n_trials, "n_tuples": n_tuples,
                "iterations": r["iterations"], "scale_global": r["scale_global"], "host_waits": r["host_waits"]}
    return res


def registration_fgr_based_on_feature_matching(source, target, source_feature, target_feature, option=None):
    """``o3d.pipelines.registration.registration_fgr_based_on_feature_matching`` (Open3D 0.16): exact feature 1-NN both ways, the
    reciprocal pairs only (no fall-back to the one-way set), then ``registration_fgr_based_on_correspondence``."""
    corres, _ = _F.feature_match(source_feature.rows, target_feature.rows, mutual=True, ransac_n=0, device=source.device_index)
    return registration_fgr_based_on_correspondence(source, target, corres, option)


def do_fgr_registration(point_cloud_first, point_cloud_second, registration_params):
    source_down, source_fpfh = preprocess_point_cloud(point_cloud_first, registration_params.voxel_size, orient=getattr(registration_params, "orient_normals", "centroid"))
    target_down, target_fpfh = preprocess_point_cloud(point_cloud_second, registration_params.voxel_size, orient=getattr(registration_params, "orient_normals", "centroid"))

    options = FastGlobalRegistrationOption(registration_params.division_factor,
                                           registration_params.use_absolute_scale,
                                           registration_params.decrease_mu,
                                           registration_params.maximum_correspondence,
                                           registration_params.max_iterations,
                                           registration_params.tuple_scale,
                                           registration_params.max_tuple_count,
                                           registration_params.tuple_test,
                                           seed=getattr(registration_params, "seed", 0))

    result = registration_fgr_based_on_feature_matching(source_down, target_down, source_fpfh, target_fpfh, options)

    return result


class SC2Option:
    """The parameters of the compatibility-graph method (``gsr_sc2_params`` without the threshold, which the shims take as
    ``max_correspondence_distance``)."""

    def __init__(self, seed_ratio=0.2, max_seeds=4096, k1=30, k2=20, refine_iterations=20):
        self.seed_ratio, self.max_seeds = float(seed_ratio), int(max_seeds)
        self.k1, self.k2, self.refine_iterations = int(k1), int(k2), int(refine_iterations)


def registration_sc2_based_on_correspondence(source, target, corres, max_correspondence_distance, option=None):
    """Compatibility-graph global registration over given correspondences ``(m, 2)`` (source row, target row): rigid, deterministic,
    no sampling (``features.sc2_correspondence``).  ``max_correspondence_distance`` is both the compatibility and the inlier
    threshold.  ``fitness`` and ``inlier_rmse`` are over the correspondences, as for RANSAC."""
    o = option or SC2Option()
    r = _F.sc2_correspondence(source.xyz32, target.xyz32, corres, max_correspondence_distance, seed_ratio=o.seed_ratio,
                              max_seeds=o.max_seeds, k1=o.k1, k2=o.k2, refine_iters=o.refine_iterations, device=source.device_index)
    info = {k: r[k] for k in ("best_seed", "best_index", "n_seeds", "n_valid", "n_edges", "refine_steps", "host_waits")}
    return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"], info=info)


def registration_sc2_based_on_feature_matching(source, target, source_feature, target_feature, mutual_filter,
                                               max_correspondence_distance, option=None):
    """Exact feature 1-NN, optional mutual filter (RANSAC's rule: the one-way set below 9 reciprocal pairs), then
    ``registration_sc2_based_on_correspondence``."""
    if not (max_correspondence_distance > 0.0):
        return RegistrationResult()
    corres, used_mutual = _F.feature_match(source_feature.rows, target_feature.rows, mutual=bool(mutual_filter), ransac_n=3,
                                           device=source.device_index)
    res = registration_sc2_based_on_correspondence(source, target, corres, max_correspondence_distance, option)
    res.info["used_mutual"] = used_mutual
    res.info["n_corres"] = int(corres.shape[0])
    return res


def do_sc2_registration(point_cloud_first, point_cloud_second, params):
    source_down, source_fpfh = preprocess_point_cloud(point_cloud_first, params.voxel_size, orient=getattr(params, "orient_normals", "centroid"))
    target_down, target_fpfh = preprocess_point_cloud(point_cloud_second, params.voxel_size, orient=getattr(params, "orient_normals", "centroid"))
    option = SC2Option(params.seed_ratio, params.max_seeds, params.k1, params.k2, params.refine_iterations)
    return registration_sc2_based_on_feature_matching(source_down, target_down, source_fpfh, target_fpfh, params.mutual_filter,
                                                      params.max_correspondence, option)
