"""Floater removal restated in float64 NumPy / SciPy: the reference gsr_outlier_mask (csrc/clean.hip) is held to, the cases the
GPU tests run, and for every case how far it is from a decision that rounding could turn.

The definition (include/gsr_hip.h; Open3D 0.16's RemoveStatisticalOutlier / RemoveRadiusOutlier restated from the published
source -- recalled, parity with Open3D is unpinned).  All arithmetic is float64 on the float32 inputs, every comparison is written
so that NaN fails it, d2(i, j) = (xi - xj)^2 + (yi - yj)^2 + (zi - zj)^2 summed left to right without contraction.  The stages run
in this order; each sees only the survivors of the one before, a dead row is neither a query nor a candidate.

1. finite       a row with a non-finite coordinate is dead (n_nonfinite).  A stated deviation: nanoflann on NaN is undefined.
2. gates        dead unless raw_opacity >= min_raw_opacity (-inf: off; Python passes logit(min_opacity) computed once in float64);
                dead unless max(scaling[i, 0..2]) <= max_log_scale (+inf: off; ln(max_extent)).
3. statistical  on iff nb_neighbors >= 1 (std_ratio > 0).  A = the alive set, k' = min(nb_neighbors, |A|);
                mean_i = (sum of sqrt(d2) over the k' smallest d2(i, j), j in A INCLUDING j = i, added in ascending d2 order from 0.0)
                / k';  valid = |A|;  cloud_mean = sum_{mean_i > 0} mean_i / valid;
                std_dev = sqrt(sum_{mean_i > 0} (mean_i - cloud_mean)^2 / (valid - 1));  threshold = cloud_mean + std_ratio std_dev;
                keep iff mean_i > 0 and mean_i < threshold.  valid <= 1: the threshold is NaN, nothing survives.  Ties among equal
                distances cannot change mean_i: no index tie-break.
4. radius       on iff radius > 0.  count_i = #{j alive : d2(i, j) < radius radius}, self included, STRICT (nanoflann's radius
                result set);  keep iff count_i > nb_points.

Output: mask (uint8, 1 = kept), mean_dist (float64, -1 for rows that did not reach stage 3), count (int32, -1 likewise).
"""
import math

import numpy as np
from scipy.spatial import cKDTree

INF = math.inf


def _d2(a, b):
    """d2 of the definition: float64, (dx dx + dy dy) + dz dz"""
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return dx * dx + dy * dy + dz * dz


def _knn_d2(x, k):
    """(m, k): the k smallest d2(i, j) over j (self included) per row, ascending.  Small clouds by brute force; large ones take
    k + 16 candidates from a k-d tree (whose own distances round differently) and re-rank them by the exact d2."""
    m = x.shape[0]
    if m <= 700:
        d2 = _d2(x[:, None, :], x[None, :, :])
        return np.sort(d2, axis=1)[:, :k]
    kk = min(m, k + 16)
    _, idx = cKDTree(x).query(x, k=kk)
    d2 = _d2(x[:, None, :], x[idx])
    return np.sort(d2, axis=1)[:, :k]


def outlier_model(xyz, nb_neighbors=20, std_ratio=2.0, radius=0.0, nb_points=16, min_raw_opacity=-INF, max_log_scale=INF,
                  raw_opacity=None, scaling=None):
    """-> dict(mask, mean_dist, count, stage, cloud_mean, std_dev, threshold, n_*, margin_stat, margin_radius)"""
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32
    x = xyz.astype(np.float64)
    n = x.shape[0]
    stage = np.zeros(n, np.int32)
    with np.errstate(invalid="ignore"):
        stage[~np.isfinite(x).all(axis=1)] = 1
        if min_raw_opacity > -INF:
            op = np.asarray(raw_opacity, np.float32).astype(np.float64).reshape(n)
            stage[(stage == 0) & ~(op >= min_raw_opacity)] = 2
        if max_log_scale < INF:
            sc = np.asarray(scaling, np.float32).astype(np.float64).reshape(n, 3)
            stage[(stage == 0) & ~(np.max(sc, axis=1) <= max_log_scale)] = 3        # (np.max hands a NaN on: it fails the comparison)
    mean_dist = np.full(n, -1.0)
    count = np.full(n, -1, np.int32)
    out = {"cloud_mean": 0.0, "std_dev": 0.0, "threshold": 0.0, "margin_stat": INF, "margin_radius": INF}
    if nb_neighbors >= 1:
        A = np.flatnonzero(stage == 0)
        valid = len(A)
        kp = min(nb_neighbors, valid)
        mean = np.zeros(valid)
        if valid:
            d2 = _knn_d2(x[A], kp)
            s = np.zeros(valid)
            for t in range(kp):                       # ascending d2 order, from 0.0
                s = s + np.sqrt(d2[:, t])
            mean = s / kp
        mean_dist[A] = mean
        pos = mean > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            cloud_mean = np.float64(mean[pos].sum()) / np.float64(valid)
            std_dev = np.sqrt(np.float64(((mean[pos] - cloud_mean) ** 2).sum()) / np.float64(valid - 1))
            threshold = cloud_mean + std_ratio * std_dev
            keep = pos & (mean < threshold)
            if valid and np.isfinite(threshold):
                out["margin_stat"] = float(np.min(np.abs(mean - threshold)) / threshold)
        stage[A[~keep]] = 4
        out.update(cloud_mean=float(cloud_mean), std_dev=float(std_dev), threshold=float(threshold))
    if radius > 0:
        A = np.flatnonzero(stage == 0)
        r2 = radius * radius
        cnt = np.zeros(len(A), np.int32)
        if len(A):
            xa = x[A]
            nbrs = cKDTree(xa).query_ball_point(xa, radius * (1 + 1e-6) + 1e-300)
            for i, js in enumerate(nbrs):
                d2 = _d2(xa[i][None, :], xa[js])
                cnt[i] = int(np.count_nonzero(d2 < r2))
                out["margin_radius"] = min(out["margin_radius"], float(np.min(np.abs(d2 - r2)) / r2))
        count[A] = cnt
        stage[A[~(cnt > nb_points)]] = 5
    out.update(mask=(stage == 0).astype(np.uint8), mean_dist=mean_dist, count=count, stage=stage,
               n_nonfinite=int((stage == 1).sum()), n_gate_opacity=int((stage == 2).sum()), n_gate_scale=int((stage == 3).sum()),
               n_statistical=int((stage == 4).sum()), n_radius=int((stage == 5).sum()), n_kept=int((stage == 0).sum()))
    return out


def logit(a):
    """what CleanParams hands the library for min_opacity (float64)"""
    return -INF if a <= 0 else math.log(a) - math.log1p(-a)


# ---- the cases ---------------------------------------------------------------------------------------------------------------

N_CORE, N_FLOAT = 4000, 40


def base_cloud(seed=0, far=False):
    """4000 x U(-1, 1)^3 and 40 floaters at radii U(5, 50) along random directions (far: at 10^6 box radii), float32"""
    rng = np.random.default_rng(seed)
    core = rng.uniform(-1.0, 1.0, (N_CORE, 3))
    dirs = rng.normal(size=(N_FLOAT, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    radii = rng.uniform(5.0, 50.0, N_FLOAT)
    if far:
        radii = np.full(N_FLOAT, 1e6 * math.sqrt(3.0))
    return np.concatenate([core, dirs * radii[:, None]]).astype(np.float32)


def _f32_next(v, up):
    v = np.float32(v)
    return np.nextafter(v, np.float32(INF if up else -INF), dtype=np.float32)


def gates_case():
    """base + an isolated point P whose only near neighbours are a clump the opacity gate removes, + opacities and log-scales one
    float32 on either side of the thresholds.  The stage order decides P: with the clump gated out it has no neighbour and the
    statistical stage drops it; were gated rows still candidates it would be kept."""
    rng = np.random.default_rng(11)
    xyz = base_cloud()
    P = np.float32([[20.0, 20.0, 20.0]])
    clump = (P + rng.normal(scale=0.01, size=(30, 3))).astype(np.float32)
    xyz = np.concatenate([xyz, P, clump])
    n = len(xyz)
    min_opacity, max_extent = 0.1, 0.5
    thr_o, thr_s = logit(min_opacity), math.log(max_extent)
    op = np.full(n, 2.0, np.float32)
    sc = np.full((n, 3), -3.0, np.float32)
    op[N_CORE + N_FLOAT + 1:] = -5.0                              # the clump: nearly transparent
    lo_o, hi_o = np.float32(thr_o), np.float32(thr_o)
    lo_o = lo_o if float(lo_o) < thr_o else _f32_next(lo_o, False)
    hi_o = hi_o if float(hi_o) >= thr_o else _f32_next(hi_o, True)
    op[0:10], op[10:20] = lo_o, hi_o                              # just below: dropped; at or just above: kept
    lo_s, hi_s = np.float32(thr_s), np.float32(thr_s)
    lo_s = lo_s if float(lo_s) <= thr_s else _f32_next(lo_s, False)
    hi_s = hi_s if float(hi_s) > thr_s else _f32_next(hi_s, True)
    sc[20:30, 1], sc[30:40, 2] = lo_s, hi_s                       # at or just below: kept; just above: dropped
    sc[5, 0] = hi_s                                               # fails both gates: counted by the first
    op[40], sc[41, 1] = np.nan, np.nan                            # NaN fails either comparison
    return dict(xyz=xyz, raw_opacity=op, scaling=sc, min_opacity=min_opacity, max_extent=max_extent, nb_neighbors=20, std_ratio=2.0,
                p_row=N_CORE + N_FLOAT)


def nonfinite_case():
    xyz = base_cloud().copy()
    rows = [0, 63, 64, 1000, 2047, 3999, N_CORE, N_CORE + 7, N_CORE + N_FLOAT - 1]
    vals = [np.nan, np.inf, -np.inf]
    for t, r in enumerate(rows):
        xyz[r, t % 3] = vals[t % 3]
    return dict(xyz=xyz, nb_neighbors=20, std_ratio=2.0, rows=rows)


def duplicates_cloud():
    xyz = base_cloud()
    dup = np.tile(np.float32([[0.25, -0.5, 0.125]]), (40, 1))
    return np.concatenate([xyz[:2000], dup, xyz[2000:]])


def clustered_cloud(seed=7):
    rng = np.random.default_rng(seed)
    a = rng.normal(scale=0.05, size=(3000, 3))
    b = rng.normal(scale=0.5, size=(300, 3)) + np.array([6.0, 0.0, 0.0])
    return np.concatenate([a, b]).astype(np.float32)


def lattice_cloud(m=6):
    g = np.arange(m, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def small_cloud(n):
    return np.random.default_rng(100 + n).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


SMALL_N = (1, 5, 63, 64, 65, 257)
DUP_K = (8, 20, 32)


def gpu_cases():
    """name -> (xyz, keyword arguments of outlier_model, exact): every case the GPU tests compare with the model.  exact: integer
    coordinates, every d2 is computed without rounding (the lattice sits on radius^2 on purpose)."""
    c = {}
    c["base"] = (base_cloud(), dict(nb_neighbors=20, std_ratio=2.0), False)
    c["far"] = (base_cloud(far=True), dict(nb_neighbors=20, std_ratio=2.0), False)
    c["clustered"] = (clustered_cloud(), dict(nb_neighbors=20, std_ratio=1.0), False)
    c["lattice_1"] = (lattice_cloud(), dict(nb_neighbors=0, radius=1.0, nb_points=6), True)
    c["lattice_next"] = (lattice_cloud(), dict(nb_neighbors=0, radius=float(np.nextafter(1.0, 2.0)), nb_points=6), True)
    for n in SMALL_N:
        c[f"small_{n}"] = (small_cloud(n), dict(nb_neighbors=20, std_ratio=2.0), False)
    for k in DUP_K:
        c[f"duplicates_{k}"] = (duplicates_cloud(), dict(nb_neighbors=k, std_ratio=2.0), False)
    nf = nonfinite_case()
    c["nonfinite"] = (nf["xyz"], dict(nb_neighbors=20, std_ratio=2.0), False)
    g = gates_case()
    c["gates"] = (g["xyz"], dict(nb_neighbors=20, std_ratio=2.0, min_raw_opacity=logit(g["min_opacity"]), max_log_scale=math.log(g["max_extent"]),
                                 raw_opacity=g["raw_opacity"], scaling=g["scaling"]), False)
    c["base_radius"] = (base_cloud(), dict(nb_neighbors=20, std_ratio=2.0, radius=0.25, nb_points=16), False)
    return c


_MODEL_CACHE = {}


def model_of(name):
    """the model's answer for a case, computed once per process"""
    if name not in _MODEL_CACHE:
        xyz, kw, _ = gpu_cases()[name]
        _MODEL_CACHE[name] = outlier_model(xyz, **kw)
    return _MODEL_CACHE[name]
