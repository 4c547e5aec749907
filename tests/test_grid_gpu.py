"""The four public routes over the uniform point grid (csrc/grid.hip, csrc/gsr_grid.h) on the smallest inputs where a grid walk can
go wrong, each against the CPU model the route's own tests use, with their assertions and tolerances:

    icp.normals_knn            oracle.normals_knn                      < 1e-9                    (tests/test_sparse_gpu.py)
    features.hybrid_search     global_model.hybrid_search              exact lists               (tests/test_global_registration_gpu.py)
    clean.outlier_mask         clean_model.outlier_model               mask, counts exact; means within (k + 2) 2^-52 relative
                                                                                                  (tests/test_clean_gpu.py)
    IcpContext.color_gradient  oracle.color_gradient                   < 1e-9 max(1, |want|)     (tests/test_icp_gpu.py)

Inputs (seeded, n <= 2 003): 1, 2 and 3 points (fewer than any k); 64 copies of one point (one cell, every distance tied); 1 000
points on a line and in an axis-aligned plane (gy = gz = 1 / gz = 1: rings leave the grid on several sides at once); an 8 x 8 x 8
integer lattice (exact ties in d^2 at every shell); 2 000 uniform points plus 3 at 10^4 times the extent (a robust box: queries and
neighbours clamped into boundary cells).  k at both ends of each route's range.

Before the GPU runs, every pairing is shown to be one the CPU model decides without a coin toss.  Ties: the oracle and the
restatement order neighbours by (d^2, input index), as the kernels do, and the floater model's means do not depend on the order of
equal distances -- no tie is broken arbitrarily anywhere.  Normals: the two smallest eigenvalues of every neighbourhood covariance
are apart (or the covariance is the identity / exactly zero, where the model has a documented answer).  Colour gradients: every 3x3
system solved is well conditioned.  Floaters: no mean within 1e-9 of the threshold, no d^2 within 1e-9 of radius^2.  Pairings the
models do NOT decide are left out, not loosened: the line under normals_knn(30) (two equal smallest eigenvalues) and, of the robust
box input, the rows of the three far points (their covariances cancel to noise); two points under nb_neighbors > 1 (both means equal
the threshold); the line and the 64 copies under the colour gradient (a singular system)."""
import functools
import math

import numpy as np
import pytest
import torch

import clean_model as M
import global_model as G

pytestmark = pytest.mark.gpu

FAR = 1e4


@functools.lru_cache(maxsize=None)
def cloud(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("n1", "n2", "n3"):
        x = rng.uniform(-1.0, 1.0, (int(name[1]), 3))
    elif name == "dup64":
        x = np.tile([[0.25, -0.5, 0.125]], (64, 1))
    elif name == "line":
        x = np.stack([rng.uniform(0.0, 1.0, 1000), np.full(1000, 0.5), np.full(1000, -0.25)], 1)
    elif name == "plane":
        x = np.stack([rng.uniform(0.0, 1.0, 1000), rng.uniform(0.0, 1.0, 1000), np.full(1000, 0.5)], 1)
    elif name == "lattice":
        g = np.arange(8.0)
        x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    elif name == "far":
        x = np.concatenate([rng.uniform(-1.0, 1.0, (2000, 3)), [[2 * FAR, 0.0, 0.0], [-2 * FAR, 2 * FAR, 0.0], [0.3, -0.2, 2 * FAR]]])
    else:
        raise KeyError(name)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


ALL = ("n1", "n2", "n3", "dup64", "line", "plane", "lattice", "far")


@functools.lru_cache(maxsize=None)
def ranked(name):
    """(order, d2): per row every point in (d^2, input index) order and the sorted d^2 (float64 from the float32 coordinates)"""
    x = cloud(name).astype(np.float64)
    d = x[:, None, :] - x[None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    order = np.argsort(d2, axis=1, kind="stable")
    return order, np.take_along_axis(d2, order, 1)


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


# ---- normals_knn ----------------------------------------------------------------------------------------------------------
def _normals_decided(name, knn):
    """per row: the neighbourhood covariance is the identity (< 3 neighbours), exactly zero, or has its two smallest eigenvalues apart"""
    x = cloud(name).astype(np.float64)
    order, _ = ranked(name)
    k = min(knn, len(x))
    if k < 3:
        return np.ones(len(x), bool)
    P = x[order[:, :k]]
    mu = P.mean(1, keepdims=True)
    C = np.einsum("nki,nkj->nij", P - mu, P - mu) / k
    lam = np.linalg.eigvalsh(C)
    return (lam[:, 2] == 0) | (lam[:, 1] - lam[:, 0] > 1e-6 * lam[:, 2])


NORMALS = [(n, 1) for n in ALL] + [(n, 30) for n in ALL if n != "line"]


def test_normals_pairing_left_out_is_the_undecided_one():
    assert not _normals_decided("line", 30).any()


@pytest.mark.parametrize("name,knn", NORMALS)
def test_normals_knn(lib, oracle, name, knn):
    from gaussiansplattingregistration_amd import icp
    xyz = cloud(name)
    rows = _normals_decided(name, knn)
    if name == "far" and knn == 30:     # a far point and 29 of the cube: the small eigenvalues drown in the cancellation of the cumulants
        assert rows[:2000].all() and not rows[2000:].any()
    else:
        assert rows.all()
    want = oracle.normals_knn(xyz.astype(np.float64), knn)
    if knn < 3 or len(xyz) < 3 or name == "dup64":          # identity covariance, or the zero matrix: the model's documented (0, 0, 1)
        assert np.array_equal(want, np.tile([[0.0, 0.0, 1.0]], (len(xyz), 1)))
    got = icp.normals_knn(xyz, knn)
    assert got.shape == want.shape and np.abs(got - want)[rows].max() < 1e-9


# ---- hybrid search --------------------------------------------------------------------------------------------------------
# radius per input: some neighbours; "far" also with every point of the cube in reach (2 000 candidates: the LDS list overflows and
# is cut by rank).  The lattice at radius 2: d^2 = 4 sits ON the bound (d^2 <= r^2 keeps it), exact in float64.
HYBRID_RADII = {"n1": (10.0,), "n2": (10.0,), "n3": (10.0,), "dup64": (1.0,), "line": (0.05,), "plane": (0.1,), "lattice": (2.0,), "far": (0.3, 4.0)}
HYBRID = [(n, r, k) for n in ALL for r in HYBRID_RADII[n] for k in (1, 65, 512)]


@pytest.mark.parametrize("name,radius,max_nn", HYBRID)
def test_hybrid_search(lib, name, radius, max_nn):
    from gaussiansplattingregistration_amd import features
    xyz = cloud(name)
    want = G.hybrid_search(xyz, radius, max_nn)
    # the restatement against the brute-force ranking: (d^2, index) order, nothing arbitrary
    order, d2 = ranked(name)
    for i in (0, len(xyz) // 2, len(xyz) - 1):
        m = min(int(np.count_nonzero(d2[i] <= radius * radius)), max_nn)
        assert np.array_equal(want[i], order[i, :m])
    nbr, cnt = features.hybrid_search(xyz, radius, max_nn)
    for i in range(len(xyz)):
        assert cnt[i] == len(want[i]) and np.array_equal(nbr[i, :cnt[i]], want[i]), i
    if name == "far" and radius == 4.0:
        assert cnt[:2000].min() == min(max_nn, 2000) and (cnt[2000:] == 1).all()


# ---- outlier mask ---------------------------------------------------------------------------------------------------------
CLEAN_RADIUS = {"n1": 1.0, "n2": 1.0, "n3": 1.0, "dup64": 0.5, "line": 0.01, "plane": 0.08, "lattice": 1.5, "far": 0.25}
CLEAN = [(n, k) for n in ALL for k in (1, 8, 9, 32) if not (n == "n2" and k > 1)]     # two points, k' = 2: both means EQUAL the threshold


@functools.lru_cache(maxsize=None)
def _clean_model(name, k, stat_only):
    return M.outlier_model(cloud(name), nb_neighbors=k, std_ratio=2.0, radius=0.0 if stat_only else CLEAN_RADIUS[name], nb_points=2)


def _clean_decided(want):
    thr, mean = want["threshold"], want["mean_dist"]
    pos = mean > 0
    if math.isfinite(thr) and pos.any() and not np.min(np.abs(mean[pos] - thr)) >= 1e-9 * thr:
        return False
    return want["margin_radius"] >= 1e-9


def _clean_check(name, k, want, mask, info):
    """tests/test_clean_gpu.py::_check, for a model computed here"""
    assert mask.dtype == np.uint8 and np.array_equal(mask, want["mask"]), np.flatnonzero(mask != want["mask"])[:10]
    for key in ("n_nonfinite", "n_gate_opacity", "n_gate_scale", "n_statistical", "n_radius", "n_kept"):
        assert info[key] == want[key], (key, info[key], want[key])
    assert info["n"] == len(mask)
    got, ref = info["mean_dist"], want["mean_dist"]
    assert np.array_equal(got == -1, ref == -1)
    reached = ref >= 0
    err = float(np.max(np.abs(got[reached] - ref[reached]) / np.maximum(ref[reached], 1e-300))) if reached.any() else 0.0
    print(f"grid clean[{name}, k {k}]: kept {info['n_kept']} deferred {info['deferred_queries']} max relative mean_dist error {err:.3g}")
    assert err <= (k + 2) * 2.0 ** -52
    assert np.array_equal(info["count"], want["count"])
    if math.isfinite(want["threshold"]):
        assert abs(info["threshold"] - want["threshold"]) <= 1e-12 * want["threshold"]
        assert abs(info["cloud_mean"] - want["cloud_mean"]) <= 1e-12 * want["cloud_mean"]
    else:
        assert math.isnan(info["threshold"])


@pytest.mark.parametrize("stat_only", [False, True])
@pytest.mark.parametrize("name,k", CLEAN)
def test_outlier_mask(lib, name, k, stat_only):
    """stat_only: the grid is built for the statistical stage alone (no radius: the finest cells); else both stages, mean_dist and count"""
    from gaussiansplattingregistration_amd import clean
    from gaussiansplattingregistration_amd.params.clean_parameters import CleanParams
    want = _clean_model(name, k, stat_only)
    assert _clean_decided(want)
    P = CleanParams(nb_neighbors=k, std_ratio=2.0, radius=0.0 if stat_only else CLEAN_RADIUS[name], nb_points=2)
    mask, info = clean.outlier_mask(cloud(name), P, with_mean_dist=True, with_count=True)
    _clean_check(name, k, want, mask, info)
    if name == "far":
        assert not mask[2000:].any()
        if k > 1:                                        # (k = 1: a query is its own nearest neighbour and stops in ring 0)
            assert info["deferred_queries"] > 0          # the three far queries leave the lane-per-query walk


# ---- colour gradient ------------------------------------------------------------------------------------------------------
# two radii where the walk can stop either way: on the radius (fewer than 30 within it) and on the full list
COLOR_RADII = {"n1": (1.0,), "n2": (1.0,), "n3": (10.0,), "plane": (0.05, 1.0), "lattice": (1.5, 3.0), "far": (0.3, 4.0)}
COLOR = [(n, r) for n in COLOR_RADII for r in COLOR_RADII[n]]


@functools.lru_cache(maxsize=None)
def _dressing(name):
    rng = np.random.default_rng(7 + len(name))
    nrm = rng.normal(size=(len(cloud(name)), 3))
    if name == "plane":                                  # the plane's own normal, tilted a little: random ones make the fit nearly singular
        nrm = 0.1 * nrm + [0.0, 0.0, 1.0]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return nrm, rng.uniform(0.0, 1.0, (len(nrm), 3))


def _gradient_decided(name, radius):
    """the worst condition number of the 3x3 systems InitializePointCloudForColoredICP solves (1 when none is solved)"""
    x = cloud(name).astype(np.float64)
    nrm, _ = _dressing(name)
    order, d2 = ranked(name)
    worst = 1.0
    for i in range(len(x)):
        nn = int(np.count_nonzero(d2[i, :30] < radius * radius))
        if nn < 4:
            continue
        v = x[order[i, 1:nn]] - x[i]
        rows = v - (v @ nrm[i])[:, None] * nrm[i]
        A = rows.T @ rows + (nn - 1) ** 2 * np.outer(nrm[i], nrm[i])
        worst = max(worst, np.linalg.cond(A))
    return worst < 1e8


def test_gradient_pairings_left_out_are_the_undecided_ones():
    assert not _gradient_decided("line", 0.05) and not _gradient_decided("dup64", 1.0)


@pytest.mark.parametrize("name,radius", COLOR)
def test_color_gradient(lib, oracle, name, radius):
    from gaussiansplattingregistration_amd import icp
    assert _gradient_decided(name, radius)
    xyz = cloud(name)
    nrm, col = _dressing(name)
    want = oracle.color_gradient(xyz.astype(np.float64), nrm, col, radius)
    if len(xyz) < 4:
        assert not want.any()                           # fewer than 4 neighbours: the zero gradient
    else:
        assert want.any() and np.isfinite(want).all()
    with icp.IcpContext() as c:
        c.set_target(xyz, nrm, radius / 2.0)              # gradients use Hybrid(2 * max_corr, 30)
        c.set_target_color(col)
        got = c.color_gradient()
    assert np.abs(got - want).max() < 1e-9 * max(1.0, np.abs(want).max())
