"""Edge-shape inputs of csrc/features.hip (test infrastructure): the inputs of tests/test_global_edges_gpu.py and what the restatement
(tests/global_model.py) says about each, built once and shared with tests/test_global_model_cpu.py, which shows without a GPU
that the restatement decides every one of them.  Nothing here touches the library."""
from __future__ import annotations

import functools

import numpy as np

import global_model as G

TRIP = 524288          # one trip of the grid-stride loops: k_spfh 4096 x 128 threads, stride_grid 2048 x 256
TAIL = 300


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def lattice(side):
    """side^3 integer points, float32, x slowest (index = (x * side + y) * side + z)"""
    g = np.arange(float(side))
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- FPFH
RADII = (1.0, 1.5, 2.0)
Z = np.array([0.0, 0.0, 1.0])


def _lattice_normals(kind):
    x = lattice(6)
    n = len(x)
    if kind == "plusz":            # p2 - p1 parallel to both normals, no swap
        return np.repeat(Z[None], n, 0)
    if kind == "checker":          # the +z point of a z-pair is the better aligned one: the parallel pair through the swap branch
        even = (x.sum(1).astype(np.int64) % 2) == 0
        return np.where(even[:, None], np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), Z)
    if kind == "parity":           # +-z by index parity (= parity of the z coordinate)
        return np.where((np.arange(n) % 2 == 0)[:, None], Z, -Z)
    if kind == "mod3":             # the x, y, z axis by index mod 3
        return np.eye(3)[np.arange(n) % 3]
    if kind == "zero":
        return np.zeros((n, 3))
    raise KeyError(kind)


def _small(name):
    """n1, n2, n3 and dup64 as tests/test_grid_gpu.py builds them"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "dup64":
        return np.tile([[0.25, -0.5, 0.125]], (64, 1)).astype(np.float32)
    return rng.uniform(-1.0, 1.0, (int(name[1]), 3)).astype(np.float32)


UNIFORM_SEED = 0       # the first seed at which no pair feature of the three uniform clouds lies within 1e-9 of a bin edge
TAIL_SEED = 0          # the same for the 300 clustered points of the two-trip cloud
SMALL_SEED = 0         # normals of n1, n2, n3 and dup64

# name -> (radius, max_nn); the inputs come from fpfh_input(name)
FPFH_CASES = {}
for _k in ("plusz", "checker", "zero"):
    for _r in RADII:
        FPFH_CASES["%s-r%.1f" % (_k, _r)] = (_r, 100)
FPFH_CASES["parity-r1.0"] = (1.0, 100)
FPFH_CASES["dup64"] = (1.0, 100)
for _s in ("n1", "n2", "n3"):
    for _nn in (1, 2, 100):
        FPFH_CASES["%s-nn%d" % (_s, _nn)] = (10.0, _nn)
for _n in (127, 128, 129):
    FPFH_CASES["uniform%d" % _n] = (0.25, 65)
# left out of the GPU file (the restatement does not decide them); test_global_model_cpu.py shows why
FPFH_UNDECIDED = {"parity-r1.5": (1.5, 100), "parity-r2.0": (2.0, 100), "mod3-r1.0": (1.0, 100), "mod3-r1.5": (1.5, 100),
                  "mod3-r2.0": (2.0, 100)}


@functools.lru_cache(maxsize=None)
def fpfh_input(name):
    """(xyz float32 (n, 3), normals float64 (n, 3), radius, max_nn), read-only"""
    radius, max_nn = FPFH_CASES[name] if name in FPFH_CASES else FPFH_UNDECIDED[name]
    head = name.split("-")[0]
    if head in ("plusz", "checker", "parity", "mod3", "zero"):
        xyz, nrm = lattice(6), _lattice_normals(head)
    elif head in ("dup64", "n1", "n2", "n3"):
        xyz = _small(head)
        nrm = _unit(np.random.default_rng(SMALL_SEED), len(xyz))
    else:
        n = int(head[len("uniform"):])
        rng = np.random.default_rng(UNIFORM_SEED)
        xyz = rng.random((n, 3)).astype(np.float32)
        nrm = _unit(rng, n)
    nrm = np.ascontiguousarray(nrm, np.float64)
    xyz.setflags(write=False)
    nrm.setflags(write=False)
    return xyz, nrm, radius, max_nn


@functools.lru_cache(maxsize=None)
def fpfh_want(name):
    """(neighbour lists, spfh, fpfh) of the restatement"""
    xyz, nrm, radius, max_nn = fpfh_input(name)
    nbrs = G.hybrid_search(xyz, radius, max_nn)
    spfh, fpfh = G.spfh_fpfh(xyz, nrm, radius, max_nn, nbrs)
    return nbrs, spfh, fpfh


# the known answer derived by hand in tests/test_global_model_cpu.py: (xyz, normals, radius, max_nn) and both FPFH rows
TWO_POINTS = (np.array([[0, 0, 0], [0, 0, 1]], np.float32), np.array([[0.0, 0, 1], [0, 0, 1]]), 2.0, 10)
TWO_POINTS_FPFH = np.zeros((2, 33))
TWO_POINTS_FPFH[:, [5, 16, 27]] = 200.0

TWO_TRIP_RADIUS, TWO_TRIP_NN = 0.25, 16


@functools.lru_cache(maxsize=None)
def two_trip_cloud():
    """TRIP + TAIL points: the first TRIP points of the 81^3 integer lattice (every one alone within the radius), then TAIL points in
    a box of side 0.2 about (40.5, 40.5, 40.5), farther than 0.5 from every lattice point.  Random unit normals."""
    rng = np.random.default_rng(TAIL_SEED)
    tail = (40.5 + 0.2 * (rng.random((TAIL, 3)) - 0.5)).astype(np.float32)
    xyz = np.concatenate([lattice(81)[:TRIP], tail])
    nrm = np.ascontiguousarray(_unit(rng, TRIP + TAIL))
    xyz.setflags(write=False)
    nrm.setflags(write=False)
    return xyz, nrm


# ---------------------------------------------------------------------------------------------------------------- matching
FM_SHAPES = [(1, 1), (1, 33), (255, 31), (256, 32), (257, 33), (300, 512), (300, 513), (70, 1025)]
FM_PLANTED = [(300, 513), (70, 1025)]
FM_TIE_SRC, FM_TIE_TGT, FM_LAST_SRC, FM_NAN_SRC = 5, 3, 9, 11      # planted rows, see fm_planted


def fm_chunks(na, nb):
    """(number of chunks, chunk length) of the target in nn_rows of csrc/features.hip:
        gx = ceil(na / 256); nch = min(ceil(2048 / gx), ceil(nb / 512), 65535), at least 1; chunk = ceil(nb / nch); nch = ceil(nb / chunk)
    Chunk c covers target rows [c * chunk, min((c + 1) * chunk, nb))."""
    gx = (na + 255) // 256
    nch = max(1, min((2048 + gx - 1) // gx, (nb + 511) // 512, 65535))
    chunk = (nb + nch - 1) // nch
    return (nb + chunk - 1) // chunk, chunk


@functools.lru_cache(maxsize=None)
def fm_input(na, nb):
    rng = np.random.default_rng(1000 * na + nb)
    fs, ft = rng.random((na, 33)) * 50, rng.random((nb, 33)) * 50
    fs.setflags(write=False)
    ft.setflags(write=False)
    return fs, ft


@functools.lru_cache(maxsize=None)
def fm_planted(na, nb, nan):
    """fm_input with: target row FM_TIE_TGT (chunk 0) repeated as the last target row (last chunk) and as source row FM_TIE_SRC, whose
    two zero distances meet only in k_fm_merge; source row FM_LAST_SRC equal to target row nb - 2 (a strict minimum in the last
    chunk); with `nan`, source row FM_NAN_SRC all NaN."""
    fs, ft = (a.copy() for a in fm_input(na, nb))
    ft[nb - 1] = ft[FM_TIE_TGT]
    fs[FM_TIE_SRC] = ft[FM_TIE_TGT]
    fs[FM_LAST_SRC] = ft[nb - 2]
    if nan:
        fs[FM_NAN_SRC] = np.nan
    fs.setflags(write=False)
    ft.setflags(write=False)
    return fs, ft


FM_TWO_TRIP = (TRIP + TAIL, 40)


# ---------------------------------------------------------------------------------------------------------------- RANSAC
MAX_CORR = 0.02
CHECKS_ALL = [(G.EDGE, 0.9), (G.DIST, 0.03), (G.NORMAL, 0.5)]       # CHECKS["all"] of tests/test_global_registration_gpu.py
RANSAC_M = (3, 5, 255, 256, 257)
_VARIANTS = {
    "b250": dict(max_iteration=1001, batch=250, confidence=0.999),   # with confidence 1: batches of 250, 250, 250, 250 and 1
    "b1": dict(max_iteration=7, batch=1, confidence=0.999),
    "conf1": dict(max_iteration=1001, batch=250, confidence=1.0),
    "it1": dict(max_iteration=1, batch=250, confidence=0.999),
}
# The sampler seed of each case: the first one (from 0) at which the restatement finds a best hypothesis, no inlier decision of a
# valid hypothesis lies within 1e-6 max_corr^2 of the threshold and the best hypothesis' system is well conditioned
# (tests/test_global_model_cpu.py asserts all three).
RANSAC_SEEDS = {"m3-it1": 5, "m5-it1": 2, "m255-it1": 2, "m256-b1": 6, "m256-it1": 6}        # every other case: 0
RANSAC_CASES = {}
for _m in RANSAC_M:
    for _v, _kw in _VARIANTS.items():
        RANSAC_CASES["m%d-%s" % (_m, _v)] = dict(m=_m, kind=0, ransac_n=3, checkers=(), **_kw)
RANSAC_CASES["m257-checkers"] = dict(m=257, kind=0, ransac_n=3, checkers=tuple(CHECKS_ALL), **_VARIANTS["b250"])
for _m in (6, 70):
    RANSAC_CASES["plane-m%d" % _m] = dict(m=_m, kind=1, ransac_n=6, checkers=(), max_iteration=203, batch=8192, confidence=0.99)
# m = ransac_n leaves one hypothesis, all six rows: the first scene seed (from 5, the default) at which its system is well conditioned
RANSAC_CASES["plane-m6"]["scene_seed"] = 12
RANSAC_CASES["gather-two-trips"] = dict(m=TRIP + TAIL, kind=0, ransac_n=3, checkers=(), max_iteration=8, batch=8, confidence=0.999)


def _small_motion():
    T0 = np.eye(4)                                      # the motion of test_ransac_point_to_plane
    T0[:3, :3] = G.rot((0.2, 1.0, 0.3), 2.0)
    T0[:3, 3] = (0.01, -0.004, 0.006)
    return T0


@functools.lru_cache(maxsize=None)
def ransac_input(name):
    """(positional arguments src, tgt, corres, max_corr; keyword arguments) for features.ransac_correspondence and global_model.ransac"""
    c = RANSAC_CASES[name]
    m = c["m"]
    if name == "gather-two-trips":                      # rows drawn with replacement from the 4 000-point scene, 40 % of them right
        src, tgt, ns, nt, _, _ = G._ransac_case()
        rng = np.random.default_rng(7)
        i = rng.integers(0, len(src), m)
        j = i.copy()
        bad = rng.random(m) > 0.4
        j[bad] = rng.integers(0, len(src), bad.sum())
        corres = np.stack([i, j], 1).astype(np.int32)
    elif c["kind"] == 1:
        src, tgt, ns, nt, corres, _ = G._ransac_case(m=m, inlier=1.0 if m == 6 else 0.7, seed=c.get("scene_seed", 5), curved=True,
                                                     T=_small_motion())
    else:
        src, tgt, ns, nt, corres, _ = G._ransac_case(m=m, inlier=1.0 if m <= 5 else 0.4)
    kw = dict(kind=c["kind"], ransac_n=c["ransac_n"], checkers=list(c["checkers"]), max_iteration=c["max_iteration"],
              confidence=c["confidence"], seed=RANSAC_SEEDS.get(name, 0), batch=c["batch"])
    if c["checkers"]:
        kw.update(src_normals=ns, tgt_normals=nt)
    elif c["kind"] == 1:
        kw.update(tgt_normals=nt)
    return (src, tgt, corres, MAX_CORR), kw


@functools.lru_cache(maxsize=None)
def ransac_want(name):
    """(result of the restatement, its probe)"""
    args, kw = ransac_input(name)
    probe = {}
    return G.ransac(*args, probe=probe, **kw), probe


def ransac_best_rows(name):
    """the sorted correspondence rows of the restatement's best hypothesis"""
    args, kw = ransac_input(name)
    want, _ = ransac_want(name)
    return np.sort(G.ransac_sample(kw["seed"], want["best_index"], 1, len(args[2]), kw["ransac_n"]), axis=1)[0]


def ransac_undecided(name):
    """Reasons why the restatement would not decide the case (empty: it does)."""
    args, kw = ransac_input(name)
    src, tgt, corres, max_corr = args
    want, probe = ransac_want(name)
    why = []
    if want["best_index"] < 0 or want["n_valid"] <= 0:
        return ["no best hypothesis: the case would test nothing"]
    if not probe["min_gap"] > 1e-6 * max_corr * max_corr:
        why.append("a d2 within 1e-6 max_corr^2 of the threshold: %g" % probe["min_gap"])
    rows = ransac_best_rows(name)
    P = src.astype(np.float64)[corres[rows, 0]]
    Q = tgt.astype(np.float64)[corres[rows, 1]]
    if kw["kind"] == 0:
        # Umeyama: the rotation is fixed by the two largest singular values of the cross-covariance; a rank-1 (collinear) triple leaves it open
        s = np.linalg.svd((Q - Q.mean(0)).T @ (P - P.mean(0)), compute_uv=False)
        if not s[1] > 1e-3 * s[0]:
            why.append("best triple nearly collinear: singular values %s" % s)
    else:
        # the 6 x 6 normal equations: two correct solves differ by about 6 cond 2^-52 |x|, |x| < 0.05 here; cond < 1e5 keeps that
        # under 1e-11, a hundredth of the 1e-9 the transformation is held to
        J = np.hstack([np.cross(P, kw["tgt_normals"][corres[rows, 1]]), kw["tgt_normals"][corres[rows, 1]]])
        cond = np.linalg.cond(J.T @ J)
        if not cond < 1e5:
            why.append("best point-to-plane system ill conditioned: %g" % cond)
    # with repeated points among the rows (rows drawn with replacement), a hypothesis of three distinct rows may still hold one point twice
    k = want["n_evaluated"]
    draws = np.sort(G.ransac_sample(kw["seed"], 0, k, len(corres), kw["ransac_n"]), axis=1)
    ok = np.all(draws[:, 1:] != draws[:, :-1], axis=1)
    pts = np.sort(corres[draws[ok], 0], axis=1)
    if np.any(pts[:, 1:] == pts[:, :-1]):
        why.append("a valid hypothesis holds one source point twice")
    return why
