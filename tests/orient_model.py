"""CPU models of the consistent normal orientation (``include/gsr_hip.h``) and the inputs of its tests.

Two independent models of the same definition:

* ``kruskal_dfs``: the unique undirected edge set of the lists, Kruskal in ``np.lexsort((hi, lo, w))`` order, a depth-first
  propagation from every component's lowest vertex, then the vote.
* ``boruvka``: rounds of "every component takes its least outgoing edge in the total order", hooks with a parity, pointer
  doubling -- the algorithm of the device code, written over whole arrays and with one rank per edge instead of the device's two
  atomic passes.

Nothing here has a floating-point sum whose order could differ: the weights are ``1 - |dot|`` with ``dot`` summed x, y, z, the
votes are integer counts.  So the GPU result is compared exactly.
"""
from __future__ import annotations

import functools

import numpy as np


def edges_from_lists(normals, nbr, count):
    """-> (live, lo, hi, dot, w) of the unique undirected edges {lo < hi}: j in i's list or i in j's, both live"""
    normals = np.asarray(normals, np.float64).reshape(-1, 3)
    n = normals.shape[0]
    nbr = np.asarray(nbr, np.int64).reshape(n, -1)
    stride = nbr.shape[1]
    live = np.isfinite(normals).all(1)
    length = np.clip(np.asarray(count, np.int64), 0, stride)
    v = np.repeat(np.arange(n, dtype=np.int64), stride).reshape(n, stride)
    used = np.arange(stride)[None, :] < length[:, None]
    inside = (nbr >= 0) & (nbr < n)
    j = np.where(inside, nbr, 0)
    ok = used & inside & (j != v) & live[v] & live[j]
    a, b = v[ok], j[ok]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    code = np.unique(lo * n + hi)
    lo, hi = code // max(n, 1), code % max(n, 1)
    with np.errstate(all="ignore"):
        dot = normals[lo, 0] * normals[hi, 0] + normals[lo, 1] * normals[hi, 1] + normals[lo, 2] * normals[hi, 2]
        w = 1.0 - np.abs(dot)
    return live, lo, hi, dot, w


def _votes(xyz, normals, flip, reference):
    """+1 toward, -1 away, 0 none per vertex, with the normals as oriented by ``flip``"""
    n = normals.shape[0]
    if reference is None:
        return np.zeros(n, np.int64)
    c = np.asarray(reference, np.float64)
    p = np.asarray(xyz, np.float32).reshape(n, 3).astype(np.float64)
    nn = np.where(flip[:, None], -normals, normals)
    with np.errstate(all="ignore"):
        t = (c[0] - p[:, 0]) * nn[:, 0] + (c[1] - p[:, 1]) * nn[:, 1] + (c[2] - p[:, 2]) * nn[:, 2]
    t = np.where(np.isfinite(normals).all(1) & np.isfinite(p).all(1), t, 0.0)
    return (t > 0).astype(np.int64) - (t < 0).astype(np.int64)


def _result(normals, live, flip, component, rounds=None):
    out = normals.copy()
    out[flip] = -out[flip]
    return {"flip": flip, "component": component.astype(np.int32), "normals": out, "n": int(normals.shape[0]),
            "n_components": int(np.unique(component).size), "n_flipped": int(flip.sum()), "n_not_live": int((~live).sum()), "rounds": rounds}


def kruskal_dfs(xyz, normals, nbr, count, reference=None):
    normals = np.asarray(normals, np.float64).reshape(-1, 3)
    n = normals.shape[0]
    live, lo, hi, dot, w = edges_from_lists(normals, nbr, count)
    order = np.lexsort((hi, lo, w))
    uf = list(range(n))

    def find(a):
        while uf[a] != a:
            uf[a] = uf[uf[a]]
            a = uf[a]
        return a
    tree = [[] for _ in range(n)]
    for e in order:
        a, b = find(int(lo[e])), find(int(hi[e]))
        if a != b:
            uf[a] = b
            neg = bool(dot[e] < 0)
            tree[int(lo[e])].append((int(hi[e]), neg))
            tree[int(hi[e])].append((int(lo[e]), neg))
    flip = np.zeros(n, bool)
    component = np.full(n, -1, np.int64)
    members_of = []
    for s in range(n):
        if component[s] >= 0:
            continue
        component[s] = s
        if not live[s]:
            continue
        stack, members = [s], []
        while stack:
            v = stack.pop()
            members.append(v)
            for j, neg in tree[v]:
                if component[j] < 0:
                    component[j] = s
                    flip[j] = flip[v] ^ neg
                    stack.append(j)
        members_of.append(np.array(members))
    vote = _votes(xyz, normals, flip, reference)
    for members in members_of:
        if (vote[members] < 0).sum() > (vote[members] > 0).sum():
            flip[members] ^= True
    return _result(normals, live, flip, component)


def boruvka(xyz, normals, nbr, count, reference=None):
    normals = np.asarray(normals, np.float64).reshape(-1, 3)
    n = normals.shape[0]
    live, lo, hi, dot, w = edges_from_lists(normals, nbr, count)
    m = lo.size
    order = np.lexsort((hi, lo, w))
    lo, hi, neg = lo[order], hi[order], dot[order] < 0                # edge e now has rank e in the total order
    root = np.arange(n)                                               # every vertex points at its component's root ...
    par = np.zeros(n, bool)                                           # ... with this parity relative to it
    rounds = 0
    while True:
        assert rounds < 32, "the forest still grows after 32 rounds"
        out = np.flatnonzero(root[lo] != root[hi])
        choice = np.full(n, m, np.int64)
        np.minimum.at(choice, root[lo[out]], out)
        np.minimum.at(choice, root[hi[out]], out)
        r = np.flatnonzero(choice < m)
        if r.size == 0:
            break
        e = choice[r]
        lo_in = root[lo[e]] == r
        x, y = np.where(lo_in, lo[e], hi[e]), np.where(lo_in, hi[e], lo[e])
        ry = root[y]
        stays = (choice[ry] == e) & (r < ry)                          # both took this edge: the lower root stays
        r, x, y, ry, e = r[~stays], x[~stays], y[~stays], ry[~stays], e[~stays]
        parent, ppar = np.arange(n), np.zeros(n, bool)
        parent[r] = ry
        ppar[r] = par[x] ^ par[y] ^ neg[e]
        for _ in range(40):                                           # pointer doubling over the old roots
            up = parent[parent]
            if (up == parent).all():
                break
            ppar = ppar ^ ppar[parent]
            parent = up
        else:
            raise AssertionError("a cycle among the hooks")
        par = par ^ ppar[root]
        root = parent[root]
        rounds += 1
    component = np.full(n, n, np.int64)
    np.minimum.at(component, root, np.arange(n))
    component = component[root]
    flip = par ^ par[component]
    vote = _votes(xyz, normals, flip, reference)
    toward = np.bincount(component, weights=vote > 0, minlength=n)
    away = np.bincount(component, weights=vote < 0, minlength=n)
    flip = flip ^ (away > toward)[component]
    flip &= live
    return _result(normals, live, flip, component, rounds)


# ---- the inputs ----------------------------------------------------------------------------------------------------------------
def knn_lists(xyz, k):
    """the k nearest of every point, itself included (the layout of gsr_hybrid_search: (n, k) int32 rows and their lengths)"""
    from scipy.spatial import cKDTree
    xyz = np.asarray(xyz, np.float64)
    k = min(k, xyz.shape[0])
    _, idx = cKDTree(xyz).query(xyz, k=k)
    idx = np.asarray(idx).reshape(xyz.shape[0], k)
    return idx.astype(np.int32), np.full(xyz.shape[0], k, np.int32)


def centroid(xyz):
    """as ``orient_normals_towards_centroid`` computes it: the float64 mean of the float32 points"""
    return np.asarray(xyz, np.float32).astype(np.float64).mean(0)


def _unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def torus_points(n, seed, R=1.0, r=0.35):
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], 1)
    out = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
    return p.astype(np.float32), out


def torus_case(n=2000, seed=11):
    rng = np.random.default_rng(seed + 1)
    xyz, outward = torus_points(n, seed)
    nrm = _unit(outward + 0.05 * rng.normal(size=(n, 3)))
    nrm[rng.random(n) < 0.5] *= -1.0
    nbr, cnt = knn_lists(xyz, 9)
    return {"xyz": xyz, "normals": nrm, "nbr": nbr, "count": cnt, "reference": centroid(xyz), "outward": outward}


def sheets_case(seed=5):
    rng = np.random.default_rng(seed)
    g = np.arange(40) * 0.1
    gx, gy = np.meshgrid(g, g, indexing="ij")
    flat = np.stack([gx.ravel(), gy.ravel()], 1)
    xyz = np.concatenate([np.c_[flat, np.zeros(1600)], np.c_[flat, np.full(1600, 5.0)], [[100.0, 100.0, 100.0]]]).astype(np.float32)
    n = xyz.shape[0]
    nrm = np.zeros((n, 3))
    nrm[:, 2] = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    nrm[[1600 + 17, 1600 + 803]] = np.nan                             # two dead rows, both in the upper sheet
    perm = rng.permutation(n)
    xyz, nrm = xyz[perm], nrm[perm]
    nbr, cnt = knn_lists(xyz, 7)                                      # the 6 nearest and the point itself
    sheet = np.where(xyz[:, 2] > 50, 1, (xyz[:, 2] > 2.5).astype(int))      # the far point attaches to the upper sheet
    return {"xyz": xyz, "normals": nrm, "nbr": nbr, "count": cnt, "reference": None, "sheet": sheet}


def chain_case(n=4096, seed=3):
    rng = np.random.default_rng(seed)
    step = 1e-3 + np.arange(n) / n                                    # strictly increasing turns, below a right angle
    angle = np.cumsum(step)
    nrm = np.stack([np.cos(angle), np.sin(angle), np.zeros(n)], 1)
    nrm[rng.random(n) < 0.5] *= -1.0
    xyz = np.c_[np.arange(n), np.zeros(n), np.zeros(n)].astype(np.float32)
    i = np.arange(n)
    nbr = np.stack([i, i - 1, i + 1], 1).astype(np.int32)
    nbr[0] = [0, 1, 0]
    nbr[-1] = [n - 1, n - 2, 0]
    cnt = np.full(n, 3, np.int32)
    cnt[[0, -1]] = 2
    return {"xyz": xyz, "normals": nrm, "nbr": nbr, "count": cnt, "reference": None}


def junk_case(n=500, stride=8, seed=9):
    rng = np.random.default_rng(seed)
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    nrm = _unit(rng.normal(size=(n, 3)))
    nrm[rng.choice(n, 7, replace=False), 1] = np.nan
    nbr = rng.integers(0, n, size=(n, stride))
    rows = np.arange(n)
    nbr[:, 0] = rows                                                  # self entries
    nbr[:, 3] = nbr[:, 2]                                             # duplicates
    what = rng.integers(0, 6, size=(n, stride))
    nbr = np.where(what == 0, -1, np.where(what == 1, n, np.where(what == 2, 2 ** 31 - 1, nbr))).astype(np.int32)
    cnt = rng.integers(0, stride + 1, size=n).astype(np.int32)
    cnt[rng.choice(n, 40, replace=False)] = 0
    return {"xyz": xyz, "normals": nrm, "nbr": nbr, "count": cnt, "reference": np.array([0.3, -0.1, 0.2])}


def tiny_cases():
    one = {"xyz": np.float32([[1, 2, 3]]), "normals": np.array([[0.0, 0.0, 1.0]]), "nbr": np.int32([[0]]), "count": np.int32([1]),
           "reference": np.array([1.0, 2.0, 0.0])}
    two = {"xyz": np.float32([[0, 0, 0], [1, 0, 0]]), "normals": np.array([[0.0, 0.0, -1.0], [0.0, 0.6, 0.8]]), "nbr": np.int32([[1], [1]]),
           "count": np.int32([1, 1]), "reference": None}
    three = {"xyz": np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0]]), "normals": np.array([[0.0, 0.0, 1.0], [np.nan, 0.0, 1.0], [0.0, 0.0, -1.0]]),
             "nbr": np.int32([[1, 2], [0, 2], [1, 0]]), "count": np.int32([2, 2, 2]), "reference": np.array([1.0, 0.0, 5.0])}
    return {"tiny1": one, "tiny2": two, "tiny3": three}


def sphere_case(n=1500, seed=21):
    rng = np.random.default_rng(seed)
    outward = _unit(rng.normal(size=(n, 3)))
    xyz = (outward * 1.5 + np.array([0.4, -0.3, 0.2])).astype(np.float32)
    nrm = _unit(outward + 0.05 * rng.normal(size=(n, 3)))
    nrm[rng.random(n) < 0.5] *= -1.0
    nbr, cnt = knn_lists(xyz, 9)
    return {"xyz": xyz, "normals": nrm, "nbr": nbr, "count": cnt, "reference": centroid(xyz), "outward": outward}


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> input dict (xyz float32, normals float64, nbr (n, stride) int32, count int32, reference or None).  Computed once and
    shared: treat the arrays as read-only."""
    cases = {"torus": torus_case(), "sheets": sheets_case(), "chain": chain_case(), "junk": junk_case(), "sphere": sphere_case()}
    cases.update(tiny_cases())
    for c in cases.values():
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return cases


@functools.lru_cache(maxsize=None)
def expected(name):
    """the Boruvka model's result of a case (the one that also has ``rounds``)"""
    c = gpu_cases()[name]
    return boruvka(c["xyz"], c["normals"], c["nbr"], c["count"], c["reference"])
