"""Float64 NumPy / SciPy restatement of the N-way overlap merge (``gsr_fuse_multi``, include/gsr_hip.h),
and the inputs the CPU and GPU tests share.  Nothing here touches the library.

Definition (validity, the three gates, J, the clamp and J32 are section 16's: ``fuse_model.prep``, ``_tr``, ``_quad``):

  global index   model-major: the rows of models[0] first, ascending
  J of a pair    the lower global index in the role of section 16's `a`, the higher in the role of `b`
  best[i][m]     for a valid row i and every model m != model(i): the gated candidate j of model m with the smallest (J32, j), or -1
  mutual edge    {i, j}, i < j, iff best[i][model(j)] = j and best[j][model(i)] = i; key (J32, i, j)
  rounds         every row starts as a component with the mask 1 << model; an edge is live while its ends are in different components
                 with disjoint masks; per round every component picks its smallest live edge, an edge picked by both its components
                 merges them (label = the lower label, masks OR-ed); until a round has no live edge.  An edge that dies between two
                 components whose masks intersect is a REJECTED edge; `rounds` counts the rounds that had a live edge.
  fusion         members i_1 < ... < i_k: W = sum w, m = (sum w m_i) / W, C = (sum w (C_i + (m_i - m)(m_i - m)^T)) / W, dc / sh / raw
                 opacity (sum w v_i) / W; sums in ascending member order in float64, narrowed to float32 once
  output         the rows in no group of >= 2 members in global order, then the fused rows ascending by lowest member

``fuse_multi`` also reports AMBIGUITY in section 16's sense: a gate within 1e-9 / 1e-6 relative of its threshold, a runner-up within
1e-6 relative of a best J on non-identical rows, or two live edges of one component whose J32 are equal -- or, for a component's
smallest live edge and its runner-up, whose J lie within 4e-7 relative (3 float32 ulps) of each other: the narrowing of two correct
float64 values could then order them either way.
"""
from __future__ import annotations

import functools

import numpy as np
from scipy.spatial import cKDTree

import fuse_model as F
from fuse_model import _quad, _tr, prep
from gaussiansplattingregistration_amd import synth

MAX_MODELS = 16
NAMES = F.NAMES


def _flat(a):
    a = np.asarray(a)
    return a.reshape(len(a), int(np.prod(a.shape[1:])))


def union_of(models):
    """-> (U: name -> (n_total, width) float32 over the arrays every non-empty model carries, model id per row, offsets)"""
    sizes = [len(m["xyz"]) for m in models]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    full = [m for m, n in zip(models, sizes) if n > 0] or models[:1]
    names = [k for k in NAMES if all(k in m for m in full)]
    U = {k: np.concatenate([_flat(np.asarray(m[k], np.float32)) for m in full]) for k in names}
    mid = np.repeat(np.arange(len(models)), sizes).astype(np.int64)
    return U, mid, off


def fuse_multi(models, max_distance, kld_max=0.5, color_delta=np.inf):
    """-> dict: the output arrays (float32, n_out rows; scaling / rot of fused rows NaN), group_of (n_total,), groups (list of member
    arrays, ascending by lowest member), `fused` (float64 rows before narrowing), the report fields and `ambiguous`."""
    N = len(models)
    assert 1 <= N <= MAX_MODELS
    U, mid, off = union_of(models)
    n = len(mid)
    r2 = float(max_distance) ** 2
    valid, w, inv = prep({"xyz": U["xyz"], "cov6": U["cov6"], "opacity": U["opacity"]})
    xyz, cov, dc = U["xyz"].astype(np.float64), U["cov6"].astype(np.float64), U["dc"].astype(np.float64)
    why = []                                                # what made the case ambiguous
    rows = np.flatnonzero(valid)
    ii = jj = np.zeros(0, np.int64)
    if len(rows) > 1:
        pr = cKDTree(xyz[rows]).query_pairs(float(max_distance) * (1 + 1e-6) + 1e-300, output_type="ndarray").astype(np.int64)
        a, b = rows[pr[:, 0]], rows[pr[:, 1]]
        ii, jj = np.minimum(a, b), np.maximum(a, b)
        k = mid[ii] != mid[jj]
        ii, jj = ii[k], jj[k]
    d = xyz[ii] - xyz[jj]                                   # a - b, a = the lower global index
    d2 = (d * d).sum(1)
    if (np.abs(d2 - r2) <= 1e-9 * r2).any():
        why.append("distance gate")
    k = d2 <= r2
    ii, jj, d = ii[k], jj[k], d[k]
    cn = np.sqrt(((dc[ii] - dc[jj]) ** 2).sum(1))
    if np.isfinite(color_delta):
        if (np.abs(cn - color_delta) <= 1e-9 * color_delta).any():
            why.append("colour gate")
    k = cn <= color_delta
    ii, jj, d = ii[k], jj[k], d[k]
    J = 0.25 * (_tr(inv[jj], cov[ii]) + _tr(inv[ii], cov[jj]) - 6.0 + _quad(inv[ii], d) + _quad(inv[jj], d))
    J = np.where(J < 0, 0.0, J)
    if (np.abs(J - kld_max) <= 1e-6 * kld_max).any():
        why.append("J gate")
    k = J <= kld_max
    ii, jj, J = ii[k], jj[k], J[k]
    J32 = J.astype(np.float32)
    gated = len(ii)
    # best[i][m]: both directions of every gated pair, grouped by the slot i * N + model(j)
    src, dst = np.concatenate([ii, jj]), np.concatenate([jj, ii])
    Jd, J32d = np.concatenate([J, J]), np.concatenate([J32, J32])
    best, amb = F._best(src * N + mid[dst], dst, Jd, J32d, n * N, U)
    if amb:
        why.append("runner-up of a best")
    best = best.reshape(n, N) if n else best.reshape(0, N)
    # mutual edges in ascending (i, j)
    si, sm = np.nonzero(best >= 0)
    sj = best[si, sm]
    k = (si < sj)
    si, sj = si[k], sj[k]
    k = best[sj, mid[si]] == si
    eu, ev = si[k].astype(np.int64), sj[k].astype(np.int64)
    code = ii * max(n, 1) + jj
    o = np.argsort(code)
    pos = o[np.searchsorted(code[o], eu * max(n, 1) + ev)] if len(eu) else np.zeros(0, np.int64)
    eJ, eJ32 = J[pos], J32[pos]
    E = len(eu)
    rank = np.empty(E, np.int64)
    rank[np.lexsort((ev, eu, eJ32))] = np.arange(E)         # the strict total order of the keys (J32, i, j)
    # rounds
    label = np.arange(n, dtype=np.int64)
    mask = (1 << mid).astype(np.int64)
    alive = np.ones(E, bool)
    rejected = rounds = 0
    while True:
        cu, cv = label[eu], label[ev]
        alive &= cu != cv
        clash = alive & ((mask[cu] & mask[cv]) != 0)
        rejected += int(clash.sum())
        alive &= ~clash
        if not alive.any():
            break
        rounds += 1
        le = np.flatnonzero(alive)
        comp, Jc, J32c = np.concatenate([cu[le], cv[le]]), np.concatenate([eJ[le], eJ[le]]), np.concatenate([eJ32[le], eJ32[le]])
        o = np.lexsort((Jc, comp))
        same = comp[o][1:] == comp[o][:-1]
        Js, J32s = Jc[o], J32c[o]
        first = np.r_[True, ~same]
        # any two with equal J32; and the component's smallest against its runner-up -- the comparison that decides the pick -- within
        # 3 float32 ulps (4e-7 relative): either J32 may land one ulp off in another correct float64 implementation
        if (same & ((J32s[1:] == J32s[:-1]) | (first[:-1] & (Js[1:] - Js[:-1] <= 4e-7 * Js[1:])))).any():
            why.append(f"two live edges of a component, round {rounds}")
        pick = np.full(n, E, np.int64)
        np.minimum.at(pick, cu[le], rank[le])
        np.minimum.at(pick, cv[le], rank[le])
        merge = le[(pick[cu[le]] == rank[le]) & (pick[cv[le]] == rank[le])]
        assert len(merge) > 0
        lo, hi = np.minimum(cu[merge], cv[merge]), np.maximum(cu[merge], cv[merge])
        assert len(np.unique(np.concatenate([lo, hi]))) == 2 * len(merge)      # a component merges at most once per round
        parent = np.arange(n, dtype=np.int64)
        parent[hi] = lo
        mask[lo] |= mask[hi]
        label = parent[label]
        alive[merge] = False
    # groups
    size = np.bincount(label, minlength=n) if n else np.zeros(0, np.int64)
    grouped = size[label] >= 2 if n else np.zeros(0, bool)
    roots = np.flatnonzero((size >= 2) & (label[:len(size)] == np.arange(len(size)))) if n else np.zeros(0, np.int64)
    ng = len(roots)
    rank_of = np.full(n, -1, np.int64)
    rank_of[roots] = np.arange(ng)
    n_copied = int(n - grouped.sum())
    group_of = np.where(grouped, n_copied + rank_of[label], -1).astype(np.int32) if n else np.zeros(0, np.int32)
    gr = np.flatnonzero(grouped)
    gr = gr[np.lexsort((gr, label[gr]))]                    # by group, members ascending
    grank = rank_of[label[gr]]
    first = np.r_[True, grank[1:] != grank[:-1]] if len(gr) else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(first, np.arange(len(gr)), 0)) if len(gr) else np.zeros(0, np.int64)
    posn = np.arange(len(gr)) - start                       # the member's position in its group
    groups = np.split(gr, np.flatnonzero(first)[1:]) if ng else []
    kmax = int(posn.max()) + 1 if len(gr) else 0

    def wsum(vals):                                         # sum over the members in ascending order, one position at a time
        acc = np.zeros((ng,) + vals.shape[1:])
        for p in range(kmax):
            k = posn == p
            acc[grank[k]] += vals[gr[k]]
        return acc
    err = np.errstate(all="ignore")                         # (rows that are in no group may hold NaN or inf)
    err.__enter__()
    W = wsum(w[:, None])
    fused = {}
    mu = wsum(w[:, None] * xyz) / W
    fused["xyz"] = mu
    dm = xyz - (mu[rank_of[label]] if ng else np.zeros((n, 3)))        # (rows in no group: unused)
    r, c = [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]
    fused["cov6"] = wsum(w[:, None] * (cov + dm[:, r] * dm[:, c])) / W
    for name in ("dc", "sh", "opacity"):
        if name in U and U[name].shape[1] > 0:
            fused[name] = wsum(w[:, None] * U[name].astype(np.float64)) / W
    err.__exit__(None, None, None)
    out = {}
    for name in U:
        if name in ("scaling", "rot"):
            fused[name] = np.full((ng, U[name].shape[1]), np.nan)
        f = fused[name].astype(np.float32) if name in fused else np.zeros((ng, 0), np.float32)
        out[name] = np.concatenate([U[name][~grouped], f])
    hist = np.bincount(size[roots], minlength=MAX_MODELS + 1) if ng else np.zeros(MAX_MODELS + 1, np.int64)
    out.update(group_of=group_of, groups=groups, fused=fused, n_out=n_copied + ng, n_groups=ng, n_grouped_rows=int(grouped.sum()),
               n_invalid=int((~valid).sum()), gated_pairs=gated, mutual_edges=E, rejected_edges=rejected, rounds=rounds,
               groups_of_size=[int(x) for x in hist], ambiguous=bool(why), why=why, n_copied=n_copied, w=w, model_id=mid, offsets=off,
               edges=np.stack([eu, ev], 1) if E else np.zeros((0, 2), np.int64), edge_J=eJ, labels=label)
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

GATES = F.BASE_GATES[0]


def _cloud(n, seed, h, sh_degree):
    if n == 0:
        return F._empty_like(F.model_of(synth.make_cloud(1, seed=seed, h=h, sh_degree=sh_degree)))
    return F.model_of(synth.make_cloud(n, seed=seed, h=h, sh_degree=sh_degree))


def make_models(sizes, sh_degree=3, seed=0):
    """models[0] = a synth cloud; every other model its own cloud in the same box with a random half of the rows it shares with
    models[0] overwritten by noisy copies of them (``fuse_model.plant``): a row of models[0] has copies in about half of the models"""
    h = synth.half_extent(max(max(sizes), 1))
    models = [_cloud(sizes[0], 100 + seed, h, sh_degree)]
    for m in range(1, len(sizes)):
        B = _cloud(sizes[m], 100 + seed + 7 * m, h, sh_degree)
        if sizes[m] and sizes[0]:
            F.plant(models[0], B, np.random.default_rng(2000 + seed + m))
        models.append(B)
    return models


def conflict_chain():
    """Rows a1 - b1 - c1 - a2 on a line, models A = {a1, a2}, B = {b1}, C = {c1}, global indices a1 = 0, a2 = 1, b1 = 2, c1 = 3.  With
    one isotropic covariance (sigma 0.01) J = 5000 d^2; the spacings 0.010, 0.012, 0.011 make c1's best in A a2 (0.011 < 0.022) and
    b1's best in A a1, so the mutual edges are a1-b1 (J 0.5), c1-a2 (0.605) and b1-c1 (0.72).  Round 1: a1 and b1 both pick a1-b1,
    c1 and a2 both pick c1-a2: two merges.  Round 2: b1-c1 joins {a1, b1} and {a2, c1}, which both hold a row of A: rejected."""
    cov = np.float32([1e-4, 0, 0, 1e-4, 0, 1e-4])

    def rows(xs):
        n = len(xs)
        return {"xyz": np.stack([np.float32(xs), np.zeros(n, np.float32), np.zeros(n, np.float32)], 1), "cov6": np.tile(cov, (n, 1)),
                "dc": np.zeros((n, 3), np.float32), "sh": np.zeros((n, 0), np.float32), "opacity": np.zeros(n, np.float32)}
    A, B, C = rows([0.0, 0.033]), rows([0.010]), rows([0.022])
    return [A, B, C], (0.05, 50.0, np.inf)


def make_case(name):
    """-> (models, (max_distance, kld_max, color_delta)) of the named case; the same bytes for the CPU and the GPU tests"""
    if name.startswith("grid_"):                            # grid_<N>_<rows>_<K>
        _, N, rows, K = name.split("_")
        total = int(N) * int(rows)                          # the radius shrinks with the density: about as many neighbours as 2 x 2000 rows have
        r = round(GATES[0] * min(1.0, (4000.0 / max(total, 1)) ** (1.0 / 3.0)), 3)
        return make_models([int(rows)] * int(N), sh_degree={"0": 0, "15": 3}[K], seed=int(N)), (r,) + GATES[1:]
    if name == "one_empty":
        return make_models([300, 0, 257, 300], sh_degree=1, seed=40), GATES
    if name == "unequal":
        return make_models([3000, 65, 1], sh_degree=1, seed=41), GATES
    if name == "invalid":
        models = make_models([500, 500, 500], sh_degree=0, seed=42)
        for m, M in enumerate(models):
            M["cov6"][3 + m] = 0.0                                       # zero determinant
            M["cov6"][40 + m] = np.float32([1, 0, 0, 1, 0, -1])           # negative determinant
            M["xyz"][77 + m, 1] = np.nan
            M["opacity"][130 + m] = -np.inf
        return models, GATES
    if name == "one_cell":                                  # every centre inside a ball of diameter < r: one cell, long spans
        models = make_models([400, 400, 400], sh_degree=0, seed=43)
        rng = np.random.default_rng(44)
        r = 0.25
        for M in models:
            v = rng.normal(size=(400, 3))
            v *= (0.5 * r * rng.random(400) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
            M["xyz"] = v.astype(np.float32)
        for m in (1, 2):
            F.plant(models[0], models[m], np.random.default_rng(45 + m))
            nrm = np.linalg.norm(models[m]["xyz"].astype(np.float64), axis=1)
            models[m]["xyz"] = (models[m]["xyz"] * np.minimum(1.0, 0.499 * r / nrm)[:, None]).astype(np.float32)
        return models, (r, 0.5, np.inf)
    if name == "outliers":
        models = make_models([500, 500, 500], sh_degree=0, seed=46)
        h = synth.half_extent(500)
        rng = np.random.default_rng(47)
        for m, M in enumerate(models):
            rows_ = [1 + m, 100, 250 + m, 333, 498 - m]
            M["xyz"][rows_] = (500.0 * 2.0 * h * rng.choice([-1.0, 1.0], (5, 3)) * rng.uniform(0.5, 1.0, (5, 3))).astype(np.float32)
        return models, GATES
    if name == "plain3":                                    # the comparison of the outliers case: four times the rows
        return make_models([2000, 2000, 2000], sh_degree=0, seed=48), GATES
    if name == "chain":
        return conflict_chain()
    if name == "scaling_rot":
        models = make_models([500, 500, 500], sh_degree=1, seed=49)
        F.add_scaling_rot(models[0], 50)
        for m in (1, 2):
            F.add_scaling_rot(models[m], 50 + m)
            F.plant(models[0], models[m], np.random.default_rng(60 + m))
        return models, GATES
    if name == "large":                                     # more rows than one pass of every launch (2048 x 256 threads)
        return make_models([300000, 300000], sh_degree=0, seed=70), (0.06, 0.5, np.inf)
    if name.startswith("pair_"):                            # the cases of fuse_model, as two models
        A, B, gates = F.make_case(name[5:])
        return [A, B], gates
    raise KeyError(name)


GRID_N, GRID_ROWS, GRID_K = (1, 2, 3, 5, 16), (0, 1, 63, 64, 65, 257, 3000), (0, 15)
GRID_CASES = tuple(f"grid_{N}_{rows}_{K}" for N in GRID_N for rows in GRID_ROWS for K in GRID_K)
SPECIAL_CASES = ("one_empty", "unequal", "invalid", "one_cell", "outliers", "plain3", "chain", "scaling_rot", "large")
GPU_CASES = GRID_CASES + SPECIAL_CASES


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (models, gates, the model's result) of the named case, computed once per process and shared: treat it as read-only"""
    models, gates = make_case(name)
    return models, gates, fuse_multi(models, *gates)
