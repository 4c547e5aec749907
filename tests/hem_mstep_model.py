"""An independent float64 model of ONE ``createClusterLevel`` and the hand-built levels that put chosen parents on the switch points of
the HEM kernels (test infrastructure: tests/test_hem_mstep_cpu.py checks the model, tests/test_hem_mstep_gpu.py judges the kernels by it).

``level`` restates the semantics of the reference's level (the oracle's ``run_level`` steps 1-6 and 8, oracle/hem_oracle.cpp, are the
readable statement of them; the moment sums are those of the reference's mixture.cpp:209-238) in NumPy float64 on the float32 inputs:
pairs by brute force over parents x components (no grid), gates as comparisons of float64 values, sums in float64.  Two decisions of the
reference are decisions of EXACT float32 values and are taken in ``np.float32`` here too: the clamp of the likelihood followed by the
product with the parent's weight (``float32(weight) * float32(clamp(L))``, gradual underflow included) and the ``sumLw == 0`` test.
Beside every output element the model returns its magnitude ``mag``: the same expression with every term replaced by its absolute
value -- what an error of one float32 rounding per term is proportional to -- and the smallest relative margin of every decision it
took, so that a test can require the decisions to be unambiguous in float32.

Nothing here imports the package or its kernels.
"""
from __future__ import annotations

import functools
import json
import os
import zlib

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
CLAMP_HI = 1e8
EPS32 = 2.0 ** -24
FIELDS = ("xyz", "color", "cov6", "opacity", "weight", "sh")
TOLERANCE_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hem_mstep_tolerance.json")
MARGIN = 4.0            # the project's margin for another summation order, contracted multiply-adds and the device expf (test_raster_gpu.py)

_IJ = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # cov6: xx xy xz yy yz zz


def _full(c6):
    c6 = np.asarray(c6, np.float64)
    m = np.empty(c6.shape[:-1] + (3, 3))
    for k, (i, j) in enumerate(_IJ):
        m[..., i, j] = m[..., j, i] = c6[..., k]
    return m


def _det_terms(c6):
    """The five products of the symmetric 3x3 determinant (their sum is det)."""
    xx, xy, xz, yy, yz, zz = (np.asarray(c6, np.float64)[..., k] for k in range(6))
    return np.stack([-xz * xz * yy, 2 * xy * xz * yz, -xx * yz * yz, -xy * xy * zz, xx * yy * zz], -1)


def det6(c6):
    return _det_terms(c6).sum(-1)


# ====================================================================================================================== the model
def level(cloud, parent_mask, weight, rho, delta, kappa, tau, mutation=None):
    """One level.  ``cloud``: float32 ``xyz color cov6 opacity sh``; ``parent_mask`` (n,) bool; ``weight`` (n,) float32.  ``rho`` only
    draws the next level's parent flags in the reference and decides nothing here.

    ``mutation`` (tests of the checks' teeth only): ``{"drop_last_pair_of": input row of a parent}``, ``{"unit_weight_child": row}``,
    ``{"sumlw_skip": (child row, parent row)}`` or ``{"no_dm": True}`` -- each a way a kernel could be subtly wrong.

    Returns a dict: the output arrays (float64, parents in parent input order, then orphans in input order, validity erase applied),
    ``mag`` (same keys), ``n_parent_rows`` (surviving parent rows, at the front), ``parent_in`` / ``orphan_in`` (input rows of the output
    rows), ``pairs_of`` (pair count per parent, parent input order), ``stats`` and ``margins``."""
    mutation = mutation or {}
    f64 = np.float64
    xyz, col, op = (np.asarray(cloud[k], np.float32).astype(f64) for k in ("xyz", "color", "opacity"))
    c6 = np.asarray(cloud["cov6"], np.float32).astype(f64)
    sh = np.asarray(cloud["sh"], np.float32).astype(f64).reshape(xyz.shape[0], -1)
    w32 = np.asarray(weight, np.float32)
    wgt = w32.astype(f64)
    mask = np.asarray(parent_mask).astype(bool)
    delta, kappa, tau = (float(np.float32(v)) for v in (delta, kappa, tau))
    n, F = xyz.shape[0], sh.shape[1]
    C = _full(c6)
    detc = det6(c6)
    thr_c, thr_k = kappa * kappa / 2, delta * delta / 2
    parents = np.nonzero(mask)[0]
    mg = {"radius": np.inf, "color": np.inf, "kl": np.inf, "clamp_lo": np.inf, "clamp_hi": np.inf, "det": np.inf}

    # ---- gates and pairs, brute force
    p_slot, p_child, p_wl = [], [], []
    with np.errstate(all="ignore"):
        for k, s in enumerate(parents):
            R = delta * np.sqrt(np.linalg.eigvalsh(C[s])[-1])
            d = xyz - xyz[s]
            d2 = (d * d).sum(1)
            mg["radius"] = min(mg["radius"], float(np.min(np.abs(np.sqrt(d2) - R) / R)))
            cand = np.nonzero(d2 < R * R)[0]
            dc = np.sqrt(((col[cand] - col[s]) ** 2).sum(1))
            if cand.size:
                mg["color"] = min(mg["color"], float(np.min(np.abs(dc - thr_c) / thr_c)))
            keep = ~(dc > thr_c)
            cand, dc = cand[keep], dc[keep]
            Pinv = np.linalg.inv(C[s])
            dd = d[cand]
            smd = np.einsum("ni,ij,nj->n", dd, Pinv, dd)
            tr = np.einsum("ij,nji->n", Pinv, C[cand])
            kld = 0.5 * (smd + tr - 3.0 - np.log(detc[cand] / detc[s]))
            if cand.size:
                mg["kl"] = min(mg["kl"], float(np.nanmin(np.abs(kld - thr_k) / thr_k)))
            keep = ~(kld > thr_k) & ~(mask[cand] & (cand != s))          # a parent is nobody else's child
            cand, dc = cand[keep], dc[keep]
            L = np.exp(-d2[cand] / (tau * tau)) * op[cand] * np.exp(-dc * dc / (tau * tau)) * np.sqrt(detc[cand])
            if cand.size:
                mg["clamp_lo"] = min(mg["clamp_lo"], float(np.min(np.abs(L - FLT_MIN) / FLT_MIN)))
                mg["clamp_hi"] = min(mg["clamp_hi"], float(np.min(np.abs(L - CLAMP_HI) / CLAMP_HI)))
            Lc = np.maximum(FLT_MIN, np.minimum(L, CLAMP_HI))
            wl = w32[s] * Lc.astype(np.float32)                          # float32 x float32, in float32: an exact decision of the reference
            assert wl.dtype == np.float32
            p_slot.append(np.full(cand.size, k, np.int64))
            p_child.append(cand)
            p_wl.append(wl)
    slot = np.concatenate(p_slot) if p_slot else np.zeros(0, np.int64)
    child = np.concatenate(p_child) if p_child else np.zeros(0, np.int64)
    wl32 = np.concatenate(p_wl) if p_wl else np.zeros(0, np.float32)
    pairs_of = np.bincount(slot, minlength=parents.size).astype(np.int64)

    # ---- per-child sums: float32 for the decision, float64 for the arithmetic
    in_sum = np.ones(slot.size, bool)
    if "sumlw_skip" in mutation:
        ci, pi = mutation["sumlw_skip"]
        hit = (child == ci) & (parents[slot] == pi)
        assert hit.sum() == 1
        in_sum &= ~hit
    sum32 = np.zeros(n, np.float32)
    np.add.at(sum32, child[in_sum], wl32[in_sum])
    sum64 = np.bincount(child[in_sum], weights=wl32[in_sum].astype(f64), minlength=n)
    orphan = sum32 == np.float32(0)
    live = ~orphan[child]
    wchild = wgt.copy()
    if "unit_weight_child" in mutation:
        wchild[mutation["unit_weight_child"]] = 1.0
    with np.errstate(all="ignore"):
        w = np.where(live, wl32.astype(f64) / sum64[child], 0.0) * wchild[child]
    if "drop_last_pair_of" in mutation:
        k = int(np.nonzero(parents == mutation["drop_last_pair_of"])[0][0])
        w[np.nonzero(slot == k)[0][-1]] = 0.0

    # ---- moment matching, parent by parent
    P = parents.size
    out = {"xyz": np.zeros((P, 3)), "color": np.zeros((P, 3)), "cov6": np.zeros((P, 6)), "opacity": np.zeros(P), "weight": np.zeros(P),
           "sh": np.zeros((P, F))}
    mag = {k: np.zeros_like(v) for k, v in out.items()}
    start = np.concatenate([[0], np.cumsum(pairs_of)])
    with np.errstate(all="ignore"):
        for k, s in enumerate(parents):
            sl = slice(start[k], start[k + 1])
            i, wk = child[sl], w[sl][:, None]
            ws = wk.sum()
            d = xyz[i] - xyz[s]
            dd6 = np.stack([d[:, a] * d[:, b] for a, b in _IJ], 1)
            mean = (xyz[i] * wk).sum(0) / ws
            dm = mean - xyz[s]
            dm6 = np.array([dm[a] * dm[b] for a, b in _IJ])
            if mutation.get("no_dm"):
                dm6 = dm6 * 0.0
            out["weight"][k], mag["weight"][k] = ws, ws
            out["xyz"][k], mag["xyz"][k] = mean, (np.abs(xyz[i]) * wk).sum(0) / ws
            out["color"][k], mag["color"][k] = (col[i] * wk).sum(0) / ws, (np.abs(col[i]) * wk).sum(0) / ws
            out["cov6"][k] = ((c6[i] + dd6) * wk).sum(0) / ws - dm6
            mag["cov6"][k] = (np.abs(c6[i] + dd6) * wk).sum(0) / ws + np.abs(dm6)
            out["opacity"][k], mag["opacity"][k] = (op[i] * wk[:, 0]).sum() / ws, (np.abs(op[i]) * wk[:, 0]).sum() / ws
            if F:
                out["sh"][k], mag["sh"][k] = (sh[i] * wk).sum(0) / ws, (np.abs(sh[i]) * wk).sum(0) / ws

        # ---- orphans behind the parents, then the validity erase
        orph = np.nonzero(orphan)[0]
        dets = det6(out["cov6"])
        ok_p = ~(np.isnan(out["xyz"]).any(1) | np.isnan(dets) | (dets <= 0))
        dm_p = dets / np.abs(_det_terms(out["cov6"])).sum(-1)
        do = det6(c6[orph])
        ok_o = ~(np.isnan(xyz[orph]).any(1) | np.isnan(do) | (do <= 0))
    if ok_p.any():
        mg["det"] = float(np.min(dm_p[ok_p]))
    res = {}
    src = {"xyz": xyz, "color": col, "cov6": c6, "opacity": op, "weight": wgt, "sh": sh}
    for f in FIELDS:
        res[f] = np.concatenate([out[f][ok_p], src[f][orph][ok_o]])
    res["mag"] = {f: np.concatenate([mag[f][ok_p], np.abs(src[f][orph][ok_o])]) for f in FIELDS}
    res["n_parent_rows"] = int(ok_p.sum())
    res["parent_in"] = parents[ok_p]
    res["orphan_in"] = orph[ok_o]
    res["pairs_of"] = pairs_of
    res["det_margin_of"] = dm_p                       # per parent, parent input order (NaN for a non-finite row)
    res["stats"] = {"parents": int(P), "pairs": int(slot.size), "orphans": int(orph.size), "dropped": int((~ok_p).sum() + (~ok_o).sum()),
                    "n_out": int(ok_p.sum() + ok_o.sum()), "max_pairs_of_a_parent": int(pairs_of.max()) if P else 0}
    res["margins"] = mg
    return res


# ====================================================================================================================== the cases
# Every case is built the same way: clusters on a cubic lattice, at least 20 radii of the largest parent apart; one or more hand-flagged
# parents per cluster; children drawn around them well inside the gates (Mahalanobis offset at most 1/3, covariance eigenvalues within a
# factor 2 of the cluster's, random rotations), colours / opacities / weights in [0.25, 4] / SH rows differing per child; the rows
# shuffled, so that input order, processing order (the kernels' is spatial) and output order all differ.
DEFAULT = {"rho": 3.0, "delta": 3.0, "kappa": 2.5, "tau": 1.0}
LADDER_PAIRS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 257)
HEAVY_PAIRS = (2047, 2048, 2049, 4097, 8200, 3, 9, 16)
# The selection calls a parent heavy, and cuts it into work items of 8192 candidates, when it scans more than 16 x the level's mean:
# with eight parents none can.  40 more parents of 2 .. 6 pairs bring the mean down to about 390 candidates, so the 8200-pair parent
# (and no other) is heavy and its candidates exceed one work item.
HEAVY_FILL = tuple(2 + k % 5 for k in range(40))
SHARED = ((2, 1), (2, 40), (3, 16), (7, 5), (8, 9), (9, 9), (64, 3), (65, 3), (300, 2))          # (parents, children) per cluster
ORPHAN_BLOCKS = (0, 1, 4, 5, 64, 0)              # orphans per 64-row input block; a partial block with the last row an orphan follows
CASES = ("ladder", "heavy", "shared", "orphans", "last_row_child", "clamps", "zero_weight_parent")
WIDTHS = (0, 9, 24, 45)
WIDE = (1, 47, 72, 105, 193, 256)                # 1 / 2 / 4 / 8 / 16 / 32 lanes per row, no multiple of 4, the unpacked fold, the largest width
WIDE_CASES = ("ladder", "heavy")
ANISO = np.array([1.0, 0.8, 0.6])


def widths(name):
    return WIDTHS + (WIDE if name in WIDE_CASES else ())


def _rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _cov6(q, lam):
    m = (q * lam) @ q.T
    return np.array([m[i, j] for i, j in _IJ])


def _sites(rng, k, spacing):
    """k lattice sites of a cube around the origin, in random order."""
    m = 1
    while m ** 3 < k:
        m += 1
    g = np.stack(np.meshgrid(*[np.arange(m) - (m - 1) / 2] * 3, indexing="ij"), -1).reshape(-1, 3) * spacing
    return g[rng.permutation(len(g))[:k]]


class _Rows:
    def __init__(self):
        self.f = {k: [] for k in ("xyz", "color", "cov6", "opacity", "weight", "parent", "tag", "cluster")}

    def add(self, xyz, color, cov6, opacity, weight, parent, tag, cluster):
        for k, v in zip(self.f, (xyz, color, cov6, opacity, weight, parent, tag, cluster)):
            self.f[k].append(v)
        return len(self.f["tag"]) - 1

    def finish(self, perm, params, **info):
        a = {k: np.asarray(v) for k, v in self.f.items()}
        c = {"xyz": a["xyz"][perm].astype(np.float32), "color": a["color"][perm].astype(np.float32), "cov6": a["cov6"][perm].astype(np.float32),
             "opacity": a["opacity"][perm].astype(np.float32), "weight": a["weight"][perm].astype(np.float32),
             "mask": a["parent"][perm].astype(np.uint8), "tag": a["tag"][perm], "cluster": a["cluster"][perm], "params": dict(params)}
        c.update(info)
        return c


def _cluster(rows, rng, cid, centre, n_par, n_child, s=1.0, lam=None, child_r=(0.0, 1.0 / 3), child_f=(0.5, 2.0), par_weights=None,
             color_spread=0.05, op_range=(0.3, 0.95), tag="child", rot=None):
    """One cluster: ``n_par`` parents and ``n_child`` children every parent takes.  Returns the builder rows of the parents."""
    lam = s * s * ANISO if lam is None else np.asarray(lam, np.float64)
    qb = _rot(rng) if rot is None else rot
    A = qb * np.sqrt(lam)
    base_col = rng.uniform(0.2, 0.8, 3)
    jitter = 0.05 if n_par > 1 else 0.0
    r_hi = child_r[1] - jitter
    par = []
    for k in range(n_par):
        u = rng.normal(size=3)
        u *= jitter * rng.uniform(0.2, 1.0) / np.linalg.norm(u)
        cov = _cov6(qb, lam) if n_par == 1 else _cov6(_rot(rng), lam * rng.uniform(0.8, 1.25, 3))
        wt = np.exp(rng.uniform(np.log(0.25), np.log(4.0))) if par_weights is None else par_weights[k]
        par.append(rows.add(centre + A @ u, base_col + rng.uniform(-color_spread, color_spread, 3), cov, rng.uniform(*op_range), wt, 1,
                            "parent", cid))
    for _ in range(n_child):
        u = rng.normal(size=3)
        u *= rng.uniform(child_r[0], r_hi) / np.linalg.norm(u)
        rows.add(centre + A @ u, base_col + rng.uniform(-color_spread, color_spread, 3), _cov6(_rot(rng), lam * rng.uniform(*child_f, 3)),
                 rng.uniform(*op_range), np.exp(rng.uniform(np.log(0.25), np.log(4.0))), 0, tag, cid)
    return par


def _simple(seed, specs, params=DEFAULT, spacing=100.0, last_tag=None):
    """Clusters of (parents, children) with s in [0.75, 1.5] (radius at most 4.5: 20 radii = 90 < spacing)."""
    rng = np.random.default_rng(seed)
    rows = _Rows()
    sites = _sites(rng, len(specs), spacing)
    for cid, ((n_par, n_child), centre) in enumerate(zip(specs, sites)):
        _cluster(rows, rng, cid, centre, n_par, n_child, s=rng.uniform(0.75, 1.5), tag=f"child{cid}")
    n = len(rows.f["tag"])
    perm = rng.permutation(n)
    if last_tag is not None:                   # the array's last row: a row of that tag
        j = next(k for k in range(n) if rows.f["tag"][perm[k]] == last_tag)
        perm[[j, n - 1]] = perm[[n - 1, j]]
    return rows.finish(perm, params, specs=tuple(specs))


def _ladder():
    return _simple(101, [(1, p - 1) for p in LADDER_PAIRS])


def _heavy():
    return _simple(102, [(1, p - 1) for p in HEAVY_PAIRS + HEAVY_FILL])


def _shared():
    return _simple(103, list(SHARED))


def _last_row_child():
    return _simple(105, [(1, 39), (1, 20), (2, 7), (1, 0)], last_tag="child0")


def _orphans():
    """Parents of 8 .. 16 pairs (the small-parent path and the per-pair expression chain alone), run at kappa = 1 (colour gate 0.5), and
    three kinds of orphans: out of every radius, inside a radius but 1.0 away in colour, inside a radius but with a covariance 1e-3 of
    the parent's (KL about 9 > 4.5) -- placed in input order as ORPHAN_BLOCKS says, the array's last row among them."""
    rng = np.random.default_rng(104)
    params = dict(DEFAULT, kappa=1.0)
    n_orph = sum(ORPHAN_BLOCKS) + 3                     # the partial last block: 10 rows, 3 orphans, the last row one of them
    n_rows = 64 * len(ORPHAN_BLOCKS) + 10
    sizes, left = [], n_rows - n_orph
    while left > 0:
        p = min(left, 8 + len(sizes) % 9)               # pair counts 8 .. 16
        sizes.append(p)
        left -= p
    rows = _Rows()
    sites = _sites(rng, len(sizes) + 4, 100.0)
    info = []
    for cid, p in enumerate(sizes):
        s = rng.uniform(0.75, 1.5)
        par = _cluster(rows, rng, cid, sites[cid], 1, p - 1, s=s)
        info.append((par[0], s))
    for k in range(n_orph):
        kind = k % 3
        if kind == 0:                                   # out of every radius: around an empty lattice site
            c = sites[len(sizes) + k % 4] + rng.uniform(-5, 5, 3)
            rows.add(c, rng.uniform(0.2, 0.8, 3), _cov6(_rot(rng), ANISO * rng.uniform(0.5, 2.0, 3)), rng.uniform(0.3, 0.95),
                     np.exp(rng.uniform(np.log(0.25), np.log(4.0))), 0, "orphan_far", -1)
            continue
        pr, s = info[rng.integers(len(info))]
        pc, pcol, pcov = (np.asarray(rows.f[f][pr]) for f in ("xyz", "color", "cov6"))
        u = rng.normal(size=3)
        u *= 0.3 * s * np.sqrt(0.6) * rng.uniform(0.2, 1.0) / np.linalg.norm(u)
        if kind == 1:
            colr, cov, tag = pcol + np.eye(3)[rng.integers(3)] * rng.choice([-1.0, 1.0]), _cov6(_rot(rng), s * s * ANISO * rng.uniform(0.5, 2.0, 3)), "orphan_color"
        else:
            colr, cov, tag = pcol + rng.uniform(-0.05, 0.05, 3), pcov * 1e-3, "orphan_kl"
        rows.add(pc + u, colr, cov, rng.uniform(0.3, 0.95), np.exp(rng.uniform(np.log(0.25), np.log(4.0))), 0, tag, -1)
    tags = np.asarray(rows.f["tag"])
    is_o = np.char.startswith(tags, "orphan")
    o_rows, c_rows = rng.permutation(np.nonzero(is_o)[0]), rng.permutation(np.nonzero(~is_o)[0])
    slot_is_orphan = np.zeros(n_rows, bool)
    for b, k in enumerate(ORPHAN_BLOCKS):
        slot_is_orphan[64 * b + rng.permutation(64)[:k]] = True
    tail = 64 * len(ORPHAN_BLOCKS)
    slot_is_orphan[[tail + 2, tail + 5, n_rows - 1]] = True
    perm = np.empty(n_rows, np.int64)
    perm[slot_is_orphan], perm[~slot_is_orphan] = o_rows, c_rows
    return rows.finish(perm, params, specs=tuple((1, p - 1) for p in sizes), orphan_slots=np.nonzero(slot_is_orphan)[0])


def _clamps():
    """tau = 0.1.  G1: a giant parent (sigma 10, weight 1) whose children lie 1.5 .. 3.3 away: exp(-d^2 / tau^2) < 1e-97, the likelihood
    clamps to FLT_MIN.  G2: two such parents of weights 0.25 and 0.75 sharing their children: wL = 0.25 FLT_MIN is subnormal, the
    responsibilities are 0.25 and 0.75.  G3: cov = 1e6 I (children 1e6 .. 2e6, offsets <= 0.03, opacity >= 0.5): the likelihood is
    >= 4e8 and clamps to 1e8.  G4: an ordinary cluster, unclamped.  G3's radius is 3000, so it sits 1e5 away from the others, which
    are 20 of their own radii (30) apart."""
    rng = np.random.default_rng(106)
    params = dict(DEFAULT, tau=0.1)
    rows = _Rows()
    lam10 = 100.0 * ANISO
    _cluster(rows, rng, 0, np.array([0.0, 0.0, 0.0]), 1, 30, lam=lam10, child_r=(0.2, 1.0 / 3), par_weights=[1.0], tag="lo1")
    _cluster(rows, rng, 1, np.array([700.0, 0.0, 0.0]), 2, 20, lam=lam10, child_r=(0.2, 1.0 / 3 + 0.03), par_weights=[0.25, 0.75], tag="lo2")
    _cluster(rows, rng, 2, np.array([1e5, 0.0, 0.0]), 1, 25, lam=1e6 * np.ones(3), child_r=(0.0, 3e-5), child_f=(1.0, 2.0), color_spread=0.01,
             op_range=(0.5, 0.95), par_weights=[2.0], tag="hi", rot=np.eye(3))
    _cluster(rows, rng, 3, np.array([0.0, 700.0, 0.0]), 1, 12, s=1.0, tag="plain")
    n = len(rows.f["tag"])
    return rows.finish(rng.permutation(n), params, specs=((1, 30), (2, 20), (1, 25), (1, 12)))


def _zero_weight_parent():
    """Isotropic unit covariances.  Z (weight 0) at the origin with two children of its own on the side away from O; O (an ordinary
    parent) 4 away (each other's radius is 3) with five children of its own on its far side; one child halfway (2 from each: inside both
    radii, KL = 2 < 4.5 to both).  A third, ordinary cluster far away.  By the reference's rules Z's wL are all 0: Z and its own
    children have sumLw == 0 and leave as orphans, Z's merged row is 0 / 0 and is erased, the shared child goes wholly to O."""
    rng = np.random.default_rng(107)
    rows = _Rows()
    eye = np.array([1.0, 0, 0, 1.0, 0, 1.0])

    def row(p, parent, wt, tag):
        return rows.add(np.asarray(p, np.float64), 0.5 + rng.uniform(-0.05, 0.05, 3), eye * rng.uniform(0.8, 1.25), rng.uniform(0.3, 0.95), wt, parent, tag, 0)

    wt = lambda: np.exp(rng.uniform(np.log(0.25), np.log(4.0)))
    z = row([0, 0, 0], 1, 0.0, "Z")
    row([-0.3, 0.2, 0.1], 0, wt(), "z_child")
    row([-0.25, -0.2, -0.1], 0, wt(), "z_child")
    o = row([4, 0, 0], 1, wt(), "O")
    for _ in range(5):
        row([4.3, 0, 0] + rng.uniform(-0.2, 0.2, 3), 0, wt(), "o_child")
    sc = row([2, 0.05, -0.05], 0, wt(), "shared")
    _cluster(rows, rng, 1, np.array([100.0, 0.0, 0.0]), 1, 9, s=1.0)
    n = len(rows.f["tag"])
    perm = rng.permutation(n)
    inv = np.argsort(perm)
    return rows.finish(perm, DEFAULT, specs=(), Z=int(inv[z]), O=int(inv[o]), shared=int(inv[sc]))


_BUILD = {"ladder": _ladder, "heavy": _heavy, "shared": _shared, "orphans": _orphans, "last_row_child": _last_row_child, "clamps": _clamps,
          "zero_weight_parent": _zero_weight_parent}


@functools.lru_cache(maxsize=None)
def case(name):
    """The level without its SH rows: float32 ``xyz color cov6 opacity weight``, ``mask``, ``params``, ``tag`` / ``cluster`` per row."""
    return _BUILD[name]()


def cloud(name, F):
    """The case's cloud with SH rows of width F (seeded by the case and the width)."""
    c = case(name)
    n = c["xyz"].shape[0]
    rng = np.random.default_rng([zlib.crc32(name.encode()), F])
    sh = rng.normal(0.0, 0.3, (n, F)).astype(np.float32)
    return {"xyz": c["xyz"], "color": c["color"], "cov6": c["cov6"], "opacity": c["opacity"], "sh": sh}


@functools.lru_cache(maxsize=None)
def model(name, F):
    c = case(name)
    return level(cloud(name, F), c["mask"], c["weight"], **c["params"])


def mutated(name, F, mutation):
    c = case(name)
    return level(cloud(name, F), c["mask"], c["weight"], mutation=mutation, **c["params"])


# ============================================================================================================ the tolerance constant
def oracle_level(O, name, F):
    """The case on the CPU oracle (``O`` = the oracle module): the reference's float32 arithmetic in serial order.  -> (level, stats)."""
    c, cl = case(name), cloud(name, F)
    p = c["params"]
    o = O.HemOracle(cl["xyz"], cl["color"], cl["cov6"], cl["opacity"], cl["sh"], p["rho"], p["delta"], p["kappa"], p["tau"])
    o.set_parent_mask(c["mask"])
    o.set_weights(c["weight"])
    o.run_level()
    lv, st = o.level(1), o.stats()
    o.close()
    return lv, st


def ratio(got, mdl, f, rows=None):
    """max over the elements of |got - model| / (2^-24 mag) of field f (rows: how many leading rows; default all); an element of
    magnitude 0 must be equal."""
    a, b, m = np.asarray(got[f], np.float64), mdl[f], mdl["mag"][f]
    if rows is not None:
        a, b, m = a[:rows], b[:rows], m[:rows]
    a = a.reshape(b.shape)
    if a.size == 0:
        return 0.0
    err = np.abs(a - b)
    with np.errstate(all="ignore"):
        r = np.where(m > 0, err / (EPS32 * m), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def k_ref(O, name):
    """Per output field: the largest |oracle - model| / (2^-24 mag) of the case over its widths."""
    out = {f: 0.0 for f in FIELDS}
    for F in widths(name):
        lv, _ = oracle_level(O, name, F)
        mdl = model(name, F)
        assert lv["xyz"].shape[0] == mdl["xyz"].shape[0], (name, F)
        for f in FIELDS:
            if f == "sh" and F == 0:
                continue
            out[f] = max(out[f], ratio(lv, mdl, f))
    return out


def tolerances(O):
    return {name: k_ref(O, name) for name in CASES}


def load_tolerances():
    with open(TOLERANCE_JSON) as fh:
        return json.load(fh)


def small_cases():
    """The cases whose parents all have at most 16 pairs: what the per-pair expression chain alone costs float32."""
    return tuple(n for n in CASES if model(n, 0)["stats"]["max_pairs_of_a_parent"] <= 16)


def bound_constants(tol=None):
    """K(case, field) = MARGIN * max(K_ref(case, field), K_small(field))."""
    tol = load_tolerances() if tol is None else tol
    small = small_cases()
    assert small
    k_small = {f: max(tol[n][f] for n in small) for f in FIELDS}
    return {n: {f: MARGIN * max(tol[n][f], k_small[f]) for f in FIELDS} for n in CASES}
