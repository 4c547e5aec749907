"""Float64 NumPy / SciPy model of non-rigid refinement (the contract in include/gsr_hip.h), independent of the
library: weights, field and F; brute-force correspondences with the tie rule; per-cell sums that return sum |term| beside every sum;
dense assembly, a dense solve and the whole coarse-to-fine loop.  Every term is formed in the operation order the header states, so
that the library's sums differ from these only by the order of summation.
"""
import numpy as np

CELL_LEN = 326
IU = np.triu_indices(24)                # the upper triangle row by row: slot t <-> (IU[0][t], IU[1][t])
BITS = np.array([[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)])


# ---------------------------------------------------------------------------------------------------- lattice and field
def default_box(points):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(1)]
    lo, hi = p.min(0), p.max(0)
    big = (hi - lo).max()
    short = np.maximum(1e-3 * big - (hi - lo), 0.0) * 0.5
    lo, hi = lo - short, hi + short
    return lo - 1e-6 * big, hi + 1e-6 * big


def spacing(lo, hi, dims):
    return (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)) / (np.asarray(dims) - 1).astype(np.float64)


def node_positions(lo, hi, dims):
    h = spacing(lo, hi, dims)
    ax = [lo[a] + np.arange(dims[a], dtype=np.float64) * h[a] for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def locate(lo, hi, dims, p):
    """-> c (n, 3) int, f (n, 3), active (n, 3) bool, h (3,) for finite float64 points"""
    n = np.asarray(dims, np.int64)
    h = spacing(lo, hi, dims)
    s = (p - np.asarray(lo, np.float64)) / h
    top = (n - 1).astype(np.float64)
    sb = np.minimum(np.maximum(s, 0.0), top)
    c = np.minimum(np.floor(sb).astype(np.int64), n - 2)
    f = sb - c
    return c, f, (s > 0.0) & (s < top), h


def weights(f):
    """(n, 8): w_k = (X Y) Z"""
    w = np.empty((f.shape[0], 8))
    for k in range(8):
        X, Y, Z = (f[:, a] if BITS[k, a] else 1.0 - f[:, a] for a in range(3))
        w[:, k] = (X * Y) * Z
    return w


def grad_weights(f, active, h):
    """(n, 8, 3): dw_k / dp_a, 0 on clamped axes and on the outer faces"""
    inv = np.where(active, 1.0 / h, 0.0)
    g = np.empty((f.shape[0], 8, 3))
    for k in range(8):
        X, Y, Z = (f[:, a] if BITS[k, a] else 1.0 - f[:, a] for a in range(3))
        sx, sy, sz = (inv[:, a] if BITS[k, a] else -inv[:, a] for a in range(3))
        g[:, k, 0] = (sx * Y) * Z
        g[:, k, 1] = (X * sy) * Z
        g[:, k, 2] = (X * Y) * sz
    return g


def cell_nodes(dims, c):
    """(n, 8) node indices of the cells c (n, 3)"""
    return np.stack([((c[:, 0] + BITS[k, 0]) * dims[1] + c[:, 1] + BITS[k, 1]) * dims[2] + c[:, 2] + BITS[k, 2] for k in range(8)], 1)


def cell_index(dims, c):
    return (c[:, 0] * (dims[1] - 1) + c[:, 1]) * (dims[2] - 1) + c[:, 2]


def displacement(lo, hi, dims, U, p):
    """d(p) for finite float64 points: sum_k w_k U_k, k ascending"""
    c, f, _, _ = locate(lo, hi, dims, p)
    w, nd = weights(f), cell_nodes(dims, c)
    d = np.zeros_like(p)
    for k in range(8):
        d += w[:, k, None] * U[nd[:, k]]
    return d


def deformation(lo, hi, dims, U, p):
    """F(p) (n, 3, 3) = I + sum_k U_k grad w_k'"""
    c, f, act, h = locate(lo, hi, dims, p)
    gw, nd = grad_weights(f, act, h), cell_nodes(dims, c)
    J = np.zeros((p.shape[0], 3, 3))
    for k in range(8):
        J += U[nd[:, k]][:, :, None] * gw[:, k, None, :]
    return np.eye(3)[None] + J


def warp_points(lo, hi, dims, U, xyz32):
    """float64 p + d(p) of the finite rows (the others as they are); round with .astype(float32) to compare"""
    p = np.asarray(xyz32, np.float32).astype(np.float64)
    out = p.copy()
    ok = np.isfinite(p).all(1)
    out[ok] = p[ok] + displacement(lo, hi, dims, U, p[ok])
    return out


def warp_model(lo, hi, dims, U, xyz32, cov6_32):
    """-> (xyz' float64, cov6' float64, n_folded): cov' = F cov F' with the products summed left to right"""
    p = np.asarray(xyz32, np.float32).astype(np.float64)
    S = np.asarray(cov6_32, np.float32).astype(np.float64)
    ok = np.isfinite(p).all(1)
    xyz, cov = p.copy(), S.copy()
    q = p[ok]
    F = deformation(lo, hi, dims, U, q)
    xyz[ok] = q + displacement(lo, hi, dims, U, q)
    s = S[ok]
    Cm = np.stack([s[:, [0, 1, 2]], s[:, [1, 3, 4]], s[:, [2, 4, 5]]], 1)
    Mx = np.empty_like(Cm)
    for a in range(3):
        for b in range(3):
            Mx[:, a, b] = (F[:, a, 0] * Cm[:, 0, b] + F[:, a, 1] * Cm[:, 1, b]) + F[:, a, 2] * Cm[:, 2, b]
    out, t = np.empty_like(s), 0
    for a in range(3):
        for b in range(a, 3):
            out[:, t] = (Mx[:, a, 0] * F[:, b, 0] + Mx[:, a, 1] * F[:, b, 1]) + Mx[:, a, 2] * F[:, b, 2]
            t += 1
    cov[ok] = out
    det = (F[:, 0, 0] * (F[:, 1, 1] * F[:, 2, 2] - F[:, 1, 2] * F[:, 2, 1]) - F[:, 0, 1] * (F[:, 1, 0] * F[:, 2, 2] - F[:, 1, 2] * F[:, 2, 0])) + \
        F[:, 0, 2] * (F[:, 1, 0] * F[:, 2, 1] - F[:, 1, 1] * F[:, 2, 0])
    return xyz, cov, int((det <= 0.0).sum())


def prolong(lo, hi, dims, U, fine_dims):
    return displacement(lo, hi, dims, U, node_positions(lo, hi, fine_dims))


# ---------------------------------------------------------------------------------------------------- correspondences
def correspond_brute(q, tgt32, max_corr, chunk=4096):
    """nearest target point of every float64 query q: strict d^2 < max_corr^2, lowest index on a tie; -1 without one"""
    t = np.asarray(tgt32, np.float32).astype(np.float64)
    out = np.full(q.shape[0], -1, np.int64)
    if t.shape[0] == 0:
        return out
    for s in range(0, q.shape[0], chunk):
        a = q[s:s + chunk]
        dx, dy, dz = (a[:, None, k] - t[None, :, k] for k in range(3))
        d2 = dx * dx + dy * dy + dz * dz
        d2[np.isnan(d2)] = np.inf
        j = np.argmin(d2, 1)                      # the first of equal minima: the lowest index
        ok = d2[np.arange(a.shape[0]), j] < max_corr * max_corr
        out[s:s + chunk] = np.where(ok, j, -1)
    return out


def correspond_tree(q, tgt32, max_corr):
    """the same by a k-d tree, for clouds where exact ties do not occur (the loop on 20 000 random points)"""
    from scipy.spatial import cKDTree
    t = np.asarray(tgt32, np.float32).astype(np.float64)
    _, j = cKDTree(t).query(q, k=1)
    dx, dy, dz = (q[:, k] - t[j, k] for k in range(3))
    return np.where(dx * dx + dy * dy + dz * dz < max_corr * max_corr, j, -1)


# ---------------------------------------------------------------------------------------------------- sums
def point_terms(lo, hi, dims, U, src32, tgt32, nrm, max_corr, search=correspond_brute):
    """-> rows (indices of the matched source points), cell (per row), v (n, 25): g[24] and r0, j (matched target)"""
    p = np.asarray(src32, np.float32).astype(np.float64)
    fin = np.where(np.isfinite(p).all(1))[0]
    pf = p[fin]
    j = search(pf + displacement(lo, hi, dims, U, pf), tgt32, max_corr)
    m = j >= 0
    rows, pf, j = fin[m], pf[m], j[m]
    c, f, _, _ = locate(lo, hi, dims, pf)
    w = weights(f)
    q = np.asarray(tgt32, np.float32).astype(np.float64)[j]
    n = np.asarray(nrm, np.float64)[j]
    r0 = ((pf[:, 0] - q[:, 0]) * n[:, 0] + (pf[:, 1] - q[:, 1]) * n[:, 1]) + (pf[:, 2] - q[:, 2]) * n[:, 2]
    g = (w[:, :, None] * n[:, None, :]).reshape(-1, 24)
    return rows, cell_index(dims, c), np.concatenate([g, r0[:, None]], 1), j, cell_nodes(dims, c)


def cell_sums(dims, cell, v):
    """-> (sums, abs_sums), each (ncells, 326): the 300 + 24 + 1 + 1 sums of every cell and the sums of the terms' magnitudes"""
    ncells = int(np.prod(np.asarray(dims) - 1))
    sums, mags = np.zeros((ncells, CELL_LEN)), np.zeros((ncells, CELL_LEN))
    g, r0 = v[:, :24], v[:, 24]
    for c in np.unique(cell):
        m = cell == c
        gc, rc = g[m], r0[m]
        terms = np.concatenate([gc[:, IU[0]] * gc[:, IU[1]], gc * rc[:, None], (rc * rc)[:, None], np.ones((gc.shape[0], 1))], 1)
        sums[c] = terms.sum(0)
        mags[c] = np.abs(terms).sum(0)
    return sums, mags


def accumulate(lo, hi, dims, U, src32, tgt32, nrm, max_corr, search=correspond_brute):
    """-> sums, abs_sums, n_corr, rmse (at U, evaluated point by point)"""
    rows, cell, v, j, nd = point_terms(lo, hi, dims, U, src32, tgt32, nrm, max_corr, search)
    sums, mags = cell_sums(dims, cell, v)
    n = rows.shape[0]
    rmse = 0.0
    if n:
        u = U[nd].reshape(n, 24)
        rmse = float(np.sqrt(((v[:, 24] + (v[:, :24] * u).sum(1)) ** 2).sum() / n))
    return sums, mags, n, rmse


# ---------------------------------------------------------------------------------------------------- energy, assembly, solve
def stencils(dims):
    """-> (triples (nT, 3), edges (nE, 2)) of node indices"""
    idx = np.arange(int(np.prod(dims))).reshape(dims)
    tri, edg = [], []
    for a in range(3):
        m = np.moveaxis(idx, a, 0)
        if dims[a] >= 2:
            edg.append(np.stack([m[:-1].ravel(), m[1:].ravel()], 1))
        if dims[a] >= 3:
            tri.append(np.stack([m[:-2].ravel(), m[1:-1].ravel(), m[2:].ravel()], 1))
    return (np.concatenate(tri) if tri else np.zeros((0, 3), np.int64)), np.concatenate(edg)


def reg_weights(dims, n_corr, lam, lam0):
    tri, edg = stencils(dims)
    M = int(np.prod(dims))
    return (lam * n_corr / len(tri) if len(tri) else 0.0), 0.01 * lam * n_corr / len(edg), lam0 * n_corr / M


def all_cell_nodes(dims):
    d = np.asarray(dims)
    cc = np.stack(np.meshgrid(*[np.arange(d[a] - 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    return cell_nodes(dims, cc)


def energy(dims, sums, lam, lam0, U):
    """E(U) from the sums, term by term"""
    n_corr = sums[:, 325].sum()
    wT, wE, w0 = reg_weights(dims, n_corr, lam, lam0)
    tri, edg = stencils(dims)
    nd = all_cell_nodes(dims)
    E = 0.0
    for c in range(sums.shape[0]):
        u = U[nd[c]].reshape(24)
        A = np.zeros((24, 24))
        A[IU] = sums[c, :300]
        A = A + A.T - np.diag(np.diag(A))
        E += sums[c, 324] + 2.0 * sums[c, 300:324] @ u + u @ A @ u
    if len(tri):
        E += wT * ((U[tri[:, 0]] - 2.0 * U[tri[:, 1]] + U[tri[:, 2]]) ** 2).sum()
    E += wE * ((U[edg[:, 0]] - U[edg[:, 1]]) ** 2).sum()
    E += w0 * (U ** 2).sum()
    return float(E)


def assemble(dims, sums, lam, lam0):
    """-> (H (3M, 3M), b (3M,)) with E(U) = U' H U + 2 b' U + const: the minimiser solves H U = -b"""
    M = int(np.prod(dims))
    n_corr = sums[:, 325].sum()
    wT, wE, w0 = reg_weights(dims, n_corr, lam, lam0)
    tri, edg = stencils(dims)
    nd = all_cell_nodes(dims)
    H, b = np.zeros((3 * M, 3 * M)), np.zeros(3 * M)
    for c in range(sums.shape[0]):
        A = np.zeros((24, 24))
        A[IU] = sums[c, :300]
        A = A + A.T - np.diag(np.diag(A))
        ix = (3 * nd[c][:, None] + np.arange(3)[None]).reshape(24)
        H[np.ix_(ix, ix)] += A
        b[ix] += sums[c, 300:324]
    D = np.zeros((len(tri), M))
    if len(tri):
        r = np.arange(len(tri))
        D[r, tri[:, 0]] += 1.0; D[r, tri[:, 1]] -= 2.0; D[r, tri[:, 2]] += 1.0
    G = np.zeros((len(edg), M))
    r = np.arange(len(edg))
    G[r, edg[:, 0]] += 1.0; G[r, edg[:, 1]] -= 1.0
    R = wT * D.T @ D + wE * G.T @ G + w0 * np.eye(M)
    H += np.kron(R, np.eye(3))
    return H, b


def solve_dense(dims, sums, lam, lam0):
    """-> (U (M, 3), cond(H)); U = 0 without a correspondence"""
    M = int(np.prod(dims))
    if sums[:, 325].sum() == 0:
        return np.zeros((M, 3)), 1.0
    H, b = assemble(dims, sums, lam, lam0)
    from scipy.linalg import cho_factor, cho_solve
    U = cho_solve(cho_factor(H), -b)
    return U.reshape(M, 3), float(np.linalg.cond(H))


# ---------------------------------------------------------------------------------------------------- the loop
def refine(src32, tgt32, nrm, max_corr, levels=3, max_iteration=6, lam=0.01, lam0=1e-6, relative_rmse=1e-6, box=None, search=correspond_tree):
    """the coarse-to-fine loop -> dict(lo, hi, dims, U, rmse_before, rmse_after, n_corr, log)"""
    lo, hi = box if box is not None else default_box(src32)
    U, dims, log, first = None, None, [], None
    for level in range(levels):
        fine = (2 ** level + 1,) * 3
        U = np.zeros((int(np.prod(fine)), 3)) if U is None else prolong(lo, hi, dims, U, fine)
        dims, prev = fine, None
        for _ in range(max_iteration):
            sums, _, n, rmse = accumulate(lo, hi, dims, U, src32, tgt32, nrm, max_corr, search)
            if first is None:
                first = rmse
            if n == 0 or (prev is not None and abs(prev - rmse) < relative_rmse * prev):
                break
            prev = rmse
            U, _ = solve_dense(dims, sums, lam, lam0)
            log.append((dims, n, rmse))
    _, _, n, rmse = accumulate(lo, hi, dims, U, src32, tgt32, nrm, max_corr, search)
    return {"lo": lo, "hi": hi, "dims": dims, "U": U, "rmse_before": first, "rmse_after": rmse, "n_corr": n, "log": log}


# ---------------------------------------------------------------------------------------------------- the drift scene
def sheets(n, rng):
    """n points on three mutually orthogonal wavy sheets z = 0.2 sin 3x cos 2y, x, y in [-1, 1], with their analytic unit normals: a
    third as it is, a third with its coordinates cycled (x, y, z) -> (z, x, y) and shifted by (-1, 0, 1), a third cycled the other
    way and shifted by (0, -1, 1)"""
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    p = np.stack([x, y, 0.2 * np.sin(3 * x) * np.cos(2 * y)], 1)
    nr = np.stack([-0.6 * np.cos(3 * x) * np.cos(2 * y), 0.4 * np.sin(3 * x) * np.sin(2 * y), np.ones(n)], 1)
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    k = n // 3
    p[k:2 * k], nr[k:2 * k] = p[k:2 * k][:, [2, 0, 1]] + np.array([-1.0, 0.0, 1.0]), nr[k:2 * k][:, [2, 0, 1]]
    p[2 * k:], nr[2 * k:] = p[2 * k:][:, [1, 2, 0]] + np.array([0.0, -1.0, 1.0]), nr[2 * k:][:, [1, 2, 0]]
    return p, nr


def drift(p, a=0.04):
    return a * np.stack([0.5 * p[:, 1] ** 2, -0.3 * p[:, 0] * p[:, 1], p[:, 0] ** 2], 1)


def drift_scene(n=20000, seed=0, jitter=0.002, a=0.04):
    """-> dict: tgt (float32), nrm (float64), clean (float64: the third sample, undrifted), src (float32: clean + drift),
    null (float32: clean itself)"""
    rng = np.random.default_rng(seed)
    _ = sheets(n, rng)                                   # the scene's own sample: the target and the source are independent of it
    t, nr = sheets(n, rng)
    t = t + rng.normal(0.0, jitter, t.shape)
    clean, _ = sheets(n, rng)
    return {"tgt": t.astype(np.float32), "nrm": nr, "clean": clean, "src": (clean + drift(clean, a)).astype(np.float32),
            "null": clean.astype(np.float32)}


def rms(a):
    return float(np.sqrt((np.asarray(a, np.float64) ** 2).sum(1).mean()))
