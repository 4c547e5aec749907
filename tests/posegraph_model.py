"""Independent float64 model of the multiway registration contract (NumPy + SciPy; nothing of the library):

* information matrix of a pair: correspondences by ``cKDTree`` with the strict ``d^2 < max_corr^2`` gate, ``Lambda = sum G^T G`` from
  explicit rows ``G = [-[q]x | I3]`` at the matched target points;
* edge residual ``D = X_t^-1 X_s T^-1``, ``r = [log_SO3(R_D); t_D]`` (SciPy's rotation vectors), ``chi = r^T Lambda r``;
* the objective with the line process eliminated (a certain edge costs ``chi``, an uncertain one ``mu chi / (mu + chi)``) minimised by
  ``scipy.optimize.least_squares`` on Cholesky-whitened residuals, poses parametrised as (rotation vector, translation);
* the procedure: optimise, prune the uncertain edges with ``l = (mu / (mu + chi))^2 < threshold``, optimise the rest with ``mu`` recomputed.
"""
import numpy as np
from scipy.optimize import least_squares
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation


# ------------------------------------------------------------------------------------------------------------------ information
def skew(q):
    return np.array([[0.0, -q[2], q[1]], [q[2], 0.0, -q[0]], [-q[1], q[0], 0.0]])


def information_from_points(q):
    """sum over the rows of q (n, 3) of G^T G, G = [-[q]x | I3] (3 x 6, rotation columns first)"""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    L = np.zeros((6, 6))
    for a in range(0, len(q), 65536):                      # the rows G of a chunk of points, explicitly: (m, 3, 6)
        c = q[a:a + 65536]
        G = np.zeros((len(c), 3, 6))
        G[:, 0, 1], G[:, 0, 2] = c[:, 2], -c[:, 1]          # -[q]x
        G[:, 1, 0], G[:, 1, 2] = -c[:, 2], c[:, 0]
        G[:, 2, 0], G[:, 2, 1] = c[:, 1], -c[:, 0]
        G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1.0
        L += np.einsum("nia,nib->ab", G, G)
    return L


def correspondences(src, tgt, T, max_corr):
    """-> (index of the nearest target point or -1 per source point, squared distance) at transform T, strict gate"""
    p = np.asarray(src, np.float64) @ T[:3, :3].T + T[:3, 3]
    tgt = np.asarray(tgt, np.float64)
    d, j = cKDTree(tgt).query(p, k=1)
    d2 = ((p - tgt[j]) ** 2).sum(1)
    ok = d2 < max_corr * max_corr
    return np.where(ok, j, -1), d2


def information(src, tgt, T, max_corr):
    j, _ = correspondences(src, tgt, T, max_corr)
    return information_from_points(np.asarray(tgt, np.float64)[j[j >= 0]]), int((j >= 0).sum())


# ------------------------------------------------------------------------------------------------------------------ poses
def pose(rotvec, t):
    X = np.eye(4)
    X[:3, :3] = Rotation.from_rotvec(np.asarray(rotvec, np.float64)).as_matrix()
    X[:3, 3] = t
    return X


def inv(X):
    Y = np.eye(4)
    Y[:3, :3] = X[:3, :3].T
    Y[:3, 3] = -X[:3, :3].T @ X[:3, 3]
    return Y


def residual(Xs, Xt, T):
    D = inv(Xt) @ Xs @ inv(T)
    return np.concatenate([Rotation.from_matrix(D[:3, :3]).as_rotvec(), D[:3, 3]])


class Edge:
    def __init__(self, s, t, T, info, uncertain):
        self.s, self.t, self.T, self.info, self.uncertain = int(s), int(t), np.asarray(T, np.float64), np.asarray(info, np.float64), bool(uncertain)


def chi(e, poses):
    r = residual(poses[e.s], poses[e.t], e.T)
    return float(r @ e.info @ r)


def mu_of(edges, max_corr, preference=1.0):
    u = [e.info[5, 5] for e in edges if e.uncertain]
    return preference * max_corr * max_corr * float(np.mean(u)) if u else 0.0


def objective(poses, edges, mu):
    E = 0.0
    for e in edges:
        c = chi(e, poses)
        E += mu * c / (mu + c) if e.uncertain else c
    return E


def line_process(poses, edges, mu):
    return np.array([(mu / (mu + chi(e, poses))) ** 2 if e.uncertain else 1.0 for e in edges])


def _unpack(x, poses0, ref):
    poses, k = [], 0
    for i, X0 in enumerate(poses0):
        if i == ref:
            poses.append(X0)
        else:
            poses.append(pose(x[6 * k:6 * k + 3], x[6 * k + 3:6 * k + 6]))
            k += 1
    return poses


def minimise(poses0, edges, mu, ref=0, method="trf", tol=1e-14):
    """least squares over the non-reference poses; -> list of 4x4"""
    chol = [np.linalg.cholesky(e.info) for e in edges]

    def fun(x):
        poses = _unpack(x, poses0, ref)
        out = []
        for e, Lc in zip(edges, chol):
            r = residual(poses[e.s], poses[e.t], e.T)
            w = Lc.T @ r                                   # |w|^2 = chi
            if e.uncertain:
                w = w * np.sqrt(mu / (mu + w @ w))          # |.|^2 = mu chi / (mu + chi)
            out.append(w)
        return np.concatenate(out)

    x0 = np.concatenate([np.concatenate([Rotation.from_matrix(X[:3, :3]).as_rotvec(), X[:3, 3]]) for i, X in enumerate(poses0) if i != ref])
    sol = least_squares(fun, x0, method=method, xtol=tol, ftol=tol, gtol=tol, x_scale=1.0, max_nfev=20000)
    return _unpack(sol.x, poses0, ref)


def global_optimization(poses0, edges, max_corr, prune=0.25, preference=1.0, ref=0, method="trf", tol=1e-14):
    """the whole procedure -> dict(poses, line_process (per input edge), pruned (bool per input edge), mu, mu_first, E)"""
    mu1 = mu_of(edges, max_corr, preference)
    poses = minimise(poses0, edges, mu1, ref, method, tol)
    l = line_process(poses, edges, mu1)
    pruned = np.array([e.uncertain and lv < prune for e, lv in zip(edges, l)])
    rest = [e for e, gone in zip(edges, pruned) if not gone]
    mu2 = mu_of(rest, max_corr, preference)
    poses = minimise(poses, rest, mu2, ref, method, tol)
    l2 = line_process(poses, rest, mu2)
    l[~pruned] = l2
    return {"poses": poses, "line_process": l, "pruned": pruned, "mu": mu2, "mu_first": mu1, "E": objective(poses, rest, mu2)}


# ------------------------------------------------------------------------------------------------------------------ test graphs
def make_graph(seed=0, n_nodes=6, scale=2.0, n_points=2000, odometry_noise=1e-3, loop_noise=2e-4, false_edge=True, exact=False):
    """A ring of scenes: ground-truth poses, odometry edges (i, i + 1), four loop closures and (optionally) one false edge about 30
    degrees and 0.6 units off.  Every edge carries the information matrix of ``n_points`` random scene points seen in its target's
    frame.  -> (gt poses, edges, index of the false edge or None)"""
    rng = np.random.default_rng(seed)
    gt = [np.eye(4)] + [pose(rng.normal(size=3) * 0.4, rng.normal(size=3) * scale * 0.5) for _ in range(n_nodes - 1)]

    def edge(s, t, noise, uncertain, off=None):
        T = inv(gt[t]) @ gt[s]
        if not exact:
            T = pose(rng.normal(size=3) * noise, rng.normal(size=3) * noise) @ T
        if off is not None:
            T = off @ T
        pts = (rng.random((n_points, 3)) - 0.5) * scale
        q = pts @ inv(gt[t])[:3, :3].T + inv(gt[t])[:3, 3]
        return Edge(s, t, T, information_from_points(q), uncertain)

    edges = [edge(i, i + 1, odometry_noise, False) for i in range(n_nodes - 1)]
    for s, t in [(0, 2), (1, 4), (0, n_nodes - 1), (2, n_nodes - 1)]:
        edges.append(edge(s, t, loop_noise, True))
    k_false = None
    if false_edge:
        k_false = len(edges)
        edges.append(edge(1, 3, loop_noise, True, off=pose(np.array([0.3, -0.35, 0.25]), np.array([0.4, -0.3, 0.33]))))
    return gt, edges, k_false


def chain_odometry(n_nodes, edges, ref_pose=None):
    """poses from chaining the certain edges (i, i + 1): X_{i+1} = X_i T_{i,i+1}^-1"""
    poses = [np.eye(4) if ref_pose is None else ref_pose]
    for i in range(n_nodes - 1):
        e = next(e for e in edges if e.s == i and e.t == i + 1 and not e.uncertain)
        poses.append(poses[i] @ inv(e.T))
    return poses


def pose_error(poses, gt):
    return max(np.linalg.norm(np.asarray(a) - b) for a, b in zip(poses, gt))
