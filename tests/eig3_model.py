"""Inputs and float64 references for the per-splat 3x3 eigen kernels (no GPU code is imported here).

Kernels under test (tests/test_eig3_gpu.py), conditions on the references themselves (tests/test_eig3_cpu.py):
  normal_of_cov_d   csrc/gsr_normals.h   behind icp.normals_from_cov: Open3D's FastEigen3x3, eigenvector of the smallest eigenvalue
  k_decompose_cov   csrc/model.hip       cyclic Jacobi, GSR_DECOMP_EXACT / GSR_DECOMP_REFERENCE
  k_cov_from_normals csrc/icp.hip        generalized ICP's discs, C = Rx diag(eps, 1, 1) Rx^T

Every random family is seeded; a row is R diag(lambda) R^T in float64, narrowed to float32 (cov6 = xx xy xz yy yz zz).  The references
work on those float32 values widened back to float64, i.e. on exactly what the kernels read.
"""
import functools

import numpy as np

N_FAMILY = 2048
N_GENERIC = 4096
CLAMP = 1e-30                                            # GSR_DECOMP_EXACT clamps eigenvalues there (csrc/model.hip)
S_CLAMP = np.float32(0.5 * np.log(CLAMP))
I6 = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])            # cov6 slots of a 3x3


def cov33(c6):
    c = np.asarray(c6, np.float64).reshape(-1, 6)
    return np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], 1)


def _rotations(rng, n):
    """uniform proper rotations from unit quaternions"""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return quat_to_rot(q)


def quat_to_rot(q):
    w, x, y, z = (q[:, k] for k in range(4))
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def _build(R, lam):
    A = (R * lam[:, None, :]) @ R.transpose(0, 2, 1)
    A = 0.5 * (A + A.transpose(0, 2, 1))
    return A[:, I6[0], I6[1]].astype(np.float32)


def _logu(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape))


@functools.lru_cache(maxsize=None)
def family(name):
    """-> float32 (n, 6), read-only"""
    names = ["generic", "flat", "needle_eq", "disc_eq", "iso_rot", "rank2", "rank1", "diag", "symmetric"]
    if name in ("tiny30", "tiny12", "huge30"):
        s = {"tiny30": 1e-30, "tiny12": 1e-12, "huge30": 1e+30}[name]
        out = (family("generic").astype(np.float64) * s).astype(np.float32)
        out.setflags(write=False)
        return out
    rng = np.random.default_rng(20240 + names.index(name))
    n = N_GENERIC if name == "generic" else N_FAMILY
    R = _rotations(rng, n)
    if name == "generic":
        lam = _logu(rng, 1e-4, 1.0, (n, 3))
    elif name == "flat":
        lam = np.concatenate([_logu(rng, 1e-10, 1e-4, (n, 1)), rng.uniform(0.3, 1.0, (n, 2))], 1)
    elif name == "needle_eq":
        a, b = _logu(rng, 1e-4, 1.0, (2, n))
        lam = np.stack([np.minimum(a, b), np.minimum(a, b), np.maximum(a, b)], 1)
    elif name == "disc_eq":
        a, b = _logu(rng, 1e-4, 1.0, (2, n))
        lam = np.stack([np.minimum(a, b), np.maximum(a, b), np.maximum(a, b)], 1)
    elif name == "iso_rot":
        lam = np.ones((n, 3))
    elif name == "rank2":
        lam = np.concatenate([np.zeros((n, 1)), _logu(rng, 1e-4, 1.0, (n, 2))], 1)
    elif name == "rank1":
        lam = np.concatenate([np.zeros((n, 2)), _logu(rng, 1e-4, 1.0, (n, 1))], 1)
    elif name == "diag":
        R = np.broadcast_to(np.eye(3), (n, 3, 3))
        lam = _logu(rng, 1e-4, 1.0, (n, 3))
    elif name == "symmetric":
        # [[a, b, b], [b, d, e], [b, e, d]]: c01 == c02 and c11 == c22 exactly, also after narrowing, so two of the three cross products
        # eigvec0_d chooses from have exactly equal lengths.  Positive definite: eigenvalues d - e and those of [[a, r2 b], [r2 b, d + e]].
        d = rng.uniform(0.3, 1.0, n)
        e = rng.uniform(-0.9, 0.9, n) * d
        a = _logu(rng, 1e-2, 1.0, n)
        b = rng.uniform(-0.9, 0.9, n) * np.sqrt(a * (d + e) / 2)
        out = np.stack([a, b, b, d, e, d], 1).astype(np.float32)
        out.setflags(write=False)
        return out
    else:
        raise KeyError(name)
    out = _build(R, lam)
    out.setflags(write=False)
    return out


NORMAL_FAMILIES = ("generic", "flat", "needle_eq", "disc_eq", "iso_rot", "rank2", "rank1", "diag", "tiny30", "huge30", "symmetric")
# the decomposition documents a clamp at lambda < 1e-30: scales below that mean nothing to it
DECOMP_FAMILIES = ("generic", "flat", "needle_eq", "disc_eq", "iso_rot", "rank2", "rank1", "diag", "tiny12", "huge30", "symmetric")


def _diag(a, b, c):
    return [a, 0, 0, b, 0, c]


# hand-written rows: (name, cov6, normal Open3D's rule gives or None where only "equal to the oracle" is pinned)
# In the diagonal branch Open3D answers the axis of a STRICTLY smallest diagonal entry, (0, 0, 1) on every tie -- even for diag(0, 0, 1) and
# diag(1, 1, 2), where that is the eigenvector of the LARGEST eigenvalue.  Reference behaviour: pinned, and outside every eigen-residual check.
HAND = [
    ("zero", _diag(0, 0, 0), (0, 0, 1)),
    ("identity", _diag(1, 1, 1), (0, 0, 1)),
    ("3.5 I", _diag(3.5, 3.5, 3.5), (0, 0, 1)),
    ("1e-20 I", _diag(1e-20, 1e-20, 1e-20), (0, 0, 1)),
    ("1e+20 I", _diag(1e+20, 1e+20, 1e+20), (0, 0, 1)),
    ("min at 0", _diag(1, 2, 3), (1, 0, 0)),
    ("min at 1", _diag(2, 1, 3), (0, 1, 0)),
    ("min at 2", _diag(3, 2, 1), (0, 0, 1)),
    ("tie 0 1", _diag(1, 1, 2), (0, 0, 1)),
    ("tie 0 2", _diag(1, 2, 1), (0, 0, 1)),
    ("tie 1 2", _diag(2, 1, 1), (0, 0, 1)),
    ("diag(0, 0, 1)", _diag(0, 0, 1), (0, 0, 1)),
    ("diag(0, 1, 0)", _diag(0, 1, 0), (0, 0, 1)),
    ("diag(1, 0, 0)", _diag(1, 0, 0), (0, 0, 1)),
    # the largest COEFFICIENT (Open3D scales by maxCoeff, not by the largest magnitude) is an off-diagonal zero: the zero-matrix answer
    ("negative definite", _diag(-1, -2, -3), (0, 0, 1)),
]
HAND_COV6 = np.array([h[1] for h in HAND], np.float32)
HAND_NORMALS = np.array([h[2] for h in HAND], np.float64)
HAND_COV6.setflags(write=False)
HAND_PSD = np.array([h[0] not in ("zero", "negative definite") for h in HAND])       # rows GSR_DECOMP_EXACT can reproduce

# each of the six entries in turn NaN, +Inf, -Inf on a base whose smallest diagonal entry is NOT the last one: a leak of the non-finite
# entry into the diagonal branch answers (1, 0, 0) there, which the fallback (0, 0, 1) cannot be mistaken for
NONFINITE_BASE = (1, 0, 0, 2, 0, 3)


def nonfinite_rows():
    rows = []
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(6):
            r = list(NONFINITE_BASE)
            r[k] = bad
            rows.append(r)
    return np.array(rows, np.float32)


# ---- eigen references ------------------------------------------------------------------------------------------------------
def eig(c6):
    """-> (lam (n,3) ascending, V (n,3,3) columns = eigenvectors) of the float32 rows in float64 (LAPACK)"""
    return np.linalg.eigh(cov33(c6))


def decided(lam):
    """the smallest eigenvalue has an eigenvector of its own: (lam1 - lam0) >= 1e-2 max|lam|"""
    return (lam[:, 1] - lam[:, 0]) >= 1e-2 * np.abs(lam).max(1)


def excess(c6, v, lam=None):
    """e / max|lam| per row, e = v^T A v - lam0 on decided rows and max(0, v^T A v - lam1) on the others (any unit vector of the
    two-dimensional eigenspace is right there).  The Rayleigh quotient is taken in long double, so the figure is the vector's, not ours."""
    A = cov33(c6).astype(np.longdouble)
    if lam is None:
        lam = np.linalg.eigvalsh(cov33(c6))
    vl = np.asarray(v, np.float64).astype(np.longdouble)
    ray = np.einsum("ni,nij,nj->n", vl, A, vl) / np.einsum("ni,ni->n", vl, vl)
    d = decided(lam)
    e = np.where(d, ray - lam[:, 0], np.maximum(0, ray - lam[:, 1]))
    return (e / np.abs(lam).max(1)).astype(np.float64)


def norm_ld(v):
    """|v| per row in long double: the figure is the vector's, not the rounding of the check"""
    vl = np.asarray(v, np.float64).astype(np.longdouble)
    return np.sqrt(np.einsum("ni,ni->n", vl, vl))


def angle_to(v, w):
    """angle between the lines spanned by unit vectors v and w (cross product: accurate at small angles)"""
    return np.arcsin(np.minimum(1.0, np.linalg.norm(np.cross(v, w), axis=1)))


def up_to_sign(got, want):
    """min(|got - want|_inf, |got + want|_inf) per row"""
    return np.minimum(np.abs(got - want).max(1), np.abs(got + want).max(1))


# ---- GSR_DECOMP_EXACT in float64 -------------------------------------------------------------------------------------------
def exact_rotation(c6):
    """-> (lam, R): eigh with the kernel's documented conventions -- largest-magnitude component of every eigenvector positive (first
    maximum on ties), third column flipped when the determinant is negative"""
    lam, V = eig(c6)
    n = len(lam)
    m = np.abs(V).argmax(1)
    sgn = np.sign(V[np.arange(n)[:, None], m, np.arange(3)[None, :]])
    sgn[sgn == 0] = 1
    R = V * sgn[:, None, :]
    R[np.linalg.det(R) < 0, :, 2] *= -1
    return lam, R


def shepperd(R):
    """-> (branch (n,) in 0..3 = w x y z by the kernel's rule: trace > 0, else the largest diagonal entry; q (n,4) float64 with w >= 0;
    margin (n,)).  The four candidates are 4 q_k^2 = 1 +- R00 +- R11 +- R22; margin = q_branch^2 - (largest other q_k^2): where it is
    positive the branch's component is also the largest component of the quaternion, and only there does the class of an OUTPUT quaternion
    (its largest component) tell the branch.  (With trace > 0 the kernel takes w although another component may be larger; both branches
    are then well conditioned and give the same quaternion.)"""
    d0, d1, d2 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    tr = d0 + d1 + d2
    branch = np.where(tr > 0, 0, np.where((d0 > d1) & (d0 > d2), 1, np.where(d1 > d2, 2, 3)))
    four = np.stack([1 + tr, 1 + d0 - d1 - d2, 1 - d0 + d1 - d2, 1 - d0 - d1 + d2], 1)        # 4 w^2, 4 x^2, 4 y^2, 4 z^2
    n = len(R)
    s = np.sqrt(np.maximum(four[np.arange(n), branch], 0)) * 2
    anti = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1)      # 4 w (x, y, z)
    sym = np.stack([R[:, 0, 1] + R[:, 1, 0], R[:, 0, 2] + R[:, 2, 0], R[:, 1, 2] + R[:, 2, 1]], 1)       # 4 xy, 4 xz, 4 yz
    q = np.empty((n, 4))
    with np.errstate(all="ignore"):
        for b in range(4):
            r = branch == b
            if b == 0:
                cand = np.stack([0.25 * s, anti[:, 0] / s, anti[:, 1] / s, anti[:, 2] / s], 1)
            elif b == 1:
                cand = np.stack([anti[:, 0] / s, 0.25 * s, sym[:, 0] / s, sym[:, 1] / s], 1)
            elif b == 2:
                cand = np.stack([anti[:, 1] / s, sym[:, 0] / s, 0.25 * s, sym[:, 2] / s], 1)
            else:
                cand = np.stack([anti[:, 2] / s, sym[:, 1] / s, sym[:, 2] / s, 0.25 * s], 1)
            q[r] = cand[r]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 0] < 0] *= -1
    q2 = four / 4
    other = np.where(np.arange(4)[None, :] == branch[:, None], -np.inf, q2).max(1)
    return branch, q, q2[np.arange(n), branch] - other


def exact_model(c6):
    """what GSR_DECOMP_EXACT should hand on: -> (s float32 (n,3), q float32 (n,4))"""
    lam, R = exact_rotation(c6)
    _, q, _ = shepperd(R)
    return (0.5 * np.log(np.maximum(lam, CLAMP))).astype(np.float32), q.astype(np.float32)


def reconstruct(s, q):
    """R(q) diag(exp 2s) R(q)^T in float64 from the float32 outputs -> (C (n,3,3), R (n,3,3))"""
    R = quat_to_rot(np.asarray(q, np.float64))
    C = (R * np.exp(2 * np.asarray(s, np.float64))[:, None, :]) @ R.transpose(0, 2, 1)
    return C, R


def recon_error(c6, s, q):
    """max|R diag(exp 2s) R^T - A| / max|A| per row"""
    A = cov33(c6)
    C, _ = reconstruct(s, q)
    return np.abs(C - A).max((1, 2)) / np.abs(A).max((1, 2))


# ---- cov_from_normals ------------------------------------------------------------------------------------------------------
CFN_X = (1.0, 0.0, -1.0, -0.99, np.nextafter(-0.99, -1.0), np.nextafter(-0.99, 0.0), -0.98, -0.999)
CFN_SPECIAL = np.array([[0.0, 0.0, 0.0], [3.0, -4.0, 12.0], [np.nan, 0.6, 0.8]])      # zero, unnormalised, NaN (last three input rows)


@functools.lru_cache(maxsize=None)
def cfn_normals():
    """-> float64 (n,3): per x of CFN_X eight unit normals (x kept exactly; x = +-1 once), the six axes, 2000 random ones, CFN_SPECIAL"""
    rows = []
    for x in CFN_X:
        r = np.sqrt(max(0.0, 1 - x * x))
        if r == 0:
            rows.append([x, 0.0, 0.0])
            continue
        for phi in np.arange(8) * (np.pi / 4) + 0.1:
            rows.append([x, r * np.cos(phi), r * np.sin(phi)])
        rows += [[x, r, 0.0], [x, 0.0, -r]]              # and in the coordinate planes
    rows += [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    rng = np.random.default_rng(77)
    u = rng.standard_normal((2000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    out = np.concatenate([np.array(rows, np.float64), u, CFN_SPECIAL])
    out.setflags(write=False)
    return out


def cfn_identity_side(nrm):
    """rows on the identity side of Open3D's branch: one float64 compare"""
    return np.asarray(nrm, np.float64)[:, 0] < -0.99


def cfn_model(nrm, eps):
    """C = Rx diag(eps, 1, 1) Rx^T, Rx = I + [v]x + [v]x^2 / (1 + c), v = e1 x n, c = e1 . n (the identity when c < -0.99), in long double.
    -> (cov6 (n,6) long double, mag (n,6)): mag is the sum of the absolute values of all terms of the expanded entry,
    sum_k d_k (|I_ak| + |S_ak| + sum_j |S_aj S_jk| / |1 + c|) (the same for b) -- every rounding error of a float64 evaluation is a few
    2^-53 of it, in whatever order it adds."""
    L = np.longdouble
    n = np.asarray(nrm, np.float64).astype(L)
    m = len(n)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    zero = np.zeros(m, L)
    S = np.stack([np.stack([zero, -y, -z], 1), np.stack([y, zero, zero], 1), np.stack([z, zero, zero], 1)], 1)     # [v]x, v = (0, -z, y)
    ident = np.broadcast_to(np.eye(3, dtype=L), (m, 3, 3))
    with np.errstate(all="ignore"):
        f = L(1) / (L(1) + x)
        R = ident + S + (S @ S) * f[:, None, None]
        Rabs = ident + np.abs(S) + (np.abs(S) @ np.abs(S)) * np.abs(f)[:, None, None]
    side = cfn_identity_side(nrm)
    R[side] = ident[side]
    Rabs[side] = ident[side]
    d = np.array([eps, 1.0, 1.0], L)
    with np.errstate(all="ignore"):
        C = (R * d) @ R.transpose(0, 2, 1)
        mag = (Rabs * d) @ Rabs.transpose(0, 2, 1)
    return C[:, I6[0], I6[1]], mag[:, I6[0], I6[1]]


CFN_BOUND = 32 * 2.0 ** -52


def cfn_worst_ratio(diff, mag):
    """worst |diff| / mag over the entries that have terms at all (for printing; an entry without terms must be exact)"""
    has = mag > 0
    return float((diff[has] / mag[has]).max())
