"""gsr_model_transform: positions, covariances, quaternions and SH-rest coefficients of a splat model moved by a rigid 4x4 in one
kernel, and the merge that writes straight into the merged arrays.

Reference = the same formulas in float64 numpy with the matrices the kernel uses (narrowed to float32 once).  Every row is judged
on its own scale; with u = 2^-24 the bounds are twice the worst-case rounding of the float32 evaluation:
    xyz   4 terms (3 products + t)                     |d| <= 8 u (|R||x| + |t|)
    cov   two 3-term products in a row                 |d| <= 16 u (|R||S||R^T|)
    sh    at most 7 terms per coefficient              |d| <= 16 u (|D||c|)
    rot   rotation matrix of q' against R R(q)         1e-5 (the bar of tests/test_ply_io.py::test_transform_and_merge_models)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from gaussiansplattingregistration_amd import synth
from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435]
BANDS = (slice(0, 3), slice(3, 8), slice(8, 15))
T37 = synth.rigid_transform(37.0, (0.4, -1.0, 0.7), (0.3, -0.2, 0.15))


def sh_basis_rest(d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return np.stack([-C1 * y, C1 * z, -C1 * x,
                     C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy),
                     C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy), C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                     C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy), C3[6] * x * (xx - 3 * yy)], axis=1)


def narrowed(T):
    """-> R, t as the kernel holds them: float32 values, in float64"""
    T = np.asarray(T, np.float64)
    return T[:3, :3].astype(np.float32).astype(np.float64), T[:3, 3].astype(np.float32).astype(np.float64)


def full_cov(c6):
    c = np.asarray(c6, np.float64)
    return c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def six(Cf):
    return Cf[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]


def ref_xyz(xyz, T):
    R, t = narrowed(T)
    x = np.asarray(xyz, np.float64)
    return x @ R.T + t, 8 * U * (np.abs(x) @ np.abs(R).T + np.abs(t))


def ref_cov(cov6, T):
    R, _ = narrowed(T)
    S = full_cov(cov6)
    return six(R @ S @ R.T), 16 * U * six(np.abs(R) @ np.abs(S) @ np.abs(R).T)


def ref_sh(sh, T, deg):
    """sh (n, K, 3) -> (rotated, bound), band after band with the float32-narrowed D of the float64 rotation"""
    s = np.asarray(sh, np.float64)
    out, bound = s.copy(), np.zeros_like(s)
    D = GaussianModel.rotate_sh_matrices(np.asarray(T, np.float64)[:3, :3], deg)
    for l in range(deg):
        Dl = D[l].astype(np.float32).astype(np.float64)
        out[:, BANDS[l], :] = np.einsum("ij,njc->nic", Dl, s[:, BANDS[l], :])
        bound[:, BANDS[l], :] = 16 * U * np.einsum("ij,njc->nic", np.abs(Dl), np.abs(s[:, BANDS[l], :]))
    return out, bound


def worst(got, want, bound, what):
    """largest |got - want| / bound over the entries (entries with a zero bound must be exact); printed before it is judged"""
    d = np.abs(np.asarray(got, np.float64) - want)
    r = float(np.max(np.where(bound > 0, d / np.where(bound > 0, bound, 1.0), np.where(d > 0, np.inf, 0.0)))) if d.size else 0.0
    print(f"{what}: worst error / bound = {r:.3f}")
    return r


def make_model(n, deg, seed, device="cuda:0"):
    c = synth.make_cloud(n, seed=seed, sh_degree=deg)
    g = GaussianModel(device).from_arrays(c["xyz"], c["color"], c["opacity"], c["cov6"], c["sh"], deg)
    rng = np.random.default_rng(seed + 100)
    q = rng.normal(size=(n, 4)).astype(np.float32)                   # not normalised, as 3DGS leaves them on disk
    g._rotation = torch.from_numpy(q).to(device)
    g._scaling = torch.from_numpy(rng.normal(-2.5, 0.5, (n, 3)).astype(np.float32)).to(device)
    return g, c, q


def host(t):
    return t.detach().cpu().numpy()


def check_rot(q_out, q_in, T, what):
    Rq = synth._quat_to_rot(q_in.astype(np.float64) / np.linalg.norm(q_in.astype(np.float64), axis=1, keepdims=True))
    Ro = synth._quat_to_rot(np.asarray(q_out, np.float64))
    err = float(np.abs(Ro - np.asarray(T, np.float64)[:3, :3] @ Rq).max())
    nrm = float(np.abs(np.linalg.norm(np.asarray(q_out, np.float64), axis=1) - 1).max())
    print(f"{what}: rotation matrix error {err:.2e}, |q| - 1 {nrm:.2e}")
    assert err <= 1e-5 and nrm <= 1e-6


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_against_float64(deg):
    n, K = 20000, (deg + 1) ** 2 - 1
    g, c, q = make_model(n, deg, seed=20 + deg)
    sh_in = c["sh"].reshape(n, K, 3)
    g.transform_gaussian_model(T37, rotate_sh=True)
    assert g.get_xyz.is_cuda and g._features_rest.shape == (n, K, 3)
    assert worst(host(g.get_xyz), *ref_xyz(c["xyz"], T37), "xyz") <= 1.0
    assert worst(host(g.get_covariance(1)), *ref_cov(c["cov6"], T37), "cov") <= 1.0
    want_sh, bound_sh = ref_sh(sh_in, T37, deg)
    assert worst(host(g._features_rest), want_sh, bound_sh, f"sh degree {deg}") <= 1.0
    check_rot(host(g._rotation), q, T37, "rot")
    if deg:
        assert not np.array_equal(host(g._features_rest), sh_in)
    # colour invariance through the device: the moved splat seen from the moved direction shows the colour it had.  Exact for the
    # exact D; the float32 D adds at most (u/2)|D||c| per coefficient to the kernel's rounding, both inside the sh bound.
    d = np.random.default_rng(5).normal(size=(32, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y, YR = sh_basis_rest(d)[:, :K], sh_basis_rest(d @ T37[:3, :3].T)[:, :K]
    before = np.einsum("sk,nkc->nsc", Y, sh_in.astype(np.float64))
    after = np.einsum("sk,nkc->nsc", YR, host(g._features_rest).astype(np.float64))
    if deg:
        assert worst(after, before, np.einsum("sk,nkc->nsc", np.abs(YR), bound_sh), "colour") <= 1.0
    # host tensors are staged by the library and give the same bits
    gh, _, _ = make_model(n, deg, seed=20 + deg, device="cpu")
    gh.transform_gaussian_model(T37, rotate_sh=True)
    for name in ("_xyz", "_covariance", "_rotation", "_features_rest"):
        assert not getattr(gh, name).is_cuda and np.array_equal(host(getattr(gh, name)), host(getattr(g, name))), name


@pytest.mark.parametrize("deg", [1, 3])
def test_there_and_back(deg):
    n, K = 20000, (deg + 1) ** 2 - 1
    g, c, q = make_model(n, deg, seed=31)
    g.transform_gaussian_model(T37, rotate_sh=True)
    g.transform_gaussian_model(np.linalg.inv(T37), rotate_sh=True)
    _, bx = ref_xyz(c["xyz"], T37)
    _, bc = ref_cov(c["cov6"], T37)
    _, bs = ref_sh(c["sh"].reshape(n, K, 3), T37, deg)
    assert worst(host(g.get_xyz), c["xyz"].astype(np.float64), 2 * bx, "xyz there and back") <= 1.0
    assert worst(host(g.get_covariance(1)), c["cov6"].astype(np.float64), 2 * bc, "cov there and back") <= 1.0
    assert worst(host(g._features_rest), c["sh"].reshape(n, K, 3).astype(np.float64), 2 * bs, "sh there and back") <= 1.0


@pytest.mark.parametrize("deg", [0, 2, 3])
def test_rotate_sh_off_copies_the_bits(deg):
    n = 20000
    g, c, q = make_model(n, deg, seed=41)
    special = np.array([np.nan, -0.0, np.inf, 1e-42], np.float32)     # a copy, not arithmetic: NaN payloads, signed zeros and denormals survive
    sh = c["sh"].copy()
    if sh.size:
        sh.reshape(-1)[:4] = special
        g._features_rest = torch.from_numpy(sh.reshape(n, -1, 3)).to("cuda:0")
    g.transform_gaussian_model(T37)                                   # CUDA tensors: the kernel, rotate_sh=False
    assert np.array_equal(host(g._features_rest).view(np.uint32).reshape(-1), sh.view(np.uint32).reshape(-1))
    assert worst(host(g.get_xyz), *ref_xyz(c["xyz"], T37), "xyz") <= 1.0
    assert worst(host(g.get_covariance(1)), *ref_cov(c["cov6"], T37), "cov") <= 1.0
    check_rot(host(g._rotation), q, T37, "rot")


def test_edge_arguments(hip_lib):
    """K = 0, n = 0, a NULL quaternion array: fine.  Outputs that overlap inputs, a K that is no SH degree, a scaled matrix:
    GSR_E_INVALID."""
    n = 777
    c = synth.make_cloud(n, seed=3, sh_degree=1)
    T = np.ascontiguousarray(T37)
    p = lambda a: a.ctypes.data
    ox, oc, oq, osh = (np.full(s, np.nan, np.float32) for s in ((n, 3), (n, 6), (n, 4), (n, 9)))
    call = lambda *a: hip_lib.gsr_model_transform(p(T), *a, 0, 0, None)
    assert call(n, 0, 1, p(c["xyz"]), p(c["cov6"]), None, None, p(ox), p(oc), None, None) == 0, hip_lib.gsr_last_error()
    assert worst(ox, *ref_xyz(c["xyz"], T37), "xyz, K = 0, no rot") <= 1.0 and worst(oc, *ref_cov(c["cov6"], T37), "cov") <= 1.0
    assert call(0, 3, 1, None, None, None, None, None, None, None, None) == 0
    assert call(n, 3, 1, p(c["xyz"]), p(c["cov6"]), None, p(c["sh"]), p(ox), p(oc), None, p(osh)) == 0
    assert worst(osh.reshape(n, 3, 3), *ref_sh(c["sh"].reshape(n, 3, 3), T37, 1), "sh, no rot") <= 1.0 and np.isnan(oq).all()
    for bad in ((n, 3, 1, p(c["xyz"]), p(c["cov6"]), None, p(c["sh"]), p(c["xyz"]), p(oc), None, p(osh)),          # in place
                (n, 3, 1, p(c["xyz"]), p(c["cov6"]), None, p(c["sh"]), p(ox), p(oc), None, p(c["sh"]) + 36 * (n - 1)),  # tail of the input
                (n, 3, 1, p(c["xyz"]), p(c["cov6"]), None, p(c["sh"]), p(ox), p(ox) + 4, None, p(osh)),             # two outputs
                (n, 4, 1, p(c["xyz"]), p(c["cov6"]), None, p(c["sh"]), p(ox), p(oc), None, p(osh)),
                (n, 3, 1, p(c["xyz"]), p(c["cov6"]), None, None, p(ox), p(oc), None, p(osh))):
        assert call(*bad) == -1 and b"gsr_model_transform" in hip_lib.gsr_last_error()
    S = np.ascontiguousarray(T37 * 1.01)
    assert hip_lib.gsr_model_transform(p(S), n, 0, 0, p(c["xyz"]), p(c["cov6"]), None, None, p(ox), p(oc), None, None, 0, 0, None) == -1


def test_past_2_to_24_rows():
    """The count a batched matmul faults at on this stack: 2^24 + 1000 splats of degree 1 (about 3 GB in and out).  The first row,
    the last and 10 000 sampled ones against float64."""
    n = (1 << 24) + 1000
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=gen, device="cuda:0", dtype=torch.float32)
    g = GaussianModel("cuda:0")
    g.sh_degree = 1
    g._xyz, g._covariance, g._rotation, g._features_rest = rnd(n, 3) * 5, rnd(n, 6) * 0.01, rnd(n, 4), rnd(n, 3, 3) * 0.1
    idx = np.unique(np.concatenate([[0, n - 1, (1 << 24) - 1, 1 << 24], np.random.default_rng(9).integers(0, n, 10000)]))
    ti = torch.from_numpy(idx).to("cuda:0")
    before = {k: host(getattr(g, k)[ti]) for k in ("_xyz", "_covariance", "_rotation", "_features_rest")}
    g.transform_gaussian_model(T37, rotate_sh=True)
    after = {k: host(getattr(g, k)[ti]) for k in before}
    assert len(g) == n
    assert worst(after["_xyz"], *ref_xyz(before["_xyz"], T37), "xyz") <= 1.0
    assert worst(after["_covariance"], *ref_cov(before["_covariance"], T37), "cov") <= 1.0
    assert worst(after["_features_rest"], *ref_sh(before["_features_rest"], T37, 1), "sh") <= 1.0
    check_rot(after["_rotation"], before["_rotation"], T37, "rot")


@pytest.mark.parametrize("rotate_sh", [True, False])
def test_merge_writes_into_the_merged_arrays(rotate_sh):
    n1, n2, deg = 20000, 12345, 3
    ga, ca, qa = make_model(n1, deg, seed=51)
    gb, cb, qb = make_model(n2, deg, seed=52)
    names = ("_xyz", "_rotation", "_scaling", "_features_dc", "_features_rest", "_opacity", "_covariance")
    keep = {k: host(getattr(ga, k)).copy() for k in names}
    m = GaussianModel.get_merged_gaussian_point_clouds(ga, gb, T37, rotate_sh=rotate_sh)
    assert len(m) == n1 + n2 and m.sh_degree == deg
    for k in names:
        assert getattr(m, k).is_cuda and getattr(m, k).shape[0] == n1 + n2, k
        assert np.array_equal(host(getattr(m, k))[n1:].view(np.uint32), host(getattr(gb, k)).view(np.uint32)), k      # gb: bit-equal
        assert np.array_equal(host(getattr(ga, k)).view(np.uint32), keep[k].view(np.uint32)), k                       # ga: untouched
    moved = ga.clone_gaussian().transform_gaussian_model(T37, rotate_sh=rotate_sh)
    for k in names:
        assert np.array_equal(host(getattr(m, k))[:n1].view(np.uint32), host(getattr(moved, k)).view(np.uint32)), k
    # and against the float64 evaluation, not against the code under test
    assert worst(host(m.get_xyz)[:n1], *ref_xyz(ca["xyz"], T37), "xyz") <= 1.0
    assert worst(host(m.get_covariance(1))[:n1], *ref_cov(ca["cov6"], T37), "cov") <= 1.0
    check_rot(host(m._rotation)[:n1], qa, T37, "rot")
    sh_in = ca["sh"].reshape(n1, 15, 3)
    if rotate_sh:
        assert worst(host(m._features_rest)[:n1], *ref_sh(sh_in, T37, deg), "sh") <= 1.0
    else:
        assert np.array_equal(host(m._features_rest)[:n1], sh_in)


def test_merge_without_rotation_and_scaling():
    """mixture levels built without decompose carry no _rotation / _scaling: those arrays are skipped"""
    ca, cb = synth.make_cloud(5000, seed=61, sh_degree=2), synth.make_cloud(3000, seed=62, sh_degree=2)
    mk = lambda c: GaussianModel("cuda:0").from_arrays(c["xyz"], c["color"], c["opacity"], c["cov6"], c["sh"], 2)
    ga, gb = mk(ca), mk(cb)
    m = GaussianModel.get_merged_gaussian_point_clouds(ga, gb, T37, rotate_sh=True)
    assert len(m) == 8000 and m._rotation.numel() == 0 and m._scaling.numel() == 0
    assert worst(host(m.get_xyz)[:5000], *ref_xyz(ca["xyz"], T37), "xyz") <= 1.0
    assert worst(host(m._features_rest)[:5000], *ref_sh(ca["sh"].reshape(5000, 8, 3), T37, 2), "sh") <= 1.0
    assert np.array_equal(host(m._features_rest)[5000:], cb["sh"].reshape(3000, 8, 3))
