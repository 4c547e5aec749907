"""Similarity (scaled) registration on the GPU: the kind-4 accumulate kernels, ICP with scaling through the device-resident and the
host loop, RANSAC with the scaled estimator, gsr_model_similarity, and scripts/register_ply.py --with-scaling end to end.
References: tests/sim3_model.py (float64 NumPy / SciPy) and tests/global_model.py's RANSAC driven with the scaled Umeyama.
Open3D is absent: parity with it is unpinned, like the rest of the ICP half.
"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import global_model as G
import sim3_model as M
import test_model_transform_gpu as MT
from gaussiansplattingregistration_amd import _lib, features, icp
from gaussiansplattingregistration_amd.utils.similarity_util import initial_similarity, split_similarity

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
KIND0, KIND4 = icp.KIND_POINT_TO_POINT, icp.KIND_POINT_TO_POINT_SCALED

# gsr_icp_register, kind 0, on the c = 0.8 pair of test_register below (identity start, max_corr 0.15, 50 iterations), as the commit
# before the scaled kind existed computed it: the rigid path must not have moved
PARENT_RIGID_T = ['0x1.fecbebf111e44p-1', '-0x1.e9cd99ee293cdp-5', '-0x1.12374728eaf00p-5', '0x1.0cc803399321ap-6',
                  '0x1.e2c1442a39010p-5', '0x1.feef64bb9f7bap-1', '-0x1.ac0c7cf4f9641p-6', '-0x1.16a97399507f3p-5',
                  '0x1.1e71352b08ebdp-5', '0x1.8ab93b221c300p-6', '0x1.ff89c825e5f22p-1', '0x1.31d88b40a85bap-5',
                  '0x0.0p+0', '0x0.0p+0', '0x0.0p+0', '0x1.0000000000000p+0']
PARENT_RIGID_ITERATIONS = 39


def _centre(ctx):
    c = np.zeros(3)
    _lib.check(ctx._L.gsr_icp_get_centre(ctx._h, c.ctypes.data), "gsr_icp_get_centre")
    return c


def _solve(acc, kind, centre):
    upd = np.zeros(16)
    _lib.check(_lib.load().gsr_icp_solve(acc.ctypes.data, kind, centre.ctypes.data, upd.ctypes.data), "gsr_icp_solve")
    return upd.reshape(4, 4)


# ------------------------------------------------------------------------------------------------------------- accumulate
@pytest.fixture(scope="module")
def target2000():
    return np.random.default_rng(11).random((2000, 3)).astype(np.float32)


@pytest.mark.parametrize("ns", [1, 63, 257, 3001])
def test_accumulate_slots(target2000, ns):
    """Kind 4 against kind 0 and float64 NumPy at T with c = 1.3: slots 0..16 bit for bit kind 0's, slot 17 = sum |T p - ctr|^2 over
    the matched pairs to 1e-12 relative (fewer than 3 001 positive float64 terms: reordering costs at most n 2^-53), slots 18..31
    zero.  Every second source point lies 1e-3 from a target point, the others anywhere in the box: 40-70 % match at max_corr 0.03."""
    tgt = target2000
    rng = np.random.default_rng(100 + ns)
    T = M.similarity(1.3, 5.0, (0.2, 1.0, -0.3), (0.05, -0.02, 0.03))
    moved = tgt[rng.integers(0, len(tgt), ns)].astype(np.float64) + 1e-3 * rng.normal(size=(ns, 3))
    far = np.arange(ns) % 2 == 1
    moved[far] = rng.random((int(far.sum()), 3))
    src = ((moved - T[:3, 3]) @ np.linalg.inv(T[:3, :3]).T).astype(np.float32)
    max_corr = 0.03
    ctx = icp.IcpContext(device=0)
    try:
        ctx.set_target(tgt, None, max_corr)
        ctx.set_source(src)
        a0, a4 = ctx.accumulate(T, KIND0), ctx.accumulate(T, KIND4)
        ctr = _centre(ctx)
    finally:
        ctx.close()
    p = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    d, j = cKDTree(tgt.astype(np.float64)).query(p, k=1)
    m = d * d < max_corr * max_corr
    frac = m.mean()
    print(f"ns {ns}: matched {int(m.sum())} ({100 * frac:.1f} %), kind-4 count {a4[0]:.0f}")
    assert ns < 63 or 0.4 <= frac <= 0.7
    assert a4[0] == m.sum()
    assert a4[:17].tobytes() == a0[:17].tobytes()
    want = float((((p[m] - ctr) ** 2).sum(1)).sum())
    rel = abs(a4[17] - want) / want
    print(f"slot 17: {a4[17]!r} against {want!r}, relative {rel:.2e}")
    assert rel <= 1e-12
    assert not a4[18:].any() and not a0[17:].any()


# --------------------------------------------------------------------------------------------------------------- register
def _pair(c):
    """target: 2 000 points; source = the target moved by the inverse of a similarity (5 degrees, translation of 0.05 extent, c)"""
    tgt = (np.random.default_rng(21).random((2000, 3)) - 0.5).astype(np.float32)
    T_gt = M.similarity(c, 5.0, (0.3, -0.5, 1.0), (0.03, -0.05, 0.04))
    src = ((tgt.astype(np.float64) - T_gt[:3, 3]) @ np.linalg.inv(T_gt[:3, :3]).T).astype(np.float32)
    return src, tgt, T_gt


MAX_CORR, MAX_ITER = 0.15, 50


@pytest.fixture(scope="module")
def model_runs():
    """the float64 model's registration of both pairs, computed once"""
    out = {}
    for c in (0.8, 1.25):
        src, tgt, T_gt = _pair(c)
        init = initial_similarity(src, tgt)
        out[c] = (src, tgt, T_gt, init, M.icp(src, tgt, init, MAX_CORR, MAX_ITER, with_scaling=True))
    return out


@pytest.mark.parametrize("c", [0.8, 1.25])
def test_register(model_runs, c):
    """ICP with scaling from initial_similarity, through gsr_icp_register and through do_icp_registration(with_scaling=True): the
    model's iteration count, its T to 1e-9 (the project's GPU-versus-oracle bar for ICP), the true c to 1e-6; the host loop
    (gsr_icp_accumulate + gsr_icp_solve repeated) agrees with the device-resident loop to 1e-12."""
    from gaussiansplattingregistration_amd.models.point_cloud import PointCloud
    from gaussiansplattingregistration_amd.utils import local_registration_util as L
    src, tgt, T_gt, init, (Tm, fitm, rmsem, itm) = model_runs[c]
    assert 0 < itm < MAX_ITER and abs(M.scale_of(Tm) - c) <= 1e-6
    ctx = icp.IcpContext(device=0)
    try:
        ctx.set_target(tgt, None, MAX_CORR)
        ctx.set_source(src)
        r = ctx.register(init, KIND4, max_iter=MAX_ITER)
        # the host loop, written out
        ctr = _centre(ctx)
        T = init.copy()
        acc = ctx.accumulate(T, KIND4)
        fit, rmse, it = acc[0] / len(src), math.sqrt(acc[1] / acc[0]), 0
        while it < MAX_ITER:
            T = _solve(acc, KIND4, ctr) @ T
            it += 1
            acc = ctx.accumulate(T, KIND4)
            fit2, rmse2 = acc[0] / len(src), math.sqrt(acc[1] / acc[0])
            stop = abs(fit - fit2) < 1e-6 and abs(rmse - rmse2) < 1e-6
            fit, rmse = fit2, rmse2
            if stop:
                break
    finally:
        ctx.close()
    Td = r["transformation"]
    print(f"c {c}: iterations device {r['iterations']} host {it} model {itm}; |T - model| {np.abs(Td - Tm).max():.2e}; "
          f"|host - device| {np.abs(T - Td).max():.2e}; c {M.scale_of(Td)!r}")
    assert r["iterations"] == itm and it == itm
    assert np.abs(Td - Tm).max() <= 1e-9 and abs(r["fitness"] - fitm) <= 1e-12 and abs(r["inlier_rmse"] - rmsem) <= 1e-9
    assert abs(M.scale_of(Td) - c) <= 1e-6
    assert np.abs(T - Td).max() <= 1e-12
    res = L.do_icp_registration(PointCloud(xyz32=src), PointCloud(xyz32=tgt), init, L.LocalRegistrationType.ICP_Point_To_Point, MAX_CORR, 1e-6, 1e-6,
                                MAX_ITER, L.KernelLossFunctionType.Loss_None, 0.0, with_scaling=True)
    assert res.iterations == itm and np.abs(res.transformation - Tm).max() <= 1e-9 and abs(split_similarity(res.transformation)[0] - c) <= 1e-6


def test_rigid_kind_unchanged(model_runs):
    """Kind 0 on the c = 0.8 pair from the identity: the transform the parent commit computed, to the bit."""
    src, tgt = model_runs[0.8][:2]
    ctx = icp.IcpContext(device=0)
    try:
        ctx.set_target(tgt, None, MAX_CORR)
        ctx.set_source(src)
        r = ctx.register(np.eye(4), KIND0, max_iter=MAX_ITER)
    finally:
        ctx.close()
    print("rigid T:", [float.hex(float(v)) for v in r["transformation"].reshape(-1)], "iterations", r["iterations"])
    assert r["iterations"] == PARENT_RIGID_ITERATIONS
    assert [float.hex(float(v)) for v in r["transformation"].reshape(-1)] == PARENT_RIGID_T


def test_no_correspondences(target2000):
    """A source far from the target: identity updates, fitness 0, nothing worse."""
    src = (target2000[:500] + np.float32(100.0)).astype(np.float32)
    init = M.similarity(1.1, 3.0, (0, 0, 1), (0.01, 0.0, 0.0))
    ctx = icp.IcpContext(device=0)
    try:
        ctx.set_target(target2000, None, 0.05)
        ctx.set_source(src)
        acc = ctx.accumulate(init, KIND4)
        r = ctx.register(init, KIND4, max_iter=5)
    finally:
        ctx.close()
    assert not acc.any()
    assert np.array_equal(r["transformation"], init) and r["fitness"] == 0.0 and r["inlier_rmse"] == 0.0


# ----------------------------------------------------------------------------------------------------------------- RANSAC
def test_ransac_scaled(monkeypatch):
    """300 correspondences, 30 % random outliers, c = 1.5, ransac_n = 3, the distance checker only, a fixed seed: T, best_index,
    n_valid and fitness are those of tests/global_model.py's serial rule replaying the same draws with the scaled Umeyama; T within
    the bound of the host-solve test (4 x kind 0's worst deviation from NumPy's rigid Umeyama); the inlier sets are equal."""
    import test_sim3_cpu as CPU
    rng = np.random.default_rng(5)
    m = 300
    P = (rng.random((m, 3)) - 0.5).astype(np.float32)
    T_gt = M.similarity(1.5, 40.0, (0.5, 0.2, -1.0), (0.2, -0.1, 0.3))
    Q = P.astype(np.float64) @ T_gt[:3, :3].T + T_gt[:3, 3] + 0.002 * rng.normal(size=(m, 3))
    out = rng.permutation(m)[: int(0.3 * m)]
    Q[out] = (rng.random((len(out), 3)) - 0.5) * 2.0
    Q = Q.astype(np.float32)
    corres = np.stack([np.arange(m), np.arange(m)], 1).astype(np.int32)
    kw = dict(max_corr=0.02, ransac_n=3, checkers=[(G.DIST, 0.02)], max_iteration=4000, confidence=0.999, seed=12345)
    got = features.ransac_correspondence(P, Q, corres, kind=features.KIND_POINT_TO_POINT_SCALED, batch=512, **kw)
    monkeypatch.setattr(G, "umeyama", lambda p, q: M.umeyama(p, q, with_scaling=True))
    want = G.ransac(P, Q, corres, kind=0, batch=512, **kw)
    bound = 4.0 * CPU._deviation(_lib.load(), 0)
    dT = np.abs(got["transformation"] - want["transformation"]).max()
    print(f"best {got['best_index']} / {want['best_index']}, valid {got['n_valid']} / {want['n_valid']}, fitness {got['fitness']}, "
          f"|dT| {dT:.2e}, bound {bound:.2e}, c {M.scale_of(got['transformation']):.6f}")
    assert want["best_index"] >= 0 and want["fitness"] > 0.5
    for k in ("best_index", "n_valid", "n_evaluated", "exit_index", "fitness"):
        assert got[k] == want[k], k
    assert dT <= bound

    def inliers(T):
        p, q = P.astype(np.float64), Q.astype(np.float64)
        x = [T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1] + T[r, 2] * p[:, 2] + T[r, 3] for r in range(3)]
        d2 = (x[0] - q[:, 0]) ** 2 + (x[1] - q[:, 1]) ** 2 + (x[2] - q[:, 2]) ** 2
        return d2 < 0.02 * 0.02
    assert np.array_equal(inliers(got["transformation"]), inliers(want["transformation"]))
    assert inliers(got["transformation"]).sum() == round(got["fitness"] * m)


# ------------------------------------------------------------------------------------------------------------------ model
def _raw_similarity(T, n, K, rotate_sh, a, o, on_device):
    """gsr_model_similarity on dicts of numpy arrays (host) or CUDA tensors (device)"""
    p = (lambda t: None if t is None else t.data_ptr()) if on_device else (lambda t: None if t is None else t.ctypes.data)
    T = np.ascontiguousarray(T, np.float64)
    if on_device:
        torch.cuda.synchronize()
    rc = _lib.load().gsr_model_similarity(T.ctypes.data, n, K, 1 if rotate_sh else 0, p(a["xyz"]), p(a["cov6"]), p(a["rot"]), p(a["sh"]), p(a["scaling"]),
                                          p(o["xyz"]), p(o["cov6"]), p(o["rot"]), p(o["sh"]), p(o["scaling"]), 1 if on_device else 0, 0, None)
    _lib.check(rc, "gsr_model_similarity")
    if on_device:
        torch.cuda.synchronize()


@pytest.mark.parametrize("K", [0, 3, 15])
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_model_similarity(n, K):
    """gsr_model_similarity against the float64 model with the kernel's float32 constants, rotate_sh on and off, c in {0.5, 2}.
    Bounds as tests/test_model_transform_gpu.py counts them (twice the worst-case rounding, u = 2^-24), one multiply more each:
        xyz  3 products + the multiply by c + t: 5 roundings      |d| <= 10 u (c |R||x| + |t|)      (rigid: 8 u)
        cov  two 3-term products + the multiply by c^2            |d| <= 18 u (c^2 |R||S||R^T|)     (rigid: 16 u)
        sh   unchanged: 16 u (|D||c|);  rot: the rigid test's 1e-5 on the rotation matrix
    scaling_out is the float32 sum scaling + float32(ln c), bit for bit; untouched arrays are not arguments (opacity, DC), SH is
    bit-equal with rotate_sh off; outputs land in the middle of larger arrays whose other rows keep their bits; host and device
    calls agree bit for bit; a c = 1 matrix gives gsr_model_transform's values."""
    deg = {0: 0, 3: 1, 15: 3}[K]
    rng = np.random.default_rng(1000 * n + K)
    a = {"xyz": rng.normal(size=(n, 3)).astype(np.float32), "rot": rng.normal(size=(n, 4)).astype(np.float32),
         "scaling": rng.normal(-2.5, 0.5, (n, 3)).astype(np.float32), "sh": (0.1 * rng.normal(size=(n, K, 3))).astype(np.float32) if K else None}
    L = rng.normal(size=(n, 3, 3)) * 0.05
    a["cov6"] = np.ascontiguousarray(M.six(L @ L.transpose(0, 2, 1)), dtype=np.float32)      # (fancy indexing returns a transposed layout)
    cols = {"xyz": 3, "cov6": 6, "rot": 4, "scaling": 3, "sh": 3 * K}
    PAD, SENT = 3, np.float32(-7.25)
    for c in (0.5, 2.0):
        T = M.similarity(c, 37.0, (0.4, -1.0, 0.7), (0.3, -0.2, 0.15))
        TR = np.eye(4)
        TR[:3, :3] = split_similarity(T)[1]
        want = M.model_similarity(T, a["xyz"], a["cov6"], a["rot"], a["scaling"])
        for rotate in (False, True):
            ho = {k: (np.full((n, cols[k]), SENT, np.float32) if a[k] is not None else None) for k in cols}
            _raw_similarity(T, n, K, rotate, a, ho, False)
            da = {k: (torch.from_numpy(v).cuda() if v is not None else None) for k, v in a.items()}
            big = {k: (torch.full((n + 2 * PAD, cols[k]), float(SENT), device="cuda") if a[k] is not None else None) for k in cols}
            do = {k: (v[PAD:PAD + n] if v is not None else None) for k, v in big.items()}
            _raw_similarity(T, n, K, rotate, da, do, True)
            for k in cols:
                if a[k] is None:
                    continue
                b = big[k].cpu().numpy()
                assert (b[:PAD] == SENT).all() and (b[PAD + n:] == SENT).all(), k                       # the rows around: untouched
                assert b[PAD:PAD + n].tobytes() == ho[k].tobytes(), k                                      # host == device, bit for bit
            what = f"n {n} K {K} c {c} rotate {rotate}"
            assert MT.worst(ho["xyz"], want["xyz"], 10 * U * want["abs_xyz"], what + " xyz") <= 1.0
            assert MT.worst(ho["cov6"], want["cov6"], 18 * U * want["abs_cov"], what + " cov") <= 1.0
            MT.check_rot(ho["rot"], a["rot"], TR, what + " rot")
            lnc32 = np.float32(math.log(c))
            assert np.float32(want["lnc"]) == lnc32
            assert (ho["scaling"] == a["scaling"] + lnc32).all()                                          # float32 sum, exact
            if K:
                if rotate:
                    sh_want, sh_bound = MT.ref_sh(a["sh"], TR, deg)
                    assert MT.worst(ho["sh"].reshape(n, K, 3), sh_want, sh_bound, what + " sh") <= 1.0
                else:
                    assert ho["sh"].tobytes() == a["sh"].tobytes()
    # c = 1: the rigid entry's values (== : a negative zero may change sign)
    T1 = M.similarity(1.0, 37.0, (0.4, -1.0, 0.7), (0.3, -0.2, 0.15))
    hs = {k: (np.zeros((n, cols[k]), np.float32) if a[k] is not None else None) for k in cols}
    hr = {k: (np.zeros((n, cols[k]), np.float32) if a[k] is not None else None) for k in cols}
    _raw_similarity(T1, n, K, True, a, hs, False)
    p = lambda t: None if t is None else t.ctypes.data
    _lib.check(_lib.load().gsr_model_transform(np.ascontiguousarray(T1).ctypes.data, n, K, 1, p(a["xyz"]), p(a["cov6"]), p(a["rot"]), p(a["sh"]), p(hr["xyz"]),
                                               p(hr["cov6"]), p(hr["rot"]), p(hr["sh"]), 0, 0, None), "gsr_model_transform")
    for k in ("xyz", "cov6", "rot", "sh"):
        if a[k] is not None:
            assert (hs[k] == hr[k]).all(), k
    assert (hs["scaling"] == a["scaling"]).all()


def test_gaussian_model_similarity_and_merge():
    """The Python surface on a GaussianModel: similarity_transform_gaussian_model moves _scaling too; the merge with
    with_scaling=True writes the same rows; opacity and DC keep their bits; the rigid entry refuses the matrix."""
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    g, c0, q = MT.make_model(700, 3, seed=4)
    g2, _, _ = MT.make_model(300, 3, seed=5)
    T = M.similarity(1.7, 20.0, (1, 0.3, 0.2), (0.5, 0.1, -0.2))
    with pytest.raises(RuntimeError):
        g.clone_gaussian().transform_gaussian_model(T, rotate_sh=True)
    moved = g.clone_gaussian().similarity_transform_gaussian_model(T, rotate_sh=True)
    assert (MT.host(moved._scaling) == MT.host(g._scaling) + np.float32(math.log(1.7))).all()
    assert torch.equal(moved._opacity, g._opacity) and torch.equal(moved._features_dc, g._features_dc)
    merged = GaussianModel.get_merged_gaussian_point_clouds(g, g2, T, rotate_sh=True, with_scaling=True)
    assert len(merged) == 1000
    for name in ("_xyz", "_covariance", "_rotation", "_scaling", "_features_rest", "_opacity", "_features_dc"):
        assert torch.equal(getattr(merged, name)[:700], getattr(moved, name)), name
        assert torch.equal(getattr(merged, name)[700:], getattr(g2, name)), name
    host = g.clone_gaussian()
    host.move_to_device("cpu")
    host.similarity_transform_gaussian_model(T, rotate_sh=True)               # host tensors: staged by the library, the same kernel
    assert np.array_equal(MT.host(host._xyz), MT.host(moved._xyz)) and np.array_equal(MT.host(host._scaling), MT.host(moved._scaling))


@pytest.mark.parametrize("with_scaling_array", [True, False])
def test_pairwise_merge_is_the_multi_merge(with_scaling_array):
    """Two models on one device, 257 and 130 rows (more than one 256-thread block, an odd tail), K = 3, with and without _scaling:
    the rigid pairwise merge is bit for bit get_merged_gaussian_point_clouds_multi([g1, g2], [T, I]), and with with_scaling=True
    it is similarity_transform_gaussian_model followed by concatenation."""
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    names = ("_xyz", "_covariance", "_rotation", "_scaling", "_features_rest", "_opacity", "_features_dc")
    g1, _, _ = MT.make_model(257, 1, seed=7)
    g2, _, _ = MT.make_model(130, 1, seed=8)
    if not with_scaling_array:
        g1._scaling, g2._scaling = torch.empty(0), torch.empty(0)
    before = {k: getattr(g1, k).clone() for k in names}
    R = M.similarity(1.0, 33.0, (0.3, 1.0, -0.2), (0.2, -0.4, 0.1))
    pair = GaussianModel.get_merged_gaussian_point_clouds(g1, g2, R, rotate_sh=True)
    multi = GaussianModel.get_merged_gaussian_point_clouds_multi([g1, g2], [R, np.eye(4)], rotate_sh=True)
    S = M.similarity(1.7, 33.0, (0.3, 1.0, -0.2), (0.2, -0.4, 0.1))
    scaled = GaussianModel.get_merged_gaussian_point_clouds(g1, g2, S, rotate_sh=True, with_scaling=True)
    moved = g1.clone_gaussian().similarity_transform_gaussian_model(S, rotate_sh=True)
    assert len(pair) == len(multi) == len(scaled) == 387 and pair.sh_degree == scaled.sh_degree == 1
    for k in names:
        a, b, c = getattr(pair, k), getattr(multi, k), getattr(scaled, k)
        assert a.shape == b.shape and torch.equal(a, b), k
        want = torch.cat((getattr(moved, k).to(c.device), getattr(g2, k).to(c.device)))
        assert c.shape == want.shape and torch.equal(c, want), k
        assert torch.equal(getattr(g1, k), before[k]), k                                              # the input is left as it was
    assert (pair._scaling.numel() > 0) == with_scaling_array and not torch.equal(scaled._xyz[:257], pair._xyz[:257])
    if with_scaling_array:
        assert torch.equal(pair._scaling[:257], g1._scaling) and not torch.equal(scaled._scaling[:257], g1._scaling)


# --------------------------------------------------------------------------------------------------------------- pipeline
def test_register_ply_with_scaling(tmp_path):
    """scripts/register_ply.py --with-scaling as a child process on two 20 000-splat models, the second the first scaled by 1.2 and
    moved: n1 + n2 rows in the merged file, the moved cloud's scale_* columns = the input's + ln c of the printed transform (to
    two float32 units in the last place: the printed scale has nine decimals), and c within 1e-3 of 1.2 -- loose, because the HEM
    levels of a scaled cloud are not the scaled levels: this checks the plumbing, not the accuracy."""
    from conftest import ROOT
    from gaussiansplattingregistration_amd.utils import ply_io
    n = 20000
    sc = G.make_scene(n, 1)
    n = len(sc["xyz"])
    T_gt = M.similarity(1.2, 5.0, (0.2, 0.3, 1.0), (0.05, -0.03, 0.04))
    sb = G.transform_scene(sc, T_gt)
    sb["frames"] = split_similarity(T_gt)[1][None] @ sc["frames"]
    sb["log_scale"] = sc["log_scale"] + math.log(1.2)
    pa, pb, pm = tmp_path / "first.ply", tmp_path / "second.ply", tmp_path / "merged.ply"
    G.save_scene_ply(str(pa), sc)
    G.save_scene_ply(str(pb), sb)
    script = os.path.join(ROOT, "scripts", "register_ply.py")
    r = subprocess.run([sys.executable, script, str(pa), str(pb), "--with-scaling", "--levels", "2", "--max-corr", "0.3", "0.15", "0.08", "--iters", "40",
                        "30", "20", "--out", str(pm)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    rows = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("[") or ln.strip().startswith("[[")]
    T = np.array([[float(x) for x in ln.replace("[", " ").replace("]", " ").split()] for ln in rows[:4]])
    c = float([ln for ln in r.stdout.splitlines() if ln.startswith("scale ")][0].split()[1])
    assert T.shape == (4, 4) and abs(M.scale_of(T) - c) <= 1e-5
    assert abs(c - 1.2) <= 1e-3, c
    merged, first = ply_io.load_gaussian_arrays(str(pm)), ply_io.load_gaussian_arrays(str(pa))
    assert len(merged["xyz"]) == 2 * n
    want = first["scale"].astype(np.float64) + math.log(c)
    assert np.abs(merged["scale"][:n].astype(np.float64) - want).max() <= 2 * 2.0 ** -23 * np.abs(want).max()
    assert np.array_equal(merged["scale"][n:], ply_io.load_gaussian_arrays(str(pb))["scale"])
    r = subprocess.run([sys.executable, script, str(pa), str(pb), "--with-scaling", "--type", "plane"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "point-to-point only" in r.stderr
