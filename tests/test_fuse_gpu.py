"""gsr_model_fuse on the GPU against the float64 model (tests/fuse_model.py).

Every case is unambiguous under the model (tests/test_fuse_cpu.py asserts it), so the pair list and the counts must be EQUAL, the
unpaired rows and the block order equal bit for bit, and a fused row within one rounding of the model's:
    |got - float32(model)| <= 2^-23 x (that row's largest magnitude in that array)
(both sides round one float64 result once; the two float64 results differ by ~1e-15 relative, which can move a value across one
float32 rounding boundary: one ulp of the row's largest entry covers it).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fuse_model as F
from conftest import ROOT
from gaussiansplattingregistration_amd import synth
from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
from gaussiansplattingregistration_amd.params import FuseOverlapParams

pytestmark = pytest.mark.gpu

ATTR = {"xyz": "_xyz", "cov6": "_covariance", "dc": "_features_dc", "sh": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rot": "_rotation"}


def to_model(M, device):
    n = len(M["xyz"])
    K = M["sh"].shape[1] // 3
    deg = {0: 0, 3: 1, 8: 2, 15: 3}[K]
    g = GaussianModel(device).from_arrays(M["xyz"], M["dc"], M["opacity"].reshape(n, 1), M["cov6"], M["sh"].reshape(n, K, 3), deg)
    if "scaling" in M:
        g._scaling = torch.as_tensor(M["scaling"], device=device)
        g._rotation = torch.as_tensor(M["rot"], device=device)
    return g


def arrays_of(m):
    """the model's tensors as (n, width) float32 numpy arrays"""
    n = len(m)
    out = {}
    for k, attr in ATTR.items():
        t = getattr(m, attr)
        if t.numel() == 0 and t.dim() < 2:
            continue
        out[k] = t.detach().cpu().numpy().reshape(n, -1)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def reconstruct(scaling, rot):
    R = synth._quat_to_rot(rot.astype(np.float64))
    C = (R * np.exp(2.0 * scaling.astype(np.float64))[:, None, :]) @ R.transpose(0, 2, 1)
    return C[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]


def run(name, device="cuda:0"):
    A, B, gates, want = F.case(name)
    m, info = GaussianModel.fuse_overlap(to_model(A, device), to_model(B, device), FuseOverlapParams(*gates))
    return A, B, want, m, info


def check(want, m, info):
    for k in ("n_out", "n_pairs", "n_a_only", "n_b_only", "n_invalid_a", "n_invalid_b"):
        assert info[k] == want[k], (k, info[k], want[k])
    assert np.array_equal(info["pairs"].cpu().numpy(), want["pairs"])
    assert len(m) == want["n_out"]
    got = arrays_of(m)
    a0, p0 = want["n_a_only"], want["n_a_only"] + want["n_pairs"]
    for k, g in got.items():
        w = np.asarray(want[k], np.float32).reshape(want["n_out"], -1)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.array_equal(bits(g[:a0]), bits(w[:a0])), k                      # A rows not in a pair, in order, bit for bit
        assert np.array_equal(bits(g[p0:]), bits(w[p0:])), k                      # B rows not in a pair
        if k in ("scaling", "rot") or want["n_pairs"] == 0 or g.shape[1] == 0:
            continue
        err = np.abs(g[a0:p0].astype(np.float64) - w[a0:p0].astype(np.float64))
        bound = 2.0 ** -23 * np.abs(w[a0:p0].astype(np.float64)).max(1, keepdims=True)
        assert (err <= bound).all(), (k, float((err / np.maximum(bound, 1e-300)).max()))
    if "scaling" in got and want["n_pairs"]:
        s, q, c = got["scaling"][a0:p0], got["rot"][a0:p0], got["cov6"][a0:p0].astype(np.float64)
        assert np.abs(np.linalg.norm(q.astype(np.float64), axis=1) - 1).max() < 1e-6
        rel = np.abs(reconstruct(s, q) - c).max(1) / np.abs(c).max(1)
        assert rel.max() < 1e-5, rel.max()
    return got


@pytest.mark.parametrize("name", [c for c in F.CASES if c not in ("scaling_rot", "large")])
def test_case_equals_the_model(name):
    A, B, want, m, info = run(name)
    check(want, m, info)
    if name == "no_overlap":                                # the concatenation, bit for bit
        got = arrays_of(m)
        for k in ("xyz", "cov6", "dc", "sh", "opacity"):
            cat = np.concatenate([A[k].reshape(len(A["xyz"]), -1), B[k].reshape(len(B["xyz"]), -1)])
            assert np.array_equal(bits(got[k]), bits(cat)), k
    if name == "ties":                                      # only the lowest-index twin pairs; the other copies pass through
        assert np.array_equal(info["pairs"].cpu().numpy(), np.stack([np.arange(250), np.arange(250)], 1))
    if name == "invalid":
        pairs = info["pairs"].cpu().numpy()
        assert info["n_invalid_a"] == 4 and info["n_invalid_b"] == 4
        assert not set(pairs[:, 0]) & {3, 40, 77, 130} and not set(pairs[:, 1]) & {3, 41, 200, 499}
    if name == "one_pairs":
        assert info["n_pairs"] == 1 and len(m) == 1
    if name == "one_apart":
        assert info["n_pairs"] == 0 and len(m) == 2


def test_far_outliers_do_not_size_the_allocation():
    """five rows of each model at 500 x the scene extent: what the call allocates is a few hundred bytes per row (about 200 per row of A,
    80 per row of B, the table of max(na, 1024) cells, rocPRIM's temporaries), not a table over the extent -- at edge 0.25 that would
    be (1000 h / 0.25)^3 = 2e9 cells"""
    A, B, want, m, info = run("outliers")
    check(want, m, info)
    assert 0 < info["workspace_bytes"] <= 400 * (len(A["xyz"]) + len(B["xyz"])) + (1 << 20), info["workspace_bytes"]
    _, _, _, _, plain = run("base0")
    assert info["workspace_bytes"] <= plain["workspace_bytes"]        # (base0 has four times the rows)


def test_more_rows_than_one_pass_of_the_grids():
    """600 000 + 600 000 rows (K = 0): more than the 2048 x 256 threads a launch has, so every grid-stride loop takes a second trip
    (the ballot in the pre-pass included), the table has more than 1024 cells, the sort keys more than 11 bits, and the box (8.6 units
    at edge 0.06) makes the cell edge grow.  Against the model, like every other case."""
    A, B, gates, want = F.case("large")
    assert not want["ambiguous"] and want["n_pairs"] > 250000
    m, info = GaussianModel.fuse_overlap(to_model(A, "cuda:0"), to_model(B, "cuda:0"), FuseOverlapParams(*gates))
    check(want, m, info)
    assert info["gated_pairs"] == want["n_gated"]


def test_host_and_device_arrays_and_two_runs_give_the_same_bits():
    _, _, want, m_dev, i_dev = run("base1", "cuda:0")
    _, _, _, m_host, i_host = run("base1", "cpu")
    _, _, _, m_again, i_again = run("base1", "cuda:0")
    assert not m_host._xyz.is_cuda and m_dev._xyz.is_cuda
    d, h, a = arrays_of(m_dev), arrays_of(m_host), arrays_of(m_again)
    for k in d:
        assert np.array_equal(bits(d[k]), bits(h[k])), k
        assert np.array_equal(bits(d[k]), bits(a[k])), k
    assert torch.equal(i_dev["pairs"].cpu(), i_host["pairs"]) and torch.equal(i_dev["pairs"], i_again["pairs"])
    # the result tensors are views of arrays allocated for na + nb rows
    assert m_dev._xyz.untyped_storage().nbytes() >= 4000 * 12 and len(m_dev) == want["n_out"] < 4000


def test_models_with_scaling_and_rotation(tmp_path):
    A, B, want, m, info = run("scaling_rot")
    got = check(want, m, info)                              # unpaired rows keep theirs bit for bit, fused rows reproduce their covariance
    assert want["n_pairs"] > 100
    p = tmp_path / "fused.ply"
    m.save_ply(str(p))
    back = GaussianModel("cpu").from_ply(str(p))
    assert len(back) == want["n_out"]
    for k in ("xyz", "dc", "sh", "opacity", "scaling", "rot"):
        assert np.array_equal(bits(arrays_of(back)[k]), bits(got[k])), k
    a0, p0 = want["n_a_only"], want["n_a_only"] + want["n_pairs"]
    c = got["cov6"][a0:p0].astype(np.float64)
    assert (np.abs(arrays_of(back)["cov6"][a0:p0] - c).max(1) / np.abs(c).max(1)).max() < 1e-5


def test_merge_with_fuse_end_to_end(tmp_path):
    A, B, _ = F.base_pair(2000)
    T = synth.rigid_transform(20.0, (0.3, 1.0, -0.5), (0.2, -0.1, 0.05))
    params = FuseOverlapParams(0.25, 0.5, 0.2)
    g2 = to_model(B, "cuda:0")
    # g1 = A moved by inv(T) with its SH turned along, so that T brings it back into B's frame
    g1 = to_model(A, "cuda:0").transform_gaussian_model(np.linalg.inv(T), rotate_sh=True)
    merged = GaussianModel.get_merged_gaussian_point_clouds(g1, g2, T, rotate_sh=True, fuse=params)
    moved = g1.clone_gaussian().transform_gaussian_model(T, rotate_sh=True)
    want, info = GaussianModel.fuse_overlap(moved, g2, params)
    assert info["n_pairs"] > 900 and len(merged) == 4000 - info["n_pairs"]
    for k, v in arrays_of(want).items():
        assert np.array_equal(bits(arrays_of(merged)[k]), bits(v)), k
    # fuse=None is today's result, bit for bit
    plain = GaussianModel.get_merged_gaussian_point_clouds(g1, g2, T, rotate_sh=True)
    plain_none = GaussianModel.get_merged_gaussian_point_clouds(g1, g2, T, rotate_sh=True, fuse=None)
    assert len(plain) == 4000
    for k, v in arrays_of(plain).items():
        assert np.array_equal(bits(arrays_of(plain_none)[k]), bits(v)), k
        cat = torch.cat((getattr(moved, ATTR[k]), getattr(g2, ATTR[k]))).cpu().numpy().reshape(4000, -1)
        assert np.array_equal(bits(v), bits(cat)), k
    # an average of SH rows in two frames means nothing
    with pytest.raises(RuntimeError, match="rotate_sh"):
        GaussianModel.get_merged_gaussian_point_clouds(g1, g2, T, rotate_sh=False, fuse=params)
    # a pure translation does not turn anything: allowed without rotate_sh
    shift = np.eye(4)
    shift[:3, 3] = (1e-3, 0.0, 0.0)
    assert len(GaussianModel.get_merged_gaussian_point_clouds(moved, g2, shift, rotate_sh=False, fuse=params)) < 4000


def test_register_ply_fuse_overlap(tmp_path):
    """the script, end to end: the merged file has n1 + n2 - n_pairs rows"""
    import re
    from gaussiansplattingregistration_amd.utils import ply_io
    A, B, _ = F.base_pair(2000, sh_degree=1)
    F.add_scaling_rot(A, 31)
    F.add_scaling_rot(B, 32)
    rng = np.random.default_rng(33)
    rows = np.sort(rng.choice(2000, 1000, replace=False))            # half of the second scene: the first one's splats, slightly off
    for k in B:
        B[k][rows] = A[k][rows]
    B["xyz"][rows] += (0.005 * rng.normal(size=(1000, 3))).astype(np.float32)
    B["scaling"][rows] += (0.05 * rng.normal(size=(1000, 3))).astype(np.float32)
    B["dc"][rows] += (0.02 * rng.normal(size=(1000, 3))).astype(np.float32)
    paths = []
    for M, name in ((A, "a.ply"), (B, "b.ply")):
        paths.append(str(tmp_path / name))
        ply_io.save_gaussian_ply(paths[-1], M["xyz"], M["dc"], M["sh"], M["opacity"].reshape(-1, 1), M["scaling"], M["rot"])
    out = str(tmp_path / "merged.ply")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "register_ply.py"), paths[0], paths[1], "--voxel", "--type", "point", "--max-corr", "0.1",
                        "--iters", "5", "--out", out, "--fuse-overlap", "0.25", "--fuse-kld", "3.0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"n_pairs (\d+)\s+n_out (\d+)", r.stdout)
    assert m, r.stdout
    n_pairs, n_out = int(m.group(1)), int(m.group(2))
    assert n_pairs > 0 and n_out == 4000 - n_pairs
    assert len(ply_io.load_gaussian_arrays(out)["xyz"]) == n_out
