"""gsr_fuse_multi on the GPU against the float64 model (tests/fuse_multi_model.py).

Every fixture is unambiguous under the model (tests/test_fuse_multi_cpu.py asserts it), so group_of and every count of the report must
be EQUAL, the copied rows equal bit for bit, and a fused value within one float32 ulp of the model's narrowed float64 value: both sides
form the same float64 sums in the same stated order, so only the narrowing is left.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fuse_model as F
import fuse_multi_model as M
from conftest import ROOT
from gaussiansplattingregistration_amd import synth
from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
from gaussiansplattingregistration_amd.params import FuseOverlapParams

pytestmark = pytest.mark.gpu

ATTR = {"xyz": "_xyz", "cov6": "_covariance", "dc": "_features_dc", "sh": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rot": "_rotation"}
COUNTS = ("n_out", "n_groups", "n_grouped_rows", "n_invalid", "gated_pairs", "mutual_edges", "rejected_edges", "rounds", "groups_of_size")


def to_model(M_, device):
    n = len(M_["xyz"])
    K = M_["sh"].shape[1] // 3
    g = GaussianModel(device).from_arrays(M_["xyz"], M_["dc"], M_["opacity"].reshape(n, 1), M_["cov6"], M_["sh"].reshape(n, K, 3), {0: 0, 3: 1, 8: 2, 15: 3}[K])
    if "scaling" in M_:
        g._scaling = torch.as_tensor(M_["scaling"], device=device)
        g._rotation = torch.as_tensor(M_["rot"], device=device)
    return g


def flat(a):
    """(n, width), also when n is 0"""
    a = np.asarray(a)
    return a.reshape(len(a), int(np.prod(a.shape[1:])))


def arrays_of(m):
    """the model's tensors as (n, width) float32 numpy arrays"""
    n = len(m)
    out = {}
    for k, attr in ATTR.items():
        t = getattr(m, attr)
        if t.numel() == 0 and t.dim() < 2:
            continue
        out[k] = flat(t.detach().cpu().numpy())
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def within_one_ulp(got, want32):
    """|got - want| <= the float32 spacing at |want|, element by element"""
    err = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    return err <= np.spacing(np.abs(want32)).astype(np.float64)


def reconstruct(scaling, rot):
    R = synth._quat_to_rot(rot.astype(np.float64))
    C = (R * np.exp(2.0 * scaling.astype(np.float64))[:, None, :]) @ R.transpose(0, 2, 1)
    return C[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]


def run(name, device="cuda:0"):
    models, gates, want = M.case(name)
    m, info = GaussianModel.fuse_overlap_multi([to_model(x, device) for x in models], FuseOverlapParams(*gates))
    return models, want, m, info


def check(want, m, info):
    for k in COUNTS:
        assert info[k] == want[k], (k, info[k], want[k])
    assert np.array_equal(info["group_of"].cpu().numpy(), want["group_of"])
    assert len(m) == want["n_out"]
    got = arrays_of(m)
    c0 = want["n_copied"]
    for k, g in got.items():
        w = flat(np.asarray(want[k], np.float32))
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.array_equal(bits(g[:c0]), bits(w[:c0])), k                      # the rows in no group, in global order, bit for bit
        if k in ("scaling", "rot") or want["n_groups"] == 0 or g.shape[1] == 0:
            continue
        ok = within_one_ulp(g[c0:], w[c0:])
        assert ok.all(), (k, int((~ok).sum()), g[c0:][~ok][:4], w[c0:][~ok][:4])
    if "scaling" in got and want["n_groups"]:
        s, q, c = got["scaling"][c0:], got["rot"][c0:], got["cov6"][c0:].astype(np.float64)
        assert np.abs(np.linalg.norm(q.astype(np.float64), axis=1) - 1).max() < 1e-6
        rel = np.abs(reconstruct(s, q) - c).max(1) / np.abs(c).max(1)
        assert rel.max() < 1e-5, rel.max()
    return got


@pytest.mark.parametrize("name", M.GRID_CASES)
def test_grid_equals_the_model(name):
    """N in {1, 2, 3, 5, 16} x rows per model in {0, 1, 63, 64, 65, 257, 3000} x K in {0, 15}"""
    models, want, m, info = run(name)
    check(want, m, info)
    if name.startswith("grid_1_"):                          # one model: copied, bit for bit
        got = arrays_of(m)
        for k in ("xyz", "cov6", "dc", "sh", "opacity"):
            assert np.array_equal(bits(got[k]), bits(flat(models[0][k]))), k
        assert info["n_groups"] == 0 and (info["group_of"] == -1).all()


@pytest.mark.parametrize("name", ["one_empty", "unequal", "invalid", "one_cell"])
def test_special_case_equals_the_model(name):
    models, want, m, info = run(name)
    check(want, m, info)
    if name == "invalid":                                   # a NaN centre, det <= 0 and -inf opacity in every model: never grouped
        assert info["n_invalid"] == 12
        go = info["group_of"].cpu().numpy()
        for mi in range(3):
            assert (go[want["offsets"][mi] + np.array([3, 40, 77, 130]) + mi] == -1).all()
    if name == "one_cell":
        assert info["rejected_edges"] > 0 and info["gated_pairs"] > 5 * info["mutual_edges"]
    if name == "unequal":
        assert [len(x["xyz"]) for x in models] == [3000, 65, 1]


def test_far_outliers_do_not_size_the_allocation():
    """five rows of each of three models at 500 x the scene extent.  What the call allocates is per row: the union copies 52 B, the
    pre-pass 56, the cell-ordered search arrays 98, keys and order 16, labels, masks, picks and ranks 36, and per row AND model the
    best table 8, the slot flags and their scan 8, edges and member table below 8 -- (260 + 24 N) B per row, the table of max(n, 1024)
    cells and rocPRIM's temporaries (1 MiB covers both here); not a table over the extent, which at edge 0.25 would have 2e9 cells"""
    models, want, m, info = run("outliers")
    check(want, m, info)
    n, N = len(want["group_of"]), len(models)
    assert 0 < info["workspace_bytes"] <= (260 + 24 * N) * n + (1 << 20), info["workspace_bytes"]
    _, _, _, plain = run("plain3")
    assert info["workspace_bytes"] <= plain["workspace_bytes"]        # (plain3 has four times the rows)


def test_conflict_chain():
    """a1 - b1 - c1 - a2 on a line: the edge b1 - c1 would put a1 and a2 into one group and is rejected"""
    models, want, m, info = run("chain")
    check(want, m, info)
    go = info["group_of"].cpu().numpy()
    assert info["rejected_edges"] > 0 and info["n_groups"] == 2
    assert go[0] != go[1] and go[0] == go[2] and go[1] == go[3]      # (a1, b1) and (a2, c1): no group with two rows of A
    for rank in range(info["n_groups"]):
        members = np.flatnonzero(go == want["n_copied"] + rank)
        assert len(set(want["model_id"][members])) == len(members)


@pytest.mark.parametrize("name", ["base0", "base1", "k0", "k3", "one_pairs", "one_apart", "odd_257_63", "empty_a", "empty_b", "no_overlap", "ties", "invalid",
                                  "outliers", "crowded", "scaling_rot"])
def test_two_models_against_the_pairwise_entry_point(name):
    """N = 2 against gsr_model_fuse itself: the same pair set; the same copied rows bit for bit and the same fused rows to one ulp, up
    to the documented row order (pairwise: A-only, fused, B-only; N-way: A-only, B-only, fused)"""
    A, B, gates = F.make_case(name)
    params = FuseOverlapParams(*gates)
    pm, pinfo = GaussianModel.fuse_overlap(to_model(A, "cuda:0"), to_model(B, "cuda:0"), params)
    mm, minfo = GaussianModel.fuse_overlap_multi([to_model(A, "cuda:0"), to_model(B, "cuda:0")], params)
    na, npairs = len(A["xyz"]), pinfo["n_pairs"]
    assert minfo["n_groups"] == npairs and minfo["n_out"] == pinfo["n_out"] and minfo["gated_pairs"] == pinfo["gated_pairs"]
    assert minfo["n_invalid"] == pinfo["n_invalid_a"] + pinfo["n_invalid_b"] and minfo["rejected_edges"] == 0
    go = minfo["group_of"].cpu().numpy()
    pairs = pinfo["pairs"].cpu().numpy()
    c0 = minfo["n_out"] - npairs
    assert np.array_equal(np.flatnonzero(go[:na] >= 0), pairs[:, 0]) and np.array_equal(go[pairs[:, 0]], c0 + np.arange(npairs))
    assert np.array_equal(go[na + pairs[:, 1]], c0 + np.arange(npairs)) and (go >= 0).sum() == 2 * npairs
    p, g = arrays_of(pm), arrays_of(mm)
    a0, p0 = pinfo["n_a_only"], pinfo["n_a_only"] + npairs
    for k in g:
        assert np.array_equal(bits(g[k][:c0]), bits(np.concatenate([p[k][:a0], p[k][p0:]]))), k
        if k in ("scaling", "rot") or g[k].shape[1] == 0 or npairs == 0:
            continue
        assert within_one_ulp(g[k][c0:], p[k][a0:p0]).all(), k


def test_more_rows_than_one_pass_of_the_grids():
    """300 000 + 300 000 rows (K = 0): more than the 2048 x 256 threads a launch has, so the grid-stride loops over rows and over slots
    take a second trip (the ballot in the pre-pass included), the table has more than 1024 cells and the sort keys more than 11 bits"""
    models, want, m, info = run("large")
    assert len(want["group_of"]) > 2048 * 256 and want["n_groups"] > 100000
    check(want, m, info)


def test_host_and_device_arrays_and_two_runs_give_the_same_bits():
    _, want, m_dev, i_dev = run("grid_3_257_15", "cuda:0")
    _, _, m_host, i_host = run("grid_3_257_15", "cpu")
    _, _, m_again, i_again = run("grid_3_257_15", "cuda:0")
    assert not m_host._xyz.is_cuda and m_dev._xyz.is_cuda
    d, h, a = arrays_of(m_dev), arrays_of(m_host), arrays_of(m_again)
    for k in d:
        assert np.array_equal(bits(d[k]), bits(h[k])), k
        assert np.array_equal(bits(d[k]), bits(a[k])), k
    assert torch.equal(i_dev["group_of"].cpu(), i_host["group_of"]) and torch.equal(i_dev["group_of"], i_again["group_of"])
    for k in COUNTS:
        assert i_dev[k] == i_host[k] == i_again[k], k
    # the result tensors are views of arrays allocated for all rows
    assert m_dev._xyz.untyped_storage().nbytes() >= 771 * 12 and len(m_dev) == want["n_out"] < 771


def test_models_with_scaling_and_rotation():
    models, want, m, info = run("scaling_rot")
    got = check(want, m, info)                              # copied rows keep theirs bit for bit, fused rows reproduce their covariance
    assert want["n_groups"] > 100 and "scaling" in got and want["groups_of_size"][3] > 0


def test_merge_multi_with_fuse():
    models, gates = M.make_case("grid_3_257_15")
    params = FuseOverlapParams(*gates)
    poses = [np.eye(4), synth.rigid_transform(20.0, (0.3, 1.0, -0.5), (0.2, -0.1, 0.05)), synth.rigid_transform(-35.0, (1.0, 0.2, 0.1), (-0.3, 0.0, 0.4))]
    # every model sits in its own frame: pose i brings it back
    gs = [to_model(x, "cuda:0") for x in models]
    for g, T in zip(gs[1:], poses[1:]):
        g.transform_gaussian_model(np.linalg.inv(T), rotate_sh=True)
    merged = GaussianModel.get_merged_gaussian_point_clouds_multi(gs, poses, rotate_sh=True, fuse=params)
    moved = [g.clone_gaussian().transform_gaussian_model(T, rotate_sh=True) if i else g for i, (g, T) in enumerate(zip(gs, poses))]
    want, info = GaussianModel.fuse_overlap_multi(moved, params)
    twin, tinfo = GaussianModel.get_merged_gaussian_point_clouds_fused_multi(gs, poses, params, rotate_sh=True)
    assert info["n_groups"] > 100 and len(merged) == 771 - (info["n_grouped_rows"] - info["n_groups"]) == tinfo["n_out"]
    for k, v in arrays_of(want).items():
        assert np.array_equal(bits(arrays_of(merged)[k]), bits(v)), k
        assert np.array_equal(bits(arrays_of(twin)[k]), bits(v)), k
    # fuse=None is the concatenation, bit for bit
    plain = GaussianModel.get_merged_gaussian_point_clouds_multi(gs, poses, rotate_sh=True)
    plain_none = GaussianModel.get_merged_gaussian_point_clouds_multi(gs, poses, rotate_sh=True, fuse=None)
    assert len(plain) == 771
    for k, v in arrays_of(plain).items():
        assert np.array_equal(bits(arrays_of(plain_none)[k]), bits(v)), k
        cat = torch.cat([getattr(g, ATTR[k]) for g in moved]).cpu().numpy().reshape(771, -1)
        assert np.array_equal(bits(v), bits(cat)), k
    # an average of SH rows in two frames means nothing
    with pytest.raises(RuntimeError, match="rotate_sh"):
        GaussianModel.get_merged_gaussian_point_clouds_multi(gs, poses, rotate_sh=False, fuse=params)


def test_register_many_fuse_overlap(tmp_path):
    """the script, end to end, in fresh child processes: with --fuse-overlap the merged file has n_out rows, fewer than the concatenation
    by the printed sum of (k - 1); without it the file is byte for byte the plain concatenation of the moved scenes"""
    from gaussiansplattingregistration_amd.utils import ply_io
    n, scenes = 1500, []
    A = F.add_scaling_rot(F.model_of(synth.make_cloud(n, seed=81, h=synth.half_extent(n), sh_degree=1)), 82)
    scenes.append(A)
    rng = np.random.default_rng(83)
    for s in range(3):                                      # half of every further scene: the first one's splats, slightly off
        B = F.add_scaling_rot(F.model_of(synth.make_cloud(n, seed=84 + s, h=synth.half_extent(n), sh_degree=1)), 90 + s)
        rows = np.sort(rng.choice(n, n // 2, replace=False))
        for k in B:
            B[k][rows] = A[k][rows]
        B["xyz"][rows] += (0.005 * rng.normal(size=(len(rows), 3))).astype(np.float32)
        B["scaling"][rows] += (0.05 * rng.normal(size=(len(rows), 3))).astype(np.float32)
        B["dc"][rows] += (0.02 * rng.normal(size=(len(rows), 3))).astype(np.float32)
        scenes.append(B)
    paths = []
    for i, S in enumerate(scenes):
        paths.append(str(tmp_path / f"s{i}.ply"))
        ply_io.save_gaussian_ply(paths[-1], S["xyz"], S["dc"], S["sh"], S["opacity"].reshape(-1, 1), S["scaling"], S["rot"])
    script = os.path.join(ROOT, "scripts", "register_many.py")
    common = ["--type", "point", "--max-corr", "0.1", "--iters", "5"]
    fused, plain, poses = str(tmp_path / "fused.ply"), str(tmp_path / "plain.ply"), str(tmp_path / "poses.json")
    r = subprocess.run([sys.executable, script] + paths + common + ["--out", fused, "--fuse-overlap", "0.25", "--fuse-kld", "3.0"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    mt = re.search(r"fuse: n_groups (\d+)\s+sizes \{([^}]*)\}.*n_out (\d+)", r.stdout)
    assert mt, r.stdout
    n_groups, n_out = int(mt.group(1)), int(mt.group(3))
    sizes = {int(k): int(c) for k, c in re.findall(r"(\d+): (\d+)", mt.group(2))}
    assert n_groups == sum(sizes.values()) > 0 and max(sizes) >= 3
    assert n_out == 4 * n - sum((k - 1) * c for k, c in sizes.items())
    assert len(ply_io.load_gaussian_arrays(fused)["xyz"]) == n_out
    r = subprocess.run([sys.executable, script] + paths + common + ["--out", plain, "--poses-out", poses], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fuse:" not in r.stdout
    X = json.load(open(poses))["poses"]
    models = [GaussianModel("cuda:0").from_ply(p) for p in paths]
    want = str(tmp_path / "want.ply")
    GaussianModel.get_merged_gaussian_point_clouds_multi(models, X).save_ply(want)
    assert open(plain, "rb").read() == open(want, "rb").read()
