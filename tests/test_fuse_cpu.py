"""The overlap-aware merge without a GPU: invariants of the float64 model (tests/fuse_model.py), unambiguity of every case the GPU
tests compare exactly, and the C ABI of gsr_model_fuse (declaration, binding, argument checks, behaviour without a device)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fuse_model as F
from conftest import ROOT


@pytest.mark.parametrize("name", F.CASES)
def test_every_gpu_case_is_unambiguous(name):
    """The GPU tests demand exact equality of the pair list; that is only fair where no float64 implementation could decide
    otherwise.  An ambiguous case gets another seed in fuse_model.make_case, it is never excluded."""
    A, B, gates, want = F.case(name)
    assert not want["ambiguous"], (name, gates)
    assert want["n_out"] == len(A["xyz"]) + len(B["xyz"]) - want["n_pairs"]
    if name.startswith("base") or name in ("k0", "k3", "crowded", "invalid", "outliers", "scaling_rot", "ties", "large"):
        assert want["n_pairs"] > 100, (name, want["n_pairs"])          # the case exercises the fusion at all


def test_base_case_figures():
    """what the inputs give under the model (the issue's table, with this generator's draws)"""
    rows = [(F.case(f"base{i}")[3]["n_candidates"], F.case(f"base{i}")[3]["n_gated"], F.case(f"base{i}")[3]["n_pairs"]) for i in range(3)]
    assert rows == [(183776, 1000, 997), (183776, 35012, 1177), (15056, 1000, 997)], rows
    A, B, gates, want = F.case("base1")
    assert len(set(want["pairs"][:, 0])) == want["n_pairs"]


@pytest.mark.parametrize("name", ["base0", "base1", "ties", "invalid", "crowded"])
def test_model_invariants(name):
    A, B, gates, want = F.case(name)
    pairs = want["pairs"]
    # every splat is in at most one pair; ascending a
    assert len(np.unique(pairs[:, 0])) == len(pairs) and len(np.unique(pairs[:, 1])) == len(pairs)
    assert (np.diff(pairs[:, 0]) > 0).all()
    # symmetric under swapping A and B
    swapped = F.fuse(B, A, *gates)
    sp = swapped["pairs"][:, ::-1]
    assert np.array_equal(sp[np.argsort(sp[:, 0])], pairs)
    # the w-weighted first moments are conserved by the fusion (float64 rows before narrowing)
    wa, wb = want["w_a"][pairs[:, 0]], want["w_b"][pairs[:, 1]]
    for k in ("xyz", "dc", "sh"):
        a = A[k][pairs[:, 0]].astype(np.float64).reshape(len(pairs), -1)
        b = B[k][pairs[:, 1]].astype(np.float64).reshape(len(pairs), -1)
        lhs = (wa + wb)[:, None] * want["fused"][k]
        rhs = wa[:, None] * a + wb[:, None] * b
        assert np.abs(lhs - rhs).max() <= 1e-12 * np.abs(rhs).max()
    # invalid rows are never in a pair
    va, vb = F.prep(A)[0], F.prep(B)[0]
    assert va[pairs[:, 0]].all() and vb[pairs[:, 1]].all()


def test_fusing_a_model_with_its_own_copy_returns_its_rows():
    A, _, _ = F.base_pair(400)
    want = F.fuse(A, {k: v.copy() for k, v in A.items()}, 0.25, 0.5, 0.2)
    assert want["n_pairs"] == 400 and np.array_equal(want["pairs"][:, 0], want["pairs"][:, 1])
    for k in ("xyz", "cov6", "dc", "sh", "opacity"):
        assert np.array_equal(want[k], A[k]), k


def test_ties_go_to_the_lowest_index():
    A, B, gates, want = F.case("ties")
    assert np.array_equal(want["pairs"], np.stack([np.arange(250), np.arange(250)], 1))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------

def _views(n=8, K=15, with_sr=False):
    from gaussiansplattingregistration_amd import _lib
    rng = np.random.default_rng(0)
    keep = []

    def arr(*shape, fill=None):
        a = rng.random(shape).astype(np.float32) if fill is None else np.full(shape, fill, np.float32)
        keep.append(a)
        return a.ctypes.data

    def view(rows, out=False):
        v = _lib.ModelView()
        v.n = rows
        v.xyz, v.dc, v.sh, v.opacity = arr(rows, 3), arr(rows, 3), arr(rows, 3 * K), arr(rows)
        c = np.tile(np.float32([1, 0, 0, 1, 0, 1]), (rows, 1))
        keep.append(c)
        v.cov6 = c.ctypes.data
        if with_sr:
            v.scaling, v.rot = arr(rows, 3), arr(rows, 4)
        return v
    a, b, o = view(n), view(n), view(2 * n)
    P, R = _lib.FuseParams(0.25, 0.5, float("inf")), _lib.FuseReport()
    return a, b, o, P, R, keep


def _call(L, a, b, K, P, o, R, pairs=None):
    return L.gsr_model_fuse(C.addressof(a), C.addressof(b), K, C.addressof(P), C.addressof(o), pairs, C.addressof(R), 0, 0, None)


def test_declared_exported_and_bound(hip_lib):
    from gaussiansplattingregistration_amd import _lib
    text = open(os.path.join(ROOT, "include", "gsr_hip.h")).read()
    assert "gsr_model_fuse(" in text and "gsr_model_fuse" in _lib.SIGNATURES and hasattr(hip_lib, "gsr_model_fuse")
    assert [n for n in _lib.SIGNATURES if n.startswith("gsr_model_fuse")] == ["gsr_model_fuse"]          # one entry point
    assert len(_lib.SIGNATURES["gsr_model_fuse"][1]) == 10
    assert C.sizeof(_lib.ModelView) == 64 and C.sizeof(_lib.FuseParams) == 24 and C.sizeof(_lib.FuseReport) == 80
    for struct in ("gsr_model_view", "gsr_fuse_params", "gsr_fuse_report"):
        assert "} " + struct + ";" in text


def test_without_a_device(hip_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    a, b, o, P, R, keep = _views()
    assert _call(hip_lib, a, b, 15, P, o, R) == -3                      # GSR_E_NO_DEVICE
    msg = hip_lib.gsr_last_error()
    assert b"no HIP device" in msg and b"gsr_model_fuse" in msg, msg


def test_invalid_arguments(hip_lib):
    """the checks come before the device is opened: they give GSR_E_INVALID with or without a GPU"""
    L = hip_lib

    def refused(mutate, K=15, with_sr=False, null=None):
        a, b, o, P, R, keep = _views(with_sr=with_sr)
        mutate(a, b, o, P)
        args = [C.addressof(a), C.addressof(b), K, C.addressof(P), C.addressof(o), None, C.addressof(R), 0, 0, None]
        if null is not None:
            args[null] = None
        assert L.gsr_model_fuse(*args) == -1, mutate
        assert b"gsr_model_fuse" in L.gsr_last_error()
    nothing = lambda a, b, o, P: None
    for i in (0, 1, 3, 4, 6):
        refused(nothing, null=i)                                        # NULL a, b, params, out, report
    for K in (-1, 1, 2, 4, 16):
        refused(nothing, K=K)
    for r in (0.0, -1.0, float("inf"), float("nan")):
        refused(lambda a, b, o, P: setattr(P, "max_distance", r))
    refused(lambda a, b, o, P: setattr(P, "kld_max", -0.1))
    refused(lambda a, b, o, P: setattr(P, "kld_max", float("nan")))
    refused(lambda a, b, o, P: setattr(P, "color_delta", -1.0))
    for f in ("xyz", "cov6", "dc", "sh", "opacity"):
        refused(lambda a, b, o, P: setattr(a, f, None))
        refused(lambda a, b, o, P: setattr(o, f, None))
    refused(lambda a, b, o, P: setattr(b, "scaling", None), with_sr=True)       # scaling without rot
    refused(lambda a, b, o, P: (setattr(b, "scaling", None), setattr(b, "rot", None)), with_sr=True)      # on one side only
    refused(lambda a, b, o, P: (setattr(o, "scaling", None), setattr(o, "rot", None)), with_sr=True)
    refused(lambda a, b, o, P: setattr(a, "n", 1 << 31))
    refused(lambda a, b, o, P: setattr(b, "n", -1))
    refused(lambda a, b, o, P: setattr(o, "n", 15))                     # capacity below na + nb
    refused(lambda a, b, o, P: setattr(o, "xyz", a.xyz))                # not in place
    refused(lambda a, b, o, P: setattr(o, "sh", b.sh + 16))
    refused(lambda a, b, o, P: setattr(o, "dc", o.xyz + 12))            # two outputs overlap


def test_python_surface():
    import math
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.params import FuseOverlapParams
    p = FuseOverlapParams(0.1)
    assert (p.max_distance, p.kld_max, p.color_delta) == (0.1, 0.5, math.inf)
    assert callable(GaussianModel.fuse_overlap)
    import inspect
    assert inspect.signature(GaussianModel.get_merged_gaussian_point_clouds).parameters["fuse"].default is None


@pytest.mark.parametrize("script", ["register_ply.py", "evaluate_registration.py"])
def test_scripts_show_the_flags(script):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"], capture_output=True, text=True, check=True).stdout
    for flag in ("--fuse-overlap", "--fuse-kld", "--fuse-color"):
        assert flag in out
