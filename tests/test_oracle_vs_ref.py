"""The oracle against the REFERENCE ITSELF: the reference's levels of three synthetic clouds, computed by its own compiled extension
(oracle/_ref, built from the reference's C++ sources by `make -C oracle ref`), are stored in tests/golden/ref_live_cases.npz
(tests/golden/make_golden_ref_live.py).  The oracle must equal them bit for bit; where oracle/_ref is built, the live reference is
run as well and must still produce exactly the stored levels."""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

REF = glob.glob(os.path.join(ROOT, "oracle", "_ref", "mixture_bind*.so"))
STORED = os.path.join(GOLDEN, "ref_live_cases.npz")
FIELDS = ("xyz", "color", "opacity", "cov6", "sh")
CASES = [
    (6000, 0.75, 3, 3, dict(rho=3.0, delta=3.0, kappa=2.5, tau=1.0)),
    (3000, 0.6, 1, 2, dict(rho=2.0, delta=2.0, kappa=1.0, tau=0.5)),       # colour gate active
    (2000, 0.5, 0, 2, dict(rho=4.0, delta=4.0, kappa=2.5, tau=2.0)),
]


def _cloud(n, h, deg):
    from gaussiansplattingregistration_amd import synth
    return synth.make_cloud(n, seed=n, h=h, sh_degree=deg)


def _input_sum(cloud):
    """float64 sum of every input array: the stored case's fingerprint of its (regenerated) input."""
    return float(sum(np.asarray(cloud[f], np.float64).sum() for f in FIELDS))


def _run_ref(cloud, levels, **p):
    with tempfile.TemporaryDirectory() as td:
        inp, out = os.path.join(td, "i.npz"), os.path.join(td, "o.npz")
        np.savez(inp, levels=levels, **{k: cloud[k] for k in FIELDS}, **p)
        subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "run_ref.py"), inp, out], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return dict(np.load(out))


@pytest.mark.parametrize("n,h,deg,levels,params", CASES)
def test_oracle_equals_live_reference(oracle, n, h, deg, levels, params):
    c = _cloud(n, h, deg)
    stored = np.load(STORED)
    assert float(stored[f"n{n}_input_sum"]) == _input_sum(c), "synth.make_cloud no longer draws the stored case's input"
    ref = {f"{f}_{k}": stored[f"n{n}_{f}_{k}"] for k in range(levels) for f in FIELDS}
    if REF:
        live = _run_ref(c, levels, **params)
        for key, want in ref.items():
            assert live[key].shape == want.shape and np.array_equal(live[key].view(np.uint32), want.view(np.uint32)), ("live reference", key)
    got, _ = oracle.hem(c, levels, **params)
    for k in range(levels):
        for f in FIELDS:
            a, b = got[k][f], ref[f"{f}_{k}"]
            assert a.shape == b.shape, (k, f, a.shape, b.shape)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, f)
