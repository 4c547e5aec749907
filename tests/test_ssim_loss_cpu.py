"""The fine-tuner's L1 + D-SSIM loss without a GPU: the NumPy model of the kernel (tests/ssim_loss_model.py) against central
differences of its own loss, against the SSIM the evaluation is pinned to, against torch autograd on the CPU, the recorded cost of its
float64 arithmetic, the three C-ABI entries without a device and the fine-tuner's new parameter.

Finite differences.  A central difference of the float64 loss in one entry of the image with h = 2^-16 and h / 2; the analytic value must
lie within ``4 |FD(h) - FD(h/2)| + 8 eps |L| / h`` of FD(h/2): Richardson's estimate of the truncation error plus the round-off floor of
evaluating L (eps = 2^-52), the bound tests/test_raster_grad_cpu.py uses.  The scenes keep a and b at least 2^-11 apart (or equal
everywhere: ``identical`` and ``black``, where the central difference of |a - b| is 0 = sign(0)), so no step crosses the kink of the L1 term.
The differences are taken of the model's loss evaluated in np.longdouble: L = (1 - lam) l1 + lam (1 - ssim) cancels (exactly on
``identical``, to 2e-3 on ``flat``, where every S is besides ill-conditioned by 1 / C2), so eps |L| understates the round-off of a float64
evaluation of L -- on ``flat`` a float64 difference carries 1e-11 of noise against a floor of 3e-13.  One precision higher the differences
are clean and the bound stays as stated, eps = 2^-52 included; the gradient under test is the float64 model's.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import raster_model as M
import ssim_loss_model as L
from conftest import GOLDEN

TOLERANCE = os.path.join(GOLDEN, "ssim_loss_tolerance.json")
H_STEP = 2.0 ** -16
_cache = {}


def _model(name, lam):
    if (name, lam) not in _cache:
        a, b = L.build(name)
        _cache[name, lam] = (a, b, L.loss_grad(a, b, lam))
    return _cache[name, lam]


def test_scenes_are_what_the_tests_need():
    for name in L.SCENES:
        a, b = L.build(name)
        assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and a.shape[2] == 3
        if name in L.SIZES:
            assert "%dx%d" % a.shape[:2] == name
        if name in ("identical", "black"):
            assert np.array_equal(a, b)
        else:
            assert np.abs(a.astype(np.float64) - b).min() >= 2.0 ** -11
    assert L.build("over_range")[0].max() > 1.25 and not L.build("black")[0].any()
    a, b = L.build("flat")
    assert np.ptp(a) == 0 and set(np.unique(np.round((b.astype(np.float64) - a) * 2048))) == {-1.0, 8.0}


@pytest.mark.parametrize("name", L.SCENES)
def test_model_gradient_matches_central_differences(name):
    """16 random entries per scene and lambda in {0.2, 1}, h = 2^-16 and 2^-17"""
    rng = np.random.default_rng(11)
    worst = 0.0
    for lam in (0.2, 1.0):
        a, b, ref = _model(name, lam)
        a64 = a.astype(np.float64)
        a64 = a.astype(np.longdouble)
        for _ in range(16):
            at = tuple(int(rng.integers(0, s)) for s in a.shape)
            fd = []
            for h in (H_STEP, H_STEP / 2):
                vals = []
                for sign in (1.0, -1.0):
                    moved = a64.copy()
                    moved[at] += sign * h
                    vals.append(L.loss_grad(moved, b, lam, np.longdouble)["loss"])
                fd.append(float((vals[0] - vals[1]) / (2 * h)))
            allowed = 4 * abs(fd[0] - fd[1]) + 8 * 2.0 ** -52 * abs(float(ref["loss"])) / H_STEP
            err = abs(float(ref["grad"][at]) - fd[1])
            assert err <= allowed, (name, lam, at, float(ref["grad"][at]), fd, err, allowed)
            worst = max(worst, err / float(ref["scale"][at])) if ref["scale"][at] > 0 else worst
    print(f"{name}: largest |analytic - FD(h/2)| / scale {worst:.3e}")


# The nearly flat pair is left out of the next test by reasoning, not by what the code gives: there B2 = s1 + s2 + C2 is about 1e-3 while
# the moments it is formed from are about 0.5, so every float64 evaluation of S carries about 2000 roundings' worth of relative error,
# whichever order it filters in.  metrics64 (a direct 2-D filter) and the model (two separable passes) are then each some 1e-14 from the
# longdouble value, on opposite sides (measured: 6.6e-14 and 2.4e-14).  The flat pair's ssim is held to the longdouble model below
# (test_recorded_cost_of_float64) and on the GPU.
@pytest.mark.parametrize("name", [n for n in L.SCENES if n != "flat"])
def test_ssim_is_the_one_the_evaluation_is_pinned_to(name):
    a, b, ref = _model(name, 1.0)
    want = M.metrics64(a.transpose(2, 0, 1), b.transpose(2, 0, 1))[2]
    print(f"{name}: ssim {float(ref['ssim'])!r}, metrics64 {want!r}, difference {abs(float(ref['ssim']) - want):.2e}")
    assert abs(float(ref["ssim"]) - want) <= 1e-14


def test_flat_pair_is_where_float64_is_needed():
    """the two float64 evaluations of the flat pair's ssim and the longdouble one, printed; the float32 model's gradient is off by more
    than 1e-5 of the largest entry there and by less than 1e-5 on noise: why the kernel works in float64"""
    a, b = L.build("flat")
    lo, hi = L.loss_grad(a, b, 1.0), L.loss_grad(a, b, 1.0, np.longdouble)
    m = M.metrics64(a.transpose(2, 0, 1), b.transpose(2, 0, 1))[2]
    print(f"flat: model - longdouble {float(lo['ssim'] - hi['ssim']):.2e}, metrics64 - longdouble {float(m - hi['ssim']):.2e}")
    assert abs(float(lo["ssim"] - hi["ssim"])) < 1e-12 and abs(float(m - hi["ssim"])) < 1e-12
    cost = {}
    for name in ("flat", "37x50"):
        a, b = L.build(name)
        g32, g64 = L.loss_grad(a, b, 0.2, np.float32)["grad"], L.loss_grad(a, b, 0.2)["grad"]
        cost[name] = float(np.abs(g32 - g64).max() / np.abs(g64).max())
    print(f"float32 model against float64 model, largest gradient error / largest gradient: {cost}")
    assert cost["37x50"] < 1e-5 < cost["flat"]


def test_identical_and_black():
    for lam in L.LAMBDAS:
        _, _, r = _model("identical", lam)
        assert r["l1"] == 0.0 and abs(float(r["ssim"]) - 1.0) <= 1e-14 and not r["grad_l1"].any()
        _, _, r = _model("black", lam)
        assert r["ssim"] == 1.0 and r["l1"] == 0.0 and r["loss"] == 0.0


@pytest.mark.parametrize("name", L.SCENES)
def test_model_matches_torch_autograd_of_the_conv2d_formulation(name):
    """the same loss through a float64 grouped conv2d and autograd on the CPU: value and gradient within 1e-12 (of the scale)"""
    import torch
    import torch.nn.functional as Fn
    g = torch.as_tensor(L.window())
    w2 = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()
    for lam in L.LAMBDAS:
        a, b, ref = _model(name, lam)
        x = torch.as_tensor(a.astype(np.float64)).permute(2, 0, 1)[None].clone().requires_grad_(True)
        y = torch.as_tensor(b.astype(np.float64)).permute(2, 0, 1)[None]
        conv = lambda t: Fn.conv2d(t, w2, padding=5, groups=3)
        mu1, mu2 = conv(x), conv(y)
        s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
        ssim = (((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))).mean()
        loss = (1 - lam) * (x - y).abs().mean() + lam * (1 - ssim)
        loss.backward()
        got = x.grad[0].permute(1, 2, 0).numpy()
        err = np.abs(got - ref["grad"])
        assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-12 and (err <= 1e-12 * ref["scale"]).all(), (name, lam, float(loss.detach()), float(ref["loss"]))


def test_recorded_cost_of_float64():
    """tests/golden/ssim_loss_tolerance.json holds, per scene and lambda, max |g_64 - g_hi| / scale and |loss_64 - loss_hi| (l1 and ssim
    likewise), hi the same model in np.longdouble: regenerated here and compared.  tests/test_ssim_loss_gpu.py allows the kernel four
    times these figures."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60          # one precision higher than the kernel's
    want = json.load(open(TOLERANCE))
    assert sorted(want) == sorted(L.SCENES)
    for name in L.SCENES:
        for lam in L.LAMBDAS:
            got = L.tolerance_figures(name, lam)
            print(f"{name} lambda {lam}: {got}")
            rec = want[name][str(lam)]
            assert sorted(rec) == sorted(got)
            for k in got:
                assert got[k] == pytest.approx(rec[k], rel=1e-6, abs=1e-30)
                assert got[k] < (1e-12 if name == "flat" else 4e-15)          # a few dozen roundings of 2^-53 each; the flat pair amplifies them by 1 / C2


def test_loss_entries_without_a_device(hip_lib):
    import torch
    assert hip_lib.gsr_loss_create(0, None) == -1                         # GSR_E_INVALID
    assert b"gsr_loss_create" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_loss_l1_dssim(None, None, None, 8, 8, 0.2, None, None, None) == -1
    assert b"gsr_loss_l1_dssim" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_loss_destroy(None) == 0
    if torch.cuda.is_available():                  # the rest is about a machine without one
        return
    h = C.c_void_p()
    assert hip_lib.gsr_loss_create(0, C.byref(h)) == -3                   # GSR_E_NO_DEVICE
    assert b"gsr_loss_create" in hip_lib.gsr_last_error() and not h.value
    from gaussiansplattingregistration_amd import loss
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.l1_dssim(torch.zeros(4, 4, 3), torch.zeros(4, 4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.LossContext(0)


def test_finetune_params_take_the_new_loss():
    from gaussiansplattingregistration_amd.finetune import FinetuneParams, ModelFinetuner
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    assert FinetuneParams().lambda_dssim == 0.2 and FinetuneParams().loss == "l2"
    p = FinetuneParams(loss="l1_dssim", lambda_dssim=0.2)
    assert (p.loss, p.lambda_dssim) == ("l1_dssim", 0.2)
    assert list(FinetuneParams.__dataclass_fields__)[-1] == "lambda_dssim"          # appended: positional construction is unchanged
    scene, _, _ = M.build(M.EXACT_SCENE)
    model = GaussianModel("cpu").from_arrays(scene["xyz"], scene["color"], scene["opacity"], scene["cov6"], scene["sh"], scene["sh_degree"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):              # a model on the host: not a ValueError about the loss
        ModelFinetuner(model, [], [], p)
    with pytest.raises(ValueError, match="lambda_dssim"):
        ModelFinetuner(model, [], [], FinetuneParams(loss="l1_dssim", lambda_dssim=1.5))
