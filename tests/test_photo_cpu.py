"""Photometric refinement without a GPU: the float64 model against finite differences of its own energy, the model's
loop on a case geometry cannot solve, the C ABI's argument checks, the parameters and the command-line flags."""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest

import photo_model as P
from conftest import GOLDEN, ROOT


# ---- the model against itself ----------------------------------------------------------------------------------------------------------
def _y64(img):
    return (0.299 * img[..., 0] + 0.587 * img[..., 1]) + 0.114 * img[..., 2]


def _grad4(F):
    """4th-order central differences (gx, gy) on the interior (H-4, W-4): the stencil the Sobel gradient is judged by"""
    c = lambda dy, dx: F[2 + dy:F.shape[0] - 2 + dy, 2 + dx:F.shape[1] - 2 + dx]
    return (-c(0, 2) + 8 * c(0, 1) - 8 * c(0, -1) + c(0, -2)) / 12, (-c(2, 0) + 8 * c(1, 0) - 8 * c(-1, 0) + c(-2, 0)) / 12


def test_b_is_the_gradient_of_the_energy():
    """``b = sum(J_I' r_I + J_D' r_D)`` against the central finite difference of ``F(xi) = n E / 2 = sum(r_I^2 + r_D^2) / 2`` along the
    six components of ``xi``, ``T(xi) = [exp(omega) | v] T``: this pins the signs, the frames (left perturbation, world frame) and the
    order (rotation first).  ``F`` is evaluated here, from float64 ray-plane maps, without ``accumulate``.

    The point: the source is the plane itself (T = I) and the target is the same render plus a constant 0.05 in colour and in depth.
    The formulation takes the TARGET's gradients for the source's, which is exact only when the two agree: with a constant offset
    they do, and the residuals (0.05 everywhere) are not small, so b is far from zero.

    Margin per component, from the two discretisations alone:
      * the central difference's second-order error, estimated by Richardson from the steps h and h / 2: (4 / 3) |FD_h - FD_h/2|,
        doubled;
      * the Sobel stencil's truncation: ``eps`` = the largest difference between the Sobel gradient and the 4th-order central
        difference of the analytic float64 target maps over the largest gradient there.  Every term of b_k is linear in those
        gradients, so its error is of the size ``eps |term|``: ``eps sum|term|`` (the model returns ``sum|term|``).  This is loose (the
        stencil's errors oscillate and largely cancel in the sum) but two orders of magnitude below what a wrong sign, frame or
        component order would give (of the order of ``sum|term|`` itself).
    The float32 rounding of the maps (2^-24 relative) is far below both."""
    lam, off, mdd = P.LAMBDA, 0.05, 0.5
    cams = P.plane_cameras()
    b, asum, fd, fd2, eps = np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6), 0.0
    h = 1e-4
    for cam in cams:
        t64 = P.plane_maps(cam, float32=False)
        t64 = dict(image=t64["image"] + off, depth=t64["depth"] + off, alpha=t64["alpha"])
        tgt = {k: v.astype(np.float32) for k, v in t64.items()}
        src = P.plane_maps(cam)
        s, a = P.accumulate(src, tgt, cam, lam, P.TAU, mdd)
        assert s[29] == (cam["width"] - 2) * (cam["height"] - 2)            # every interior pixel counts
        b += s[21:27]
        asum += a[21:27]
        ok = P.counted(src, tgt, P.TAU, mdd)

        def F(xi):
            m = P.plane_maps(cam, P.se3_exp(xi), float32=False)
            rI, rD = _y64(t64["image"]) - _y64(m["image"]), t64["depth"] - m["depth"]
            return 0.5 * (((1 - lam) * rI ** 2 + lam * rD ** 2)[ok]).sum()
        for k in range(6):
            e = np.zeros(6)
            e[k] = 1.0
            fd[k] += (F(h * e) - F(-h * e)) / (2 * h)
            fd2[k] += (F(0.5 * h * e) - F(-0.5 * h * e)) / h
        for Fm in (_y64(t64["image"]), t64["depth"]):
            sx, sy = (g[1:-1, 1:-1] for g in P._sobel(Fm))
            gx, gy = _grad4(Fm)
            eps = max(eps, max(np.abs(sx - gx).max(), np.abs(sy - gy).max()) / max(np.abs(gx).max(), np.abs(gy).max()))
    margin = 2 * (4 / 3) * np.abs(fd - fd2) + eps * asum
    print("b", b, "\nfd", fd, "\n|b - fd|", np.abs(b - fd), "\nmargin", margin, "eps", eps)
    assert eps < 0.02                                   # the maps are smooth at this resolution: the margin means something
    assert np.all(margin < 0.05 * asum)                 # ... and is a small share of what the terms weigh
    assert np.all(np.abs(b - fd) <= margin), (b, fd, margin)


def test_sums_are_symmetric_in_their_layout_and_empty_images_give_zeros():
    cam = P.plane_cameras()[0]
    tgt, src = P.plane_maps(cam), P.plane_maps(cam, P.plane_start())
    s, a = P.accumulate(src, tgt, cam, max_depth_diff=0.5)
    Hm, b, eI, eD, n = P.unpack(s)
    assert np.array_equal(Hm, Hm.T) and np.all(np.linalg.eigvalsh(Hm) > 0) and np.all(a >= np.abs(s)) and n > 0 and eI > 0
    for shape in ((1, 1), (2, 5)):
        m = dict(image=np.ones(shape + (3,), np.float32), depth=np.ones(shape, np.float32), alpha=np.ones(shape, np.float32))
        s, a = P.accumulate(m, m, dict(cam, width=shape[1], height=shape[0]), max_depth_diff=0.5)
        assert not s.any() and not a.any()


# ---- the model's loop ------------------------------------------------------------------------------------------------------------------
def _plane_problem():
    cams = P.plane_cameras()
    return cams, [P.plane_maps(c) for c in cams], (lambda cam, T: P.plane_maps(cam, T))


def test_loop_reaches_the_truth_from_a_start_geometry_cannot_see():
    """2 degrees about the plane's normal and (0.06, -0.04, 0): E falls at every accepted step and the pose error ends below 1e-6 -- the
    maps are float32 (2^-24 relative: 1.4e-7 of a depth of 2.4, 6e-8 of a colour) and ~1 600 pixels per camera average it, so 1e-6 in
    length and angle is an order of magnitude above what their rounding can hold the fixed point away from the truth"""
    cams, targets, render = _plane_problem()
    r = P.refine(render, targets, cams, P.plane_start(), max_depth_diff=0.5)
    E = r["energies"]
    print("energies", E, "pose error", P.pose_error(r["T"]), "iterations", r["iterations"])
    assert len(E) >= 4 and all(b <= a for a, b in zip(E, E[1:])) and E[-1] < 1e-9 * E[0]
    te, re = P.pose_error(r["T"])
    assert te < 1e-6 and re < 1e-6
    assert P.pose_error(P.plane_start())[0] > 0.07


def test_depth_alone_is_singular_and_leaves_the_in_plane_motion():
    """lambda = 1: a plane's depth maps do not change under a motion inside the plane, the normal matrix has three eigenvalues that
    are zero up to the float32 rounding of the depths pushed through the Sobel stencil and squared -- (2^-24 fx)^2 ~ 1e-11 of the
    largest; asserted below 1e-8, with the other three above 1e-2 -- and the loop leaves the translation where it was."""
    cams, targets, render = _plane_problem()
    T0 = P.plane_start()
    r = P.refine(render, targets, cams, T0, lam=1.0, max_depth_diff=0.5)
    w = np.linalg.eigvalsh(r["H"])
    print("eigenvalues", w, "ratios", w / w[-1])
    assert np.all(w[:3] < 1e-8 * w[-1]) and np.all(w[3:] > 1e-2 * w[-1])
    assert np.abs(r["T"][:3, 3] - T0[:3, 3]).max() <= 4 * np.finfo(np.float64).eps
    assert P.pose_error(r["T"])[0] > 0.07                       # and so the error stays where it was
    full = P.refine(render, targets, cams, T0, max_depth_diff=0.5)
    assert np.linalg.eigvalsh(full["H"])[0] > 1e-6 * np.linalg.eigvalsh(full["H"])[-1]        # the intensity term pins all six down


def test_golden_of_the_end_to_end_case_is_what_the_float64_run_gives():
    """``photo_refine_expected.json`` (the bar of the GPU end-to-end test) against a fresh run of the NumPy renderer and this loop"""
    want = json.load(open(os.path.join(GOLDEN, P.GOLDEN_E2E)))
    got = P.e2e_expected()
    assert got["settings"] == want["settings"] and got["n_pixels"] == want["n_pixels"]
    assert got["initial_in_plane_error"] == pytest.approx(want["initial_in_plane_error"], rel=1e-12)
    for k in ("translation_error", "rotation_error", "in_plane_error"):
        assert got[k] <= 4 * want[k] + 1e-9 and got[k] < 1e-6, (k, got[k], want[k])
    assert got["energy_final"] < 1e-6 * got["energy_initial"]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def _call(hip_lib, **over):
    H, W = over.pop("H", 4), over.pop("W", 5)
    img = np.full((4, 5, 3), 0.5, np.float32)
    m = np.ones((4, 5), np.float32)
    V = np.eye(4)
    V[2, 3] = 2.0
    a = dict(I_s=img.ctypes.data, D_s=m.ctypes.data, A_s=m.ctypes.data, I_t=img.ctypes.data, D_t=m.ctypes.data, A_t=m.ctypes.data, V=V, fx=5.0, fy=5.0, cx=2.5,
             cy=2.0, lam=0.968, tau=0.5, mdd=0.25)
    out = np.full(30, 7.0)
    a["out"] = out.ctypes.data
    a.update(over)
    V = None if a["V"] is None else (C.c_double * 16)(*np.asarray(a["V"], np.float64).reshape(16))
    o = None if a["out"] is None else C.cast(a["out"], C.POINTER(C.c_double))
    rc = hip_lib.gsr_photo_accumulate(a["I_s"], a["D_s"], a["A_s"], a["I_t"], a["D_t"], a["A_t"], H, W, V, a["fx"], a["fy"], a["cx"], a["cy"], a["lam"], a["tau"],
                                      a["mdd"], 0, o, 0, None)
    return rc, hip_lib.gsr_last_error(), out


def test_symbol_is_exported_and_bound(hip_lib):
    from gaussiansplattingregistration_amd import _lib
    assert hasattr(hip_lib, "gsr_photo_accumulate") and "gsr_photo_accumulate" in _lib.SIGNATURES and _lib.GSR_PHOTO_SUMS_LEN == 30 == P.NSUMS


def test_no_device_code(hip_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    rc, msg, _ = _call(hip_lib)
    assert rc == -3 and b"no HIP device" in msg and b"gsr_photo_accumulate" in msg, (rc, msg)
    from gaussiansplattingregistration_amd import photo
    from gaussiansplattingregistration_amd.params import PhotometricParams
    m = dict(image=np.zeros((4, 5, 3), np.float32), depth=np.ones((4, 5), np.float32), alpha=np.ones((4, 5), np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        photo.accumulate(m, m, photo.PhotoCamera(np.eye(4), 5.0, 5.0, 2.5, 2.0, 5, 4), PhotometricParams(max_depth_diff=0.25))


nan, inf = float("nan"), float("inf")
BAD = ([(f"null {k}", {k: None}) for k in ("I_s", "D_s", "A_s", "I_t", "D_t", "A_t", "V", "out")] +
       [("height 0", dict(H=0)), ("width 0", dict(W=0)), ("height < 0", dict(H=-3)), ("width < 0", dict(W=-1)),
        ("lambda < 0", dict(lam=-0.1)), ("lambda > 1", dict(lam=1.5)), ("lambda nan", dict(lam=nan)),
        ("tau 0", dict(tau=0.0)), ("tau < 0", dict(tau=-0.5)), ("tau > 1", dict(tau=1.25)), ("tau nan", dict(tau=nan)),
        ("max_depth_diff 0", dict(mdd=0.0)), ("max_depth_diff < 0", dict(mdd=-1.0)), ("max_depth_diff inf", dict(mdd=inf)), ("max_depth_diff nan", dict(mdd=nan)),
        ("viewmat nan", dict(V=np.full((4, 4), nan))), ("viewmat inf", dict(V=np.diag([1.0, 1.0, inf, 1.0]))), ("fx inf", dict(fx=inf)), ("fy nan", dict(fy=nan)),
        ("cx nan", dict(cx=nan)), ("cy inf", dict(cy=-inf))])


@pytest.mark.parametrize("name,over", BAD, ids=[b[0] for b in BAD])
def test_bad_arguments_are_refused_before_any_device_call(hip_lib, name, over):
    """GSR_E_INVALID (-1) with a message under the entry's name -- on a machine without a device too, where anything that reached the
    device check would answer GSR_E_NO_DEVICE (-3); the output is not written"""
    rc, msg, out = _call(hip_lib, **over)
    assert rc == -1 and b"gsr_photo_accumulate" in msg and b"no HIP device" not in msg, (name, rc, msg)
    assert np.all(out == 7.0)


def test_the_ends_of_the_ranges_are_valid(hip_lib):
    """lambda = 0 and 1, tau = 1: not refused (they reach the device check or run)"""
    for over in (dict(lam=0.0), dict(lam=1.0), dict(tau=1.0)):
        assert _call(hip_lib, **over)[0] in (0, -3)


# ---- parameters and flags ---------------------------------------------------------------------------------------------------------------
def test_params_defaults():
    from gaussiansplattingregistration_amd.params import PhotometricParams
    p = PhotometricParams()
    assert p.lambda_depth == 0.968 == P.LAMBDA and p.tau == 0.5 == P.TAU and p.max_depth_diff is None and tuple(p.scales) == (4, 2, 1)
    assert p.max_iteration > 0 and p.min_increment > 0 and p.damping == 0.0
    from gaussiansplattingregistration_amd import photo
    with pytest.raises(ValueError, match="max_depth_diff"):
        photo.PhotometricRefiner(None, None, [], p).run()
    assert photo.RCOND == P.RCOND


def test_host_helpers_agree_with_the_model():
    from gaussiansplattingregistration_amd import photo
    rng = np.random.default_rng(0)
    xi = rng.normal(size=6) * 0.3
    assert np.array_equal(photo.se3_exp(xi), P.se3_exp(xi)) and np.array_equal(photo.se3_exp(np.zeros(6)), np.eye(4))
    A = rng.normal(size=(6, 6))
    Hm, b = A @ A.T, rng.normal(size=6)
    assert np.allclose(photo.solve_step(Hm, b, 0.0), -np.linalg.solve(Hm, b), rtol=1e-9) and np.array_equal(photo.solve_step(Hm, b, 0.3), P.solve_step(Hm, b, 0.3))
    Hs = np.diag([1.0, 1.0, 1.0, 1e-12, 1.0, 1.0])                  # a direction the data do not constrain is left alone
    assert photo.solve_step(Hs, np.ones(6), 0.0)[3] == 0.0
    s = rng.normal(size=30)
    s[29] = 12.0
    for a, w in zip(photo.unpack(s), P.unpack(s)):
        assert np.array_equal(a, w)
    from gaussiansplattingregistration_amd.models.camera import Camera
    V = P.look_at((0.5, -0.3, -2.4))
    c = photo.PhotoCamera.of(Camera(V[:3, :3].T, V[:3, 3], 100.0, 110.0, "a", 97, 72), 4)
    assert (c.width, c.height, c.fx, c.fy, c.cx, c.cy, c.image_name) == (24, 18, 25.0, 27.5, 97 / 8, 9.0, "a") and np.allclose(c.viewmat, V, atol=1e-6)


def test_command_line_flags():
    from gaussiansplattingregistration_amd import photo

    def parse(argv, with_cameras=True):
        ap = argparse.ArgumentParser()
        photo.add_photo_arguments(ap, with_cameras)
        return ap.parse_args(argv)
    assert photo.photo_params_from_args(parse([])) is None
    a = parse(["--photo-refine", "cams.json", "--photo-max-depth-diff", "0.2"])
    p = photo.photo_params_from_args(a)
    assert a.photo_refine == "cams.json" and p.max_depth_diff == 0.2 and tuple(p.scales) == (4, 2, 1) and p.lambda_depth == 0.968
    p = photo.photo_params_from_args(parse(["--photo-refine", "--photo-max-depth-diff", "1.5", "--photo-scales", "8,2", "--photo-lambda", "0.5"], False))
    assert p.max_depth_diff == 1.5 and tuple(p.scales) == (8, 2) and p.lambda_depth == 0.5
    with pytest.raises(SystemExit):
        photo.photo_params_from_args(parse(["--photo-refine", "cams.json"]))                    # no unit of length given
    with pytest.raises(SystemExit):
        photo.photo_params_from_args(parse(["--photo-refine", "c", "--photo-max-depth-diff", "0.2", "--photo-lambda", "2"]))
    for bad in ("4,0", "a,b", ""):
        with pytest.raises(SystemExit):
            parse(["--photo-scales", bad])
    for script, call in (("register_ply.py", "add_photo_arguments(ap)"), ("evaluate_registration.py", "add_photo_arguments(ap, with_cameras=False)")):
        text = open(os.path.join(ROOT, "scripts", script)).read()
        assert call in text and "photo_params_from_args(a)" in text, script
