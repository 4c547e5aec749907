"""Photometric refinement on the device: ``gsr_photo_accumulate`` against ``photo_model`` on all 30 sums, its gates at
exactly representable values, its bits from run to run and from host or device maps, and ``PhotometricRefiner`` end to end on a case
geometry cannot solve.

The tolerance of a sum is derived: kernel and model form every per-pixel term in float64 from the same float32 inputs with the same
operations in the same order (no fused multiply-add on either side), so they differ by the order of the summation alone.  Any order
of N terms is within (N - 1) 2^-53 sum|term| of the exact sum, two orders within N 2^-52 sum|term| of each other; N is the pixel
count and sum|term| what the model returns beside each sum."""
import functools
import json
import os

import numpy as np
import pytest

import photo_model as P
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TAU, MDD, GUARD = 0.5, 0.25, 1e-4


def _params(**kw):
    from gaussiansplattingregistration_amd.params import PhotometricParams
    return PhotometricParams(**dict(dict(max_depth_diff=MDD, tau=TAU), **kw))


def _camera(W, H, seed):
    rng = np.random.default_rng(seed)
    V = P.look_at(rng.uniform(-0.5, 0.5, 3) + (0.0, 0.0, -2.5), rng.uniform(-0.2, 0.2, 3))
    return dict(viewmat=V, fx=1.1 * max(W, 8) + 0.37, fy=1.2 * max(W, 8) - 0.21, cx=W / 2 + 0.3, cy=H / 2 - 0.4, width=W, height=H)


def _maps(W, H, seed, holes=True, count_from_x=0):
    """seeded synthetic maps: smooth plus noise, rounded to float32; holes in both coverages; every value at least ``GUARD`` from its gate"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = []
    base = 2.0 + 0.3 * np.sin(0.21 * x + 0.4) * np.cos(0.17 * y) + 0.01 * rng.normal(size=(H, W))
    for k in range(2):
        img = np.stack([0.5 + 0.3 * np.sin(0.3 * x + 0.2 * y + c + 0.05 * k) for c in range(3)], -1) + 0.02 * rng.normal(size=(H, W, 3))
        alpha = rng.uniform(0.6, 1.0, (H, W))
        if holes:
            alpha = np.where(rng.random((H, W)) < (0.03 if k else 0.08), rng.uniform(0.0, 0.4, (H, W)), alpha)
        if k == 0:                       # the source: only the pixels from column count_from_x on are covered
            alpha = np.where(x >= count_from_x, alpha, rng.uniform(0.0, 0.4, (H, W)))
        depth = base
        if k == 1:                       # the target: within the gate, except one pixel in eight, well outside it
            d = rng.uniform(-0.2, 0.2, (H, W))
            depth = base + np.where(rng.random((H, W)) < 0.125 if holes else False, np.sign(d) * rng.uniform(0.3, 0.4, (H, W)), d)
        out.append(dict(image=img.astype(np.float32), depth=depth.astype(np.float32), alpha=alpha.astype(np.float32)))
    return out[0], out[1]


# (name, W, H, seed, holes, count_from_x, expected count or None)
CASES = [("1x1", 1, 1, 1, False, 0, 0), ("2x5", 2, 5, 2, False, 0, 0), ("3x3", 3, 3, 3, False, 0, 1), ("16x16", 16, 16, 4, True, 0, None),
         ("17x13", 17, 13, 5, True, 0, None), ("37x29", 37, 29, 6, True, 0, None), ("33x16_from_16", 33, 16, 7, True, 16, None),
         ("35x16_last_tiles", 35, 16, 8, False, 32, None)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """the inputs and the model's sums of a case, computed once and left unchanged"""
    _, W, H, seed, holes, cfx, want_n = next(c for c in CASES if c[0] == name)
    cam = _camera(W, H, seed)
    src, tgt = _maps(W, H, seed, holes, cfx)
    sums, asum = P.accumulate(src, tgt, cam, P.LAMBDA, TAU, MDD)
    for a in list(src.values()) + list(tgt.values()) + [sums, asum]:
        a.setflags(write=False)
    return dict(cam=cam, src=src, tgt=tgt, sums=sums, asum=asum, W=W, H=H, want_n=want_n, count_from_x=cfx)


def _photo_camera(cam):
    from gaussiansplattingregistration_amd import photo
    return photo.PhotoCamera(np.asarray(cam["viewmat"], np.float64), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"])


def _kernel(src, tgt, cam, **kw):
    from gaussiansplattingregistration_amd import photo
    return photo.accumulate_sums(src, tgt, _photo_camera(cam), _params(**kw))


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_sums_against_the_model(name):
    """33 x 16 and 35 x 16 are W x H.  In the first the source covers x >= 16 only: the second column of tiles is the last that can
    count (x = 32 is the image's border, which never counts; x = 31 needs it as halo, from the third column).  In the second x >= 32:
    the only counted pixels (x = 32, 33) are in the last, partial column of tiles."""
    c = _case(name)
    m = P.gate_margins(c["src"], c["tgt"], TAU, MDD)
    assert min(m) >= GUARD, m                                       # no decision is fragile
    got = _kernel(c["src"], c["tgt"], c["cam"])
    N = c["W"] * c["H"]
    tol = N * 2.0 ** -52 * c["asum"]
    err = np.abs(got - c["sums"])
    worst = int(np.argmax(err - tol))
    print(f"{name}: n {got[29]:.0f}; largest |kernel - model| / (N 2^-52 sum|term|) = {np.max(err / np.maximum(tol, 1e-300)):.3g} (sum {worst}); "
          f"largest relative error {np.max(err / np.maximum(np.abs(c['sums']), 1e-300)):.3g}")
    assert got[29] == c["sums"][29]
    if c["want_n"] is not None:
        assert got[29] == c["want_n"]
    else:
        assert got[29] > 0
    if c["want_n"] == 0:
        assert not got.any() and not np.signbit(got).any()         # thirty exact zeros
    if c["count_from_x"]:
        ok = P.counted(c["src"], c["tgt"], TAU, MDD)
        assert ok.any() and not ok[:, :c["count_from_x"]].any()
    assert np.all(err <= tol), (name, worst, got[worst], c["sums"][worst], tol[worst])


def test_lambda_ends_and_another_tau():
    """lambda = 0 and 1 (one term switched off) and tau = 0.7 on the 37 x 29 maps, against the model"""
    c = _case("37x29")
    N = c["W"] * c["H"]
    for lam, tau in ((0.0, TAU), (1.0, TAU), (P.LAMBDA, 0.7)):
        assert min(P.gate_margins(c["src"], c["tgt"], tau, MDD)[:2]) >= GUARD
        want, asum = P.accumulate(c["src"], c["tgt"], c["cam"], lam, tau, MDD)
        got = _kernel(c["src"], c["tgt"], c["cam"], lambda_depth=lam, tau=tau)
        assert got[29] == want[29] > 0 and np.all(np.abs(got - want) <= N * 2.0 ** -52 * asum), (lam, tau)
        assert (got[27] == 0) == (lam == 1.0) and (got[28] == 0) == (lam == 0.0)


# ---- the gates at exactly representable values ------------------------------------------------------------------------------------------
def _flat(W=7, H=7):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.stack([0.4 + 0.03 * x, 0.5 - 0.02 * y, 0.3 + 0.01 * (x + y)], -1).astype(np.float32)
    mk = lambda d, k: dict(image=(img + np.float32(0.0625 * k)), depth=np.full((H, W), d, np.float32), alpha=np.ones((H, W), np.float32))
    return mk(0.125, 0), mk(0.375, 1), _camera(W, H, 11)          # D_t - D_s = 0.25 exactly = max_depth_diff: every interior pixel counts


def _count(src, tgt, cam):
    got = _kernel(src, tgt, cam)
    want, asum = P.accumulate(src, tgt, cam, P.LAMBDA, TAU, MDD)
    assert got[29] == want[29] and np.all(np.abs(got - want) <= 49 * 2.0 ** -52 * asum)
    return int(got[29])


def test_gates_at_exactly_representable_values():
    src, tgt, cam = _flat()
    below = np.nextafter(np.float32(0.5), np.float32(0))
    assert _count(src, tgt, cam) == 25                              # |D_t - D_s| = 0.25 = max_depth_diff counts, everywhere
    s = dict(src, alpha=src["alpha"].copy())
    s["alpha"][3, 3] = 0.5
    assert _count(s, tgt, cam) == 25                                # A_s = tau counts
    s["alpha"][3, 3] = below
    assert _count(s, tgt, cam) == 24                                # the float32 below it does not
    t = dict(tgt, alpha=tgt["alpha"].copy())
    t["alpha"][3, 3] = 0.5
    assert _count(src, t, cam) == 25                                # A_t = tau counts, for all nine pixels that look at it
    t["alpha"][3, 3] = below
    assert _count(src, t, cam) == 16                                # one hole removes exactly the nine pixels around it
    ok = P.counted(src, t, TAU, MDD)
    assert not ok[2:5, 2:5].any() and ok[1:6, 1:6].sum() == 16
    t["alpha"][3, 3] = 1.0
    t["alpha"][0, 0] = below                                        # a hole in the corner of the image: only (1, 1) looks at it
    assert _count(src, t, cam) == 24
    t = dict(tgt, depth=tgt["depth"].copy())
    t["depth"][3, 3] = np.nextafter(np.float32(0.375), np.float32(1))          # 0.375 + 2^-25: the difference is the float32 above 0.25
    assert float(t["depth"][3, 3]) - 0.125 == float(np.nextafter(np.float32(0.25), np.float32(1)))
    assert _count(src, t, cam) == 24                                # ... which does not count; its neighbours still do
    t["depth"][3, 3] = np.nextafter(np.float32(0.375), np.float32(0))
    assert _count(src, t, cam) == 25
    s = dict(src, depth=src["depth"].copy())
    s["depth"][2, 4] = np.float32(0.625)                            # D_t - D_s = -0.25: the gate is on the absolute value
    assert _count(s, tgt, cam) == 25
    s["depth"][2, 4] = np.nextafter(np.float32(0.625), np.float32(1))
    assert _count(s, tgt, cam) == 24
    s["depth"][2, 4] = np.float32("nan")                            # a NaN fails the comparison and is left out
    assert _count(s, tgt, cam) == 24


# ---- reproducibility and residency ----------------------------------------------------------------------------------------------------
def test_same_bits_from_run_to_run_and_from_host_or_device_maps():
    import torch
    c = _case("37x29")
    a = _kernel(c["src"], c["tgt"], c["cam"])
    b = _kernel(c["src"], c["tgt"], c["cam"])
    assert a.tobytes() == b.tobytes()
    dev = lambda m: {k: torch.from_numpy(np.array(v)).cuda() for k, v in m.items()}
    d = _kernel(dev(c["src"]), dev(c["tgt"]), c["cam"])
    assert a.tobytes() == d.tobytes()
    from gaussiansplattingregistration_amd import photo
    Hm, bb, eI, eD, n = photo.accumulate(dev(c["src"]), dev(c["tgt"]), _photo_camera(c["cam"]), _params())
    assert n == int(a[29]) and eI == a[27] and eD == a[28] and np.array_equal(bb, a[21:27]) and Hm[2, 4] == Hm[4, 2] == a[P.TRIU.index((2, 4))]
    with pytest.raises(ValueError, match="all host arrays or all CUDA"):
        _kernel(dev(c["src"]), c["tgt"], c["cam"])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _gaussian_model(scene, device="cuda:0"):
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    return GaussianModel(device).from_arrays(scene["xyz"], scene["color"], scene["opacity"], scene["cov6"], scene["sh"], scene["sh_degree"])


def _cameras(cams):
    from gaussiansplattingregistration_amd.models.camera import Camera
    out = []
    for cd in cams:
        V = np.asarray(cd["viewmat"], np.float64)
        out.append(Camera(V[:3, :3].T, V[:3, 3], cd["fx"], cd["fy"], cd["image_name"], cd["width"], cd["height"]))
    return out


def _e2e_params(**kw):
    E = P.E2E
    return _params(**dict(dict(max_depth_diff=E["max_depth_diff"], scales=E["scales"], max_iteration=E["max_iteration"], min_increment=E["min_increment"]), **kw))


def _float32_floor():
    """what the float32 of the renders can hold the fixed point away from the truth, from ``raster_aux_tolerance.json`` (what float32
    costs the renderer's own model): the depth's relative error times the largest depth of the scene (along the view), plus the
    blend's absolute error -- the same weights make the colour -- over the RMS gradient of the texture's intensity per unit of
    length (inside the plane)"""
    tol = json.load(open(os.path.join(GOLDEN, "raster_aux_tolerance.json")))
    d_rel, c_abs = max(t["depth_max_rel_diff"] for t in tol.values()), max(t["alpha_max_abs_diff"] for t in tol.values())
    z_max = max(np.linalg.norm(np.linalg.inv(c["viewmat"])[:3, 3]) for c in P.plane_cameras()) + P.PLANE_WIDTH
    g = np.linspace(-P.PLANE_WIDTH / 2, P.PLANE_WIDTH / 2, 401)
    x, y = np.meshgrid(g, g)
    tex = P.texture(x, y)
    Y = (0.299 * tex[..., 0] + 0.587 * tex[..., 1]) + 0.114 * tex[..., 2]
    gy, gx = np.gradient(Y, g, g)
    return d_rel * z_max + c_abs / float(np.sqrt((gx * gx + gy * gy).mean()))


def test_refinement_recovers_the_motion_inside_a_textured_plane():
    """400 flat disc splats on a plane, coloured by a smooth function of position; the source is the SAME splats started 2 degrees
    about the normal and 3 % of the plane's width off inside it, so the fixed point is the identity; two cameras at 96 x 72.

    Bar (DESIGN.md 14.3's rule): the float64 run of the same loop on the NumPy renderer (``photo_refine_expected.json``: in-plane error
    3.7e-9, translation 2.5e-8, rotation 4.9e-9 rad) times 4, plus the float32 floor of the renders (``_float32_floor``: 3.9e-5), and
    in any case a tenth of the initial error.  Point-to-plane ICP from the same start is run and its in-plane error printed, not
    asserted: it documents the case.  Measured figures: DESIGN.md 23.4."""
    from gaussiansplattingregistration_amd import photo
    want = json.load(open(os.path.join(GOLDEN, P.GOLDEN_E2E)))
    model = _gaussian_model(P.splat_plane())
    cams = _cameras(P.plane_cameras(P.E2E["width"], P.E2E["height"]))
    T0 = P.splat_start()
    r = photo.PhotometricRefiner(model, model, cams, _e2e_params(), init=T0).run()
    T = r.transformation
    te, re = P.pose_error(T)
    ip, ip0 = float(np.linalg.norm(T[:2, 3])), float(np.linalg.norm(T0[:2, 3]))
    floor = _float32_floor()
    allow_ip, allow_t, allow_r = 4 * want["in_plane_error"] + floor, 4 * want["translation_error"] + floor, 4 * want["rotation_error"] + floor / (P.PLANE_WIDTH / 2)
    print(f"photometric: E {r.energy_initial:.4g} -> {r.energy_final:.4g}; pixels {r.n_pixels_per_camera}; iterations {r.iterations}; "
          f"in-plane error {ip0:.4g} -> {ip:.4g} (allowed {allow_ip:.4g}); translation {te:.4g} (allowed {allow_t:.4g}); rotation {re:.4g} rad "
          f"(allowed {allow_r:.4g}); float32 floor {floor:.4g}")
    for row in r.trace:
        print("  level", row["scale"], row["width"], "x", row["height"], "iterations", row["iterations"], "accepted", row["accepted"], "E",
              ["%.4g" % e for e in row["energies"]], "n", row["n_pixels"])
    # documentation of the case, not a check: point-to-plane ICP from the same start
    try:
        from gaussiansplattingregistration_amd.params import LocalRegistrationParams
        from gaussiansplattingregistration_amd.utils.local_registration_util import LocalRegistrationType, do_icp_registration
        from gaussiansplattingregistration_amd.utils.point_cloud_converter import convert_gs_to_open3d_pc
        pc = convert_gs_to_open3d_pc(model)
        icp = do_icp_registration(pc, pc, T0, LocalRegistrationParams(registration_type=LocalRegistrationType.ICP_Point_To_Plane, max_correspondence=0.3))
        Ti = np.asarray(icp.transformation, np.float64)
        print(f"point-to-plane ICP from the same start: in-plane error {ip0:.4g} -> {np.linalg.norm(Ti[:2, 3]):.4g}, rotation "
              f"{P.pose_error(T0)[1]:.4g} -> {P.pose_error(Ti)[1]:.4g} rad (fitness {icp.fitness:.3f})")
    except Exception as e:                                          # the rank-deficient system may be refused: that is an answer too
        print("point-to-plane ICP from the same start:", type(e).__name__, e)
    assert not r.error_list, r.error_list
    assert r.energy_final < r.energy_initial
    assert all(len(row["energies"]) == row["accepted"] + 1 and all(b <= a for a, b in zip(row["energies"], row["energies"][1:])) for row in r.trace)
    assert len(r.n_pixels_per_camera) == 2 and min(r.n_pixels_per_camera) > 0 and r.n_pixels == sum(r.n_pixels_per_camera)
    assert ip <= allow_ip and ip < 0.1 * ip0
    assert te <= allow_t and re <= allow_r and te < 0.1 * P.pose_error(T0)[0] and re < 0.1 * P.pose_error(T0)[1]


def test_controller_refines_the_current_transform():
    from gaussiansplattingregistration_amd.controllers.registration_controller import RegistrationController
    from gaussiansplattingregistration_amd.models.data_repository import DataRepository, UIStateRepository
    model = _gaussian_model(P.splat_plane())
    repo, ui = DataRepository(), UIStateRepository()
    repo.pc_gaussian_list_first.append(model)
    repo.pc_gaussian_list_second.append(model)
    ui.transformation_matrix = P.splat_start()
    rc = RegistrationController(repo, ui)
    r = rc.refine_photometric(_cameras(P.plane_cameras(P.E2E["width"], P.E2E["height"])), _e2e_params(scales=(4,), max_iteration=4))
    assert np.array_equal(ui.transformation_matrix, r.transformation) and np.linalg.norm(r.transformation[:2, 3]) < 0.1 * np.linalg.norm(P.splat_start()[:2, 3])
    assert len(r.trace) == 1 and r.trace[0]["width"] == 24 and 1 <= r.iterations <= 4


# ---- degenerate runs -----------------------------------------------------------------------------------------------------------------
def test_cameras_that_look_away_return_the_initial_transform():
    from gaussiansplattingregistration_amd import photo
    model = _gaussian_model(P.splat_plane())
    away = [dict(c, viewmat=P.look_at(np.linalg.inv(c["viewmat"])[:3, 3], 2 * np.linalg.inv(c["viewmat"])[:3, 3])) for c in P.plane_cameras(96, 72)]
    T0 = P.splat_start()
    r = photo.PhotometricRefiner(model, model, _cameras(away), _e2e_params(), init=T0).run()
    assert np.array_equal(r.transformation, T0) and r.n_pixels == 0 and r.iterations == 0 and r.energy_final is None
    assert len(r.error_list) == 1 and "no camera has a counted pixel" in r.error_list[0]
    # one camera of two looks away: it is named and skipped, the other one does the work
    cams = _cameras([P.plane_cameras(96, 72)[0], dict(away[1], image_name="away")])
    r = photo.PhotometricRefiner(model, model, cams, _e2e_params(scales=(2,), max_iteration=6), init=T0).run()
    assert r.n_pixels_per_camera[0] > 0 and r.n_pixels_per_camera[1] == 0 and any(e.startswith("away:") for e in r.error_list)
    assert np.linalg.norm(r.transformation[:2, 3]) < 0.1 * np.linalg.norm(T0[:2, 3])


def test_no_iteration_returns_the_initial_transform_and_cancel_returns_none():
    from gaussiansplattingregistration_amd import photo
    model = _gaussian_model(P.splat_plane())
    cams = _cameras(P.plane_cameras(96, 72))
    T0 = P.splat_start()
    r = photo.PhotometricRefiner(model, model, cams, _e2e_params(scales=(1,), max_iteration=0), init=T0).run()
    assert np.array_equal(r.transformation, T0) and r.iterations == 0 and r.n_pixels > 0 and r.energy_final == r.energy_initial > 0 and not r.error_list
    w = photo.PhotometricRefiner(model, model, cams, _e2e_params(), init=T0)
    w.cancel()
    assert w.run() is None


# ---- the command-line tool ---------------------------------------------------------------------------------------------------------------
def test_evaluate_registration_script_refines_and_logs_without_and_with(tmp_path, monkeypatch, capsys):
    """``evaluate_registration.py --geometry --photo-refine`` on the splat plane written as a 3DGS file twice, with ``splat_start`` as the
    transform: the depth log is written without and with the refinement, the depth agreement is no worse with it, and the printed
    transform has lost the in-plane error"""
    import importlib.util
    from conftest import ROOT
    from gaussiansplattingregistration_amd.utils import ply_io
    sc = P.splat_plane()
    n = len(sc["xyz"])
    scale = 0.5 * np.log(np.stack([sc["cov6"][:, 0], sc["cov6"][:, 3], sc["cov6"][:, 5]], 1).astype(np.float64))
    quat = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    for name in ("a.ply", "b.ply"):
        ply_io.save_gaussian_ply(str(tmp_path / name), sc["xyz"].astype(np.float64), sc["color"].astype(np.float64), np.zeros((n, 9)), sc["opacity"].astype(np.float64),
                                 scale, quat)
    T0 = P.splat_start()
    np.savetxt(tmp_path / "T.txt", T0)
    entries = []
    for k, c in enumerate(P.plane_cameras(P.E2E["width"], P.E2E["height"])):
        V = np.asarray(c["viewmat"], np.float64)
        entries.append({"id": k, "img_name": c["image_name"], "width": c["width"], "height": c["height"], "fx": c["fx"], "fy": c["fy"],
                        "rotation": V[:3, :3].T.tolist(), "position": (-V[:3, :3].T @ V[:3, 3]).tolist()})
    (tmp_path / "cameras.json").write_text(json.dumps(entries))
    monkeypatch.setattr("sys.argv", ["evaluate_registration.py", str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--transform", str(tmp_path / "T.txt"),
                                     "--cameras", str(tmp_path / "cameras.json"), "--geometry", "--log", str(tmp_path / "geo.json"), "--photo-refine",
                                     "--photo-max-depth-diff", "0.5"])
    spec = importlib.util.spec_from_file_location("evaluate_registration", os.path.join(ROOT, "scripts", "evaluate_registration.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main()
    lines = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    before = next(r for r in lines if r.get("photo_refine") is False)
    after = next(r for r in lines if r.get("photo_refine") is True)
    final = next(r for r in lines if "cameras" in r)
    T = np.array(after["transformation"])
    assert after["energy_final"] < after["energy_initial"] and after["n_pixels"] > 0
    assert np.linalg.norm(T[:2, 3]) < 0.1 * np.linalg.norm(T0[:2, 3]) and P.pose_error(T)[1] < 0.1 * P.pose_error(T0)[1]
    assert os.path.exists(tmp_path / "geo.json") and os.path.exists(str(tmp_path / "geo.json") + ".no_photo_refine")
    print("depth_rmse without / with the refinement:", before["depth_rmse"], final["depth_rmse"], "overlap", before["depth_overlap"], final["depth_overlap"])
    # with the refined transform the two renders are of the same splats in the same place: they agree to the float32 of the renderer
    # (4 x 7.3e-6 relative, raster_aux_tolerance.json, of a depth below 3)
    assert final["depth_rmse"] < 1e-4 and final["depth_rmse"] < before["depth_rmse"] and final["depth_overlap"] >= before["depth_overlap"]
