"""The evaluation stage without a GPU: cameras against the reference's matrices, the NumPy model of the rasteriser against what can
be said about it analytically, the conditions tests/test_raster_gpu.py relies on (fragile fractions, colour range), the new C-ABI
entries without a device, and the evaluator's log."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import raster_model as M
from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "eval_metrics.npz")))


def test_camera_and_loader_equal_the_reference(golden, tmp_path):
    from gaussiansplattingregistration_amd.models.camera import load_cameras
    path = tmp_path / "cameras.json"
    path.write_text(str(golden["cameras_json"]))
    cams = load_cameras(str(path))
    entries = json.loads(str(golden["cameras_json"]))
    assert len(cams) == 3
    for k, (cam, e) in enumerate(zip(cams, entries)):
        assert tuple(cam.viewmat.shape) == (1, 4, 4) and tuple(cam.intrinsics.shape) == (1, 3, 3)
        assert np.array_equal(cam.viewmat[0].numpy(), golden[f"cam{k}_viewmat"])
        assert np.array_equal(cam.intrinsics[0].numpy(), golden[f"cam{k}_intrinsics"])
        assert (cam.image_name, cam.width, cam.height) == (e["img_name"], e["width"], e["height"])


def _one_splat(s=0.05, depth=4.0, op_raw=1.2, f=120.0, W=96, H=80):
    scene = dict(xyz=np.float32([[0, 0, depth]]), cov6=np.float32([[s * s, 0, 0, s * s, 0, s * s]]), opacity=np.float32([op_raw]),
                 color=np.float32([[1.0, -0.5, 0.25]]), sh=np.zeros((1, 0), np.float32), sh_degree=0)
    cam = dict(viewmat=np.eye(4, dtype=np.float32), fx=f, fy=f, cx=W / 2, cy=H / 2, width=W, height=H)
    return scene, cam


def test_model_single_isotropic_splat_is_the_analytic_image():
    s, depth, op_raw, f, W, H = 0.0625, 4.0, 1.25, 120.0, 96, 80     # all exact in float32: the model widens float32 inputs
    scene, cam = _one_splat(s, depth, op_raw, f, W, H)
    bg = np.array([0.25, 0.5, 0.75])
    r = M.render(scene, cam, bg)
    a = (f * s / depth) ** 2 + 0.3                               # the projected variance plus the dilation, both axes
    radius = np.ceil(3 * np.sqrt(a + np.sqrt(max(0.01, 0.0))))   # b = a, det = a^2: b^2 - det = 0
    yy, xx = np.mgrid[0:H, 0:W]
    dx, dy = W / 2 - (xx + 0.5), H / 2 - (yy + 0.5)
    alpha = np.minimum(0.999, 1 / (1 + np.exp(-op_raw)) * np.exp(-0.5 * (dx * dx + dy * dy) / a))
    x0, x1 = int(np.floor((W / 2 - radius) / 16)) * 16, int(np.ceil((W / 2 + radius) / 16)) * 16
    y0, y1 = int(np.floor((H / 2 - radius) / 16)) * 16, int(np.ceil((H / 2 + radius) / 16)) * 16
    inbox = (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)
    alpha = np.where(inbox & (alpha >= 1 / 255), alpha, 0.0)
    colour = np.maximum(M.C0 * np.array([1.0, -0.5, 0.25]) + 0.5, 0)
    want = alpha[:, :, None] * colour + (1 - alpha[:, :, None]) * bg
    assert r["visible"] == 1 and r["intersections"] == ((x1 - x0) // 16) * ((y1 - y0) // 16)
    assert np.abs(r["image"] - want).max() < 1e-12
    assert alpha.max() > 0.7 and (alpha > 0).sum() > 20


@pytest.mark.parametrize("point", [(0.7, -0.4, 3.0), (2.9, 0.3, 2.5)], ids=["off_axis", "beyond_the_clamped_frustum"])
def test_model_single_anisotropic_splat_off_axis(point):
    """The projection written independently with matrix algebra (J Sigma J^T, eigenvalues for the radius): the off-diagonal Jacobian
    terms, the camera rotation and the frustum clamp all take part.  The second point lies outside the widened frustum, so its
    Jacobian is taken at the clamped position while its mean is not."""
    W, H, fx, fy = 160, 96, 100.0, 120.0
    ang = np.deg2rad(20.0)
    Rv = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]) @ np.array([[1, 0, 0], [0, 0.8, -0.6], [0, 0.6, 0.8]])
    V = np.eye(4)
    V[:3, :3], V[:3, 3] = Rv, [0.25, -0.5, 1.0]
    V = V.astype(np.float32)
    A = np.float32([[0.30, 0.05, -0.02], [0.0, 0.12, 0.04], [0.0, 0.0, 0.45]])
    S = (A.astype(np.float64) @ A.astype(np.float64).T).astype(np.float32)
    pw = (np.linalg.inv(V.astype(np.float64)) @ np.array([*point, 1.0]))[:3].astype(np.float32)
    scene = dict(xyz=pw[None], cov6=S[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]][None], opacity=np.float32([2.0]), color=np.float32([[0.5, -1.0, 1.0]]),
                 sh=np.zeros((1, 0), np.float32), sh_degree=0)
    cam = dict(viewmat=V, fx=fx, fy=fy, cx=W / 2, cy=H / 2, width=W, height=H)
    bg = np.array([0.5, 0.25, 0.0])
    r = M.render(scene, cam, bg)
    # the independent computation, float64 from the same float32 inputs
    V64, S64 = V.astype(np.float64), S.astype(np.float64)
    x, y, z = V64[:3, :3] @ pw.astype(np.float64) + V64[:3, 3]
    lim_x, lim_y = 1.3 * (W / 2) / fx, 1.3 * (H / 2) / fy                    # centred principal point: both sides alike
    xc, yc = np.clip(x / z, -lim_x, lim_x) * z, np.clip(y / z, -lim_y, lim_y) * z
    if point[0] > 2:
        assert abs(x / z) > lim_x                                               # the clamp is really active
    J = np.array([[fx / z, 0, -fx * xc / z ** 2], [0, fy / z, -fy * yc / z ** 2]])
    S2 = J @ V64[:3, :3] @ S64 @ V64[:3, :3].T @ J.T + 0.3 * np.eye(2)
    Q = np.linalg.inv(S2)
    mean = np.array([fx * x / z + W / 2, fy * y / z + H / 2])
    lam = np.linalg.eigvalsh(S2).max()
    assert (0.5 * np.trace(S2)) ** 2 - np.linalg.det(S2) > 0.01                 # the floor under the root plays no part here
    radius = np.ceil(3 * np.sqrt(lam))
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.stack([mean[0] - (xx + 0.5), mean[1] - (yy + 0.5)], -1)
    sigma = 0.5 * np.einsum("...i,ij,...j->...", d, Q, d)
    alpha = np.minimum(0.999, 1 / (1 + np.exp(-2.0)) * np.exp(-sigma))
    tx0, tx1 = np.clip([np.floor((mean[0] - radius) / 16), np.ceil((mean[0] + radius) / 16)], 0, W // 16).astype(int)
    ty0, ty1 = np.clip([np.floor((mean[1] - radius) / 16), np.ceil((mean[1] + radius) / 16)], 0, H // 16).astype(int)
    inbox = (xx >= 16 * tx0) & (xx < 16 * tx1) & (yy >= 16 * ty0) & (yy < 16 * ty1)
    alpha = np.where(inbox & (alpha >= 1 / 255), alpha, 0.0)
    colour = np.maximum(M.C0 * np.array([0.5, -1.0, 1.0]) + 0.5, 0)
    want = alpha[:, :, None] * colour + (1 - alpha[:, :, None]) * bg
    assert r["visible"] == 1 and r["intersections"] == (tx1 - tx0) * (ty1 - ty0) > 0
    assert (alpha > 0).sum() > 200 and abs(S2[0, 1]) > 1.0                      # a visible, really anisotropic footprint
    assert np.abs(r["image"] - want).max() < 1e-9


def test_model_is_invariant_to_the_input_order():
    scene, cam, bg = M.build("deg3_white_odd")
    s = M.scaled(scene)
    z = M.project(s, cam)["z"]
    assert len(np.unique(z)) == len(z)                           # no two depths tie
    perm = np.random.default_rng(5).permutation(len(z))
    p = dict(s, **{k: s[k][perm] for k in ("xyz", "cov6", "opacity", "color", "sh")})
    a, b = M.render(s, cam, bg), M.render(p, cam, bg)
    assert np.array_equal(a["image"], b["image"])
    assert (a["visible"], a["intersections"], a["nonempty_tiles"]) == (b["visible"], b["intersections"], b["nonempty_tiles"])


@pytest.mark.parametrize("name", list(M.SCENES))
def test_scenes_meet_the_conditions_of_the_gpu_test(name):
    """fragile pixels at most 1 % (none in the exact scene), colours within [0, 1], the recorded float32 cost is the model's"""
    scene, cam, bg = M.build(name)
    s = M.scaled(scene)
    r64, r32 = M.render(s, cam, bg), M.render(s, cam, bg, np.float32)
    frac = r64["fragile"].mean()
    assert frac <= 0.01, frac
    if name == M.EXACT_SCENE:
        assert frac == 0.0
        assert (r64["visible"], r64["intersections"]) == (r32["visible"], r32["intersections"])
    assert r64["max_rgb"] <= 1.0 and r64["image"].max() <= 1.0 and r64["image"].min() >= 0.0
    assert 0 < r64["visible"] < len(s["xyz"])                    # something is culled in every scene
    tol = json.load(open(os.path.join(GOLDEN, "raster_tolerance.json")))[name]
    d = np.abs(r32["image"].astype(np.float64) - r64["image"])[~r64["fragile"]].max()
    assert d == pytest.approx(tol["float32_model_max_abs_diff"], rel=1e-6, abs=1e-12)
    assert d < 2e-5                                              # a few float32 ulps of a value in [0, 1], summed over the splats of a pixel


def test_scene_features_are_really_there():
    """behind the camera / beyond the frame, giants over every tile, a cluster at or under the 3-pixel clip"""
    scene, cam, bg = M.build("giants_tiny")
    P = M.project(M.scaled(scene), cam)
    whole = (P["x1"] - P["x0"] == P["tiles_x"]) & (P["y1"] - P["y0"] == P["tiles_y"]) & P["ok"]
    assert whole[:3].all()
    tiny = slice(3, 153)
    assert (P["rad"][tiny] <= 3).sum() > 20 and (P["rad"][tiny] > 3).sum() > 20
    scene, cam, bg = M.build("inside")
    P = M.project(M.scaled(scene), cam)
    assert (P["z"] < M.NEAR).sum() > 100
    assert ((P["z"] > M.NEAR) & (P["rad"] > 3) & ~P["ok"]).sum() > 100       # in front, large enough, outside the frame


def test_model_metrics_match_the_recorded_float64(golden):
    pairs = M.image_pairs()
    assert sorted(pairs) == sorted(str(n) for n in golden["names"])
    for name, (a, b) in pairs.items():
        assert np.allclose([a.astype(np.float64).sum(), b.astype(np.float64).sum()], golden[f"{name}_sum"], rtol=1e-12)
        got, want = np.array(M.metrics64(a, b)), golden[f"{name}_f64"]
        assert np.allclose(got[[0, 2]], want[[0, 2]], rtol=1e-12, atol=0)


def test_new_abi_entries_without_a_device(hip_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    h = C.c_void_p()
    assert hip_lib.gsr_raster_create(C.byref(h), 0, None) == -3                 # GSR_E_NO_DEVICE
    msg = hip_lib.gsr_last_error()
    assert b"no HIP device" in msg and b"gsr_raster_create" in msg, msg
    assert not h.value
    a = np.zeros((3, 8, 8), np.float32)
    out = (C.c_double * 2)()
    assert hip_lib.gsr_image_metrics(a.ctypes.data, a.ctypes.data, 8, 8, 0, out, 0, None) == -3
    msg = hip_lib.gsr_last_error()
    assert b"no HIP device" in msg and b"gsr_image_metrics" in msg, msg
    assert hip_lib.gsr_raster_render(None, 0, 0, 0, None, None, None, None, None, None, 1.0, 1.0, 0.0, 0.0, 8, 8, None, 3.0, None, None, None) == -1
    assert b"gsr_raster_render" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_raster_destroy(None) == 0
    from gaussiansplattingregistration_amd import raster
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raster.RasterContext()


def test_evaluator_logs_a_missing_image_and_writes_the_json(golden, tmp_path):
    from gaussiansplattingregistration_amd.models.camera import cameras_from_json
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.workers.evaluator import RegistrationEvaluator
    scene, _, _ = M.build(M.EXACT_SCENE)
    mk = lambda: GaussianModel("cpu").from_arrays(scene["xyz"], scene["color"], scene["opacity"], scene["cov6"], scene["sh"], scene["sh_degree"])
    cams = cameras_from_json(json.loads(str(golden["cameras_json"])))
    (tmp_path / (cams[1].image_name + ".png")).write_bytes(b"this is not a PNG file")
    log = tmp_path / "eval.json"
    # no camera has a readable photograph (two missing, one not an image): nothing is rendered, the log is still written
    ev = RegistrationEvaluator(mk(), mk(), np.eye(4), cams, str(tmp_path), str(log), (0, 0, 0), None, False)
    result = ev.run()
    data = json.loads(log.read_text())
    assert sorted(data) == ["error_list", "lpips", "mse", "psnr", "registration_data", "rmse", "ssim"]
    assert data["lpips"] is None and result.lpips is None
    assert data["registration_data"] == {}
    errs = data["error_list"]
    assert len(errs) == 4 and cams[0].image_name in errs[0] and cams[1].image_name in errs[1] and "lpips" in errs[-1].lower()


def test_evaluator_cancel_is_polled_between_cameras(golden, tmp_path):
    from gaussiansplattingregistration_amd.models.camera import cameras_from_json
    from gaussiansplattingregistration_amd.workers.evaluator import RegistrationEvaluator
    cams = cameras_from_json(json.loads(str(golden["cameras_json"])))
    ev = RegistrationEvaluator(None, None, np.eye(4), cams, str(tmp_path), str(tmp_path / "log.json"), (0, 0, 0), None, False)
    ev.cancel_evaluation()
    assert ev.run() is None and not (tmp_path / "log.json").exists()


def test_ssim_with_another_window_raises():
    import torch
    from gaussiansplattingregistration_amd.utils import evaluation_utils as E
    a = torch.zeros(1, 3, 16, 16)
    with pytest.raises(NotImplementedError):
        E.ssim(a, a, window_size=7)
    with pytest.raises(NotImplementedError):
        E.ssim(a, a, size_average=False)
    assert float(E.ssim(a + 0.5, a + 0.5)) == pytest.approx(1.0, abs=1e-6)
    assert float(E.mse(a, a + 0.5)) == pytest.approx(0.25)
