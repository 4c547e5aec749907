"""The HIP rasteriser against the float64 NumPy model (tests/raster_model.py), the metrics kernel against the reference's recorded
values, the evaluator end to end, and one full-size render.

Tolerance of the image comparison: tests/golden/raster_tolerance.json records, per scene, the largest difference between the model
run in float32 and in float64 over the non-fragile pixels (what float32 costs the model itself); the kernel may differ from the
float64 model by 4 x that (another summation order of the LDS batches, the device exp).  Fragile pixels (a discrete decision within
1e-4 of its threshold, at most 1 % of an image: tests/test_raster_cpu.py) must be finite and within the sum of the alphas of the
splats flagged there (every flag carries an alpha of at least (1 - 1e-4) / 255).
"""
import json
import os

import numpy as np
import pytest
import torch

import raster_model as M
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_cache = {}


def _model(name):
    """the float64 model's render of a scene, computed once and left unchanged"""
    if name not in _cache:
        scene, cam, bg = M.build(name)
        r = M.render(M.scaled(scene), cam, bg)
        r["image"].setflags(write=False)
        _cache[name] = (scene, cam, bg, r)
    return _cache[name]


def _gaussian_model(scene, device):
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    return GaussianModel(device).from_arrays(scene["xyz"], scene["color"], scene["opacity"], scene["cov6"], scene["sh"], scene["sh_degree"])


def _render(scene, cam, bg, host=False, with_stats=True):
    from gaussiansplattingregistration_amd import raster
    s = M.scaled(scene)
    conv = (lambda a: a) if host else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())
    K = (scene["sh_degree"] + 1) ** 2 - 1
    img, stats = raster.context(0).render(conv(s["xyz"]), conv(s["cov6"]), conv(s["opacity"]), conv(s["color"]), conv(s["sh"].reshape(-1, K, 3)) if K else None,
                                          s["sh_degree"], cam["viewmat"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"], bg, 3.0,
                                          with_stats=True)
    return img.cpu().numpy(), stats.cpu().numpy()


# every scene from CUDA tensors; host arrays take the same kernels after one upload: two scenes cover that path
RENDER_CASES = [(name, False) for name in M.SCENES] + [("deg0_black", True), ("deg3_white_odd", True)]


@pytest.mark.parametrize("name,host", RENDER_CASES, ids=[f"{n}-{'host_arrays' if h else 'cuda_tensors'}" for n, h in RENDER_CASES])
def test_render_matches_the_float64_model(name, host):
    scene, cam, bg, want = _model(name)
    got, stats = _render(scene, cam, bg, host=host)
    tol = 4.0 * json.load(open(os.path.join(GOLDEN, "raster_tolerance.json")))[name]["float32_model_max_abs_diff"]
    assert got.shape == want["image"].shape and np.isfinite(got).all()
    d = np.abs(got.astype(np.float64) - want["image"]).max(axis=2)
    frag = want["fragile"]
    assert frag.mean() <= 0.01
    err = d[~frag].max()
    print(f"{name}: max |gpu - float64 model| on non-fragile pixels {err:.3e} (allowed {tol:.3e}); fragile {frag.mean():.4f}; stats {stats.tolist()} "
          f"model {(want['visible'], want['intersections'], want['nonempty_tiles'])}")
    assert err <= tol, (err, tol)
    assert (d[frag] <= want["fragile_alpha"][frag]).all()
    if not frag.any():
        assert stats.tolist() == [want["visible"], want["intersections"], want["nonempty_tiles"]]


def test_exact_scene_has_an_empty_fragile_mask_and_equal_counts():
    scene, cam, bg, want = _model(M.EXACT_SCENE)
    assert not want["fragile"].any()
    _, stats = _render(scene, cam, bg)
    assert stats.tolist() == [want["visible"], want["intersections"], want["nonempty_tiles"]]


def test_two_renders_are_bit_identical():
    scene, cam, bg, _ = _model("giants_tiny")
    a, sa = _render(scene, cam, bg)
    b, sb = _render(scene, cam, bg)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(sa, sb)


def test_rasterize_image_through_the_model_and_a_second_camera():
    """the reference-named entry: GaussianModel + Camera, scale != 1 through get_full_covariance, two cameras of one scene"""
    from gaussiansplattingregistration_amd.models.camera import Camera
    from gaussiansplattingregistration_amd.utils.rasterization_util import rasterize_image
    scene, cam, bg, want = _model("scaled")
    model = _gaussian_model(scene, "cuda:0")
    tol = 4.0 * json.load(open(os.path.join(GOLDEN, "raster_tolerance.json")))["scaled"]["float32_model_max_abs_diff"]
    V = cam["viewmat"].astype(np.float64)
    c = Camera(V[:3, :3].T, V[:3, 3], cam["fx"], cam["fy"], "v", cam["width"], cam["height"])
    assert np.abs(c.viewmat[0].numpy() - cam["viewmat"]).max() < 1e-6
    cam2 = dict(cam, viewmat=c.viewmat[0].numpy())
    want2 = M.render(M.scaled(scene), cam2, bg)
    img = rasterize_image(model, c, scene["scale"], bg, "cuda:0")
    assert tuple(img.shape) == (1, cam["height"], cam["width"], 3) and img.is_cuda
    d = np.abs(img[0].cpu().numpy().astype(np.float64) - want2["image"]).max(axis=2)
    assert want2["fragile"].mean() <= 0.01
    assert d[~want2["fragile"]].max() <= tol
    assert (d[want2["fragile"]] <= want2["fragile_alpha"][want2["fragile"]]).all()
    host = rasterize_image(model, c, scene["scale"], bg, "cuda:0", leave_on_gpu=False)
    assert not host.is_cuda and torch.equal(host, img.cpu())
    # another camera of the same model: a different image, held to the model the same way
    cam3 = M.make_camera((-1.5, 0.8, -2.5), (0.0, 0.0, 0.0), 112, 64, 95.0)
    want3 = M.render(M.scaled(scene), cam3, bg)
    assert want3["fragile"].mean() <= 0.01
    got3, _ = _render(scene, cam3, bg)
    d3 = np.abs(got3.astype(np.float64) - want3["image"]).max(axis=2)
    assert d3[~want3["fragile"]].max() <= tol
    assert (d3[want3["fragile"]] <= want3["fragile_alpha"][want3["fragile"]]).all()


@pytest.mark.parametrize("on_device", [True, False], ids=["cuda_tensors", "host_arrays"])
def test_metrics_kernel_against_the_reference(on_device):
    from gaussiansplattingregistration_amd import raster
    from gaussiansplattingregistration_amd.utils import evaluation_utils as E
    g = dict(np.load(os.path.join(GOLDEN, "eval_metrics.npz")))
    for name, (a, b) in M.image_pairs().items():
        ref, f64 = g[f"{name}_ref"], g[f"{name}_f64"]
        ta, tb = (torch.from_numpy(x).cuda() for x in (a, b)) if on_device else (a, b)
        mse, ssim = raster.image_metrics(ta, tb)
        tol_ssim = 4.0 * abs(ref[2] - f64[2])          # what float32 cost the reference itself, x 4
        print(f"{name}: mse {mse:.9g} (ref {ref[0]:.9g})  ssim {ssim:.12g} (ref {ref[2]:.9g}, float64 {f64[2]:.12g}, allowed {tol_ssim:.3e})")
        assert abs(mse - ref[0]) <= 1e-6 * ref[0]
        assert abs(ssim - ref[2]) <= tol_ssim
        if on_device:                                  # the reference-named functions on (1,3,H,W) CUDA tensors
            assert float(E.mse(ta[None], tb[None])) == pytest.approx(ref[0], rel=1e-6)
            assert float(E.ssim(ta[None], tb[None])) == pytest.approx(ref[2], abs=tol_ssim + 6e-8)      # + half a float32 ulp: the tensor it returns
            if np.isfinite(ref[1]):
                tol_psnr = max(4.0 * abs(ref[1] - f64[1]), 1e-5)
                assert float(E.psnr(ta[None], tb[None])) == pytest.approx(ref[1], abs=tol_psnr)


@pytest.fixture(scope="module")
def pair20k():
    """synth.make_pair at 20 000 splats with DC colours that keep every splat colour, hence every pixel, within [0, 1]"""
    from gaussiansplattingregistration_amd import synth
    src, tgt, T_gt = synth.make_pair(20000, seed=9, sh_degree=1)
    rng = np.random.default_rng(99)
    for c in (src, tgt):
        c["color"] = ((rng.uniform(0.2, 0.8, c["color"].shape) - 0.5) / M.C0).astype(np.float32)
        c["sh"] = (c["sh"] * 0.2).astype(np.float32)
    h = tgt["h"]
    cams = [M.make_camera(e, (0, 0, 0), 160, 120, 130.0) for e in ((0.0, 0.0, -3.5 * h), (3.0 * h, 0.5 * h, -2.0 * h), (-2.5 * h, -1.0 * h, -2.5 * h))]
    return src, tgt, T_gt, cams


def test_end_to_end_evaluation(pair20k, tmp_path):
    from PIL import Image
    from gaussiansplattingregistration_amd import synth
    from gaussiansplattingregistration_amd.models.camera import Camera
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.utils.rasterization_util import rasterize_image
    from gaussiansplattingregistration_amd.workers.evaluator import RegistrationEvaluator
    src, tgt, T_gt, cam_dicts = pair20k
    mk = lambda c: GaussianModel("cuda:0").from_arrays(c["xyz"], c["color"], c["opacity"], c["cov6"], c["sh"], c["sh_degree"])
    pc1, pc2 = mk(src), mk(tgt)
    cams = []
    for k, cd in enumerate(cam_dicts):
        V = cd["viewmat"].astype(np.float64)
        cams.append(Camera(V[:3, :3].T, V[:3, 3], cd["fx"], cd["fy"], f"view_{k}", cd["width"], cd["height"]))
    merged = GaussianModel.get_merged_gaussian_point_clouds(pc1, pc2, T_gt)
    # the CPU model of one camera: every pixel within [0, 1], so the 8-bit PNG loses at most half a step
    m = {k: t.cpu().numpy() for k, t in (("xyz", merged.get_xyz), ("cov6", merged.get_covariance()), ("opacity", merged.get_raw_opacity.reshape(-1)),
                                         ("color", merged.get_colors), ("sh", merged.get_spherical_harmonics))}
    m["sh_degree"] = merged.sh_degree
    cd0 = dict(cam_dicts[0], viewmat=cams[0].viewmat[0].numpy())
    model0 = M.render(m, cd0, (0.0, 0.0, 0.0), np.float32)["image"]
    assert model0.min() >= 0.0 and model0.max() <= 1.0
    for cam in cams:
        img = rasterize_image(merged, cam, 1, (0, 0, 0), "cuda:0")[0].cpu().numpy()
        assert img.min() >= 0.0 and img.max() <= 1.0
        Image.fromarray(np.floor(img * 255.0 + 0.5).astype(np.uint8)).save(tmp_path / (cam.image_name + ".png"))
    good = RegistrationEvaluator(pc1, pc2, T_gt, cams, str(tmp_path), str(tmp_path / "good.json"), (0, 0, 0), None, True).run()
    print("T_gt: mse %.3e rmse %.3e psnr %.2f ssim %.6f" % (good.mse, good.rmse, good.psnr, good.ssim))
    assert good.mse <= (0.5 / 255.0) ** 2 * (1 + 1e-3)
    assert json.load(open(tmp_path / "good.json"))["lpips"] is None
    T_off = synth.rigid_transform(5.0, (0.3, 1.0, 0.2)) @ T_gt
    bad = RegistrationEvaluator(pc1, pc2, T_off, cams, str(tmp_path), str(tmp_path / "bad.json"), (0, 0, 0), None, True).run()
    print("5 degrees off: mse %.3e psnr %.2f ssim %.6f" % (bad.mse, bad.psnr, bad.ssim))
    assert bad.psnr < good.psnr and bad.ssim < good.ssim


def _write_ply(path, n, seed, T=None):
    """a small 3DGS file (SH degree 1, colours within [0, 1]); with T, the same splats moved rigidly (positions and orientations)"""
    from gaussiansplattingregistration_amd import synth
    from gaussiansplattingregistration_amd.utils import ply_io
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1, 1, (n, 3))
    scale = rng.normal(-2.8, 0.3, (n, 3))
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    if T is not None:
        xyz = xyz @ T[:3, :3].T + T[:3, 3]
        R = T[:3, :3] @ synth._quat_to_rot(q)
        w = np.maximum(np.sqrt(np.maximum(0.0, 1.0 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2])) / 2, 1e-6)
        q = np.stack([w, (R[:, 2, 1] - R[:, 1, 2]) / (4 * w), (R[:, 0, 2] - R[:, 2, 0]) / (4 * w), (R[:, 1, 0] - R[:, 0, 1]) / (4 * w)], 1)
    dc = (rng.uniform(0.2, 0.8, (n, 3)) - 0.5) / M.C0
    ply_io.save_gaussian_ply(path, xyz, dc, rng.normal(0, 0.02, (n, 9)), rng.normal(1.0, 1.0, n), scale, q)


def test_headless_script_and_controller_on_ply_files(tmp_path, monkeypatch, capsys):
    """scripts/evaluate_registration.py on two .ply files, a cameras.json, a T.txt and PNGs: through the controller, and through the
    worker with --save-renders; both write the reference's log"""
    import importlib.util
    from PIL import Image
    from gaussiansplattingregistration_amd import synth
    from gaussiansplattingregistration_amd.models.camera import load_cameras
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.utils.rasterization_util import rasterize_image
    from conftest import ROOT
    T = synth.rigid_transform(12.0, (0.2, 1.0, 0.4), (0.3, -0.1, 0.2))
    _write_ply(tmp_path / "a.ply", 3000, 1, np.linalg.inv(T))             # a.ply moved by T lies in b.ply's frame
    _write_ply(tmp_path / "b.ply", 2500, 2)
    np.savetxt(tmp_path / "T.txt", T)
    entries = []
    for k, eye in enumerate(((0.0, 0.0, -4.0), (3.0, 1.0, -2.5))):
        V = M.look_at(eye, (0, 0, 0)).astype(np.float64)
        entries.append({"id": k, "img_name": f"photo_{k}", "width": 144, "height": 100, "fx": 150.0, "fy": 155.0, "rotation": V[:3, :3].T.tolist(),
                        "position": list(eye)})
    (tmp_path / "cameras.json").write_text(json.dumps(entries))
    images = tmp_path / "images"
    images.mkdir()
    cams = load_cameras(str(tmp_path / "cameras.json"))
    pc1, pc2 = (GaussianModel("cuda:0").from_ply(str(tmp_path / f)) for f in ("a.ply", "b.ply"))
    merged = GaussianModel.get_merged_gaussian_point_clouds(pc1, pc2, T)
    for cam in cams[:1]:                                                     # photo_1 stays missing: one entry of error_list
        img = rasterize_image(merged, cam, 1, (0, 0, 0), "cuda:0")[0].cpu().numpy()
        assert 0.0 <= img.min() and img.max() <= 1.0 and img.max() > 0.3
        Image.fromarray(np.floor(img * 255.0 + 0.5).astype(np.uint8)).save(images / (cam.image_name + ".png"))
    spec = importlib.util.spec_from_file_location("evaluate_registration", os.path.join(ROOT, "scripts", "evaluate_registration.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    base = ["evaluate_registration.py", str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--transform", str(tmp_path / "T.txt"), "--cameras",
            str(tmp_path / "cameras.json"), "--images", str(images)]
    logs = []
    for tag, extra in (("controller", []), ("worker", ["--save-renders", str(tmp_path / "renders")])):
        monkeypatch.setattr("sys.argv", base + ["--log", str(tmp_path / f"{tag}.json")] + extra)
        script.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        log = json.loads((tmp_path / f"{tag}.json").read_text())
        assert list(log) == ["registration_data", "mse", "rmse", "ssim", "psnr", "lpips", "error_list"]
        assert log["lpips"] is None and log["registration_data"] == {}
        assert len(log["error_list"]) == 2 and "photo_1" in log["error_list"][0] and "lpips" in log["error_list"][1]
        assert 0.0 < log["mse"] <= (0.5 / 255.0) ** 2 * (1 + 1e-3) and log["ssim"] > 0.99 and log["psnr"] > 50.0
        assert log["rmse"] == pytest.approx(np.sqrt(log["mse"]), rel=1e-12)
        assert line["cameras"] == 2 and line["mse"] == log["mse"] and line["errors"] == 2
        logs.append(log)
    assert logs[0] == logs[1]
    saved = np.asarray(Image.open(tmp_path / "renders" / "photo_0.png"))
    assert np.array_equal(saved, np.asarray(Image.open(images / "photo_0.png")))
    assert not (tmp_path / "renders" / "photo_1.png").exists()


def test_full_size_render():
    """the merged 2 x 1 M pair (config C2's size) at 1280 x 720: status 0, a finite image, the background alone where no splat reaches"""
    from gaussiansplattingregistration_amd import raster, synth
    n = 1_000_000
    a = synth.make_cloud_torch(n, seed=1, device="cuda:0", sh_degree=3)
    T = synth.rigid_transform(5.0, (1, 1, 1), (0.1, -0.1, 0.05))
    b = synth.apply_rigid_torch(a, T)
    cat = lambda k: torch.cat((a[k], b[k])).contiguous()
    h = a["h"]
    cam = M.make_camera((0.0, 0.0, -4.0 * h), (0, 0, 0), 1280, 720, 1100.0)
    bg = (0.25, 0.5, 0.75)
    ctx = raster.context(0)
    img, stats = ctx.render(cat("xyz"), cat("cov6"), cat("opacity"), cat("color"), cat("sh").reshape(2 * n, 15, 3), 3, cam["viewmat"], cam["fx"], cam["fy"],
                            cam["cx"], cam["cy"], 1280, 720, bg, 3.0, with_stats=True)
    torch.cuda.synchronize()
    t = ctx.timing()
    stats = stats.cpu().numpy()
    print("full size: stats", stats.tolist(), "ms", t)
    assert torch.isfinite(img).all()
    assert stats[0] > 0 and stats[1] >= stats[0] and 0 < stats[2] <= 80 * 45
    # the box spans about +-(h + 3 sigma) / (3 h) * focal = 400 px around the centre: the image's corners see no splat
    corner = img[:16, :16].reshape(-1, 3)
    assert torch.equal(corner, torch.tensor(bg, device="cuda").expand_as(corner))
    centre = img[352:368, 632:648].reshape(-1, 3)
    assert not torch.equal(centre, torch.tensor(bg, device="cuda").expand_as(centre))
