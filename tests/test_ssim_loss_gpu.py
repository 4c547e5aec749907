"""The fused L1 + D-SSIM loss kernel (gsr_loss_l1_dssim, csrc/imgloss.hip) against the model of tests/ssim_loss_model.py
in np.longdouble, its autograd front, the fine-tuner with ``loss="l1_dssim"`` and the script flag.

Tolerance: tests/golden/ssim_loss_tolerance.json records per scene and lambda what float64 costs the model itself against the same
function one precision higher (tests/test_ssim_loss_cpu.py checks the file against the model); the kernel gets 4 x that (the margin of
tests/test_raster_gpu.py and tests/test_raster_grad_gpu.py), and every gradient entry besides ``2^-24 |g|``: the one rounding to float32
at the store, which the model does not make.  Every image is at most 40 x 50.
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import raster_grad_model as G
import raster_model as M
import ssim_loss_model as L
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

_hi = {}


def _reference(name, lam):
    """(a, b, the longdouble model, the recorded figures, the float64 model): computed once, shared, never written to"""
    if (name, lam) not in _hi:
        a, b = L.build(name)
        rec = json.load(open(os.path.join(GOLDEN, "ssim_loss_tolerance.json")))[name][str(lam)]
        _hi[name, lam] = (a, b, L.loss_grad(a, b, lam, np.longdouble), rec, L.loss_grad(a, b, lam))
    return _hi[name, lam]


def _call(a, b, lam, with_grad=True, ctx=None, **kw):
    from gaussiansplattingregistration_amd import loss
    ctx = ctx if ctx is not None else loss.context(0)
    parts, grad = ctx.l1_dssim(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), lam, with_grad=with_grad, **kw)
    return parts.cpu().numpy(), None if grad is None else grad.cpu().numpy()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("lam", L.LAMBDAS)
@pytest.mark.parametrize("name", L.SCENES)
def test_kernel_matches_the_higher_precision_model(name, lam):
    a, b, hi, rec, same = _reference(name, lam)
    parts, grad = _call(a, b, lam)
    assert grad.shape == a.shape and grad.dtype == np.float32 and np.isfinite(grad).all() and np.isfinite(parts).all()
    line = []
    for k, key in enumerate(("loss", "l1", "ssim")):
        err = float(abs(np.longdouble(parts[k]) - hi[key]))
        line.append(f"{key} {err:.2e} (allowed {4 * rec[key]:.2e})")
        assert err <= 4 * rec[key], (key, parts[k], hi[key], err, 4 * rec[key])
    err = np.abs(grad.astype(np.longdouble) - hi["grad"])
    allowed = 4 * rec["grad"] * hi["scale"] + 2.0 ** -24 * np.abs(hi["grad"])
    live = hi["scale"] > 0
    worst = float((err[live] / hi["scale"][live]).max()) if live.any() else 0.0
    store = np.abs(grad.astype(np.longdouble) - hi["grad"].astype(np.float32))          # what is left once the model is rounded to float32 as well
    bits = np.array_equal(_bits(grad), _bits(same["grad"].astype(np.float32))) and all(parts[k] == same[key] for k, key in enumerate(("loss", "l1", "ssim")))
    print(f"{name} lambda {lam}: " + ", ".join(line) + f"; gradient max |gpu - model| / scale {worst:.2e} (allowed {4 * rec['grad']:.2e} + the float32 store), "
          f"max |gpu - model| / allowed {float((err[allowed > 0] / allowed[allowed > 0]).max()) if (allowed > 0).any() else 0.0:.3f}, "
          f"max |gpu - float32(model)| / scale {float((store[live] / hi['scale'][live]).max()) if live.any() else 0.0:.2e}; the bits of the float64 model: {bits}")
    assert (err <= allowed).all(), (name, lam, float((err - allowed).max()))
    if lam == 0.0:          # the L1 term alone: bit for bit
        want = (np.sign(a.astype(np.float64) - b) / (3.0 * a.shape[0] * a.shape[1])).astype(np.float32)
        assert np.array_equal(_bits(grad), _bits(want))


def test_identical_images_have_no_gradient_beyond_rounding():
    a, b, hi, rec, _ = _reference("identical", 1.0)
    parts, grad = _call(a, b, 1.0)
    allowed = 4 * rec["grad"] * hi["scale"] + 2.0 ** -24 * np.abs(hi["grad"])
    print(f"identical, lambda 1: max |g| {np.abs(grad).max():.3e}, max |g| / allowed {float((np.abs(grad) / (allowed + 1e-300)).max()):.3f}")
    assert (np.abs(grad).astype(np.longdouble) <= allowed).all() and parts[1] == 0.0 and abs(parts[2] - 1.0) <= 1e-14


def test_same_bits_without_the_gradient_twice_and_over_garbage():
    for name in ("37x50", "17x33", "1x1"):
        a, b = L.build(name)
        parts, grad = _call(a, b, 0.2)
        alone, none = _call(a, b, 0.2, with_grad=False)
        assert none is None and np.array_equal(_bits(parts), _bits(alone))                  # grad_image = NULL: the same three values
        again, grad2 = _call(a, b, 0.2)
        assert np.array_equal(_bits(parts), _bits(again)) and np.array_equal(_bits(grad), _bits(grad2))
        junk_parts = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
        junk_grad = torch.full(a.shape, float("nan"), dtype=torch.float32, device="cuda")
        over, grad3 = _call(a, b, 0.2, parts_out=junk_parts, grad_out=junk_grad)             # overwritten, not accumulated into
        assert np.array_equal(_bits(parts), _bits(over)) and np.array_equal(_bits(grad), _bits(grad3))
        assert np.array_equal(_bits(junk_grad.cpu().numpy()), _bits(grad))


def test_a_grown_context_leaves_no_stale_partials():
    from gaussiansplattingregistration_amd import loss
    big, small = L.build("37x50"), L.build("3x7")
    with loss.LossContext(0) as fresh:
        want = _call(*small, 0.2, ctx=fresh)
    with loss.LossContext(0) as used:
        _call(*big, 0.2, ctx=used)
        got = _call(*small, 0.2, ctx=used)
    assert np.array_equal(_bits(want[0]), _bits(got[0])) and np.array_equal(_bits(want[1]), _bits(got[1]))


def test_argument_validation_messages():
    from gaussiansplattingregistration_amd import loss
    ctx = loss.context(0)
    a = torch.zeros(4, 5, 3, device="cuda")
    out = torch.zeros(3, dtype=torch.float64, device="cuda")
    Lb = ctx._L
    for args, word in (((ctx._h, None, a.data_ptr(), 4, 5, 0.2, out.data_ptr(), None, None), "NULL"),
                       ((ctx._h, a.data_ptr(), a.data_ptr(), 4, 5, 0.2, None, None, None), "NULL"),
                       ((ctx._h, a.data_ptr(), a.data_ptr(), 0, 5, 0.2, out.data_ptr(), None, None), "size"),
                       ((ctx._h, a.data_ptr(), a.data_ptr(), 4, -1, 0.2, out.data_ptr(), None, None), "size"),
                       ((ctx._h, a.data_ptr(), a.data_ptr(), 4, 5, 1.5, out.data_ptr(), None, None), "lambda"),
                       ((ctx._h, a.data_ptr(), a.data_ptr(), 4, 5, float("nan"), out.data_ptr(), None, None), "lambda"),
                       ((ctx._h, a.data_ptr(), a.data_ptr(), 16 * 65536, 1, 0.2, out.data_ptr(), None, None), "too tall")):
        assert Lb.gsr_loss_l1_dssim(*args) == -1
        msg = Lb.gsr_last_error().decode()
        assert msg.startswith("gsr_loss_l1_dssim: ") and word in msg, msg
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.l1_dssim(torch.zeros(4, 5, 3), a)
    with pytest.raises(ValueError, match="H, W, 3"):
        loss.l1_dssim(torch.zeros(3, 4, 5, device="cuda"), torch.zeros(3, 4, 5, device="cuda"))
    with pytest.raises(ValueError, match="lambda_dssim"):
        loss.l1_dssim(a, a, -0.1)


def test_autograd_front():
    from gaussiansplattingregistration_amd import loss
    a, b = L.build("17x33")
    parts, grad = _call(a, b, 0.2)
    image = torch.from_numpy(a).cuda().requires_grad_(True)
    target = torch.from_numpy(b).cuda()
    value, triple = loss.l1_dssim(image, target, 0.2, return_parts=True)
    assert value.shape == () and value.dtype == torch.float32 and value.item() == np.float32(parts[0])
    assert np.array_equal(_bits(triple.cpu().numpy()), _bits(parts)) and not triple.requires_grad          # the triple of the same launch
    (value * 2.5).backward()
    assert np.array_equal(_bits(image.grad.cpu().numpy()), _bits(grad * np.float32(2.5)))
    assert target.grad is None
    plain = loss.l1_dssim(torch.from_numpy(a).cuda(), target)                   # nothing asks for a gradient: the value alone, the same bits
    assert not plain.requires_grad and plain.item() == value.item()


def test_loss_behind_the_differentiable_rasteriser():
    """the ``exact`` scene of tests/raster_grad_model.py, its own render shifted by (2, 3) pixels as the target: backward() reaches dc, twice the same bits"""
    from gaussiansplattingregistration_amd import loss, raster
    m = G.scene_models(M.EXACT_SCENE)
    scene, cam = m["scene"], m["cam"]
    K = (scene["sh_degree"] + 1) ** 2 - 1
    up = lambda x: torch.from_numpy(np.array(x)).cuda()
    runs = []
    for _ in range(2):
        leaves = [up(scene["xyz"]), up(scene["cov6"]), up(scene["opacity"]), up(scene["color"]).requires_grad_(True), up(scene["sh"].reshape(-1, K, 3)) if K else None]
        image, _ = raster.render_differentiable(*leaves, scene["sh_degree"], cam["viewmat"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"],
                                                background=m["bg"])
        target = torch.roll(image.detach(), (2, 3), (0, 1)).contiguous()
        value = loss.l1_dssim(image, target, 0.2)
        value.backward()
        runs.append((value.item(), leaves[3].grad.cpu().numpy()))
    assert runs[0][1].shape == scene["color"].shape and np.isfinite(runs[0][1]).all() and np.abs(runs[0][1]).max() > 0
    assert runs[0][0] == runs[1][0] and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))


def _cameras(dicts):
    from gaussiansplattingregistration_amd.models.camera import Camera
    cams = []
    for k, cd in enumerate(dicts):
        V = cd["viewmat"].astype(np.float64)
        cams.append(Camera(V[:3, :3].T, V[:3, 3], cd["fx"], cd["fy"], f"view_{k}", cd["width"], cd["height"]))
    return cams


def test_finetuner_repairs_a_seam_with_l1_dssim():
    """the scene of tests/test_raster_grad_gpu.py::test_finetuner_repairs_a_seam (200 splats, 3 cameras of 64 x 48, the DC of half the splats
    darkened, 60 iterations on dc alone with lr_dc = 0.02) with ``loss="l1_dssim"``.  Measured figures: DESIGN.md 29."""
    from gaussiansplattingregistration_amd.finetune import FinetuneParams, ModelFinetuner
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.utils.rasterization_util import rasterize_image
    rng = np.random.default_rng(77)
    scene = M.make_scene(200, 71, 1)
    scene["cov6"] = M._cov6(rng, 200, 0.06, 0.2)
    cams = _cameras([M.make_camera(e, (0, 0, 0), 64, 48, 50.0) for e in ((0.3, -0.4, -3.2), (2.4, 0.5, -2.2), (-2.2, -0.8, -2.4))])
    mk = lambda color: GaussianModel("cuda:0").from_arrays(scene["xyz"], color, scene["opacity"], scene["cov6"], scene["sh"], 1)
    targets = [rasterize_image(mk(scene["color"]), c, 1, (0, 0, 0), "cuda:0")[0] for c in cams]
    bad = scene["color"].copy()
    bad[:100] = ((bad[:100] * M.C0 + 0.5) * 0.7 - 0.5) / M.C0
    runs = []
    for _ in range(2):
        model = mk(bad)
        log = ModelFinetuner(model, cams, targets, FinetuneParams(iterations=60, params=("dc",), lr_dc=0.02, loss="l1_dssim", lambda_dssim=0.2)).run()
        runs.append((model.get_colors.cpu().numpy(), log))
    log = runs[0][1]
    print(f"seam, l1_dssim: loss {log.losses[0]:.4e} -> {log.losses[-1]:.4e} (x {log.losses[-1] / log.losses[0]:.4f}); PSNR {np.round(log.psnr_before, 2)} -> "
          f"{np.round(log.psnr_after, 2)}")
    assert len(log.losses) == 60 and log.losses[-1] < log.losses[0]
    assert all(after > before for before, after in zip(log.psnr_before, log.psnr_after)) and len(log.psnr_after) == 3
    assert runs[0][1].losses == runs[1][1].losses and np.array_equal(_bits(runs[0][0]), _bits(runs[1][0]))


def _write_ply(path, n, seed):
    from gaussiansplattingregistration_amd.utils import ply_io
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    dc = (rng.uniform(0.2, 0.8, (n, 3)) - 0.5) / M.C0
    ply_io.save_gaussian_ply(path, rng.uniform(-1, 1, (n, 3)), dc, rng.normal(0, 0.02, (n, 9)), rng.normal(1.0, 1.0, n), rng.normal(-2.3, 0.3, (n, 3)), q)


def test_register_ply_takes_the_loss_flag(tmp_path, monkeypatch, capsys):
    """scripts/register_ply.py --finetune ... --finetune-loss l1_dssim on the tiny pair of tests/test_raster_grad_gpu.py's script test"""
    from PIL import Image
    from gaussiansplattingregistration_amd.models.camera import load_cameras
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.utils import ply_io
    from gaussiansplattingregistration_amd.utils.rasterization_util import rasterize_image
    _write_ply(tmp_path / "a.ply", 400, 1)
    _write_ply(tmp_path / "b.ply", 300, 1)
    entries = []
    for k, eye in enumerate(((0.0, 0.0, -4.0), (3.0, 1.0, -2.5), (-3.0, 0.5, -2.5), (0.5, -2.0, -3.5))):
        V = M.look_at(eye, (0, 0, 0)).astype(np.float64)
        entries.append({"id": k, "img_name": f"photo_{k}", "width": 72, "height": 48, "fx": 70.0, "fy": 72.0, "rotation": V[:3, :3].T.tolist(), "position": list(eye)})
    (tmp_path / "cameras.json").write_text(json.dumps(entries))
    images = tmp_path / "images"
    images.mkdir()
    cams = load_cameras(str(tmp_path / "cameras.json"))
    pc1, pc2 = (GaussianModel("cuda:0").from_ply(str(tmp_path / f)) for f in ("a.ply", "b.ply"))
    pc2._features_dc = pc2._features_dc + 0.3
    merged = GaussianModel.get_merged_gaussian_point_clouds(pc1, pc2, np.eye(4))
    for cam in cams:
        img = rasterize_image(merged, cam, 1, (0, 0, 0), "cuda:0")[0].clamp(0, 1).cpu().numpy()
        Image.fromarray(np.floor(img * 255.0 + 0.5).astype(np.uint8)).save(images / (cam.image_name + ".png"))
    spec = importlib.util.spec_from_file_location("register_ply", os.path.join(ROOT, "scripts", "register_ply.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "merged.ply"
    monkeypatch.setattr("sys.argv", ["register_ply.py", str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--voxel", "--type", "point", "--max-corr", "0.05", "--iters", "1",
                                     "--out", str(out), "--finetune", str(tmp_path / "cameras.json"), "--finetune-images", str(images), "--finetune-iters", "8",
                                     "--finetune-params", "dc,opacity", "--finetune-loss", "l1_dssim", "--finetune-lambda", "0.2"])
    mod.main()
    text = capsys.readouterr().out
    assert "fine-tuning (dc,opacity): 8 iterations over 4 cameras, l1_dssim loss (lambda 0.2) " in text
    assert len(ply_io.load_gaussian_arrays(str(out))["xyz"]) == 700
