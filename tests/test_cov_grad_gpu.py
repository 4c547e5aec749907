"""The covariance build kernels (csrc/covgrad.hip: gsr_cov_build, gsr_cov_build_backward), the autograd node over them and the fine-tuner
on ``("scaling", "rotation")`` on the MI355X.

Forward and backward against the float64 model of tests/cov_grad_model.py on every scene; the allowance per entry is 4 x the recorded
float32 cost of the model itself (tests/golden/cov_grad_tolerance.json, checked by tests/test_cov_grad_cpu.py) times the entry's scale, the
convention of DESIGN.md 14.3 and 26.3.  Everything else here is about bits: the loader's covariance, shapes around the 256-thread group,
subsets of outputs, overwriting, repeatability, host arrays against CUDA tensors, the zero-gradient and ``q = 0`` rows, the autograd node.

End to end: 200 anisotropic splats, three 64 x 48 cameras, targets rendered from the true scene; the scales of half the splats times 1.3
and their rotations turned by 10 degrees; 60 iterations on ``("scaling", "rotation")``.  Measured on the MI355X (pytest -s prints them;
nothing of this is asserted but "the last loss is below the first"): DESIGN.md 31.5.
"""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import cov_grad_model as M
import ply_model as P
import raster_model as RM
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _tolerance(name):
    return json.load(open(os.path.join(GOLDEN, "cov_grad_tolerance.json")))[name]


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _on(a):
    return torch.as_tensor(np.array(a)).to(DEV)                 # (a copy: the scenes' arrays are read-only)


def _run(name, host=False, wants=("scaling", "rotation"), rows=None):
    """-> dict(cov6, scaling, rotation) of the two entries on a scene (its first ``rows`` rows)"""
    from gaussiansplattingregistration_amd import covariance
    m = M.scene_models(name)
    s, q, g = (m[k][:rows] for k in ("scaling", "rotation", "grad_cov6"))
    if not host:
        s, q, g = _on(s), _on(q), _on(g)
    out = {"cov6": covariance.build_covariance(s, q)}
    out.update(covariance.build_covariance_backward(s, q, g, wants))
    for k, v in out.items():
        assert isinstance(v, np.ndarray) if host else (isinstance(v, torch.Tensor) and v.is_cuda), k
    return out


@pytest.mark.parametrize("host", (False, True), ids=("cuda_tensors", "host_arrays"))
@pytest.mark.parametrize("name", M.SCENES)
def test_forward_and_backward_match_the_float64_model(name, host):
    m, tol = M.scene_models(name), _tolerance(name)
    got = _run(name, host)
    for k in M.OUTPUTS:
        a = _np(got[k]).astype(np.float64)
        assert a.shape == m["ref"][k].shape and np.isfinite(a).all()
        err = np.abs(a - m["ref"][k]) / (m["scale"][k] + M.TINY)
        print(f"{name} {k}: max |kernel - float64 model| / scale {err.max():.3e} (recorded float32 cost {tol[k]:.3e}, allowed {4 * tol[k]:.3e})")
        assert (np.abs(a - m["ref"][k]) <= 4 * tol[k] * m["scale"][k]).all(), (name, k, float(err.max()))
    if name == "generic":                                                   # its last eight rows have a zero gradient
        assert not _bits(got["scaling"]).reshape(-1, 3)[-8:].any() and not _bits(got["rotation"]).reshape(-1, 4)[-8:].any()


def test_host_arrays_and_cuda_tensors_and_two_calls_give_the_same_bits():
    for name in M.SCENES:
        a, b, c = _run(name), _run(name), _run(name, host=True)
        for k in M.OUTPUTS:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (name, k)
            assert np.array_equal(_bits(a[k]), _bits(c[k])), (name, k)


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257))
def test_shapes_around_one_thread_group(n):
    """every row is computed alone: the first n rows of a scene give the bits they have in the whole scene, and n = 0 gives empty arrays"""
    full = _run("generic")
    for host in (False, True):
        part = _run("generic", host=host, rows=n)
        for k, width in (("cov6", 6), ("scaling", 3), ("rotation", 4)):
            assert tuple(part[k].shape) == (n, width)
            assert np.array_equal(_bits(part[k]), _bits(full[k][:n])), (n, host, k)


def _raw_backward(hip_lib, s, q, g, gs, gq):
    from gaussiansplattingregistration_amd import _lib
    n = int(s.shape[0])
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    torch.cuda.synchronize()
    st = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    _lib.check(hip_lib.gsr_cov_build_backward(p(s), p(q), p(g), n, p(gs), p(gq), 1, 0, st), "gsr_cov_build_backward")
    torch.cuda.synchronize()


def test_every_subset_of_outputs_gives_the_bits_of_the_full_call_and_outputs_are_overwritten(hip_lib):
    from gaussiansplattingregistration_amd import _lib
    full = _run("needles_discs")
    only_s = _run("needles_discs", wants=("scaling",))
    only_q = _run("needles_discs", wants=("rotation",))
    assert sorted(only_s) == ["cov6", "scaling"] and sorted(only_q) == ["cov6", "rotation"]
    assert np.array_equal(_bits(only_s["scaling"]), _bits(full["scaling"])) and np.array_equal(_bits(only_q["rotation"]), _bits(full["rotation"]))
    # straight through the C ABI into NaN-filled arrays: every entry is overwritten, and a skipped output is not touched
    m = M.scene_models("needles_discs")
    s, q, g = _on(m["scaling"]), _on(m["rotation"]), _on(m["grad_cov6"])
    n = len(s)
    nan = lambda w: torch.full((n, w), float("nan"), dtype=torch.float32, device=DEV)
    gs, gq, cov = nan(3), nan(4), nan(6)
    _raw_backward(hip_lib, s, q, g, gs, gq)
    assert np.array_equal(_bits(gs), _bits(full["scaling"])) and np.array_equal(_bits(gq), _bits(full["rotation"]))
    torch.cuda.synchronize()
    _lib.check(hip_lib.gsr_cov_build(C.c_void_p(s.data_ptr()), C.c_void_p(q.data_ptr()), n, C.c_void_p(cov.data_ptr()), 1, 0,
                                     C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "gsr_cov_build")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(cov), _bits(full["cov6"]))
    gs, gq = nan(3), nan(4)
    _raw_backward(hip_lib, s, q, g, gs, None)
    assert np.array_equal(_bits(gs), _bits(full["scaling"]))
    _raw_backward(hip_lib, s, q, g, None, gq)
    assert np.array_equal(_bits(gq), _bits(full["rotation"]))
    # n = 0 touches nothing, whatever the pointers
    assert hip_lib.gsr_cov_build_backward(None, None, None, 0, None, None, 1, 0, None) == 0
    assert hip_lib.gsr_cov_build(None, None, 0, None, 1, 0, None) == 0
    assert hip_lib.gsr_cov_build_backward(C.c_void_p(s.data_ptr()), C.c_void_p(q.data_ptr()), C.c_void_p(g.data_ptr()), n, None, None, 1, 0, None) == -1


@pytest.mark.parametrize("kind", ("canonical", "row4k3"))
def test_rebuilding_the_loaders_scale_and_rotation_gives_the_loaders_covariance_bits(hip_lib, kind):
    """gsr_cov_build of the scale / rot gsr_ply_unpack returned equals the cov6 it returned: one function (csrc/gsr_covbuild.h) behind both"""
    from gaussiansplattingregistration_amd import _lib, covariance
    n = 389
    spec = P.layout(kind, 0)
    _, v, cols, K = P.build(spec, n, seed=31)
    row_bytes, offsets, _ = P.offsets_of(spec)
    rows = torch.from_numpy(np.frombuffer(v.tobytes(), np.uint8).copy()).to(DEV)
    shape = {"xyz": (n, 3), "color": (n, 3), "opacity": (n,), "scale": (n, 3), "rot": (n, 4), "cov6": (n, 6)}
    out = {k: torch.full(s, 7.0, dtype=torch.float32, device=DEV) for k, s in shape.items()}
    p = lambda k: C.c_void_p(out[k].data_ptr())
    torch.cuda.synchronize()
    _lib.check(hip_lib.gsr_ply_unpack(C.c_void_p(rows.data_ptr()), n, row_bytes, (C.c_int32 * 15)(*offsets), 0, p("xyz"), p("color"), None, p("opacity"), p("scale"),
                                      p("rot"), p("cov6"), 0, C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "gsr_ply_unpack")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out["scale"]), P.bits(cols["scale"])) and np.array_equal(_bits(out["rot"]), P.bits(cols["rot"]))
    assert np.isfinite(out["cov6"].cpu().numpy()).all()
    assert np.array_equal(_bits(covariance.build_covariance(out["scale"], out["rot"])), _bits(out["cov6"]))
    assert np.array_equal(_bits(covariance.build_covariance(cols["scale"], cols["rot"])), _bits(out["cov6"]))          # host arrays too


def test_zero_gradient_rows_and_a_zero_quaternion():
    """rows with grad_cov6 = 0 and s = 100 (exp overflows float32) get exact +0.0; a row with q = 0 gets NaN and its neighbours keep their bits"""
    from gaussiansplattingregistration_amd import covariance
    m = M.scene_models("generic")
    s, q, g = m["scaling"][:64].copy(), m["rotation"][:64].copy(), m["grad_cov6"][:64].copy()
    want = covariance.build_covariance_backward(_on(s), _on(q), _on(g))
    want_cov = covariance.build_covariance(_on(s), _on(q))
    zero_rows, dead = [3, 17, 40], 29
    s[zero_rows] = 100.0
    g[zero_rows] = 0.0
    g[40, 2] = -0.0                                             # a negative zero is a zero
    q[dead] = 0.0
    assert g[dead].any()
    for host in (False, True):
        a = (s, q, g) if host else (_on(s), _on(q), _on(g))
        got = covariance.build_covariance_backward(*a)
        cov = covariance.build_covariance(a[0], a[1])
        keep = np.ones(64, bool)
        keep[zero_rows + [dead]] = False
        for k, w in (("scaling", 3), ("rotation", 4)):
            b, wb = _bits(got[k]).reshape(64, w), _bits(want[k]).reshape(64, w)
            assert not b[zero_rows].any(), (host, k)                                       # all bits clear: +0.0
            assert np.isnan(_np(got[k])[dead]).all(), (host, k)
            assert np.array_equal(b[keep], wb[keep]), (host, k)
        c = _np(cov)
        assert np.isnan(c[dead]).all() and np.array_equal(_bits(cov).reshape(64, 6)[keep], _bits(want_cov).reshape(64, 6)[keep])
        assert np.isinf(c[zero_rows]).any() or np.isnan(c[zero_rows]).any()                # the forward does overflow there: only the backward promises zeros


def test_autograd_node_is_the_two_kernels():
    """torch.autograd.gradcheck is of no use in float32: the node's gradients are build_covariance_backward's, bit for bit, and it asks
    only for the inputs that need one"""
    from gaussiansplattingregistration_amd import covariance
    m = M.scene_models("generic")
    s0, q0, g = _on(m["scaling"]), _on(m["rotation"]), _on(m["grad_cov6"])
    want = covariance.build_covariance_backward(s0, q0, g)
    want_cov = covariance.build_covariance(s0, q0)
    calls = []
    real = covariance.build_covariance_backward

    def spy(scaling, rotation, grad, wants=covariance.BACKWARD_OUTPUTS, device=None):
        calls.append(tuple(wants))
        return real(scaling, rotation, grad, wants, device)
    covariance.build_covariance_backward = spy
    try:
        for need_s, need_q in ((True, True), (True, False), (False, True)):
            s, q = s0.clone().requires_grad_(need_s), q0.clone().requires_grad_(need_q)
            cov = covariance.covariance_from_scale_rotation(s, q)
            assert np.array_equal(_bits(cov), _bits(want_cov))
            (cov * g).sum().backward()
            assert (s.grad is not None) == need_s and (q.grad is not None) == need_q
            if need_s:
                assert np.array_equal(_bits(s.grad), _bits(want["scaling"]))
            if need_q:
                assert np.array_equal(_bits(q.grad), _bits(want["rotation"]))
    finally:
        covariance.build_covariance_backward = real
    assert calls == [("scaling", "rotation"), ("scaling",), ("rotation",)]
    with torch.no_grad():
        assert not covariance.covariance_from_scale_rotation(s0, q0).requires_grad


# ---- the fine-tuner on scaling and rotation -------------------------------------------------------------------------------------------
def _cameras():
    from gaussiansplattingregistration_amd.models.camera import Camera
    cams = []
    for k, eye in enumerate(((0.3, -0.4, -3.2), (2.4, 0.5, -2.2), (-2.2, -0.8, -2.4))):
        cd = RM.make_camera(eye, (0, 0, 0), 64, 48, 50.0)
        V = cd["viewmat"].astype(np.float64)
        cams.append(Camera(V[:3, :3].T, V[:3, 3], cd["fx"], cd["fy"], f"view_{k}", cd["width"], cd["height"]))
    return cams


def _hamilton(a, b):
    w1, x1, y1, z1 = a.T
    w0, x0, y0, z0 = b.T
    return np.stack([w1 * w0 - x1 * x0 - y1 * y0 - z1 * z0, w1 * x0 + x1 * w0 + y1 * z0 - z1 * y0, w1 * y0 - x1 * z0 + y1 * w0 + z1 * x0,
                     w1 * z0 + x1 * y0 - y1 * x0 + z1 * w0], 1)


def _seam():
    """-> dict: the true scene (200 anisotropic splats as log-scales and quaternions), the damaged scales / rotations, cameras and targets"""
    from gaussiansplattingregistration_amd import covariance
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.utils.rasterization_util import rasterize_image
    rng = np.random.default_rng(77)
    n = 200
    scene = RM.make_scene(n, 71, 1)
    s = np.log(rng.uniform(0.04, 0.2, (n, 3))).astype(np.float32)
    q = rng.normal(size=(n, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.7, 1.4, (n, 1))).astype(np.float32)          # raw, as a .ply stores them
    s_bad, q_bad = s.copy(), q.copy()
    s_bad[:100] += np.float32(np.log(1.3))
    axis = rng.normal(size=(100, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    half = np.deg2rad(10.0) / 2
    turn = np.concatenate([np.full((100, 1), np.cos(half)), np.sin(half) * axis], 1)
    q_bad[:100] = _hamilton(turn, q[:100].astype(np.float64)).astype(np.float32)

    def model(scaling, rotation):
        g = GaussianModel(DEV).from_arrays(scene["xyz"], scene["color"], scene["opacity"], covariance.build_covariance(_on(scaling), _on(rotation)), scene["sh"], 1)
        g._scaling, g._rotation = _on(scaling), _on(rotation)
        return g
    cams = _cameras()
    truth = model(s, q)
    targets = [rasterize_image(truth, c, 1, (0, 0, 0), DEV)[0] for c in cams]
    return dict(scene=scene, s=s, q=q, s_bad=s_bad, q_bad=q_bad, model=model, cams=cams, targets=targets, truth=truth)


@pytest.fixture(scope="module")
def seam():
    return _seam()


def test_finetuner_repairs_the_shape_of_the_splats(seam, tmp_path):
    from gaussiansplattingregistration_amd import covariance
    from gaussiansplattingregistration_amd.finetune import FinetuneParams, ModelFinetuner
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    params = FinetuneParams(iterations=60, params=("scaling", "rotation"))
    runs = []
    for _ in range(2):
        model = seam["model"](seam["s_bad"], seam["q_bad"])
        log = ModelFinetuner(model, seam["cams"], seam["targets"], params).run()
        runs.append((model, log))
    model, log = runs[0]
    ratio = log.losses[-1] / log.losses[0]
    ds = lambda sc: float(np.abs(_np(sc) - seam["s"])[:100].mean())
    print(f"shape seam: loss {log.losses[0]:.4e} -> {log.losses[-1]:.4e} (x {ratio:.4f}); mean of the last three / first three "
          f"{np.mean(log.losses[-3:]) / np.mean(log.losses[:3]):.4f}; PSNR {np.round(log.psnr_before, 2)} -> {np.round(log.psnr_after, 2)}; "
          f"mean |s - truth| of the damaged half {ds(seam['s_bad']):.4f} -> {ds(model._scaling):.4f}")
    assert log.geometry_source == "stored" and len(log.losses) == 60 and log.iterations == 60
    assert log.losses[-1] < log.losses[0]
    # two runs: the same bits
    for name in ("_scaling", "_rotation", "_covariance"):
        assert np.array_equal(_bits(getattr(runs[0][0], name)), _bits(getattr(runs[1][0], name))), name
    assert runs[0][1].losses == runs[1][1].losses
    # the tensors moved, the others did not, and the quaternion was not renormalised
    assert not np.array_equal(_bits(model._scaling), _bits(seam["s_bad"])) and not np.array_equal(_bits(model._rotation), _bits(seam["q_bad"]))
    assert np.array_equal(_bits(model._xyz), _bits(seam["scene"]["xyz"])) and np.array_equal(_bits(model._features_dc), _bits(seam["scene"]["color"]))
    assert tuple(model._scaling.shape) == (200, 3) and tuple(model._rotation.shape) == (200, 4) and tuple(model._covariance.shape) == (200, 6)
    assert model._scaling.is_cuda and model._covariance.is_cuda and not model._scaling.requires_grad
    # a consistent triple, and the file stores it
    assert np.array_equal(_bits(model._covariance), _bits(covariance.build_covariance(model._scaling, model._rotation)))
    path = str(tmp_path / "tuned.ply")
    model.save_ply(path)
    back = GaussianModel(DEV).from_ply(path)
    assert np.array_equal(_bits(back.get_covariance()), _bits(model.get_covariance()))
    assert np.array_equal(_bits(back._scaling), _bits(model._scaling)) and np.array_equal(_bits(back._rotation), _bits(model._rotation))
    # a model from a file starts from what the file stores
    again = ModelFinetuner(back, seam["cams"], seam["targets"], FinetuneParams(iterations=3, params=("scaling",))).run()
    assert again.geometry_source == "stored" and len(again.losses) == 3
    assert np.array_equal(_bits(back._rotation), _bits(model._rotation))                     # not tuned: a constant input, written back as it was
    assert np.array_equal(_bits(back._covariance), _bits(covariance.build_covariance(back._scaling, back._rotation)))
    # cancelled: the model is left alone
    fresh = seam["model"](seam["s_bad"], seam["q_bad"])
    before = {k: _bits(getattr(fresh, k)) for k in ("_scaling", "_rotation", "_covariance")}
    worker = ModelFinetuner(fresh, seam["cams"], seam["targets"], params)
    worker.cancel()
    assert worker.run() is None and all(np.array_equal(_bits(getattr(fresh, k)), v) for k, v in before.items())


def test_a_model_without_stored_factors_is_decomposed_and_tunes(seam):
    from gaussiansplattingregistration_amd import covariance
    from gaussiansplattingregistration_amd.finetune import FinetuneParams, ModelFinetuner
    from gaussiansplattingregistration_amd.models.gaussian_mixture_level import GaussianMixtureModel
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    bad = seam["model"](seam["s_bad"], seam["q_bad"])
    level = GaussianMixtureModel(bad._xyz, bad.get_colors, bad._opacity, bad._covariance, bad._features_rest)
    model = GaussianModel(DEV).from_mixture(level, 1, decompose=False)
    assert model._scaling.numel() == 0
    start = _bits(model._covariance).copy()
    log = ModelFinetuner(model, seam["cams"], seam["targets"], FinetuneParams(iterations=30, params=("scaling", "rotation"))).run()
    print(f"decomposed start: loss {log.losses[0]:.4e} -> {log.losses[-1]:.4e}; PSNR {np.round(log.psnr_before, 2)} -> {np.round(log.psnr_after, 2)}")
    assert log.geometry_source == "decomposed" and len(log.losses) == 30 and log.losses[-1] < log.losses[0]
    assert tuple(model._scaling.shape) == (200, 3) and tuple(model._rotation.shape) == (200, 4)
    assert not np.array_equal(_bits(model._covariance), start)
    assert np.array_equal(_bits(model._covariance), _bits(covariance.build_covariance(model._scaling, model._rotation)))
    # the reference's decomposition stores the eigenvalue itself as "scaling": wrong by O(1), so the tuner does not start from it
    ref = GaussianModel(DEV).from_mixture(level, 1, decompose=True)
    log = ModelFinetuner(ref, seam["cams"], seam["targets"], FinetuneParams(iterations=2, params=("rotation",))).run()
    assert log.geometry_source == "decomposed"
    # an exact decomposition is a consistent triple: kept
    exact = GaussianModel(DEV).from_mixture(level, 1, decompose="exact")
    log = ModelFinetuner(exact, seam["cams"], seam["targets"], FinetuneParams(iterations=2, params=("rotation",))).run()
    assert log.geometry_source == "stored"


def test_default_params_give_the_bits_of_the_appearance_only_tuner(seam):
    """the tuner as it was before scaling / rotation, written out in plain torch against the same renders: Adam over (dc, sh_rest, opacity)
    with the published rates, the model's covariance a constant"""
    from gaussiansplattingregistration_amd import raster
    from gaussiansplattingregistration_amd.finetune import FinetuneParams, ModelFinetuner
    from gaussiansplattingregistration_amd.utils.rasterization_util import _camera_args
    model = seam["model"](seam["s_bad"], seam["q_bad"])
    model._features_dc = model._features_dc * 0.8
    twin = model.clone_gaussian()
    p = FinetuneParams(iterations=12)
    assert p.params == ("dc", "sh_rest", "opacity")
    log = ModelFinetuner(model, seam["cams"], seam["targets"], p).run()
    assert log.geometry_source is None
    n = len(twin)
    dc = twin._features_dc.detach().reshape(n, 3).clone().contiguous().requires_grad_(True)
    sh = twin._features_rest.detach().reshape(n, 3, 3).clone().contiguous().requires_grad_(True)
    op = twin._opacity.detach().reshape(n).clone().contiguous().requires_grad_(True)
    xyz, cov6 = twin.get_xyz.detach().reshape(n, 3), twin.get_covariance().detach().reshape(n, 6).contiguous()
    opt = torch.optim.Adam([{"params": [dc], "lr": 2.5e-3}, {"params": [sh], "lr": 1.25e-4}, {"params": [op], "lr": 0.05}], eps=1e-15)
    losses = []
    for it in range(12):
        cam, tgt = seam["cams"][it % 3], seam["targets"][it % 3]
        opt.zero_grad(set_to_none=True)
        diff = raster.render_differentiable(xyz, cov6, op, dc, sh, 1, *_camera_args(cam), background=(0.0, 0.0, 0.0), radius_clip=3.0, device=0)[0] - tgt
        loss = (diff * diff).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses == log.losses
    assert np.array_equal(_bits(model._features_dc), _bits(dc)) and np.array_equal(_bits(model._features_rest), _bits(sh)) and np.array_equal(_bits(model._opacity), _bits(op))
    for name in ("_xyz", "_covariance", "_scaling", "_rotation"):                             # untouched
        assert np.array_equal(_bits(getattr(model, name)), _bits(getattr(twin, name))), name


def test_register_ply_tunes_and_saves_scaling_and_rotation(tmp_path, monkeypatch, capsys):
    """scripts/register_ply.py ... --finetune-params dc,opacity,scaling,rotation writes a .ply whose reloaded covariances are the tuned ones:
    not those of the plain merge, and consistent with the stored scales and quaternions"""
    from PIL import Image
    from gaussiansplattingregistration_amd import covariance
    from gaussiansplattingregistration_amd.models.camera import load_cameras
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.utils import ply_io
    from gaussiansplattingregistration_amd.utils.rasterization_util import rasterize_image

    def write(path, n, seed):
        rng = np.random.default_rng(seed)
        q = rng.normal(size=(n, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        dc = (rng.uniform(0.2, 0.8, (n, 3)) - 0.5) / RM.C0
        ply_io.save_gaussian_ply(path, rng.uniform(-1, 1, (n, 3)), dc, rng.normal(0, 0.02, (n, 9)), rng.normal(1.0, 1.0, n), rng.normal(-2.3, 0.3, (n, 3)), q)
    write(tmp_path / "a.ply", 300, 1)
    write(tmp_path / "b.ply", 200, 1)          # the same generator: its splats sit on the first 200 of a.ply, so the registration has pairs
    entries = []
    for k, eye in enumerate(((0.0, 0.0, -4.0), (3.0, 1.0, -2.5), (-3.0, 0.5, -2.5))):
        V = RM.look_at(eye, (0, 0, 0)).astype(np.float64)
        entries.append({"id": k, "img_name": f"photo_{k}", "width": 72, "height": 48, "fx": 70.0, "fy": 72.0, "rotation": V[:3, :3].T.tolist(), "position": list(eye)})
    (tmp_path / "cameras.json").write_text(json.dumps(entries))
    images = tmp_path / "images"
    images.mkdir()
    cams = load_cameras(str(tmp_path / "cameras.json"))
    pc1, pc2 = (GaussianModel(DEV).from_ply(str(tmp_path / f)) for f in ("a.ply", "b.ply"))
    plain = GaussianModel.get_merged_gaussian_point_clouds(pc1, pc2, np.eye(4))
    shrunk = plain.clone_gaussian()
    shrunk._scaling = shrunk._scaling - 0.25                          # the photographs show thinner splats than the files hold
    shrunk._covariance = covariance.build_covariance(shrunk._scaling, shrunk._rotation)
    for cam in cams:
        img = rasterize_image(shrunk, cam, 1, (0, 0, 0), DEV)[0].clamp(0, 1).cpu().numpy()
        Image.fromarray(np.floor(img * 255.0 + 0.5).astype(np.uint8)).save(images / (cam.image_name + ".png"))
    spec = importlib.util.spec_from_file_location("register_ply", os.path.join(ROOT, "scripts", "register_ply.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "merged.ply"
    monkeypatch.setattr("sys.argv", ["register_ply.py", str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--voxel", "--type", "point", "--max-corr", "0.05", "--iters", "1",
                                     "--out", str(out), "--finetune", str(tmp_path / "cameras.json"), "--finetune-images", str(images), "--finetune-iters", "9",
                                     "--finetune-params", "dc,opacity,scaling,rotation"])
    mod.main()
    text = capsys.readouterr().out
    assert "fine-tuning (dc,opacity,scaling,rotation): 9 iterations over 3 cameras" in text and "from the stored factors" in text
    back = GaussianModel(DEV).from_ply(str(out))
    assert len(back) == 500
    assert np.array_equal(_bits(back._covariance), _bits(covariance.build_covariance(back._scaling, back._rotation)))
    assert not np.array_equal(_bits(back._scaling), _bits(plain._scaling)) and not np.array_equal(_bits(back._rotation), _bits(plain._rotation))
    moved = float((back._scaling - plain._scaling).mean())
    print(f"register_ply: mean change of the log-scales {moved:+.4f} (the photographs were rendered 0.25 thinner)")
    assert moved < 0
