"""The backward pass of the HIP rasteriser (gsr_raster_backward) against the float64 analytic NumPy model
(tests/raster_grad_model.py), its autograd front, the fine-tuner and the two script flags.

Tolerance of the parity tests: tests/golden/raster_grad_tolerance.json records, per scene and per output array, what float32 costs the
model itself, ``max |g32 - g64| / (scale + tiny)`` with ``scale`` the sum of the absolute values of the terms an entry is made of
(tests/test_raster_grad_cpu.py checks the file against the model); the kernel gets 4 x that, the convention of tests/test_raster_gpu.py.
The upstream gradients are zeroed on the forward's fragile pixels (at most 1 % of an image), so a legitimately different float32
decision cannot reach any gradient; the decisions only the backward pass looks at sit at least 1e-4 from their switch on every scene
used here (tests/test_raster_grad_cpu.py).  Measured on an MI355X: profiles/raster_grad_pytest_gpu.log.
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import raster_grad_model as G
import raster_model as M
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

OUT = G.OUTPUTS


def _tolerance(name):
    return {k: 4.0 * v for k, v in json.load(open(os.path.join(GOLDEN, "raster_grad_tolerance.json")))[name].items()}


def _args(scene, cam, host=False):
    conv = (lambda a: np.ascontiguousarray(a)) if host else (lambda a: torch.from_numpy(np.array(a)).cuda())
    K = (scene["sh_degree"] + 1) ** 2 - 1
    return (conv(scene["xyz"]), conv(scene["cov6"]), conv(scene["opacity"]), conv(scene["color"]), conv(scene["sh"].reshape(-1, K, 3)) if K else None,
            scene["sh_degree"], cam["viewmat"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["width"], cam["height"])


def _backward(m, host=False, G_C="both", G_A="both", wants=OUT, with_stats=False):
    from gaussiansplattingregistration_amd import raster
    conv = (lambda a: np.array(a)) if host else (lambda a: torch.from_numpy(np.array(a)).cuda())
    gc = conv(m["G_C"]) if G_C == "both" else G_C
    ga = conv(m["G_A"]) if G_A == "both" else G_A
    out = raster.context(0).render_backward(*_args(m["scene"], m["cam"], host), grad_image=gc, grad_alpha=ga, background=m["bg"], radius_clip=3.0, wants=wants,
                                            with_stats=with_stats)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(name, got, want, tol):
    worst = {}
    for k in got:
        if k == "stats":
            continue
        assert got[k].shape == want[k].shape and np.isfinite(got[k]).all(), k
        err = float((np.abs(got[k].astype(np.float64) - want[k]) / (want["scale"][k] + G.TINY)).max())
        worst[k] = err
    print(f"{name}: max |gpu - float64 model| / scale " + ", ".join(f"{k} {v:.3e} (allowed {tol[k]:.3e})" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= tol[k], (k, v, tol[k])


CASES = [(n, False) for n in G.GPU_SCENES] + [(M.EXACT_SCENE, True), (G.GRAD_EDGES, True)]


@pytest.mark.parametrize("name,host", CASES, ids=[f"{n}-{'host_arrays' if h else 'cuda_tensors'}" for n, h in CASES])
def test_backward_matches_the_float64_model(name, host):
    m = G.scene_models(name)
    assert m["ref"]["fragile"].mean() <= 0.01
    got = _backward(m, host=host, with_stats=True)
    _check(name, got, m["both"], _tolerance(name))
    ok = m["both"]["ok"]
    for k in OUT:                                                   # culled splats: exact zeros (+0.0) in every output
        assert not _bits(got[k][~ok]).any(), k
    if not m["ref"]["fragile"].any() or name == G.GRAD_EDGES:       # no splat-level decision is fragile there: the counts are the model's
        assert got["stats"].tolist() == [m["ref"]["visible"], m["ref"]["intersections"], m["ref"]["nonempty_tiles"]]


def test_grad_edges_culls_and_counts():
    m = G.scene_models(G.GRAD_EDGES)
    got = _backward(m, with_stats=True)
    assert got["stats"].tolist() == [m["ref"]["visible"], m["ref"]["intersections"], m["ref"]["nonempty_tiles"]]
    for r in G.ROW_BEHIND:
        for k in OUT:
            assert not _bits(got[k][r]).any()
    assert np.abs(got["dc"][G.ROW_CLAMPED_COLOUR, 0]) == 0 and np.abs(got["dc"][G.ROW_CLAMPED_COLOUR, 1]) > 0


def test_two_calls_are_bit_identical_and_outputs_are_overwritten():
    from gaussiansplattingregistration_amd import raster
    m = G.scene_models("giants_tiny")
    a, b = _backward(m), _backward(m)
    for k in OUT:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    # the library overwrites: NaN-filled outputs through the C entry itself
    ctx = raster.context(0)
    dev, n, K, (x, c, o, d, s), V, bg = ctx._inputs(*_args(m["scene"], m["cam"])[:5], m["cam"]["viewmat"], m["bg"])
    outs = [torch.full(shape, float("nan"), device=dev) for shape in ((n, 3), (n, 6), (n,), (n, 3), (n, 3 * K))]
    gc, ga = torch.from_numpy(m["G_C"].copy()).cuda(), torch.from_numpy(m["G_A"].copy()).cuda()
    cam = m["cam"]
    import ctypes as C
    rc = ctx._L.gsr_raster_backward(ctx._h, n, K, m["scene"]["sh_degree"], x.data_ptr(), c.data_ptr(), o.data_ptr(), d.data_ptr(), s.data_ptr(), V, cam["fx"], cam["fy"],
                                    cam["cx"], cam["cy"], cam["width"], cam["height"], bg, 3.0, gc.data_ptr(), ga.data_ptr(), *[t.data_ptr() for t in outs], None,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for k, t in zip(OUT, outs):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a[k])), k


def test_every_subset_of_outputs_gives_the_same_bits():
    m = G.scene_models(G.GRAD_EDGES)
    full = _backward(m)
    for mask in range(1, 31):
        wants = tuple(k for i, k in enumerate(OUT) if mask >> i & 1)
        got = _backward(m, wants=wants)
        assert set(got) == set(wants)
        for k in wants:
            assert np.array_equal(_bits(got[k]), _bits(full[k])), (wants, k)


def test_grad_image_alone_grad_alpha_alone_and_both():
    """each alone against the model; the colour records (dc, sh_rest) do not see G_A at all, so with both they are the bits of G_C alone.  The
    other arrays mix the two in one float32 expression per pixel: both = the sum only up to rounding, held to the model's scale."""
    m = G.scene_models(G.GRAD_EDGES)
    tol = _tolerance(G.GRAD_EDGES)
    only_c = G.backward(m["scene"], m["cam"], m["G_C"], None, m["bg"])
    only_a = G.backward(m["scene"], m["cam"], None, m["G_A"], m["bg"])
    got_c, got_a, both = _backward(m, G_A=None), _backward(m, G_C=None), _backward(m)
    _check("grad_image alone", got_c, only_c, tol)
    _check("grad_alpha alone", got_a, only_a, tol)
    for k in ("dc", "sh_rest"):
        assert np.array_equal(_bits(both[k]), _bits(got_c[k])) and (got_a[k] == 0).all()
    for k in ("xyz", "cov6", "raw_opacity"):
        scale = only_c["scale"][k] + only_a["scale"][k] + G.TINY
        assert (np.abs(both[k].astype(np.float64) - got_c[k] - got_a[k]) / scale).max() <= 3 * tol[k]


def test_empty_model_and_a_scene_with_no_visible_splat():
    from gaussiansplattingregistration_amd import raster
    cam = M.make_camera(**G.EDGE_CAM)
    H, W = cam["height"], cam["width"]
    g = torch.ones((H, W, 3), device="cuda")
    cargs = (cam["viewmat"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], W, H)
    e = lambda *s: torch.zeros(s, device="cuda")
    out = raster.context(0).render_backward(e(0, 3), e(0, 6), e(0), e(0, 3), e(0, 3, 3), 1, *cargs, grad_image=g)
    assert [tuple(out[k].shape) for k in OUT] == [(0, 3), (0, 6), (0,), (0, 3), (0, 9)]
    scene = G.make_grad_edges()
    rows = list(G.ROW_BEHIND)
    out = raster.context(0).render_backward(*(torch.from_numpy(scene[k][rows]).cuda() for k in ("xyz", "cov6", "opacity", "color")),
                                            torch.from_numpy(scene["sh"][rows]).cuda(), 1, *cargs, grad_image=g, grad_alpha=torch.ones((H, W), device="cuda"),
                                            with_stats=True)
    assert out["stats"].tolist() == [0, 0, 0]
    for k in OUT:
        assert not _bits(out[k].cpu().numpy()).any()


def test_argument_validation_messages():
    import ctypes as C
    from gaussiansplattingregistration_amd import raster
    m = G.scene_models(M.EXACT_SCENE)
    ctx = raster.context(0)
    args = _args(m["scene"], m["cam"])
    g = torch.from_numpy(m["G_C"].copy()).cuda()
    with pytest.raises(ValueError, match="both None"):
        ctx.render_backward(*args)
    with pytest.raises(ValueError, match="unknown output 'depth'"):
        ctx.render_backward(*args, grad_image=g, wants=("depth",))
    with pytest.raises(ValueError, match="no output requested"):
        ctx.render_backward(*args, grad_image=g, wants=())
    with pytest.raises(ValueError, match="expected"):
        ctx.render_backward(*args, grad_image=g[:-1])
    # the library's own checks, under the entry's name
    dev, n, K, (x, c, o, d, s), V, bg = ctx._inputs(*args[:5], m["cam"]["viewmat"], m["bg"])
    cam = m["cam"]
    out = torch.empty((n, 3), device=dev)

    def call(n_=n, deg=1, gi=g.data_ptr(), ga=None, ox=out.data_ptr(), width=cam["width"], bgp=bg):
        rc = ctx._L.gsr_raster_backward(ctx._h, n_, K, deg, x.data_ptr(), c.data_ptr(), o.data_ptr(), d.data_ptr(), s.data_ptr(), V, cam["fx"], cam["fy"], cam["cx"],
                                        cam["cy"], width, cam["height"], bgp, 3.0, gi, ga, ox, None, None, None, None, None, C.c_void_p(0))
        return rc, ctx._L.gsr_last_error().decode()
    assert call()[0] == 0
    for kwargs, text in ((dict(gi=None), "gsr_raster_backward: grad_image and grad_alpha are both NULL"), (dict(ox=None), "gsr_raster_backward: no output requested"),
                         (dict(n_=-1), "gsr_raster_backward: n = -1 out of range"), (dict(deg=2), "gsr_raster_backward: sh_degree 2 needs 8 rest coefficients, K = 3"),
                         (dict(width=0), "gsr_raster_backward: bad image size"), (dict(bgp=None), "gsr_raster_backward: NULL argument")):
        rc, msg = call(**kwargs)
        assert rc == -1 and text in msg, (kwargs, rc, msg)
    torch.cuda.synchronize()
    t = ctx.backward_timing()
    assert set(t) == {"preprocess", "sort", "blend_backward", "splat_backward"} and all(v >= 0 for v in t.values())


def test_render_differentiable_is_render_aux_and_render_backward():
    from gaussiansplattingregistration_amd import raster
    m = G.scene_models("scaled")
    args = _args(m["scene"], m["cam"])
    leaves = [a.clone().requires_grad_(True) for a in args[:5]]
    image, alpha = raster.render_differentiable(*leaves, *args[5:], background=m["bg"])
    ref = raster.context(0).render_aux(*args, background=m["bg"], outputs=("image", "alpha"))
    assert torch.equal(image, ref["image"]) and torch.equal(alpha, ref["alpha"])
    gc, ga = torch.from_numpy(m["G_C"].copy()).cuda(), torch.from_numpy(m["G_A"].copy()).cuda()
    ((image * gc).sum() + (alpha * ga).sum()).backward()
    direct = _backward(m)
    for leaf, k in zip(leaves, OUT):
        assert leaf.grad.shape == leaf.shape
        assert np.array_equal(_bits(leaf.grad.reshape(direct[k].shape).cpu().numpy()), _bits(direct[k])), k
    # only what needs a gradient is asked for
    only = [a.clone() for a in args[:5]]
    only[3].requires_grad_(True)
    image, _ = raster.render_differentiable(*only, *args[5:], background=m["bg"])
    (image * gc).sum().backward()
    assert np.array_equal(_bits(only[3].grad.cpu().numpy()), _bits(_backward(m, G_A=None)["dc"]))


def test_pose_gradients_through_torch_composition():
    """xyz' = R xyz + t and Sigma' = R Sigma R^T composed in torch in front of the rasteriser, R and t requiring grad, against the float64
    model's per-splat gradients (at the very float32 xyz', cov6' torch produced) contracted with the same Jacobian in float64 NumPy.
    Allowed: 4 x the model's float32 cost of xyz and cov6 times the contraction of the scales with |Jacobian|, plus n float32 roundings
    (2^-24 each) of the contraction's own absolute sum, which torch adds up in float32."""
    from gaussiansplattingregistration_amd import raster, synth
    name = M.EXACT_SCENE
    m = G.scene_models(name)
    scene, cam = m["scene"], m["cam"]
    T = synth.rigid_transform(3.0, (0.3, 1.0, -0.2), (0.02, -0.03, 0.04))
    R = torch.tensor(T[:3, :3], dtype=torch.float32, device="cuda", requires_grad=True)
    t = torch.tensor(T[:3, 3], dtype=torch.float32, device="cuda", requires_grad=True)
    args = _args(scene, cam)
    xyz, c6 = args[0], args[1]
    S = torch.stack([c6[:, [0, 1, 2]], c6[:, [1, 3, 4]], c6[:, [2, 4, 5]]], dim=1)
    xyz2 = xyz @ R.T + t
    S2 = R @ S @ R.T
    cov2 = torch.stack([S2[:, 0, 0], S2[:, 0, 1], S2[:, 0, 2], S2[:, 1, 1], S2[:, 1, 2], S2[:, 2, 2]], dim=1)
    image, alpha = raster.render_differentiable(xyz2, cov2, *args[2:], background=m["bg"])
    moved = dict(scene, xyz=xyz2.detach().cpu().numpy(), cov6=cov2.detach().cpu().numpy())
    ref = M.render(moved, cam, m["bg"])
    H, W = ref["fragile"].shape
    gc, ga = G.upstream("pose", H, W)
    gc[ref["fragile"]] = 0
    ga[ref["fragile"]] = 0
    assert ref["fragile"].mean() <= 0.01
    ((image * torch.from_numpy(gc).cuda()).sum() + (alpha * torch.from_numpy(ga).cuda()).sum()).backward()
    want = G.backward(moved, cam, gc, ga, m["bg"])
    x64, S64, R64 = scene["xyz"].astype(np.float64), S.cpu().numpy().astype(np.float64), R.detach().cpu().numpy().astype(np.float64)
    gx, sx = want["xyz"], want["scale"]["xyz"]
    full = lambda g6: np.stack([np.stack([g6[:, 0], g6[:, 1] / 2, g6[:, 2] / 2], 1), np.stack([g6[:, 1] / 2, g6[:, 3], g6[:, 4] / 2], 1),
                                np.stack([g6[:, 2] / 2, g6[:, 4] / 2, g6[:, 5]], 1)], 1)
    GS, GSs = full(want["cov6"]), full(want["scale"]["cov6"])
    want_t, want_R = gx.sum(0), gx.T @ x64 + 2.0 * np.einsum("nij,jk,nkl->il", GS, R64, S64)
    cost = json.load(open(os.path.join(GOLDEN, "raster_grad_tolerance.json")))[name]
    n = len(x64)
    eps = 2.0 ** -24
    tol_t = 4 * cost["xyz"] * sx.sum(0) + n * eps * np.abs(gx).sum(0)
    abs_R = np.abs(gx).T @ np.abs(x64) + 2.0 * np.einsum("nij,jk,nkl->il", np.abs(GS), np.abs(R64), np.abs(S64))
    tol_R = 4 * cost["xyz"] * (sx.T @ np.abs(x64)) + 4 * cost["cov6"] * 2.0 * np.einsum("nij,jk,nkl->il", GSs, np.abs(R64), np.abs(S64)) + n * eps * abs_R
    err_t, err_R = np.abs(t.grad.cpu().numpy() - want_t), np.abs(R.grad.cpu().numpy() - want_R)
    print(f"pose: |dt error| / allowed {np.max(err_t / tol_t):.3f}, |dR error| / allowed {np.max(err_R / tol_R):.3f}; dt {want_t}, dR row 0 {want_R[0]}")
    assert (err_t <= tol_t).all() and (err_R <= tol_R).all()


def _cameras(dicts):
    from gaussiansplattingregistration_amd.models.camera import Camera
    cams = []
    for k, cd in enumerate(dicts):
        V = cd["viewmat"].astype(np.float64)
        cams.append(Camera(V[:3, :3].T, V[:3, 3], cd["fx"], cd["fy"], f"view_{k}", cd["width"], cd["height"]))
    return cams


def test_finetuner_repairs_a_seam():
    """200 splats, 3 cameras of 64 x 48, targets = renders of the true scene; the DC of half the splats darkened (colour x 0.7); 60
    iterations on dc alone with lr_dc = 0.02.  Measured ratios: DESIGN.md 26."""
    from gaussiansplattingregistration_amd.finetune import FinetuneParams, ModelFinetuner
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.utils.rasterization_util import rasterize_image
    rng = np.random.default_rng(77)
    scene = M.make_scene(200, 71, 1)
    scene["cov6"] = M._cov6(rng, 200, 0.06, 0.2)
    cams = _cameras([M.make_camera(e, (0, 0, 0), 64, 48, 50.0) for e in ((0.3, -0.4, -3.2), (2.4, 0.5, -2.2), (-2.2, -0.8, -2.4))])
    mk = lambda color: GaussianModel("cuda:0").from_arrays(scene["xyz"], color, scene["opacity"], scene["cov6"], scene["sh"], 1)
    truth = mk(scene["color"])
    targets = [rasterize_image(truth, c, 1, (0, 0, 0), "cuda:0")[0] for c in cams]
    contribution = truth.max_contribution(cams, radius_clip=3.0).cpu().numpy() > 0
    bad = scene["color"].copy()
    bad[:100] = ((bad[:100] * M.C0 + 0.5) * 0.7 - 0.5) / M.C0
    runs = []
    for _ in range(2):
        model = mk(bad)
        log = ModelFinetuner(model, cams, targets, FinetuneParams(iterations=60, params=("dc",), lr_dc=0.02)).run()
        runs.append((model.get_colors.cpu().numpy(), log))
    dc, log = runs[0]
    before = np.abs(bad - scene["color"])[contribution].mean()
    after = np.abs(dc - scene["color"])[contribution].mean()
    print(f"seam: visible {contribution.sum()} of 200; loss {log.losses[0]:.4e} -> {log.losses[-1]:.4e} (x {log.losses[-1] / log.losses[0]:.4f}); "
          f"mean |dc - truth| {before:.4f} -> {after:.4f} (x {after / before:.4f}); PSNR {np.round(log.psnr_before, 2)} -> {np.round(log.psnr_after, 2)}")
    assert len(log.losses) == 60 and all(v < log.losses[0] for v in log.losses[-10:])
    assert after < before
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and runs[0][1].losses == runs[1][1].losses
    # cancel is polled between iterations: the model is left alone
    model = mk(bad)
    worker = ModelFinetuner(model, cams, targets, FinetuneParams(iterations=5, params=("dc",)))
    worker.cancel()
    assert worker.run() is None and np.array_equal(model.get_colors.cpu().numpy(), bad)


def _write_ply(path, n, seed):
    from gaussiansplattingregistration_amd.utils import ply_io
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    dc = (rng.uniform(0.2, 0.8, (n, 3)) - 0.5) / M.C0
    ply_io.save_gaussian_ply(path, rng.uniform(-1, 1, (n, 3)), dc, rng.normal(0, 0.02, (n, 9)), rng.normal(1.0, 1.0, n), rng.normal(-2.3, 0.3, (n, 3)), q)


def test_the_two_script_flags_on_tiny_ply_files(tmp_path, monkeypatch, capsys):
    """scripts/evaluate_registration.py --finetune and scripts/register_ply.py --finetune on two small .ply files, a cameras.json and PNGs
    rendered from the merged model with the second scene's colours brightened: the flags run, log, and save"""
    from PIL import Image
    from gaussiansplattingregistration_amd.models.camera import load_cameras
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.utils import ply_io
    from gaussiansplattingregistration_amd.utils.rasterization_util import rasterize_image
    _write_ply(tmp_path / "a.ply", 400, 1)
    _write_ply(tmp_path / "b.ply", 300, 1)          # the same generator: its splats sit on the first 300 of a.ply, so the registration has pairs
    np.savetxt(tmp_path / "T.txt", np.eye(4))
    entries = []
    for k, eye in enumerate(((0.0, 0.0, -4.0), (3.0, 1.0, -2.5), (-3.0, 0.5, -2.5), (0.5, -2.0, -3.5))):
        V = M.look_at(eye, (0, 0, 0)).astype(np.float64)
        entries.append({"id": k, "img_name": f"photo_{k}", "width": 72, "height": 48, "fx": 70.0, "fy": 72.0, "rotation": V[:3, :3].T.tolist(), "position": list(eye)})
    (tmp_path / "cameras.json").write_text(json.dumps(entries))
    images = tmp_path / "images"
    images.mkdir()
    cams = load_cameras(str(tmp_path / "cameras.json"))
    pc1, pc2 = (GaussianModel("cuda:0").from_ply(str(tmp_path / f)) for f in ("a.ply", "b.ply"))
    pc2._features_dc = pc2._features_dc + 0.3                       # the photographs show a brighter second scene than b.ply holds
    merged = GaussianModel.get_merged_gaussian_point_clouds(pc1, pc2, np.eye(4))
    for cam in cams:
        img = rasterize_image(merged, cam, 1, (0, 0, 0), "cuda:0")[0].clamp(0, 1).cpu().numpy()
        Image.fromarray(np.floor(img * 255.0 + 0.5).astype(np.uint8)).save(images / (cam.image_name + ".png"))

    def load(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    monkeypatch.setattr("sys.argv", ["evaluate_registration.py", str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--transform", str(tmp_path / "T.txt"), "--cameras",
                                     str(tmp_path / "cameras.json"), "--images", str(images), "--log", str(tmp_path / "log.json"), "--finetune", "30",
                                     "--finetune-holdout", "2"])
    load("evaluate_registration").main()
    lines = [json.loads(ln) for ln in capsys.readouterr().out.strip().splitlines() if ln.startswith("{")]
    line = [ln for ln in lines if "finetune" in ln][0]
    rec = json.loads((tmp_path / "log.json.finetune").read_text())
    assert line["finetune"] == 30 and line["train_cameras"] == 2 and line["held_out_cameras"] == 2 and len(rec["losses"]) == 30
    assert rec["held_out_with"]["mse"] < rec["held_out_without"]["mse"] and rec["losses"][-1] < rec["losses"][0]
    assert "mse" in lines[-1] and "finetune" not in lines[-1]                      # the evaluation's own line stays the last
    out = tmp_path / "merged.ply"
    monkeypatch.setattr("sys.argv", ["register_ply.py", str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--voxel", "--type", "point", "--max-corr", "0.05", "--iters", "1",
                                     "--out", str(out), "--finetune", str(tmp_path / "cameras.json"), "--finetune-images", str(images), "--finetune-iters", "8",
                                     "--finetune-params", "dc,opacity"])
    load("register_ply").main()
    text = capsys.readouterr().out
    assert "fine-tuning (dc,opacity): 8 iterations over 4 cameras" in text
    saved = ply_io.load_gaussian_arrays(str(out))
    assert len(saved["xyz"]) == 700
