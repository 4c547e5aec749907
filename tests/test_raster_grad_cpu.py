"""The backward pass of the rasteriser without a GPU: the analytic NumPy model (tests/raster_grad_model.py) against central differences
of the float64 forward model, per-pixel closed forms for one isotropic splat, the scene ``grad_edges`` and the conditions
tests/test_raster_grad_gpu.py relies on, the recorded float32 cost, the two new C-ABI entries without a device and the argument checks
that need none.

Finite differences.  ``L = sum G_C . image + sum G_A . alpha`` with fixed random G zeroed on the forward's fragile pixels.  G is drawn from
[0.5, 1.5]: image and alpha are not negative, so L is a sum of terms of one sign and ``eps |L|`` is the round-off of evaluating it (with G of
both signs L cancels to a small number and that floor would mean nothing; the GPU tests draw G from a normal distribution).  Image and alpha
are ``raster_aux_model.render_aux``'s in float64 (its image is ``raster_model.render``'s bit for bit: tests/test_raster_aux_cpu.py).  The
forward model narrows its inputs to float32 before it widens them, so a step must add to a value EXACTLY in float32 or the rounding of
the input (2^-24 / h) swamps the difference: the scenes used here hold values of 11 significant bits (``grad_edges`` is built so, ``exact``
is rounded with ``raster_grad_model.coarse`` -- its fragile mask is still empty, asserted below), directions are ``2^floor(log2 |x|)`` times
a multiple of 1/4 in [-1, 1] per entry, and the step is h = 2^-20 (and h / 2 = 2^-21), relative to each entry's own power of two.  The
analytic value must lie within ``4 |FD(h) - FD(h/2)| + 8 eps |L| / h`` of ``FD(h/2)`` (Richardson's estimate of the truncation error plus the
round-off floor, eps = 2^-52).
"""
import json
import os

import numpy as np
import pytest

import raster_aux_model as A
import raster_grad_model as G
import raster_model as M
from conftest import GOLDEN

TOLERANCE = os.path.join(GOLDEN, "raster_grad_tolerance.json")
H_STEP = 2.0 ** -20
KEYS = dict(xyz="xyz", cov6="cov6", raw_opacity="opacity", dc="color", sh_rest="sh")
_cache = {}


def _fd_case(name):
    if name not in _cache:
        scene, cam, bg = G.build(name)
        scene = G.coarse(scene)
        ref = M.render(scene, cam, bg)
        H, W = ref["fragile"].shape
        rng = np.random.default_rng(G.hash_name(name))
        G_C, G_A = rng.uniform(0.5, 1.5, (H, W, 3)).astype(np.float32), rng.uniform(0.5, 1.5, (H, W)).astype(np.float32)
        G_C[ref["fragile"]] = 0
        G_A[ref["fragile"]] = 0
        ana = G.backward(scene, cam, G_C, G_A, bg)
        _cache[name] = dict(scene=scene, cam=cam, bg=bg, ref=ref, G_C=G_C.astype(np.float64), G_A=G_A.astype(np.float64), ana=ana)
    return _cache[name]


def _loss(c, scene):
    r = A.render_aux(scene, c["cam"], c["bg"])
    return float((c["G_C"] * r["image"]).sum() + (c["G_A"] * r["alpha"]).sum())


def _unit(x):
    """2^floor(log2 |x|) per entry; for a zero entry that of the largest entry of its row (any float32 step adds to zero exactly)"""
    x = np.asarray(x, np.float64)
    rows = np.abs(x.reshape(len(x), -1)).max(axis=1).reshape((len(x),) + (1,) * (x.ndim - 1))
    mag = np.where(x == 0, np.where(rows == 0, 1.0, rows), np.abs(x))
    return 2.0 ** np.floor(np.log2(mag))


def _directional(c, key, d):
    """-> (FD(h), FD(h/2), |L|) along d (already scaled by the entries' units)"""
    base = c["scene"][key].astype(np.float64)
    out = []
    for h in (H_STEP, H_STEP / 2):
        vals = []
        for sign in (1.0, -1.0):
            moved = base + sign * h * d
            assert np.array_equal(moved.astype(np.float32).astype(np.float64), moved)          # the step is exact in float32
            vals.append(_loss(c, dict(c["scene"], **{key: moved.astype(np.float32)})))
        out.append((vals[0] - vals[1]) / (2 * h))
    return out[0], out[1], abs(_loss(c, c["scene"]))


def _assert_close(what, ana, fd_h, fd_h2, L):
    allowed = 4 * abs(fd_h - fd_h2) + 8 * 2.0 ** -52 * L / H_STEP
    assert abs(ana - fd_h2) <= allowed, (what, ana, fd_h2, abs(ana - fd_h2), allowed)
    return abs(ana - fd_h2), allowed


@pytest.mark.parametrize("name", [M.EXACT_SCENE, G.GRAD_EDGES])
def test_analytic_backward_matches_central_differences_along_random_directions(name):
    """h = 2^-20 (see the module docstring); 16 directions per input array"""
    c = _fd_case(name)
    assert c["ref"]["fragile"].mean() <= 0.01
    rng = np.random.default_rng(5)
    worst = {}
    for out, key in KEYS.items():
        base = c["scene"][key]
        unit = _unit(base)
        for trial in range(16):
            d = unit * rng.integers(-4, 5, base.shape) / 4.0
            ana = float((c["ana"][out].reshape(base.shape) * d).sum())
            err, allowed = _assert_close((name, out, trial), ana, *_directional(c, key, d))
            worst[out] = max(worst.get(out, 0.0), err / max(abs(ana), 1e-300))
    print(f"{name}: largest |analytic - FD(h/2)| / |analytic| per array {worst}")


def _five(name, c):
    if name == G.GRAD_EDGES:
        return [G.ROW_CLAMPED_OPACITY, G.ROW_CLAMPED_COLOUR, G.ROW_CLAMPED_JACOBIAN, G.ROW_EVERY_TILE, G.ROW_STOP]
    return [int(i) for i in np.nonzero(c["ana"]["ok"])[0][:5]]


@pytest.mark.parametrize("name", [M.EXACT_SCENE, G.GRAD_EDGES])
def test_analytic_backward_matches_central_differences_on_every_coordinate_of_five_splats(name):
    """h = 2^-20 of each coordinate's own power of two; on grad_edges the clamped-opacity, clamped-colour and clamped-Jacobian splats are
    among the five"""
    c = _fd_case(name)
    for row in _five(name, c):
        assert c["ana"]["ok"][row]
        for out, key in KEYS.items():
            base = c["scene"][key]
            unit = _unit(base)
            for col in range(base[row].size):
                d = np.zeros(base.shape)
                d.reshape(len(base), -1)[row, col] = unit.reshape(len(base), -1)[row, col]
                ana = float((c["ana"][out].reshape(base.shape) * d).sum())
                _assert_close((name, row, out, col), ana, *_directional(c, key, d))


def test_one_isotropic_splat_has_the_closed_form_gradients():
    """one splat on the optical axis of an identity camera, SH degree 0: alpha_p = o exp(-r_p^2 / (2 s2)), s2 = (f s / z)^2 + 0.3,
    C_p = alpha_p c + (1 - alpha_p) bg, A_p = alpha_p; the gradients with respect to dc, the raw opacity, x and the isotropic variance
    follow per pixel"""
    z, W, H, f, s, raw = 4.0, 48, 40, 60.0, 0.25, 0.4
    scene = dict(xyz=np.float32([[0, 0, z]]), cov6=np.float32([[s * s, 0, 0, s * s, 0, s * s]]), opacity=np.float32([raw]), color=np.float32([[0.3, -0.2, 0.9]]),
                 sh=np.zeros((1, 0), np.float32), sh_degree=0)
    cam = dict(viewmat=np.eye(4, dtype=np.float32), fx=f, fy=f, cx=W / 2 + 0.5, cy=H / 2 + 0.5, width=W, height=H)
    bg = (0.1, 0.2, 0.3)
    rng = np.random.default_rng(3)
    G_C, G_A = rng.normal(size=(H, W, 3)).astype(np.float32), rng.normal(size=(H, W)).astype(np.float32)
    got = G.backward(scene, cam, G_C, G_A, bg)
    o = 1 / (1 + np.exp(-np.float64(np.float32(raw))))
    s2 = (f * np.float64(np.float32(s * s)) ** 0.5 / z) ** 2 + 0.3
    dx = (W / 2 + 0.5) - (np.arange(W) + 0.5)[None, :]
    dy = (H / 2 + 0.5) - (np.arange(H) + 0.5)[:, None]
    sigma = 0.5 * (dx * dx + dy * dy) / s2
    alpha = o * np.exp(-sigma)
    counted = alpha >= 1 / 255
    (sl, upd, clamped), = got["counted"].values()
    assert np.array_equal(upd, counted[sl]) and not clamped.any() and counted.sum() > 100
    colour = M.C0 * scene["color"][0].astype(np.float64) + 0.5
    gc = G_C.astype(np.float64)
    dalpha = np.where(counted, (gc * (colour - np.float64(np.float32(bg)))).sum(2) + G_A, 0.0)          # dL/dalpha_p
    assert got["dc"][0] == pytest.approx(M.C0 * (np.where(counted, alpha, 0)[..., None] * gc).sum((0, 1)), rel=1e-12)
    assert got["raw_opacity"][0] == pytest.approx((dalpha * alpha).sum() * (1 - o), rel=1e-12)
    # x moves the mean by f / z per unit (the Jacobian's x / z term multiplies Sigma_c's zero xz entry): d alpha / d mx = -alpha dx / s2
    assert got["xyz"][0, 0] == pytest.approx((dalpha * alpha * (-dx / s2)).sum() * f / z, rel=1e-10)
    assert got["xyz"][0, 1] == pytest.approx((dalpha * alpha * (-dy / s2)).sum() * f / z, rel=1e-10)
    # the xx entry of the covariance: a = (f / z)^2 S_xx + 0.3, sigma = dx^2 / (2 a) + dy^2 / (2 c): d sigma / d S_xx = -(f / z)^2 dx^2 / (2 a^2)
    assert got["cov6"][0, 0] == pytest.approx((dalpha * alpha * (f / z) ** 2 * dx * dx / (2 * s2 * s2)).sum(), rel=1e-10)
    assert got["cov6"][0, 1] == pytest.approx((dalpha * alpha * (f / z) ** 2 * dx * dy / (s2 * s2)).sum(), rel=1e-9, abs=1e-12)


def test_grad_edges_holds_every_case_it_was_built_for():
    m = G.scene_models(G.GRAD_EDGES)
    scene, cam, both, P = m["scene"], m["cam"], m["both"], m["both"]["P"]
    assert (cam["width"], cam["height"]) == (41, 27) and (P["tiles_x"], P["tiles_y"]) == (3, 2)          # partial tiles at both edges
    assert float(scene["opacity"][G.ROW_CLAMPED_OPACITY]) == 9.0
    assert both["counted"][G.ROW_CLAMPED_OPACITY][2].any()                                                # the 0.999 clamp is active on a pixel it counts
    sw = G.switches(scene, cam)
    assert sw["colour_off"][G.ROW_CLAMPED_COLOUR, 0] and P["ok"][G.ROW_CLAMPED_COLOUR]
    assert (both["dc"][G.ROW_CLAMPED_COLOUR, 0] == 0) and both["dc"][G.ROW_CLAMPED_COLOUR, 1] != 0
    assert sw["jac_active"][G.ROW_CLAMPED_JACOBIAN] and both["counted"][G.ROW_CLAMPED_JACOBIAN][1].sum() > 50      # clamped, off-screen centre, visible
    assert not (0 <= P["mx"][G.ROW_CLAMPED_JACOBIAN] < 41)
    stack = np.arange(G.ROW_STACK, G.ROW_STACK + G.STACK)
    assert P["ok"][stack].all() and (P["x0"][stack] == 1).all() and (P["x1"][stack] == 2).all() and (P["y0"][stack] == 0).all() and (P["y1"][stack] == 1).all()
    in_tile = P["ok"] & (P["x0"] <= 1) & (P["x1"] > 1) & (P["y0"] <= 0) & (P["y1"] > 0)
    assert in_tile.sum() > 256 + 16                                                                        # two LDS batches in tile (1, 0)
    # the reverse walk crosses the batch boundary with live pixels: a pixel of that tile counts splats on both sides of sorted position 256
    pp = G.pixel_pass(scene, cam, m["G_C"], m["G_A"], m["bg"])
    order = [int(i) for i in pp["order"] if in_tile[i]]
    early, late = np.zeros((27, 41), bool), np.zeros((27, 41), bool)
    for pos, i in enumerate(order):
        sl, upd, _ = pp["counted"][i]
        (early if pos < 256 else late)[sl] |= upd
    crossing = early & late
    assert crossing[0:16, 16:32].sum() >= 16
    stop = np.arange(G.ROW_STOP, G.ROW_STOP + G.STOPPERS)
    assert both["stopped"].sum() >= 16 and both["stopped"][both["counted"][int(stop[0])][0]].any()          # the 1e-4 stop is reached on the stoppers' spot
    a, b = G.ROW_EQUAL_DEPTH
    assert np.float32(P["z"][a]) == np.float32(P["z"][b]) and P["ok"][a] and P["ok"][b]
    assert P["x0"][b] >= P["x0"][a] and P["x1"][b] <= P["x1"][a] and P["y0"][b] >= P["y0"][a] and P["y1"][b] <= P["y1"][a]      # they share tiles
    r = G.ROW_EVERY_TILE
    assert (P["x0"][r], P["x1"][r], P["y0"][r], P["y1"][r]) == (0, 3, 0, 2) and P["ok"][r]
    assert not P["ok"][list(G.ROW_BEHIND)].any()
    for k in G.OUTPUTS:
        assert not both[k][list(G.ROW_BEHIND)].any()
    # every array rounded to 11 significant bits, as the finite differences need
    for k in ("xyz", "cov6", "opacity", "color", "sh"):
        assert np.array_equal(G.coarse(scene)[k], scene[k])


@pytest.mark.parametrize("name", list(G.GPU_SCENES))
def test_scenes_meet_the_conditions_of_the_gpu_test(name):
    """fragile pixels at most 1 %; no (splat, pixel) within a relative 1e-4 of the 0.999 clamp, no colour channel within 1e-4 of its clamp, no
    Jacobian clamp within 1e-4 of its switch; the recorded float32 cost is the model's"""
    m = G.scene_models(name)
    assert m["ref"]["fragile"].mean() <= 0.01
    if name == M.EXACT_SCENE:
        assert not m["ref"]["fragile"].any()
    sw = G.switches(m["scene"], m["cam"])
    print(f"{name}: fragile {m['ref']['fragile'].mean():.4f}, switches " + str({k: v for k, v in sw.items() if not isinstance(v, np.ndarray)}))
    assert sw["opacity_clamp"] > M.REL and sw["colour"] > M.REL and sw["jacobian"] > M.REL
    assert (m["both"]["abs9"] > 0).any()
    got = G.float32_cost(name)
    want = json.load(open(TOLERANCE))[name]
    print(f"{name}: float32 model against float64 model {got}")
    for k in G.OUTPUTS:
        assert got[k] == pytest.approx(want[k], rel=1e-6, abs=1e-12)
        assert 0 < got[k] < 1e-3          # some float32 roundings (2^-24 each) of terms that are sums of up to a few thousand pixel terms and a chain of about 40 operations


def test_coarse_exact_scene_keeps_an_empty_fragile_mask():
    c = _fd_case(M.EXACT_SCENE)
    assert not c["ref"]["fragile"].any() and c["ref"]["visible"] > 30


def test_float32_model_follows_the_tile_tree():
    """the fold of a tile is the tree of adjacent pairs, not a running sum: on values chosen so that float32 tells the two apart"""
    v = np.zeros((16, 16), np.float32)
    v[0, 0], v[0, 1], v[0, 2] = 1.0, 2.0 ** -24, 2.0 ** -24
    assert G.tile_fold(v) == np.float32(1.0)                       # (1 + 2^-24) rounds to 1, then + (2^-24 + 0) rounds to 1 again
    v[0, 1], v[0, 3] = 0.0, 2.0 ** -24
    assert G.tile_fold(v) == np.float32(1.0 + 2.0 ** -23)          # (2^-24 + 2^-24) is added to 1 as one value
    assert G.tile_fold(v.astype(np.float64)) == 1.0 + 2.0 ** -23


def test_backward_entries_without_a_device(hip_lib):
    import torch
    nul = None
    args = [nul, 0, 0, 0, nul, nul, nul, nul, nul, nul, 1.0, 1.0, 0.0, 0.0, 8, 8, nul, 3.0] + [nul] * 9
    assert hip_lib.gsr_raster_backward(*args) == -1                          # GSR_E_INVALID
    assert b"gsr_raster_backward" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_raster_get_backward_timing(None, None) == -1
    assert b"gsr_raster_get_backward_timing" in hip_lib.gsr_last_error()
    if torch.cuda.is_available():                  # the rest is about a machine without one
        return
    from gaussiansplattingregistration_amd import raster
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raster.render_differentiable(torch.zeros(1, 3), torch.zeros(1, 6), torch.zeros(1), torch.zeros(1, 3), None, 0, np.eye(4), 1.0, 1.0, 0.0, 0.0, 8, 8)


def test_finetuner_argument_checks():
    from gaussiansplattingregistration_amd.finetune import FinetuneParams, ModelFinetuner
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    p = FinetuneParams()
    assert (p.iterations, p.params, p.lr_dc, p.lr_sh_rest, p.lr_opacity, p.lr_xyz, p.loss, p.background) == (200, ("dc", "sh_rest", "opacity"), 2.5e-3, 1.25e-4, 0.05,
                                                                                                             1.6e-4, "l2", (0, 0, 0))
    scene, _, _ = M.build(M.EXACT_SCENE)
    model = GaussianModel("cpu").from_arrays(scene["xyz"], scene["color"], scene["opacity"], scene["cov6"], scene["sh"], scene["sh_degree"])
    with pytest.raises(ValueError, match="covariance is not tunable"):
        ModelFinetuner(model, [], [], FinetuneParams(params=("dc", "cov6")))
    with pytest.raises(ValueError, match="loss"):
        ModelFinetuner(model, [], [], FinetuneParams(loss="ssim"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):              # a model on the host, with or without a GPU in the machine
        ModelFinetuner(model, [], [], FinetuneParams())
