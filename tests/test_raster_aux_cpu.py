"""The auxiliary outputs of the rasteriser without a GPU: the NumPy model (tests/raster_aux_model.py) against raster_model and against
what can be said analytically, the conditions tests/test_raster_aux_gpu.py relies on (fragile fractions, tight splats, the recorded
float32 cost, the pruning scene), the new C-ABI entry without a device, the geometric evaluator's log and the depth-agreement formulas."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import raster_aux_model as A
import raster_model as M
from conftest import GOLDEN

TOLERANCE = os.path.join(GOLDEN, "raster_aux_tolerance.json")


@pytest.mark.parametrize("name", list(M.SCENES))
def test_model_image_is_raster_models_bit_for_bit(name):
    m = A.scene_models(name)
    assert np.array_equal(m["r64"]["image"], m["ref"]["image"])
    r32 = M.render(m["scaled"], m["cam"], m["bg"], np.float32)
    assert m["r32"]["image"].dtype == np.float32 and np.array_equal(m["r32"]["image"].view(np.uint32), r32["image"].view(np.uint32))


def _splat(xyz, s, op_raw):
    n = len(xyz)
    return dict(xyz=np.float32(xyz), cov6=np.float32([[s * s, 0, 0, s * s, 0, s * s]] * n), opacity=np.float32(op_raw), color=np.zeros((n, 3), np.float32),
                sh=np.zeros((n, 0), np.float32), sh_degree=0)


def _axis_cam(W=96, H=80, f=120.0):
    # the principal point on a pixel centre: the splat on the axis has its mean exactly there
    return dict(viewmat=np.eye(4, dtype=np.float32), fx=f, fy=f, cx=W / 2 + 0.5, cy=H / 2 + 0.5, width=W, height=H)


@pytest.mark.parametrize("op_raw", [1.25, 12.0], ids=["translucent", "clamped_at_0.999"])
def test_one_splat_on_the_axis_gives_its_depth_and_opacity(op_raw):
    z, W, H = 4.0, 96, 80
    r = A.render_aux(_splat([[0, 0, z]], 0.0625, [op_raw]), _axis_cam(W, H))
    want = min(0.999, 1.0 / (1.0 + np.exp(-op_raw)))
    assert r["alpha"][H // 2, W // 2] == pytest.approx(want, rel=1e-12)
    assert r["depth"][H // 2, W // 2] == pytest.approx(z, rel=1e-12)
    covered = r["alpha"] > 0
    assert covered.sum() > 20 and r["alpha"][covered].min() >= 1.0 / 255.0
    assert np.allclose(r["depth"][covered], z, rtol=1e-12) and (r["depth"][~covered] == 0).all() and (r["alpha"][~covered] == 0).all()
    (sl, w, _), = r["per"].values()
    assert w.max() == pytest.approx(want, rel=1e-12)           # the splat's largest weight: its opacity, T = 1 in front of it


def test_two_splats_in_a_line_give_the_analytic_expected_depth():
    z1, z2, o1, o2, W, H = 3.0, 5.0, 0.5, -0.25, 96, 80
    r = A.render_aux(_splat([[0, 0, z2], [0, 0, z1]], 0.0625, [o2, o1]), _axis_cam(W, H))       # given back to front: the model sorts
    a1, a2 = 1 / (1 + np.exp(-o1)), 1 / (1 + np.exp(-o2))
    w1, w2 = a1, a2 * (1 - a1)
    assert r["alpha"][H // 2, W // 2] == pytest.approx(w1 + w2, rel=1e-12)
    assert r["depth"][H // 2, W // 2] == pytest.approx((z1 * w1 + z2 * w2) / (w1 + w2), rel=1e-12)
    assert r["per"][1][1].max() == pytest.approx(w1, rel=1e-12) and r["per"][0][1].max() == pytest.approx(w2, rel=1e-12)


def _costs():
    return {name: A.float32_cost(name) for name in M.SCENES}


@pytest.mark.parametrize("name", list(M.SCENES))
def test_scenes_meet_the_conditions_of_the_gpu_test(name):
    """fragile pixels at most 1 %, tight splats at least 85 % of the visible ones, and the recorded float32 cost is the model's"""
    m = A.scene_models(name)
    assert m["ref"]["fragile"].mean() <= 0.01
    vis = np.array(sorted(m["r64"]["per"]))
    tight = (m["hi"][vis] <= m["lo"][vis]).mean()
    print(f"{name}: visible {len(vis)}, tight {tight:.3f}, lo > 0: {(m['lo'][vis] > 0).mean():.3f}")
    assert tight >= 0.85, tight
    covered = (m["r64"]["alpha"] > 0).mean()
    assert covered > 0.1, covered
    if not os.path.exists(TOLERANCE):                                   # the committed file is the record; a fresh one is written only when it is absent
        with open(TOLERANCE, "w") as out:
            json.dump(_costs(), out, indent=1)
    want = json.load(open(TOLERANCE))[name]
    got = A.float32_cost(name)
    print(f"{name}: float32 model against float64 model {got}")
    for key, bound in (("alpha_max_abs_diff", 2e-5), ("depth_max_rel_diff", 1e-4), ("contribution_max_abs_diff", 2e-5)):
        assert got[key] == pytest.approx(want[key], rel=1e-6, abs=1e-12)
        assert 0 < got[key] < bound           # a few float32 ulps of values in [0, 1] (depth: of a quotient of two such sums), summed over a pixel's splats


def test_prune_scene_meets_its_conditions():
    p = A.prune_models()
    keep, drop = p["keep"].mean(), p["drop"].mean()
    print(f"prune scene: keep {keep:.3f} drop {drop:.3f} undecided {1 - keep - drop:.3f} fragile {p['fragile']}")
    assert keep >= 0.10 and drop >= 0.10 and 1 - keep - drop <= 0.05
    assert not (p["keep"] & p["drop"]).any()
    for ref, _ in p["refs"]:
        assert ref["max_rgb"] <= 1.0                       # the bound on the pruned render needs colours within [0, 1]
    # without a clip (prune_unseen's default) the small splats count: more rows are kept, and still almost every row is decided
    p0 = A.prune_models(0.0)
    print(f"prune scene, no clip: keep {p0['keep'].mean():.3f} drop {p0['drop'].mean():.3f}")
    assert p0["keep"].sum() > p["keep"].sum() and p0["drop"].any() and (~p0["keep"] & ~p0["drop"]).mean() <= 0.05


def test_render_aux_entry_without_a_device(hip_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    nul = None
    args = [nul, 0, 0, 0, nul, nul, nul, nul, nul, nul, 1.0, 1.0, 0.0, 0.0, 8, 8, nul, 3.0, nul, nul, nul, nul, nul, nul]
    assert hip_lib.gsr_raster_render_aux(*args) == -1                         # GSR_E_INVALID
    assert b"gsr_raster_render_aux" in hip_lib.gsr_last_error()
    from gaussiansplattingregistration_amd import raster
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raster.RasterContext()
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    scene, _, _ = M.build(M.EXACT_SCENE)
    model = GaussianModel("cpu").from_arrays(scene["xyz"], scene["color"], scene["opacity"], scene["cov6"], scene["sh"], scene["sh_degree"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.max_contribution([])


def test_geometry_evaluator_with_no_cameras_writes_null_metrics(tmp_path):
    from gaussiansplattingregistration_amd.workers.evaluator import GEOMETRY_LOG_FIELDS, GeometryEvaluator
    log = tmp_path / "geometry.json"
    result = GeometryEvaluator(None, None, np.eye(4), [], str(log), coverage=0.25).run()
    data = json.loads(log.read_text())
    assert list(data) == list(GEOMETRY_LOG_FIELDS)
    assert all(data[k] is None for k in ("depth_mae", "depth_rmse", "depth_rel", "depth_overlap"))
    assert data["per_camera"] == [] and data["error_list"] == [] and data["registration_data"] == {} and data["coverage"] == 0.25
    assert result.depth_mae is None


def test_geometry_evaluator_cancel_is_polled_between_cameras(tmp_path):
    from gaussiansplattingregistration_amd.models.camera import cameras_from_json
    from gaussiansplattingregistration_amd.workers.evaluator import GeometryEvaluator
    golden = dict(np.load(os.path.join(GOLDEN, "eval_metrics.npz")))
    cams = cameras_from_json(json.loads(str(golden["cameras_json"])))
    ev = GeometryEvaluator(None, None, np.eye(4), cams, str(tmp_path / "log.json"))
    ev.cancel_evaluation()
    assert ev.run() is None and not (tmp_path / "log.json").exists()


def test_depth_agreement_formulas_on_hand_made_maps():
    from gaussiansplattingregistration_amd.workers.evaluator import depth_agreement
    d1 = np.float32([[1, 2, 3, 4], [2, 2, 2, 2], [5, 5, 5, 5], [0, 0, 0, 0]])
    d2 = np.float32([[1, 2.5, 2, 4], [3, 2, 2, 2], [5, 5, 5, 5], [7, 7, 0, 0]])
    a1 = np.float32([[1, 1, 1, 0.5], [0.9, 0.4, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])
    a2 = np.float32([[1, 0.6, 1, 0.5], [0.5, 1, 1, 0], [0, 0, 0, 0], [1, 0.7, 0, 0]])
    # both >= 0.5: (0,0) (0,1) (0,2) (0,3) (1,0) -> differences 0, -0.5, 1, 0, -1; either: those + (1,1) (1,2) (3,0) (3,1)
    r = depth_agreement(d1, a1, d2, a2, 0.5)
    assert (r["n_mask"], r["n_union"]) == (5, 9)
    assert r["depth_mae"] == pytest.approx(2.5 / 5, rel=1e-15)
    assert r["depth_rmse"] == pytest.approx(np.sqrt(2.25 / 5), rel=1e-15)
    assert r["depth_rel"] == pytest.approx((0.5 / 2.25 + 1 / 2.5 + 1 / 2.5) / 5, rel=1e-15)
    assert r["depth_overlap"] == pytest.approx(5 / 9, rel=1e-15)
    # a stricter threshold: only (0,0) and (0,2) remain; the union is those + (0,1) (1,0)->a1 0.9, (1,1) (1,2) (3,0)
    r = depth_agreement(d1, a1, d2, a2, 0.9)
    assert (r["n_mask"], r["n_union"]) == (2, 7) and r["depth_mae"] == pytest.approx(0.5)
    # an empty mask: the three depth figures are None, the overlap is 0; nothing covered at all: the overlap is None too
    r = depth_agreement(d1, a1, d2, np.zeros_like(a2), 0.5)
    assert r["n_mask"] == 0 and r["depth_mae"] is None and r["depth_rmse"] is None and r["depth_rel"] is None and r["depth_overlap"] == 0.0
    r = depth_agreement(d1, np.zeros_like(a1), d2, np.zeros_like(a2), 0.5)
    assert r["depth_overlap"] is None and r["n_union"] == 0
