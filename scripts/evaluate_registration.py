"""Image-based evaluation of a registration result, headless: the reference's Evaluation tab without the GUI.

    python scripts/evaluate_registration.py a.ply b.ply --transform T.txt --cameras cameras.json --images DIR --log out.json
                                            [--rotate-sh] [--with-scaling] [--fuse-overlap MAX_DIST [--fuse-kld X] [--fuse-color X]]
                                            [--save-renders DIR] [--background R G B] [--cpu-metrics]
                                            [--photo-refine --photo-max-depth-diff D [--photo-scales 4,2,1] [--photo-lambda L]]
    python scripts/evaluate_registration.py a.ply b.ply --transform T.txt --cameras cameras.json --geometry [--coverage 0.5] --log out.json

``a.ply`` is moved by the 4x4 in ``T.txt`` (whitespace-separated, row-major) and merged with ``b.ply``; the merged model is rendered
from every camera of ``cameras.json`` (the file a 3DGS training run writes) and compared with ``DIR/<img_name>.png``.  The log has the
reference's fields: registration_data, mse, rmse, ssim, psnr, lpips (null: no LPIPS weights here), error_list.

``--geometry`` needs no photographs: ``a.ply`` moved by the transform and ``b.ply`` are rendered separately to depth and coverage maps
from every camera, and compared where both cover a pixel (coverage >= ``--coverage``): depth_mae, depth_rmse, depth_rel, depth_overlap,
per camera and as means (``GeometryEvaluator``).  With ``--images`` as well, both evaluations run; the geometric log then goes to
``<log>.geometry``.

``--finetune N [--finetune-holdout K] [--finetune-params dc,sh_rest,opacity] [--finetune-loss l2|l1|l1_dssim] [--finetune-lambda L]``: the merged model is fine-tuned for N
iterations (``finetune.ModelFinetuner``) on the cameras that are not held out (every K-th is, default 8); MSE / PSNR / SSIM on the held-out
cameras without and with it go to ``<log>.finetune``.  ``l1_dssim`` is (1 - L) L1 + L (1 - SSIM), L = 0.2 by default.

``--photo-refine`` (rigid transforms only): the evaluations asked for run first on the transform as given, their logs beside the others
as ``<log>.no_photo_refine``; the transform is then refined on renders of the two scenes from the same cameras (``PhotometricRefiner``;
``--photo-max-depth-diff`` in scene units is required) and everything is evaluated again with the refined transform, which is printed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("first")
    ap.add_argument("second")
    ap.add_argument("--transform", required=True)
    ap.add_argument("--cameras", required=True)
    ap.add_argument("--images", help="the photographs DIR/<img_name>.png (required unless only --geometry is asked)")
    ap.add_argument("--geometry", action="store_true", help="geometric evaluation: depth maps of the two scenes from the same cameras")
    ap.add_argument("--coverage", type=float, default=0.5, help="--geometry: a pixel is compared when both renders have at least this alpha")
    ap.add_argument("--log", required=True)
    ap.add_argument("--rotate-sh", action="store_true", help="turn the SH coefficients of the first cloud with it")
    ap.add_argument("--with-scaling", action="store_true", help="the transform is a similarity [c R | t] (register_ply.py --with-scaling): the first "
                    "cloud's sizes and log-scales move with it")
    ap.add_argument("--fuse-overlap", type=float, metavar="MAX_DIST", help="fuse the splats the two clouds share before rendering (fuse_overlap: mutual "
                    "best matches within this distance); implies --rotate-sh")
    ap.add_argument("--fuse-kld", type=float, default=0.5, help="largest symmetrised KL divergence of a fused pair")
    ap.add_argument("--fuse-color", type=float, default=float("inf"), help="largest L2 distance of the DC colours of a fused pair")
    from gaussiansplattingregistration_amd.harmonize import add_match_colors_arguments, match_colors_from_args
    add_match_colors_arguments(ap)
    from gaussiansplattingregistration_amd.photo import add_photo_arguments, photo_params_from_args
    add_photo_arguments(ap, with_cameras=False)
    ap.add_argument("--save-renders", metavar="DIR", help="write every render as DIR/<img_name>.png")
    ap.add_argument("--background", type=float, nargs=3, default=(0.0, 0.0, 0.0))
    ap.add_argument("--cpu-metrics", action="store_true", help="use_gpu=False: the metrics in host torch arithmetic")
    ap.add_argument("--warp", metavar="FIELD.npz", help="a non-rigid field (register_ply.py --warp-out): every evaluation runs without it first "
                    "(logs with the suffix .no_warp), then with the first cloud warped behind the transform")
    ap.add_argument("--finetune", type=int, metavar="N", help="fine-tune the merged model for N iterations (finetune.ModelFinetuner, DESIGN.md 26) on the "
                    "cameras that are not held out and log MSE / PSNR / SSIM on the held-out ones without and with it (log suffix .finetune)")
    ap.add_argument("--finetune-holdout", type=int, default=8, metavar="K", help="every K-th camera (the first included) is held out of the fine-tuning")
    ap.add_argument("--finetune-loss", choices=("l2", "l1", "l1_dssim"), default="l2", help="l1_dssim: (1 - lambda) L1 + lambda (1 - SSIM), the fused loss kernel")
    ap.add_argument("--finetune-lambda", type=float, default=0.2, metavar="L", help="the weight of the SSIM term of --finetune-loss l1_dssim")
    ap.add_argument("--finetune-params", default="dc,sh_rest,opacity", help="the tensors --finetune tunes: comma-separated, of dc, sh_rest, opacity, xyz, "
                    "scaling, rotation (the last two tune the shape of the splats, DESIGN.md 31)")
    a = ap.parse_args()
    if a.finetune is not None and a.images is None:
        ap.error("--finetune needs --images")
    if a.images is None and not a.geometry:
        ap.error("the following arguments are required: --images")
    photo = photo_params_from_args(a)
    if photo is not None and a.with_scaling:
        ap.error("--photo-refine estimates a rigid motion: refused with --with-scaling")
    import __graft_entry__ as g
    g.build_hip()
    from gaussiansplattingregistration_amd.controllers.registration_controller import RegistrationController
    from gaussiansplattingregistration_amd.models.camera import load_cameras
    from gaussiansplattingregistration_amd.models.data_repository import DataRepository, UIStateRepository
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.params import FuseOverlapParams
    from gaussiansplattingregistration_amd.workers.evaluator import RegistrationEvaluator
    fuse = FuseOverlapParams(a.fuse_overlap, a.fuse_kld, a.fuse_color) if a.fuse_overlap is not None else None
    cm, gate = match_colors_from_args(a, fuse)
    a.rotate_sh = a.rotate_sh or fuse is not None or cm is not None
    repo, ui = DataRepository(), UIStateRepository()
    repo.pc_gaussian_list_first.append(GaussianModel("cuda:0").from_ply(a.first))
    repo.pc_gaussian_list_second.append(GaussianModel("cuda:0").from_ply(a.second))
    ui.transformation_matrix = np.loadtxt(a.transform, dtype=np.float64).reshape(4, 4)
    cameras = load_cameras(a.cameras)
    field = None
    if a.warp:
        from gaussiansplattingregistration_amd.warp import WarpField
        field = WarpField.load(a.warp)
        rcw = RegistrationController(repo, ui)
        if a.geometry:
            gw = rcw.evaluate_geometry(cameras, (a.log if a.images is None else a.log + ".geometry") + ".no_warp", coverage=a.coverage, rotate_sh=a.rotate_sh,
                                       with_scaling=a.with_scaling)
            print(json.dumps({"warp": False, "geometry": True, "depth_mae": gw.depth_mae, "depth_rmse": gw.depth_rmse, "depth_rel": gw.depth_rel,
                              "depth_overlap": gw.depth_overlap}))
        if a.images is not None:
            bw = rcw.evaluate_registration(cameras, a.images, a.log + ".no_warp", tuple(a.background), not a.cpu_metrics, rotate_sh=a.rotate_sh,
                                           with_scaling=a.with_scaling, fuse=fuse, match_colors=cm, match_colors_gate=gate)
            print(json.dumps({"warp": False, "psnr": bw.psnr, "ssim": bw.ssim, "mse": bw.mse}))
    if photo is not None:
        # the effect of the refinement: the same evaluations on the transform as given first (their logs beside the others), then with it
        rc0 = RegistrationController(repo, ui)
        if a.geometry:
            geo0 = rc0.evaluate_geometry(cameras, (a.log if a.images is None else a.log + ".geometry") + ".no_photo_refine", coverage=a.coverage,
                                         rotate_sh=a.rotate_sh, with_scaling=False)
            print(json.dumps({"photo_refine": False, "geometry": True, "depth_mae": geo0.depth_mae, "depth_rmse": geo0.depth_rmse, "depth_rel": geo0.depth_rel,
                              "depth_overlap": geo0.depth_overlap}))
        if a.images is not None:
            base0 = rc0.evaluate_registration(cameras, a.images, a.log + ".no_photo_refine", tuple(a.background), not a.cpu_metrics, rotate_sh=a.rotate_sh,
                                              fuse=fuse, match_colors=cm, match_colors_gate=gate)
            print(json.dumps({"photo_refine": False, "psnr": base0.psnr, "ssim": base0.ssim, "mse": base0.mse}))
        from gaussiansplattingregistration_amd.photo import report_lines
        pr = rc0.refine_photometric(cameras, photo)
        print("photometric refinement:")
        print("\n".join("  " + line for line in report_lines(pr)))
        print(json.dumps({"photo_refine": True, "transformation": np.asarray(pr.transformation).tolist(), "energy_initial": pr.energy_initial,
                          "energy_final": pr.energy_final, "n_pixels": pr.n_pixels, "iterations": pr.iterations}))
    if a.geometry:
        geo_log = a.log if a.images is None else a.log + ".geometry"
        geo = RegistrationController(repo, ui).evaluate_geometry(cameras, geo_log, coverage=a.coverage, rotate_sh=a.rotate_sh, with_scaling=a.with_scaling, warp=field)
        print(json.dumps({"geometry": True, "cameras": len(cameras), "coverage": a.coverage, "depth_mae": geo.depth_mae, "depth_rmse": geo.depth_rmse,
                          "depth_rel": geo.depth_rel, "depth_overlap": geo.depth_overlap, "errors": len(geo.error_list), "log": geo_log}))
        if a.images is None:
            return
    if cm is not None:
        # the effect against the photographs: the same evaluation without the harmonisation first (its log beside the other), then with it
        base = RegistrationController(repo, ui).evaluate_registration(cameras, a.images, a.log + ".no_match_colors", tuple(a.background), not a.cpu_metrics,
                                                                      rotate_sh=a.rotate_sh, with_scaling=a.with_scaling, fuse=fuse, warp=field)
        print(json.dumps({"match_colors": None, "psnr": base.psnr, "ssim": base.ssim, "mse": base.mse}))
        from gaussiansplattingregistration_amd import harmonize
        _, (transforms, cinfo) = GaussianModel.move_and_match_colors(repo.pc_gaussian_list_first[0], repo.pc_gaussian_list_second[0], ui.transformation_matrix,
                                                                     a.rotate_sh, a.with_scaling, cm, gate, warp=field)
        print("colours (scene 0 = first, scene 1 = second, the reference):")
        print("\n".join("  " + line for line in harmonize.report_lines(transforms, cinfo)))
        if a.colors_out:
            harmonize.write_json(a.colors_out, transforms, cinfo)
    if a.finetune is not None:
        from gaussiansplattingregistration_amd.finetune import FinetuneParams
        from gaussiansplattingregistration_amd.utils.evaluation_utils import metrics
        from gaussiansplattingregistration_amd.utils.rasterization_util import rasterize_image
        from gaussiansplattingregistration_amd.workers.evaluator import _json_value, _read_image
        k = max(2, a.finetune_holdout)
        held = [c for i, c in enumerate(cameras) if i % k == 0]
        train = [c for i, c in enumerate(cameras) if i % k != 0]
        rcf = RegistrationController(repo, ui)

        def held_out(model):
            rows = []
            for c in held:
                try:
                    gt = _read_image(os.path.join(a.images, c.image_name + ".png")).to("cuda:0")
                except (OSError, IOError):
                    continue
                img = rasterize_image(model, c, 1, tuple(a.background), "cuda:0").permute(0, 3, 1, 2)
                if tuple(img.shape) == tuple(gt.shape):
                    rows.append(metrics(img, gt))
            return {key: float(np.mean([r[key] for r in rows])) if rows else None for key in ("mse", "psnr", "ssim")}
        merge_args = dict(rotate_sh=a.rotate_sh, with_scaling=a.with_scaling, fuse=fuse, match_colors=cm, match_colors_gate=gate, warp=field)
        plain, _ = rcf.finetune_merged([], a.images, FinetuneParams(iterations=0, background=tuple(a.background)), **merge_args)
        before = held_out(plain)
        tuned, fr = rcf.finetune_merged(train, a.images, FinetuneParams(iterations=a.finetune, params=tuple(x for x in a.finetune_params.split(",") if x),
                                                                       background=tuple(a.background), loss=a.finetune_loss, lambda_dssim=a.finetune_lambda),
                                        **merge_args)
        after = held_out(tuned)
        record = {"finetune": a.finetune, "loss": a.finetune_loss, "train_cameras": len(fr.psnr_before), "held_out_cameras": len(held), "held_out_without": before, "held_out_with": after,
                  "train_psnr_before": fr.psnr_before, "train_psnr_after": fr.psnr_after, "losses": fr.losses, "error_list": fr.error_list}
        with open(a.log + ".finetune", "w") as out:
            json.dump(_json_value(record), out, indent=2)
        print(json.dumps(_json_value({key: record[key] for key in ("finetune", "train_cameras", "held_out_cameras", "held_out_without", "held_out_with")})))
    if a.save_renders:
        # the controller's call with a hook on the worker: the same evaluation, the renders kept
        os.makedirs(a.save_renders, exist_ok=True)
        from PIL import Image

        def keep(camera, render):
            img = render[0].clamp(0, 1).mul(255).add(0.5).floor().to("cpu").numpy().astype(np.uint8)
            Image.fromarray(img).save(os.path.join(a.save_renders, camera.image_name + ".png"))
        worker = RegistrationEvaluator(repo.pc_gaussian_list_first[0], repo.pc_gaussian_list_second[0], ui.transformation_matrix, cameras, a.images, a.log,
                                       tuple(a.background), None, not a.cpu_metrics, rotate_sh=a.rotate_sh, with_scaling=a.with_scaling, fuse=fuse,
                                       match_colors=cm, match_colors_gate=gate, warp=field)
        worker.on_render = keep
        result = worker.run()
    else:
        result = RegistrationController(repo, ui).evaluate_registration(cameras, a.images, a.log, tuple(a.background), not a.cpu_metrics, rotate_sh=a.rotate_sh,
                                                                        with_scaling=a.with_scaling, fuse=fuse, match_colors=cm, match_colors_gate=gate, warp=field)
    print(json.dumps({"warp": a.warp, "match_colors": cm.mode if cm is not None else None, "cameras": len(cameras), "mse": result.mse, "rmse": result.rmse, "psnr": result.psnr, "ssim": result.ssim, "lpips": result.lpips,
                      "errors": len(result.error_list), "log": a.log}))


if __name__ == "__main__":
    main()
