#!/usr/bin/env python3
"""Headless registration of two 3DGS .ply scenes on one MI355X: what the reference's GUI does through its "Mixture" and
"Multiscale registration" tabs (qt_gaussian_mixture.py, qt_multiscale_registrator.py), as a script.

    python scripts/register_ply.py first.ply second.ply --levels 3 --max-corr 0.5 0.3 0.2 0.1 --iters 50 30 20 10 \\
           [--type plane|point|color|general] [--loss none|tukey|cauchy|gm|huber --k 0.1] [--voxel] [--out merged.ply [--rotate-sh]]
           [--with-scaling] [--fuse-overlap MAX_DIST [--fuse-kld X] [--fuse-color X]]
           [--clean-knn K --clean-std R [--clean-radius R --clean-nb N] [--clean-min-opacity A] [--clean-max-extent S]]
           [--prune-unseen CAMERAS.json ... [--min-contribution 0.01]]
           [--match-colors [gain|channel_gain|affine] [--match-colors-huber K] [--match-colors-dist D] [--colors-out colors.json]]
           [--photo-refine CAMERAS.json --photo-max-depth-diff D [--photo-scales 4,2,1] [--photo-lambda L]]
           [--mixture-refine MAX_CORR [--mixture-cov-scale S] [--mixture-cov-floor F]]

`--with-scaling`: the two scenes do not share a unit of length (separate structure-from-motion runs).  Point-to-point ICP with scaling
(`--type point` is implied, any other type is refused); without a global method the start is `initial_similarity` (centroids and RMS
radii aligned); the result is a similarity [c R | t], and the merged .ply has the moved cloud's scale_* columns shifted by ln c.

`--fuse-overlap MAX_DIST` (with `--out`): the merged cloud stores the splats the two scenes share once (`GaussianModel.fuse_overlap`:
mutual best matches within MAX_DIST, a symmetrised KL divergence of at most `--fuse-kld` and DC colours within `--fuse-color` are
replaced by their moment-matched union); prints n_pairs / n_out.  Implies `--rotate-sh`.

`--clean-*`: both scenes go through floater removal (`GaussianModel.remove_floaters`, scripts/clean_ply.py has the stages) right after
loading: mixtures, registration and the merged cloud see the cleaned scenes.  Prints n -> n_kept per scene.

`--match-colors [MODE]` (with `--out`): the two scenes were captured with different exposure or white balance.  After the move the first
scene's colour transform is fitted against the second's over the splats they share (`GaussianModel.match_colors`: mutual best matches
within `--match-colors-dist`, default the fuse distance; a Huber-weighted fit of a gain, a gain per channel or an affine 3 x 4) and
applied to its DC and SH coefficients before the clouds are concatenated or fused.  Prints the transform and the colour residual
before and after; `--colors-out` writes them as JSON.  Implies `--rotate-sh`.

`--prune-unseen CAMERAS.json` (with `--out`, may be repeated): the merged cloud loses the splats no camera shows with a blending weight
of `--min-contribution` (`GaussianModel.prune_unseen`).  The cameras must be in the merged cloud's frame (the second scene's) and cover
BOTH scenes: a splat outside every frustum is dropped like an occluded one.

`--photo-refine CAMERAS.json --photo-max-depth-diff D`: after ICP and before the merge, the transform is refined on renders of the
two scenes from these cameras (in the second scene's frame; `PhotometricRefiner`): intensity and depth, coarse to fine over
`--photo-scales`, for the motions geometry alone does not constrain (a wall, a floor).  D, in scene units, is how far apart the two
rendered depths of a pixel may be for it to count.  Rigid only: refused with `--with-scaling`.

`--mixture-refine MAX_CORR`: after ICP and before `--photo-refine`, the transform is refined by mixture-to-mixture registration
(`do_mixture_registration`) on the finest clouds the script holds: every pair of splats within MAX_CORR counts, weighted by the
overlap of the two Gaussians (covariances times `--mixture-cov-scale` squared, plus `--mixture-cov-floor` on the diagonal), so the
sampling noise of a one-nearest match does not reach the transform.  Rigid only: refused with `--with-scaling`.

`--finetune CAMERAS.json --finetune-images DIR [--finetune-iters N] [--finetune-params dc,sh_rest,opacity] [--finetune-loss l2|l1|l1_dssim]
[--finetune-lambda L]` (with `--out`): the merged cloud is fine-tuned against the photographs of those cameras (`finetune.ModelFinetuner`,
DESIGN.md 26) after the merge and before the save.  `l1_dssim` is (1 - L) L1 + L (1 - SSIM), L = 0.2 by default, from the fused loss
kernel.  `--finetune-params` names the tensors to tune, of dc, sh_rest, opacity, xyz, scaling, rotation; with `scaling` /
`rotation` the shape of the splats is tuned and the saved file holds the tuned scales and quaternions.

Prints the 4x4 transformation (first -> second), fitness and inlier RMSE; `--out` saves the merged cloud.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("first")
    ap.add_argument("second")
    ap.add_argument("--levels", type=int, default=3, help="HEM mixture levels per cloud (ignored with --voxel)")
    ap.add_argument("--max-corr", type=float, nargs="+", default=[0.5, 0.3, 0.2, 0.1], help="coarse -> fine (voxel sizes with --voxel)")
    ap.add_argument("--iters", type=int, nargs="+", default=[50, 30, 20, 10])
    ap.add_argument("--type", choices=["point", "plane", "color", "general"], default=None, help="default: plane (point with --with-scaling)")
    ap.add_argument("--with-scaling", action="store_true", help="estimate a similarity (scale, rotation, translation): point-to-point only")
    ap.add_argument("--loss", choices=["none", "tukey", "cauchy", "gm", "huber"], default="none")
    ap.add_argument("--k", type=float, default=0.0)
    ap.add_argument("--voxel", action="store_true", help="voxel multiscale path instead of HEM mixtures")
    ap.add_argument("--hem", type=float, nargs=4, default=[3.0, 3.0, 2.5, 1.0], metavar=("RHO", "DELTA", "KAPPA", "TAU"))
    method = ap.add_mutually_exclusive_group()
    method.add_argument("--global-ransac", type=float, metavar="VOXEL", help="global registration first (FPFH + RANSAC at this voxel size, the "
                    "reference's Global tab); its pose is the multiscale ICP's initial transform")
    method.add_argument("--global-fgr", type=float, metavar="VOXEL", help="global registration first by Fast Global Registration (FPFH + FGR at "
                    "this voxel size, the tab's other method); its pose is the multiscale ICP's initial transform")
    method.add_argument("--global-sc2", type=float, metavar="VOXEL", help="global registration first by the compatibility-graph method (FPFH + "
                        "second-order consensus at this voxel size: deterministic, no sampling, rigid only); its pose is the multiscale ICP's "
                        "initial transform")
    ap.add_argument("--ransac-iters", type=int, default=100000, help="RANSAC hypotheses (max_iteration) of --global-ransac")
    ap.add_argument("--orient-normals", choices=("centroid", "consistent"), default="centroid", help="how --global-ransac / --global-fgr fix the "
                    "normals' signs before FPFH: towards the cloud's centroid, or propagated along the neighbour graph's spanning forest "
                    "(for scenes that are not star-shaped)")
    ap.add_argument("--out")
    ap.add_argument("--rotate-sh", action="store_true", help="turn the SH coefficients (view-dependent colour) of the moved cloud with it in the "
                    "merged output")
    ap.add_argument("--fuse-overlap", type=float, metavar="MAX_DIST", help="fuse the splats the two scenes share in the merged output (mutual best "
                    "matches within this distance); implies --rotate-sh")
    ap.add_argument("--fuse-kld", type=float, default=0.5, help="largest symmetrised KL divergence of a fused pair")
    ap.add_argument("--fuse-color", type=float, default=float("inf"), help="largest L2 distance of the DC colours of a fused pair")
    from gaussiansplattingregistration_amd.clean import add_clean_arguments, add_prune_arguments, clean_params_from_args, prune_unseen_from_args
    add_clean_arguments(ap)
    add_prune_arguments(ap)
    from gaussiansplattingregistration_amd.harmonize import add_match_colors_arguments, match_colors_from_args
    add_match_colors_arguments(ap)
    from gaussiansplattingregistration_amd.photo import add_photo_arguments, photo_params_from_args
    add_photo_arguments(ap)
    ap.add_argument("--nonrigid", type=float, metavar="MAX_CORR", help="non-rigid refinement behind the registration (and behind --photo-refine): a "
                    "lattice warp of the first scene that absorbs the smooth drift one matrix leaves; correspondences within this distance")
    ap.add_argument("--nonrigid-levels", type=int, default=3, help="lattices of 2^l + 1 nodes per axis, l = 0 .. levels - 1 (default 3: 2^3, 3^3, 5^3)")
    ap.add_argument("--nonrigid-smooth", type=float, default=0.01, metavar="LAMBDA", help="weight of the second differences of the node displacements")
    ap.add_argument("--warp-out", metavar="FIELD.npz", help="write the fitted field (evaluate_registration.py --warp reads it)")
    ap.add_argument("--mixture-refine", type=float, metavar="MAX_CORR", help="mixture-to-mixture refinement after ICP (and before --photo-refine): "
                    "every pair of splats within this distance counts, weighted by the overlap of the two Gaussians")
    ap.add_argument("--mixture-cov-scale", type=float, default=1.0, metavar="S", help="the covariances of a pair are multiplied by S^2")
    ap.add_argument("--mixture-cov-floor", type=float, default=0.0, metavar="F", help="added to the diagonal of a pair's summed covariance")
    ap.add_argument("--finetune", metavar="CAMERAS.json", help="fine-tune the merged cloud against photographs (with --out and --finetune-images): a "
                    "short Adam run through the differentiable rasteriser, after the merge and before the save; cameras in the merged cloud's frame")
    ap.add_argument("--finetune-images", metavar="DIR", help="directory of <img_name>.png, one per camera of --finetune")
    ap.add_argument("--finetune-iters", type=int, default=200, metavar="N")
    ap.add_argument("--finetune-params", default="dc,sh_rest,opacity", help="comma-separated, of dc, sh_rest, opacity, xyz, scaling, rotation (the last two tune the shape of "
                    "the splats: the saved file holds the tuned scales and quaternions, DESIGN.md 31)")
    ap.add_argument("--finetune-loss", choices=("l2", "l1", "l1_dssim"), default="l2", help="l1_dssim: (1 - lambda) L1 + lambda (1 - SSIM), the fused loss kernel")
    ap.add_argument("--finetune-lambda", type=float, default=0.2, metavar="L", help="the weight of the SSIM term of --finetune-loss l1_dssim")
    a = ap.parse_args()
    if a.finetune and not (a.out and a.finetune_images):
        raise SystemExit("--finetune needs --out and --finetune-images")
    if a.global_sc2 and a.with_scaling:
        raise SystemExit("--global-sc2 compares lengths of the two clouds and estimates a rigid motion: refused with --with-scaling "
                         "(--global-ransac is the scaled global method)")
    if a.mixture_refine is not None and a.with_scaling:
        raise SystemExit("--mixture-refine estimates a rigid motion: refused with --with-scaling")
    clean = clean_params_from_args(a)
    photo = photo_params_from_args(a)
    if photo is not None and a.with_scaling:
        raise SystemExit("--photo-refine estimates a rigid motion: refused with --with-scaling")
    if a.fuse_overlap is not None or a.match_colors is not None:
        a.rotate_sh = True
    if a.with_scaling and a.type not in (None, "point"):
        raise SystemExit(f"--with-scaling is point-to-point only (Open3D offers scaling for no other estimator): --type {a.type} refused")
    a.type = a.type or ("point" if a.with_scaling else "plane")

    import __graft_entry__ as g
    g.build_hip()
    from gaussiansplattingregistration_amd import mixture_bind
    from gaussiansplattingregistration_amd.controllers.downsampler_controller import DownsamplerController
    from gaussiansplattingregistration_amd.controllers.registration_controller import RegistrationController
    from gaussiansplattingregistration_amd.models.data_repository import DataRepository, UIStateRepository
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.params import GaussianMixtureParams
    from gaussiansplattingregistration_amd.utils.local_registration_util import KernelLossFunctionType as K, LocalRegistrationType as T
    from gaussiansplattingregistration_amd.utils.point_cloud_converter import convert_gs_to_open3d_pc

    rtype = {"point": T.ICP_Point_To_Point, "plane": T.ICP_Point_To_Plane, "color": T.ICP_Color, "general": T.ICP_General}[a.type]
    loss = {"none": K.Loss_None, "tukey": K.Tukey_Loss, "cauchy": K.Cauchy_Loss, "gm": K.GMLoss, "huber": K.Huber_Loss}[a.loss]
    repo, ui = DataRepository(), UIStateRepository()
    t0 = time.perf_counter()
    for path, gl, ol in ((a.first, repo.pc_gaussian_list_first, repo.pc_open3d_list_first),
                         (a.second, repo.pc_gaussian_list_second, repo.pc_open3d_list_second)):
        tm = {}
        gm = GaussianModel("cuda:0").from_ply(path, timing=tm)        # pinned chunks -> HBM -> device SoA (utils/ply_io.load_gaussian_device)
        print(f"{path}: {len(gm)} splats, SH degree {gm.sh_degree}; file -> device arrays {tm['seconds'] * 1e3:.1f} ms "
              f"({tm['bytes'] / tm['seconds'] / 1e9:.2f} GB/s of file bytes)")
        if clean is not None:
            gm, info = gm.remove_floaters(clean)
            print(f"{path}: cleaned {info['n']} -> {info['n_kept']} splats")
        gl.append(gm)
        ol.append(convert_gs_to_open3d_pc(gm))
    t1 = time.perf_counter()
    if not a.voxel:
        if len(a.max_corr) != a.levels + 1 or len(a.iters) != a.levels + 1:
            raise SystemExit("--max-corr and --iters need levels + 1 values (coarsest first)")
        mixture_bind.reset_rng()
        rho, delta, kappa, tau = a.hem
        DownsamplerController(repo).create_mixture(GaussianMixtureParams(hem_reduction=rho, distance_delta=delta, color_delta=kappa,
                                                                         decay_rate=tau, cluster_level=a.levels))
        print("levels:", [len(x) for x in repo.pc_gaussian_list_first], "/", [len(x) for x in repo.pc_gaussian_list_second])
    t2 = time.perf_counter()
    rc = RegistrationController(repo, ui)
    if a.with_scaling and not (a.global_ransac or a.global_fgr):
        from gaussiansplattingregistration_amd.utils.similarity_util import initial_similarity, split_similarity
        ui.transformation_matrix = initial_similarity(repo.pc_gaussian_list_first[0].get_xyz, repo.pc_gaussian_list_second[0].get_xyz)
        print(f"initial similarity: scale {split_similarity(ui.transformation_matrix)[0]:.6f}")
    if a.global_ransac:
        from gaussiansplattingregistration_amd.params.registration_parameters import RANSACRegistrationParams
        from gaussiansplattingregistration_amd.utils import global_registration_util as G
        v = a.global_ransac
        gp = RANSACRegistrationParams(voxel_size=v, max_correspondence=1.5 * v, max_iteration=a.ransac_iters, confidence=0.999,
                                      checkers=[G.CorrespondenceCheckerBasedOnEdgeLength(0.9), G.CorrespondenceCheckerBasedOnDistance(1.5 * v)])
        gp.orient_normals = a.orient_normals                          # read by do_ransac_registration; not a field of the reference's record
        tg = time.perf_counter()
        g = rc.execute_ransac_registration_normal(gp)
        print(f"global RANSAC: fitness {g.fitness:.4f}  rmse {g.inlier_rmse:.6f}  hypotheses {g.info.get('n_evaluated')}  "
              f"{time.perf_counter() - tg:.3f} s")
    if a.global_fgr:
        from gaussiansplattingregistration_amd.params.registration_parameters import FGRRegistrationParams
        v = a.global_fgr
        tg = time.perf_counter()
        fp = FGRRegistrationParams(voxel_size=v, maximum_correspondence=1.5 * v)
        fp.orient_normals = a.orient_normals
        g = rc.execute_fgr_registration_normal(fp)
        print(f"global FGR: fitness {g.fitness:.4f}  rmse {g.inlier_rmse:.6f}  reciprocal pairs {g.info.get('n_reciprocal')}  "
              f"tuples {g.info.get('n_tuples')} of {g.info.get('n_trials')} trials  {time.perf_counter() - tg:.3f} s")
    if a.global_sc2:
        from gaussiansplattingregistration_amd.params.registration_parameters import SC2RegistrationParams
        v = a.global_sc2
        tg = time.perf_counter()
        sp = SC2RegistrationParams(voxel_size=v, max_correspondence=1.5 * v)
        sp.orient_normals = a.orient_normals
        g = rc.execute_sc2_registration_normal(sp)
        print(f"global SC2: fitness {g.fitness:.4f}  rmse {g.inlier_rmse:.6f}  correspondences {g.info.get('n_corres')}  "
              f"seeds {g.info.get('n_valid')} valid of {g.info.get('n_seeds')}  edges {g.info.get('n_edges')}  "
              f"refinement steps {g.info.get('refine_steps')}  {time.perf_counter() - tg:.3f} s")
    res = rc.execute_multiscale_registration(False, "", "", rtype, 1e-6, 1e-6, a.max_corr, a.iters, loss, a.k, not a.voxel, with_scaling=a.with_scaling)
    t3 = time.perf_counter()
    if res is None:
        raise SystemExit("registration failed: " + "; ".join(rc.errors))
    np.set_printoptions(precision=6, suppress=True)
    print("transformation (first -> second):\n", res.result.transformation)
    if a.with_scaling:
        from gaussiansplattingregistration_amd.utils.similarity_util import split_similarity
        print(f"scale {split_similarity(res.result.transformation)[0]:.9f}")
    print(f"fitness {res.result.fitness:.4f}  inlier RMSE {res.result.inlier_rmse:.6f}")
    print(f"load {t1 - t0:.2f} s, mixtures {t2 - t1:.3f} s, registration {t3 - t2:.3f} s")
    T_final = res.result.transformation
    if a.mixture_refine is not None:
        from gaussiansplattingregistration_amd.params import MixtureRegistrationParams
        from gaussiansplattingregistration_amd.utils.local_registration_util import do_mixture_registration
        tm0 = time.perf_counter()
        mr = do_mixture_registration(repo.pc_open3d_list_first[0], repo.pc_open3d_list_second[0], T_final,
                                     MixtureRegistrationParams(max_correspondence=a.mixture_refine, cov_scale=a.mixture_cov_scale, cov_floor=a.mixture_cov_floor))
        T_final = ui.transformation_matrix = mr.transformation
        print(f"mixture-to-mixture refinement: score {mr.score:.6g}  fitness {mr.fitness:.4f}  Mahalanobis rmse {mr.mahalanobis_rmse:.6f}  "
              f"{mr.iterations} iterations ({mr.status}), {mr.n_pairs} pairs, {mr.n_singular} singular  {time.perf_counter() - tm0:.3f} s")
        print("transformation after the mixture-to-mixture refinement (first -> second):\n", T_final)
    if photo is not None:
        from gaussiansplattingregistration_amd.models.camera import load_cameras
        from gaussiansplattingregistration_amd.photo import report_lines
        repo.current_index = 0                                        # the original clouds
        pr = rc.refine_photometric(load_cameras(a.photo_refine), photo)
        T_final = pr.transformation
        print("photometric refinement:")
        print("\n".join("  " + line for line in report_lines(pr)))
        print("transformation after the photometric refinement (first -> second):\n", T_final)
        print(f"photometric refinement {time.perf_counter() - t3:.3f} s")
    field = None
    if a.nonrigid is not None:
        from gaussiansplattingregistration_amd.params import WarpParams
        tw = time.perf_counter()
        repo.current_index = 0                                        # the finest clouds the script holds: the original ones
        ui.transformation_matrix = T_final
        wr = rc.refine_nonrigid(WarpParams(max_corr=a.nonrigid, levels=a.nonrigid_levels, lam=a.nonrigid_smooth))
        field = wr.field
        print(f"non-rigid refinement: point-to-plane RMSE {wr.rmse_before:.6f} without the warp, {wr.rmse_after:.6f} with it "
              f"({wr.n_corr} correspondences, {wr.n_folded} folded points)")
        for lv in wr.levels:
            print(f"  lattice {'x'.join(str(d) for d in lv['dims'])}: " + ", ".join(f"{it['rmse']:.6f}" for it in lv["iterations"]))
        print(f"non-rigid refinement {time.perf_counter() - tw:.3f} s (accumulate {wr.timings['accumulate']:.3f} s, solve {wr.timings['solve']:.3f} s)")
        if a.warp_out:
            field.save(a.warp_out)
            print(f"warp field -> {a.warp_out}")
    if a.out:
        from gaussiansplattingregistration_amd import harmonize
        from gaussiansplattingregistration_amd.params import FuseOverlapParams
        fuse = FuseOverlapParams(a.fuse_overlap, a.fuse_kld, a.fuse_color) if a.fuse_overlap is not None else None
        first, second, T = repo.pc_gaussian_list_first[0], repo.pc_gaussian_list_second[0], T_final
        cm, gate = match_colors_from_args(a, fuse)
        if cm is not None:          # move, fit the first scene's colours against the second's, apply: what is merged below is already in place
            first, (transforms, cinfo) = GaussianModel.move_and_match_colors(first, second, T, a.rotate_sh, a.with_scaling, cm, gate, warp=field)
            T, field = None, None
            print("colours (scene 0 = first, scene 1 = second, the reference):")
            print("\n".join("  " + line for line in harmonize.report_lines(transforms, cinfo)))
            if a.colors_out:
                harmonize.write_json(a.colors_out, transforms, cinfo)
        if fuse is not None:
            merged, info = GaussianModel.get_fused_gaussian_point_clouds(first, second, T, fuse, rotate_sh=a.rotate_sh, with_scaling=a.with_scaling, warp=field)
            print(f"fuse overlap: n_pairs {info['n_pairs']}  n_out {info['n_out']}  (invalid rows: {info['n_invalid_a']} / {info['n_invalid_b']})")
        else:
            merged = GaussianModel.get_merged_gaussian_point_clouds(first, second, T, rotate_sh=a.rotate_sh, with_scaling=a.with_scaling, warp=field)
        merged = prune_unseen_from_args(merged, a)          # (cameras in the frame of the merged cloud: the second / reference scene's)
        if a.finetune:
            from gaussiansplattingregistration_amd.finetune import FinetuneParams, ModelFinetuner
            from gaussiansplattingregistration_amd.models.camera import load_cameras
            tf = time.perf_counter()
            merged.move_to_device("cuda:0")
            fr = ModelFinetuner(merged, load_cameras(a.finetune), a.finetune_images,
                                FinetuneParams(iterations=a.finetune_iters, params=tuple(x for x in a.finetune_params.split(",") if x), loss=a.finetune_loss,
                                               lambda_dssim=a.finetune_lambda)).run()
            mean = lambda v: sum(v) / len(v) if v else float("nan")
            which = "loss" if a.finetune_loss == "l2" else f"{a.finetune_loss} loss (lambda {a.finetune_lambda:g})" if a.finetune_loss == "l1_dssim" else f"{a.finetune_loss} loss"
            print(f"fine-tuning ({a.finetune_params}): {fr.iterations} iterations over {len(fr.psnr_before)} cameras, {which} {fr.losses[0] if fr.losses else float('nan'):.6g} -> "
                  f"{fr.losses[-1] if fr.losses else float('nan'):.6g}, mean PSNR {mean(fr.psnr_before):.3f} -> {mean(fr.psnr_after):.3f} dB  {time.perf_counter() - tf:.3f} s")
            if fr.geometry_source:
                print(f"  scaling / rotation tuned from the {fr.geometry_source} factors of the covariances")
            for e in fr.error_list:
                print("  " + e)
        merged.save_ply(a.out)
        print(f"merged cloud ({len(merged)} splats) -> {a.out}")


if __name__ == "__main__":
    main()
