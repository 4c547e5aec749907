#!/usr/bin/env python3
"""Headless multiway registration of N 3DGS .ply scenes on one MI355X: pairwise ICP per edge, the information matrix of every
registered pair, a pose graph with a line process that prunes wrongly registered pairs, and the merged cloud.

    python scripts/register_many.py a.ply b.ply c.ply ... --out merged.ply [--poses-out poses.json]
           [--edges sequential|all] [--edge S T ...] [--global-fgr VOXEL | --global-ransac VOXEL | --global-sc2 VOXEL]
           [--type point|plane|color|general] [--loss none|tukey|cauchy|gm|huber --k 0.1] [--max-corr 0.05] [--iters 30]
           [--prune 0.25] [--preference 1.0] [--reference 0] [--rotate-sh]
           [--clean-knn K --clean-std R [--clean-radius R --clean-nb N] [--clean-min-opacity A] [--clean-max-extent S]]
           [--prune-unseen CAMERAS.json ... [--min-contribution 0.01]]
           [--fuse-overlap MAX_DIST [--fuse-kld 0.5] [--fuse-color X]]
           [--match-colors [gain|channel_gain|affine] [--match-colors-huber K] [--match-colors-dist D] [--colors-out colors.json]]

Edges: `--edges sequential` registers each scene to the next (a chain), `--edges all` every pair; `--edge S T` (repeatable) adds the pair
(S, T).  An edge (i, i + 1) is certain ("odometry"); every other edge is a loop closure the optimiser may prune (`--prune`: the line
process value below which it does).  Without a global method every pair starts from the identity: the scenes must be roughly aligned.
The poses map each scene into the frame of scene `--reference`; `--poses-out` holds them with the edges, their line process values
and the pruned edges.  `--clean-*`: every scene goes through floater removal right after loading (scripts/clean_ply.py has the stages);
prints n -> n_kept per scene.  `--fuse-overlap MAX_DIST`: the merged cloud stores a surface that k scenes share once
(GaussianModel.fuse_overlap_multi: groups of at most one splat per scene, moment-matched); it implies --rotate-sh and prints n_groups, the
histogram of the group sizes and n_out.  `--match-colors [MODE]`: the scenes differ in exposure or white balance; after the move every
scene's colour transform (a gain, a gain per channel or an affine 3 x 4) is fitted jointly against scene `--reference` over the splats
each pair of scenes shares (GaussianModel.match_colors; matches within `--match-colors-dist`, default the fuse distance, else --max-corr)
and applied before the merge.  Prints the transform per scene and the colour residual per pair before and after; `--colors-out` writes
them as JSON.  Implies --rotate-sh.  `--prune-unseen CAMERAS.json` (repeatable): the merged cloud loses the splats no camera shows with a
blending weight of `--min-contribution` (GaussianModel.prune_unseen); the cameras must be in the frame of scene `--reference` and cover ALL
the scenes, since a splat outside every frustum is dropped like an occluded one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scenes", nargs="+")
    ap.add_argument("--out", help="the merged cloud (.ply)")
    ap.add_argument("--poses-out", help="poses, edges with their line process values and the pruned edges (.json)")
    ap.add_argument("--edges", choices=["sequential", "all"], default=None, help="default: sequential (nothing when --edge is given)")
    ap.add_argument("--edge", type=int, nargs=2, action="append", default=[], metavar=("S", "T"))
    method = ap.add_mutually_exclusive_group()
    method.add_argument("--global-fgr", type=float, metavar="VOXEL", help="initial transform of every pair by Fast Global Registration at this voxel size")
    method.add_argument("--global-ransac", type=float, metavar="VOXEL", help="initial transform of every pair by FPFH + RANSAC at this voxel size")
    method.add_argument("--global-sc2", type=float, metavar="VOXEL", help="initial transform of every pair by the compatibility-graph method at this voxel "
                        "size (deterministic, no sampling)")
    ap.add_argument("--ransac-iters", type=int, default=100000)
    ap.add_argument("--type", choices=["point", "plane", "color", "general"], default="plane")
    ap.add_argument("--loss", choices=["none", "tukey", "cauchy", "gm", "huber"], default="none")
    ap.add_argument("--k", type=float, default=0.0)
    ap.add_argument("--max-corr", type=float, default=0.075, help="correspondence distance of the ICP, of the information matrices and of the optimiser")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--prune", type=float, default=0.25, help="edge_prune_threshold")
    ap.add_argument("--preference", type=float, default=1.0, help="preference_loop_closure")
    ap.add_argument("--reference", type=int, default=0, help="reference_node: the scene whose frame the result is in")
    ap.add_argument("--rotate-sh", action="store_true", help="turn the SH coefficients of every moved scene with it in the merged output")
    ap.add_argument("--fuse-overlap", type=float, metavar="MAX_DIST", help="fuse the splats the scenes share (within this distance) in the merged output; implies --rotate-sh")
    ap.add_argument("--fuse-kld", type=float, default=0.5, help="symmetrised KL gate of --fuse-overlap")
    ap.add_argument("--fuse-color", type=float, default=float("inf"), help="DC colour gate of --fuse-overlap (default: none)")
    from gaussiansplattingregistration_amd.clean import add_clean_arguments, add_prune_arguments, clean_params_from_args, prune_unseen_from_args
    add_clean_arguments(ap)
    add_prune_arguments(ap)
    from gaussiansplattingregistration_amd.harmonize import add_match_colors_arguments, match_colors_from_args
    add_match_colors_arguments(ap)
    a = ap.parse_args()
    clean = clean_params_from_args(a)
    n = len(a.scenes)
    if n < 2:
        raise SystemExit("at least two scenes")

    import __graft_entry__ as g
    g.build_hip()
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    from gaussiansplattingregistration_amd.params.registration_parameters import (FGRRegistrationParams, LocalRegistrationParams,
                                                                                  RANSACRegistrationParams, SC2RegistrationParams)
    from gaussiansplattingregistration_amd.utils import global_registration_util as G
    from gaussiansplattingregistration_amd.utils.local_registration_util import KernelLossFunctionType as K, LocalRegistrationType as T
    from gaussiansplattingregistration_amd.utils.point_cloud_converter import convert_gs_to_open3d_pc
    from gaussiansplattingregistration_amd.utils.pose_graph import GlobalOptimizationOption
    from gaussiansplattingregistration_amd.workers.multiway import MultiwayRegistrator, edge_list

    edges = edge_list(n, a.edges or ("sequential" if not a.edge else []))
    for s, t in edge_list(n, a.edge):
        if (s, t) not in edges:
            edges.append((s, t))
    rtype = {"point": T.ICP_Point_To_Point, "plane": T.ICP_Point_To_Plane, "color": T.ICP_Color, "general": T.ICP_General}[a.type]
    loss = {"none": K.Loss_None, "tukey": K.Tukey_Loss, "cauchy": K.Cauchy_Loss, "gm": K.GMLoss, "huber": K.Huber_Loss}[a.loss]
    t0 = time.perf_counter()
    models = [GaussianModel("cuda:0").from_ply(p) for p in a.scenes]
    if clean is not None:
        for i, p in enumerate(a.scenes):
            models[i], info = models[i].remove_floaters(clean)
            print(f"{p}: cleaned {info['n']} -> {info['n_kept']} splats")
    clouds = [convert_gs_to_open3d_pc(m) for m in models]
    for p, m in zip(a.scenes, models):
        print(f"{p}: {len(m)} splats, SH degree {m.sh_degree}")
    t1 = time.perf_counter()

    init = None
    if a.global_fgr:
        gp = FGRRegistrationParams(voxel_size=a.global_fgr, maximum_correspondence=1.5 * a.global_fgr)
        init = lambda s, t, cs, ct: G.do_fgr_registration(cs, ct, gp).transformation
    elif a.global_sc2:
        gp = SC2RegistrationParams(voxel_size=a.global_sc2, max_correspondence=1.5 * a.global_sc2)
        init = lambda s, t, cs, ct: G.do_sc2_registration(cs, ct, gp).transformation
    elif a.global_ransac:
        v = a.global_ransac
        gp = RANSACRegistrationParams(voxel_size=v, max_correspondence=1.5 * v, max_iteration=a.ransac_iters, confidence=0.999,
                                      checkers=[G.CorrespondenceCheckerBasedOnEdgeLength(0.9), G.CorrespondenceCheckerBasedOnDistance(1.5 * v)])
        init = lambda s, t, cs, ct: G.do_ransac_registration(cs, ct, gp).transformation
    params = LocalRegistrationParams(registration_type=rtype, max_correspondence=a.max_corr, max_iteration=a.iters, rejection_type=loss, k_value=a.k)
    option = GlobalOptimizationOption(max_correspondence_distance=a.max_corr, edge_prune_threshold=a.prune, preference_loop_closure=a.preference,
                                      reference_node=a.reference)
    fuse = None
    if a.fuse_overlap is not None:
        from gaussiansplattingregistration_amd.params import FuseOverlapParams
        fuse = FuseOverlapParams(a.fuse_overlap, a.fuse_kld, a.fuse_color)
    cm, gate = match_colors_from_args(a, fuse, default_distance=a.max_corr)
    worker = MultiwayRegistrator(clouds, params, edges=edges, init=init, option=option, fuse=fuse, match_colors=cm, match_colors_gate=gate)
    res = worker.run()
    t2 = time.perf_counter()
    if res is None:
        raise SystemExit("multiway registration failed: " + "; ".join(worker.errors))
    np.set_printoptions(precision=6, suppress=True)
    for r in res.edge_reports:
        print(f"edge ({r['source']}, {r['target']}){' loop' if r['uncertain'] else ''}: fitness {r['fitness']:.4f}  rmse {r['inlier_rmse']:.6f}  "
              f"correspondences {r['n_correspondences']}  l {r['line_process']:.4f}{'  PRUNED' if r['pruned'] else ''}")
    print(res.optimization)
    for i, X in enumerate(res.poses):
        print(f"pose of scene {i} (-> scene {a.reference}):\n", X)
    print(f"load {t1 - t0:.2f} s, registration {t2 - t1:.3f} s (pairwise {worker.timing['pairwise_s']:.3f}, information "
          f"{worker.timing['information_s']:.3f}, optimisation {worker.timing['optimization_s']:.3f})")
    if a.poses_out:
        doc = {"reference_node": a.reference, "poses": [X.tolist() for X in res.poses],
               "edges": [{"source": r["source"], "target": r["target"], "uncertain": r["uncertain"], "transformation": np.asarray(r["transformation"]).tolist(),
                          "fitness": r["fitness"], "inlier_rmse": r["inlier_rmse"], "n_correspondences": r["n_correspondences"],
                          "line_process": r["line_process"], "pruned": r["pruned"]} for r in res.edge_reports],
               "pruned": [[r["source"], r["target"]] for r in res.edge_reports if r["pruned"]],
               "optimization": {"iterations": list(res.optimization.iterations), "E_initial": res.optimization.E_initial, "E_final": res.optimization.E_final,
                                "mu": res.optimization.mu, "n_pruned": res.optimization.n_pruned}}
        with open(a.poses_out, "w") as f:
            json.dump(doc, f, indent=1)
        print(f"poses -> {a.poses_out}")
    if a.out:
        merged = worker.merge(models, res, rotate_sh=a.rotate_sh or fuse is not None or cm is not None)
        if cm is not None:          # every scene's colours were fitted jointly against the reference scene's and applied before the merge
            from gaussiansplattingregistration_amd import harmonize
            transforms, cinfo = worker.color_info
            print("colours:")
            print("\n".join("  " + line for line in harmonize.report_lines(transforms, cinfo)))
            if a.colors_out:
                harmonize.write_json(a.colors_out, transforms, cinfo)
        if fuse is not None:
            info = worker.fuse_info
            sizes = "  ".join(f"{k}: {c}" for k, c in enumerate(info["groups_of_size"]) if c)
            print(f"fuse: n_groups {info['n_groups']}  sizes {{{sizes}}}  n_grouped_rows {info['n_grouped_rows']}  rejected_edges {info['rejected_edges']}  "
                  f"rounds {info['rounds']}  n_out {info['n_out']}")
        merged = prune_unseen_from_args(merged, a)          # (cameras in the frame of the merged cloud: the second / reference scene's)
        merged.save_ply(a.out)
        print(f"merged cloud ({len(merged)} splats) -> {a.out}")


if __name__ == "__main__":
    main()
