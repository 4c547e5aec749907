#!/usr/bin/env python3
"""Floater removal of one 3DGS .ply scene on one MI355X (`GaussianModel.remove_floaters`: `gsr_outlier_mask` + `gsr_model_select`).

    python scripts/clean_ply.py in.ply --out out.ply --clean-knn K --clean-std R [--clean-radius R --clean-nb N]
           [--clean-min-opacity A] [--clean-max-extent S] [--prune-unseen CAMERAS.json ... [--min-contribution 0.01]]

Stages, in this order, each over the survivors of the one before: rows with a non-finite coordinate; `--clean-min-opacity` (activated
opacity below A); `--clean-max-extent` (largest scale above S); the statistical filter (Open3D `remove_statistical_outlier(K, R)`);
the radius filter (Open3D `remove_radius_outlier(N, R)`).  The kept rows are written bit for bit.  Prints `n -> n_kept` and what each
stage dropped.

`--prune-unseen CAMERAS.json` (may be repeated; alone or after the stages above): `GaussianModel.prune_unseen` drops the splats whose
largest blending weight over all the cameras of the given files stays below `--min-contribution`.  A splat outside every frustum goes
like an occluded one: give the cameras of every scene the file was merged from.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from gaussiansplattingregistration_amd.clean import add_clean_arguments, add_prune_arguments, clean_params_from_args, prune_unseen_from_args
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("--out", required=True)
    add_clean_arguments(ap)
    add_prune_arguments(ap)
    a = ap.parse_args()
    params = clean_params_from_args(a)
    if params is None and not a.prune_unseen:
        raise SystemExit("no cleaning flag given: nothing to do")

    import __graft_entry__ as g
    g.build_hip()
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    model = GaussianModel("cuda:0").from_ply(a.scene)
    cleaned = model
    if params is not None:
        cleaned, info = model.remove_floaters(params)
        print(f"{a.scene}: {info['n']} -> {info['n_kept']} splats (non-finite {info['n_nonfinite']}, opacity {info['n_gate_opacity']}, "
              f"extent {info['n_gate_scale']}, statistical {info['n_statistical']}, radius {info['n_radius']}; threshold {info['threshold']:.6g}, "
              f"deferred queries {info['deferred_queries']})")
    cleaned = prune_unseen_from_args(cleaned, a)
    cleaned.save_ply(a.out)
    print(f"-> {a.out}")


if __name__ == "__main__":
    main()
