"""Headless ``RegistrationController`` (reference ``src/controllers/registration_controller.py:24-28,47-91,93-120,145-163``)."""
from __future__ import annotations

import numpy as np

from ..workers.registrators import (FGRRegistrator, LocalRegistrator, MultiScaleRegistratorMixture, MultiScaleRegistratorVoxel,
                                    RANSACRegistrator, SC2Registrator)


class RegistrationController:
    def __init__(self, data_repository, ui_repository):
        self.data_repository = data_repository
        self.ui_repository = ui_repository
        self.errors = []

    def execute_local_registration_normal(self, params, with_scaling=False):
        repo = self.data_repository
        pc1 = repo.pc_open3d_list_first[repo.current_index]
        pc2 = repo.pc_open3d_list_second[repo.current_index]
        worker = LocalRegistrator(pc1, pc2, self.ui_repository.transformation_matrix, params, with_scaling=with_scaling)
        result = worker.run()
        self.handle_registration_result_local(result)
        return result

    def execute_ransac_registration_normal(self, params):       # :47-52, 61-68
        repo = self.data_repository
        pc1 = repo.pc_open3d_list_first[repo.current_index]
        pc2 = repo.pc_open3d_list_second[repo.current_index]
        worker = RANSACRegistrator(pc1, pc2, self.ui_repository.transformation_matrix, params)
        result = worker.run()
        self.handle_registration_result_global(result)
        return result

    def execute_fgr_registration_normal(self, params):          # :70-74, 84-91
        repo = self.data_repository
        pc1 = repo.pc_open3d_list_first[repo.current_index]
        pc2 = repo.pc_open3d_list_second[repo.current_index]
        worker = FGRRegistrator(pc1, pc2, self.ui_repository.transformation_matrix, params)
        result = worker.run()
        self.handle_registration_result_global(result)
        return result

    execute_fgr_registration = execute_fgr_registration_normal

    def execute_sc2_registration_normal(self, params):          # the compatibility-graph method, handled like the two above
        repo = self.data_repository
        pc1 = repo.pc_open3d_list_first[repo.current_index]
        pc2 = repo.pc_open3d_list_second[repo.current_index]
        worker = SC2Registrator(pc1, pc2, self.ui_repository.transformation_matrix, params)
        result = worker.run()
        self.handle_registration_result_global(result)
        return result

    execute_sc2_registration = execute_sc2_registration_normal

    def execute_multiscale_registration(self, use_corresponding, sparse_first, sparse_second, registration_type,
                                        relative_fitness, relative_rmse, voxel_values, iter_values, rejection_type, k_value,
                                        use_mixture=True, with_scaling=False):
        repo = self.data_repository
        if use_mixture:
            worker = MultiScaleRegistratorMixture(repo.pc_open3d_list_first, repo.pc_open3d_list_second,
                                                  self.ui_repository.transformation_matrix, use_corresponding, sparse_first,
                                                  sparse_second, registration_type, relative_fitness, relative_rmse,
                                                  voxel_values, iter_values, rejection_type, k_value, with_scaling=with_scaling)
        else:
            # the original clouds (the reference indexes the second list with [1], registration_controller.py:108 --
            # an IndexError without mixtures and the wrong cloud with them; the original cloud [0] is what is meant)
            worker = MultiScaleRegistratorVoxel(repo.pc_open3d_list_first[0], repo.pc_open3d_list_second[0],
                                                self.ui_repository.transformation_matrix, use_corresponding, sparse_first,
                                                sparse_second, registration_type, relative_fitness, relative_rmse,
                                                voxel_values, iter_values, rejection_type, k_value, with_scaling=with_scaling)
        result = worker.run()
        self.errors = worker.errors
        if result is not None:
            self.handle_registration_result_local(result)
        return result

    def execute_multiway_registration(self, clouds, params, edges="sequential", init=None, option=None, criteria=None, match_colors=None,
                                      match_colors_gate=None):
        """N clouds into one frame (``workers/multiway.py``): pairwise ICP per edge, information matrices, pose-graph optimisation.
        The repository holds two clouds, so the N ``PointCloud`` records are arguments.  Returns the worker's ``ResultData`` (poses,
        graph, per-edge report) or ``None`` with ``self.errors`` set; the pairwise ``transformation_matrix`` is left alone."""
        from ..workers.multiway import MultiwayRegistrator
        worker = MultiwayRegistrator(clouds, params, edges=edges, init=init, option=option, criteria=criteria, match_colors=match_colors,
                                     match_colors_gate=match_colors_gate)
        result = worker.run()
        self.errors = worker.errors
        self.multiway_worker = worker       # its merge() carries match_colors
        return result

    @staticmethod
    def merge_multiway(models, poses, rotate_sh=False, match_colors=None, match_colors_gate=None):
        """The N ``GaussianModel`` s moved by their poses into one model (``GaussianModel.get_merged_gaussian_point_clouds_multi``;
        ``get_merged_gaussian_point_clouds_multi_colors``);
        ``match_colors`` (``ColorMatchParams``) with its gate harmonises their colours on the way."""
        from ..models.gaussian_model import GaussianModel
        return GaussianModel.get_merged_gaussian_point_clouds_multi_colors(models, poses, match_colors, match_colors_gate, rotate_sh=rotate_sh)

    def evaluate_registration(self, cameras_list, images_path, log_path, color, use_gpu, registration_result=None, rotate_sh=False, with_scaling=False,
                              fuse=None, match_colors=None, match_colors_gate=None, warp=None):
        """``warp`` (``warp.WarpField``): the first cloud is warped between the move and the merge (``refine_nonrigid``).
        ``match_colors`` (``ColorMatchParams``; its gate: ``fuse``, else ``match_colors_gate``): the merge harmonises the first cloud's colours with the second's.
        ``with_scaling``: the current transform is a similarity (a registration with scaling); the merge before rendering applies it as one.
        ``fuse`` (``FuseOverlapParams``): the merge fuses the splats the two clouds share (``GaussianModel.fuse_overlap``).
        Image-based evaluation of the current transform on the repository's original clouds (reference :122-143): renders of
        the merged model against the photographs, the JSON log at ``log_path``.  Returns the evaluator's ``EvaluationObject``."""
        from ..workers.evaluator import RegistrationEvaluator
        repo = self.data_repository
        pc1 = repo.pc_gaussian_list_first[repo.current_index]
        pc2 = repo.pc_gaussian_list_second[repo.current_index]
        worker = RegistrationEvaluator(pc1, pc2, self.ui_repository.transformation_matrix, cameras_list, images_path, log_path, color,
                                       registration_result, use_gpu, rotate_sh=rotate_sh, with_scaling=with_scaling, fuse=fuse, match_colors=match_colors,
                                       match_colors_gate=match_colors_gate, warp=warp)
        return worker.run()

    def evaluate_geometry(self, cameras_list, log_path, coverage=0.5, registration_result=None, rotate_sh=False, with_scaling=False, warp=None):
        """Geometric evaluation of the current transform on the repository's original clouds, without photographs: the depth maps of
        the first cloud moved by it and of the second, from the same cameras (``GeometryEvaluator``); the JSON log at ``log_path``.
        Returns the evaluator's ``GeometryEvaluationObject``."""
        from ..workers.evaluator import GeometryEvaluator
        repo = self.data_repository
        pc1 = repo.pc_gaussian_list_first[repo.current_index]
        pc2 = repo.pc_gaussian_list_second[repo.current_index]
        worker = GeometryEvaluator(pc1, pc2, self.ui_repository.transformation_matrix, cameras_list, log_path, with_scaling=with_scaling,
                                   rotate_sh=rotate_sh, coverage=coverage, registration_result=registration_result, warp=warp)
        return worker.run()

    def refine_photometric(self, cameras_list, params, device=0):
        """Render-based refinement of the current transform on the repository's original clouds (``photo.PhotometricRefiner``,
        DESIGN.md 23): both scenes rendered from ``cameras_list`` (in the second cloud's frame), intensity + depth, damped Gauss-Newton.
        ``params``: ``PhotometricParams`` (``max_depth_diff`` has no default).  The refined transform becomes the current one; returns
        the ``PhotometricResult`` (``None`` when cancelled: the transform is left alone).  Rigid only: not for a similarity."""
        from ..photo import PhotometricRefiner
        repo = self.data_repository
        pc1 = repo.pc_gaussian_list_first[repo.current_index]
        pc2 = repo.pc_gaussian_list_second[repo.current_index]
        self.photometric_worker = worker = PhotometricRefiner(pc1, pc2, cameras_list, params, init=self.ui_repository.transformation_matrix, device=device)
        result = worker.run()
        if result is not None:
            self.errors = list(result.error_list)
            self.ui_repository.transformation_matrix = result.transformation
        return result

    def finetune_merged(self, cameras_list, images, params=None, rotate_sh=False, with_scaling=False, fuse=None, match_colors=None,
                        match_colors_gate=None, warp=None, device="cuda:0"):
        """Merges the repository's original clouds with the current transform (the arguments of the merge as in ``evaluate_registration``)
        and fine-tunes the merged model against photographs (``finetune.ModelFinetuner``).  ``images``: a directory of
        ``<image_name>.png`` or one ``(H, W, 3)`` image per camera; ``params``: ``FinetuneParams``, handed on as it is -- with ``"scaling"`` /
        ``"rotation"`` in ``params.params`` the shape of the splats is tuned too and the merged model comes back with a consistent
        ``_scaling`` / ``_rotation`` / ``_covariance`` triple that ``save_ply`` stores.  Returns ``(merged model, FinetuneResult)``
        (the result is ``None`` when cancelled: the merged model is then untouched); the model is kept in ``self.finetuned_model``."""
        from ..finetune import ModelFinetuner
        from ..models.gaussian_model import GaussianModel
        repo = self.data_repository
        pc1 = repo.pc_gaussian_list_first[repo.current_index]
        pc2 = repo.pc_gaussian_list_second[repo.current_index]
        merged = GaussianModel.get_merged_gaussian_point_clouds(pc1, pc2, self.ui_repository.transformation_matrix, rotate_sh=rotate_sh,
                                                                with_scaling=with_scaling, fuse=fuse, match_colors=match_colors,
                                                                match_colors_gate=match_colors_gate, warp=warp)
        merged.move_to_device(device)
        self.finetune_worker = worker = ModelFinetuner(merged, cameras_list, images, params)
        result = worker.run()
        self.finetuned_model = merged
        return merged, result

    def refine_nonrigid(self, params, device=None):
        """Non-rigid refinement behind the current transform (``warp.NonRigidRefiner``) on the repository's current
        clouds: the first cloud is moved by the current matrix (rigid or a similarity), then a lattice warp is fitted that brings it
        onto the second.  ``params``: ``WarpParams`` (``max_corr`` has no default).  The matrix is left alone; the field is kept in
        ``self.warp_field`` for the merges (``GaussianModel.get_merged_gaussian_point_clouds(..., warp=field)``).  Returns the
        ``WarpResult``."""
        from ..warp import NonRigidRefiner
        repo = self.data_repository
        pc1 = repo.pc_open3d_list_first[repo.current_index]
        pc2 = repo.pc_open3d_list_second[repo.current_index]
        self.nonrigid_worker = worker = NonRigidRefiner(pc1, pc2, params, init=self.ui_repository.transformation_matrix, device=device)
        result = worker.run()
        self.warp_field = result.field
        return result

    def execute_mixture_registration(self, max_corr_values, cov_scale_values, iter_values, cov_floor=0.0, relative_score=1e-6, levels=None):
        """Mixture-to-mixture registration (``MixtureToMixtureRegistrator``) from the current transform, coarse to fine
        over the repository's two lists of clouds (one value per entry: the coarsest level first), or over ``levels = (list1, list2)``
        -- e.g. the level dicts of ``hem.create_mixture``, which carry the components' weights.  The result's transform becomes the
        current one; returns the worker's ``ResultData`` or ``None`` with ``self.errors`` set.  Rigid only."""
        from ..workers.registrators import MixtureToMixtureRegistrator
        repo = self.data_repository
        l1, l2 = levels if levels is not None else (repo.pc_open3d_list_first, repo.pc_open3d_list_second)
        self.mixture_worker = worker = MixtureToMixtureRegistrator(l1, l2, self.ui_repository.transformation_matrix, max_corr_values, cov_scale_values,
                                                                   iter_values, cov_floor=cov_floor, relative_score=relative_score)
        result = worker.run()
        self.errors = worker.errors
        if result is not None:
            self.handle_registration_result_local(result)
        return result

    def handle_registration_result_local(self, result_data):       # :145-163
        self.ui_repository.transformation_matrix = result_data.result.transformation

    def handle_registration_result_global(self, results):      # :150-152
        self.ui_repository.transformation_matrix = np.dot(results.transformation, self.ui_repository.transformation_matrix)
