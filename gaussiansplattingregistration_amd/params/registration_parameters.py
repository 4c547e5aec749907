"""Registration parameters: field names and defaults of the reference's ``src/params/registration_parameters.py:7-40``."""
from dataclasses import dataclass, field
from typing import List

from ..utils.global_registration_util import RANSACEstimationMethod
from ..utils.local_registration_util import KernelLossFunctionType, LocalRegistrationType


@dataclass
class LocalRegistrationParams:
    registration_type: LocalRegistrationType = LocalRegistrationType.ICP_Point_To_Point
    max_correspondence: float = 5.0
    relative_fitness: float = 0.000001
    relative_rmse: float = 0.000001
    max_iteration: int = 30
    rejection_type: KernelLossFunctionType = KernelLossFunctionType.Loss_None
    k_value: float = 0.0


@dataclass
class MultiScaleRegistrationParams:
    """The argument list of ``signal_do_registration`` (``src/gui/tabs/multi_scale_registration_tab.py:13-15``)
    as one record; GUI defaults ``iter "50,30,20"`` / ``correspondences "5,2.5,2"`` (``:83,92``)."""
    use_corresponding: bool = False
    sparse_first: str = ""
    sparse_second: str = ""
    registration_type: LocalRegistrationType = LocalRegistrationType.ICP_Point_To_Point
    relative_fitness: float = 0.000001
    relative_rmse: float = 0.000001
    voxel_values: List[float] = field(default_factory=lambda: [5.0, 2.5, 2.0])
    iter_values: List[int] = field(default_factory=lambda: [50, 30, 20])
    rejection_type: KernelLossFunctionType = KernelLossFunctionType.Loss_None
    k_value: float = 0.0
    use_mixture: bool = True


@dataclass
class MixtureRegistrationParams:
    """Mixture-to-mixture registration (``d2d.D2DContext``); the reference has no such method.
    ``max_correspondence`` has no default: scenes have no common unit of length."""
    max_correspondence: float           # a pair of components counts when its squared centre distance is strictly below this, squared
    cov_scale: float = 1.0              # the summed covariance of a pair is multiplied by cov_scale^2 (coarse-to-fine: 8, 4, 2, 1)
    cov_floor: float = 0.0              # added to the diagonal of a pair's covariance (keeps flat-on-flat pairs invertible)
    max_iteration: int = 30
    relative_score: float = 1e-6        # stop when the score changes by no more than this, relatively


@dataclass
class RANSACRegistrationParams:
    """The reference's fields and defaults, plus ``seed``: the RANSAC sampler is counter-based and deterministic here."""
    voxel_size: float = 0.05
    mutual_filter: bool = False
    max_correspondence: float = 5.0
    estimation_method: RANSACEstimationMethod = RANSACEstimationMethod.TransformationEstimationPointToPoint
    ransac_n: int = 3
    checkers: list = field(default_factory=list)
    max_iteration: int = 100000
    confidence: float = 0.999
    seed: int = 0


@dataclass
class FGRRegistrationParams:
    """The reference's fields and defaults, plus ``seed``: the tuple test draws with the counter-based sampler and is deterministic."""
    voxel_size: float = 0.05
    division_factor: float = 1.4
    use_absolute_scale: bool = False
    decrease_mu: bool = False
    maximum_correspondence: float = 0.025
    max_iterations: int = 64
    tuple_scale: float = 0.95
    max_tuple_count: int = 1000
    tuple_test: bool = True
    seed: int = 0


@dataclass
class SC2RegistrationParams:
    """Compatibility-graph global registration (``do_sc2_registration``); the reference has no such method.  Rigid
    only, deterministic, no seed: nothing is drawn."""
    voxel_size: float = 0.05
    mutual_filter: bool = True
    max_correspondence: float = 0.075   # compatibility and inlier threshold d_thr (1.5 voxels)
    seed_ratio: float = 0.2             # share of the correspondences taken as seeds
    max_seeds: int = 4096
    k1: int = 30                        # first consensus set
    k2: int = 20                        # second consensus set: 3 <= k2 <= k1 <= 64
    refine_iterations: int = 20


@dataclass
class PhotometricParams:
    """Render-based photometric refinement (``photo.PhotometricRefiner``); the reference has no such step.
    ``max_depth_diff`` has no default: scenes have no common unit of length."""
    max_depth_diff: float = None        # a pixel counts when the two rendered depths differ by at most this
    lambda_depth: float = 0.968         # weight of the depth term (Open3D's hybrid RGB-D odometry); the intensity term has 1 - lambda
    tau: float = 0.5                    # coverage a pixel needs in both renders (depth_agreement's)
    scales: tuple = (4, 2, 1)           # image pyramid, coarse to fine: W/s x H/s pixels, intrinsics over s
    max_iteration: int = 20             # per level, rejected steps included
    min_increment: float = 1e-6         # a level stops when the norm of the accepted increment (omega, v) falls below this
    damping: float = 0.0                # initial Levenberg-Marquardt mu; a rejected step raises it tenfold, an accepted one lowers it
    radius_clip: float = 0.0            # splats of this 3-sigma pixel radius or less are not rendered (the evaluation uses 3; coarse levels need 0)


@dataclass
class WarpParams:
    """Non-rigid refinement (``warp.NonRigidRefiner``); the reference has no such step.
    ``max_corr`` has no default: scenes have no common unit of length."""
    max_corr: float = None              # a correspondence counts when its squared distance is strictly below max_corr^2
    levels: int = 3                     # lattices of 2^l + 1 nodes per axis, l = 0 .. levels - 1 (2^3, 3^3, 5^3); at most 5 (17^3)
    max_iteration: int = 6              # per level; every iteration is one exact solve at fresh correspondences
    lam: float = 0.01                   # weight of the second differences (they do not see affine drift), per correspondence
    lam0: float = 1e-6                  # weight of |U|^2 (and, with 0.01 lam, of the first differences): keeps the system definite
    relative_rmse: float = 1e-6         # a level stops when the point-to-plane RMSE changes by less than this, relatively
