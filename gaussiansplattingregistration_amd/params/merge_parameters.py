"""HEM parameters: field names and defaults of the reference's ``src/params/merge_parameters.py:5-10``; the gates of the
overlap-aware merge (``GaussianModel.fuse_overlap``), which the reference does not have."""
import math
from dataclasses import dataclass


@dataclass
class GaussianMixtureParams:
    hem_reduction: float = 3.0
    distance_delta: float = 3.0
    color_delta: float = 2.5
    decay_rate: float = 1.0
    cluster_level: int = 3


@dataclass
class FuseOverlapParams:
    """Gates of ``gsr_model_fuse``: a splat of each model pair up when they are each other's best match among the candidates with
    centres within ``max_distance``, DC colours within ``color_delta`` (L2; ``inf``: no colour gate) and a symmetrised KL divergence
    of at most ``kld_max``."""
    max_distance: float
    kld_max: float = 0.5
    color_delta: float = math.inf
