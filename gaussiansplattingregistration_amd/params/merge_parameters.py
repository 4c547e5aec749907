"""HEM parameters: field names and defaults of the reference's ``src/params/merge_parameters.py:5-10``; the gates of the
overlap-aware merge (``GaussianModel.fuse_overlap``) and the colour harmonisation (``GaussianModel.match_colors``), which the reference does not have."""
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


@dataclass
class ColorMatchParams:
    """Colour harmonisation of registered scenes (``GaussianModel.match_colors``).  ``mode``: ``"gain"``
    (exposure: one factor), ``"channel_gain"`` (white balance: a factor per channel) or ``"affine"`` (a free 3 x 4).  ``huber``: the
    threshold of the robust weight on the colour residual (``inf``: plain least squares); ``iterations``: reweighting rounds;
    ``prior``: the pull towards the identity, relative to the mean weight of an edge; ``min_pairs``: an edge with fewer matched pairs
    does not connect a scene to the reference."""
    mode: str = "affine"
    huber: float = 0.1
    iterations: int = 5
    prior: float = 1e-4
    min_pairs: int = 100

    def validate(self):
        if self.mode not in ("gain", "channel_gain", "affine"):
            raise ValueError(f"mode {self.mode!r} (gain, channel_gain or affine)")
        if not self.huber > 0:
            raise ValueError("huber must be positive (inf: least squares)")
        if self.iterations < 1:
            raise ValueError("iterations must be at least 1")
        if not (self.prior >= 0 and math.isfinite(self.prior)):
            raise ValueError("prior must be finite and >= 0")
        return self
