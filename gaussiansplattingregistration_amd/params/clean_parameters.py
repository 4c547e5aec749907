"""Parameters of floater removal (``clean.outlier_mask``, ``GaussianModel.remove_floaters``): the two Open3D filters --
``remove_statistical_outlier(nb_neighbors, std_ratio)``, ``remove_radius_outlier(nb_points, radius)`` -- behind two splat gates.
Every stage is off at its neutral value; the reference has no cleaning step."""
import math
from dataclasses import dataclass

MAX_NB_NEIGHBORS = 32


@dataclass
class CleanParams:
    """``min_opacity``: drop splats whose activated opacity is below it (0: off).  ``max_extent``: drop splats whose largest
    scale (``exp`` of the stored log-scale) exceeds it (``inf``: off).  ``nb_neighbors`` / ``std_ratio``: the statistical
    filter (``nb_neighbors = 0``: off).  ``radius`` / ``nb_points``: the radius filter (``radius = 0``: off)."""
    min_opacity: float = 0.0
    max_extent: float = math.inf
    nb_neighbors: int = 20
    std_ratio: float = 2.0
    radius: float = 0.0
    nb_points: int = 16

    def __post_init__(self):
        self.validate()

    def validate(self):
        if not (0.0 <= float(self.min_opacity) < 1.0):
            raise ValueError(f"min_opacity must lie in [0, 1) (got {self.min_opacity})")
        if not (float(self.max_extent) > 0.0):
            raise ValueError(f"max_extent must be > 0 (got {self.max_extent})")
        if int(self.nb_neighbors) != self.nb_neighbors or not (0 <= int(self.nb_neighbors) <= MAX_NB_NEIGHBORS):
            raise ValueError(f"nb_neighbors must be an integer in [0, {MAX_NB_NEIGHBORS}] (got {self.nb_neighbors})")
        if int(self.nb_neighbors) >= 1 and not (float(self.std_ratio) > 0.0):
            raise ValueError(f"std_ratio must be > 0 (got {self.std_ratio})")
        if not (float(self.radius) >= 0.0) or math.isinf(float(self.radius)):
            raise ValueError(f"radius must be finite and >= 0 (got {self.radius})")
        if int(self.nb_points) != self.nb_points or int(self.nb_points) < 0:
            raise ValueError(f"nb_points must be an integer >= 0 (got {self.nb_points})")
        return self

    @property
    def min_raw_opacity(self):
        """``logit(min_opacity)`` in float64, what the device compares the raw opacity with (``-inf``: gate off)."""
        a = float(self.min_opacity)
        return -math.inf if a <= 0.0 else math.log(a) - math.log1p(-a)

    @property
    def max_log_scale(self):
        """``ln(max_extent)`` (``+inf``: gate off)."""
        return math.inf if math.isinf(float(self.max_extent)) else math.log(float(self.max_extent))
