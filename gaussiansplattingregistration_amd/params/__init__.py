from .merge_parameters import ColorMatchParams, FuseOverlapParams, GaussianMixtureParams  # noqa: F401
from .registration_parameters import LocalRegistrationParams, MixtureRegistrationParams, MultiScaleRegistrationParams, PhotometricParams, WarpParams  # noqa: F401
