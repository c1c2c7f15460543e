from swarmrl_amd.utils import utils
from swarmrl_amd.utils.colloid_utils import TrajectoryInformation
from swarmrl_amd.utils.utils import (
    calc_ellipsoid_friction_factors_rotation,
    calc_ellipsoid_friction_factors_translation,
)

__all__ = [
    "TrajectoryInformation",
    "calc_ellipsoid_friction_factors_rotation",
    "calc_ellipsoid_friction_factors_translation",
    "utils",
]
