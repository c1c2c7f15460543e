"""
Trajectory buffer of an agent (reference: swarmrl/utils/colloid_utils.py:15-26)
and the torque partition of the rod tasks (colloid_utils.py:29-117).
"""

from dataclasses import dataclass, field

import numpy as np


@dataclass
class TrajectoryInformation:
    """Per-episode features, actions, log-probs and rewards of one agent."""

    particle_type: int
    features: list = field(default_factory=list)
    actions: list = field(default_factory=list)
    log_probs: list = field(default_factory=list)
    rewards: list = field(default_factory=list)
    killed: bool = False
    # auto-reset engines: per reward, the uint8 [E] mask of the envs that were
    # reset after that transition (empty: no episode ended inside)
    dones: list = field(default_factory=list)


def compute_torque_partition_on_rod(colloid_positions, rod_positions, rod_directions):
    """
    The share of every colloid in the torque on a rod
    (reference: swarmrl/utils/colloid_utils.py:29-117), numpy fp64.

    Per colloid i and rod particle b: r = r_b - r_i (xy components, as given:
    unwrapped, no minimum image), f_ib = grad(1 / |r|^12) = -12 r / |r|^14,
    torque_ib = cross(director_b, f_ib); the colloid's weight is
    |sum_b torque_ib| + 1e-8, normalised over the colloids.  The reference's
    quirks are kept: the cross product takes the rod's director, not the
    lever arm.

    colloid_positions (n_colloids, 3), rod_positions (n_rod, 3),
    rod_directions (n_rod, 3) -> (n_colloids,)
    """
    cp = np.asarray(colloid_positions, dtype=np.float64)
    rp = np.asarray(rod_positions, dtype=np.float64)
    rd = np.asarray(rod_directions, dtype=np.float64)
    r = (rp[None, :, :] - cp[:, None, :])[:, :, :2]  # (n_colloids, n_rod, 2)
    r2 = np.sum(r * r, axis=-1, keepdims=True)
    forces = -12.0 * r / r2**7
    forces3 = np.concatenate([forces, np.zeros_like(forces[..., :1])], axis=-1)
    torques = np.cross(rd[None, :, :], forces3)
    net_rod_torque = torques.sum(axis=1)
    torque_magnitude = np.linalg.norm(net_rod_torque, axis=-1) + 1e-8
    return torque_magnitude / torque_magnitude.sum()
