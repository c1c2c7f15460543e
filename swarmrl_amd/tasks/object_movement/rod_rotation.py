"""
RotateRod task (reference: swarmrl/tasks/object_movement/rod_rotation.py):
the colloids are rewarded for turning a rod.  The reward is the rod's mean
angular step (degrees per call, over the last ``velocity_history`` calls),
signed by the wanted direction and shared among the colloids by their part in
the torque on the rod (``compute_torque_partition_on_rod``).

The list path restates the reference in numpy.  For a device view of an
engine with a rod (``SwarmEngine.add_rod``) the whole reward is one HIP launch
(``swarm_rod_reward``), with the history kept per env on the device: the
angular step is then the exact wrapped difference of the centre's stored
angle instead of an arctan2 of two directors.
"""

from typing import List

import numpy as np
import torch

from swarmrl_amd.engine import ops
from swarmrl_amd.engine.swarm_view import is_view
from swarmrl_amd.tasks.task import Task
from swarmrl_amd.utils.colloid_utils import compute_torque_partition_on_rod


class RotateRod(Task):
    """Rotate a rod."""

    supports_device = True

    def __init__(
        self,
        partition: bool = True,
        rod_type: int = 1,
        particle_type: int = 0,
        direction: str = "CCW",
        angular_velocity_scale: int = 1,
        velocity_history: int = 100,
    ):
        super().__init__(particle_type=particle_type)
        self.partition = partition
        self.rod_type = rod_type
        if direction == "CW":
            angular_velocity_scale *= -1  # CW is negative
        self.angular_velocity_scale = angular_velocity_scale
        self._history_length = int(velocity_history)
        self._velocity_history = np.nan * np.ones(self._history_length)
        self._append_index = int(velocity_history - 1)
        self._historic_rod_director = None
        self._historic_velocity = 1.0
        self.decomp_fn = compute_torque_partition_on_rod
        # device path: (id(engine), historic angles [E], ring [E, H], count [E]);
        # _pending: (id(engine), historic angles [E] on the host) of an
        # initialize() with the engine's particle handles
        self._dev = None
        self._pending = None

    # ---------------------------------------------------------- device path
    def _rod_of(self, view):
        rod = getattr(view.engine, "_rod", None)
        if rod is None or rod["type"] != self.rod_type:
            raise ValueError(
                f"{type(self).__name__}: the engine has no rod of type {self.rod_type} "
                "(SwarmEngine.add_rod)"
            )
        return rod

    def _device_state(self, view, hist):
        E, H = view.n_envs, self._history_length
        ring = torch.zeros((E, H), dtype=torch.float64, device=view.device)
        count = torch.zeros(E, dtype=torch.int32, device=view.device)
        self._dev = (id(view.engine), hist, ring, count)

    def _initialize_device(self, view):
        rod = self._rod_of(view)
        self._pending = None
        self._device_state(view, view.ang[:, rod["first"]].clone().contiguous())
        self._historic_rod_director = view.directors()[0, rod["first"]].cpu().numpy()

    def _snapshot_angles(self, engine):
        """The centre's stored angle in every env, taken now: from the
        registry before the first integrate (what the upload will convert),
        else from the device."""
        rod = engine._rod
        if engine._native is None:
            d = np.stack([engine._dir[e][rod["first"]] for e in range(engine.n_envs)])
            a = np.rint(np.arctan2(d[:, 1], d[:, 0]) / (2 * np.pi) * 4294967296.0)
            return (a.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
        ang = engine.get_raw_state()["ang"].reshape(engine.n_envs, engine.n_particles)
        return np.ascontiguousarray(ang[:, rod["first"]])

    def _call_device(self, view):
        if self._dev is None and self._pending is not None:
            if self._pending[0] == id(view.engine):
                hist = torch.as_tensor(self._pending[1].view(np.int32), device=view.device).clone()
                self._device_state(view, hist)
            self._pending = None
        if self._dev is None or self._dev[0] != id(view.engine):
            raise ValueError(f"{type(self).__name__} was not initialised for this engine")
        self._rod_of(view)
        _, hist, ring, count = self._dev
        agents = view.indices_of_type(self.particle_type).to(torch.int32).contiguous()
        A = int(agents.numel())
        out = torch.empty((view.n_envs, A), dtype=torch.float32, device=view.device)
        native = view.engine._native
        native.bind_stream()
        native.call("swarm_rod_reward", agents.data_ptr(), A, hist.data_ptr(), ring.data_ptr(),
                    count.data_ptr(), self._history_length, float(self.angular_velocity_scale),
                    1 if self.partition else 0, out.data_ptr())
        return out

    def reinitialize_envs(self, view, mask):
        raise NotImplementedError("RotateRod cannot re-initialise single envs: an engine with a "
                                  "rod cannot reset in place")

    # ------------------------------------------------------------ list path
    def initialize(self, colloids):
        """The rod's director now is the historic one (all rod particles
        share it, so the first is taken)."""
        if is_view(colloids):
            self._initialize_device(colloids)
            return
        self._dev = None
        self._pending = None
        engine = ops.engine_of(colloids)
        rod = getattr(engine, "_rod", None)
        if rod is not None and rod["type"] == self.rod_type:
            # the engine's own particle handles: a device call may follow
            self._pending = (id(engine), self._snapshot_angles(engine))
        for item in colloids:
            if item.type == self.rod_type:
                self._historic_rod_director = np.copy(item.director)
                break

    def _compute_angular_velocity(self, new_director: np.ndarray):
        """Angular step of the rod in degrees, pushed into the history; the
        scaled mean over the filled history is returned."""
        old = np.asarray(self._historic_rod_director, dtype=np.float64)
        new = np.asarray(new_director, dtype=np.float64)
        angular_velocity = np.arctan2(
            old[0] * new[1] - old[1] * new[0],
            old[0] * new[0] + old[1] * new[1],
        )
        angular_velocity = np.rad2deg(angular_velocity)
        self._historic_rod_director = new_director
        self._velocity_history = np.roll(self._velocity_history, -1)
        self._velocity_history[self._append_index] = angular_velocity
        return self.angular_velocity_scale * np.nanmean(self._velocity_history)

    def partition_reward(
        self,
        reward: float,
        colloid_positions: np.ndarray,
        rod_positions: np.ndarray,
        rod_directors: np.ndarray,
    ) -> np.ndarray:
        """The reward shared among the colloids: by their part in the torque
        on the rod, or uniformly."""
        if self.partition:
            colloid_partitions = self.decomp_fn(colloid_positions, rod_positions, rod_directors)
        else:
            colloid_partitions = np.ones(colloid_positions.shape[0]) / colloid_positions.shape[0]
        return reward * colloid_partitions

    def _compute_angular_velocity_reward(self, rod_directors, rod_positions, colloid_positions):
        angular_velocity = self._compute_angular_velocity(rod_directors[0])
        return self.partition_reward(
            angular_velocity, colloid_positions, rod_positions, rod_directors
        )

    def __call__(self, colloids: List):
        """Rewards: (A,) numpy for lists, [E, A] device tensor for views."""
        if is_view(colloids):
            return self._call_device(colloids)
        rod = [colloid for colloid in colloids if colloid.type == self.rod_type]
        rod_positions = np.array([colloid.pos for colloid in rod], dtype=np.float64)
        rod_directors = np.array([colloid.director for colloid in rod], dtype=np.float64)
        chosen_colloids = [colloid for colloid in colloids if colloid.type == self.particle_type]
        colloid_positions = np.array([colloid.pos for colloid in chosen_colloids],
                                     dtype=np.float64)
        reward = self._compute_angular_velocity_reward(
            rod_directors, rod_positions, colloid_positions
        )
        return np.asarray(reward, dtype=np.float32)
