"""
Gradient-sensing ("find the source") task (reference:
swarmrl/tasks/searching/gradient_sensing.py:21-150).

reward = clip(scale * (f(|x_t/L - src/L|) - f(|x_{t-1}/L - src/L|)), 0, inf)
per agent, with a per-id history.  Distances and the history update run in
the HIP kernel ``k_field``.
"""

import numpy as np
import torch

from swarmrl_amd.engine import ops
from swarmrl_amd.engine.swarm_view import is_view
from swarmrl_amd.tasks.task import Task


class GradientSensing(Task):
    """Reward for climbing a radial field towards a source."""

    supports_device = True

    def __init__(
        self,
        source: np.ndarray = np.array([0, 0, 0]),
        decay_function: callable = None,
        box_length: np.ndarray = np.array([1.0, 1.0, 0.0]),
        reward_scale_factor: int = 10,
        particle_type: int = 0,
    ):
        super().__init__(particle_type=particle_type)
        self.source = source / box_length
        self._source_raw = np.asarray(source, dtype=float)
        self.decay_fn = decay_function
        self.reward_scale_factor = reward_scale_factor
        self.box_length = box_length
        self._historic_positions = {}
        self._dev_hist = None
        self._pending = None
        self._affine = None

    def initialize(self, colloids):
        """Store the starting positions of particle_type colloids (lines 60-79)."""
        if is_view(colloids):
            view = colloids
            agents = view.indices_of_type(self.particle_type)
            A = int(agents.numel()) * view.n_envs
            hq = torch.zeros((3, A), dtype=torch.int32, device=view.device)
            hi = torch.zeros((3, A), dtype=torch.int32, device=view.device)
            ops.field_distance(
                view.engine._native, view.n_envs, agents, self._source_raw, self.box_length,
                hq, hi, update=True, init_only=True,
            )
            self._dev_hist = (id(view.engine), hq, hi)
            return
        engine = ops.engine_of(colloids)
        self._pending = None
        self._dev_hist = None
        if engine is not None:
            self._pending = (id(engine), *ops.snapshot_history(engine, self.particle_type))
        for item in colloids:
            if item.type == self.particle_type:
                index = np.copy(item.id)
                position = np.copy(item.pos) / self.box_length
                self._historic_positions[str(index)] = position

    def reinitialize_envs(self, view, mask):
        """The marked envs' history <- their current (fresh) positions."""
        hq, hi = ops.device_history(self, view)
        ops.field_history_marked(view.engine._native, mask,
                                 view.indices_of_type(self.particle_type), hq, hi)

    def change_source(self, new_source: np.ndarray):
        self.source = new_source
        self._source_raw = np.asarray(new_source, dtype=float) * np.asarray(self.box_length)

    def _reward(self, d_cur, d_prev):
        delta = self.decay_fn(d_cur) - self.decay_fn(d_prev)
        r = self.reward_scale_factor * delta
        if isinstance(r, torch.Tensor):
            return torch.clamp(r, min=0.0)
        return np.clip(r, 0.0, None)

    def compute_colloid_reward(self, index: int, colloids):
        colloid_id = str(np.copy(colloids[index].id))
        current_position = np.copy(colloids[index].pos) / self.box_length
        old_position = self._historic_positions[colloid_id]
        d_cur, d_prev = ops.list_field_distance(current_position[None], old_position[None], self.source)
        self._historic_positions[colloid_id] = current_position
        return self._reward(d_cur, d_prev)[0]

    def __call__(self, colloids):
        """Rewards per agent: (A,) numpy for lists, [E, A] device tensor for views."""
        if is_view(colloids):
            view = colloids
            if self._dev_hist is None and getattr(self, "_pending", None) is not None:
                if self._pending[0] == id(view.engine):
                    self._dev_hist = (self._pending[0], *ops.history_tensors(
                        self._pending[1], self._pending[2], view.device))
                self._pending = None
            if self._dev_hist is None or self._dev_hist[0] != id(view.engine):
                raise ValueError("GradientSensing was not initialised for this engine")
            agents = view.indices_of_type(self.particle_type)
            _, hq, hi = self._dev_hist
            if self._affine is None:
                self._affine = ops.affine_coefficients(self.decay_fn) or False
            if self._affine:
                return ops.field_transform(
                    view.engine._native, view.n_envs, agents, self._source_raw, self.box_length,
                    hq, hi, self._affine[0], self._affine[1], float(self.reward_scale_factor),
                    True,
                )
            d_cur, d_prev = ops.field_distance(
                view.engine._native, view.n_envs, agents, self._source_raw, self.box_length,
                hq, hi, update=True,
            )
            return self._reward(d_cur, d_prev)
        colloid_indices = self.get_colloid_indices(colloids)
        if len(colloid_indices) == 0:
            return np.zeros(0, dtype=np.float32)
        keys = [str(np.copy(colloids[i].id)) for i in colloid_indices]
        cur = np.stack([np.copy(colloids[i].pos) / self.box_length for i in colloid_indices])
        prev = np.stack([self._historic_positions[k] for k in keys])
        d_cur, d_prev = ops.list_field_distance(cur, prev, self.source)
        for k, p in zip(keys, cur):
            self._historic_positions[k] = p
        return np.asarray(self._reward(d_cur, d_prev), dtype=np.float32)
