"""
End conditions for SwarmEngine.set_auto_reset: callables done_fn(view) ->
uint8 [n_envs] device tensor (non-zero: the env's episode ends after this
slice and the env is reset), evaluated with no host synchronisation.
"""

import numpy as np
import torch


class EverySlices:
    """Env e is done every n-th slice, shifted by e * offset_per_env: after
    the calls number c (counted from 1) with (c + e * offset_per_env) % n == 0.
    The call count lives on the device and advances by a device op, so a
    captured episode graph goes on counting when it is replayed."""

    def __init__(self, n: int, offset_per_env: int = 0):
        if int(n) < 1:
            raise ValueError("n must be >= 1")
        self.n = int(n)
        self.offset_per_env = int(offset_per_env)
        self._state = None  # (device, calls int64 [1], shift int64 [E])

    def __call__(self, view) -> torch.Tensor:
        dev = torch.device(view.device)
        if (self._state is None or self._state[0] != dev
                or self._state[2].numel() != view.n_envs):
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("EverySlices: first call under a stream capture (call it, or "
                                   "integrate one slice, before capturing)")
            shift = torch.arange(view.n_envs, dtype=torch.int64, device=dev) * self.offset_per_env
            self._state = (dev, torch.zeros(1, dtype=torch.int64, device=dev), shift)
        _, calls, shift = self._state
        calls += 1
        return ((calls + shift) % self.n == 0).to(torch.uint8)


class AllWithin:
    """Env done when all its agents (particle_type) lie within `radius` of
    `centre` (unwrapped positions, the engine's length unit)."""

    def __init__(self, centre, radius: float, particle_type: int = 0):
        self.centre = np.asarray(centre, dtype=float).reshape(3)
        self.radius = float(radius)
        self.particle_type = int(particle_type)
        self._centre_dev = None

    def __call__(self, view) -> torch.Tensor:
        dev = torch.device(view.device)
        if self._centre_dev is None or self._centre_dev.device != dev:
            self._centre_dev = torch.as_tensor(self.centre, dtype=torch.float64, device=dev)
        idx = view.indices_of_type(self.particle_type).long()
        d = view.positions()[:, idx, :] - self._centre_dev
        if view.n_dims == 2:
            d = d[..., :2]
        inside = torch.linalg.vector_norm(d, dim=-1) <= self.radius
        return inside.all(dim=1).to(torch.uint8)


__all__ = ["EverySlices", "AllWithin"]
