"""
fp64 statement of the Langevin scheme and of the flow field's sampling (a
helper, not a test): what tests/csrc/langevin_oracle.c and the kernel are
compared against where the comparison is not bit for bit.

The flow is sampled as the reference builds it (espresso.py:986-989): every
component padded by one cell with np.pad(mode="wrap"), element (0, 0, 0) of
the padded array at -h / 2, trilinear interpolation.
"""

import numpy as np


def flow_sample(u, pos, h):
    """u (nx, ny, nz, 3), pos (N, 3) folded positions, h [3] -> (N, 3) fp64."""
    u = np.asarray(u, np.float64)
    h = np.asarray(h, np.float64)
    pos = np.asarray(pos, np.float64)
    pad = np.stack([np.pad(u[:, :, :, c], pad_width=1, mode="wrap") for c in range(3)], axis=3)
    g = (pos + 0.5 * h) / h  # padded element k sits at (k - .5) h
    i0 = np.floor(g).astype(np.int64)
    t = g - i0
    out = np.zeros((len(pos), 3))
    for cx in range(2):
        for cy in range(2):
            for cz in range(2):
                w = ((t[:, 0] if cx else 1.0 - t[:, 0]) * (t[:, 1] if cy else 1.0 - t[:, 1])
                     * (t[:, 2] if cz else 1.0 - t[:, 2]))
                out += w[:, None] * pad[i0[:, 0] + cx, i0[:, 1] + cy, i0[:, 2] + cz]
    return out


def recurrence(x, v, n_steps, dt, mass, gamma_t, f, gamma_flow=0.0, flow=None):
    """The deterministic (kT = 0) translation of one particle in fp64:
        F = f + gamma_flow (u(x) - v) - gamma_t v,  v += (dt / m) F,  x += dt v.
    x, v, f: [2]; flow: None or a callable x -> u(x) [2].  Returns (x, v)
    unwrapped."""
    x = np.array(x, np.float64)
    v = np.array(v, np.float64)
    f = np.asarray(f, np.float64)
    for _ in range(n_steps):
        u = np.zeros(2) if flow is None else np.asarray(flow(x), np.float64)
        F = f + gamma_flow * (u - v) - gamma_t * v
        v = v + (dt / mass) * F
        x = x + dt * v
    return x, v


def stationary_variance(kT, inertia, a):
    """<v^2> of the free scheme v' = (1 - a) v + (dt / m) sig (U - 1/2) with
    sig^2 / 12 = 2 kT gamma / dt and a = dt gamma / m:
    (dt / m)^2 (2 kT gamma / dt) / (1 - (1 - a)^2) = (kT / m) / (1 - a / 2)."""
    return (kT / inertia) / (1.0 - 0.5 * a)
