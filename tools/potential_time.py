"""Cost of the gridded external potential in the 2-D run kernel: the mean
duration of the cluster run launch (engine HIP events, swarm_engine_profile)
with and without a smooth 128 x 128 potential, on the bench-like window (4096
colloids per env, area fraction 0.1, kT > 0, 100 sub-steps): k_cluster_run_wide
at E = 1 and k_cluster_run at E = 64.  The two variants alternate in one
process, REPS times each, on the same engine (the field is set and removed at
the C level), so the spread of the repeats is known.  Prints one JSON line.
Usage: python tools/potential_time.py [E ...]"""
import ctypes
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
sys.path.insert(0, "tests")
from bench_states import disc_states  # noqa: E402
from gpu_harness import Harness, species_list  # noqa: E402

REPS, WINDOWS = 6, 20


def smooth_field(L, n=128, fmax=2.0):
    """cos x cos potential whose force stays below fmax; fp32 [n][n][1]."""
    c = 2 * np.pi * (np.arange(n) + 0.5) / n
    phi = np.cos(2 * c)[:, None] * np.cos(3 * c)[None, :]
    h = L / n
    g = max(np.max(np.abs(np.roll(phi, -1, a) - phi)) for a in (0, 1)) / h
    return np.ascontiguousarray((phi * (fmax / (np.sqrt(2.0) * g)))[:, :, None], np.float32)


def set_field(h, phi, L):
    h.native.bind_stream()
    if phi is None:
        h.native.call("swarm_engine_set_potential_field", None, 0, 0, 0, None)
        return
    sp = np.array([L / phi.shape[0], L / phi.shape[1], L], np.float64)
    h.native.call("swarm_engine_set_potential_field", phi.ctypes.data, phi.shape[0], phi.shape[1],
                  1, sp.ctypes.data)


def timed(h, windows):
    ms, cnt = ctypes.c_double(), ctypes.c_int32()
    h.integrate(100)  # the variant's first launch (code object load) stays outside
    torch.cuda.synchronize()
    h.native.call("swarm_engine_profile", 1, ctypes.byref(ms), ctypes.byref(cnt))
    fb = 0
    for _ in range(windows):
        h.integrate(100)
        fb += int(np.count_nonzero(h.window_stats()[0]))
    torch.cuda.synchronize()
    h.native.call("swarm_engine_profile", 0, ctypes.byref(ms), ctypes.byref(cnt))
    return 1e3 * ms.value / max(cnt.value, 1), fb


def main():
    torch.cuda.set_device(0)
    n = 4096
    L = float(2 * np.sqrt(n / 0.1))
    phi = smooth_field(L)
    out = {}
    for E in [int(a) for a in sys.argv[1:]] or [1, 64]:
        rng = np.random.default_rng(1)
        h = Harness([L, L, L], 1e-3, 1.0239, 1.0239, 42, species_list()[:1], np.zeros(n, int),
                    n_envs=E)
        h.upload(disc_states(rng, n, L, E))
        h.sd(1000)
        h.set_actions(rng.choice([0.0, 10.0], E * n).astype(np.float32),
                      rng.choice([-10.0, 0.0, 10.0], E * n).astype(np.float32))
        h.integrate(100)
        us = {"plain": [], "potential": []}
        fallbacks = 0
        for _ in range(REPS):
            for name, field in (("plain", None), ("potential", phi)):
                set_field(h, field, L)
                t, fb = timed(h, WINDOWS)
                us[name].append(t)
                fallbacks += fb
        a, b = np.asarray(us["plain"]), np.asarray(us["potential"])
        out[f"E{E}"] = {
            "run_us_plain": [round(float(x), 2) for x in a],
            "run_us_potential": [round(float(x), 2) for x in b],
            "mean_plain": round(float(a.mean()), 2), "mean_potential": round(float(b.mean()), 2),
            "ratio": round(float(b.mean() / a.mean()), 4),
            "spread_plain": round(float((a.max() - a.min()) / a.mean()), 4),
            "spread_potential": round(float((b.max() - b.min()) / b.mean()), 4),
            "windows_per_repeat": WINDOWS, "fallback_windows": fallbacks,
        }
    print(json.dumps({"potential_time": out, "grid": [128, 128, 1]}), flush=True)


if __name__ == "__main__":
    main()
