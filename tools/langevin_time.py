"""
What the Langevin thermostat costs per slice: times one RL slice (100
sub-steps) of 64 envs x 1024 spheres of radius 0.5 at an area fraction of
0.066 in the same box on

  langevin       k_langevin_run, no flow field;
  langevin_flow  k_langevin_run with a 128 x 128 flow field;
  brownian       k_global (SWARMRL_AMD_CLUSTER_PATH=0: the one-workgroup-per-
                 env path whose body, block_env_run, the Langevin kernel
                 shares).

The three engines are timed alternately (device events around back-to-back
slices after a warm-up); one JSON line is printed with the median over the
rounds, their range and every round's figure.

    python tools/langevin_time.py [--envs 64] [--n 1024] [--steps 100] [--slices 50] [--rounds 5]
                                  [--force 5.0] [--dt 0.005]

--force: the swim force (0: passive particles).  --dt: the time step.
"max_abs_image" in the output is the largest image counter of each engine at
the end: a particle whose displacement saturates at half a box every sub-step
crosses the box every other sub-step, so a figure near half the number of
sub-steps run says that the engine's state, and with it its slice time, is
not the stationary one ("Langevin").
"""

import argparse
import json
import os
import pathlib
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

BOX = 110.0
FLOW_CELLS = 128


def make_engine(n_envs, n, steps, thermostat, flow, out_folder, dt=0.005):
    from swarmrl_amd.engine import MDParams, SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    params = MDParams(
        ureg=ureg,
        box_length=ureg.Quantity(3 * [BOX], "micrometer"),
        time_step=ureg.Quantity(dt, "second"),
        time_slice=ureg.Quantity(dt * steps, "second"),
        write_interval=ureg.Quantity(dt * steps * 1000, "second"),
        thermostat_type=thermostat,
    )
    eng = SwarmEngine(params, n_dims=2, seed=3, out_folder=out_folder, n_envs=n_envs)
    centre = ureg.Quantity(np.array([BOX / 2, BOX / 2, 0.0]), "micrometer")
    spread = ureg.Quantity(0.49 * BOX, "micrometer")
    kw = {}
    if thermostat == "langevin":  # dt gamma / m = 0.012 with the sphere's Stokes friction
        kw = dict(mass=ureg.Quantity(1.0, "sim_mass"),
                  rinertia=ureg.Quantity(3 * [1.0], "sim_rinertia"))
    eng.add_colloids(n, ureg.Quantity(0.5, "micrometer"), centre, spread, **kw)
    if flow:
        k = (np.arange(FLOW_CELLS) + 0.5) * (2.0 * np.pi / FLOW_CELLS)
        u = np.zeros((FLOW_CELLS, FLOW_CELLS, 1, 3))
        u[..., 0] = 2.0 * np.sin(k)[:, None, None] * np.cos(k)[None, :, None]
        u[..., 1] = -2.0 * np.cos(k)[:, None, None] * np.sin(k)[None, :, None]
        gamma_t, _ = eng.get_friction_coefficients(0)
        eng.add_flowfield(ureg.Quantity(u, "sim_velocity"),
                          ureg.Quantity(float(gamma_t), "sim_mass/sim_time"),
                          ureg.Quantity(np.array([BOX / FLOW_CELLS, BOX / FLOW_CELLS, BOX]),
                                        "micrometer"))
    return eng


def time_slices(eng, steps, slices):
    """ms per slice over `slices` back-to-back slices (device events)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng._native.bind_stream()
    start.record()
    for _ in range(slices):
        eng._native.call("swarm_engine_integrate", int(steps))
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / slices


def main():
    from swarmrl_amd import _capi
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--slices", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--force", type=float, default=5.0)
    ap.add_argument("--dt", type=float, default=0.005)
    args = ap.parse_args()
    _capi.require_gpu()
    torch.cuda.set_device(0)
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="langevin_time_"))
    ff = ForceFunction({"0": dummy_models.ConstForce(args.force)})
    engines = {}
    for name, thermostat, flow in (("langevin", "langevin", False),
                                   ("langevin_flow", "langevin", True),
                                   ("brownian", "brownian", False)):
        # read when the engine is created: the global path for the comparison
        os.environ["SWARMRL_AMD_CLUSTER_PATH"] = "0"
        eng = make_engine(args.envs, args.n, args.steps, thermostat, flow, tmp / name, args.dt)
        eng.integrate(2, ff)  # set-up, overlap removal, actions; warm-up
        engines[name] = eng
    times = {name: [] for name in engines}
    for _ in range(args.rounds):
        for name, eng in engines.items():
            times[name].append(time_slices(eng, args.steps, args.slices))
    med = {name: float(np.median(v)) for name, v in times.items()}
    print(json.dumps({
        "device": torch.cuda.get_device_name(0),
        "envs": args.envs, "particles_per_env": args.n, "sub_steps_per_slice": args.steps,
        "slices_timed": args.slices, "flow_cells": FLOW_CELLS, "swim_force": args.force,
        "time_step": args.dt,
        "max_abs_image": {n: int(np.abs(e.get_raw_state()["img"]).max())
                          for n, e in engines.items()},
        "ms_per_slice": med,
        "ms_per_slice_range": {n: [round(min(v), 4), round(max(v), 4)] for n, v in times.items()},
        "ms_per_slice_all": {n: [round(x, 4) for x in v] for n, v in times.items()},
        "ratio_langevin_over_brownian": med["langevin"] / med["brownian"],
        "ratio_langevin_flow_over_langevin": med["langevin_flow"] / med["langevin"],
    }))


if __name__ == "__main__":
    main()
