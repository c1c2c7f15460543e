"""
What a rod costs per slice: times one RL slice (100 BD sub-steps) of

  rod     64 envs x (50 colloids + a 101-particle rod), on k_rod_run;
  no_rod  the same 64 x 50 colloids without a rod, on k_global
          (SWARMRL_AMD_CLUSTER_PATH=0: the one-workgroup-per-env path whose
          body, block_env_run, the rod kernel shares),

so that their difference is the rod's 101 extra particles, its two barriers
and its reduction.  The two engines are timed alternately (device events
around back-to-back slices after a warm-up); one JSON line is printed.

    python tools/rod_time.py [--envs 64] [--steps 100] [--slices 50] [--rounds 5]
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


def make_engine(n_envs, steps, rod, out_folder):
    from swarmrl_amd.engine import MDParams, SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    dt = 0.005
    params = MDParams(
        ureg=ureg,
        box_length=ureg.Quantity(3 * [150.0], "micrometer"),
        time_step=ureg.Quantity(dt, "second"),
        time_slice=ureg.Quantity(dt * steps, "second"),
        write_interval=ureg.Quantity(dt * steps * 1000, "second"),
    )
    eng = SwarmEngine(params, n_dims=2, seed=3, out_folder=out_folder, n_envs=n_envs)
    eng.add_colloids(50, ureg.Quantity(1.0, "micrometer"),
                     ureg.Quantity(np.array([75.0, 75.0, 0.0]), "micrometer"),
                     ureg.Quantity(40.0, "micrometer"), type_colloid=0)
    if rod:
        eng.add_rod(ureg.Quantity(np.array([75.0, 75.0, 0.0]), "micrometer"),
                    ureg.Quantity(100.0, "micrometer"), ureg.Quantity(5.0, "micrometer"), 0.3,
                    101, ureg.Quantity(20.0, "sim_force / sim_velocity"),
                    ureg.Quantity(2000.0, "sim_force * sim_length * sim_time"), 2, fixed=False)
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--slices", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    _capi.require_gpu()
    torch.cuda.set_device(0)
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="rod_time_"))
    ff = ForceFunction({"0": dummy_models.ConstForce(5.0)})
    engines = {}
    for name, rod in (("rod", True), ("no_rod", False)):
        # read when the engine is created: the global path for the comparison
        os.environ["SWARMRL_AMD_CLUSTER_PATH"] = "0"
        eng = make_engine(args.envs, args.steps, rod, tmp / name)
        eng.integrate(2, ff)  # set-up, overlap removal, actions; warm-up
        engines[name] = eng
    times = {name: [] for name in engines}
    for _ in range(args.rounds):
        for name, eng in engines.items():
            times[name].append(time_slices(eng, args.steps, args.slices))
    med = {name: float(np.median(v)) for name, v in times.items()}
    print(json.dumps({
        "device": torch.cuda.get_device_name(0),
        "envs": args.envs, "sub_steps_per_slice": args.steps, "slices_timed": args.slices,
        "particles_per_env": {n: e.n_particles for n, e in engines.items()},
        "ms_per_slice": med,
        "ms_per_slice_all": {n: [round(x, 4) for x in v] for n, v in times.items()},
        "ratio_rod_over_no_rod": med["rod"] / med["no_rod"],
    }))


if __name__ == "__main__":
    main()
