"""
What ellipsoids cost per slice: times one RL slice (100 BD sub-steps) of

  ellipsoids  64 envs x 1024 prolate spheroids, aspect ratio 3, equatorial
              radius 0.5, on k_ellipsoid_run<true> (Gay-Berne, cutoff 6);
  spheres     64 envs x 1024 spheres of the same area (radius 0.5 sqrt(3)) in
              the same box, on k_global (SWARMRL_AMD_CLUSTER_PATH=0: the
              one-workgroup-per-env path whose body, block_env_run, the
              ellipsoid kernel shares),

at equal area fraction.  The two engines are timed alternately (device events
around back-to-back slices after a warm-up); one JSON line is printed with the
median over the rounds and every round's figure.

    python tools/ellipsoid_time.py [--envs 64] [--n 1024] [--steps 100] [--slices 50] [--rounds 5]
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

BOX = 110.0  # area fraction 0.2 with 1024 particles of area 0.75 pi


def make_engine(n_envs, n, steps, ellipsoids, out_folder):
    from swarmrl_amd.engine import MDParams, SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    ureg = UnitRegistry()
    dt = 0.005
    params = MDParams(
        ureg=ureg,
        box_length=ureg.Quantity(3 * [BOX], "micrometer"),
        time_step=ureg.Quantity(dt, "second"),
        time_slice=ureg.Quantity(dt * steps, "second"),
        write_interval=ureg.Quantity(dt * steps * 1000, "second"),
    )
    eng = SwarmEngine(params, n_dims=2, seed=3, out_folder=out_folder, n_envs=n_envs)
    centre = ureg.Quantity(np.array([BOX / 2, BOX / 2, 0.0]), "micrometer")
    spread = ureg.Quantity(0.49 * BOX, "micrometer")
    if ellipsoids:
        eng.add_colloids(
            n, ureg.Quantity(0.5, "micrometer"), centre, spread,
            gamma_translation=ureg.Quantity(np.array([7.0, 7.0, 4.0]), "sim_force / sim_velocity"),
            gamma_rotation=ureg.Quantity(np.array([6.0, 6.0, 3.0]),
                                         "sim_torque / sim_angular_velocity"),
            aspect_ratio=3.0)
    else:
        eng.add_colloids(n, ureg.Quantity(0.5 * np.sqrt(3.0), "micrometer"), centre, spread)
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
    args = ap.parse_args()
    _capi.require_gpu()
    torch.cuda.set_device(0)
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="ellipsoid_time_"))
    ff = ForceFunction({"0": dummy_models.ConstForce(5.0)})
    engines = {}
    for name, ell in (("ellipsoids", True), ("spheres", False)):
        # read when the engine is created: the global path for the comparison
        os.environ["SWARMRL_AMD_CLUSTER_PATH"] = "0"
        eng = make_engine(args.envs, args.n, args.steps, ell, tmp / name)
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
        "slices_timed": args.slices,
        "violations": {n: e.wall_violations() for n, e in engines.items()},
        "ms_per_slice": med,
        "ms_per_slice_range": {n: [round(min(v), 4), round(max(v), 4)] for n, v in times.items()},
        "ms_per_slice_all": {n: [round(x, 4) for x in v] for n, v in times.items()},
        "ratio_ellipsoids_over_spheres": med["ellipsoids"] / med["spheres"],
    }))


if __name__ == "__main__":
    main()
