"""
What an episodic reset costs, the two ways there are to do one:

  rebuild   a fresh SwarmEngine from get_engine, as EpisodicTrainer does by
            default: the old engine destroyed, add_colloids (one numpy draw
            per colloid and env on the host), engine creation and upload, and
            the first overlap removal (1000 steepest-descent steps);
  in_place  SwarmEngine.reset_envs() on the live engine: the placement kernel
            and the masked overlap removal, split into the two.

The two are timed alternately at each shape (default 1 x 4096 and 64 x 1024
colloids of radius 1 at an area fraction of 0.1); one JSON line is printed
with, per figure, the median over the rounds, their range and every round.
Host wall clock is taken with the device drained before and after; the device
figures are HIP events on the engine's stream.

    python tools/reset_time.py [--shapes 1x4096,64x1024] [--rounds 5] [--slices 2]

--slices: RL slices run on the live engine before each in-place reset, so a
reset always meets a spread-out system, as in training.
"""

import argparse
import json
import pathlib
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_engine(n_envs, n, out_folder, stamps=None):
    """The engine a get_engine would build; stamps: receives the wall clock
    after construction and after add_colloids."""
    from swarmrl_amd.engine import MDParams, SwarmEngine
    from swarmrl_amd.units import UnitRegistry

    L = 2.0 * np.sqrt(n / 0.1)
    ureg = UnitRegistry()
    params = MDParams(ureg=ureg, box_length=ureg.Quantity(3 * [L], "micrometer"),
                      time_step=ureg.Quantity(1e-3, "second"),
                      time_slice=ureg.Quantity(0.1, "second"),
                      write_interval=ureg.Quantity(1000.0, "second"))
    eng = SwarmEngine(params, n_dims=2, seed=3, out_folder=out_folder, n_envs=n_envs)
    if stamps is not None:
        stamps.append(time.perf_counter())
    eng.add_colloids(n, ureg.Quantity(1.0, "micrometer"),
                     ureg.Quantity(np.array([L / 2, L / 2, 0.0]), "micrometer"),
                     ureg.Quantity(L / 2 - 2.0, "micrometer"))
    if stamps is not None:
        stamps.append(time.perf_counter())
    return eng


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def time_rebuild(holder, n_envs, n, out_folder):
    """holder[0]: the engine of the last episode, replaced.  ms: wall total,
    its add_colloids part, its create + upload part, and the overlap
    removal's device time."""
    torch.cuda.synchronize()
    stamps = [time.perf_counter()]
    holder[0] = None  # the trainer drops the old engine first
    eng = make_engine(n_envs, n, out_folder, stamps)
    eng._validate_rod()
    eng._validate_ellipsoids()
    eng._setup_interactions()
    torch.cuda.synchronize()
    stamps.append(time.perf_counter())
    ev0, ev1 = events()
    ev0.record()
    eng._remove_overlap()
    ev1.record()
    eng._init_h5_output()
    eng.integration_initialised = True
    eng.slice_idx = eng.step_idx = 0
    torch.cuda.synchronize()
    stamps.append(time.perf_counter())
    holder[0] = eng
    ms = lambda a, b: (stamps[b] - stamps[a]) * 1e3  # noqa: E731
    return {"wall_ms": ms(0, 4), "add_colloids_ms": ms(1, 2), "create_upload_ms": ms(2, 3),
            "overlap_removal_device_ms": ev0.elapsed_time(ev1)}


def time_in_place(eng):
    """ms: the whole reset_envs() by wall clock and on the device, and the
    placement alone (a reset without overlap removal) on the device."""
    torch.cuda.synchronize()
    ev0, ev1 = events()
    ev0.record()
    eng.reset_envs(remove_overlap=False)
    ev1.record()
    torch.cuda.synchronize()
    place = ev0.elapsed_time(ev1)
    ev0, ev1 = events()
    t0 = time.perf_counter()
    ev0.record()
    eng.reset_envs()
    ev1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    total = ev0.elapsed_time(ev1)
    return {"wall_ms": wall, "device_ms": total, "placement_device_ms": place,
            "overlap_removal_device_ms": total - place}


def summary(rows):
    out = {}
    for k in rows[0]:
        v = [r[k] for r in rows]
        out[k] = {"median": round(float(np.median(v)), 4),
                  "range": [round(min(v), 4), round(max(v), 4)],
                  "all": [round(x, 4) for x in v]}
    return out


def main():
    from swarmrl_amd import _capi
    from swarmrl_amd.agents import dummy_models
    from swarmrl_amd.force_functions import ForceFunction

    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x4096,64x1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slices", type=int, default=2)
    args = ap.parse_args()
    _capi.require_gpu()
    torch.cuda.set_device(0)
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="reset_time_"))
    ff = ForceFunction({"0": dummy_models.ConstForce(5.0)})
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "build_id": _capi.build_id(), "shapes": {}}
    for shape in args.shapes.split(","):
        n_envs, n = (int(v) for v in shape.split("x"))
        live = make_engine(n_envs, n, tmp / f"live_{shape}")
        live.integrate(args.slices, ff)
        live.reset_envs()  # hands the plan over; warm-up
        holder = [make_engine(n_envs, n, tmp / f"rebuilt_{shape}")]
        holder[0].integrate(1, ff)
        rebuild, in_place = [], []
        for _ in range(args.rounds):
            rebuild.append(time_rebuild(holder, n_envs, n, tmp / f"rebuilt_{shape}"))
            holder[0].integrate(args.slices, ff)
            live.integrate(args.slices, ff)
            in_place.append(time_in_place(live))
        rb, ip = summary(rebuild), summary(in_place)
        result["shapes"][shape] = {
            "rebuild": rb, "in_place": ip,
            "wall_ratio_rebuild_over_in_place":
                round(rb["wall_ms"]["median"] / ip["wall_ms"]["median"], 1)}
        holder[0].finalize()
        live.finalize()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
