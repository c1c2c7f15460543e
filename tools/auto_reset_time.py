"""
What auto-reset costs per slice, through a captured episode graph
(bench.capture_episode on bench.build_workload), three builds of the same
workload side by side:

  off       no auto-reset: today's schedule (the next slice's build forked
            early, riding in the reward launch);
  never     set_auto_reset with an end condition that never fires
            (EverySlices with n far above anything run): the done mask, its
            record, the three reset launches of unmarked envs and the history
            launch every slice, and no early fork;
  one       one env done per slice (EverySlices(E, offset_per_env=1)): the
            same plus one env's placement and 1000 steps of overlap removal.

The three episode graphs are replayed alternately; one JSON line is printed
with, per figure, the median over the rounds, their range and every round
(ms per slice, HIP events round --replays replays of the T-slice graph).

    python tools/auto_reset_time.py [--shapes 1x4096,64x1024] [--rounds 5]
                                    [--episode-length 10] [--replays 3]
"""

import argparse
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build(mode, n_envs, n, T, dev):
    import bench
    from swarmrl_amd.engine.termination import EverySlices

    ns = argparse.Namespace(colloids=n, envs_per_gpu=n_envs, write_interval=1000.0)
    eng, ff, agent = bench.build_workload(ns, 42, dev)
    if mode == "never":
        eng.set_auto_reset(EverySlices(1 << 40))
    elif mode == "one":
        eng.set_auto_reset(EverySlices(n_envs, offset_per_env=1))
    eng.integrate(1, ff)  # set-up, overlap removal, first slice; the reset plan
    _, graph, _ = bench.capture_episode(eng, ff, agent, T)
    return eng, agent, graph


def time_replays(graph, replays):
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(replays):
        graph.replay()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1)


def summary(v):
    return {"median": round(float(np.median(v)), 4), "range": [round(min(v), 4), round(max(v), 4)],
            "all": [round(x, 4) for x in v]}


def main():
    from swarmrl_amd import _capi

    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x4096,64x1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--episode-length", type=int, default=10)
    ap.add_argument("--replays", type=int, default=3)
    args = ap.parse_args()
    _capi.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    T = args.episode_length
    modes = ("off", "never", "one")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "episode_length": T, "replays": args.replays, "build_id": _capi.build_id(),
              "unit": "ms per slice", "shapes": {}}
    for shape in args.shapes.split(","):
        n_envs, n = (int(v) for v in shape.split("x"))
        built = {m: build(m, n_envs, n, T, dev) for m in modes}
        for m in modes:  # warm-up replay
            time_replays(built[m][2], 1)
        counts0 = {m: built[m][0].reset_counts().astype(np.int64) for m in modes}
        rows = {m: [] for m in modes}
        for _ in range(args.rounds):
            for m in modes:
                rows[m].append(time_replays(built[m][2], args.replays) / (args.replays * T))
        slices = args.rounds * args.replays * T
        out = {m: summary(rows[m]) for m in modes}
        for m in modes:
            done = built[m][0].reset_counts().astype(np.int64) - counts0[m]
            out[m]["resets_per_slice"] = round(float(done.sum()) / slices, 4)
        out["never_minus_off_ms"] = round(out["never"]["median"] - out["off"]["median"], 4)
        out["one_minus_never_ms"] = round(out["one"]["median"] - out["never"]["median"], 4)
        result["shapes"][shape] = out
        for m in modes:
            built[m][0].finalize()
        del built
    print(json.dumps(result))


if __name__ == "__main__":
    main()
