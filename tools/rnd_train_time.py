"""Time RNDReward.update (the RND predictor's training) with HIP events, the
torch loop (SWARMRL_AMD_FUSED_RND_TRAIN=0, the code before the fused
kernels) and the fused path (swarm_rnd_targets + swarm_rnd_train_epoch)
alternating, three runs each, one epoch per run:

    n = 4096 and 16384 observations (a headline slice, a C5 slice), d_in = 1,
    batch 8 (the reference's RNDConfig), and 16384 once more with batch 64.

Prints microseconds per minibatch step for both paths and, labelled as
extrapolated, the time of a full C5 update (T slices of 16384 observations,
100 epochs of batch 8) at the measured per-step times.

usage: python tools/rnd_train_time.py [--runs 3] [--fused-only] [--slices 10]
       rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- \
           python tools/rnd_train_time.py --fused-only --runs 1
       (the kernel's own time: k_rnd_train rows of the kernel trace)
--rnd-module FILE times the RNDReward of another version of
intrinsic_reward/random_network_distillation.py (e.g. the parent commit's)."""
import argparse
import importlib.util
import os
import sys

import torch

sys.path.insert(0, ".")
from swarmrl_amd.intrinsic_reward import RNDConfig  # noqa: E402
from swarmrl_amd.utils.colloid_utils import TrajectoryInformation  # noqa: E402

SWITCH = "SWARMRL_AMD_FUSED_RND_TRAIN"
SIZES = ((4096, 8), (16384, 8), (16384, 64))


def reward_class(path):
    if path is None:
        from swarmrl_amd.intrinsic_reward import RNDReward
        return RNDReward
    spec = importlib.util.spec_from_file_location("rnd_other_version", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.RNDReward


def time_update(cls, n, batch, fused, seed=0):
    """Milliseconds of one update (one epoch) from a fresh RNDReward: the
    first update warms up (code objects, optimizer state), the second is
    timed."""
    os.environ[SWITCH] = "1" if fused else "0"
    dev = torch.device("cuda", 0)
    torch.manual_seed(seed)
    rnd = cls(RNDConfig(input_shape=(1,), n_epochs=1, batch_size=batch, device=dev))
    traj = TrajectoryInformation(particle_type=0)
    traj.features = [torch.rand(1, n, 1, device=dev)]
    warm = TrajectoryInformation(particle_type=0)
    warm.features = [torch.rand(1, 64 * batch, 1, device=dev)]
    rnd.update(warm)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rnd.update(traj)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--slices", type=int, default=10, help="T of the extrapolated C5 episode")
    ap.add_argument("--rnd-module", default=None)
    ns = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnd_train_time: no HIP device")
    cls = reward_class(ns.rnd_module)
    per_step = {}
    for n, batch in SIZES:
        steps = -(-n // batch)
        times = {True: [], False: []}
        for run in range(ns.runs):
            for fused in ((True,) if ns.fused_only else (False, True)):
                times[fused].append(time_update(cls, n, batch, fused, seed=run))
        row = f"n={n:6d} B={batch:2d} steps={steps:5d}"
        for fused, name in ((False, "torch"), (True, "fused")):
            if times[fused]:
                us = sorted(1e3 * t / steps for t in times[fused])
                per_step[(n, batch, fused)] = us[len(us) // 2]
                row += f" | {name} us/step " + " ".join(f"{u:8.2f}" for u in us)
        if times[False] and times[True]:
            row += f" | ratio {per_step[(n, batch, False)] / per_step[(n, batch, True)]:6.1f}x"
        print(row, flush=True)
    full = ns.slices * 2048 * 100
    for fused, name in ((False, "torch"), (True, "fused")):
        us = per_step.get((16384, 8, fused))
        if us is not None:
            print(f"EXTRAPOLATED (not run): full C5 update, {ns.slices} slices x 16384 "
                  f"observations, 100 epochs of batch 8 = {full} steps at {us:.2f} us/step "
                  f"({name}): {full * us * 1e-6:.1f} s", flush=True)


if __name__ == "__main__":
    main()
