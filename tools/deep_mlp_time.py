"""Rollout and PPO update cost of a deep actor-critic MLP, 3-(128,128)-(4+1), on
the bench workload (4096 colloids per env, vision cones, gradient sensing):

  python tools/deep_mlp_time.py [E] [--plain]

prints, for E envs (default 1),
  - the rollout time per slice, from a replayed episode graph of 20 slices
    (as bench.py times the rollout), and
  - the update time per PPO epoch (compute_loss over the episode / n_epochs;
    episodes after the first eager one and the graph capture).

The network is DeepActorCriticMLP where the package has it -- rollout through
swarm_policy_deep_sample and the update through swarm_ppo_deep_epoch_grad --
and otherwise (an older checkout, or --plain) the same layers as a plain
nn.Module, which takes the torch fallback of both halves: one GEMM per layer
and swarm_sample_actions in the rollout, torch autograd in the update.  The
baseline of the table in DESIGN.md is this tool run in a checkout of the
parent commit."""
import argparse
import sys
import time

import torch
from torch import nn

sys.path.insert(0, ".")
import bench  # noqa: E402
from swarmrl_amd.networks import TorchModel  # noqa: E402

try:
    from swarmrl_amd.networks import DeepActorCriticMLP
except ImportError:
    DeepActorCriticMLP = None


class PlainDeepMLP(nn.Module):
    """The layers of DeepActorCriticMLP(input_dim, n_actions, hidden) under
    names no fused gate knows."""

    def __init__(self, input_dim, n_actions=4, hidden=(128, 128)):
        super().__init__()
        widths = [input_dim, *hidden]
        self.trunk = nn.ModuleList(nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))
        self.actor = nn.Linear(widths[-1], n_actions)
        self.critic = nn.Linear(widths[-1], 1)

    def _h(self, x):
        for layer in self.trunk:
            x = torch.relu(layer(x))
        return x

    def forward(self, x):
        h = self._h(x)
        return self.actor(h), self.critic(h)

    def logits(self, x):
        return self.actor(self._h(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("envs", nargs="?", type=int, default=1)
    ap.add_argument("--plain", action="store_true",
                    help="the plain nn.Module (torch fallback) even where the deep class exists")
    ap.add_argument("--replays", type=int, default=10, help="timed episode-graph replays")
    ap.add_argument("--episodes", type=int, default=5, help="updates (the first two untimed)")
    args = ap.parse_args()
    E, T = args.envs, 20
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ns = argparse.Namespace(colloids=4096, envs_per_gpu=E)
    eng, ff, agent = bench.build_workload(ns, 42, dev)
    deep = DeepActorCriticMLP is not None and not args.plain
    torch.manual_seed(42)
    module = (DeepActorCriticMLP if deep else PlainDeepMLP)(3, 4, (128, 128))
    agent.network = TorchModel(module, input_shape=(3,), device=dev)
    kind = "fused deep kernels" if deep and agent.network.ppo_layers(3) is not None else \
        "torch fallback"
    eng.integrate(1, ff)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eng.integrate(1, ff)
    torch.cuda.current_stream().wait_stream(side)
    agent.reset_trajectory()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.integrate(T, ff)
    traj = agent.trajectory  # the graph's output tensors, rewritten by every replay
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.replays):
        graph.replay()
    torch.cuda.synchronize()
    slice_us = 1e6 * (time.perf_counter() - t0) / (args.replays * T)
    epoch_ms = []
    for ep in range(args.episodes):
        graph.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.loss.compute_loss(agent.network, traj)
        torch.cuda.synchronize()
        epoch_ms.append(1e3 * (time.perf_counter() - t0) / agent.loss.n_epochs)
    timed = epoch_ms[2:] or epoch_ms
    print(f"deep_mlp_time E={E} 3-(128,128)-(4+1) [{kind}]: rollout {slice_us:.1f} us/slice "
          f"({args.replays} x {T} replayed slices), update {sum(timed) / len(timed):.3f} ms/epoch "
          f"(episodes {[round(v, 3) for v in epoch_ms]}, first two untimed)", flush=True)


if __name__ == "__main__":
    main()
