"""
PPO for an ensemble of independent actor-critic MLPs (EnsembleTorchModel).

The episode [T, E, A, ...] of an engine whose E envs are split among M
members (member m: envs [m E/M, (m + 1) E/M)) is repacked once to
member-major [M, T, (E/M) A, ...]; each of the n_epochs steps is then one
ensemble gradient (swarm_ppo_ensemble_epoch_grad: every member's GAE,
advantage normalisation and gradient in four launches) and one optimizer
step over the stacked parameters.  The loss is the sum over the members of
ProximalPolicyLoss._calculate_loss on the member's slice, so member m's
gradient is the one a stock network gets from its slice alone -- from the
kernels bit for bit (csrc/swarm_ensemble.cuh).
"""

import os

import torch

from swarmrl_amd.engine import ops
from swarmrl_amd.losses.proximal_policy_loss import ProximalPolicyLoss, _stack


class EnsembleProximalPolicyLoss(ProximalPolicyLoss):
    """ProximalPolicyLoss for a network with n_members stacked members."""

    def member_major(self, network, episode_data):
        """(features [M, T, S, d...], actions, old_log_probs, rewards
        [M, T, S]) of the episode, S = (E / M) A agent columns per member."""
        dev = network.device
        M = int(network.n_members)
        old_log_probs = _stack(episode_data.log_probs, dev).float()
        features = _stack(episode_data.features, dev).float()
        actions = _stack(episode_data.actions, dev).long()
        rewards = _stack(episode_data.rewards, dev).float()
        if actions.ndim == 2:  # [T, A]: one env
            actions, old_log_probs = actions.unsqueeze(1), old_log_probs.unsqueeze(1)
            features, rewards = features.unsqueeze(1), rewards.unsqueeze(1)
        T, E, A = actions.shape
        if E % M != 0:
            raise ValueError(f"{E} envs do not divide among {M} ensemble members")

        def pack(t):  # [T, E, A, ...] -> [M, T, (E / M) A, ...]
            rest = t.shape[3:]
            t = t.reshape(T, M, E // M, A, *rest).permute(1, 0, 2, 3, *range(4, 4 + len(rest)))
            return t.reshape(M, T, (E // M) * A, *rest).contiguous()

        return pack(features), pack(actions), pack(old_log_probs), pack(rewards)

    def _ensemble_loss(self, network, features, actions, rewards, old_log_probs):
        """The torch path: the sum over the members of _calculate_loss, each
        on its slice of one batched forward."""
        obs_ndim = features.ndim - 3
        logits, values = network(features, obs_ndim=obs_ndim)
        total = 0.0
        for m in range(int(network.n_members)):
            member = lambda f, obs_ndim, m=m: (logits[m], values[m])  # noqa: E731
            total = total + self._calculate_loss(member, features[m], actions[m], rewards[m],
                                                 old_log_probs[m])
        return total

    def compute_loss(self, network, episode_data):
        features, actions, old_log_probs, rewards = self.member_major(network, episode_data)
        layers = self._fused_ensemble_layers(network, features, actions)
        if layers is not None:
            features = features.reshape(*features.shape[:3], -1).contiguous()
            if self._graph_epochs(network, layers, features, actions, old_log_probs, rewards):
                return
        for _ in range(self.n_epochs):
            if layers is not None:
                grad = ops.ppo_ensemble_epoch_grad(
                    features, actions, old_log_probs, rewards, layers,
                    self.value_function.gamma, self.value_function.lambda_, self.epsilon,
                    self.entropy_coefficient, workspaces=self._workspaces())
                network.apply_gradients(layers, grad)
                continue
            loss = self._ensemble_loss(network, features, actions, rewards, old_log_probs)
            network.update_model(loss)

    def _graph_epochs(self, network, layers, features, actions, old_log_probs, rewards):
        """The n_epochs ensemble steps (gradient launches + the optimizer's
        own step over the stacked tensors) as one captured HIP graph, replayed
        per episode: the mechanism of ProximalPolicyLoss._graph_epochs.  The
        single model's fused-Adam launch is never used (its segment sizes are
        the single model's).  Returns False when the eager loop should run."""
        opt = getattr(network, "optimizer", None)
        if os.environ.get("SWARMRL_AMD_PPO_GRAPH", "1") == "0" or opt is None:
            return False
        if not all(g.get("capturable", False) for g in opt.param_groups):
            return False
        states = [opt.state.get(p, {}) for p in layers]
        if not all(states) or any(p.grad is None for p in layers):
            return False  # optimizer state not initialised yet: first episode is eager
        sig = (id(network), id(opt), tuple(features.shape), tuple(actions.shape),
               tuple((float(g["lr"]), tuple(float(b) for b in g.get("betas", ())),
                      float(g.get("eps", 0.0)), float(g.get("weight_decay", 0.0)),
                      bool(g.get("amsgrad", False)), bool(g.get("maximize", False)))
                     for g in opt.param_groups),
               tuple(t.data_ptr() for st in states for t in st.values()
                     if isinstance(t, torch.Tensor)),
               tuple(p.data_ptr() for p in layers), self.n_epochs,
               self.value_function.gamma, self.value_function.lambda_, self.epsilon,
               self.entropy_coefficient)
        cache = getattr(self, "_ppo_graph", None)
        if cache is None or cache["sig"] != sig:
            cache = None
            self._ppo_graph = None
            x = features.clone()
            act = actions.to(torch.int64).clone()
            olp = old_log_probs.to(torch.float32).clone()
            rew = rewards.to(torch.float32).clone()
            grad = torch.zeros(sum(p.numel() for p in layers), dtype=torch.float32,
                               device=features.device)
            off = 0
            for p in layers:
                p.grad = grad[off:off + p.numel()].view_as(p)
                off += p.numel()
            args = (x, act, olp, rew, layers, self.value_function.gamma,
                    self.value_function.lambda_, self.epsilon, self.entropy_coefficient)
            ws = self._workspaces()
            # sizes the workspace outside the capture
            ops.ppo_ensemble_epoch_grad(*args, out=grad, workspaces=ws)
            torch.cuda.synchronize(features.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                for _ in range(self.n_epochs):
                    ops.ppo_ensemble_epoch_grad(*args, out=grad, workspaces=ws)
                    opt.step()
            cache = self._ppo_graph = {"sig": sig, "graph": graph, "inputs": (x, act, olp, rew),
                                       "grad": grad}
        x, act, olp, rew = cache["inputs"]
        x.copy_(features)
        act.copy_(actions)
        olp.copy_(old_log_probs)
        rew.copy_(rewards)
        cache["graph"].replay()
        if hasattr(network, "epoch_count"):
            network.epoch_count += self.n_epochs
        return True

    def _fused_ensemble_layers(self, network, features, actions):
        """The stacked layers when the epoch gradient runs as the ensemble
        kernels: device tensors, stock GAE and entropy, sizes within the
        kernels' limits; else None (the torch path).
        SWARMRL_AMD_FUSED_ENSEMBLE=0 forces the torch path."""
        if os.environ.get("SWARMRL_AMD_FUSED_ENSEMBLE", "1") == "0":
            return None
        # [T, S, ...] of one member: the single-model conditions
        return self._fused_layers(network, features[0], actions[0])
