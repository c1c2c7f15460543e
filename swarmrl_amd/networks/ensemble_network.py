"""
An ensemble (population) of independent actor-critic MLPs in one module.

The reference trains N models with one process and one engine each
(swarmrl/training_routines/ensemble_submit.py:17-176).  Here the N networks
are the slices of six stacked parameters, member m owns a contiguous block
of the engine's envs, and one kernel launch serves every member: the rollout
policy through swarm_policy_ensemble_sample, the PPO gradient through
swarm_ppo_ensemble_epoch_grad (csrc/swarm_ensemble.cuh).  A member's results
are bit-identical to the single-model kernels on its slice, so a member
trained in an ensemble is the model it would have been trained alone with
the same seed and data.  One elementwise Adam over the stacked tensors is N
independent Adams.

EnsembleDeepActorCriticMLP is the same for DeepActorCriticMLP members (2 L + 4
stacked parameters; swarm_policy_deep_ensemble_sample and
swarm_ppo_deep_ensemble_epoch_grad for L = 2 or 3 within the deep kernels'
limits), and EnsembleTorchModel.select_members is the selection step of a
genetic routine (training_routines/genetic.py).
"""

import os

import numpy as np
import torch
from torch import nn

from swarmrl_amd.exploration_policies.random_exploration import RandomExploration
from swarmrl_amd.networks.torch_network import (ActorCriticMLP, DeepActorCriticMLP,
                                                deep_mlp_within_limits)
from swarmrl_amd.sampling_strategies.gumbel_distribution import GumbelDistribution

_NAMES = ("hidden.weight", "hidden.bias", "actor.weight", "actor.bias", "critic.weight",
          "critic.bias")


class EnsembleActorCriticMLP(nn.Module):
    """n_members independent ActorCriticMLPs (Dense(hidden) -> ReLU ->
    {Dense(n_actions) logits, Dense(1) value}) as six stacked parameters in
    torch Linear layouts: w1 [M, hidden, d], b1 [M, hidden], wa [M, k,
    hidden], ba [M, k], wc [M, 1, hidden], bc [M, 1].  Member m is
    initialised exactly as the m-th ActorCriticMLP constructed in order
    under the current torch RNG."""

    def __init__(self, n_members: int, input_dim: int, n_actions: int = 4, hidden: int = 128):
        super().__init__()
        if n_members < 1:
            raise ValueError("an ensemble needs at least one member")
        self.n_members = int(n_members)
        self.input_dim, self.n_actions, self.hidden_units = int(input_dim), int(n_actions), \
            int(hidden)
        members = [ActorCriticMLP(input_dim, n_actions, hidden) for _ in range(self.n_members)]
        self._stack(members)

    def _stack(self, members):
        stacked = [torch.stack([m.ppo_layers()[i].detach() for m in members])
                   for i in range(6)]
        self.w1, self.b1, self.wa, self.ba, self.wc, self.bc = (
            nn.Parameter(t.contiguous()) for t in stacked)

    @classmethod
    def from_members(cls, members):
        """The ensemble whose member m is a copy of members[m]."""
        members = list(members)
        first = members[0]
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.n_members = len(members)
        self.input_dim = int(first.hidden.in_features)
        self.n_actions = int(first.actor.out_features)
        self.hidden_units = int(first.hidden.out_features)
        shapes = [tuple(t.shape) for t in first.ppo_layers()]
        for m in members:
            if [tuple(t.shape) for t in m.ppo_layers()] != shapes:
                raise ValueError("ensemble members must have the same layer sizes")
        self._stack(members)
        return self

    def ppo_layers(self):
        """The stacked (w1, b1, wa, ba, wc, bc), the order of the ensemble
        PPO gradient (swarm_ppo_ensemble_epoch_grad)."""
        return (self.w1, self.b1, self.wa, self.ba, self.wc, self.bc)

    def rollout_layers(self):
        """The stacked (w1, b1, wa, ba) of the actor path
        (swarm_policy_ensemble_sample)."""
        return (self.w1, self.b1, self.wa, self.ba)

    def member(self, m: int) -> ActorCriticMLP:
        """A copy of member m as a stock ActorCriticMLP."""
        net = ActorCriticMLP(self.input_dim, self.n_actions, self.hidden_units)
        net.to(self.w1.device)
        with torch.no_grad():
            for dst, src in zip(net.ppo_layers(), self.ppo_layers()):
                dst.copy_(src[m])
        return net

    def set_member(self, m: int, module: ActorCriticMLP):
        """Overwrite member m's weights with the module's."""
        with torch.no_grad():
            for dst, src in zip(self.ppo_layers(), module.ppo_layers()):
                dst[m].copy_(src)

    def member_state_dict(self, m: int) -> dict:
        """Member m's weights under ActorCriticMLP's state-dict names."""
        return {name: t[m].detach().clone() for name, t in zip(_NAMES, self.ppo_layers())}

    def forward(self, x):
        """x [M, n, d] -> (logits [M, n, k], values [M, n, 1]) by batched
        matmul (the torch path; the kernels' reference in the tests).  The
        same products and bias adds as the members' Linear layers: equal to
        member(m)(x[m]) within fp32 rounding, and bit for bit where torch's
        batched and single products run the same GEMM (on the CPU from about
        25 rows per member on: below, bmm takes a loop of its own).  The
        one-column value head is the product W_c h^T, the form whose
        summation order matches Linear(hidden, 1)."""
        h = torch.relu(torch.bmm(x, self.w1.transpose(1, 2)) + self.b1.unsqueeze(1))
        logits = torch.bmm(h, self.wa.transpose(1, 2)) + self.ba.unsqueeze(1)
        values = torch.bmm(self.wc, h.transpose(1, 2)).transpose(1, 2) + self.bc.unsqueeze(1)
        return logits, values

    def reset_parameters(self):
        """Fresh members, drawn in order from the current torch RNG."""
        fresh = [ActorCriticMLP(self.input_dim, self.n_actions, self.hidden_units)
                 for _ in range(self.n_members)]
        with torch.no_grad():
            for i, dst in enumerate(self.ppo_layers()):
                dst.copy_(torch.stack([m.ppo_layers()[i].detach() for m in fresh]))


def _deep_names(n_hidden: int):
    names = []
    for l in range(n_hidden):
        names += [f"layers.{l}.weight", f"layers.{l}.bias"]
    return (*names, "actor.weight", "actor.bias", "critic.weight", "critic.bias")


def _deep_ppo_layers(module: DeepActorCriticMLP):
    """(w1, b1, ..., wL, bL, wa, ba, wc, bc) of a DeepActorCriticMLP."""
    ws, bs, wa, ba, wc, bc = module.deep_layers()
    return (*(t for pair in zip(ws, bs) for t in pair), wa, ba, wc, bc)


class EnsembleDeepActorCriticMLP(nn.Module):
    """n_members independent DeepActorCriticMLPs (L = len(hidden) hidden ReLU
    layers, then {Dense(n_actions) logits, Dense(1) value}) as 2 L + 4
    stacked parameters in torch Linear layouts: w_l [M, h_l, h_(l-1)],
    b_l [M, h_l] (h_0 = input_dim), wa [M, k, h_L], ba [M, k],
    wc [M, 1, h_L], bc [M, 1].  Member m is initialised exactly as the m-th
    DeepActorCriticMLP constructed in order under the current torch RNG."""

    def __init__(self, n_members: int, input_dim: int, n_actions: int = 4, hidden=(128, 128)):
        super().__init__()
        if n_members < 1:
            raise ValueError("an ensemble needs at least one member")
        self.n_members = int(n_members)
        self.input_dim, self.n_actions = int(input_dim), int(n_actions)
        self.hidden_widths = tuple(int(h) for h in hidden)
        members = [DeepActorCriticMLP(input_dim, n_actions, self.hidden_widths)
                   for _ in range(self.n_members)]
        self._stack(members)

    def _stack(self, members):
        per_member = [_deep_ppo_layers(m) for m in members]
        n_hidden = len(self.hidden_widths)
        names = [n for l in range(n_hidden) for n in (f"w{l + 1}", f"b{l + 1}")]
        names += ["wa", "ba", "wc", "bc"]
        for i, name in enumerate(names):  # registered in the order of ppo_layers()
            stacked = torch.stack([layers[i].detach() for layers in per_member])
            setattr(self, name, nn.Parameter(stacked.contiguous()))
        self._layer_names = tuple(names)

    @classmethod
    def from_members(cls, members):
        """The ensemble whose member m is a copy of members[m]."""
        members = list(members)
        first = members[0]
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.n_members = len(members)
        self.input_dim = int(first.layers[0].in_features)
        self.n_actions = int(first.actor.out_features)
        self.hidden_widths = tuple(int(layer.out_features) for layer in first.layers)
        shapes = [tuple(t.shape) for t in _deep_ppo_layers(first)]
        for m in members:
            if [tuple(t.shape) for t in _deep_ppo_layers(m)] != shapes:
                raise ValueError("ensemble members must have the same layer sizes")
        self._stack(members)
        return self

    def ppo_layers(self):
        """The stacked (w1, b1, ..., wL, bL, wa, ba, wc, bc), the order of
        the ensemble PPO gradient (swarm_ppo_deep_ensemble_epoch_grad)."""
        return tuple(getattr(self, name) for name in self._layer_names)

    def rollout_layers(self):
        """The stacked (ws, bs, wa, ba) of the actor path
        (swarm_policy_deep_ensemble_sample)."""
        layers = self.ppo_layers()
        return (list(layers[0:-4:2]), list(layers[1:-4:2]), layers[-4], layers[-3])

    def member(self, m: int) -> DeepActorCriticMLP:
        """A copy of member m as a stock DeepActorCriticMLP."""
        net = DeepActorCriticMLP(self.input_dim, self.n_actions, self.hidden_widths)
        net.to(self.wa.device)
        with torch.no_grad():
            for dst, src in zip(_deep_ppo_layers(net), self.ppo_layers()):
                dst.copy_(src[m])
        return net

    def set_member(self, m: int, module: DeepActorCriticMLP):
        """Overwrite member m's weights with the module's."""
        with torch.no_grad():
            for dst, src in zip(self.ppo_layers(), _deep_ppo_layers(module)):
                dst[m].copy_(src)

    def member_state_dict(self, m: int) -> dict:
        """Member m's weights under DeepActorCriticMLP's state-dict names."""
        return {name: t[m].detach().clone()
                for name, t in zip(_deep_names(len(self.hidden_widths)), self.ppo_layers())}

    def forward(self, x):
        """x [M, n, d] -> (logits [M, n, k], values [M, n, 1]) by batched
        matmul (the torch path; the kernels' reference in the tests), the
        products and bias adds of the members' Linear layers in their order;
        the value head in the form of EnsembleActorCriticMLP.forward."""
        layers = self.ppo_layers()
        h = x
        for w, b in zip(layers[0:-4:2], layers[1:-4:2]):
            h = torch.relu(torch.bmm(h, w.transpose(1, 2)) + b.unsqueeze(1))
        wa, ba, wc, bc = layers[-4:]
        logits = torch.bmm(h, wa.transpose(1, 2)) + ba.unsqueeze(1)
        values = torch.bmm(wc, h.transpose(1, 2)).transpose(1, 2) + bc.unsqueeze(1)
        return logits, values

    def reset_parameters(self):
        """Fresh members, drawn in order from the current torch RNG."""
        fresh = [_deep_ppo_layers(DeepActorCriticMLP(self.input_dim, self.n_actions,
                                                     self.hidden_widths))
                 for _ in range(self.n_members)]
        with torch.no_grad():
            for i, dst in enumerate(self.ppo_layers()):
                dst.copy_(torch.stack([layers[i].detach() for layers in fresh]))


def _is_deep(model) -> bool:
    return hasattr(model, "hidden_widths")


class EnsembleTorchModel:
    """The TorchModel surface the agent and the loss use, for an
    EnsembleActorCriticMLP or an EnsembleDeepActorCriticMLP.  The flat batch
    [E * A, d] an agent builds is member-major: with E envs and M members, member m owns envs
    [m E/M, (m + 1) E/M), so rows [m n_per, (m + 1) n_per), n_per = (E/M) A."""

    # the one-launch observable + policy and the ride-along build stay
    # single-model: the observable runs first, then the ensemble policy
    accepts_engine = False

    def __init__(
        self,
        torch_model: nn.Module,
        input_shape: tuple = None,
        optimizer=None,
        exploration_policy=RandomExploration(probability=0.0),
        sampling_strategy=GumbelDistribution(),
        rng_key: int = None,
        deployment_mode: bool = False,
        device=None,
        learning_rate: float = 1e-3,
    ):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) \
                if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        if rng_key is not None:
            torch.manual_seed(int(rng_key))
        self.model = torch_model.to(self.device)
        self.n_members = int(torch_model.n_members)
        self.input_shape = input_shape
        self.sampling_strategy = sampling_strategy
        self.exploration_policy = exploration_policy
        self.deployment_mode = deployment_mode
        if optimizer is None:
            # the same fused capturable Adam as TorchModel: elementwise, so
            # one step over the stacked tensors is n_members independent Adams
            fused = self.device.type == "cuda"
            optimizer = lambda params: torch.optim.Adam(  # noqa: E731
                params, lr=learning_rate, fused=fused, capturable=fused)
        self._optimizer_factory = optimizer
        self.optimizer = None if deployment_mode else optimizer(self.model.parameters())
        self.epoch_count = 0
        self.generator = None
        # per-member Philox seeds, drawn in member order the way
        # TorchModel.__init__ draws its one
        self.member_seeds = [int(torch.randint(0, 2**62, (1,)).item())
                             for _ in range(self.n_members)]
        self._seeds = None  # the seeds on the device
        self._fused_state = None  # [M, ceil(n_per / 64)] call counters

    def reinitialize_network(self):
        self.model.reset_parameters()
        self.optimizer = self._optimizer_factory(self.model.parameters())

    def __call__(self, features: torch.Tensor, obs_ndim: int = 1):
        """Forward over member-major features [M, ..., *obs]; the trailing
        obs_ndim dims are flattened per sample.  Returns (logits, values)
        with the leading dims of the input."""
        lead = features.shape[: features.ndim - obs_ndim]
        x = features.reshape(lead[0], -1, int(np.prod(features.shape[len(lead):])))
        logits, values = self.model(x.to(torch.float32))
        return logits.reshape(*lead, -1), values.reshape(*lead, 1)

    def _member_major(self, obs: torch.Tensor) -> torch.Tensor:
        if obs.shape[0] % self.n_members != 0:
            raise ValueError(f"{obs.shape[0]} observations do not divide among "
                             f"{self.n_members} ensemble members")
        return obs.reshape(self.n_members, obs.shape[0] // self.n_members, -1)

    @torch.no_grad()
    def compute_action(self, observables):
        """(indices, log_probs) for every agent of the flat member-major
        batch through torch; tensors in -> tensors out."""
        host = not isinstance(observables, torch.Tensor)
        if host:
            obs = torch.as_tensor(np.asarray(observables, dtype=np.float32), device=self.device)
        else:
            obs = observables.to(torch.float32)
        obs = self._member_major(obs.reshape(obs.shape[0], -1))
        logits, _ = self.model(obs)
        logits = logits.reshape(-1, logits.shape[-1])
        indices = self.sampling_strategy(logits, generator=self.generator)
        log_probs = torch.log(torch.softmax(logits, dim=-1) + 1e-8)
        indices = self.exploration_policy(indices, logits.shape[-1], generator=self.generator)
        chosen = torch.gather(log_probs, 1, indices.reshape(-1, 1)).reshape(-1)
        if host:
            return indices.cpu().numpy(), chosen.cpu().numpy()
        return indices, chosen

    def fused_sampling_ok(self, observables) -> bool:
        """The one-kernel ensemble policy applies: stock Gumbel sampling and
        random exploration, device tensors and parameters, sizes within
        swarm_policy_ensemble_sample's limits (a deep ensemble:
        swarm_policy_deep_ensemble_sample's)."""
        if os.environ.get("SWARMRL_AMD_FUSED_ENSEMBLE", "1") == "0":
            return False
        if not (isinstance(observables, torch.Tensor) and observables.is_cuda
                and type(self.sampling_strategy) is GumbelDistribution
                and type(self.exploration_policy) is RandomExploration):
            return False
        m = self.model
        if _is_deep(m):
            sizes_ok = deep_mlp_within_limits(m.input_dim, m.hidden_widths, m.n_actions)
        else:
            sizes_ok = m.input_dim <= 16 and m.hidden_units <= 256 and m.n_actions <= 16
        return (m.wa.is_cuda and sizes_ok and self.n_members <= 1024
                and observables.shape[0] % self.n_members == 0)

    @torch.no_grad()
    def compute_action_fused(self, observables: torch.Tensor, f_table: torch.Tensor,
                             t_table: torch.Tensor):
        """Every member's compute_action + action-table lookup in one launch
        (swarm_policy_ensemble_sample, or swarm_policy_deep_ensemble_sample
        for a deep ensemble): (indices, log_probs, f_swim, torque_z) for the
        flat member-major batch."""
        from swarmrl_amd.engine import ops

        obs = observables.to(torch.float32)
        obs = obs.reshape(obs.shape[0], -1)
        if obs.shape[0] % self.n_members != 0:
            raise ValueError(f"{obs.shape[0]} observations do not divide among "
                             f"{self.n_members} ensemble members")
        n_per = obs.shape[0] // self.n_members
        self._member_counters(n_per, obs.device)
        p = float(self.exploration_policy.probability)
        sample = ops.policy_deep_ensemble_sample if _is_deep(self.model) \
            else ops.policy_ensemble_sample
        return sample(obs, *self.model.rollout_layers(), self._seeds, self._fused_state, p,
                      f_table, t_table)

    def _member_counters(self, n_per: int, device):
        """The seeds on the device and [M, ceil(n_per / 64)] call counters
        (grown, never shrunk; a member's existing groups keep their counts)."""
        if self._seeds is None or self._seeds.device != device:
            self._seeds = torch.tensor(self.member_seeds, dtype=torch.int64, device=device)
        need = max(1, (n_per + 63) // 64)
        st = self._fused_state
        if st is None or st.device != device:
            self._fused_state = torch.zeros(self.n_members, need, dtype=torch.int64,
                                            device=device)
        elif st.shape[1] < need:
            grown = torch.zeros(self.n_members, need, dtype=torch.int64, device=device)
            grown[:, : st.shape[1]] = st
            self._fused_state = grown

    def fused_policy_args(self, n: int, d_in: int, k: int, device):
        """None: the one-launch observable + policy is single-model."""
        return None

    def ppo_layers(self, d_in: int):
        """The stacked layers when the fused ensemble PPO gradient applies
        (fp32 contiguous device parameters within
        swarm_ppo_ensemble_epoch_grad's limits, or for a deep ensemble
        swarm_ppo_deep_ensemble_epoch_grad's), else None."""
        if self.optimizer is None:
            return None
        layers = self.model.ppo_layers()
        ok = all(t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() for t in layers)
        ok = ok and self.model.input_dim == d_in and d_in <= 32
        if _is_deep(self.model):
            ok = ok and deep_mlp_within_limits(d_in, self.model.hidden_widths,
                                               self.model.n_actions)
        else:
            ok = ok and self.model.hidden_units <= 256 and self.model.n_actions <= 16
        ok = ok and self.n_members <= 1024
        return layers if ok else None

    def apply_gradients(self, layers, flat_grad: torch.Tensor):
        """One optimizer step with the gradient given as the concatenation of
        the stacked layers' gradients (swarm_ppo_ensemble_epoch_grad and its
        deep twin)."""
        self.optimizer.zero_grad(set_to_none=True)
        off = 0
        for t in layers:
            n = t.numel()
            t.grad = flat_grad[off:off + n].view_as(t)
            off += n
        self.optimizer.step()
        self.epoch_count += 1

    def update_model(self, loss: torch.Tensor):
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        self.epoch_count += 1

    def export_model(self, filename: str = "model", directory: str = "Models"):
        os.makedirs(directory, exist_ok=True)
        torch.save(
            {
                "model": self.model.state_dict(),
                "optimizer": self.optimizer.state_dict() if self.optimizer else None,
                "epoch": self.epoch_count,
                "member_seeds": list(self.member_seeds),
            },
            os.path.join(directory, filename + ".pt"),
        )

    def restore_model_state(self, filename, directory):
        state = torch.load(os.path.join(directory, filename + ".pt"), weights_only=True,
                           map_location=self.device)
        self.model.load_state_dict(state["model"])
        if self.optimizer is not None and state["optimizer"] is not None:
            self.optimizer.load_state_dict(state["optimizer"])
        self.epoch_count = int(state["epoch"])

    def _member_optimizer_state(self, m: int):
        """Member m's Adam state in the form a stock TorchModel's optimizer
        loads (parameters in the member module's order, which is that of
        ppo_layers()), or None."""
        if self.optimizer is None:
            return None
        full = self.optimizer.state_dict()
        state = {}
        layers = self.model.ppo_layers()
        for i, p in enumerate(layers):
            st = self.optimizer.state.get(p)
            if not st:
                continue
            state[i] = {}
            for key, v in st.items():  # the moments per member, the step count shared
                if isinstance(v, torch.Tensor):
                    v = (v[m] if v.shape == p.shape else v).detach().clone()
                state[i][key] = v
        groups = [{**{k: v for k, v in g.items() if k != "params"},
                   "params": list(range(len(layers)))}
                  for g in full["param_groups"][:1]]
        return {"state": state, "param_groups": groups}

    def export_member(self, m: int, filename: str = "model", directory: str = "Models"):
        """Write member m alone, in the file format of TorchModel.export_model:
        a stock TorchModel(ActorCriticMLP(...)) -- for a deep ensemble
        TorchModel(DeepActorCriticMLP(...)) -- restores it with
        restore_model_state, so a trained member can be deployed alone."""
        if not 0 <= m < self.n_members:
            raise IndexError(f"member {m} of {self.n_members}")
        os.makedirs(directory, exist_ok=True)
        torch.save(
            {
                "model": self.model.member_state_dict(m),
                "optimizer": self._member_optimizer_state(m),
                "epoch": self.epoch_count,
            },
            os.path.join(directory, filename + ".pt"),
        )

    @torch.no_grad()
    def copy_member(self, src: int, dst: int, with_optimizer_state: bool = True):
        """Overwrite member dst's weights (and Adam moments) with member
        src's: the primitive of a genetic selection.  The members keep their
        own sampling seeds and counters."""
        for p in self.model.ppo_layers():
            p[dst].copy_(p[src])
            st = self.optimizer.state.get(p) if self.optimizer is not None else None
            if with_optimizer_state and st:
                for v in st.values():
                    if isinstance(v, torch.Tensor) and v.shape == p.shape:
                        v[dst].copy_(v[src])

    @torch.no_grad()
    def select_members(self, parent_of, with_optimizer_state: bool = True):
        """Member i becomes a copy of member parent_of[i] (weights and, with
        with_optimizer_state, Adam moments): one gather over every stacked
        tensor, so a member that is both a source and a destination is read
        before it is overwritten -- parent_of = [1, 0, 0] swaps members 0 and
        1, which sequential copy_member calls do not.  The copies are in
        place: a captured PPO graph stays valid.  Sampling seeds and call
        counters stay with the slot."""
        parent_of = [int(i) for i in parent_of]
        if len(parent_of) != self.n_members:
            raise ValueError(f"{len(parent_of)} parents for {self.n_members} members")
        if any(not 0 <= i < self.n_members for i in parent_of):
            raise IndexError(f"parents must be members 0..{self.n_members - 1}")
        for p in self.model.ppo_layers():
            index = torch.tensor(parent_of, dtype=torch.long, device=p.device)
            p.copy_(p.index_select(0, index))
            st = self.optimizer.state.get(p) if self.optimizer is not None else None
            if with_optimizer_state and st:
                for v in st.values():
                    if isinstance(v, torch.Tensor) and v.shape == p.shape:
                        v.copy_(v.index_select(0, index))
