from swarmrl_amd.networks.torch_network import (ActorCriticMLP, DeepActorCriticMLP,
                                                 TorchModel)

__all__ = ["ActorCriticMLP", "DeepActorCriticMLP", "TorchModel"]
