from swarmrl_amd.networks.ensemble_network import (EnsembleActorCriticMLP,
                                                    EnsembleDeepActorCriticMLP,
                                                    EnsembleTorchModel)
from swarmrl_amd.networks.torch_network import (ActorCriticMLP, DeepActorCriticMLP,
                                                 TorchModel)

__all__ = ["ActorCriticMLP", "DeepActorCriticMLP", "TorchModel", "EnsembleActorCriticMLP",
           "EnsembleDeepActorCriticMLP", "EnsembleTorchModel"]
