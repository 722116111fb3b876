"""eam_rl4co_amd: MI355X-native construction rollout (TSP / CVRP and the sibling routing envs CVRPTW, SDVRP, PCTSP, OP
+ AttentionModel decode) behind the RL4CO interfaces of Tarseus/eam-rl4co.  See DESIGN.md."""
from .envs import (CVRPEnv, CVRPGenerator, CVRPTWEnv, CVRPTWGenerator, OPEnv, OPGenerator, PCTSPEnv, PCTSPGenerator, PDPEnv, PDPGenerator, RL4COEnvBase, SDVRPEnv, SPCTSPEnv,  # noqa: F401
                   TSPEnv, TSPGenerator, get_env)  # noqa: F401
from .policy import (AttentionModelDecoder, AttentionModelEncoder, AttentionModelPolicy, GraphedRollout,  # noqa: F401
                     GraphHeterogeneousAttentionEncoder, HeterogeneousAttentionModelPolicy, PolyNetDecoder, PolyNetPolicy,
                     SymNCOPolicy,
                     load_reference_checkpoint, random_policy, rollout)
from .ptrnet import PointerNetworkPolicy  # noqa: F401
from .attention import PointerAttention, PolyNetAttention, scaled_dot_product_attention  # noqa: F401
from .evolution import EA, EACvrpDraws, EAPrizeDraws, EADraws, evolution_worker, generate_batch_population  # noqa: F401
from .search import EAS, EASEmb, EASLay, eas_loss_coefficients  # noqa: F401
from .critic import CriticNetwork, create_critic_from_actor  # noqa: F401
from .train import PPOStep, ppo_loss_terms  # noqa: F401
from .baselines import (REINFORCE_BASELINES_REGISTRY, CriticBaseline, ExponentialBaseline, MeanBaseline, NoBaseline,  # noqa: F401
                        REINFORCEBaseline, RewardScaler, RolloutBaseline, SharedBaseline, WarmupBaseline,
                        get_reinforce_baseline, paired_ttest)
from .train import PolicyGradientStep, eam_am_loss, fit, reinforce_loss  # noqa: F401
from .envs import ExtraKeyDataset, TensorDictDataset  # noqa: F401
from .tensordict_lite import TensorDict  # noqa: F401
from .utils import batchify, gather_by_index, unbatchify  # noqa: F401

__version__ = "0.1.0"
