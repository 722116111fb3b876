"""The critic of the reference's actor-critic trainers (rl4co/models/rl/common/critic.py:13-77): a copy of the policy's encoder
plus a value head, `value_head(encoder(td)[0]).mean(1)` -> [B, 1].  Used by PPO (`train.PPOStep`, rl/ppo/ppo.py:82-85,183) and by
the critic baseline of REINFORCE (`train.reinforce_loss(baseline="critic")`, rl/reinforce/baselines.py:140-159).

Names, defaults and state-dict keys are the reference's: `encoder.*`, `value_head.0.{weight,bias}`, `value_head.2.{weight,bias}`.

Where it runs: without autograd the encoder's own forward (the fused kernel where it applies); under autograd the very
autograd functions of the policy's training graph (`train.encode_autograd`: the library's GEMMs, self-attention and norms with
their native backward kernels).  The value head's first layer (E -> hidden, ReLU) is `train._linear`; the second (hidden -> 1)
is taken AFTER the mean over the nodes -- it is linear, so mean_n (W h_n + b) = W mean_n h_n + b up to rounding, and the
[B * M, hidden] x [hidden, 1] product shrinks to [B, hidden] x [hidden, 1].  There is no value-head kernel: the [B * M, hidden]
round trip is small next to the three encoder layers in front of it.
"""
from __future__ import annotations

import copy
import logging
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

log = logging.getLogger(__name__)


class CriticNetwork(nn.Module):
    """critic.py:13-62.  encoder: an `AttentionModelEncoder` (anything else, like customized=True, is not built)."""

    def __init__(self, encoder: nn.Module, value_head: Optional[nn.Module] = None, embed_dim: int = 128,
                 hidden_dim: int = 512, customized: bool = False):
        super().__init__()
        from .policy import AttentionModelEncoder

        if customized:
            raise NotImplementedError("CriticNetwork(customized=True): a customized encoder / value head with a hidden input "
                                      "is not built for MI355X")
        if not isinstance(encoder, AttentionModelEncoder):
            raise NotImplementedError(f"CriticNetwork: the encoder must be an AttentionModelEncoder, got {type(encoder).__name__} "
                                      "(its training graph is what train.encode_autograd builds)")
        self.encoder = encoder
        if value_head is None:
            # check if embed dim of encoder is different, if so, use it
            if getattr(encoder, "embed_dim", embed_dim) != embed_dim:
                log.warning("Found encoder with different embed_dim %s than the value head %s. Using encoder embed_dim for "
                            "value head.", encoder.embed_dim, embed_dim)
                embed_dim = getattr(encoder, "embed_dim", embed_dim)
            value_head = nn.Sequential(nn.Linear(embed_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, 1))
        self.value_head = value_head
        self.customized = customized

    @property
    def env_name(self) -> str:
        """(what `train.encode_autograd` reads next to `.encoder` and `.training`)"""
        return self.encoder.env_name

    def _standard_head(self) -> bool:
        vh = self.value_head
        return (isinstance(vh, nn.Sequential) and len(vh) == 3 and isinstance(vh[0], nn.Linear) and isinstance(vh[1], nn.ReLU)
                and isinstance(vh[2], nn.Linear))

    def forward(self, x, hidden=None) -> torch.Tensor:
        """td -> value [B, 1]"""
        locs = x["locs"]
        if not locs.is_cuda:
            raise RuntimeError(f"TensorDict is on {locs.device}: the eam_rl4co_amd critic runs only on an MI355X (HIP) device; "
                               "there is no CPU fallback. Use td.to('cuda').")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            from .train import _linear, encode_autograd

            h = encode_autograd(self, x)
            if self._standard_head():
                l0, l2 = self.value_head[0], self.value_head[2]
                return F.linear(_linear(h, l0.weight, l0.bias, relu=True).mean(1), l2.weight, l2.bias)
        else:
            h, _ = self.encoder(x)
        return self.value_head(h).mean(1)


def create_critic_from_actor(policy: nn.Module, backbone: str = "encoder", **critic_kwargs) -> CriticNetwork:
    """critic.py:65-77: the critic re-uses (a deep copy of) the policy's backbone."""
    encoder = getattr(policy, backbone, None)
    if encoder is None:
        raise ValueError(f"CriticBaseline requires a backbone in the policy network: {backbone}")
    return CriticNetwork(copy.deepcopy(encoder), **critic_kwargs).to(next(policy.parameters()).device)
