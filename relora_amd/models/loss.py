"""Runtime loss options of the causal-LM heads (z-loss, label smoothing).

The options live on the model object, not in its config, so `config.json`
and HF checkpoint interchange are untouched.  They apply in training mode
only: evaluation always reports plain cross-entropy, which is what
perplexity is computed from.

Per valid token, with logits x, target t, lse = log sum exp x, smoothing eps
and z coefficient z:

    loss = lse - (1-eps)*x_t - (eps/V)*sum_j x_j + z*lse^2
"""

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F
from transformers.modeling_outputs import CausalLMOutputWithPast

from relora_amd import ops


@dataclass
class CausalLMLossOutput(CausalLMOutputWithPast):
    """CausalLMOutputWithPast plus the two detached by-products of a loss
    with options on: `ce_loss` (plain cross-entropy) and `z_loss`
    (z * mean(lse^2)).  Both are None when the options are off or unused."""

    ce_loss: Optional[torch.Tensor] = None
    z_loss: Optional[torch.Tensor] = None


class LossOptionsMixin:
    """`set_loss_options` plus the two attributes it sets, default 0."""

    z_loss = 0.0
    label_smoothing = 0.0

    def set_loss_options(self, z_loss=0.0, label_smoothing=0.0):
        z_loss, label_smoothing = float(z_loss), float(label_smoothing)
        if not z_loss >= 0.0:
            raise ValueError(f"z_loss must be >= 0, got {z_loss}")
        if not 0.0 <= label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
        self.z_loss = z_loss
        self.label_smoothing = label_smoothing
        return self

    def _active_loss_options(self):
        """(z, eps) to apply to this forward: the set values while training,
        (0, 0) in eval mode."""
        if not self.training:
            return 0.0, 0.0
        return self.z_loss, self.label_smoothing


def fused_lm_loss(shift_hidden, weight, shift_labels, z_loss, label_smoothing):
    """(loss, ce_loss, z_loss_term) through the fused chunked CE op; the two
    parts are None with the options off."""
    if z_loss == 0.0 and label_smoothing == 0.0:
        return ops.fused_cross_entropy(shift_hidden, weight, shift_labels), None, None
    return ops.fused_cross_entropy(
        shift_hidden, weight, shift_labels, z_loss=z_loss,
        label_smoothing=label_smoothing, return_parts=True)


def unfused_lm_loss(logits, labels, z_loss, label_smoothing):
    """The same objective from materialised [M, V] logits with torch ops (the
    path for fused_ce=False, a wrapped lm_head or a head with a bias).  Labels
    of -100 are ignored, as in the fused op and F.cross_entropy."""
    ignore_index = -100
    if z_loss == 0.0 and label_smoothing == 0.0:
        return F.cross_entropy(logits, labels), None, None
    # fp32 throughout, like the fused op: a bf16 loss near ln(V) ~ 10 is only
    # good to 2^-5, which would drown the terms added here
    logits = logits.float()
    loss = F.cross_entropy(logits, labels, ignore_index=ignore_index,
                           label_smoothing=label_smoothing)
    valid = labels != ignore_index
    n_valid = valid.sum().clamp_min(1)
    lse = torch.logsumexp(logits, dim=-1)
    zl = z_loss * torch.where(valid, lse * lse, torch.zeros_like(lse)).sum() / n_valid
    with torch.no_grad():
        ce = F.cross_entropy(logits, labels, ignore_index=ignore_index)
    return loss + zl, ce.detach(), zl.detach()
