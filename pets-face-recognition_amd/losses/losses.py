"""FocalLoss with the reference's signature (/root/reference/losses/losses.py:7-28):
`FocalLoss(num_class, gamma=0, eps=1e-7, alpha=None)`; loss = mean((1 − p_t)^γ · CE).  With the defaults every FE
config uses (γ = 0, α = None) it is the mean cross-entropy."""
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F


class Criterion(namedtuple("Criterion", "gamma alpha weight smoothing reduction")):
    """What the fused head (losses/_head_hip.py) needs to know of the criterion: focal gamma, the learnable alpha [C] of
    FocalLoss(alpha=True) or None, nn.CrossEntropyLoss's class weight [C] or None, its label smoothing and its reduction."""
    __slots__ = ()

    @property
    def is_plain(self):
        return self.alpha is None and self.weight is None and self.smoothing == 0.0 and self.reduction == "mean"


def _class_vector_ok(v, num_class, device):
    return v.dtype == torch.float32 and v.dim() == 1 and v.shape[0] == num_class and v.device == device


def describe_criterion(fl, num_class, device):
    """Criterion of a FocalLoss / nn.CrossEntropyLoss module as the fused head runs it on `device`, or None when it does not:
    reduction='none' (the controller needs a scalar), a non-default ignore_index (the reference's one_hot.scatter_ cannot take an ignored
    label anyway), alpha / weight that are not fp32 [num_class] tensors on `device`, a subclass of nn.CrossEntropyLoss."""
    if isinstance(fl, FocalLoss):
        if not fl.adaptive_flag:
            return Criterion(float(fl.gamma), None, None, 0.0, "mean")
        if _class_vector_ok(fl.alpha, num_class, device):
            return Criterion(float(fl.gamma), fl.alpha, None, 0.0, "mean")
        return None
    if type(fl) is nn.CrossEntropyLoss:
        e = float(getattr(fl, "label_smoothing", 0.0))
        if fl.reduction not in ("mean", "sum") or fl.ignore_index != -100 or not 0.0 <= e <= 1.0:
            return None
        if fl.weight is not None and not _class_vector_ok(fl.weight, num_class, device):
            return None
        return Criterion(0.0, None, None if fl.weight is None else fl.weight.detach(), e, fl.reduction)
    return None


class FocalLoss(nn.Module):
    def __init__(self, num_class: int, gamma=0, eps=1e-7, alpha=None):
        super().__init__()
        self.gamma, self.eps = gamma, eps
        self.adaptive_flag = bool(alpha)
        if self.adaptive_flag:
            self.alpha = nn.Parameter(torch.ones(num_class))

    def reset_parameters(self):
        if self.adaptive_flag:
            nn.init.ones_(self.alpha)

    def forward(self, input, target):
        if input.is_cuda:   # alpha goes into the kernel (z = alpha·input is never materialised); its gradient comes back through autograd
            from ._head_hip import FocalCEFunction
            if not self.adaptive_flag or (input.dim() == 2 and _class_vector_ok(self.alpha, input.shape[1], input.device)):
                return FocalCEFunction.apply(input, target, float(self.gamma), self.alpha if self.adaptive_flag else None)
            return FocalCEFunction.apply(self.alpha * input, target, float(self.gamma))
        if self.adaptive_flag:
            input = self.alpha * input
        ce = F.cross_entropy(input, target, reduction="none")
        pt = torch.exp(-ce)
        return ((1 - pt) ** self.gamma * ce).mean()
