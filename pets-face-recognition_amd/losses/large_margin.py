"""Cosine-margin classification heads with the reference's constructor signatures and parameter names.

API mirrored: /root/reference/losses/large_margin.py — `AddMarginProduct(in_features, out_features, s=30.0, m=0.40)`
(CosFace, lines 10-40) and `ArcMarginProduct(in_features, out_features, s=30.0, m=0.50, easy_margin=False)`
(ArcFace, lines 44-84); `.weight` is `(out_features, in_features)`, Xavier-uniform.

Beyond the reference: `sub_centers=K` (Sub-center ArcFace, Deng et al., ECCV 2020) gives every class K centres, `.weight` is then
`(out_features * K, in_features)` with row `c*K + k` the k-th centre of class c, and the class cosine is the maximum of its K
sub-cosines.  K = 1 (the default) is the reference's head, bit for bit.

CUDA inputs run on the gfx950 kernels (losses/_head_hip.py); CPU inputs run the same arithmetic with torch ops."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class _MarginHead(nn.Module):
    _mode = None

    def __init__(self, in_features, out_features, s, m, sub_centers=1):
        super().__init__()
        sub_centers = int(sub_centers)
        if not 1 <= sub_centers <= 16:
            raise ValueError(f"sub_centers must be in 1..16, got {sub_centers}")
        self.in_features, self.out_features = in_features, out_features
        self.sub_centers = sub_centers
        self.s, self.m = s, m
        self.weight = nn.Parameter(torch.empty(out_features * sub_centers, in_features))
        nn.init.xavier_uniform_(self.weight)
        self.compute_dtype = None  # HIP compute dtype (None → PFR_COMPUTE_DTYPE / bf16)
        if sub_centers > 1:
            # how often each sub-centre was the one its class's samples landed on (training-mode forwards); not part of the
            # state dict, whose keys stay the reference's
            self.register_buffer("sub_center_count", torch.zeros(out_features, sub_centers, dtype=torch.int32), persistent=False)

    def _count(self):
        """the histogram the next forward adds to: training mode with K > 1 only"""
        return self.sub_center_count if self.sub_centers > 1 and self.training else None

    def reset_sub_center_count(self):
        if self.sub_centers > 1:
            self.sub_center_count.zero_()

    def dominant_sub_centers(self, group=None):
        """[out_features] long: per class the sub-centre most of its samples selected, the lowest index on ties.
        Every data-parallel rank counts its own share of the batches (the histogram is an integer buffer, which the gradient
        reducers do not synchronise): when torch.distributed is initialised the counts are summed over `group` first, so this is a
        collective that every rank must call, and every rank gets the same answer."""
        K = self.sub_centers
        if K == 1:
            return torch.zeros(self.out_features, dtype=torch.long, device=self.weight.device)
        count = self.sub_center_count.long()
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(count, group=group)
        # count * K + (K - 1 - k) is distinct within a class and largest at the lowest k among equal counts
        key = count * K + torch.arange(K - 1, -1, -1, device=count.device)
        return key.argmax(1)

    @torch.no_grad()
    def prune_sub_centers(self, group=None):
        """The paper's post-training step, in place: keep row c*K + dominant[c] of every class and become a one-centre head whose
        state dict loads into the reference-shaped module.  Returns the kept sub-centre indices.  Under data parallelism it is a
        collective like dominant_sub_centers(): call it on every rank.
        It ends training with the objects built on the K-centre weight: `weight` gets new [out_features, in_features] storage, so an
        optimizer created before (torch's momentum state, FusedSGD / FusedAdamW's flat fp32 master, momentum and shadow buffers, an
        attached EMA / SWA average) still describes the old [out_features * K, in_features] one.  To go on training, build a new
        optimizer (and Trainer) on the pruned module."""
        K = self.sub_centers
        dom = self.dominant_sub_centers(group)
        if K > 1:
            rows = torch.arange(self.out_features, device=dom.device) * K + dom
            self.weight.data = self.weight.data[rows.to(self.weight.device)].clone()
            self.weight.grad = None
            del self.sub_center_count
            self.sub_centers = 1
        return dom

    def hip_mode(self):
        return self._mode

    def _target_logit(self, cosine):  # torch (CPU) formulation of the margin on every entry
        raise NotImplementedError

    def forward(self, input, label):
        if input.is_cuda:
            from ._head_hip import MarginFunction, resolve_dtype
            if self.sub_centers == 1:
                return MarginFunction.apply(input, self.weight, label, self.hip_mode(), self.s, self.m,
                                            resolve_dtype(self.compute_dtype))
            return MarginFunction.apply(input, self.weight, label, self.hip_mode(), self.s, self.m,
                                        resolve_dtype(self.compute_dtype), self.sub_centers, self._count())
        cosine = F.normalize(input) @ F.normalize(self.weight).t()
        if self.sub_centers > 1:
            K = self.sub_centers
            cosine, arg = cosine.view(cosine.shape[0], self.out_features, K).max(2)
            count = self._count()
            if count is not None:
                t = label.view(-1).long()
                hit = t * K + arg[torch.arange(t.numel()), t]
                count.view(-1).add_(torch.bincount(hit, minlength=count.numel()).to(count.dtype))
        target = self._target_logit(cosine)
        hot = F.one_hot(label.view(-1).long(), self.out_features).to(cosine.dtype)
        return self.s * (hot * target + (1.0 - hot) * cosine)


class AddMarginProduct(_MarginHead):
    """CosFace: s·(cos θ − m) on the target class."""
    _mode = "cos"

    def __init__(self, in_features, out_features, s=30.0, m=0.40, device=None, sub_centers=1, **_):
        super().__init__(in_features, out_features, s, m, sub_centers)
        self.device = device

    def _target_logit(self, cosine):
        return cosine - self.m


class ArcMarginProduct(_MarginHead):
    """ArcFace: s·cos(θ + m) on the target class, with the hard (default) or easy fallback outside [0, π−m]."""

    def __init__(self, in_features, out_features, s=30.0, m=0.50, easy_margin=False, sub_centers=1, **_):
        super().__init__(in_features, out_features, s, m, sub_centers)
        self.easy_margin = easy_margin
        self.cos_m, self.sin_m = math.cos(m), math.sin(m)
        self.th = math.cos(math.pi - m)
        self.mm = math.sin(math.pi - m) * m

    def hip_mode(self):
        return "arc_easy" if self.easy_margin else "arc"

    def _target_logit(self, cosine):
        sine = torch.sqrt(1.0 - cosine * cosine)
        shifted = cosine * self.cos_m - sine * self.sin_m
        if self.easy_margin:
            return torch.where(cosine > 0, shifted, cosine)
        return torch.where(cosine > self.th, shifted, cosine - self.mm)
