"""Cosine-margin classification heads with the reference's constructor signatures and parameter names.

API mirrored: /root/reference/losses/large_margin.py — `AddMarginProduct(in_features, out_features, s=30.0, m=0.40)`
(CosFace, lines 10-40) and `ArcMarginProduct(in_features, out_features, s=30.0, m=0.50, easy_margin=False)`
(ArcFace, lines 44-84); `.weight` is `(out_features, in_features)`, Xavier-uniform.

Beyond the reference: `sub_centers=K` (Sub-center ArcFace, Deng et al., ECCV 2020) gives every class K centres, `.weight` is then
`(out_features * K, in_features)` with row `c*K + k` the k-th centre of class c, and the class cosine is the maximum of its K
sub-cosines.  K = 1 (the default) is the reference's head, bit for bit.

Beyond the reference as well: `AdaFaceProduct` (Kim et al., CVPR 2022: the margin follows the sample's feature norm) and
`CurricularFaceProduct` (Huang et al., CVPR 2020: hard negatives are re-weighted by a factor that grows with training), both with
persistent one-element statistics buffers; and `MagFaceProduct` (Meng et al., CVPR 2021), whose margin follows the embedding's length
and whose loss carries a regulariser on it: the one head whose gradient has a radial part (its docstring is the definition).

Beyond the reference too: `sample_rate < 1` (Partial FC, An et al., CVPR 2022): a training-mode forward scores the batch's own classes plus
random negatives, `int(sample_rate * out_features)` centres in all (`_MarginHead.sample`); `sparse_grad=True` leaves the gradient of those
rows on `weight.row_grad` for `optim.FusedSGD` instead of a dense `weight.grad`.  The defaults (1.0, False) are the head as it was.

CUDA inputs run on the gfx950 kernels (losses/_head_hip.py); CPU inputs run the same arithmetic with torch ops."""
import math
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F


class PartialFC(namedtuple("PartialFC", "index local_label sparse cache")):
    """One forward's Partial FC draw as the head functions take it: the sampled classes (int32 [S], ascending), the labels' positions
    among them (int64 [B]), whether the weight gradient stays row-sparse (`weight.row_grad`, CUDA only) and the head's dictionary
    holding the dense gradient buffer of the CUDA path between steps."""
    __slots__ = ()


class _MarginHead(nn.Module):
    _mode = None

    def __init__(self, in_features, out_features, s, m, sub_centers=1, sample_rate=1.0, sparse_grad=False):
        super().__init__()
        sub_centers = int(sub_centers)
        if not 1 <= sub_centers <= 16:
            raise ValueError(f"sub_centers must be in 1..16, got {sub_centers}")
        sample_rate = float(sample_rate)
        if not 0.0 < sample_rate <= 1.0:
            raise ValueError(f"sample_rate must be in (0, 1], got {sample_rate}")
        if sample_rate < 1.0 and int(sample_rate * out_features) < 1:
            raise ValueError(f"sample_rate={sample_rate} of {out_features} classes samples no class at all")
        if sample_rate < 1.0 and sub_centers > 1:
            raise ValueError("sample_rate < 1 (Partial FC) is not combined with sub_centers > 1")
        self.sample_rate, self.sparse_grad = sample_rate, bool(sparse_grad)
        self.num_sample = int(sample_rate * out_features) if sample_rate < 1.0 else out_features
        self.sample_generator = None   # torch.Generator of the negatives' draw (None: the device's default generator)
        self.last_index = None         # the classes of the last sampled forward (int32, ascending)
        self._pfc_cache = {}           # dense-gradient buffer of the CUDA path and the index that last wrote it
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

    def sampling(self, label):
        """whether a forward with `label` scores a sampled subset of the classes: training mode, labels given, fewer samples than classes"""
        return self.training and label is not None and self.num_sample < self.out_features

    def sample(self, label, score=None):
        """Partial FC's draw -> (index int32 [S] ascending, local_label int64 [B]) with S = int(sample_rate * out_features):
        key[c] = 2.0 if class c occurs in `label`, else score[c] (`score`: fp32 [out_features] in [0, 1); None draws it with
        torch.rand and `sample_generator`); index = the S classes with the largest key, ties towards the lower class id;
        local_label[b] = position of label[b] in index.  A batch larger than S is refused, so every positive is in index and S is a
        host constant (nothing is read back from the device).  Also kept in `last_index`."""
        C, S = self.out_features, self.num_sample
        label = label.reshape(-1).long()
        if label.numel() > S:
            raise ValueError(f"Partial FC: a batch of {label.numel()} does not fit into the {S} sampled classes "
                             f"(sample_rate={self.sample_rate}, {C} classes)")
        if score is None:
            score = torch.rand(C, device=label.device, generator=self.sample_generator)
        if score.shape != (C,) or score.device != label.device:
            raise ValueError(f"Partial FC: score must be [{C}] on {label.device}, got {tuple(score.shape)} on {score.device}")
        score = score.float().contiguous()
        if label.is_cuda:
            from .._hip import ops
            index, local = ops.pfc_sample(label.contiguous(), score, S)
        else:
            key = score.clone()
            key[label] = 2.0
            index = torch.sort(key, descending=True, stable=True).indices[:S].sort().values
            local = torch.searchsorted(index, label)
            index = index.to(torch.int32)
        self.last_index = index
        return index, local

    def _partial(self, label):
        """the losses._head_hip.PartialFC description of this forward (a fresh draw), or None when every class is scored"""
        if not self.sampling(label):
            return None
        index, local = self.sample(label)
        if self.sparse_grad and label.is_cuda and torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size() > 1:
            from .._hip import PfrError
            raise PfrError("Partial FC with sparse_grad=True keeps the sampled rows' gradient out of weight.grad, which the "
                           "data-parallel reducers never see: use sparse_grad=False in a distributed run")
        return PartialFC(index, local, self.sparse_grad and label.is_cuda, self._pfc_cache)

    def hip_adaptive(self):
        """the losses._head_hip.AdaptiveMargin description of a head whose margin depends on the batch, None for a fixed margin"""
        return None

    def _target_logit(self, cosine):  # torch (CPU) formulation of the margin on every entry
        raise NotImplementedError

    def forward(self, input, label, partial=None):
        """logits [B, out_features]; a sampled forward (`sampling(label)`) returns [B, num_sample] over the classes `last_index`, whose
        targets are `partial.local_label` (`partial`: this forward's draw when the caller made it, else it is drawn here)"""
        if partial is None:
            partial = self._partial(label)
        if input.is_cuda:
            from ._head_hip import MarginFunction, resolve_dtype
            if partial is not None:
                return MarginFunction.apply(input, self.weight, label, self.hip_mode(), self.s, self.m,
                                            resolve_dtype(self.compute_dtype), 1, None, None, partial)
            if self.sub_centers == 1:
                return MarginFunction.apply(input, self.weight, label, self.hip_mode(), self.s, self.m,
                                            resolve_dtype(self.compute_dtype))
            return MarginFunction.apply(input, self.weight, label, self.hip_mode(), self.s, self.m,
                                        resolve_dtype(self.compute_dtype), self.sub_centers, self._count())
        if partial is not None:
            label = partial.local_label
        cosine = self._cpu_cosine(input, label, partial)
        target = self._target_logit(cosine)
        hot = F.one_hot(label.view(-1).long(), cosine.shape[1]).to(cosine.dtype)
        return self.s * (hot * target + (1.0 - hot) * cosine)

    def _cpu_cosine(self, input, label, partial=None):
        """class cosines [B, out_features] with torch ops: after sub-centre pooling (and counting) when K > 1; the cosines to the
        sampled centres [B, num_sample] under Partial FC (index_select's autograd leaves the unsampled rows' gradient exactly 0)"""
        if partial is not None:
            return F.normalize(input) @ F.normalize(self.weight.index_select(0, partial.index.long())).t()
        cosine = F.normalize(input) @ F.normalize(self.weight).t()
        if self.sub_centers > 1:
            K = self.sub_centers
            cosine, arg = cosine.view(cosine.shape[0], self.out_features, K).max(2)
            count = self._count()
            if count is not None:
                t = label.view(-1).long()
                hit = t * K + arg[torch.arange(t.numel()), t]
                count.view(-1).add_(torch.bincount(hit, minlength=count.numel()).to(count.dtype))
        return cosine


class AddMarginProduct(_MarginHead):
    """CosFace: s·(cos θ − m) on the target class."""
    _mode = "cos"

    def __init__(self, in_features, out_features, s=30.0, m=0.40, device=None, sub_centers=1, sample_rate=1.0, sparse_grad=False,
                 **_):
        super().__init__(in_features, out_features, s, m, sub_centers, sample_rate, sparse_grad)
        self.device = device

    def _target_logit(self, cosine):
        return cosine - self.m


class ArcMarginProduct(_MarginHead):
    """ArcFace: s·cos(θ + m) on the target class, with the hard (default) or easy fallback outside [0, π−m]."""

    def __init__(self, in_features, out_features, s=30.0, m=0.50, easy_margin=False, sub_centers=1, sample_rate=1.0,
                 sparse_grad=False, **_):
        super().__init__(in_features, out_features, s, m, sub_centers, sample_rate, sparse_grad)
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


class _AdaptiveMarginHead(_MarginHead):
    """A head whose margin depends on the batch through persistent statistics buffers.  CUDA inputs: one extra small launch prepares the
    step's margins and moves the buffers on the device (csrc/pfr_head.hip: margin_prepare_kernel), the row kernel is the adaptive
    instantiation.  CPU inputs: `_adaptive_logits`, the same arithmetic in torch ops."""

    def forward(self, input, label, partial=None):
        if partial is None:
            partial = self._partial(label)
        if input.is_cuda:
            from ._head_hip import MarginFunction, resolve_dtype
            if partial is not None:
                return MarginFunction.apply(input, self.weight, label, self.hip_mode(), self.s, self.m, resolve_dtype(self.compute_dtype),
                                            1, None, self.hip_adaptive(), partial)
            return MarginFunction.apply(input, self.weight, label, self.hip_mode(), self.s, self.m, resolve_dtype(self.compute_dtype),
                                        self.sub_centers, self._count(), self.hip_adaptive())
        if partial is not None:
            label = partial.local_label
        return self._adaptive_logits(input, self._cpu_cosine(input, label, partial), label.view(-1).long())

    def _adaptive_logits(self, input, cosine, label):
        raise NotImplementedError


class AdaFaceProduct(_AdaptiveMarginHead):
    """AdaFace (Kim et al., CVPR 2022): the feature norm, a proxy of image quality, moves the margin between an angular one (low norm)
    and an additive one (high norm): k = clip(h * (|x| - batch_mean) / (batch_std + eps), -1, 1), target logit
    s * (cos(clip(theta - m k, eps, pi - eps)) - (m + m k)), every cosine clamped to [-1 + eps, 1 - eps].  No gradient flows through the
    norm, the statistics or the margins.
    `batch_mean` (initially 20) and `batch_std` (initially 100) are persistent one-element fp32 buffers: exponential moving averages
    (`t_alpha`) of the batch's mean norm and unbiased deviation, updated by training-mode forwards and used after the update; a batch
    of one leaves `batch_std` alone.  Under data parallelism the buffers are per rank and not synchronised, as the BatchNorm running
    statistics of the backbones are here: every rank averages the norms of its own share of the batches."""
    _mode = "adaface"

    def __init__(self, in_features, out_features, s=64.0, m=0.4, h=0.333, t_alpha=0.01, sub_centers=1, eps=1e-3, sample_rate=1.0,
                 sparse_grad=False, **_):
        super().__init__(in_features, out_features, s, m, sub_centers, sample_rate, sparse_grad)
        self.h, self.t_alpha, self.eps = h, t_alpha, eps
        self.register_buffer("batch_mean", torch.full((1,), 20.0))
        self.register_buffer("batch_std", torch.full((1,), 100.0))

    def hip_adaptive(self):
        from ._head_hip import AdaptiveMargin
        return AdaptiveMargin("adaface", self.h, self.t_alpha, self.eps, (self.batch_mean, self.batch_std), self.training)

    def _adaptive_logits(self, input, cosine, label):
        eps, m = self.eps, self.m
        c = cosine.clamp(-1.0 + eps, 1.0 - eps)
        with torch.no_grad():
            a = input.norm(dim=1).clamp_min(1e-12).clip(1e-3, 100.0).to(c.dtype)
            if self.training:
                self.batch_mean.copy_(self.t_alpha * a.mean() + (1.0 - self.t_alpha) * self.batch_mean)
                if a.numel() > 1:
                    self.batch_std.copy_(self.t_alpha * a.std() + (1.0 - self.t_alpha) * self.batch_std)
            k = (self.h * (a - self.batch_mean.to(c.dtype)) / (self.batch_std.to(c.dtype) + eps)).clip(-1.0, 1.0)
            g_ang, g_add = -m * k, m + m * k
        theta = torch.acos(c.gather(1, label[:, None]).squeeze(1))
        phi = torch.cos((theta + g_ang).clip(eps, math.pi - eps)) - g_add
        hot = F.one_hot(label, c.shape[1]).bool()
        return self.s * torch.where(hot, phi[:, None], c)


class MagFaceProduct(_AdaptiveMarginHead):
    """MagFace (Meng et al., CVPR 2021; the arithmetic of the published models/magface.py): the angular margin grows with the length of the
    raw embedding, and a regulariser on that length is part of the loss, so that |x| is trained into a per-sample quality score.
    Per row i, with the class cosines c_ij (after sub-centre pooling, clamped to [-1, 1]) and the label t_i:
        a_i = clamp(|x_i|, l_a, u_a)
        m_i = (u_m - l_m) / (u_a - l_a) * (a_i - l_a) + l_m
        phi_i = c * cos m_i - sqrt(1 - c^2) * sin m_i = cos(theta + m_i),  c = c_{i t_i}
        target_i = phi_i where c > 0, else c                                  (easy_margin=True, the default)
                 = phi_i where c > cos(pi - m_i), else c - m_i * sin m_i      (easy_margin=False)
        logits_ij = s * target_i for j = t_i, s * c_ij elsewhere
        loss = criterion(logits, t) + lambda_g * mean_i g(a_i),  g(a) = a / u_a^2 + 1 / a      (lambda_g * sum_i g(a_i) with reduction='sum')
    Focal gamma, class weights and label smoothing act on the criterion term only.
    Unlike every other head here the gradient runs THROUGH the length: d loss / d a_i = (d loss / d logits_{i t_i}) * s * d target_i /
    d m_i * (u_m - l_m) / (u_a - l_a) + lambda_g * g'(a_i) / B, g'(a) = 1 / u_a^2 - 1 / a^2, with d target / d m = -sin(theta + m) under
    the margin, 0 on the easy fallback and -(sin m + m cos m) on the hard one; it is exactly 0 where |x_i| lies outside [l_a, u_a]
    (the clamp is active; |x_i| equal to a bound counts as inside).  The embedding gradient is the tangent term of the other heads plus
    (d loss / d a_i) * x_i / |x_i|; the class weights get no new term.  No buffers, no state: the state dict is an ArcFace head's.
    `forward` returns the logits; `forward_with_regulariser` returns (logits, lambda_g * mean_i g(a_i)).  CUDA inputs run on
    pfr_magface_prepare / pfr_margin_ce_magface / pfr_l2norm_bwd_radial; the CPU path below is this definition in torch ops."""
    _mode = "magface"

    def __init__(self, in_features, out_features, s=64.0, l_a=10.0, u_a=110.0, l_m=0.45, u_m=0.8, lambda_g=35.0, easy_margin=True,
                 sub_centers=1, sample_rate=1.0, sparse_grad=False, **_):
        if not 0.0 < l_a < u_a:
            raise ValueError(f"MagFace: need 0 < l_a < u_a, got l_a={l_a}, u_a={u_a}")
        super().__init__(in_features, out_features, s, float(l_m), sub_centers, sample_rate, sparse_grad)   # .m: the base margin l_m
        self.l_a, self.u_a, self.l_m, self.u_m = float(l_a), float(u_a), float(l_m), float(u_m)
        self.lambda_g, self.easy_margin = float(lambda_g), bool(easy_margin)

    def hip_adaptive(self):
        from ._head_hip import magface
        return magface(self.l_a, self.u_a, self.l_m, self.u_m, self.lambda_g, self.easy_margin)

    def forward(self, input, label, partial=None):
        return self.forward_with_regulariser(input, label, partial)[0]

    def forward_with_regulariser(self, input, label, partial=None):
        if partial is None:
            partial = self._partial(label)
        if input.is_cuda:
            from ._head_hip import MarginFunction, resolve_dtype
            if partial is not None:
                return MarginFunction.apply(input, self.weight, label, self.hip_mode(), self.s, self.m, resolve_dtype(self.compute_dtype),
                                            1, None, self.hip_adaptive(), partial)
            return MarginFunction.apply(input, self.weight, label, self.hip_mode(), self.s, self.m, resolve_dtype(self.compute_dtype),
                                        self.sub_centers, self._count(), self.hip_adaptive())
        if partial is not None:
            label = partial.local_label
        label = label.view(-1).long()
        c = self._cpu_cosine(input, label, partial).clamp(-1.0, 1.0)
        a = input.norm(dim=1).clamp(self.l_a, self.u_a).to(c.dtype)
        m = (self.u_m - self.l_m) / (self.u_a - self.l_a) * (a - self.l_a) + self.l_m
        ct = c.gather(1, label[:, None]).squeeze(1)
        phi = ct * torch.cos(m) - torch.sqrt((1.0 - ct * ct).clamp_min(0.0)) * torch.sin(m)
        if self.easy_margin:
            target = torch.where(ct > 0, phi, ct)
        else:
            target = torch.where(ct > torch.cos(math.pi - m), phi, ct - m * torch.sin(m))
        hot = F.one_hot(label, c.shape[1]).bool()
        reg = self.lambda_g * (a / self.u_a ** 2 + 1.0 / a).mean()
        return self.s * torch.where(hot, target[:, None], c), reg


class CurricularFaceProduct(_AdaptiveMarginHead):
    """CurricularFace (Huang et al., CVPR 2020): ArcFace's hard margin on the target, and every negative harder than the shifted target
    (cos_j > cos(theta_t + m)) becomes cos_j * (t + cos_j): easy negatives first, hard ones as t grows.  No gradient flows through t or
    the mask.
    `t` (initially 0) is a persistent one-element fp32 buffer: the exponential moving average (`momentum`) of the batch's mean target
    cosine, updated by training-mode forwards and used after the update.  Under data parallelism it is per rank and not synchronised,
    as the BatchNorm running statistics of the backbones are here."""
    _mode = "curricular"

    def __init__(self, in_features, out_features, s=64.0, m=0.5, momentum=0.01, sub_centers=1, sample_rate=1.0, sparse_grad=False,
                 **_):
        super().__init__(in_features, out_features, s, m, sub_centers, sample_rate, sparse_grad)
        self.momentum = momentum
        self.cos_m, self.sin_m = math.cos(m), math.sin(m)
        self.th = math.cos(math.pi - m)
        self.mm = math.sin(math.pi - m) * m
        self.register_buffer("t", torch.zeros(1))

    def hip_adaptive(self):
        from ._head_hip import AdaptiveMargin
        return AdaptiveMargin("curricular", 0.0, self.momentum, 0.0, (self.t,), self.training)

    def _adaptive_logits(self, input, cosine, label):
        c = cosine.clamp(-1.0, 1.0)
        ct = c.gather(1, label[:, None]).squeeze(1)
        phi = ct * self.cos_m - torch.sqrt((1.0 - ct * ct).clamp_min(0.0)) * self.sin_m
        with torch.no_grad():
            if self.training:
                self.t.copy_(self.momentum * ct.mean() + (1.0 - self.momentum) * self.t)
            t = self.t.to(c.dtype).clone()      # this step's value: a later forward moves the buffer
            hard = c > phi[:, None]
        target = torch.where(ct > self.th, phi, ct - self.mm)
        neg = torch.where(hard, c * (t + c), c)
        hot = F.one_hot(label, c.shape[1]).bool()
        return self.s * torch.where(hot, target[:, None], neg)
