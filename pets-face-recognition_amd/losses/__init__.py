"""`SoftmaxBasedMetricLearning` — backbone + cosine-margin head + criterion, with the reference's constructor
signature, attribute names (`module`, `add_margin`, `focal_loss`) and forward contract
(/root/reference/losses/__init__.py:8-46): `forward(img, label=None)` returns the embedding tensor when `label is
None`, else `{'loss', 'emb', 'logits'}` (a Partial FC training forward adds `'classes'` and `'local_label'`, a MagFace head
`'loss_g'`: the length regulariser that `'loss'` already contains; `pair_loss=` adds `'loss_pair'`, the pair term that `'loss'`
already contains with its weight); a list/tuple of images is embedded one by one and concatenated."""
import torch
import torch.nn as nn

from .large_margin import ArcMarginProduct, AddMarginProduct, AdaFaceProduct, CurricularFaceProduct, MagFaceProduct, _MarginHead
from .losses import FocalLoss, describe_criterion
from .pair import PairLoss, build_pair_loss


_ADAPTIVE_HEADS = {"adaface": AdaFaceProduct, "curricular": CurricularFaceProduct, "magface": MagFaceProduct}


class SoftmaxBasedMetricLearning(nn.Module):
    def __init__(self, model, num_class, embedding_size=512, s=64.0, m=0.5, is_focal=False, loss_kwargs=None,
                 arc_margin=False, easy_margin=False, sub_centers=1, margin=None, margin_kwargs=None, sample_rate=1.0, sparse_grad=False, pair_loss=None):
        super().__init__()
        # pair_loss (not in the reference): dict(kind='supcon' | 'circle' | 'batch_hard' | 'multi_similarity', weight=1.0, **params) adds weight * PairLoss(kind, **params) on
        # the pairs of the batch (losses/pair.py) to the head's loss; the pair term alone is returned detached as 'loss_pair'.  None: no
        # such module exists and every returned value is what it was.
        self.pair_loss, self.pair_weight = (None, 0.0) if pair_loss is None else build_pair_loss(pair_loss)
        # sample_rate / sparse_grad (not in the reference): Partial FC, see losses/large_margin.py; a sampled training forward returns
        # `logits` [B, S] over the classes `classes` with the targets `local_label`.  Passed on only when set, so that the defaults build
        # exactly the head they did.
        pfc = {}
        if sample_rate != 1.0 or sparse_grad:
            pfc = dict(sample_rate=sample_rate, sparse_grad=sparse_grad)
        # sub_centers (not in the reference): K centres per class in the head, see losses/large_margin.py; `logits` stay [B, num_class]
        # margin (not in the reference): None = arc_margin / easy_margin choose the head as ever; 'adaface' / 'curricular' build
        # AdaFaceProduct / CurricularFaceProduct(s=s, **margin_kwargs) (their own default m unless margin_kwargs sets one); 'magface'
        # builds MagFaceProduct(s=s, **margin_kwargs) and the returned loss includes its regulariser, also returned alone as 'loss_g'
        if margin in _ADAPTIVE_HEADS:
            self.add_margin = _ADAPTIVE_HEADS[margin](embedding_size, num_class, s=s, sub_centers=sub_centers, **pfc, **(margin_kwargs or {}))
        elif margin is not None:
            raise ValueError(f"margin must be None or one of {sorted(_ADAPTIVE_HEADS)}, got {margin!r}")
        elif arc_margin:
            self.add_margin = ArcMarginProduct(embedding_size, num_class, s=s, m=m, easy_margin=easy_margin, sub_centers=sub_centers, **pfc)
        else:
            self.add_margin = AddMarginProduct(embedding_size, num_class, s=s, m=m, sub_centers=sub_centers, **pfc)
        loss_kwargs = loss_kwargs or {}
        self.focal_loss = FocalLoss(num_class=num_class, **loss_kwargs) if is_focal else nn.CrossEntropyLoss(**loss_kwargs)
        if margin == "magface" and getattr(self.focal_loss, "reduction", "mean") not in ("mean", "sum"):
            raise ValueError("margin='magface' adds a scalar regulariser to the loss: the criterion's reduction must be 'mean' or 'sum'")
        if self.add_margin.sample_rate < 1.0 and (getattr(self.focal_loss, "adaptive_flag", False)
                                                   or getattr(self.focal_loss, "weight", None) is not None):
            raise ValueError("sample_rate < 1 (Partial FC) is not combined with a learnable focal alpha or a class weight: both are "
                             "indexed by the class, the sampled head's logits by the sampled position")
        self.module = model
        self.softmax = nn.Softmax(dim=1)
        self.return_logits = True  # the reference always returns logits; set False to skip writing them (bench)

    def _fusable(self, emb):
        """Criterion description (losses.losses.Criterion) when the whole head, normalise → cosine GEMM → margin → criterion, runs as
        the fused HIP path for this embedding, else None (then: the margin-logit kernels, then `self.focal_loss` on the logits).
        Fused: FocalLoss with a fixed or an adaptive (learnable) alpha; nn.CrossEntropyLoss with `weight`, `label_smoothing` and
        reduction 'mean' / 'sum'.  Left unfused on purpose: reduction='none', a non-default ignore_index, a weight / alpha that is not an
        fp32 [num_class] tensor on the embedding's device, CPU tensors, anything but a [B, in_features] embedding, a head weight that
        is not [out_features * sub_centers, in_features], a learnable focal alpha together with an adaptive margin (AdaFace /
        CurricularFace: the column kernel of d loss / d alpha recomputes the fixed margins' logits)."""
        head = self.add_margin
        if not emb.is_cuda or not isinstance(head, _MarginHead) or emb.dim() != 2 or emb.shape[1] != head.in_features:
            return None
        if head.weight.shape[0] != head.out_features * head.sub_centers:
            return None
        crit = describe_criterion(self.focal_loss, head.out_features, emb.device)
        if crit is not None and crit.alpha is not None and head.hip_adaptive() is not None:
            return None
        return crit

    def _unfused_magface(self, tensor, label, partial):
        """MagFace outside the fused path: the head returns (logits, lambda_g * mean g); 'sum' takes the regulariser as a sum too"""
        logits, reg = self.add_margin.forward_with_regulariser(tensor, label, partial)
        if getattr(self.focal_loss, "reduction", "mean") == "sum":
            reg = reg * tensor.shape[0]
        out = {'loss': self.focal_loss(logits, label if partial is None else partial.local_label) + reg, 'emb': tensor, 'logits': logits,
               'loss_g': reg.detach()}
        if partial is not None:
            out.update(classes=partial.index, local_label=partial.local_label)
        return out

    def _unfused(self, tensor, label, partial=None):
        if isinstance(self.add_margin, MagFaceProduct):
            return self._unfused_magface(tensor, label, partial)
        if partial is not None:     # Partial FC: logits [B, S], the criterion sees the labels' positions among the sampled classes
            logits = self.add_margin(tensor, label, partial)
            loss = self.focal_loss(logits, partial.local_label)
            return {'loss': loss, 'emb': tensor, 'logits': logits, 'classes': partial.index, 'local_label': partial.local_label}
        logits = self.add_margin(tensor, label)
        loss = self.focal_loss(logits, label)
        return {'loss': loss, 'emb': tensor, 'logits': logits}

    def forward(self, img, label=None, **__):
        if isinstance(img, (list, tuple)):
            tensor = torch.cat([self.module(i) for i in img], dim=0)
        else:
            tensor = self.module(img)
        if label is None:
            return tensor
        out = self._head_forward(tensor, label)
        if self.pair_loss is not None:
            head = self.add_margin
            lp = self.pair_loss(tensor, label, compute_dtype=getattr(head, "compute_dtype", None) or getattr(self.module, "compute_dtype", None))
            out['loss'] = out['loss'] + self.pair_weight * lp
            out['loss_pair'] = lp.detach()
        return out

    def _head_forward(self, tensor, label):
        crit = self._fusable(tensor)
        head = self.add_margin
        partial = head._partial(label) if isinstance(head, _MarginHead) else None
        if crit is None:
            return self._unfused(tensor, label, partial)
        from ._head_hip import MarginCEFunction, resolve_dtype
        dt = head.compute_dtype or getattr(self.module, "compute_dtype", None)
        adaptive = head.hip_adaptive()
        if adaptive is not None and adaptive.mag is not None:
            loss, logits, reg = MarginCEFunction.apply(tensor, head.weight, label, head.hip_mode(), head.s, head.m, crit, resolve_dtype(dt),
                                                       self.return_logits, None, 1 if partial is not None else head.sub_centers,
                                                       None if partial is not None else head._count(), adaptive, partial)
            out = {'loss': loss, 'emb': tensor, 'logits': logits if self.return_logits else None, 'loss_g': reg}
            if partial is not None:
                out.update(classes=partial.index, local_label=partial.local_label)
            return out
        if partial is not None:
            loss, logits = MarginCEFunction.apply(tensor, head.weight, label, head.hip_mode(), head.s, head.m, crit,
                                                  resolve_dtype(dt), self.return_logits, None, 1, None, adaptive, partial)
            return {'loss': loss, 'emb': tensor, 'logits': logits if self.return_logits else None, 'classes': partial.index,
                    'local_label': partial.local_label}
        if adaptive is not None:
            loss, logits = MarginCEFunction.apply(tensor, head.weight, label, head.hip_mode(), head.s, head.m, crit,
                                                  resolve_dtype(dt), self.return_logits, None, head.sub_centers, head._count(), adaptive)
        elif head.sub_centers == 1:
            loss, logits = MarginCEFunction.apply(tensor, head.weight, label, head.hip_mode(), head.s, head.m, crit,
                                                  resolve_dtype(dt), self.return_logits, crit.alpha)
        else:
            loss, logits = MarginCEFunction.apply(tensor, head.weight, label, head.hip_mode(), head.s, head.m, crit,
                                                  resolve_dtype(dt), self.return_logits, crit.alpha, head.sub_centers, head._count())
        return {'loss': loss, 'emb': tensor, 'logits': logits if self.return_logits else None}


class PairMetricLearning(nn.Module):
    """Backbone + a pair loss on the batch (losses/pair.py) and NO class head: the centre-free training mode, for identities that are
    too many, too few-shot or open-ended for a centre each.  Same forward contract as SoftmaxBasedMetricLearning: `forward(img,
    label=None)` returns the embedding when `label is None`, else `{'loss', 'emb', 'logits': None, 'loss_pair'}` with
    loss = weight * pair loss and 'loss_pair' the unweighted term, detached.  pair_loss: dict(kind=..., weight=1.0, **params).
    Batches want several items per identity (data_loading.PKBatchSampler): an anchor without a positive contributes nothing."""

    def __init__(self, model, pair_loss, embedding_size=512):
        super().__init__()
        self.module = model
        self.embedding_size = embedding_size
        self.pair_loss, self.pair_weight = build_pair_loss(pair_loss)

    def forward(self, img, label=None, **__):
        if isinstance(img, (list, tuple)):
            tensor = torch.cat([self.module(i) for i in img], dim=0)
        else:
            tensor = self.module(img)
        if label is None:
            return tensor
        if tensor.dim() != 2 or tensor.shape[1] != self.embedding_size:
            raise ValueError(f"PairMetricLearning: the backbone returned {tuple(tensor.shape)}, expected [B, {self.embedding_size}]")
        lp = self.pair_loss(tensor, label, compute_dtype=getattr(self.module, "compute_dtype", None))
        return {'loss': self.pair_weight * lp, 'emb': tensor, 'logits': None, 'loss_pair': lp.detach()}


class DummyWrapper(nn.Module):
    def __init__(self, model, *_, **__):
        super().__init__()
        self.module = model

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)
