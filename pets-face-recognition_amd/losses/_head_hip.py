"""HIP execution of the cosine-margin head and the (focal) cross-entropy — autograd plumbing around the C-ABI.

Replaces, for CUDA tensors, the torch ops of /root/reference/losses/large_margin.py:30-40,69-84 and
/root/reference/losses/losses.py:22-28 (see csrc/pfr_head.hip for the kernel-level mapping)."""
from collections import namedtuple

import torch

from .._hip import ops, PfrError
from ..models._fe_engine import default_compute_dtype


def _cpad(C, dtype):
    k = 8 if dtype == torch.bfloat16 else 4
    return (C + k - 1) // k * k


def _dxn_by_rows(B, Cp, T):
    """dx̂ as a row-split reduction over the classes (see _cosine_bwd) rather than a plain GEMM against ŵᵀ"""
    return B % (8 if T == torch.bfloat16 else 4) == 0 and Cp >= 2048


def _cosine_fwd(emb, weight, T, pfc=None):
    """→ cos [B, Cpad] f32 and the saved normalised operands.  `pfc` (a PartialFC): the cosines to the S sampled centres, [B, Spad]; the
    rows pfc.index of the weight are normalised straight into the GEMM operand (pfr_l2norm_gather_fwd), no [S, D] fp32 copy exists"""
    B, D = emb.shape
    C = weight.shape[0] if pfc is None else pfc.index.numel()
    Cp = _cpad(C, T)
    xn, _, inv_x = ops.l2norm_fwd(emb, T)
    if pfc is not None:
        wn_full, wnT, inv_w = ops.l2norm_gather_fwd(weight, pfc.index, T, spad=Cp, want_t=not _dxn_by_rows(B, Cp, T))
        cos = torch.empty((B, 1, 1, Cp), dtype=torch.float32, device=emb.device)
        ops.conv2d_fwd(xn.view(B, 1, 1, D), wn_full[:C].view(C, 1, 1, D), out=cos)
        return cos.view(B, Cp), (xn, wnT, inv_x, inv_w, wn_full)
    wn_full = torch.zeros((Cp, D), dtype=T, device=emb.device) if Cp != C else torch.empty((C, D), dtype=T, device=emb.device)
    # ŵᵀ is the operand of the plain-GEMM form of dx̂ only: _cosine_bwd's row-split form reads ŵ itself (and the transposed
    # write, 2-byte elements a class apart, is most of this kernel's time at 10 000 classes)
    wn, wnT, inv_w = ops.l2norm_fwd(weight, T, want_t=not _dxn_by_rows(B, Cp, T), ldt=Cp, xn=wn_full[:C])
    cos = torch.empty((B, 1, 1, Cp), dtype=torch.float32, device=emb.device)
    ops.conv2d_fwd(xn.view(B, 1, 1, D), wn.view(C, 1, 1, D), out=cos)
    return cos.view(B, Cp), (xn, wnT, inv_x, inv_w, wn_full)


def _cosine_bwd(dcos, emb, weight, saved, T, pfc=None, param=None, dnorm=None):
    """dcos [B, Cpad] (compute dtype) → (demb f32 [B,D], dweight f32 [C,D]).  `pfc`: dcos is [B, Spad] over the sampled centres and the
    weight gradient exists for those rows only, see _partial_weight_grad.  `dnorm` (fp32 [B], MagFace): d loss / d |emb| per row, added
    as dnorm · emb / |emb| in the pass that writes the tangent gradient"""
    xn, wnT, inv_x, inv_w, wn_full = saved
    B, D = emb.shape
    C = weight.shape[0]
    Cp = dcos.shape[1]
    if _dxn_by_rows(B, Cp, T):
        # dxn[b][d] = Σ_c dcos[b][c]·wn[c][d]: the reduction runs over the CLASS dimension (10 000), the output is only B x D —
        # as a plain GEMM that is 8-16 tiles with a 10 000-long k-loop (0.2 ms on 8 CUs); as a "weight gradient" over the rows
        # of (wn, dcosᵀ) it is split over ~40 row ranges and takes ~20 µs
        from .._hip import lib, dtype_id
        dcosT = torch.empty((Cp, B), dtype=dcos.dtype, device=dcos.device)
        lib.pfr_transpose2d(dcos.data_ptr(), dcosT.data_ptr(), dtype_id(dcos.dtype), B, Cp, torch.cuda.current_stream().cuda_stream)
        dxn = ops.conv2d_wgrad(wn_full.view(Cp, 1, 1, D), dcosT.view(Cp, 1, 1, B), 1, 1, 1, 0)   # [B,1,1,D] f32
    else:
        dxn = torch.empty((B, 1, 1, D), dtype=torch.float32, device=emb.device)
        ops.conv2d_fwd(dcos.view(B, 1, 1, Cp), wnT.view(D, 1, 1, Cp), out=dxn)
    dwn = ops.conv2d_wgrad(xn.view(B, 1, 1, D), dcos.view(B, 1, 1, Cp), 1, 1, 1, 0)  # [Cp,1,1,D] f32
    if dnorm is None:
        demb = ops.l2norm_bwd(emb, inv_x, dxn.view(B, D), torch.float32)
    else:
        demb = ops.l2norm_bwd_radial(emb, inv_x, dxn.view(B, D), dnorm, torch.float32)
    if pfc is not None:
        return demb, _partial_weight_grad(weight, inv_w, dwn.view(Cp, D), pfc, param)
    dw = ops.l2norm_bwd(weight, inv_w, dwn.view(Cp, D), torch.float32, out=torch.empty_like(weight))
    return demb, dw


def _partial_weight_grad(w, inv_w, dwn, pfc, param):
    """Weight gradient of a Partial FC step, as what the function returns for the weight.
    Dense mode: a [C, D] gradient whose unsampled rows are zero.  The buffer lives in the head (pfc.cache) across steps: it is zeroed
    once, each backward writes its rows and re-zeroes only those of the backward before it.  Autograd copies it into `weight.grad` (the
    head keeps a reference, so it is never adopted as the gradient itself).
    Sparse mode: None; the rows are left on the parameter as `row_grad = (index, rows fp32 [S, D])` for optim.FusedSGD.  A second
    backward before the optimizer consumed them accumulates when it reuses the same index tensor and is refused otherwise."""
    if pfc.sparse:
        rows = ops.l2norm_gather_bwd(w, pfc.index, inv_w, dwn)
        have = getattr(param, "row_grad", None)
        if have is None:
            param.row_grad = (pfc.index, rows)
        elif have[0] is pfc.index:
            have[1].add_(rows)
        else:
            raise PfrError("Partial FC with sparse_grad=True: weight.row_grad still holds the rows of another draw; call the fused "
                           "optimizer's zero_grad() before the next backward (gradients of different draws accumulate with sparse_grad=False)")
        return None
    cache = pfc.cache
    buf, prev = cache.get("dense"), cache.get("prev")
    grad = getattr(param, "grad", None)
    if buf is None or buf.shape != w.shape or buf.device != w.device or (grad is not None and grad.data_ptr() == buf.data_ptr()):
        buf, prev = torch.zeros_like(w), None
    cache["dense"], cache["prev"] = buf, pfc.index
    return ops.l2norm_gather_bwd(w, pfc.index, inv_w, dwn, dense_out=buf, prev_index=prev)


def _pool_fwd(cos_sub, C, K, T, label, count):
    """sub-cosines [B, Cpad(C*K)] → class cosines [B, Cpad(C)] (pad columns 0) and the selected sub-centre per (row, class); with
    `count` ([C, K] int32) the histogram of the labels' sub-centres is updated in the same pass"""
    return ops.subcenter_pool(cos_sub, C, K, ldc=_cpad(C, T), label=None if count is None else label, count=count)


def _split_classes(w, K):
    if not 1 <= K <= 16 or w.shape[0] % K:
        raise PfrError(f"sub-centre head: a [{w.shape[0]}, {w.shape[1]}] weight does not hold K={K} centres per class (1 <= K <= 16)")
    return w.shape[0] // K


def _check_partial(pfc, K, alpha, class_weight):
    if K != 1 or alpha is not None or class_weight is not None:
        raise ValueError("Partial FC (sample_rate < 1) is not combined with sub_centers > 1, a learnable focal alpha or a class weight: "
                         "they are indexed by the class, not by the sampled position")
    if pfc.index.dtype != torch.int32 or pfc.local_label.dtype != torch.int64 or not pfc.index.is_cuda or not pfc.local_label.is_cuda:
        raise PfrError("Partial FC: index must be an int32 and local_label an int64 CUDA tensor (_MarginHead.sample)")


class AdaptiveMargin(namedtuple("AdaptiveMargin", "kind h momentum eps state update mag", defaults=(None,))):
    """What the head functions need of an adaptive-margin head (losses/large_margin.py: AdaFaceProduct, CurricularFaceProduct,
    MagFaceProduct): the kind ('adaface' / 'curricular' / 'magface'), AdaFace's h and clamp eps, the EMA momentum (AdaFace's t_alpha), the
    module's persistent one-element buffers ((batch_mean, batch_std) / (t,) / ()) and whether this forward moves them (training mode);
    `mag`: the MagFace description of kind 'magface', which has no state and uses none of h, momentum, eps."""
    __slots__ = ()


class MagFace(namedtuple("MagFace", "l_a u_a l_m u_m lambda_g easy")):
    """MagFaceProduct's constants: the norm and margin ranges, the regulariser's weight, easy / hard fallback of the target"""
    __slots__ = ()


def magface(l_a, u_a, l_m, u_m, lambda_g, easy):
    return AdaptiveMargin("magface", 0.0, 0.0, 0.0, (), False, MagFace(float(l_a), float(u_a), float(l_m), float(u_m), float(lambda_g), bool(easy)))


def _magface_reduction(crit):
    return "mean" if crit.is_plain else ("sum" if crit.reduction == "sum" else "weighted_mean")


def _prepare_adaptive(ad, m, inv_x, cos, label):
    """one launch after the (pooled) cosines: updates the head's buffers on the device, returns this step's (row_margin, state_used)"""
    return ops.margin_prepare(ad.kind, ad.state, cos.shape[0], inv_norm=inv_x, cosv=cos, label=label, m=m, h=ad.h, momentum=ad.momentum,
                              eps=ad.eps, update=ad.update)


class MarginCEFunction(torch.autograd.Function):
    """(emb, weight, label[, alpha]) → (loss, logits): normalise → cosine GEMM → margin → scale → criterion, fused.  `crit` is the
    losses.losses.Criterion description of the loss (gamma, adaptive alpha, class weight, label smoothing, reduction); `alpha` is the
    criterion's learnable [C] vector passed as an input so that autograd hands its gradient back (None when crit.alpha is None).
    Every criterion is the same launches: only the row kernel's instantiation differs, plus one column kernel for d loss / d alpha.
    K > 1 (sub-centre head, weight [C*K, D]): the cosine GEMM runs over all C*K centres, one pooling pass takes the maximum per class
    before the row kernel, one scatter pass routes dcos to the selected centres after it; `count` ([C, K] int32 or None) collects which
    centre each sample's own class selected.  K == 1 launches neither.
    `adaptive` (an AdaptiveMargin, `mode` is then its kind): one more small launch after the pooling prepares the step's margins and moves
    the head's buffers, the row kernel is the adaptive instantiation; row_margin / state_used are saved per call, so this step's backward
    is independent of forwards that ran after it.  The learnable alpha is not fused with these margins (losses/__init__.py:_fusable).
    Kind 'magface' (adaptive.mag): its own prepare / row-kernel / loss entries; the function then returns (loss, logits, regulariser), the
    loss including the regulariser, and the backward hands the row kernel's d loss / d |emb| to the radial embedding backward.
    `pfc` (a losses.large_margin.PartialFC = (index, local_label, sparse, cache)): Partial FC, the same launches on the S sampled centres
    [B, Spad] with the gathered normalisation kernels in place of the full ones; `logits` are [B, S].  The weight's gradient is dense with
    zero unsampled rows, or with pfc.sparse None, the rows being left on `weight.row_grad` (_partial_weight_grad)."""

    @staticmethod
    def forward(ctx, emb, weight, label, mode, s, m, crit, T, want_logits, alpha=None, K=1, count=None, adaptive=None, pfc=None):
        emb = emb.contiguous().float()
        w = weight.detach().contiguous()
        label = label.contiguous().long()
        C = w.shape[0] if K == 1 else _split_classes(w, K)
        B = emb.shape[0]
        if pfc is not None:    # Partial FC: the head below runs on the S sampled centres with the labels' positions among them
            _check_partial(pfc, K, alpha, crit.weight)
            C, label = pfc.index.numel(), pfc.local_label.contiguous()
        ctx.pfc, ctx.param = pfc, weight
        cos, saved = _cosine_fwd(emb, w, T, pfc)
        arg = None
        if K > 1:
            cos, arg = _pool_fwd(cos, C, K, T, label, count)
        stats = inv_denom = row_margin = state_used = reg = None
        mag = None if adaptive is None else adaptive.mag
        if adaptive is not None and alpha is not None:
            raise PfrError("the fused head does not combine a learnable focal alpha with an adaptive margin")
        if mag is not None:
            # MagFace: the margins and g / g' per row from the inverse norms, the row kernel, then the criterion's reduction and the
            # regulariser lambda_g · mean g(a) in one launch; row_reg rides in state_used's slot of the saved tensors
            row_margin, state_used = ops.magface_prepare(saved[2], mag.l_a, mag.u_a, mag.l_m, mag.u_m)
            logits, loss_rows, stats, _, _ = ops.margin_ce_magface(cos, label, C, mag.easy, s, row_margin, state_used, gamma=crit.gamma,
                                                                   class_weight=crit.weight, label_smoothing=crit.smoothing,
                                                                   want_logits=want_logits, want_stats=not crit.is_plain)
            red = _magface_reduction(crit)
            loss, inv_denom, reg = ops.magface_loss(loss_rows, stats, state_used, red, mag.lambda_g)
            if red != "weighted_mean":
                inv_denom = None
        elif adaptive is not None:
            row_margin, state_used = _prepare_adaptive(adaptive, m, saved[2], cos, label)
            logits, loss_rows, stats, _ = ops.margin_ce_adaptive(cos, label, C, mode, s, m, adaptive.eps, row_margin, state_used,
                                                                 gamma=crit.gamma, class_weight=crit.weight, label_smoothing=crit.smoothing,
                                                                 want_logits=want_logits, want_stats=not crit.is_plain)
            if crit.is_plain:
                loss = ops.mean(loss_rows)
            elif crit.reduction == "sum":
                loss, _ = ops.loss_reduce(loss_rows, None, "sum")
            else:
                loss, inv_denom = ops.loss_reduce(loss_rows, stats, "weighted_mean")
        elif crit.is_plain:
            logits, loss_rows, _ = ops.margin_ce(cos, label, C, mode, s, m, gamma=crit.gamma, want_logits=want_logits)
            loss = ops.mean(loss_rows)
        else:
            alpha = None if alpha is None else alpha.detach().contiguous()
            logits, loss_rows, stats, _ = ops.margin_ce_ex(cos, label, C, mode, s, m, gamma=crit.gamma, alpha=alpha, class_weight=crit.weight,
                                                           label_smoothing=crit.smoothing, want_logits=want_logits)
            if alpha is not None:
                loss = ops.mean(loss_rows)
            elif crit.reduction == "sum":
                loss, _ = ops.loss_reduce(loss_rows, None, "sum")
            else:   # F.cross_entropy's 'mean' divides by the sum of the targets' weights (= B without weights)
                loss, inv_denom = ops.loss_reduce(loss_rows, stats, "weighted_mean")
        ctx.save_for_backward(emb, w, label, cos, alpha, crit.weight, stats, inv_denom, arg, row_margin, state_used, *saved)
        ctx.cfg = (mode, s, m, crit, T, C, K, None if adaptive is None or mag is not None else adaptive.eps)
        ctx.mag = mag
        if logits is None:
            logits = torch.empty(0, device=emb.device)
        ctx.mark_non_differentiable(logits)
        if mag is not None:     # the regulariser's value (already part of `loss`), for logging
            ctx.mark_non_differentiable(reg)
            return loss, logits, reg
        return loss, logits

    @staticmethod
    def backward(ctx, dloss, _dlogits, _dreg=None):
        emb, w, label, cos, alpha, cweight, stats, inv_denom, arg, row_margin, state_used, *saved = ctx.saved_tensors
        mode, s, m, crit, T, C, K, ad_eps = ctx.cfg
        B = emb.shape[0]
        dloss = dloss.contiguous().float()
        dalpha = dnorm = None
        if ctx.mag is not None:
            mag = ctx.mag
            red = _magface_reduction(crit)
            _, _, _, dcos, dnorm = ops.margin_ce_magface(cos, label, C, mag.easy, s, row_margin, state_used,
                                                         reg_scale=mag.lambda_g * (1.0 if red == "sum" else 1.0 / B), gamma=crit.gamma,
                                                         class_weight=cweight, label_smoothing=crit.smoothing,
                                                         grad_scale=1.0 / B if crit.is_plain else 1.0, grad_scale_dev=dloss,
                                                         grad_scale_dev2=inv_denom, want_logits=False, want_stats=False, dcos_dtype=T)
        elif ad_eps is not None:
            _, _, _, dcos = ops.margin_ce_adaptive(cos, label, C, mode, s, m, ad_eps, row_margin, state_used, gamma=crit.gamma,
                                                   class_weight=cweight, label_smoothing=crit.smoothing,
                                                   grad_scale=1.0 / B if crit.is_plain else 1.0, grad_scale_dev=dloss,
                                                   grad_scale_dev2=inv_denom, want_logits=False, want_stats=False, dcos_dtype=T)
        elif crit.is_plain:
            _, _, dcos = ops.margin_ce(cos, label, C, mode, s, m, gamma=crit.gamma, grad_scale=1.0 / B, grad_scale_dev=dloss,
                                       want_logits=False, dcos_dtype=T)
        else:
            # 'mean' of the focal criteria: 1 / B; weighted mean: the forward's device scalar 1 / Σ w_t; 'sum': 1
            gs = 1.0 / B if alpha is not None else 1.0
            _, _, _, dcos = ops.margin_ce_ex(cos, label, C, mode, s, m, gamma=crit.gamma, alpha=alpha, class_weight=cweight,
                                             label_smoothing=crit.smoothing, grad_scale=gs, grad_scale_dev=dloss, grad_scale_dev2=inv_denom,
                                             want_logits=False, want_stats=False, dcos_dtype=T)
            if alpha is not None and ctx.needs_input_grad[9]:
                dalpha = ops.alpha_grad(cos, label, alpha, stats, C, s, grad_scale=gs, grad_scale_dev=dloss)
        if K > 1:
            dcos = ops.subcenter_scatter(dcos, arg, K, ld_sub=_cpad(C * K, T))
        demb, dw = _cosine_bwd(dcos, emb, w, saved, T, ctx.pfc, ctx.param, dnorm)
        return demb, dw, None, None, None, None, None, None, None, dalpha, None, None, None, None


class MarginFunction(torch.autograd.Function):
    """(emb, weight, label) → logits; standalone ArcMarginProduct / AddMarginProduct (K, count, adaptive: as in MarginCEFunction)."""

    @staticmethod
    def forward(ctx, emb, weight, label, mode, s, m, T, K=1, count=None, adaptive=None, pfc=None):
        emb = emb.contiguous().float()
        w = weight.detach().contiguous()
        label = label.contiguous().long()
        C = w.shape[0] if K == 1 else _split_classes(w, K)
        if pfc is not None:
            _check_partial(pfc, K, None, None)
            C, label = pfc.index.numel(), pfc.local_label.contiguous()
        ctx.pfc, ctx.param = pfc, weight
        cos, saved = _cosine_fwd(emb, w, T, pfc)
        arg = None
        if K > 1:
            cos, arg = _pool_fwd(cos, C, K, T, label, count)
        row_margin = state_used = reg = None
        mag = None if adaptive is None else adaptive.mag
        if mag is not None:
            # MagFace returns (logits, regulariser): lambda_g · mean g(a), a differentiable output whose gradient joins dnorm
            row_margin, state_used = ops.magface_prepare(saved[2], mag.l_a, mag.u_a, mag.l_m, mag.u_m)
            logits, _, _, _, _ = ops.margin_ce_magface(cos, label, C, mag.easy, s, row_margin, state_used, want_logits=True, want_stats=False)
            _, _, reg = ops.magface_loss(None, None, state_used, "mean", mag.lambda_g)
        elif adaptive is not None:
            row_margin, state_used = _prepare_adaptive(adaptive, m, saved[2], cos, label)
            logits, _, _, _ = ops.margin_ce_adaptive(cos, label, C, mode, s, m, adaptive.eps, row_margin, state_used, want_logits=True,
                                                     want_stats=False)
        else:
            logits, _, _ = ops.margin_ce(cos, label, C, mode, s, m, want_logits=True)
        ctx.save_for_backward(emb, w, label, cos, arg, row_margin, state_used, *saved)
        ctx.cfg = (mode, s, m, T, C, K, None if adaptive is None or mag is not None else adaptive.eps)
        ctx.mag = mag
        return logits if mag is None else (logits, reg)

    @staticmethod
    def backward(ctx, dlogits, dreg=None):
        from .._hip import lib, dtype_id
        emb, w, label, cos, arg, row_margin, state_used, *saved = ctx.saved_tensors
        mode, s, m, T, C, K, ad_eps = ctx.cfg
        B, Cp = cos.shape
        dlogits = dlogits.contiguous().float()
        dnorm = None
        if ctx.mag is not None:
            dreg = None if dreg is None else dreg.contiguous().float()
            dcos, dnorm = ops.margin_bwd_magface(cos, label, C, ctx.mag.easy, s, row_margin, state_used, ctx.mag.lambda_g / emb.shape[0],
                                                 dreg, dlogits, T)
        elif ad_eps is not None:
            dcos = ops.margin_bwd_adaptive(cos, label, C, mode, s, m, ad_eps, row_margin, state_used, dlogits, T)
        else:
            dcos = torch.zeros((B, Cp), dtype=T, device=emb.device)
            lib.pfr_margin_bwd(cos.data_ptr(), label.data_ptr(), B, C, Cp, ops.MARGIN_MODES[mode], float(s), float(m),
                               dlogits.data_ptr(), dcos.data_ptr(), dtype_id(T), torch.cuda.current_stream().cuda_stream)
        if K > 1:
            dcos = ops.subcenter_scatter(dcos, arg, K, ld_sub=_cpad(C * K, T))
        demb, dw = _cosine_bwd(dcos, emb, w, saved, T, ctx.pfc, ctx.param, dnorm)
        return demb, dw, None, None, None, None, None, None, None, None, None


class FocalCEFunction(torch.autograd.Function):
    """(logits, target[, alpha]) → mean((1-p)^γ · CE) of alpha·logits: standalone FocalLoss / CrossEntropyLoss on CUDA logits."""

    @staticmethod
    def forward(ctx, logits, target, gamma, alpha=None):
        logits = logits.contiguous().float()
        target = target.contiguous().long()
        B, C = logits.shape
        stats = None
        if alpha is None:
            _, rows, _ = ops.margin_ce(logits, target, C, "none", 1.0, 0.0, gamma=gamma, want_logits=False)
        else:
            alpha = alpha.detach().contiguous()
            _, rows, stats, _ = ops.margin_ce_ex(logits, target, C, "none", 1.0, 0.0, gamma=gamma, alpha=alpha, want_logits=False)
        ctx.save_for_backward(logits, target, alpha, stats)
        ctx.gamma = gamma
        return ops.mean(rows)

    @staticmethod
    def backward(ctx, dloss):
        logits, target, alpha, stats = ctx.saved_tensors
        B, C = logits.shape
        dloss = dloss.contiguous().float()
        if alpha is None:
            _, _, d = ops.margin_ce(logits, target, C, "none", 1.0, 0.0, gamma=ctx.gamma, grad_scale=1.0 / B,
                                    grad_scale_dev=dloss, want_logits=False, dcos_dtype=torch.float32)
            return d, None, None, None
        _, _, _, d = ops.margin_ce_ex(logits, target, C, "none", 1.0, 0.0, gamma=ctx.gamma, alpha=alpha, grad_scale=1.0 / B,
                                      grad_scale_dev=dloss, want_logits=False, want_stats=False, dcos_dtype=torch.float32)
        dalpha = ops.alpha_grad(logits, target, alpha, stats, C, 1.0, grad_scale=1.0 / B, grad_scale_dev=dloss) \
            if ctx.needs_input_grad[3] else None
        return d, None, None, dalpha


def resolve_dtype(dt):
    return dt or default_compute_dtype()
