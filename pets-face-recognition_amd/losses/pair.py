"""Pair losses on the Gram matrix of the batch itself: supervised contrastive (Khosla et al. 2020, L_out) and Circle loss (Sun et al.
2020, per anchor as pytorch-metric-learning does).  Not in the reference.  The one criterion here that needs no centre per identity.

The contract (include/pfr_hip.h at pfr_pair_loss_fwd; DESIGN.md "Pair losses"): ê_i = e_i / max(|e_i|, eps), s_ij = ê_i . ê_j,
P(i) = {j != i : y_j = y_i}, N(i) = {j : y_j != y_i}; the diagonal is in neither set.
  supcon   valid when P(i) is not empty;  l_i = log sum_{a != i} exp(s_ia / tau) - mean_{p in P(i)} s_ip / tau
  circle   valid when P(i) and N(i) are not empty;  alpha_p = max(0, 1 + m - s_p), alpha_n = max(0, s_n + m), constants in the gradient;
           l_i = softplus(LSE_n gamma alpha_n (s_n - m) + LSE_p (-gamma alpha_p (s_p - 1 + m)))
  loss = mean of l_i over the valid anchors; no valid anchor: 0.0 exactly, with a zero gradient.
Rank-local: the pairs are those of this process's batch, there is no all-gather.  No mining (batch-hard triplet, multi-similarity), no
cross-batch memory, no label that means "ignore".

CUDA tensors run `PairLossFunction`: pfr_l2norm_fwd, ONE forward launch (csrc/pfr_pairloss.hip), then one backward launch and
pfr_l2norm_bwd.  CPU tensors run `pair_loss_torch`, the same contract in torch ops in the tensor's own dtype; in float64 it is the oracle
of the device tests."""
import torch
import torch.nn as nn
import torch.nn.functional as F

KINDS = ("supcon", "circle")
_DEFAULTS = {"supcon": dict(tau=0.1), "circle": dict(m=0.25, gamma=64.0)}


def _params(kind, params):
    if kind not in KINDS:
        raise ValueError(f"pair loss kind must be one of {list(KINDS)}, got {kind!r}")
    unknown = set(params) - set(_DEFAULTS[kind])
    if unknown:
        raise ValueError(f"pair loss {kind!r} takes {sorted(_DEFAULTS[kind])}, got {sorted(unknown)}")
    p = {k: float(v) for k, v in {**_DEFAULTS[kind], **params}.items()}
    if kind == "supcon" and not p["tau"] > 0:
        raise ValueError(f"supcon needs a temperature > 0, got {p['tau']}")
    if kind == "circle" and not (p["gamma"] > 0 and 0 <= p["m"] < 1):
        raise ValueError(f"circle needs gamma > 0 and 0 <= m < 1, got m={p['m']} gamma={p['gamma']}")
    return p


def pair_loss_from_scores(s, label, kind, s_alpha=None, **params):
    """The contract from the score matrix s [B, B] on: -> (loss, l [B] with 0 at invalid anchors (detached), valid [B] bool, logits [B, B]).
    `logits` is the matrix the log-sum-exps read (s / tau; Circle: the positive form where y_j = y_i, the negative form elsewhere), part of
    the graph: d loss / d logits is the softmax weight of every pair.  s_alpha: the scores Circle's alpha are taken from (None: s, detached)."""
    p = _params(kind, params)
    B = s.shape[0]
    same = label[:, None] == label[None, :]
    eye = torch.eye(B, dtype=torch.bool, device=s.device)
    pos, neg = same & ~eye, ~same
    valid = pos.any(1) if kind == "supcon" else pos.any(1) & neg.any(1)
    idx = valid.nonzero().squeeze(1)
    if kind == "supcon":
        x = s / p["tau"]
    else:
        m, gamma = p["m"], p["gamma"]
        sa = (s if s_alpha is None else s_alpha).detach()
        x = torch.where(same, -gamma * (1 + m - sa).clamp_min(0) * (s - (1 - m)), gamma * (sa + m).clamp_min(0) * (s - m))
    rows = s.new_zeros(B)
    if idx.numel() == 0:
        return (s * 0).sum(), rows, valid, x        # 0.0 exactly, and a zero gradient
    ninf = float("-inf")
    if kind == "supcon":
        xv = x[idx]
        ell = torch.logsumexp(xv.masked_fill(eye[idx], ninf), 1) - (xv * pos[idx]).sum(1) / pos[idx].sum(1)
    else:
        z = torch.logsumexp(x[idx].masked_fill(~neg[idx], ninf), 1) + torch.logsumexp(x[idx].masked_fill(~pos[idx], ninf), 1)
        ell = -F.logsigmoid(-z)      # softplus(z) without F.softplus's linear branch above its threshold (z = 24 is off by 4e-11 there)
    return ell.sum() / idx.numel(), rows.index_put((idx,), ell.detach()), valid, x


def pair_loss_torch(emb, label, kind, normalize=True, eps=1e-12, alpha_emb=None, return_rows=False, **params):
    """The contract in torch ops, differentiable, in emb's dtype.  normalize=False: `emb` already holds the rows ê (the device tests hand
    the operand bits of the kernel over).  alpha_emb: the rows Circle's weights alpha are taken from; None = emb itself, detached (they are
    constants in the gradient either way: a finite-difference check of that convention passes a fixed copy of emb here).
    return_rows: -> (loss, l [B] with 0 at invalid anchors, valid [B] bool)."""
    xn = F.normalize(emb, dim=1, eps=eps) if normalize else emb
    sa = None
    if alpha_emb is not None:
        an = F.normalize(alpha_emb, dim=1, eps=eps) if normalize else alpha_emb
        sa = an @ an.t()
    loss, rows, valid, _ = pair_loss_from_scores(xn @ xn.t(), label, kind, s_alpha=sa, **params)
    return (loss, rows, valid) if return_rows else loss


class PairLossFunction(torch.autograd.Function):
    """(emb [B, D] CUDA, label int64 [B]) -> scalar loss.  Forward: pfr_l2norm_fwd (ê and êᵀ in the compute dtype) + pfr_pair_loss_fwd;
    backward: pfr_pair_loss_bwd (dê, fp32) + pfr_l2norm_bwd.  There is no fallback: a shape the kernels refuse is an error."""

    @staticmethod
    def forward(ctx, emb, label, kind, T, params):
        from .._hip import ops
        emb = emb.contiguous()
        B = emb.shape[0]
        xn, xnT, inv = ops.l2norm_fwd(emb, T, want_t=True, ldt=(B + 31) // 32 * 32)
        out, stats, _ = ops.pair_loss_fwd(xn, label.contiguous(), kind, **params)
        ctx.save_for_backward(emb, label, xn, xnT, inv, stats, out)
        ctx.kind, ctx.params = kind, params
        return out[0]

    @staticmethod
    def backward(ctx, g):
        from .._hip import ops
        emb, label, xn, xnT, inv, stats, out = ctx.saved_tensors
        dxn = ops.pair_loss_bwd(xn, xnT, label.contiguous(), stats, out, ctx.kind, grad_scale_dev=g.float().contiguous(), **ctx.params)
        demb = ops.l2norm_bwd(emb, inv, dxn, torch.float32)
        return demb.to(emb.dtype), None, None, None, None


class PairLoss(nn.Module):
    """PairLoss(kind, **params): forward(emb [B, D], label [B]) -> scalar.  kind 'supcon' (tau=0.1) or 'circle' (m=0.25, gamma=64).
    compute_dtype (fp32 / bf16; None = the default of the HIP engines, as the margin heads resolve it) is the dtype of ê on the device:
    in bf16 the scores come from the bf16-rounded ê with fp32 accumulation.  int8 is not supported."""

    def __init__(self, kind="supcon", compute_dtype=None, **params):
        super().__init__()
        self.kind = kind
        self.params = _params(kind, params)
        self.compute_dtype = compute_dtype

    def extra_repr(self):
        return f"kind={self.kind!r}, " + ", ".join(f"{k}={v:g}" for k, v in self.params.items())

    def forward(self, emb, label, compute_dtype=None):
        if not emb.is_cuda:
            return pair_loss_torch(emb, label, self.kind, **self.params)
        from ._head_hip import resolve_dtype
        T = resolve_dtype(self.compute_dtype or compute_dtype)
        if T not in (torch.float32, torch.bfloat16):
            raise ValueError(f"pair loss: the compute dtype is fp32 or bf16, got {T}")
        return PairLossFunction.apply(emb, label, self.kind, T, self.params)


def build_pair_loss(spec):
    """dict(kind=..., weight=1.0, compute_dtype=None, **params) -> (PairLoss, weight)"""
    spec = dict(spec)
    if "kind" not in spec:
        raise ValueError("pair_loss needs a 'kind' ('supcon' or 'circle')")
    weight = float(spec.pop("weight", 1.0))
    return PairLoss(spec.pop("kind"), **spec), weight
