"""Pair losses on the Gram matrix of the batch itself: supervised contrastive (Khosla et al. 2020, L_out) and Circle loss (Sun et al.
2020, per anchor as pytorch-metric-learning does).  Not in the reference.  The one criterion here that needs no centre per identity.

The contract (include/pfr_hip.h at pfr_pair_loss_fwd; DESIGN.md "Pair losses"): ê_i = e_i / max(|e_i|, eps), s_ij = ê_i . ê_j,
P(i) = {j != i : y_j = y_i}, N(i) = {j : y_j != y_i}; the diagonal is in neither set.
  supcon   valid when P(i) is not empty;  l_i = log sum_{a != i} exp(s_ia / tau) - mean_{p in P(i)} s_ip / tau
  circle   valid when P(i) and N(i) are not empty;  alpha_p = max(0, 1 + m - s_p), alpha_n = max(0, s_n + m), constants in the gradient;
           l_i = softplus(LSE_n gamma alpha_n (s_n - m) + LSE_p (-gamma alpha_p (s_p - 1 + m)))
  loss = mean of l_i over the valid anchors; no valid anchor: 0.0 exactly, with a zero gradient.
Rank-local: the pairs are those of this process's batch, there is no all-gather.  No momentum encoder, no label that means "ignore".

Mined kinds (include/pfr_hip.h at pfr_pair_mined_fwd; DESIGN.md "Mined pair losses"; csrc/pfr_pairmine.hip), valid when P(i) and N(i) are
not empty.  s_p*(i) = min over P(i), s_n*(i) = max over N(i), ties to the smallest partner number (batch item j is number j, ring slot k
is B + k), -0.0 = +0.0, a NaN score is in neither set:
  batch_hard        (Hermans et al. 2017, on cosine scores) z_i = s_n* - s_p* + m;  gamma = 0: l_i = max(0, z_i);  gamma > 0:
                    l_i = softplus(gamma z_i) / gamma
  multi_similarity  (Wang et al., CVPR 2019) negative n kept iff s_in + epsilon > s_p*, positive p kept iff s_ip - epsilon < s_n*;
                    l_i = log(1 + sum_{kept p} exp(-alpha (s_ip - base))) / alpha + log(1 + sum_{kept n} exp(beta (s_in - base))) / beta
Two stated deviations: the mean runs over the VALID anchors (the published Multi-Similarity code divides by the batch size), and the
selection (which pair is the hardest, which pairs are kept, whether the hinge is active) is a CONSTANT in the gradient.  Not covered: an
all-gather of partners across ranks, Euclidean-distance triplets, semi-hard mining.

Cross-batch memory (Wang et al., CVPR 2020; `PairLoss(kind, memory=M)`): a ring of the normalised embeddings and labels of the last M items.
Every anchor of the batch also pairs with the live slots k < count of the ring: P(i) and N(i) grow by {k : ym_k = y_i} and {k : ym_k != y_i},
the formulas and the validity rules stay, the loss is still the mean over the valid anchors of the BATCH, and nothing flows to the ring
(include/pfr_hip.h at pfr_pair_mem_loss_fwd).  The ring is rank-local and not checkpointed: a resumed run starts with an empty one.

CUDA tensors run `PairLossFunction`: pfr_l2norm_fwd, ONE forward launch (csrc/pfr_pairloss.hip), then one backward launch and
pfr_l2norm_bwd; with a memory `PairMemLossFunction` (csrc/pfr_pairmem.hip); the mined kinds `PairMinedLossFunction`, with or without a memory.  CPU tensors run `pair_loss_torch` / `pair_loss_mem_torch`,
the same contract in torch ops in the tensor's own dtype; in float64 they are the oracles of the device tests."""
import torch
import torch.nn as nn
import torch.nn.functional as F

KINDS = ("supcon", "circle", "batch_hard", "multi_similarity")
MINED_KINDS = ("batch_hard", "multi_similarity")
_DEFAULTS = {"supcon": dict(tau=0.1), "circle": dict(m=0.25, gamma=64.0), "batch_hard": dict(m=0.3, gamma=0.0),
             "multi_similarity": dict(alpha=2.0, beta=50.0, base=0.5, epsilon=0.1)}


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
    if kind == "batch_hard" and not (p["m"] >= 0 and p["gamma"] >= 0):
        raise ValueError(f"batch_hard needs a margin >= 0 and gamma >= 0, got m={p['m']} gamma={p['gamma']}")
    if kind == "multi_similarity" and not (p["alpha"] > 0 and p["beta"] > 0 and p["epsilon"] >= 0 and p["base"] == p["base"]):
        raise ValueError(f"multi_similarity needs alpha > 0, beta > 0 and epsilon >= 0, got {p}")
    return p


def pair_mined_parts(s, pos, neg, kind, **params):
    """The mined kinds from the score matrix s [B, n] on (column j = partner number j) and the boolean sets pos / neg [B, n] -> dict:
    sp, sn (the extremes, detached, 0 where invalid), ip, inn (their partner numbers, -1 where invalid), valid, keep [B, n] (the pairs
    with a weight: p* and n* for batch_hard, the miner's choice for multi_similarity), x [B, n] (multi_similarity: the logits, part of the
    graph), a, b (batch_hard: z_i, f_i; multi_similarity: L_p, L_n; 0 where invalid, detached), rows (l_i, part of the graph)."""
    p = _params(kind, params)
    B, n = s.shape
    sd = s.detach()
    ok = ~torch.isnan(sd)                                           # a NaN score is in neither set
    pos, neg = pos & ok, neg & ok
    valid = pos.any(1) & neg.any(1)
    num = torch.arange(n, device=s.device).expand(B, n)
    inf = float("inf")

    def extreme(mask, sign):
        v = (sign * sd).masked_fill(~mask, inf).min(1).values       # min of s (sign = 1) or of -s
        at = mask & ((sign * sd) == v[:, None])                     # == : -0.0 ties with +0.0
        i = torch.where(at, num, n).min(1).values                   # the smallest partner number among the ties
        return i

    ip, inn = extreme(pos, 1.0), extreme(neg, -1.0)
    ipc, inc = ip.clamp_max(n - 1)[:, None], inn.clamp_max(n - 1)[:, None]
    zero = sd.new_zeros(B)
    sp = torch.where(valid, sd.gather(1, ipc).squeeze(1), zero)
    sn = torch.where(valid, sd.gather(1, inc).squeeze(1), zero)
    minus = torch.full_like(ip, -1)
    out = dict(sp=sp, sn=sn, ip=torch.where(valid, ip, minus), inn=torch.where(valid, inn, minus), valid=valid)
    if kind == "batch_hard":
        z = s.gather(1, inc).squeeze(1) - s.gather(1, ipc).squeeze(1) + p["m"]
        z = torch.where(valid, z, zero)
        g = p["gamma"]
        # the hinge is active iff z > 0 (clamp_min's backward would also pass the gradient at z = 0 exactly)
        rows = torch.where(z.detach() > 0, z, z * 0) if g == 0 else -F.logsigmoid(-g * z) / g
        f = (z.detach() > 0).to(s.dtype) if g == 0 else torch.sigmoid(g * z.detach())
        keep = (num == ipc) | (num == inc)
        out.update(x=s, a=z.detach(), b=torch.where(valid, f, zero), keep=keep & valid[:, None])
    else:
        al, be, lam, eps = p["alpha"], p["beta"], p["base"], p["epsilon"]
        keep = ((neg & (sd + eps > sp[:, None])) | (pos & (sd - eps < sn[:, None]))) & valid[:, None]
        x = torch.where(pos, -al * (s - lam), be * (s - lam))
        ninf = float("-inf")
        z0 = s.new_zeros(B, 1)                                      # the element 0 of log(1 + sum)
        Lp = torch.logsumexp(torch.cat([z0, x.masked_fill(~(keep & pos), ninf)], 1), 1)
        Ln = torch.logsumexp(torch.cat([z0, x.masked_fill(~(keep & neg), ninf)], 1), 1)
        rows = Lp / al + Ln / be
        out.update(x=x, a=torch.where(valid, Lp.detach(), zero), b=torch.where(valid, Ln.detach(), zero), keep=keep)
    out["rows"] = torch.where(valid, rows, zero)
    return out


def _mined_from_scores(s, pos, neg, kind, params):
    """-> (loss, l (detached), valid, logits) of the mined kinds, the return of pair_loss_from_scores"""
    r = pair_mined_parts(s, pos, neg, kind, **params)
    A = int(r["valid"].sum())
    if A == 0:
        return (s * 0).sum(), s.new_zeros(s.shape[0]), r["valid"], r["x"]        # 0.0 exactly, and a zero gradient
    return r["rows"].sum() / A, r["rows"].detach(), r["valid"], r["x"]


def pair_loss_from_scores(s, label, kind, s_alpha=None, **params):
    """The contract from the score matrix s [B, B] on: -> (loss, l [B] with 0 at invalid anchors (detached), valid [B] bool, logits [B, B]).
    `logits` is the matrix the log-sum-exps read (s / tau; Circle: the positive form where y_j = y_i, the negative form elsewhere), part of
    the graph: d loss / d logits is the softmax weight of every pair.  s_alpha: the scores Circle's alpha are taken from (None: s, detached)."""
    p = _params(kind, params)
    B = s.shape[0]
    same = label[:, None] == label[None, :]
    eye = torch.eye(B, dtype=torch.bool, device=s.device)
    pos, neg = same & ~eye, ~same
    if kind in MINED_KINDS:
        return _mined_from_scores(s, pos, neg, kind, params)
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


def pair_loss_mem_from_scores(s_batch, s_mem, label, mem_label, kind, s_alpha=None, **params):
    """pair_loss_from_scores with a memory: s_batch [B, B] are the scores inside the batch, s_mem [B, n] those against the n live slots of
    the ring (labels mem_label [n]; n may be 0).  -> (loss, l [B] with 0 at invalid anchors (detached), valid [B] bool, logits [B, B + n]).
    Only the batch items are anchors.  s_alpha: (batch, memory) scores Circle's alpha are taken from (None: the scores, detached)."""
    p = _params(kind, params)
    B, n = s_batch.shape[0], s_mem.shape[1]
    s = torch.cat([s_batch, s_mem], 1)
    same = label[:, None] == torch.cat([label, mem_label.to(label.device)])[None, :]
    eye = torch.cat([torch.eye(B, dtype=torch.bool, device=s.device), torch.zeros(B, n, dtype=torch.bool, device=s.device)], 1)
    pos, neg = same & ~eye, ~same
    if kind in MINED_KINDS:
        return _mined_from_scores(s, pos, neg, kind, params)
    valid = pos.any(1) if kind == "supcon" else pos.any(1) & neg.any(1)
    idx = valid.nonzero().squeeze(1)
    if kind == "supcon":
        x = s / p["tau"]
    else:
        m, gamma = p["m"], p["gamma"]
        sa = (s if s_alpha is None else torch.cat(list(s_alpha), 1)).detach()
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
        ell = -F.logsigmoid(-z)
    return ell.sum() / idx.numel(), rows.index_put((idx,), ell.detach()), valid, x


def pair_loss_mem_torch(emb, label, mem, mem_label, kind, normalize=True, eps=1e-12, alpha_emb=None, return_rows=False, **params):
    """pair_loss_torch with a memory: mem [n, D] are the live rows of the ring as they were stored (already normalised; used detached),
    mem_label [n] their labels.  normalize / alpha_emb / return_rows as in pair_loss_torch."""
    xn = F.normalize(emb, dim=1, eps=eps) if normalize else emb
    mem = mem.detach().to(xn.dtype)
    sa = None
    if alpha_emb is not None:
        an = F.normalize(alpha_emb, dim=1, eps=eps) if normalize else alpha_emb
        sa = (an @ an.t(), an @ mem.t())
    loss, rows, valid, _ = pair_loss_mem_from_scores(xn @ xn.t(), xn @ mem.t(), label, mem_label, kind, s_alpha=sa, **params)
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


class PairMemLossFunction(torch.autograd.Function):
    """PairLossFunction against the ring of `owner` (a PairLoss with memory > 0): pfr_l2norm_fwd + pfr_pair_mem_loss_fwd; backward:
    pfr_pair_mem_loss_bwd + pfr_l2norm_bwd.  `count` live slots are used (0 during the warm-up).  keep: leave ê and the labels with the
    owner as the rows its next training call pushes.  The backward refuses a ring that has been pushed to since this forward."""

    @staticmethod
    def forward(ctx, emb, label, owner, count, T, keep):
        from .._hip import ops
        emb = emb.contiguous()
        label = label.contiguous()
        B, D = emb.shape
        xn, xnT, inv = ops.l2norm_fwd(emb, T, want_t=True, ldt=(B + 31) // 32 * 32)
        owner._ensure(xn)
        out, stats, _ = ops.pair_mem_loss_fwd(xn, label, owner.mem, owner.mem_label, count, owner.kind, **owner.params)
        ctx.save_for_backward(emb, label, xn, xnT, inv, stats, out)
        ctx.owner, ctx.count, ctx.generation = owner, count, owner.generation
        if keep:
            owner._pending = (xn, label)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        from .._hip import ops
        emb, label, xn, xnT, inv, stats, out = ctx.saved_tensors
        o = ctx.owner
        o._guard(ctx.generation)
        dxn = ops.pair_mem_loss_bwd(xn, xnT, label, o.mem, o.memT, o.mem_label, ctx.count, stats, out, o.kind,
                                    grad_scale_dev=g.float().contiguous(), **o.params)
        demb = ops.l2norm_bwd(emb, inv, dxn, torch.float32)
        return demb.to(emb.dtype), None, None, None, None, None


class PairMinedLossFunction(torch.autograd.Function):
    """The mined kinds on the device: pfr_l2norm_fwd + pfr_pair_mined_fwd; backward: pfr_pair_mined_bwd + pfr_l2norm_bwd.  owner = None:
    the batch alone.  owner = a PairLoss with memory > 0: against its ring, with the `count`, `keep` and generation rules of
    PairMemLossFunction."""

    @staticmethod
    def forward(ctx, emb, label, kind, params, T, owner, count, keep):
        from .._hip import ops
        emb = emb.contiguous()
        label = label.contiguous()
        B = emb.shape[0]
        xn, xnT, inv = ops.l2norm_fwd(emb, T, want_t=True, ldt=(B + 31) // 32 * 32)
        ring = {}
        if owner is not None:
            owner._ensure(xn)
            ring = dict(mem=owner.mem, mem_label=owner.mem_label, count=count)
        out, stats, _ = ops.pair_mined_fwd(xn, label, kind, **ring, **params)
        ctx.save_for_backward(emb, label, xn, xnT, inv, stats, out)
        ctx.kind, ctx.params, ctx.owner, ctx.count = kind, params, owner, count
        if owner is not None:
            ctx.generation = owner.generation
            if keep:
                owner._pending = (xn, label)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        from .._hip import ops
        emb, label, xn, xnT, inv, stats, out = ctx.saved_tensors
        o = ctx.owner
        ring = {}
        if o is not None:
            o._guard(ctx.generation)
            ring = dict(mem=o.mem, memT=o.memT, mem_label=o.mem_label, count=ctx.count)
        dxn = ops.pair_mined_bwd(xn, xnT, label, stats, out, ctx.kind, grad_scale_dev=g.float().contiguous(), **ring, **ctx.params)
        demb = ops.l2norm_bwd(emb, inv, dxn, torch.float32)
        return demb.to(emb.dtype), None, None, None, None, None, None, None


class _RingGuard(torch.autograd.Function):
    """identity whose backward refuses a ring that has been pushed to since the forward (the CPU path of the generation guard)"""

    @staticmethod
    def forward(ctx, loss, owner):
        ctx.owner, ctx.generation = owner, owner.generation
        return loss.view_as(loss)

    @staticmethod
    def backward(ctx, g):
        ctx.owner._guard(ctx.generation)
        return g, None


class PairLoss(nn.Module):
    """PairLoss(kind, **params): forward(emb [B, D], label [B]) -> scalar.  kind 'supcon' (tau=0.1), 'circle' (m=0.25, gamma=64),
    'batch_hard' (m=0.3, gamma=0: the hinge; gamma > 0: softplus(gamma z) / gamma) or 'multi_similarity' (alpha=2, beta=50, base=0.5,
    epsilon=0.1).
    compute_dtype (fp32 / bf16; None = the default of the HIP engines, as the margin heads resolve it) is the dtype of ê on the device:
    in bf16 the scores come from the bf16-rounded ê with fp32 accumulation.  int8 is not supported.

    memory=M > 0 (a multiple of 32, B <= M): cross-batch memory.  The ring is `mem` [M, D], `memT` [D, M] and `mem_label` [M], non-persistent
    buffers allocated at the first batch in that batch's compute dtype (CPU: the tensor's dtype); a later change of dtype or D is an error.
    `head` and `count` are host integers.  The ring is not part of the state dict: a resumed run starts with an empty ring.
      * the push is deferred: a training-mode forward first pushes the PREVIOUS call's ê and labels, then computes the loss against the
        ring, so the backward reads the ring its forward saw.  Every push raises `generation`; a backward that finds a newer generation
        than its forward's (two forwards before the first backward) raises.
      * no push in eval mode or under torch.no_grad(): those calls read the ring and leave it alone.
      * memory_warmup=W: the first W training calls fill the ring but their loss uses no slot (early features drift).
      * rank-local: every process has its own ring."""

    def __init__(self, kind="supcon", memory=0, memory_warmup=0, compute_dtype=None, **params):
        super().__init__()
        self.kind = kind
        self.params = _params(kind, params)
        self.compute_dtype = compute_dtype
        self.memory, self.memory_warmup = int(memory), int(memory_warmup)
        if self.memory < 0 or self.memory % 32 or self.memory >= 1 << 24:
            raise ValueError(f"pair loss: memory must be 0 or a multiple of 32 below 2^24, got {memory}")
        if self.memory_warmup < 0 or (self.memory_warmup and not self.memory):
            raise ValueError(f"pair loss: memory_warmup needs memory > 0 and a count of calls >= 0, got {memory_warmup}")
        if self.memory:
            for name in ("mem", "memT", "mem_label"):
                self.register_buffer(name, None, persistent=False)
            self.reset_memory()

    def extra_repr(self):
        mem = f", memory={self.memory}, memory_warmup={self.memory_warmup}" if self.memory else ""
        return f"kind={self.kind!r}, " + ", ".join(f"{k}={v:g}" for k, v in self.params.items()) + mem

    # ---------------------------------------------------------------------------------------------- the ring
    def reset_memory(self):
        """empty the ring (the buffers are allocated again at the next batch)"""
        self.mem = self.memT = self.mem_label = None
        self.head = self.count = self.generation = self.train_calls = 0
        self._pending = None

    def _ensure(self, xn):
        if xn.shape[0] > self.memory:
            raise ValueError(f"pair loss: the batch ({xn.shape[0]}) is larger than the memory ({self.memory})")
        if self.mem is None:
            M, D = self.memory, xn.shape[1]
            self.mem = torch.zeros(M, D, dtype=xn.dtype, device=xn.device)
            self.memT = torch.zeros(D, M, dtype=xn.dtype, device=xn.device)      # zero beyond `count`: the kernels rely on it
            self.mem_label = torch.zeros(M, dtype=torch.int64, device=xn.device)
        elif self.mem.dtype != xn.dtype or self.mem.shape[1] != xn.shape[1] or self.mem.device != xn.device:
            raise ValueError(f"pair loss: the memory holds {self.mem.dtype} rows of length {self.mem.shape[1]} on {self.mem.device}, "
                             f"got {xn.dtype} rows of length {xn.shape[1]} on {xn.device} (reset_memory() starts a new ring)")

    def push(self, xn, label):
        """the normalised rows xn [B, D] and their labels into the slots (head + r) mod M, now"""
        xn, label = xn.detach().contiguous(), label.detach().contiguous()
        self._ensure(xn)
        B, M = xn.shape[0], self.memory
        if xn.is_cuda:
            from .._hip import ops
            ops.pair_mem_push(xn, label, self.mem, self.memT, self.mem_label, self.head)
        else:
            idx = (self.head + torch.arange(B)) % M
            self.mem[idx] = xn
            self.memT[:, idx] = xn.t()
            self.mem_label[idx] = label
        self.head = (self.head + B) % M
        self.count = min(self.count + B, M)
        self.generation += 1

    def _guard(self, generation):
        if generation != self.generation:
            raise RuntimeError(f"pair loss memory: the ring was pushed to (generation {self.generation}) after the forward of this backward "
                               f"(generation {generation}): run each backward before the next training-mode forward")

    def _forward_memory(self, emb, label, T):
        keep = self.training and torch.is_grad_enabled()
        if keep:
            if self._pending is not None:
                self.push(*self._pending)
                self._pending = None
            self.train_calls += 1
        # the warm-up covers the training calls 1 .. memory_warmup; a call that does not train reads the ring once those are done
        warm = self.train_calls <= self.memory_warmup if keep else self.train_calls < self.memory_warmup
        count = 0 if warm else self.count
        if emb.is_cuda and self.kind in MINED_KINDS:
            return PairMinedLossFunction.apply(emb, label, self.kind, self.params, T, self, count, keep)
        if emb.is_cuda:
            return PairMemLossFunction.apply(emb, label, self, count, T, keep)
        xn = F.normalize(emb, dim=1, eps=1e-12)
        self._ensure(xn)
        loss = pair_loss_mem_torch(xn, label, self.mem[:count], self.mem_label[:count], self.kind, normalize=False, **self.params)
        if keep:
            self._pending = (xn.detach(), label)
        return _RingGuard.apply(loss, self)

    def forward(self, emb, label, compute_dtype=None):
        if not emb.is_cuda:
            if self.memory:
                return self._forward_memory(emb, label, emb.dtype)
            return pair_loss_torch(emb, label, self.kind, **self.params)
        from ._head_hip import resolve_dtype
        T = resolve_dtype(self.compute_dtype or compute_dtype)
        if T not in (torch.float32, torch.bfloat16):
            raise ValueError(f"pair loss: the compute dtype is fp32 or bf16, got {T}")
        if self.memory:
            return self._forward_memory(emb, label, T)
        if self.kind in MINED_KINDS:
            return PairMinedLossFunction.apply(emb, label, self.kind, self.params, T, None, 0, False)
        return PairLossFunction.apply(emb, label, self.kind, T, self.params)


def build_pair_loss(spec):
    """dict(kind=..., weight=1.0, memory=0, memory_warmup=0, compute_dtype=None, **params) -> (PairLoss, weight)"""
    spec = dict(spec)
    if "kind" not in spec:
        raise ValueError(f"pair_loss needs a 'kind' (one of {list(KINDS)})")
    weight = float(spec.pop("weight", 1.0))
    return PairLoss(spec.pop("kind"), **spec), weight
