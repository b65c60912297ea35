"""Flat-buffer fused optimizers with the torch.optim interface (param_groups / step / zero_grad / state_dict), so the
config contract `optimizer(model_) -> ([optim], [sched])` (/root/reference/configs/dog_fe/fe_dogs_config.py:123-133,
body_dog_fe.py:121-131) and torch LR schedulers keep working.  Parameters that live in an FEEngine flat buffer are
updated with ONE kernel launch per contiguous range of a param group; any other CUDA parameter gets one launch.

Gradient clipping (`clip_grad_norm_` / `clip_grad_value_`, torch.nn.utils' argument conventions) is folded into the next
`step()`: the norm is reduced on the device (pfr_grad_norm) and the update kernels read its clip coefficient from device
memory, so there is no host sync and no extra pass that rewrites the gradients.  The gradients themselves are NOT scaled in
place; only the update uses the clipped values (PL steps right after clipping and zeroes the gradients before the next
backward, so a trainer cannot tell the difference).

Weight averaging (`attach_average('ema', decay)` / `attach_average('swa')`, torch.optim.swa_utils.AveragedModel's arithmetic): the
average is one more flat state buffer per run (`state[p]['avg']`).  An EMA is updated by the step kernel itself, which has the new
parameter in registers (pfr_*_step_avg: one more read and write of the average, no launch); SWA's running mean is updated by
`update_average()` (pfr_weight_avg per run).  `swap_averaged()` exchanges master and average; the engines re-derive everything
they compute with (compute-dtype shadow, weight layouts, folded inference weights) from the master at the next forward pass.

Row gradients (Partial FC with `sparse_grad=True`, losses/_head_hip.py): the head weight's `grad` stays None and backward leaves
`weight.row_grad = (index int32 [S], rows fp32 [S, D])`.  `FusedSGD.step()` updates exactly those rows with one launch
(pfr_sgd_step_rows) against a zero-initialised dense momentum state, `state[p]['momentum_buffer']`: unsampled rows and their momentum
are untouched (lazy momentum).  The clipping calls see `rows` as that parameter's gradient, `zero_grad()` clears `row_grad`.
FusedAdamW and an attached average refuse such a parameter."""
import contextlib

import torch

from .._hip import ops, PfrError


class _FusedBase(torch.optim.Optimizer):
    """State lives in `self.state[p]` like in torch.optim (so `state_dict()` / `load_state_dict()` round-trip and follow the
    parameters through `model.to()`): each entry is a VIEW, with the parameter's logical shape and strides, into one flat
    buffer per contiguous run of the group, which is what the kernels update."""
    _STATE_KEYS = ()

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._runs = {}      # group index -> (signature, [run, ...])
        self._clip_coef = None     # armed by clip_grad_norm_: 1-element device tensor, consumed by the next step()
        self._clip_value = 0.0     # armed by clip_grad_value_ (0 = off), consumed by the next step()
        self._norm = SegmentNorm()
        self._avg = None           # attach_average: (kind, decay)
        self.n_averaged = 0        # updates the average has seen (AveragedModel.n_averaged); saved in state_dict()

    # ------------------------------------------------------------------------------------------ weight averaging
    def attach_average(self, kind, decay=None):
        """Keep an averaged copy of every parameter this optimizer updates, as `state[p]['avg']`.  'ema': avg <- decay * avg +
        (1 - decay) * p after every step(), inside the update kernel; 'swa': avg <- running mean of the parameters at the calls
        of update_average().  The first update copies the parameters (torch's AveragedModel)."""
        self._avg = _check_average(kind, decay)
        self._runs = {}            # re-pack with the extra state buffer at the next step

    def _state_keys(self):
        return self._STATE_KEYS + ("avg",) if self._avg is not None else self._STATE_KEYS

    def _avg_weight(self):
        return _average_weight(self._avg, self.n_averaged)

    def _ema(self):
        return self._avg is not None and self._avg[0] == "ema"

    def _avg_pairs(self):
        """[(avg, p)] flat fp32 tensors covering every averaged parameter: the run buffers where the cached runs are current,
        any other parameter (no step since attach / load_state_dict, or not in a flat run) on its own"""
        pairs = []
        for gi, group in enumerate(self.param_groups):
            done = set()
            cached = self._runs.get(gi)
            if cached is not None and cached[0] == tuple((id(p), p.data_ptr()) for p in group["params"] if p.grad is not None) \
                    and all("avg" in r["state"] for r in cached[1]):
                for r in cached[1]:
                    pairs.append((r["state"]["avg"], r["pf"]))
                    done.update(id(p) for p, _ in r["members"])
            for p in group["params"]:
                st = self.state[p] if p in self.state else {}
                a = st.get("avg")
                if a is None or id(p) in done:
                    continue
                if a.device != p.device or a.stride() != p.stride():
                    a = st["avg"] = torch.empty_like(p.data).copy_(a)
                pairs.append((_flat_alias(a), _flat_alias(p.data)))
        return pairs

    @torch.no_grad()
    def update_average(self):
        """One update of the average from the current parameters (pfr_weight_avg per run): SWA's per-epoch call.  A parameter
        that has no average yet (never stepped: frozen, or unused so far) gets one here, starting from its current value, so
        that every parameter of the groups is averaged from this call on; one that joins after the first update therefore
        counts its current value for the updates it missed."""
        if self._avg is None:
            raise PfrError("update_average: attach_average() first")
        for group in self.param_groups:
            for p in group["params"]:
                if "avg" not in self.state[p]:
                    if not p.is_cuda or p.dtype != torch.float32:
                        raise PfrError("fused optimizers need fp32 CUDA parameters (use optim.WeightAverage on the CPU path)")
                    self.state[p]["avg"] = torch.empty_like(p.data).copy_(p.data)
        w = self._avg_weight()
        for a, p in self._avg_pairs():
            ops.weight_avg(a, p, w)
        self.n_averaged += 1

    @contextlib.contextmanager
    def swap_averaged(self):
        """Inside the block the parameters hold the average and `state[p]['avg']` the live weights; leaving it swaps back, bit
        for bit.  The engines read the master buffer at every forward pass (cast to the compute dtype, stem / data-gradient
        layouts; the folded inference weights are keyed on a checksum of it), so they follow without a call."""
        self.swap_averaged_()
        try:
            yield self
        finally:
            self.swap_averaged_()

    @torch.no_grad()
    def swap_averaged_(self):
        """the explicit half of swap_averaged(): exchanges parameters and average once"""
        _swap([(p.data, self.state[p]["avg"]) for g in self.param_groups for p in g["params"]
               if p in self.state and "avg" in self.state[p]])

    def state_dict(self):
        sd = super().state_dict()
        if self._avg is not None:
            sd["weight_average"] = {"kind": self._avg[0], "decay": self._avg[1], "n_averaged": self.n_averaged}
        return sd

    def _grads(self):
        """every gradient of every group in parameter order; a parameter with a row gradient contributes its rows"""
        grads = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    grads.append(p.grad)
                elif _row_grad(p) is not None:
                    grads.append(_row_grad(p)[1])
        return grads

    def zero_grad(self, set_to_none=True):
        super().zero_grad(set_to_none=set_to_none)
        for group in self.param_groups:
            for p in group["params"]:
                if _row_grad(p) is not None:
                    p.row_grad = None

    def _row_params(self, group):
        """the group's parameters that carry a row gradient (and no dense one), refused where the rows cannot be honoured"""
        rows = [p for p in group["params"] if p.grad is None and _row_grad(p) is not None]
        if rows and not isinstance(self, FusedSGD):
            raise PfrError(f"{type(self).__name__} has no row-wise update for a Partial FC head with sparse_grad=True: "
                           "use FusedSGD, or build the head with sparse_grad=False")
        if rows and self._avg is not None:
            raise PfrError("an attached EMA / SWA average does not follow a Partial FC head with sparse_grad=True (its rows are "
                           "updated outside the flat buffers): build the head with sparse_grad=False")
        return rows

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm, norm_type=2.0):
        """torch.nn.utils.clip_grad_norm_ over every gradient of every param group: returns the total norm as a 0-d device tensor
        (no host sync) and arms its clip coefficient min(1, max_norm / (total + 1e-6)) for the next step().  norm_type 1, 2 or
        inf (any other p > 0 too).  The gradients are not modified; the next step() uses them scaled by the coefficient."""
        grads = self._grads()
        if not grads:
            return torch.tensor(0.0)
        out = self._norm.compute(grads, norm_type, max_norm)
        self._clip_coef = out[len(grads) + 1:]
        return out[len(grads)]

    def clip_grad_value_(self, clip_value):
        """torch.nn.utils.clip_grad_value_: the next step() uses every gradient clamped to [-clip_value, clip_value] (the
        gradients themselves are not modified).  clip_value must be > 0."""
        clip_value = float(clip_value)
        if not clip_value > 0:
            raise ValueError(f"clip_value must be > 0, got {clip_value}")
        self._clip_value = clip_value

    def _take_clip(self):
        """-> (coefficient tensor or None, clamp value or 0.0) armed for this step, and disarms them"""
        armed = (self._clip_coef, self._clip_value)
        self._clip_coef, self._clip_value = None, 0.0
        return armed

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._runs = {}      # loaded tensors are private copies: re-pack them into flat run buffers at the next step
        wa = state_dict.get("weight_average")
        if wa is not None:
            if self._avg is None:
                self._avg = _check_average(wa["kind"], wa["decay"])
            self.n_averaged = int(wa["n_averaged"])

    def _group_runs(self, gi, group):
        params = [p for p in group["params"] if p.grad is not None]
        # the state layout follows the PARAMETERS; a gradient that autograd re-allocated (the ArcFace head's, 20 MB) only moves
        # the run's gradient view — it must not rebuild (re-allocate and copy) every state buffer of the group
        sig = tuple((id(p), p.data_ptr()) for p in params)
        gsig = tuple(p.grad.data_ptr() for p in params)
        cached = self._runs.get(gi)
        if cached is not None and cached[0] == sig:
            if cached[2] != gsig:
                if not self._rebind_grads(cached[1]):
                    cached = None
                else:
                    self._runs[gi] = (sig, cached[1], gsig)
            if cached is not None:
                return cached[1]
        if any(not p.is_cuda for p in params):
            raise PfrError("fused optimizers need CUDA parameters (use torch.optim on the CPU path)")
        runs = self._build_runs(params)
        for r in runs:
            n = r["n"]
            dev = r["pf"].device
            r["state"] = {k: torch.zeros(n, dtype=torch.float32, device=dev) for k in self._state_keys()}
            for p, off in r["members"]:
                st = self.state[p]
                for k in self._state_keys():
                    view = torch.as_strided(r["state"][k], p.shape, p.stride(), off)
                    old = st.get(k)
                    if old is not None:
                        view.copy_(old.to(dev))     # carried over (loaded checkpoint, or a previous buffer layout)
                    elif k == "avg":
                        view.copy_(p.data)          # a parameter that joins a running average starts from its own value
                    st[k] = view
        self._runs[gi] = (sig, runs, gsig)
        return runs

    def _rebind_grads(self, runs):
        """gradient tensors moved: re-point the flat gradient view of every run (False: the members' gradients no longer form
        the same dense run, rebuild everything)"""
        for r in runs:
            p0, _ = r["members"][0]
            sp = self._storage_span(p0.grad)
            if sp is None:
                return False
            gs = sp[0]
            for p, off in r["members"]:
                s2 = self._storage_span(p.grad)
                if s2 is None or s2[0] != gs + 4 * off or p.grad.untyped_storage().data_ptr() != p0.grad.untyped_storage().data_ptr():
                    return False
            goff = (gs - p0.grad.untyped_storage().data_ptr()) // 4
            r["gs"], r["ge"], r["gbase"] = gs, gs + 4 * r["n"], p0.grad.untyped_storage().data_ptr()
            r["gf"] = torch.empty(0, dtype=torch.float32, device=p0.device).set_(p0.grad.untyped_storage(), goff, (r["n"],), (1,))
        return True

    def _build_runs(self, params):
        """→ runs covering `params` with as few flat tensors as possible.  Neighbours are merged only across the engine's
        ALIGNMENT PADDING (< 64 floats): a gap of a whole 64-element parameter (e.g. a BN bias of another param group lying
        between two weights) must not be swallowed into this group's update."""
        dense = []
        for p in params:
            if p.dtype != torch.float32:
                raise PfrError("fused optimizers need fp32 parameters")
            st_p = self._storage_span(p.data)
            st_g = self._storage_span(p.grad)
            if st_p is None or st_g is None:
                raise PfrError("fused optimizers need parameters/gradients that are dense in memory")
            dense.append((st_p, st_g, p))
        dense.sort(key=lambda t: t[0][0])
        runs = []
        for (pa, pn), (ga, gn), p in dense:
            r = runs[-1] if runs else None
            # merge only across the engine's alignment padding of the PREVIOUS member ((-numel) % 64 floats): a small parameter
            # of another group (or a frozen one) lying in a larger gap must not be swallowed into this group's update
            if r is not None and pa - r["pe"] == 4 * ((-r["last_n"]) % 64) and (ga - r["ge"]) == (pa - r["pe"]) \
                    and r["pbase"] == p.data.untyped_storage().data_ptr() \
                    and r["gbase"] == p.grad.untyped_storage().data_ptr():
                r["members"].append((p, (pa - r["ps"]) // 4))
                r["pe"] = pa + 4 * pn
                r["ge"] = ga + 4 * pn
                r["last_n"] = pn
            else:
                runs.append({"ps": pa, "pe": pa + 4 * pn, "gs": ga, "ge": ga + 4 * pn, "p": p, "members": [(p, 0)], "last_n": pn,
                             "pbase": p.data.untyped_storage().data_ptr(), "gbase": p.grad.untyped_storage().data_ptr()})
        for r in runs:
            n = (r["pe"] - r["ps"]) // 4
            p = r["p"]
            poff = (r["ps"] - r["pbase"]) // 4
            goff = (r["gs"] - r["gbase"]) // 4
            r["n"] = n
            r["pf"] = torch.empty(0, dtype=torch.float32, device=p.device).set_(p.data.untyped_storage(), poff, (n,), (1,))
            r["gf"] = torch.empty(0, dtype=torch.float32, device=p.device).set_(p.grad.untyped_storage(), goff, (n,), (1,))
        return runs

    def _flat_views(self, group):
        """(param_flat, grad_flat, (address, numel)) per run — kept for tests / introspection"""
        return [(r["pf"], r["gf"], (r["ps"], r["n"])) for r in self._build_runs([p for p in group["params"] if p.grad is not None])]

    @staticmethod
    def _storage_span(t):
        """(address, numel) if t occupies one dense block of memory (any permutation of a contiguous tensor)."""
        n = t.numel()
        if n == 0:
            return None
        sizes, strides = list(t.shape), list(t.stride())
        order = sorted(range(len(sizes)), key=lambda i: -strides[i])
        expect = 1
        for i in reversed(order):
            if sizes[i] != 1 and strides[i] != expect:
                return None
            expect *= sizes[i]
        return (t.data_ptr(), n)


def _row_grad(p):
    """(index, rows) left on a parameter by a Partial FC backward with sparse_grad=True, else None"""
    return getattr(p, "row_grad", None)


def _check_average(kind, decay):
    if kind not in ("ema", "swa"):
        raise ValueError(f"weight average kind must be 'ema' or 'swa', got {kind!r}")
    if kind == "ema":
        if decay is None or not 0.0 < float(decay) < 1.0:
            raise ValueError(f"an 'ema' average needs 0 < decay < 1, got {decay}")
        return ("ema", float(decay))
    if decay is not None:
        raise ValueError("an 'swa' average takes no decay")
    return ("swa", None)


def _average_weight(avg, n_averaged):
    """lerp weight of the next update: 1 (copy) for the first one, then 1 - decay (EMA) or 1 / (n_averaged + 1) (SWA)"""
    if n_averaged == 0:
        return 1.0
    return 1.0 - avg[1] if avg[0] == "ema" else 1.0 / (n_averaged + 1)


def _flat_alias(t):
    """the memory of a dense tensor (any permutation of a contiguous one) as a flat tensor"""
    if _FusedBase._storage_span(t) is None:
        raise PfrError("weight averaging needs parameters that are dense in memory")
    return torch.as_strided(t, (t.numel(),), (1,), t.storage_offset())


def _swap(pairs):
    if not pairs:
        return
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    tmp = [x.clone() for x in a]
    torch._foreach_copy_(a, b)
    torch._foreach_copy_(b, tmp)


class WeightAverage:
    """The averaging interface of the fused optimizers (update_average / swap_averaged / n_averaged / state_dict) for
    parameters stepped by a torch optimizer (the CPU path): `torch._foreach_lerp_`, torch.optim.swa_utils.AveragedModel's
    arithmetic.  With kind 'ema' the caller runs update_average() after every optimizer step."""

    def __init__(self, params, kind, decay=None):
        self._avg = _check_average(kind, decay)
        self.params = [p for p in params]
        self.avg = [p.detach().clone() for p in self.params]
        self.n_averaged = 0

    @torch.no_grad()
    def update_average(self):
        cur = [p.detach() for p in self.params]
        if self.n_averaged == 0:
            torch._foreach_copy_(self.avg, cur)
        else:
            torch._foreach_lerp_(self.avg, cur, _average_weight(self._avg, self.n_averaged))
        self.n_averaged += 1

    @contextlib.contextmanager
    def swap_averaged(self):
        self.swap_averaged_()
        try:
            yield self
        finally:
            self.swap_averaged_()

    @torch.no_grad()
    def swap_averaged_(self):
        _swap([(p.data, a) for p, a in zip(self.params, self.avg)])

    def state_dict(self):
        return {"kind": self._avg[0], "decay": self._avg[1], "n_averaged": self.n_averaged, "avg": [a.clone() for a in self.avg]}

    @torch.no_grad()
    def load_state_dict(self, sd):
        if len(sd["avg"]) != len(self.avg):
            raise ValueError(f"WeightAverage: the state holds {len(sd['avg'])} tensors, this average {len(self.avg)}")
        for a, v in zip(self.avg, sd["avg"]):
            a.copy_(v)
        self.n_averaged = int(sd["n_averaged"])


def norm_order(norm_type):
    """torch norm_type -> pfr_grad_norm's norm_p: any p > 0, math.inf for the max norm"""
    p = float(norm_type)
    if not p > 0:
        raise PfrError(f"the device gradient norm needs norm_type > 0 (or inf), got {norm_type}")
    return p


class SegmentNorm:
    """Norms of a list of dense fp32 CUDA gradients on the device: one pfr_grad_norm call (two launches), no host sync.  Each
    gradient is one segment, so alignment padding between parameters of a flat buffer never enters.  The descriptor tables of
    the last layout seen are kept and rebuilt when a gradient moves.  compute(..., copy_other=True) also takes gradients of
    another dtype or a strided layout, as a contiguous fp32 copy (what the norm reads is the same values)."""

    def __init__(self):
        self._key = None

    def _tables(self, grads):
        key = tuple((g.data_ptr(), g.numel()) for g in grads)
        if key == self._key:
            return
        dev = grads[0].device
        ce = ops.grad_norm_chunk_elems()
        rows, chunk_seg, c0 = [], [], 0
        for i, g in enumerate(grads):
            if g.dtype != torch.float32 or not g.is_cuda or g.device != dev:
                raise PfrError("the device gradient norm needs fp32 CUDA gradients on one device")
            span = _FusedBase._storage_span(g)
            if span is None and g.numel() > 0:
                raise PfrError("the device gradient norm needs gradients that are dense in memory")
            n = g.numel()
            nch = -(-n // ce)
            rows.append((span[0] if n else 0, n, c0, nch))
            chunk_seg += [i] * nch
            c0 += nch
        # (pinned + non_blocking: no host sync; the caching host allocator keeps the staging buffers alive until the copies ran)
        self._segs = torch.tensor(rows, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        self._chunk_seg = torch.tensor(chunk_seg or [0], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        self._ws = torch.empty(c0 + len(grads), dtype=torch.float64, device=dev)
        self._nchunks = c0
        self._key = key

    def compute(self, grads, norm_type=2.0, max_norm=1.0, copy_other=False):
        """-> fp32 device tensor [len(grads) + 2]: every gradient's norm, the total norm (torch's norm of the stacked per-tensor
        norms), then the clip coefficient min(1, max_norm / (total + 1e-6))"""
        p = norm_order(norm_type)
        if copy_other:
            # (a copy is freed when this call returns; the caching allocator hands its memory only to work queued after the norm)
            grads = [g if g.dtype == torch.float32 and _FusedBase._storage_span(g) is not None
                     else g.detach().float().contiguous() for g in grads]
        self._tables(grads)
        out = torch.empty(len(grads) + 2, dtype=torch.float32, device=grads[0].device)
        ops.grad_norm(self._segs, self._chunk_seg, len(grads), self._nchunks, p, max_norm, self._ws, out)
        return out


class FusedSGD(_FusedBase):
    _STATE_KEYS = ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0, weight_decay=0.0, nesterov=False):
        if dampening != 0 or nesterov:
            raise PfrError("FusedSGD supports dampening=0, nesterov=False (what the reference configs use)")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        coef, clip_value = self._take_clip()
        clip = coef is not None or clip_value > 0
        ema = self._ema()
        avg_w = self._avg_weight() if ema else 0.0
        for gi, group in enumerate(self.param_groups):
            for r in self._group_runs(gi, group):
                # a zero-initialised buffer makes torch's "first step: buf = d" the general rule buf = momentum*buf + d
                buf = r["state"]["momentum_buffer"] if group["momentum"] != 0 else None
                if ema:
                    ops.sgd_step_avg(r["pf"], r["gf"], buf, None, group["lr"], group["momentum"], group["weight_decay"], coef,
                                     clip_value, r["state"]["avg"], avg_w, first_step=False)
                elif clip:
                    ops.sgd_step_clip(r["pf"], r["gf"], buf, None, group["lr"], group["momentum"], group["weight_decay"], coef,
                                      clip_value, first_step=False)
                else:
                    ops.sgd_step(r["pf"], r["gf"], buf, None, group["lr"], group["momentum"], group["weight_decay"], first_step=False)
            for p in self._row_params(group):
                index, rows = _row_grad(p)
                if not p.is_cuda or p.dtype != torch.float32 or p.dim() != 2 or not p.is_contiguous():
                    raise PfrError("a row gradient needs a contiguous fp32 [C, D] CUDA parameter")
                st = self.state[p]
                buf = st.get("momentum_buffer")
                if group["momentum"] != 0 and (buf is None or buf.shape != p.shape or buf.device != p.device or not buf.is_contiguous()):
                    # lazy momentum: a dense zero-initialised state of its own (a loaded or earlier buffer is carried over)
                    new = torch.zeros_like(p.data)
                    if buf is not None and buf.shape == p.shape:
                        new.copy_(buf)
                    buf = st["momentum_buffer"] = new
                ops.sgd_step_rows(p.data, index, rows, buf if group["momentum"] != 0 else None, group["lr"], group["momentum"],
                                  group["weight_decay"], coef, clip_value)
        if ema:
            self.n_averaged += 1
        return loss


class FusedAdamW(_FusedBase):
    _STATE_KEYS = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._t = 0

    def state_dict(self):
        for group in self.param_groups:
            for p in group["params"]:
                if p in self.state:
                    self.state[p]["step"] = torch.tensor(float(self._t))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        steps = [float(st["step"]) for st in self.state.values() if "step" in st]
        self._t = int(max(steps)) if steps else 0

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._t += 1
        coef, clip_value = self._take_clip()
        clip = coef is not None or clip_value > 0
        ema = self._ema()
        avg_w = self._avg_weight() if ema else 0.0
        for gi, group in enumerate(self.param_groups):
            self._row_params(group)
            for r in self._group_runs(gi, group):
                if ema:
                    ops.adamw_step_avg(r["pf"], r["gf"], r["state"]["exp_avg"], r["state"]["exp_avg_sq"], None, group["lr"],
                                       group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"], self._t, coef,
                                       clip_value, r["state"]["avg"], avg_w)
                elif clip:
                    ops.adamw_step_clip(r["pf"], r["gf"], r["state"]["exp_avg"], r["state"]["exp_avg_sq"], None, group["lr"],
                                        group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"], self._t, coef,
                                        clip_value)
                else:
                    ops.adamw_step(r["pf"], r["gf"], r["state"]["exp_avg"], r["state"]["exp_avg_sq"], None, group["lr"],
                                   group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"], self._t)
        if ema:
            self.n_averaged += 1
        return loss
