"""PlanEngine — the plan runtime and the plan builder shared by the seven engines: models/_fe_engine.FEEngine (ResNet), _swin_engine,
_convnext_engine, _vit_engine, _mobilenet_engine, _efficientnet_engine and _iresnet_engine.

An engine turns a model into pre-built launch lists ("plans": C-ABI calls with fixed device pointers, one plan per input
shape).  Everything that makes such a list a training step on two streams is model-independent and lives here, once:

  * Plan / PlanTicket and the plan cache: one plan instance ("slot") per forward pass that still waits for its backward,
    evict-oldest-idle, rebuild after a pfr_set_tuning call (acquire_plan, _check_tuning);
  * resolve(): the builders emit the stream roles of csrc/pfr_plan.hip directly (kinds of _hip/cplan.py); only late-bound
    entries stay symbolic — ("wgrad", args): split-K workspace pointer + accumulate flag, ("acc", (fn, args)): accumulate
    flag appended, anything else goes to the engine's _resolve_op — and are resolved into one list per accumulate variant;
  * replay: through the C executor (_run_list; its events belong to the CPlan) or, under PFR_C_PLAN=0 and always under a
    launch tracer, through run_ops, the one Python interpreter of the roles (its events belong to the engine);
  * the side-stream policy (_side_ok), the side-stream half of refresh_weights and the matching wait in backward;
  * the autograd wrapper (engine_forward);
  * PlanBuilder, the build-time half: the forward and backward lists of one plan, the backward buffer pool, the side-stream
    fork / join bookkeeping, the split-K workspace sizing, the deferred column sums and the grad-ready marks;
  * parameter adoption (_adopt_flat; _adopt_batchnorms and the 1x1 / stem records of the BatchNorm networks), the tail of
    forward() (_forward_plan) and backward().

Who uses what: all seven engines use the runtime.  Swin, ConvNeXt, ViT, MobileNetV2, EfficientNet and IResNet build their plans with
PlanBuilder and the layer emitters of models/_plan_layers.py (Linear / LayerNorm family: Swin, ConvNeXt, ViT; BatchNorm family:
MobileNetV2, EfficientNet, IResNet), adopt their parameters with _adopt_flat and run _forward_plan and backward() as they stand.  FEEngine
keeps a builder of its own (a FIFO pool with a measured lag, weight gradients that carry a BatchNorm prologue, a second workspace),
its own _adopt, forward and backward.

The engines keep what is theirs: the layer records, build_plan's model-specific middle, the argument checks of forward()."""
import os
import struct
import weakref

import torch

from .._hip import lib, dtype_id, PfrError
from .._hip.lib import _TRACER
from .._hip.cplan import CPlan, SIDE, FORK, SREC, WAIT, MWAIT

_ALIGN = 64  # elements; keeps every parameter 16-byte aligned in both fp32 and bf16 shadows


def default_compute_dtype():
    v = os.environ.get("PFR_COMPUTE_DTYPE", "bf16").lower()
    return torch.float32 if v in ("f32", "fp32", "float32") else torch.bfloat16


def _padded(n):
    return (n + _ALIGN - 1) // _ALIGN * _ALIGN


def flat_offsets(named):
    """name -> offset (in elements) of every (name, parameter) inside the flat master / gradient buffers, and their length:
    in the order given, each parameter padded to a multiple of _ALIGN elements"""
    offs, total = {}, 0
    for name, p in named:
        offs[name] = total
        total += _padded(p.numel())
    return offs, total


def _side_with_ddp():
    """main + side + communication stream + RCCL's internal stream need more than HIP's default 4 hardware queues: with
    4, two of them share a queue and serialise (measured 9.05 k vs 9.70 k img/s); the package asks for 8 at import."""
    try:
        return int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) >= 8
    except ValueError:
        return False


class PlanTicket:
    """Held by the autograd node of one forward pass: while it is alive (and its backward has not run) the plan that
    produced the saved activations is not handed to another forward pass."""
    __slots__ = ("__weakref__",)


class Plan:
    """ops: the forward list followed (from meta["n_fwd"]) by the backward list as built; bufs: every buffer the lists point
    into; meta: the resolved lists ("fwd", "bwd*"), their compiled C plans ("c_*"), the owner ticket, engine-specific notes"""
    __slots__ = ("ops", "bufs", "meta")

    def __init__(self):
        self.ops = []
        self.bufs = {}
        self.meta = {}

    def keep(self, t):
        self.bufs[len(self.bufs)] = t
        return t


def run_ops(ops, main, side, events, hook, hook_syncs_side):
    """The roles of csrc/pfr_plan.hip (what pfr_plan_run does for hook_stops 0 / 1 / 2) on torch streams: `side` None = side
    stream off (SIDE launches go to main, the sync kinds do nothing); FORK k: events[2k] recorded on main, side waits for it;
    SREC k: events[2k+1] recorded on side; WAIT k: main waits for events[2k+1]; MWAIT k: the same, but only for a hook that
    does not synchronise with the side stream itself; (None, (off,)): hook(off) when a hook is given."""
    ev = events
    stream = main.cuda_stream
    sptr = stream if side is None else side.cuda_stream
    mwait = hook is not None and not hook_syncs_side
    for fn, args in ops:
        if fn is None:
            if hook is not None:
                hook(args[0])
        elif fn.__class__ is int:
            if fn == SIDE:
                args[0](*args[1], sptr)
            elif side is None:
                pass
            elif fn == FORK:
                e = ev[2 * args]
                e.record(main)
                side.wait_event(e)
            elif fn == SREC:
                ev[2 * args + 1].record(side)
            elif fn == WAIT or mwait:
                main.wait_event(ev[2 * args + 1])
        else:
            fn(*args, stream)


class _Rec:
    pass


class PlanBuilder:
    """The build-time state of one plan: the forward and backward lists, and for the backward list the buffer pool, the side
    stream's fork / join bookkeeping, the split-K workspace need of the weight gradients and the deferred column sums.

    Weight gradients and bias / normalisation-parameter column sums feed nothing before the optimizer: they run on a SIDE stream
    (≈ 150 short launches per step that would otherwise sit in the dependency chain).  Stream roles (_hip/cplan.py): (FORK, k)
    side waits for main's current point; (SREC, k) side records "op k done"; (WAIT, k) main waits for op k — emitted before a pooled
    buffer that op k read is handed out again, before grad-ready marks and at the end.  Only the weight gradients stay symbolic
    ("wgrad": PlanEngine.resolve fills the split-K workspace pointer in)."""

    def __init__(self, plan, dtype, device, did, pool_depth):
        self.plan, self.dtype, self.device, self.did, self.pool_depth = plan, dtype, device, did, pool_depth
        self.fwd, self.bwd = [], []
        self.pool = {}         # (shape, dtype) class -> released buffers, oldest first
        self.nalloc = {}       # buffers allocated per class
        self.pending = {}      # data_ptr of a pooled buffer -> last side op that reads it
        self.side_reads = []   # (k, data_ptr) of every side-op input
        self.nside = 0
        self.ws_need = 0       # floats of split-K workspace the largest weight gradient needs
        self.pend_cs = []      # column sums whose final merge is deferred to the next flush: (partials, out, partial rows, C, tile height | 0, rows)

    def A(self, shape, dtype=None):
        return self.plan.keep(torch.empty(shape, dtype=dtype or self.dtype, device=self.device))

    def G(self, shape, dtype=None):
        key = (tuple(shape), dtype or self.dtype)
        lst = self.pool.setdefault(key, [])
        for i, t in enumerate(lst):              # a buffer no side op is reading
            if t.data_ptr() not in self.pending:
                return lst.pop(i)
        if not lst or self.nalloc.get(key, 0) < self.pool_depth:    # rotation so that the side stream may lag behind without stalling main
            self.nalloc[key] = self.nalloc.get(key, 0) + 1
            return self.A(shape, dtype)
        t = lst.pop(0)
        self.bwd.append((WAIT, self.pending.pop(t.data_ptr())))
        return t

    def release(self, t):
        lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
        ks = [k for k, ptr in self.side_reads if lo <= ptr < hi]
        if ks:
            self.pending[t.data_ptr()] = max(ks)
        self.side_reads[:] = [(k, ptr) for k, ptr in self.side_reads if not (lo <= ptr < hi)]
        self.pool.setdefault((tuple(t.shape), t.dtype), []).append(t)

    def side(self, op, *reads):
        ops = self.bwd
        if ops and ops[-1][0] == SREC:
            # no main-stream launch since the previous side op: it joins that op's fork (every fork is an event recorded on the
            # main stream, i.e. a marker packet in front of the next kernel of the dependency chain)
            k = ops.pop()[1]
        else:
            k = self.nside
            self.nside += 1
            ops.append((FORK, k))
        ops.append(op)
        ops.append((SREC, k))
        for r in reads:
            self.side_reads.append((k, r.data_ptr()))

    def wgrad(self, x, xshape, dy, dyshape, R, stride, pad, out):
        Nq, Hq, Wq, Cq = xshape
        _, OH, OW, Co = dyshape
        KK = R * R * Cq
        splits = lib.pfr_conv2d_wgrad_splits(Nq * OH * OW, Co, KK)
        self.ws_need = max(self.ws_need, splits * Co * KK)
        self.side(("wgrad", (x.data_ptr(), dy.data_ptr(), out.data_ptr(), None, self.did, Nq, Hq, Wq, Cq, Co, R, R, stride, pad,
                             OH, OW, Co, 0, 0, 0, 1.0, 0)), dy)

    def colsum(self, x, rows, C, out, dt=None):
        """bias / LayerNorm-parameter / position-table gradient = column sum of x; the partial sums run now (side stream), the
        ~100 tiny final merges of a step are batched into one launch per DDP bucket boundary (flush_colsums)"""
        d = dt if dt is not None else self.did
        n = lib.pfr_colsum_parts(d, rows, C)
        if n <= 0:   # a few hundred rows: one small kernel does it all
            self.side((SIDE, (lib.pfr_colsum, (x.data_ptr(), d, rows, C, out.data_ptr(), 0, 0))), x)
            return
        ws = self.A((lib.pfr_colsum_ws_floats(rows, C),), torch.float32)   # its own workspace: alive until the batched final
        self.side((SIDE, (lib.pfr_colsum_partial, (x.data_ptr(), d, rows, C, ws.data_ptr()))), x)
        self.pend_cs.append((ws, out, n, C, 0, 0))

    def flush_colsums(self):
        pend = self.pend_cs
        if not pend:
            return
        raw = b"".join(struct.pack("<QQiiiiii", ws.data_ptr(), out.data_ptr(), n, C, 0, mt, rws, 0) for ws, out, n, C, mt, rws in pend)
        tab = self.plan.keep(torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device))
        self.side((SIDE, (lib.pfr_colsum_final_batch, (tab.data_ptr(), len(pend), max(e[3] for e in pend)))))
        del pend[:]

    def mark(self, off, last=False):
        """grad-ready mark (DDP bucket boundary; `last`: the end of the backward pass): flat gradients [off, end) are final"""
        self.flush_colsums()
        if self.nside:   # everything the side stream was given so far is final
            self.bwd.append((WAIT if last else MWAIT, self.nside - 1))
        self.bwd.append((None, (off,)))

    def finish(self, engine):
        plan = self.plan
        plan.meta["n_side"] = self.nside
        if engine.ws is None or engine.ws.numel() < self.ws_need:
            engine.ws = torch.empty(self.ws_need, dtype=torch.float32, device=self.device)
        plan.ops = self.fwd + self.bwd
        return plan


class PlanEngine:
    max_plans = 8            # plans kept (all shapes and slots) before the oldest idle one is evicted
    bwd_lists = ("bwd",)     # resolved backward lists, one per value of the accumulate flag (0, 1, ...)
    # buffers per (shape, dtype) class of the backward pool before one that a side-stream op still reads is re-used (HBM is
    # plentiful; a shallow pool makes the main stream wait for the side stream at almost every layer)
    pool_depth = 48

    def __init__(self, model, device, compute_dtype=None):
        if not str(device).startswith("cuda"):
            raise PfrError(f"{type(self).__name__} runs on the HIP device only (no CPU fallback)")
        lib.pfr_version()  # fail loudly if the shared library is missing
        self.device = torch.device(device)
        self.dtype = compute_dtype or default_compute_dtype()
        self.did = dtype_id(self.dtype)
        self.kp = 8 if self.dtype == torch.bfloat16 else 4
        self.model_id = id(model)
        self._init_runtime()

    def _init_runtime(self):
        self.plans = {}
        self._last_plan = None
        self._tuning_epoch = None
        self.ws = None            # split-K workspace of the weight-gradient launches (sized at plan-build time)
        self.side = None          # side stream of the weight-gradient launches (see the engines' build_plan)
        self.side_events = []     # the interpreter's events (the C path's belong to each CPlan)
        self.side_stream_enabled = os.environ.get("PFR_SIDE_STREAM", "1") != "0"
        self.wt_fork = self.wt_ready = None
        self.wt_pending = False
        self._wt_table = None
        # replay the step's launch lists from C (csrc/pfr_plan.hip) instead of a Python loop: ~16 ms -> ~2 ms of host time per
        # ResNet-50 step (PFR_C_PLAN=0 keeps the interpreter loop; a launch tracer always uses it)
        self.c_plan = os.environ.get("PFR_C_PLAN", "1") != "0"
        self.grad_ready_hook = None     # callable(off): flat gradients [off, end) are final (DDP bucket hook)
        self.hook_syncs_side = False    # True: the hook makes ITS stream wait for self.side (the main stream then never waits at a mark)

    # ------------------------------------------------------------------------------------------ parameters
    def _adopt_flat(self, named):
        """the (name, parameter) list `named` into flat fp32 master / gradient buffers (the parameters become views) and their
        compute-dtype shadow"""
        dev = self.device
        offs, total = flat_offsets(named)
        self.n_flat = total
        self.master = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.shadow = self.master if self.dtype == torch.float32 else torch.zeros(total, dtype=self.dtype, device=dev)
        self.offs = offs
        self._views = {}
        self.param_list = []
        for name, p in named:
            o, n = offs[name], p.numel()
            mv = self.master[o:o + n].view(p.shape)
            mv.copy_(p.data.detach().to(dev))
            p.data = mv
            p.grad = None
            self._views[name] = (p, self.grad[o:o + n].view(p.shape))
            self.param_list.append(p)
        self.first_param = named[0][1]
        return offs

    def _adopt_batchnorms(self, model, what, kinds=(torch.nn.BatchNorm2d,)):
        """BatchNorm buffers → flat `stats` (running means, then running variances) and `nbt`, as FEEngine; running_mean /
        running_var / num_batches_tracked of the modules become views.  → id(module) -> record.  A weight that is not in the flat
        buffers (frozen; the engine has moved it to the device) is read where it stands, its gradient goes to scratch."""
        dev, offs = self.device, self.offs
        bns = [(n, m) for n, m in model.named_modules() if isinstance(m, kinds)]
        nstat = sum(m.num_features for _, m in bns)
        self.stats = torch.zeros(2 * nstat, dtype=torch.float32, device=dev)
        self.nbt = torch.zeros(len(bns), dtype=torch.int64, device=dev)
        bn_of = {}
        so = 0
        for i, (n, m) in enumerate(bns):
            if m.momentum is None or not m.affine or not m.track_running_stats:
                raise PfrError(f"{n}: the HIP {what} path needs an affine BatchNorm2d with running statistics and a momentum")
            C = m.num_features
            b = _Rec()
            b.C, b.eps, b.momentum = C, float(m.eps), float(m.momentum)
            b.rm, b.rv = self.stats[so:so + C], self.stats[nstat + so:nstat + so + C]
            b.rm.copy_(m.running_mean.detach().to(dev))
            b.rv.copy_(m.running_var.detach().to(dev))
            self.nbt[i] = int(m.num_batches_tracked.item())
            m.running_mean, m.running_var, m.num_batches_tracked = b.rm, b.rv, self.nbt[i]
            so += C
            ow, ob = offs.get(n + ".weight"), offs[n + ".bias"]
            if ow is None:
                b.gamma, b.dgamma = m.weight.data, torch.zeros(C, dtype=torch.float32, device=dev)
            else:
                b.gamma, b.dgamma = self.master[ow:ow + C], self.grad[ow:ow + C]
            b.beta, b.dbeta = self.master[ob:ob + C], self.grad[ob:ob + C]
            bn_of[id(m)] = b
        maxc = max(m.num_features for _, m in bns)
        self.bn_ws = torch.empty(max(1, lib.pfr_bn_finalize_ws_floats(1 << 20, maxc)), dtype=torch.float32, device=dev)
        return bn_of

    def _chunked(self, what, name, c):
        if c % self.kp:
            raise PfrError(f"HIP {what} path: {name} has {c} channels, not a multiple of {self.kp} in {self.dtype}")

    def _pw(self, what, prefix, m, bias=False):
        """1x1 convolution / Linear: the [O][I](x1x1) parameter is the kernel's [O][1][1][I] layout as it stands"""
        r = _Rec()
        r.out, r.inp = m.weight.shape[0], m.weight.shape[1]
        self._chunked(what, prefix, r.inp)
        self._chunked(what, prefix, r.out)
        r.off = self.offs[prefix + ".weight"]
        n = r.out * r.inp
        r.w, r.g = self.shadow[r.off:r.off + n], self.grad[r.off:r.off + n]
        r.wt = torch.zeros(n, dtype=self.dtype, device=self.device)     # [I][1][1][O]
        if bias:
            bo = self.offs[prefix + ".bias"]
            r.bias, r.dbias = self.master[bo:bo + r.out], self.grad[bo:bo + r.out]
        return r

    @staticmethod
    def _plain(m, k, stride, groups):
        return (m.kernel_size == (k, k) and m.stride == (stride, stride) and m.padding == ((k - 1) // 2,) * 2 and m.groups == groups
                and m.dilation == (1, 1) and m.bias is None)

    def _adopt_stem(self, what, sc, bn, stride=2, name="features.0.0"):
        """the 3x3 stem `name` (stride 2 unless given) and its BatchNorm record: [O][3][3][3] parameter ↔ [O][9][I padded] conv layout"""
        if not self._plain(sc, 3, stride, 1):
            raise PfrError(f"HIP {what} path: the stem is a bias-free 3x3 stride-{stride} convolution")
        st = _Rec()
        st.out, st.cin = sc.out_channels, sc.in_channels
        self._chunked(what, name, st.out)
        st.cinp = (st.cin + self.kp - 1) // self.kp * self.kp
        st.off = self.offs[name + ".weight"]
        st.g = self.grad[st.off:st.off + st.out * st.cin * 9]
        st.w = torch.zeros(st.out * 9 * st.cinp, dtype=self.dtype, device=self.device)
        st.g_conv = torch.zeros(st.out * 9 * st.cinp, dtype=torch.float32, device=self.device)
        st.bn = bn
        self.stem = st
        self.in_channels, self.cp = st.cin, st.cinp

    def matches(self, model):
        return id(model) == self.model_id and self.first_param.data.data_ptr() == self.master.data_ptr()

    def attach_grads(self):
        """Point every parameter's .grad at its slice of the flat gradient buffer."""
        for p, gv in self._views.values():
            p.grad = gv

    # ------------------------------------------------------------------------------------------ side stream, weight layouts
    def _side_ok(self, hook):
        """Side stream off: PFR_SIDE_STREAM=0; a launch tracer is active (it brackets launches with events on ONE stream); or
        gradients are being all-reduced (`hook`: the DDP bucket hook the caller decides with) while fewer than 8 hardware
        queues are available (see _side_with_ddp)."""
        return self.side_stream_enabled and _TRACER[0] is None and (hook is None or _side_with_ddp())

    def _side_stream(self, hook):
        if not self._side_ok(hook):
            return None
        if self.side is None:
            self.side = torch.cuda.Stream(device=self.device)
        return self.side

    def _refresh_dgrad_layouts(self, stream):
        """The flipped / transposed weight copies of the data-gradient launches (one record (w, wt, Cout, R, S, Cin) per layer
        from the engine's _wt_records) are first needed by the backward pass: built on the side stream, concurrent with the
        forward pass; _run_bwd waits for wt_ready."""
        side = self._side_stream(self.grad_ready_hook)
        if side is not None:
            if self.wt_fork is None:
                self.wt_fork, self.wt_ready = torch.cuda.Event(), torch.cuda.Event()
            self.wt_fork.record(torch.cuda.current_stream())
            side.wait_event(self.wt_fork)
            stream = side.cuda_stream
        # one launch for every layer (descriptor table built once: the pointers are fixed)
        tab = self._wt_table
        if tab is None:
            recs = list(self._wt_records())
            raw = b"".join(struct.pack("<QQiiii", *r) for r in recs)
            tab = self._wt_table = (torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device), len(recs))
        lib.pfr_weight_dgrad_layout_batch(tab[0].data_ptr(), tab[1], self.did, stream)
        self.wt_pending = side is not None
        if side is not None:
            self.wt_ready.record(side)

    # ------------------------------------------------------------------------------------------ plan cache
    @staticmethod
    def _plan_busy(plan):
        own = plan.meta.get("owner")
        return own is not None and own() is not None

    def _drop_idle_plans(self, oldest_only=False):
        """plans no forward pass in flight still owns (dict order = age)"""
        for k, q in list(self.plans.items()):
            if not self._plan_busy(q):
                self.plans.pop(k)
                if oldest_only:
                    break

    def _retune(self, changed):
        """engine hook of _check_tuning: re-assert the engine's own knobs after a foreign pfr_set_tuning call (`changed`);
        -> True when the plans are stale for a reason of the engine's own"""
        return False

    def _check_tuning(self):
        """A plan bakes kernel choices in (tile heights, partial-row counts, which fused form a layer takes).  When a
        pfr_set_tuning call changed a knob since the plans were built — another engine, a test, a host sweep — every plan no
        forward pass still owns is rebuilt."""
        changed = lib.pfr_tuning_epoch() != self._tuning_epoch
        if self._retune(changed) or changed:
            self._tuning_epoch = lib.pfr_tuning_epoch()
            self._drop_idle_plans()

    def _new_plan(self, *key):
        plan = self.build_plan(*key)
        self.resolve(plan)
        return plan

    def _plan_tag(self):
        """engine hook of get_plan: whatever a plan bakes in besides its key and the tuning knobs, as extra key elements"""
        return ()

    def get_plan(self, *key, slot=0):
        self._check_tuning()
        k = key + self._plan_tag() + ((slot,) if slot else ())
        p = self.plans.get(k)
        if p is None:
            if len(self.plans) >= self.max_plans:
                self._drop_idle_plans(oldest_only=True)
            p = self._new_plan(*key)
            self.plans[k] = p
        return p

    def acquire_plan(self, *key, ticket):
        """A plan owns the activation buffers its backward pass reads.  Two training forwards before a backward (list input of
        SoftmaxBasedMetricLearning — reference losses/__init__.py:39 — or any two-view step) therefore get DIFFERENT plan
        instances ("slots"); a slot is free again when its backward ran or its autograd node died.  key = build_plan's arguments."""
        slot = 0
        while True:
            plan = self.get_plan(*key, slot=slot)
            if ticket is None or not self._plan_busy(plan):
                break
            slot += 1
            if slot >= 8:
                raise PfrError("more than 8 forward passes of one shape are waiting for their backward pass")
        if ticket is not None:
            plan.meta["owner"] = weakref.ref(ticket)
        return plan

    # ------------------------------------------------------------------------------------------ symbolic -> resolved
    def _ws_key(self):
        """the split-K workspace(s) a resolved plan has baked in"""
        return self.ws.data_ptr() if self.ws is not None else 0

    def _resolve_op(self, fn, args, acc):
        raise PfrError(f"{type(self).__name__}: unknown symbolic op {fn!r}")

    def resolve(self, plan):
        """plan.ops -> meta["fwd"] and one concrete backward list per accumulate variant (bwd_lists)."""
        n = plan.meta["n_fwd"]
        plan.meta["fwd"] = plan.ops[:n]
        ws = self.ws.data_ptr() if self.ws is not None else 0
        for acc, name in enumerate(self.bwd_lists):
            res = []
            for fn, args in plan.ops[n:]:
                if fn.__class__ is not str:
                    res.append((fn, args))
                elif fn == "wgrad":
                    a = list(args)
                    a[3], a[-1] = ws, acc
                    res.append((SIDE, (lib.pfr_conv2d_wgrad, tuple(a))))
                elif fn == "acc":
                    res.append((args[0], tuple(args[1]) + (acc,)))
                else:
                    res.append(self._resolve_op(fn, args, acc))
            plan.meta[name] = res
            plan.meta.pop("c_" + name, None)
        plan.meta["ws_ptr"] = self._ws_key()

    def _fresh(self, plan):
        if plan.meta.get("ws_ptr", 0) != self._ws_key():
            self.resolve(plan)   # the shared weight-gradient workspace grew after this plan was resolved

    # ------------------------------------------------------------------------------------------ replay
    def _run_list(self, plan, key, stream, side=0, hook=None, n_events=0):
        """replays plan.meta[key] (a launch list) through the C executor when possible (compiled once per resolved list)"""
        if self.c_plan and _TRACER[0] is None:
            m = plan.meta
            ck = "c_" + key
            cp = m.get(ck, False)
            if cp is False:
                cp = m[ck] = CPlan.compile(m[key], n_events)
            if cp is not None:
                cp.run(stream, side, hook, self.hook_syncs_side)
                return True
        return False

    def _run_fwd(self, plan, stream):
        if not self._run_list(plan, "fwd", stream):
            for fn, args in plan.meta["fwd"]:
                fn(*args, stream)

    def _begin_backward(self, plan, demb):
        """the incoming gradient into the plan's buffer (compute dtype); the plan is released to the next forward pass"""
        demb = demb.contiguous()
        if demb.numel() != plan.meta["demb"].numel():
            raise PfrError(f"backward: gradient of {tuple(demb.shape)} does not match the plan's embedding buffer "
                           f"{tuple(plan.meta['demb'].shape)}")
        self._fresh(plan)
        lib.pfr_cast(demb.data_ptr(), dtype_id(demb.dtype), plan.meta["demb"].data_ptr(), self.did, demb.numel(),
                     torch.cuda.current_stream().cuda_stream)
        plan.meta["owner"] = None

    def _run_bwd(self, plan, key, hook, side_hook):
        """replays the backward list plan.meta[key]; `hook`: the grad-ready hook in effect for this pass, `side_hook`: the one
        the side-stream decision is made with (_side_ok)"""
        main = torch.cuda.current_stream()
        if self.wt_pending:
            main.wait_event(self.wt_ready)
            self.wt_pending = False
        side = self._side_stream(side_hook)
        n_events = 2 * plan.meta.get("n_side", 0)
        if self._run_list(plan, key, main.cuda_stream, 0 if side is None else side.cuda_stream, hook, n_events):
            return
        ev = self.side_events
        if side is not None:
            while len(ev) < n_events:
                ev.append(torch.cuda.Event())
        run_ops(plan.meta[key], main, side, ev, hook, self.hook_syncs_side)

    # ------------------------------------------------------------------------------------------ forward / backward
    def _forward_plan(self, x, *key, with_backward, ticket, fill=None):
        """the tail of forward(): the plan of `key` (build_plan's arguments), fresh weights, the NCHW fp32 input `x` into the plan's
        NHWC buffer, the forward list; `fill(plan)` sets further plan inputs first (a stochastic-depth draw)"""
        plan = self.acquire_plan(*key, ticket=ticket if with_backward else None)
        if with_backward:
            self._fresh(plan)
        stream = torch.cuda.current_stream().cuda_stream
        self.refresh_weights(stream, for_backward=with_backward)
        if fill is not None:
            fill(plan)
        N, C, H, W = x.shape
        lib.pfr_nchw_to_nhwc(x.data_ptr(), plan.meta["x_nhwc"].data_ptr(), self.did, N, C, H, W, self.cp, stream)
        self._run_fwd(plan, stream)
        self._last_plan = plan
        return plan.meta["emb"]

    def backward(self, demb, plan=None):
        plan = plan if plan is not None else self._last_plan
        self._begin_backward(plan, demb)
        # Every gradient kernel of these engines OVERWRITES its slice of the flat buffer.  When gradients are already present
        # (a second backward before zero_grad: gradient accumulation, list inputs) the previous sum is set aside and added
        # back afterwards — two extra passes over the flat buffer, only on that path.
        prev = self.grad.clone() if self.first_param.grad is not None else None
        hook = self.grad_ready_hook
        if prev is not None or any(self._plan_busy(q) for q in self.plans.values()):
            hook = None   # not final yet (accumulating, or another forward pass still waits for its backward)
        # (the side-stream decision follows the hook IN EFFECT: no bucket is reduced during this pass when it is None)
        self._run_bwd(plan, "bwd", hook, hook)
        if prev is not None:
            self.grad.add_(prev)
        self.attach_grads()


class _EngineFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, model, fwd_args, *params):
        eng = model.hip_engine(x.device)
        ctx.ticket = PlanTicket()
        emb = eng.forward(x, *fwd_args, True, ctx.ticket)  # only reached when a backward pass can follow (see engine_forward)
        ctx.eng = eng
        ctx.plan = eng._last_plan
        ctx.nparams = len(params)
        return emb.clone()

    @staticmethod
    def backward(ctx, demb):
        own = ctx.plan.meta.get("owner")
        if own is None or own() is not ctx.ticket:
            raise PfrError("backward: the activations of this forward pass were released (double backward?)")
        ctx.eng.backward(demb, ctx.plan)
        # parameter gradients are delivered by side effect into the flat gradient buffer (p.grad views)
        return (None, None, None) + (None,) * ctx.nparams


def engine_forward(model, x, *fwd_args):
    """model.hip_engine().forward(x, *fwd_args, with_backward[, ticket]) under autograd"""
    eng = model.hip_engine(x.device)
    if torch.is_grad_enabled() and any(p.requires_grad for p in eng.param_list):
        return _EngineFunction.apply(x, model, fwd_args, *eng.param_list)
    return eng.forward(x, *fwd_args, False).clone()
