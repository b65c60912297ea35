"""SwinEngine — executes the Swin-T/S/B/L feature extractor (forward, backward) on the gfx950 kernels.

Counterpart of /root/reference/models/swin.py:196-225 (`SwinTransformer.forward`) + autograd for BASELINE config 4.
Same design as models/_fe_engine.FEEngine: flat fp32 master / gradient buffers (the module's nn.Parameters become views,
state-dict names unchanged), compute-dtype shadow, one pre-built plan of C-ABI calls per input shape; the plan runtime (plan
cache, resolve, replay on two streams, autograd wrapper) is models/_plan_engine.PlanEngine.

Mapping (tokens are kept NHWC = [B, H, W, C] end to end; the reference's NCHW↔NHWC permutes between stages vanish):
  PatchMerging (Unfold + Linear, swin.py:155-167)  → stride-f conv on NHWC (weights re-laid out per step)
  LayerNorm / GELU / windowed attention            → csrc/pfr_swin.hip
  to_qkv / to_out / MLP / head Linear              → pfr_conv2d_fwd (GEMM, bias and residual-add fused in the epilogue),
                                                     pfr_conv2d_wgrad, data gradient through pfr_conv2d_fwd
  cyclic shift, window partition, masks            → addressing / analytic mask inside the attention kernel
"""
import struct

import torch

from .._hip import lib, dtype_id, PfrError
from .._hip.cplan import SIDE, FORK, SREC, WAIT, MWAIT
from ._plan_engine import PlanEngine, Plan, engine_forward, flat_offsets


class _Lin:
    pass


class _LN:
    pass


class SwinEngine(PlanEngine):
    max_plans = 6

    def __init__(self, model, device, compute_dtype=None):
        super().__init__(model, device, compute_dtype)
        self.fuse_gelu = True
        # buffers per (shape, dtype) class of the backward pool before one that a side-stream op still reads is re-used (HBM is
        # plentiful; a shallow pool makes the main stream wait for the side stream at almost every layer)
        self.pool_depth = 48
        self.ln_dxsum = True   # bias gradients from the LayerNorm-backward pass that produced their input
        self._adopt(model)

    # ------------------------------------------------------------------------------------------ parameters
    def _adopt(self, model):
        dev = self.device
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
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
        for n, p in model.named_parameters():          # frozen masks just move to the device
            if not p.requires_grad:
                p.data = p.data.to(dev)
        self.first_param = named[0][1]

        def lin(prefix, m, conv_f=None, cin=None):
            r = _Lin()
            r.out, r.inp = m.out_features, m.in_features
            r.off = offs[prefix + ".weight"]
            r.g = self.grad[r.off:r.off + r.out * r.inp]
            if m.bias is not None:
                bo = offs[prefix + ".bias"]
                r.bias = self.master[bo:bo + r.out]
                r.dbias = self.grad[bo:bo + r.out]
            else:
                r.bias = r.dbias = None
            r.f = conv_f
            if conv_f is None:
                r.w = self.shadow[r.off:r.off + r.out * r.inp]                       # [out][in] = [out,1,1,in]
                r.wt = torch.zeros(r.inp * r.out, dtype=self.dtype, device=dev)     # [in,1,1,out]
                r.cin = r.cinp = r.inp
            else:                                                                    # patch merging as a conv
                r.cin = cin
                r.cinp = (cin + self.kp - 1) // self.kp * self.kp
                kk = conv_f * conv_f * r.cinp
                r.w = torch.zeros(r.out * kk, dtype=self.dtype, device=dev)          # [out][f][f][cinp]
                r.wt = torch.zeros(r.out * kk, dtype=self.dtype, device=dev)         # [cinp][f][f][out]
                r.g_conv = torch.zeros(r.out * kk, dtype=torch.float32, device=dev)
            return r

        def ln(prefix, m):
            r = _LN()
            r.C, r.eps = m.normalized_shape[0], m.eps
            wo, bo = offs[prefix + ".weight"], offs[prefix + ".bias"]
            r.gamma, r.beta = self.master[wo:wo + r.C], self.master[bo:bo + r.C]
            r.dgamma, r.dbeta = self.grad[wo:wo + r.C], self.grad[bo:bo + r.C]
            return r

        self.stages = []
        cin = model.stage1.patch_partition.linear.in_features // (model.stage1.patch_partition.downscaling_factor ** 2)
        self.in_channels = cin
        for si in range(1, 5):
            st = getattr(model, f"stage{si}")
            pm = st.patch_partition
            rec = {"pm": lin(f"stage{si}.patch_partition.linear", pm.linear, conv_f=pm.downscaling_factor, cin=cin),
                   "f": pm.downscaling_factor, "blocks": [], "off": offs[f"stage{si}.patch_partition.linear.weight"]}
            for li, pair in enumerate(st.layers):
                for bi, blk in enumerate(pair):
                    pre = f"stage{si}.layers.{li}.{bi}"
                    att = blk.attention_block.fn.fn
                    ff = blk.mlp_block.fn.fn
                    if not att.relative_pos_embedding:
                        raise PfrError("HIP Swin path supports relative_pos_embedding=True (the reference default)")
                    b = {"ln1": ln(pre + ".attention_block.fn.norm", blk.attention_block.fn.norm),
                         "qkv": lin(pre + ".attention_block.fn.fn.to_qkv", att.to_qkv),
                         "out": lin(pre + ".attention_block.fn.fn.to_out", att.to_out),
                         "ln2": ln(pre + ".mlp_block.fn.norm", blk.mlp_block.fn.norm),
                         "fc1": lin(pre + ".mlp_block.fn.fn.net.0", ff.net[0]),
                         "fc2": lin(pre + ".mlp_block.fn.fn.net.2", ff.net[2]),
                         "heads": att.heads, "w": att.window_size, "scale": att.scale,
                         "shift": att.window_size // 2 if att.shifted else 0}
                    po = offs[pre + ".attention_block.fn.fn.pos_embedding"]
                    ntab = (2 * att.window_size - 1) ** 2
                    b["pos"] = self.master[po:po + ntab]
                    b["dpos"] = self.grad[po:po + ntab]
                    b["hd"] = att.to_qkv.out_features // (3 * att.heads)
                    b["tab"] = torch.empty(lib.pfr_window_bias_table_floats(att.window_size), dtype=torch.float32, device=dev)
                    rec["blocks"].append(b)
            self.stages.append(rec)
            cin = pm.linear.out_features
        self.head_ln = ln("mlp_head.0", model.mlp_head[0])
        self.head_fc = lin("mlp_head.1", model.mlp_head[1])
        self.emb_dim = self.head_fc.out
        self.cp = self.stages[0]["pm"].cinp
        torch.cuda.synchronize(dev)

    def _all_lins(self):
        for st in self.stages:
            yield st["pm"]
            for b in st["blocks"]:
                for k in ("qkv", "out", "fc1", "fc2"):
                    yield b[k]
        yield self.head_fc

    def refresh_weights(self, stream, for_backward=True):
        if self.dtype != torch.float32:
            lib.pfr_cast(self.master.data_ptr(), 0, self.shadow.data_ptr(), self.did, self.n_flat, stream)
        for r in self._all_lins():
            if r.f is not None:   # Unfold order (c, kh, kw) → conv layout [out][kh][kw][c(padded)]
                lib.pfr_nchw_to_nhwc(self.master.data_ptr() + 4 * r.off, r.w.data_ptr(), self.did, r.out, r.cin, r.f * r.f, 1,
                                     r.cinp, stream)
        if for_backward:
            self._refresh_dgrad_layouts(stream)

    def _wt_records(self):
        for r in self._all_lins():
            if r.f is None:
                yield (r.w.data_ptr(), r.wt.data_ptr(), r.out, 1, 1, r.inp)
            elif r is not self.stages[0]["pm"]:      # (the first patch merging has no data gradient)
                yield (r.w.data_ptr(), r.wt.data_ptr(), r.out, r.f, r.f, r.cinp)

    # ------------------------------------------------------------------------------------------ plan
    def build_plan(self, N, H, W, with_backward):
        T, dev, did = self.dtype, self.device, self.did
        plan = Plan()
        fwd, bwd = [], []
        tab_recs = []

        def A(shape, dtype=None):
            return plan.keep(torch.empty(shape, dtype=dtype or T, device=dev))

        def gemm(ops, x, rows, cin, r, y, bias=True, residual=None, w=None):
            ops.append((lib.pfr_conv2d_fwd, (x.data_ptr(), (w if w is not None else r.w).data_ptr(), y.data_ptr(), did,
                                             dtype_id(y.dtype), rows, 1, 1, cin, r.out, 1, 1, 1, 0, 0, 1, 1, r.out,
                                             r.bias.data_ptr() if (bias and r.bias is not None) else 0,
                                             0 if residual is None else residual.data_ptr(), 0, 0, 0, 0, 0, 0)))

        ws_need = [0]

        def wgrad(ops, x, xshape, dy, dyshape, r, R, stride, out):
            Nq, Hq, Wq, Cq = xshape
            _, OH, OW, Co = dyshape
            KK = R * R * Cq
            splits = lib.pfr_conv2d_wgrad_splits(Nq * OH * OW, Co, KK)
            ws_need[0] = max(ws_need[0], splits * Co * KK)
            side(ops, ("wgrad", (x.data_ptr(), dy.data_ptr(), out.data_ptr(), None, did, Nq, Hq, Wq, Cq, Co, R, R, stride, 0,
                                OH, OW, Co, 0, 0, 0, 1.0, 0)), dy)

        def dgrad_lin(ops, dy, rows, r, dx):
            ops.append((lib.pfr_conv2d_fwd, (dy.data_ptr(), r.wt.data_ptr(), dx.data_ptr(), did, did, rows, 1, 1, r.out, r.inp, 1,
                                             1, 1, 0, 0, 1, 1, r.inp, 0, 0, 0, 0, 0, 0, 0, 0)))

        pend_cs = []   # column sums whose final merge is deferred to the next flush: (partials, out, partial rows, C, tile height | 0, rows)

        def colsum(ops, x, rows, C, out, dt=None):
            """bias / LayerNorm-parameter / position-table gradient = column sum of x; the partial sums run now (side stream), the
            ~100 tiny final merges of a step are batched into one launch per DDP bucket boundary (flush_colsums)"""
            d = dt if dt is not None else did
            n = lib.pfr_colsum_parts(d, rows, C)
            if n <= 0:   # a few hundred rows: one small kernel does it all
                side(ops, (SIDE, (lib.pfr_colsum, (x.data_ptr(), d, rows, C, out.data_ptr(), 0, 0))), x)
                return
            ws = A((lib.pfr_colsum_ws_floats(rows, C),), torch.float32)   # its own workspace: alive until the batched final
            side(ops, (SIDE, (lib.pfr_colsum_partial, (x.data_ptr(), d, rows, C, ws.data_ptr()))), x)
            pend_cs.append((ws, out, n, C, 0, 0))

        def flush_colsums(ops):
            if not pend_cs:
                return
            raw = b"".join(struct.pack("<QQiiiiii", ws.data_ptr(), out.data_ptr(), n, C, 0, mt, rws, 0) for ws, out, n, C, mt, rws in pend_cs)
            tab = plan.keep(torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev))
            side(ops, (SIDE, (lib.pfr_colsum_final_batch, (tab.data_ptr(), len(pend_cs), max(e[3] for e in pend_cs)))))
            del pend_cs[:]

        x_nhwc = A((N, H, W, self.cp))
        cur, cshape = x_nhwc, (N, H, W, self.cp)
        saved = []
        for st in self.stages:
            f, pm = st["f"], st["pm"]
            Nn, Hh, Ww, Cc = cshape
            OH, OW = Hh // f, Ww // f
            rows = N * OH * OW
            C = pm.out
            t = A((N, OH, OW, C))
            fwd.append((lib.pfr_conv2d_fwd, (cur.data_ptr(), pm.w.data_ptr(), t.data_ptr(), did, did, N, Hh, Ww, Cc, C, f, f, f, 0,
                                             0, OH, OW, C, pm.bias.data_ptr() if pm.bias is not None else 0, 0, 0, 0, 0, 0, 0, 0)))
            srec = {"in": cur, "inshape": cshape, "t": t, "shape": (N, OH, OW, C), "blocks": []}
            x = t
            for b in st["blocks"]:
                ln1 = A((rows, C)); mu1 = A((rows,), torch.float32); rs1 = A((rows,), torch.float32)
                fwd.append((lib.pfr_layernorm_fwd, (x.data_ptr(), b["ln1"].gamma.data_ptr(), b["ln1"].beta.data_ptr(), ln1.data_ptr(),
                                                    mu1.data_ptr(), rs1.data_ptr(), did, rows, C, float(b["ln1"].eps))))
                qkv = A((rows, 3 * C))
                gemm(fwd, ln1, rows, C, b["qkv"], qkv)
                att = A((rows, C))
                tab_recs.append((b["pos"].data_ptr(), b["tab"].data_ptr(), b["w"], b["shift"]))
                fwd.append((lib.pfr_window_attn_fwd, (qkv.data_ptr(), b["tab"].data_ptr(), att.data_ptr(), did, N, OH, OW,
                                                      b["heads"], b["hd"], b["w"], b["shift"], float(b["scale"]))))
                y = A((rows, C))
                gemm(fwd, att, rows, C, b["out"], y, residual=x)
                ln2 = A((rows, C)); mu2 = A((rows,), torch.float32); rs2 = A((rows,), torch.float32)
                fwd.append((lib.pfr_layernorm_fwd, (y.data_ptr(), b["ln2"].gamma.data_ptr(), b["ln2"].beta.data_ptr(), ln2.data_ptr(),
                                                    mu2.data_ptr(), rs2.data_ptr(), did, rows, C, float(b["ln2"].eps))))
                h1 = A((rows, 4 * C))
                h2 = A((rows, 4 * C))
                if self.fuse_gelu:   # GELU in the fc1 GEMM's epilogue (writes the pre-activation h1 and h2 = gelu(h1))
                    fwd.append((lib.pfr_gemm_act, (ln2.data_ptr(), b["fc1"].w.data_ptr(), h2.data_ptr(), did, rows, C, 4 * C,
                                                   b["fc1"].bias.data_ptr(), 2, h1.data_ptr())))
                else:
                    gemm(fwd, ln2, rows, C, b["fc1"], h1)
                    fwd.append((lib.pfr_gelu_fwd, (h1.data_ptr(), h2.data_ptr(), did, rows * 4 * C)))
                z = A((rows, C))
                gemm(fwd, h2, rows, 4 * C, b["fc2"], z, residual=y)
                srec["blocks"].append(dict(x=x, ln1=ln1, mu1=mu1, rs1=rs1, qkv=qkv, att=att, y=y, ln2=ln2, mu2=mu2, rs2=rs2,
                                           h1=h1, h2=h2, z=z))
                x = z
            saved.append(srec)
            cur, cshape = x, (N, OH, OW, C)
        Nn, Hh, Ww, Cf = cshape
        pooled = A((N, Cf))
        fwd.append((lib.pfr_avgpool_fwd, (cur.data_ptr(), pooled.data_ptr(), did, N, Hh * Ww, Cf)))
        hln = A((N, Cf)); hmu = A((N,), torch.float32); hrs = A((N,), torch.float32)
        fwd.append((lib.pfr_layernorm_fwd, (pooled.data_ptr(), self.head_ln.gamma.data_ptr(), self.head_ln.beta.data_ptr(),
                                            hln.data_ptr(), hmu.data_ptr(), hrs.data_ptr(), did, N, Cf, float(self.head_ln.eps))))
        emb = A((N, self.emb_dim), torch.float32)
        gemm(fwd, hln, N, Cf, self.head_fc, emb)
        # the bias(+mask) tables of every attention block in one launch at the head of the forward pass (their inputs, the relative-position
        # tables, only change in the optimiser step)
        tabd = plan.keep(torch.frombuffer(bytearray(b"".join(struct.pack("<QQii", *r) for r in tab_recs)), dtype=torch.uint8).to(dev))
        fwd.insert(0, (lib.pfr_window_bias_table_batch, (tabd.data_ptr(), len(tab_recs))))
        plan.ops = fwd
        plan.meta.update(x_nhwc=x_nhwc, emb=emb, n_fwd=len(fwd))
        if not with_backward:
            return plan

        # ================================================================= backward
        # Weight gradients, bias / LayerNorm-parameter / position-table column sums feed nothing before the optimizer: they run on
        # a SIDE stream (≈ 150 short launches per step that would otherwise sit in the dependency chain).  Stream roles
        # (_hip/cplan.py): (FORK, k) side waits for main's current point; (SREC, k) side records "op k done"; (WAIT, k) main waits
        # for op k — emitted before a pooled buffer that op k read is handed out again, before grad-ready marks and at the end.
        # Only the weight gradients stay symbolic ("wgrad": PlanEngine.resolve fills the split-K workspace pointer in).
        pool = {}
        nalloc = {}
        pending = {}      # data_ptr of a pooled buffer -> last side op that reads it
        side_reads = []   # (k, data_ptr) of every side-op input
        nside = [0]

        def G(shape, dtype=None):
            key = (tuple(shape), dtype or T)
            lst = pool.setdefault(key, [])
            for i, t in enumerate(lst):              # a buffer no side op is reading
                if t.data_ptr() not in pending:
                    return lst.pop(i)
            if not lst or nalloc.get(key, 0) < self.pool_depth:    # rotation so that the side stream may lag behind without stalling main
                nalloc[key] = nalloc.get(key, 0) + 1
                return A(shape, dtype)
            t = lst.pop(0)
            bwd.append((WAIT, pending.pop(t.data_ptr())))
            return t

        def release(t):
            lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()
            ks = [k for k, ptr in side_reads if lo <= ptr < hi]
            if ks:
                pending[t.data_ptr()] = max(ks)
            side_reads[:] = [(k, ptr) for k, ptr in side_reads if not (lo <= ptr < hi)]
            pool.setdefault((tuple(t.shape), t.dtype), []).append(t)

        def side(ops, op, *reads):
            if ops and ops[-1][0] == SREC:
                # no main-stream launch since the previous side op: it joins that op's fork (every fork is an event recorded on the
                # main stream, i.e. a marker packet in front of the next kernel of the dependency chain)
                k = ops.pop()[1]
            else:
                k = nside[0]
                nside[0] += 1
                ops.append((FORK, k))
            ops.append(op)
            ops.append((SREC, k))
            for r in reads:
                side_reads.append((k, r.data_ptr()))

        def ln_bwd(ops, dy, xin, mu, rs, lnrec, dres, dx, rows, C, want_sum=False):
            """→ (partials, rows of partials) of the column sums of dx when want_sum and the kernel can emit them, else None"""
            nb = lib.pfr_layernorm_bwd_blocks(rows)
            # the kernel's per-workgroup partials ARE the partial sets of the deferred final merge (own buffer per LayerNorm: they
            # must survive until the batched merge at the next bucket boundary)
            part = A((2, nb, C), torch.float32)
            dsum = A((nb, C), torch.float32) if (want_sum and self.ln_dxsum and lib.pfr_layernorm_bwd_dxsum_ok(did, C)) else None
            ops.append((lib.pfr_layernorm_bwd_dxsum, (dy.data_ptr(), xin.data_ptr(), mu.data_ptr(), rs.data_ptr(), lnrec.gamma.data_ptr(),
                                                      0 if dres is None else dres.data_ptr(), dx.data_ptr(), part.data_ptr(),
                                                      0 if dsum is None else dsum.data_ptr(), did, rows, C)))
            pend_cs.append((part[0], lnrec.dgamma, nb, C, 0, 0))
            pend_cs.append((part[1], lnrec.dbeta, nb, C, 0, 0))
            return None if dsum is None else (dsum, nb)

        def bias_grad(ops, g, rows, C, dbias, gsum):
            """bias gradient = column sum of g: from the LayerNorm-backward pass that produced g when it left the sums (gsum), else
            a column-sum pass of its own on the side stream"""
            if gsum is not None:
                pend_cs.append((gsum[0], dbias, gsum[1], C, 0, 0))
            else:
                colsum(ops, g, rows, C, dbias)

        demb = A((N, self.emb_dim))
        plan.meta["demb"] = demb
        hf = self.head_fc
        if hf.dbias is not None:
            colsum(bwd, demb, N, hf.out, hf.dbias)
        wgrad(bwd, hln, (N, 1, 1, Cf), demb, (N, 1, 1, hf.out), hf, 1, 1, hf.g)
        dhln = G((N, Cf))
        dgrad_lin(bwd, demb, N, hf, dhln)
        dpooled = G((N, Cf))
        ln_bwd(bwd, dhln, pooled, hmu, hrs, self.head_ln, None, dpooled, N, Cf)
        dz_sum = None   # column sums of dz left by the pass that produced it (None: avgpool / patch-merging data gradient)
        release(dhln)
        dz = G(cshape)
        bwd.append((lib.pfr_avgpool_bwd, (dpooled.data_ptr(), dz.data_ptr(), did, N, Hh * Ww, Cf)))
        release(dpooled)
        bwd.append((None, (self.offs["mlp_head.0.weight"],)))
        for si in range(len(self.stages) - 1, -1, -1):
            st, srec = self.stages[si], saved[si]
            Nn, OH, OW, C = srec["shape"]
            rows = N * OH * OW
            for b, sv in zip(reversed(st["blocks"]), reversed(srec["blocks"])):
                # ---- MLP branch: z = fc2(gelu(fc1(ln2(y)))) + y
                bias_grad(bwd, dz.view(rows, C), rows, C, b["fc2"].dbias, dz_sum)
                wgrad(bwd, sv["h2"], (rows, 1, 1, 4 * C), dz, (rows, 1, 1, C), b["fc2"], 1, 1, b["fc2"].g)
                dh2 = G((rows, 4 * C))
                if self.fuse_gelu:   # dh1 = (dz·W2) ∘ gelu'(h1) in the data-gradient GEMM's epilogue
                    # ... which also leaves the per-m-tile column means of dh1: fc1's bias gradient = sum_t rows_t * mean_t, merged
                    # with the other deferred column sums -- no second pass over the widest gradient tensor of the block
                    nsum = lib.pfr_gemm_act_colsum_parts(rows, C, 4 * C, did)
                    if nsum > 0:     # streaming Linear kernel (csrc/pfr_slin.hip): plain column sums per row range
                        stp = A((nsum, 4 * C), torch.float32)
                        bwd.append((lib.pfr_gemm_act_colsums, (dz.data_ptr(), b["fc2"].wt.data_ptr(), dh2.data_ptr(), did, rows, C, 4 * C,
                                                               sv["h1"].data_ptr(), stp.data_ptr())))
                        pend_cs.append((stp, b["fc1"].dbias, nsum, 4 * C, 0, 0))
                    else:
                        mt = lib.pfr_gemm_act_mtile(rows, C, 4 * C, did)
                        nt = (rows + mt - 1) // mt
                        stp = A((nt, 2, 4 * C), torch.float32)
                        bwd.append((lib.pfr_gemm_act_colstats, (dz.data_ptr(), b["fc2"].wt.data_ptr(), dh2.data_ptr(), did, rows, C, 4 * C, 0,
                                                                3, sv["h1"].data_ptr(), stp.data_ptr())))
                        pend_cs.append((stp, b["fc1"].dbias, nt, 4 * C, mt, rows))
                else:
                    dgrad_lin(bwd, dz, rows, b["fc2"], dh2)
                    bwd.append((lib.pfr_gelu_bwd, (sv["h1"].data_ptr(), dh2.data_ptr(), dh2.data_ptr(), did, rows * 4 * C)))
                    colsum(bwd, dh2, rows, 4 * C, b["fc1"].dbias)
                wgrad(bwd, sv["ln2"], (rows, 1, 1, C), dh2, (rows, 1, 1, 4 * C), b["fc1"], 1, 1, b["fc1"].g)
                dln2 = G((rows, C))
                dgrad_lin(bwd, dh2, rows, b["fc1"], dln2)
                release(dh2)
                dy = G((rows, C))
                dy_sum = ln_bwd(bwd, dln2, sv["y"], sv["mu2"], sv["rs2"], b["ln2"], dz, dy, rows, C, want_sum=True)
                release(dln2)
                release(dz)
                # ---- attention branch: y = to_out(attn(to_qkv(ln1(x)))) + x
                bias_grad(bwd, dy, rows, C, b["out"].dbias, dy_sum)
                wgrad(bwd, sv["att"], (rows, 1, 1, C), dy, (rows, 1, 1, C), b["out"], 1, 1, b["out"].g)
                datt = G((rows, C))
                dgrad_lin(bwd, dy, rows, b["out"], datt)
                dqkv = G((rows, 3 * C))
                nblk = N * (OH // b["w"]) * (OW // b["w"]) * b["heads"]
                ntab = (2 * b["w"] - 1) ** 2
                dpart = G((nblk, ntab), torch.float32)
                bwd.append((lib.pfr_window_attn_bwd, (sv["qkv"].data_ptr(), b["tab"].data_ptr(), datt.data_ptr(), dqkv.data_ptr(),
                                                      dpart.data_ptr(), did, N, OH, OW, b["heads"], b["hd"], b["w"], b["shift"],
                                                      float(b["scale"]))))
                colsum(bwd, dpart, nblk, ntab, b["dpos"], 0)
                release(dpart)
                release(datt)
                wgrad(bwd, sv["ln1"], (rows, 1, 1, C), dqkv, (rows, 1, 1, 3 * C), b["qkv"], 1, 1, b["qkv"].g)
                dln1 = G((rows, C))
                dgrad_lin(bwd, dqkv, rows, b["qkv"], dln1)
                release(dqkv)
                dx = G((rows, C))
                dz_sum = ln_bwd(bwd, dln1, sv["x"], sv["mu1"], sv["rs1"], b["ln1"], dy, dx, rows, C, want_sum=True)
                release(dln1)
                release(dy)
                dz = dx
            # ---- patch merging (stride-f conv): bias, weight gradient (conv layout → Unfold layout), data gradient
            pm, f = st["pm"], st["f"]
            Ni, Hi, Wi, Ci = srec["inshape"]
            if pm.dbias is not None:
                bias_grad(bwd, dz, rows, C, pm.dbias, dz_sum)
            g_conv = pm.g_conv
            wgrad(bwd, srec["in"], (Ni, Hi, Wi, Ci), dz, (N, OH, OW, C), pm, f, f, g_conv)
            side(bwd, (SIDE, (lib.pfr_nhwc_to_nchw_f32, (g_conv.data_ptr(), pm.g.data_ptr(), pm.out, pm.cin, f * f, pm.cinp, 0))))
            if si > 0:
                din = G((Ni, Hi, Wi, Ci))
                bwd.append((lib.pfr_conv2d_fwd, (dz.data_ptr(), pm.wt.data_ptr(), din.data_ptr(), did, did, N, OH, OW, C, Ci, f, f, 1,
                                                 f - 1, {2: 1, 4: 2}[f], Hi, Wi, Ci, 0, 0, 0, 0, 0, 0, 0, 0)))
                release(dz)
                dz = din
            dz_sum = None
            flush_colsums(bwd)
            if nside[0]:   # everything the side stream was given so far is final (end of backward, or a DDP bucket boundary)
                bwd.append((WAIT if si == 0 else MWAIT, nside[0] - 1))
            bwd.append((None, (st["off"],)))
        plan.meta["n_side"] = nside[0]
        if self.ws is None or self.ws.numel() < ws_need[0]:
            self.ws = torch.empty(ws_need[0], dtype=torch.float32, device=dev)
        plan.ops = fwd + bwd
        return plan

    def forward(self, x, with_backward, ticket=None):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise PfrError(f"expected NCHW input with {self.in_channels} channels, got {tuple(x.shape)}")
        x = x.float().contiguous()
        N, _, H, W = x.shape
        plan = self.acquire_plan(N, H, W, with_backward, ticket=ticket if with_backward else None)
        if with_backward:
            self._fresh(plan)
        stream = torch.cuda.current_stream().cuda_stream
        self.refresh_weights(stream, for_backward=with_backward)
        lib.pfr_nchw_to_nhwc(x.data_ptr(), plan.meta["x_nhwc"].data_ptr(), self.did, N, x.shape[1], H, W, self.cp, stream)
        self._run_fwd(plan, stream)
        self._last_plan = plan
        return plan.meta["emb"]

    def backward(self, demb, plan=None):
        plan = plan if plan is not None else self._last_plan
        self._begin_backward(plan, demb)
        # Every gradient kernel of this engine OVERWRITES its slice of the flat buffer.  When gradients are already present
        # (a second backward before zero_grad: gradient accumulation, list inputs) the previous sum is set aside and added
        # back afterwards — two extra passes over the 110 MB buffer, only on that path.
        prev = self.grad.clone() if self.first_param.grad is not None else None
        hook = self.grad_ready_hook
        if prev is not None or any(self._plan_busy(q) for q in self.plans.values()):
            hook = None   # not final yet (accumulating, or another forward pass still waits for its backward)
        # (the side-stream decision follows the hook IN EFFECT: no bucket is reduced during this pass when it is None)
        self._run_bwd(plan, "bwd", hook, hook)
        if prev is not None:
            self.grad.add_(prev)
        self.attach_grads()


swin_forward = engine_forward
