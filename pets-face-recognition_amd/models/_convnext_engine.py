"""ConvNeXtEngine — executes the ConvNeXt-T/S feature extractor (forward, backward) on the gfx950 kernels.

Same design as models/_swin_engine.SwinEngine: flat fp32 master / gradient buffers (the module's nn.Parameters become views,
torchvision's state-dict names unchanged), compute-dtype shadow, activations NHWC end to end, one pre-built plan of C-ABI calls per
input shape; the plan runtime is models/_plan_engine.PlanEngine.

Mapping (models/convnext.py):
  4x4 stride-4 stem, 2x2 stride-2 downsample convs → pfr_conv2d_fwd on NHWC (weights re-laid out per step), pfr_conv2d_wgrad
  LayerNorm2d / LayerNorm                          → pfr_layernorm_fwd / pfr_layernorm_bwd_dxsum on the [N*H*W, C] rows
  depthwise 7x7 conv                               → pfr_dwconv2d_fwd (flip = 1: data gradient), pfr_dwconv2d_wgrad (csrc/pfr_dwconv.hip)
  Linear C→4C + GELU, Linear 4C→C                  → pfr_gemm_act / pfr_conv2d_fwd, as the Swin MLP
  layer scale · stochastic depth + residual        → pfr_layer_scale_fwd / pfr_layer_scale_bwd
  avgpool → LayerNorm2d → Linear                   → pfr_avgpool_fwd, pfr_layernorm_fwd, pfr_conv2d_fwd
"""
import struct

import torch
import torch.nn as nn

from .._hip import lib, dtype_id, PfrError
from .._hip.cplan import SIDE, FORK, SREC, WAIT, MWAIT
from ._plan_engine import PlanEngine, Plan, engine_forward, flat_offsets


class _Rec:
    pass


class ConvNeXtEngine(PlanEngine):
    max_plans = 6

    def __init__(self, model, device, compute_dtype=None):
        super().__init__(model, device, compute_dtype)
        self.pool_depth = 48   # see SwinEngine: backward buffers per class before one a side-stream op still reads is re-used
        self._adopt(model)

    # ------------------------------------------------------------------------------------------ parameters
    def _adopt(self, model):
        from .convnext import CNBlock
        dev = self.device
        if not isinstance(model.classifier[2], nn.Linear):
            raise PfrError("HIP ConvNeXt path needs a Linear embedding layer at classifier[2] (num_classes > 0)")
        named = list(model.named_parameters())
        if not all(p.requires_grad for _, p in named):
            raise PfrError("HIP ConvNeXt path trains every parameter (no frozen layers)")
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

        def vec(name, n):
            o = offs[name]
            return self.master[o:o + n], self.grad[o:o + n]

        def lin(prefix, m):
            r = _Rec()
            r.out, r.inp, r.f = m.out_features, m.in_features, None
            r.off = offs[prefix + ".weight"]
            r.g = self.grad[r.off:r.off + r.out * r.inp]
            r.bias, r.dbias = vec(prefix + ".bias", r.out)
            r.w = self.shadow[r.off:r.off + r.out * r.inp]                       # [out][in] = [out,1,1,in]
            r.wt = torch.zeros(r.inp * r.out, dtype=self.dtype, device=dev)     # [in,1,1,out]
            return r

        def conv(prefix, m):
            """a kernel = stride conv (stem, downsample): [O][I][f][f] parameter ↔ [O][f][f][I padded] conv layout"""
            r = _Rec()
            r.out, r.cin, r.f = m.out_channels, m.in_channels, m.kernel_size[0]
            r.cinp = (r.cin + self.kp - 1) // self.kp * self.kp
            r.off = offs[prefix + ".weight"]
            kk = r.f * r.f * r.cinp
            r.g = self.grad[r.off:r.off + r.out * r.cin * r.f * r.f]
            r.bias, r.dbias = vec(prefix + ".bias", r.out)
            r.w = torch.zeros(r.out * kk, dtype=self.dtype, device=dev)
            r.wt = torch.zeros(r.out * kk, dtype=self.dtype, device=dev)
            r.g_conv = torch.zeros(r.out * kk, dtype=torch.float32, device=dev)
            return r

        def ln(prefix, m):
            r = _Rec()
            r.C, r.eps = m.normalized_shape[0], m.eps
            r.gamma, r.dgamma = vec(prefix + ".weight", r.C)
            r.beta, r.dbeta = vec(prefix + ".bias", r.C)
            return r

        self.stages = []
        fi = 0
        feats = model.features
        while fi < len(feats):
            pre = f"features.{fi}"
            seq = feats[fi]
            if fi == 0:     # stem: conv then LayerNorm2d
                rec = {"conv": conv(pre + ".0", seq[0]), "ln": ln(pre + ".1", seq[1]), "stem": True}
            else:           # downsample: LayerNorm2d then conv
                rec = {"ln": ln(pre + ".0", seq[0]), "conv": conv(pre + ".1", seq[1]), "stem": False}
            rec["off"] = offs[pre + (".0.weight")]
            rec["blocks"] = []
            fi += 1
            if fi < len(feats) and isinstance(feats[fi][0], CNBlock):
                for j, blk in enumerate(feats[fi]):
                    bp = f"features.{fi}.{j}"
                    b = _Rec()
                    b.C = blk.block[0].out_channels
                    if blk.block[0].kernel_size != (7, 7):
                        raise PfrError("HIP ConvNeXt path supports the 7x7 depthwise kernel")
                    if b.C % self.kp or b.C // self.kp > 256:   # what pfr_dwconv2d_* / pfr_layer_scale_* take (csrc/pfr_dwconv.hip)
                        raise PfrError(f"HIP ConvNeXt path: block width {b.C} must be a multiple of {self.kp} and at most "
                                       f"{256 * self.kp} in {self.dtype}")
                    b.dw_off = offs[bp + ".block.0.weight"]
                    b.dw_g = self.grad[b.dw_off:b.dw_off + b.C * 49]
                    b.dw_bias, b.dw_dbias = vec(bp + ".block.0.bias", b.C)
                    b.dw_w = torch.zeros(49 * b.C, dtype=self.dtype, device=dev)    # tap-major [49][C]
                    b.ln = ln(bp + ".block.2", blk.block[2])
                    b.fc1 = lin(bp + ".block.3", blk.block[3])
                    b.fc2 = lin(bp + ".block.5", blk.block[5])
                    b.gamma, b.dgamma = vec(bp + ".layer_scale", b.C)
                    rec["blocks"].append(b)
                fi += 1
            self.stages.append(rec)
        self.n_blocks = sum(len(st["blocks"]) for st in self.stages)
        self.head_ln = ln("classifier.0", model.classifier[0])
        self.head_fc = lin("classifier.2", model.classifier[2])
        self.head_off = offs["classifier.0.weight"]
        self.emb_dim = self.head_fc.out
        self.in_channels = self.stages[0]["conv"].cin
        self.cp = self.stages[0]["conv"].cinp
        torch.cuda.synchronize(dev)

    def _all_lins(self):
        for st in self.stages:
            yield st["conv"]
            for b in st["blocks"]:
                yield b.fc1
                yield b.fc2
        yield self.head_fc

    def refresh_weights(self, stream, for_backward=True):
        """compute-dtype shadow, conv layouts and tap-major depthwise weights from the fp32 master — on every forward pass, so an
        optimizer step, swap_averaged() or a loaded checkpoint needs no call of its own"""
        if self.dtype != torch.float32:
            lib.pfr_cast(self.master.data_ptr(), 0, self.shadow.data_ptr(), self.did, self.n_flat, stream)
        for st in self.stages:
            r = st["conv"]     # [O][I][f*f] → [O][f*f][I padded]
            lib.pfr_nchw_to_nhwc(self.master.data_ptr() + 4 * r.off, r.w.data_ptr(), self.did, r.out, r.cin, r.f * r.f, 1, r.cinp, stream)
            for b in st["blocks"]:   # [C][49] → [49][C]
                lib.pfr_nchw_to_nhwc(self.master.data_ptr() + 4 * b.dw_off, b.dw_w.data_ptr(), self.did, 1, b.C, 49, 1, b.C, stream)
        if for_backward:
            self._refresh_dgrad_layouts(stream)

    def _wt_records(self):
        for r in self._all_lins():
            if r.f is None:
                yield (r.w.data_ptr(), r.wt.data_ptr(), r.out, 1, 1, r.inp)
            elif r is not self.stages[0]["conv"]:      # (the stem has no data gradient)
                yield (r.w.data_ptr(), r.wt.data_ptr(), r.out, r.f, r.f, r.cinp)

    # ------------------------------------------------------------------------------------------ plan
    def build_plan(self, N, H, W, with_backward):
        T, dev, did = self.dtype, self.device, self.did
        plan = Plan()
        fwd, bwd = [], []

        def A(shape, dtype=None):
            return plan.keep(torch.empty(shape, dtype=dtype or T, device=dev))

        def gemm(ops, x, rows, cin, r, y, residual=None):
            ops.append((lib.pfr_conv2d_fwd, (x.data_ptr(), r.w.data_ptr(), y.data_ptr(), did, dtype_id(y.dtype), rows, 1, 1, cin, r.out,
                                             1, 1, 1, 0, 0, 1, 1, r.out, r.bias.data_ptr(),
                                             0 if residual is None else residual.data_ptr(), 0, 0, 0, 0, 0, 0)))

        def ln_fwd(ops, x, lnrec, rows, C):
            y = A((rows, C)); mu = A((rows,), torch.float32); rs = A((rows,), torch.float32)
            ops.append((lib.pfr_layernorm_fwd, (x.data_ptr(), lnrec.gamma.data_ptr(), lnrec.beta.data_ptr(), y.data_ptr(), mu.data_ptr(),
                                                rs.data_ptr(), did, rows, C, float(lnrec.eps))))
            return y, mu, rs

        x_nhwc = A((N, H, W, self.cp))
        sd = A((self.n_blocks, N), torch.float32)
        cur, cshape = x_nhwc, (N, H, W, self.cp)
        saved = []
        bid = 0
        for st in self.stages:
            cv = st["conv"]
            f = cv.f
            Nn, Hh, Ww, Cc = cshape
            if Hh % f or Ww % f or Hh < f or Ww < f:
                raise PfrError(f"ConvNeXt: a {Hh}x{Ww} plane does not divide by the {f}x{f} stride-{f} convolution")
            OH, OW, C = Hh // f, Ww // f, cv.out
            rows = N * OH * OW
            srec = {"shape": (N, OH, OW, C), "inshape": cshape, "blocks": []}
            if not st["stem"]:
                srec["ln_in"] = cur
                cur, srec["mu"], srec["rs"] = ln_fwd(fwd, cur, st["ln"], N * Hh * Ww, Cc)
            srec["conv_in"] = cur
            t = A((N, OH, OW, C))
            fwd.append((lib.pfr_conv2d_fwd, (cur.data_ptr(), cv.w.data_ptr(), t.data_ptr(), did, did, N, Hh, Ww, Cc, C, f, f, f, 0, 0,
                                             OH, OW, C, cv.bias.data_ptr(), 0, 0, 0, 0, 0, 0, 0)))
            if st["stem"]:
                srec["ln_in"] = t
                t, srec["mu"], srec["rs"] = ln_fwd(fwd, t, st["ln"], rows, C)
            x = t
            for b in st["blocks"]:
                d = A((N, OH, OW, C))
                fwd.append((lib.pfr_dwconv2d_fwd, (x.data_ptr(), b.dw_w.data_ptr(), b.dw_bias.data_ptr(), d.data_ptr(), did, N, OH, OW, C,
                                                   7, 0)))
                l, mu, rs = ln_fwd(fwd, d, b.ln, rows, C)
                h1 = A((rows, 4 * C))
                h2 = A((rows, 4 * C))
                # GELU in the fc1 GEMM's epilogue (writes the pre-activation h1 and h2 = gelu(h1))
                fwd.append((lib.pfr_gemm_act, (l.data_ptr(), b.fc1.w.data_ptr(), h2.data_ptr(), did, rows, C, 4 * C, b.fc1.bias.data_ptr(),
                                               2, h1.data_ptr())))
                u = A((rows, C))
                gemm(fwd, h2, rows, 4 * C, b.fc2, u)
                z = A((N, OH, OW, C))
                row_scale = sd[bid]
                fwd.append((lib.pfr_layer_scale_fwd, (u.data_ptr(), b.gamma.data_ptr(), row_scale.data_ptr(), x.data_ptr(), z.data_ptr(),
                                                      did, N, OH * OW, C)))
                srec["blocks"].append(dict(x=x, d=d, l=l, mu=mu, rs=rs, h1=h1, h2=h2, u=u, row_scale=row_scale))
                x = z
                bid += 1
            saved.append(srec)
            cur, cshape = x, (N, OH, OW, C)
        Nn, Hh, Ww, Cf = cshape
        pooled = A((N, Cf))
        fwd.append((lib.pfr_avgpool_fwd, (cur.data_ptr(), pooled.data_ptr(), did, N, Hh * Ww, Cf)))
        hln, hmu, hrs = ln_fwd(fwd, pooled, self.head_ln, N, Cf)
        emb = A((N, self.emb_dim), torch.float32)
        gemm(fwd, hln, N, Cf, self.head_fc, emb)
        plan.ops = fwd
        plan.meta.update(x_nhwc=x_nhwc, sd=sd, emb=emb, n_fwd=len(fwd))
        if not with_backward:
            return plan

        # ================================================================= backward
        # Weight gradients (GEMM and depthwise) and column sums feed nothing before the optimizer: they run on the SIDE stream with
        # the FORK / SREC / WAIT roles of _hip/cplan.py, exactly as in SwinEngine.build_plan (see the comments there).
        pool = {}
        nalloc = {}
        pending = {}      # data_ptr of a pooled buffer -> last side op that reads it
        side_reads = []   # (k, data_ptr) of every side-op input
        nside = [0]
        ws_need = [0]
        pend_cs = []      # deferred final merges: (partials, out, partial rows, C, tile height | 0, rows)

        def G(shape, dtype=None):
            key = (tuple(shape), dtype or T)
            lst = pool.setdefault(key, [])
            for i, t in enumerate(lst):
                if t.data_ptr() not in pending:
                    return lst.pop(i)
            if not lst or nalloc.get(key, 0) < self.pool_depth:
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
                k = ops.pop()[1]
            else:
                k = nside[0]
                nside[0] += 1
                ops.append((FORK, k))
            ops.append(op)
            ops.append((SREC, k))
            for r in reads:
                side_reads.append((k, r.data_ptr()))

        def wgrad(ops, x, xshape, dy, dyshape, R, stride, out):
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

        def colsum(ops, x, rows, C, out):
            n = lib.pfr_colsum_parts(did, rows, C)
            if n <= 0:
                side(ops, (SIDE, (lib.pfr_colsum, (x.data_ptr(), did, rows, C, out.data_ptr(), 0, 0))), x)
                return
            ws = A((lib.pfr_colsum_ws_floats(rows, C),), torch.float32)
            side(ops, (SIDE, (lib.pfr_colsum_partial, (x.data_ptr(), did, rows, C, ws.data_ptr()))), x)
            pend_cs.append((ws, out, n, C, 0, 0))

        def flush_colsums(ops):
            if not pend_cs:
                return
            raw = b"".join(struct.pack("<QQiiiiii", ws.data_ptr(), out.data_ptr(), n, C, 0, mt, rws, 0) for ws, out, n, C, mt, rws in pend_cs)
            tab = plan.keep(torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev))
            side(ops, (SIDE, (lib.pfr_colsum_final_batch, (tab.data_ptr(), len(pend_cs), max(e[3] for e in pend_cs)))))
            del pend_cs[:]

        def ln_bwd(ops, dy, xin, mu, rs, lnrec, dres, dx, rows, C, want_sum=False):
            """→ (partials, rows of partials) of the column sums of dx when want_sum and the kernel can emit them, else None"""
            nb = lib.pfr_layernorm_bwd_blocks(rows)
            part = A((2, nb, C), torch.float32)
            dsum = A((nb, C), torch.float32) if (want_sum and lib.pfr_layernorm_bwd_dxsum_ok(did, C)) else None
            ops.append((lib.pfr_layernorm_bwd_dxsum, (dy.data_ptr(), xin.data_ptr(), mu.data_ptr(), rs.data_ptr(), lnrec.gamma.data_ptr(),
                                                      0 if dres is None else dres.data_ptr(), dx.data_ptr(), part.data_ptr(),
                                                      0 if dsum is None else dsum.data_ptr(), did, rows, C)))
            pend_cs.append((part[0], lnrec.dgamma, nb, C, 0, 0))
            pend_cs.append((part[1], lnrec.dbeta, nb, C, 0, 0))
            return None if dsum is None else (dsum, nb)

        def bias_grad(ops, g, rows, C, dbias, gsum):
            if gsum is not None:
                pend_cs.append((gsum[0], dbias, gsum[1], C, 0, 0))
            else:
                colsum(ops, g, rows, C, dbias)

        demb = A((N, self.emb_dim))
        plan.meta["demb"] = demb
        hf = self.head_fc
        colsum(bwd, demb, N, hf.out, hf.dbias)
        wgrad(bwd, hln, (N, 1, 1, Cf), demb, (N, 1, 1, hf.out), 1, 1, hf.g)
        dhln = G((N, Cf))
        dgrad_lin(bwd, demb, N, hf, dhln)
        dpooled = G((N, Cf))
        ln_bwd(bwd, dhln, pooled, hmu, hrs, self.head_ln, None, dpooled, N, Cf)
        release(dhln)
        dz = G(cshape)
        bwd.append((lib.pfr_avgpool_bwd, (dpooled.data_ptr(), dz.data_ptr(), did, N, Hh * Ww, Cf)))
        release(dpooled)
        flush_colsums(bwd)
        bwd.append((MWAIT, nside[0] - 1))
        bwd.append((None, (self.head_off,)))
        dz_sum = None   # column sums of dz left by the pass that produced it
        for si in range(len(self.stages) - 1, -1, -1):
            st, srec = self.stages[si], saved[si]
            Nn, OH, OW, C = srec["shape"]
            rows = N * OH * OW
            for b, sv in zip(reversed(st["blocks"]), reversed(srec["blocks"])):
                # ---- 1. layer scale · stochastic depth: du = sd γ dz, dγ = Σ sd dz u (partials merged with the deferred column sums)
                du = G((rows, C))
                nlp = lib.pfr_layer_scale_bwd_parts(N, OH * OW, C)
                lpart = A((nlp, C), torch.float32)
                bwd.append((lib.pfr_layer_scale_bwd, (dz.data_ptr(), sv["u"].data_ptr(), b.gamma.data_ptr(), sv["row_scale"].data_ptr(),
                                                      du.data_ptr(), lpart.data_ptr(), 0, did, N, OH * OW, C, 0)))
                pend_cs.append((lpart, b.dgamma, nlp, C, 0, 0))
                # ---- 2. Linear 4C→C: bias, weight and data gradient; 3. GELU backward in the data-gradient GEMM's epilogue
                colsum(bwd, du, rows, C, b.fc2.dbias)
                wgrad(bwd, sv["h2"], (rows, 1, 1, 4 * C), du, (rows, 1, 1, C), 1, 1, b.fc2.g)
                dh = G((rows, 4 * C))
                nsum = lib.pfr_gemm_act_colsum_parts(rows, C, 4 * C, did)
                if nsum > 0:     # streaming Linear kernel: plain column sums per row range
                    stp = A((nsum, 4 * C), torch.float32)
                    bwd.append((lib.pfr_gemm_act_colsums, (du.data_ptr(), b.fc2.wt.data_ptr(), dh.data_ptr(), did, rows, C, 4 * C,
                                                           sv["h1"].data_ptr(), stp.data_ptr())))
                    pend_cs.append((stp, b.fc1.dbias, nsum, 4 * C, 0, 0))
                else:
                    mt = lib.pfr_gemm_act_mtile(rows, C, 4 * C, did)
                    nt = (rows + mt - 1) // mt
                    stp = A((nt, 2, 4 * C), torch.float32)
                    bwd.append((lib.pfr_gemm_act_colstats, (du.data_ptr(), b.fc2.wt.data_ptr(), dh.data_ptr(), did, rows, C, 4 * C, 0, 3,
                                                            sv["h1"].data_ptr(), stp.data_ptr())))
                    pend_cs.append((stp, b.fc1.dbias, nt, 4 * C, mt, rows))
                release(du)
                # ---- 4. Linear C→4C
                wgrad(bwd, sv["l"], (rows, 1, 1, C), dh, (rows, 1, 1, 4 * C), 1, 1, b.fc1.g)
                dl = G((rows, C))
                dgrad_lin(bwd, dh, rows, b.fc1, dl)
                release(dh)
                # ---- 5. LayerNorm
                dd = G((N, OH, OW, C))
                ln_bwd(bwd, dl, sv["d"], sv["mu"], sv["rs"], b.ln, None, dd, rows, C)
                release(dl)
                # ---- 6. depthwise conv: weight + bias gradient (side stream), data gradient = the same conv with mirrored taps
                npart = lib.pfr_dwconv2d_wgrad_parts(did, N, OH, OW, C, 7)
                dpart = A((npart, 50, C), torch.float32)
                side(bwd, (SIDE, (lib.pfr_dwconv2d_wgrad, (sv["x"].data_ptr(), dd.data_ptr(), dpart.data_ptr(), b.dw_g.data_ptr(),
                                                           b.dw_dbias.data_ptr(), did, N, OH, OW, C, 7, 0))), dd)
                dxb = G((N, OH, OW, C))
                bwd.append((lib.pfr_dwconv2d_fwd, (dd.data_ptr(), b.dw_w.data_ptr(), 0, dxb.data_ptr(), did, N, OH, OW, C, 7, 1)))
                release(dd)
                # ---- 7. residual
                dx = G((N, OH, OW, C))
                bwd.append((lib.pfr_add, (dz.data_ptr(), dxb.data_ptr(), dx.data_ptr(), did, rows * C)))
                release(dxb)
                release(dz)
                dz = dx
                dz_sum = None
            # ---- stem (conv → LN) / downsample (LN → conv)
            cv = st["conv"]
            f = cv.f
            Ni, Hi, Wi, Ci = srec["inshape"]
            if st["stem"]:
                dconv = G((N, OH, OW, C))
                dz_sum = ln_bwd(bwd, dz, srec["ln_in"], srec["mu"], srec["rs"], st["ln"], None, dconv, rows, C, want_sum=True)
                release(dz)
                dz = dconv
            bias_grad(bwd, dz, rows, C, cv.dbias, dz_sum)
            wgrad(bwd, srec["conv_in"], (Ni, Hi, Wi, Ci), dz, (N, OH, OW, C), f, f, cv.g_conv)
            side(bwd, (SIDE, (lib.pfr_nhwc_to_nchw_f32, (cv.g_conv.data_ptr(), cv.g.data_ptr(), cv.out, cv.cin, f * f, cv.cinp, 0))))
            if not st["stem"]:
                dlin = G((Ni, Hi, Wi, Ci))
                bwd.append((lib.pfr_conv2d_fwd, (dz.data_ptr(), cv.wt.data_ptr(), dlin.data_ptr(), did, did, N, OH, OW, C, Ci, f, f, 1,
                                                 f - 1, {2: 1, 4: 2}[f], Hi, Wi, Ci, 0, 0, 0, 0, 0, 0, 0, 0)))
                release(dz)
                din = G((Ni, Hi, Wi, Ci))
                ln_bwd(bwd, dlin, srec["ln_in"], srec["mu"], srec["rs"], st["ln"], None, din, Ni * Hi * Wi, Ci)
                release(dlin)
                dz = din
            dz_sum = None
            flush_colsums(bwd)
            bwd.append((WAIT if si == 0 else MWAIT, nside[0] - 1))
            bwd.append((None, (st["off"],)))
        plan.meta["n_side"] = nside[0]
        if self.ws is None or self.ws.numel() < ws_need[0]:
            self.ws = torch.empty(ws_need[0], dtype=torch.float32, device=dev)
        plan.ops = fwd + bwd
        return plan

    def forward(self, x, sd, with_backward, ticket=None):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise PfrError(f"expected NCHW input with {self.in_channels} channels, got {tuple(x.shape)}")
        x = x.float().contiguous()
        N, _, H, W = x.shape
        if tuple(sd.shape) != (self.n_blocks, N):
            raise PfrError(f"stochastic-depth draw of shape {tuple(sd.shape)}, expected {(self.n_blocks, N)}")
        plan = self.acquire_plan(N, H, W, with_backward, ticket=ticket if with_backward else None)
        if with_backward:
            self._fresh(plan)
        stream = torch.cuda.current_stream().cuda_stream
        self.refresh_weights(stream, for_backward=with_backward)
        plan.meta["sd"].copy_(sd, non_blocking=True)
        lib.pfr_nchw_to_nhwc(x.data_ptr(), plan.meta["x_nhwc"].data_ptr(), self.did, N, x.shape[1], H, W, self.cp, stream)
        self._run_fwd(plan, stream)
        self._last_plan = plan
        return plan.meta["emb"]

    def backward(self, demb, plan=None):
        plan = plan if plan is not None else self._last_plan
        self._begin_backward(plan, demb)
        # As in SwinEngine: the plan's gradient launches overwrite their slices; a second backward before zero_grad sets the previous
        # sum aside and adds it back (the accumulate forms of pfr_dwconv2d_wgrad / pfr_layer_scale_bwd serve hosts without this detour)
        prev = self.grad.clone() if self.first_param.grad is not None else None
        hook = self.grad_ready_hook
        if prev is not None or any(self._plan_busy(q) for q in self.plans.values()):
            hook = None
        self._run_bwd(plan, "bwd", hook, hook)
        if prev is not None:
            self.grad.add_(prev)
        self.attach_grads()


convnext_forward = engine_forward
