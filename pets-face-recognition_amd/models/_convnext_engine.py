"""ConvNeXtEngine — executes the ConvNeXt-T/S feature extractor (forward, backward) on the gfx950 kernels.

Same design as models/_swin_engine.SwinEngine: flat fp32 master / gradient buffers (the module's nn.Parameters become views,
torchvision's state-dict names unchanged), compute-dtype shadow, activations NHWC end to end, one pre-built plan of C-ABI calls per
input shape; the plan runtime and the PlanBuilder that build_plan emits through are models/_plan_engine.py, the Linear / LayerNorm
emitters models/_plan_layers.py.

Mapping (models/convnext.py):
  4x4 stride-4 stem, 2x2 stride-2 downsample convs → pfr_conv2d_fwd on NHWC (weights re-laid out per step), pfr_conv2d_wgrad
  LayerNorm2d / LayerNorm                          → pfr_layernorm_fwd / pfr_layernorm_bwd_dxsum on the [N*H*W, C] rows
  depthwise 7x7 conv                               → pfr_dwconv2d_fwd (flip = 1: data gradient), pfr_dwconv2d_wgrad (csrc/pfr_dwconv.hip)
  Linear C→4C + GELU, Linear 4C→C                  → pfr_gemm_act / pfr_conv2d_fwd, as the Swin MLP
  layer scale · stochastic depth + residual        → pfr_layer_scale_fwd / pfr_layer_scale_bwd
  avgpool → LayerNorm2d → Linear                   → pfr_avgpool_fwd, pfr_layernorm_fwd, pfr_conv2d_fwd
"""
import torch
import torch.nn as nn

from .._hip import lib, PfrError
from .._hip.cplan import SIDE
from ._plan_engine import PlanEngine, PlanBuilder, Plan, engine_forward
from ._plan_layers import gemm, dgrad_lin, ln_fwd, ln_bwd, bias_grad


class _Rec:
    pass


class ConvNeXtEngine(PlanEngine):
    max_plans = 6

    def __init__(self, model, device, compute_dtype=None):
        super().__init__(model, device, compute_dtype)
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
        offs = self._adopt_flat(named)

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
        pb = PlanBuilder(plan, T, dev, did, self.pool_depth)
        A, fwd, bwd = pb.A, pb.fwd, pb.bwd

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
                cur, srec["mu"], srec["rs"] = ln_fwd(pb, cur, st["ln"], N * Hh * Ww, Cc)
            srec["conv_in"] = cur
            t = A((N, OH, OW, C))
            fwd.append((lib.pfr_conv2d_fwd, (cur.data_ptr(), cv.w.data_ptr(), t.data_ptr(), did, did, N, Hh, Ww, Cc, C, f, f, f, 0, 0,
                                             OH, OW, C, cv.bias.data_ptr(), 0, 0, 0, 0, 0, 0, 0)))
            if st["stem"]:
                srec["ln_in"] = t
                t, srec["mu"], srec["rs"] = ln_fwd(pb, t, st["ln"], rows, C)
            x = t
            for b in st["blocks"]:
                d = A((N, OH, OW, C))
                fwd.append((lib.pfr_dwconv2d_fwd, (x.data_ptr(), b.dw_w.data_ptr(), b.dw_bias.data_ptr(), d.data_ptr(), did, N, OH, OW, C,
                                                   7, 0)))
                l, mu, rs = ln_fwd(pb, d, b.ln, rows, C)
                h1 = A((rows, 4 * C))
                h2 = A((rows, 4 * C))
                # GELU in the fc1 GEMM's epilogue (writes the pre-activation h1 and h2 = gelu(h1))
                fwd.append((lib.pfr_gemm_act, (l.data_ptr(), b.fc1.w.data_ptr(), h2.data_ptr(), did, rows, C, 4 * C, b.fc1.bias.data_ptr(),
                                               2, h1.data_ptr())))
                u = A((rows, C))
                gemm(pb, h2, rows, 4 * C, b.fc2, u)
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
        hln, hmu, hrs = ln_fwd(pb, pooled, self.head_ln, N, Cf)
        emb = A((N, self.emb_dim), torch.float32)
        gemm(pb, hln, N, Cf, self.head_fc, emb)
        plan.ops = fwd
        plan.meta.update(x_nhwc=x_nhwc, sd=sd, emb=emb, n_fwd=len(fwd))
        if not with_backward:
            return plan

        # ================================================================= backward (stream roles, buffer pool: PlanBuilder; the
        # depthwise weight gradients run on the side stream like the GEMM ones)
        G, release, side, wgrad, colsum, pend_cs = pb.G, pb.release, pb.side, pb.wgrad, pb.colsum, pb.pend_cs

        demb = A((N, self.emb_dim))
        plan.meta["demb"] = demb
        hf = self.head_fc
        colsum(demb, N, hf.out, hf.dbias)
        wgrad(hln, (N, 1, 1, Cf), demb, (N, 1, 1, hf.out), 1, 1, 0, hf.g)
        dhln = G((N, Cf))
        dgrad_lin(pb, demb, N, hf, dhln)
        dpooled = G((N, Cf))
        ln_bwd(pb, dhln, pooled, hmu, hrs, self.head_ln, None, dpooled, N, Cf)
        release(dhln)
        dz = G(cshape)
        bwd.append((lib.pfr_avgpool_bwd, (dpooled.data_ptr(), dz.data_ptr(), did, N, Hh * Ww, Cf)))
        release(dpooled)
        pb.mark(self.head_off)
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
                colsum(du, rows, C, b.fc2.dbias)
                wgrad(sv["h2"], (rows, 1, 1, 4 * C), du, (rows, 1, 1, C), 1, 1, 0, b.fc2.g)
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
                wgrad(sv["l"], (rows, 1, 1, C), dh, (rows, 1, 1, 4 * C), 1, 1, 0, b.fc1.g)
                dl = G((rows, C))
                dgrad_lin(pb, dh, rows, b.fc1, dl)
                release(dh)
                # ---- 5. LayerNorm
                dd = G((N, OH, OW, C))
                ln_bwd(pb, dl, sv["d"], sv["mu"], sv["rs"], b.ln, None, dd, rows, C)
                release(dl)
                # ---- 6. depthwise conv: weight + bias gradient (side stream), data gradient = the same conv with mirrored taps
                npart = lib.pfr_dwconv2d_wgrad_parts(did, N, OH, OW, C, 7)
                dpart = A((npart, 50, C), torch.float32)
                side((SIDE, (lib.pfr_dwconv2d_wgrad, (sv["x"].data_ptr(), dd.data_ptr(), dpart.data_ptr(), b.dw_g.data_ptr(),
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
                dz_sum = ln_bwd(pb, dz, srec["ln_in"], srec["mu"], srec["rs"], st["ln"], None, dconv, rows, C, want_sum=True)
                release(dz)
                dz = dconv
            bias_grad(pb, dz, rows, C, cv.dbias, dz_sum)
            wgrad(srec["conv_in"], (Ni, Hi, Wi, Ci), dz, (N, OH, OW, C), f, f, 0, cv.g_conv)
            side((SIDE, (lib.pfr_nhwc_to_nchw_f32, (cv.g_conv.data_ptr(), cv.g.data_ptr(), cv.out, cv.cin, f * f, cv.cinp, 0))))
            if not st["stem"]:
                dlin = G((Ni, Hi, Wi, Ci))
                bwd.append((lib.pfr_conv2d_fwd, (dz.data_ptr(), cv.wt.data_ptr(), dlin.data_ptr(), did, did, N, OH, OW, C, Ci, f, f, 1,
                                                 f - 1, {2: 1, 4: 2}[f], Hi, Wi, Ci, 0, 0, 0, 0, 0, 0, 0, 0)))
                release(dz)
                din = G((Ni, Hi, Wi, Ci))
                ln_bwd(pb, dlin, srec["ln_in"], srec["mu"], srec["rs"], st["ln"], None, din, Ni * Hi * Wi, Ci)
                release(dlin)
                dz = din
            dz_sum = None
            pb.mark(st["off"], last=si == 0)
        return pb.finish(self)

    def forward(self, x, sd, with_backward, ticket=None):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise PfrError(f"expected NCHW input with {self.in_channels} channels, got {tuple(x.shape)}")
        x = x.float().contiguous()
        N, _, H, W = x.shape
        if tuple(sd.shape) != (self.n_blocks, N):
            raise PfrError(f"stochastic-depth draw of shape {tuple(sd.shape)}, expected {(self.n_blocks, N)}")
        return self._forward_plan(x, N, H, W, with_backward, with_backward=with_backward, ticket=ticket,
                                  fill=lambda plan: plan.meta["sd"].copy_(sd, non_blocking=True))


convnext_forward = engine_forward
