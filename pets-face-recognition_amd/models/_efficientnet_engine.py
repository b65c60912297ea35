"""EfficientNetEngine — executes the EfficientNet feature extractor (forward, backward) on the gfx950 kernels.

Same design as models/_mobilenet_engine.MobileNetV2Engine: flat fp32 master / gradient buffers (the module's nn.Parameters become
views, torchvision's state-dict names unchanged), compute-dtype shadow, activations NHWC end to end, one pre-built plan of C-ABI calls
per (N, H, W, train, with_backward); the plan runtime and the PlanBuilder that build_plan emits through are models/_plan_engine.py,
the BatchNorm emitters models/_plan_layers.BatchNormLayers.  The BatchNorm buffers live in one flat `stats` tensor.

Mapping (models/efficientnet.py):
  stem 3x3 stride 2, expand / project / last 1x1 → pfr_conv2d_fwd with the BatchNorm partials in its epilogue (stats_part), pfr_conv2d_wgrad
  BatchNorm (train)                               → pfr_bn_finalize from the partials; eval: pfr_bn_eval_coeff, no statistics
  expand BN + SiLU → depthwise k x k              → pfr_bn_act_silu (materialised), pfr_dwconvk_fwd / _dgrad / _wgrad; with fuse_prologue:
                                                    prologue (pro_act 2) of pfr_dwconvk_fwd, the activated expand tensor is never
                                                    stored and its weight gradient recomputes the operand — slower (see __init__)
  depthwise BN + SiLU, last BN + SiLU             → pfr_bn_act_silu (materialised)
  squeeze-and-excitation                          → pfr_avgpool_fwd, pfr_se_gate_fwd, pfr_se_scale_fwd; backward pfr_se_scale_bwd_reduce,
                                                    pfr_se_gate_bwd (fc1 / fc2 gradients), pfr_se_bwd_apply
  project BN (linear) + residual                  → pfr_bn_act(relu = 0) with the residual operand; in training mode, a block with a
                                                    stochastic-depth probability > 0: pfr_bn_residual_rows with the block's row of the
                                                    draw, backward pfr_row_scale in front of the linear BatchNorm step
  BatchNorm (+ SiLU) backward                     → pfr_bn_bwd_reduce_silu / pfr_bn_bwd_finalize / pfr_bn_bwd_apply_silu, the derivative
                                                    recomputed from the convolution output (linear BN: the _clamp forms, mask_mode 0)
  avgpool → Linear                                → pfr_avgpool_fwd, pfr_conv2d_fwd
"""
import torch
import torch.nn as nn

from .._hip import lib, dtype_id, PfrError
from .._hip.cplan import SIDE
from ._plan_engine import PlanEngine, PlanBuilder, Plan, engine_forward
from ._plan_layers import BatchNormLayers


class _Rec:
    pass


class EfficientNetEngine(PlanEngine):
    max_plans = 6

    def __init__(self, model, device, compute_dtype=None):
        super().__init__(model, device, compute_dtype)
        # True: the expand BatchNorm + SiLU as the prologue of pfr_dwconvk_fwd / pfr_dwconvk_wgrad (the activated expand tensor is never
        # stored).  False: a materialising pfr_bn_act_silu before each depthwise conv.  The A/B of tools/efficientnet_bench.py went to
        # the materialised form (profiles/efficientnet_b2.txt, bs 256: 43.70 against 51.10 ms/step; the prologue pays one exponential per TAP, 9 or 25 per element, and
        # the depthwise kernels run far below the streaming rate), so that is the default; the fused form stays available.
        # Read when a plan is built and not part of the plan key: set it before the first forward
        self.fuse_prologue = False
        self._adopt(model)

    # ------------------------------------------------------------------------------------------ parameters
    def _adopt(self, model):
        from .efficientnet import MBConv, SqueezeExcitation
        dev, what = self.device, "EfficientNet"
        # the reference's head, a bare Linear (keys classifier.weight / classifier.bias), or torchvision's Sequential(Dropout, Linear)
        if isinstance(model.classifier, nn.Linear):
            lins, self._dropouts = [("classifier", model.classifier)], []
        else:
            seq = list(model.classifier) if isinstance(model.classifier, nn.Sequential) else [model.classifier]
            lins = [(f"classifier.{i}", m) for i, m in enumerate(seq) if not isinstance(m, nn.Dropout)]
            self._dropouts = [m for m in seq if isinstance(m, nn.Dropout)]
        if len(lins) != 1 or not isinstance(lins[0][1], nn.Linear):
            raise PfrError("HIP EfficientNet path needs a classifier of exactly one Linear (bare, or in a Sequential with Dropout layers)")
        named = list(model.named_parameters())
        if not all(p.requires_grad for _, p in named):
            raise PfrError("HIP EfficientNet path trains every parameter (no frozen layers)")
        offs = self._adopt_flat(named)
        bn_of = self._adopt_batchnorms(model, what)     # BatchNorm buffers → flat
        plain, chunked = self._plain, self._chunked

        def pw(prefix, m, bias=False):
            return self._pw(what, prefix, m, bias)

        def vec(name, n):
            o = offs[name]
            return self.master[o:o + n], self.grad[o:o + n]

        feats = model.features
        self._adopt_stem(what, feats[0][0], bn_of[id(feats[0][1])])
        self.blocks = []
        for fi in range(1, len(feats) - 1):
            if not isinstance(feats[fi], nn.Sequential) or not all(isinstance(m, MBConv) for m in feats[fi]):
                raise PfrError(f"features.{fi}: the HIP EfficientNet path expects stages of MBConv blocks between the stem and the last conv")
            for bi, blk in enumerate(feats[fi]):
                pre = f"features.{fi}.{bi}.block"
                b = _Rec()
                b.off = offs[pre + ".0.0.weight"]
                b.stride, b.res, b.K = blk.stride, blk.use_res_connect, blk.kernel
                b.bid = len(self.blocks)
                b.sd = blk.use_res_connect and blk.sd_prob > 0.0
                seq = list(blk.block)
                j = 0
                b.expand = None
                if len(seq) == 4:
                    if not plain(seq[0][0], 1, 1, 1):
                        raise PfrError(f"{pre}: unexpected expand convolution")
                    b.expand = pw(pre + ".0.0", seq[0][0])
                    b.expand.bn = bn_of[id(seq[0][1])]
                    j = 1
                dwc = seq[j][0]
                b.C = dwc.out_channels
                if b.K not in (3, 5) or not plain(dwc, b.K, b.stride, b.C) or dwc.in_channels != b.C:
                    raise PfrError(f"{pre}: the depthwise convolution is 3x3 or 5x5, padding k // 2, stride 1 or 2, bias-free")
                chunked(what, f"{pre}.{j}.0", b.C)
                KK = b.K * b.K
                b.dw_off = offs[f"{pre}.{j}.0.weight"]
                b.dw_g = self.grad[b.dw_off:b.dw_off + KK * b.C]
                b.dw_w = torch.zeros(KK * b.C, dtype=self.dtype, device=dev)     # tap-major [K*K][C]
                b.dw_bn = bn_of[id(seq[j][1])]
                se = seq[j + 1]
                if not isinstance(se, SqueezeExcitation) or se.fc1.in_channels != b.C or se.fc2.out_channels != b.C \
                        or se.fc1.bias is None or se.fc2.bias is None:
                    raise PfrError(f"{pre}.{j + 1}: expected SqueezeExcitation over {b.C} channels with biased fc1 / fc2")
                b.S = se.fc1.out_channels
                sp = f"{pre}.{j + 1}"
                b.w1, b.dw1 = vec(sp + ".fc1.weight", b.S * b.C)
                b.b1, b.db1 = vec(sp + ".fc1.bias", b.S)
                b.w2, b.dw2 = vec(sp + ".fc2.weight", b.S * b.C)
                b.b2, b.db2 = vec(sp + ".fc2.bias", b.C)
                if not plain(seq[j + 2][0], 1, 1, 1) or len(seq[j + 2]) != 2:
                    raise PfrError(f"{pre}: unexpected project convolution")
                b.project = pw(f"{pre}.{j + 2}.0", seq[j + 2][0])
                b.project.bn = bn_of[id(seq[j + 2][1])]
                self.blocks.append(b)
        self.n_blocks = len(self.blocks)
        li = len(feats) - 1
        if not plain(feats[li][0], 1, 1, 1):
            raise PfrError("HIP EfficientNet path: the last feature layer is a bias-free 1x1 convolution")
        self.last = pw(f"features.{li}.0", feats[li][0])
        self.last.bn = bn_of[id(feats[li][1])]
        self.last_off = offs[f"features.{li}.0.weight"]
        ci, cm = lins[0]
        if cm.bias is None:
            raise PfrError("HIP EfficientNet path: the embedding Linear has a bias")
        self.head_fc = pw(ci, cm, bias=True)
        self.head_off = offs[ci + ".weight"]
        self.head_id = id(cm)
        self.emb_dim = self.head_fc.out
        torch.cuda.synchronize(dev)

    def matches(self, model):
        cl = model.classifier
        lin = [cl] if isinstance(cl, nn.Linear) else [m for m in cl if isinstance(m, nn.Linear)] if isinstance(cl, nn.Sequential) else []
        return super().matches(model) and len(lin) == 1 and id(lin[0]) == self.head_id

    def _pws(self):
        for b in self.blocks:
            if b.expand is not None:
                yield b.expand
            yield b.project
        yield self.last
        yield self.head_fc

    def refresh_weights(self, stream, for_backward=True):
        """compute-dtype shadow, the stem's conv layout and the tap-major depthwise weights from the fp32 master — on every forward
        pass, so an optimizer step, swap_averaged() or a loaded checkpoint needs no call of its own"""
        if self.dtype != torch.float32:
            lib.pfr_cast(self.master.data_ptr(), 0, self.shadow.data_ptr(), self.did, self.n_flat, stream)
        st = self.stem     # [O][I][9] → [O][9][I padded]
        lib.pfr_nchw_to_nhwc(self.master.data_ptr() + 4 * st.off, st.w.data_ptr(), self.did, st.out, st.cin, 9, 1, st.cinp, stream)
        for b in self.blocks:   # [C][K*K] → [K*K][C]
            lib.pfr_nchw_to_nhwc(self.master.data_ptr() + 4 * b.dw_off, b.dw_w.data_ptr(), self.did, 1, b.C, b.K * b.K, 1, b.C, stream)
        if for_backward:
            self._refresh_dgrad_layouts(stream)

    def _wt_records(self):
        for r in self._pws():
            yield (r.w.data_ptr(), r.wt.data_ptr(), r.out, 1, 1, r.inp)

    # ------------------------------------------------------------------------------------------ plan
    def build_plan(self, N, H, W, train, with_backward):
        T, dev, did = self.dtype, self.device, self.did
        plan = Plan()
        pb = PlanBuilder(plan, T, dev, did, self.pool_depth)
        A, fwd, bwd = pb.A, pb.fwd, pb.bwd
        bn = BatchNormLayers(pb, train, self.bn_ws)
        coef, bn_fwd, conv_bn = bn.coef, bn.bn_fwd, bn.conv_bn

        def act(z, shape, c):
            """materialised silu(bn(z))"""
            a = A(shape)
            fwd.append((lib.pfr_bn_act_silu, (z.data_ptr(), c.scale.data_ptr(), c.shift.data_ptr(), a.data_ptr(), did,
                                              shape[0] * shape[1] * shape[2], shape[3])))
            return a

        sd = A((max(1, self.n_blocks), N), torch.float32)

        st = self.stem
        x_nhwc = A((N, H, W, self.cp))
        z0, shape, c0 = conv_bn(x_nhwc, (N, H, W, self.cp), st.w, st.out, 3, 2, 1, st.bn)
        # `cur`: the running tensor; `cur_c`: the BatchNorm + SiLU still to be applied to it (None: cur is the activation itself)
        cur, cur_c = z0, c0
        saved = []
        for b in self.blocks:
            sv = _Rec()
            sv.in_raw, sv.in_c, sv.in_shape = cur, cur_c, shape
            # a block without an expand conv leaves the BatchNorm + SiLU of its input to the depthwise prologue, unless it adds
            # that input back: the residual operand is the activation itself and has to exist
            if b.expand is not None or b.res or not self.fuse_prologue:
                if cur_c is not None:
                    cur, cur_c = act(cur, shape, cur_c), None
            sv.xin = cur
            if b.expand is not None:
                sv.ze, eshape, sv.ce = conv_bn(cur, shape, b.expand.w, b.expand.out, 1, 1, 0, b.expand.bn)
                dsrc, dc = sv.ze, sv.ce
                if not self.fuse_prologue:
                    dsrc, dc = act(sv.ze, eshape, sv.ce), None
            else:
                eshape, dsrc, dc = shape, cur, cur_c
            sv.dsrc, sv.dc, sv.eshape = dsrc, dc, eshape
            Nq, Hq, Wq, Ch = eshape
            OH, OW = (Hq - 1) // b.stride + 1, (Wq - 1) // b.stride + 1
            M = Nq * OH * OW
            sv.zd, sv.dshape = A((Nq, OH, OW, Ch)), (Nq, OH, OW, Ch)
            rpp, nparts, part = 0, 0, None
            if train:
                rpp = lib.pfr_dwconvk_rows_per_part(did, Nq, Hq, Wq, Ch, b.K, b.stride)
                nparts = (M + rpp - 1) // rpp
                part = A((nparts, 2, Ch), torch.float32)
            fwd.append((lib.pfr_dwconvk_fwd, (dsrc.data_ptr(), b.dw_w.data_ptr(), sv.zd.data_ptr(), did, Nq, Hq, Wq, Ch, b.K, b.stride,
                                              2 if dc else 0, dc.scale.data_ptr() if dc else 0, dc.shift.data_ptr() if dc else 0, 0.0,
                                              part.data_ptr() if train else 0)))
            sv.cd = coef(b.dw_bn)
            bn_fwd(sv.cd, part, nparts, rpp, M)
            sv.ad = act(sv.zd, sv.dshape, sv.cd)
            # squeeze-and-excitation: squeeze (avgpool), gate (fc1 → SiLU → fc2 → sigmoid, fp32), scale
            sv.pooled, sv.pre, sv.gate = A((Nq, Ch)), A((Nq, b.S), torch.float32), A((Nq, Ch), torch.float32)
            fwd.append((lib.pfr_avgpool_fwd, (sv.ad.data_ptr(), sv.pooled.data_ptr(), did, Nq, OH * OW, Ch)))
            fwd.append((lib.pfr_se_gate_fwd, (sv.pooled.data_ptr(), b.w1.data_ptr(), b.b1.data_ptr(), b.w2.data_ptr(), b.b2.data_ptr(),
                                              sv.pre.data_ptr(), sv.gate.data_ptr(), did, Nq, Ch, b.S)))
            sv.ys = A(sv.dshape)
            fwd.append((lib.pfr_se_scale_fwd, (sv.ad.data_ptr(), sv.gate.data_ptr(), sv.ys.data_ptr(), did, Nq, OH * OW, Ch)))
            sv.zp, pshape, sv.cp = conv_bn(sv.ys, sv.dshape, b.project.w, b.project.out, 1, 1, 0, b.project.bn)
            sv.out = A(pshape)
            sv.rows_sd = bool(b.sd and train)     # per-sample stochastic depth: this block's row of the draw scales the branch
            if sv.rows_sd:
                fwd.append((lib.pfr_bn_residual_rows, (sv.zp.data_ptr(), sv.cp.scale.data_ptr(), sv.cp.shift.data_ptr(), sv.xin.data_ptr(),
                                                       sd[b.bid].data_ptr(), sv.out.data_ptr(), did, Nq, OH * OW, pshape[3])))
            else:
                fwd.append((lib.pfr_bn_act, (sv.zp.data_ptr(), sv.cp.scale.data_ptr(), sv.cp.shift.data_ptr(),
                                             sv.xin.data_ptr() if b.res else 0, 0, 0, sv.out.data_ptr(), did, M, pshape[3], 0)))
            sv.pshape = pshape
            saved.append(sv)
            cur, cur_c, shape = sv.out, None, pshape
        if cur_c is not None:     # (a network without blocks)
            cur, cur_c = act(cur, shape, cur_c), None
        last_in, last_inshape = cur, shape
        zl, lshape, cl = conv_bn(cur, shape, self.last.w, self.last.out, 1, 1, 0, self.last.bn)
        al = act(zl, lshape, cl)
        Nn, Hh, Ww, Cf = lshape
        pooled = A((N, Cf))
        fwd.append((lib.pfr_avgpool_fwd, (al.data_ptr(), pooled.data_ptr(), did, N, Hh * Ww, Cf)))
        emb = A((N, self.emb_dim), torch.float32)
        hf = self.head_fc
        fwd.append((lib.pfr_conv2d_fwd, (pooled.data_ptr(), hf.w.data_ptr(), emb.data_ptr(), did, dtype_id(emb.dtype), N, 1, 1, Cf, hf.out,
                                         1, 1, 1, 0, 0, 1, 1, hf.out, hf.bias.data_ptr(), 0, 0, 0, 0, 0, 0, 0)))
        plan.ops = fwd
        plan.meta.update(x_nhwc=x_nhwc, sd=sd, emb=emb, n_fwd=len(fwd))
        if not with_backward:
            return plan

        # ================================================================= backward (stream roles, buffer pool: PlanBuilder; the
        # depthwise weight gradients and the bias column sum run on the side stream like the dense weight gradients)
        G, release, side, wgrad, mark = pb.G, pb.release, pb.side, pb.wgrad, pb.mark
        dgrad_pw, bn_bwd = bn.dgrad_pw, bn.bn_bwd

        demb = A((N, self.emb_dim))
        plan.meta["demb"] = demb
        side((SIDE, (lib.pfr_colsum, (demb.data_ptr(), did, N, hf.out, hf.dbias.data_ptr(), 0, 0))), demb)
        wgrad(pooled, (N, 1, 1, Cf), demb, (N, 1, 1, hf.out), 1, 1, 0, hf.g)
        dpooled = G((N, Cf))
        dgrad_pw(demb, N, hf, dpooled)
        dal = G(lshape)
        bwd.append((lib.pfr_avgpool_bwd, (dpooled.data_ptr(), dal.data_ptr(), did, N, Hh * Ww, Cf)))
        release(dpooled)
        mark(self.head_off)
        rows_l = N * Hh * Ww
        dzl = bn_bwd(dal, zl, cl, rows_l, "silu")
        release(dal)
        wgrad(last_in, last_inshape, dzl, lshape, 1, 1, 0, self.last.g)
        dout = G(last_inshape)
        dgrad_pw(dzl, rows_l, self.last, dout)
        release(dzl)
        mark(self.last_off)
        for b, sv in zip(reversed(self.blocks), reversed(saved)):
            Nq, OH, OW, Ch = sv.dshape
            rows_o = Nq * OH * OW
            # ---- project BN (linear) and conv
            dbr = dout
            if sv.rows_sd:     # the branch gradient of a block under stochastic depth: row_scale[n] * dout
                dbr = G(sv.pshape)
                bwd.append((lib.pfr_row_scale, (dout.data_ptr(), sd[b.bid].data_ptr(), dbr.data_ptr(), did, Nq, OH * OW, sv.pshape[3])))
            dzp = bn_bwd(dbr, sv.zp, sv.cp, rows_o)
            if sv.rows_sd:
                release(dbr)
            wgrad(sv.ys, sv.dshape, dzp, sv.pshape, 1, 1, 0, b.project.g)
            dys = G(sv.dshape)
            dgrad_pw(dzp, rows_o, b.project, dys)
            release(dzp)
            # ---- squeeze-and-excitation: dgate = Σ_hw dys·a, the gate's backward (dpooled and the fc1 / fc2 gradients, main stream:
            # they are a few hundred kFLOP and dpooled is needed at once), da = dys·gate + dpooled / HW
            dgate, dpool, dpre = A((Nq, Ch), torch.float32), A((Nq, Ch), torch.float32), A((Nq, b.S), torch.float32)
            bwd.append((lib.pfr_se_scale_bwd_reduce, (dys.data_ptr(), sv.ad.data_ptr(), dgate.data_ptr(), did, Nq, OH * OW, Ch)))
            bwd.append((lib.pfr_se_gate_bwd, (dgate.data_ptr(), sv.pooled.data_ptr(), sv.pre.data_ptr(), sv.gate.data_ptr(), b.w1.data_ptr(),
                                              b.w2.data_ptr(), dpre.data_ptr(), dpool.data_ptr(), b.dw1.data_ptr(), b.db1.data_ptr(),
                                              b.dw2.data_ptr(), b.db2.data_ptr(), did, Nq, Ch, b.S, 0)))
            dad = G(sv.dshape)
            bwd.append((lib.pfr_se_bwd_apply, (dys.data_ptr(), sv.gate.data_ptr(), dpool.data_ptr(), dad.data_ptr(), did, Nq, OH * OW, Ch)))
            release(dys)
            # ---- depthwise BN + SiLU, depthwise conv: weight gradient from the recomputed operand (side), gather data gradient
            dzd = bn_bwd(dad, sv.zd, sv.cd, rows_o, "silu")
            release(dad)
            Ne, He, We, _ = sv.eshape
            npart = lib.pfr_dwconvk_wgrad_parts(did, Ne, He, We, Ch, b.K, b.stride)
            dpart = A((npart, b.K * b.K, Ch), torch.float32)
            dc = sv.dc
            side((SIDE, (lib.pfr_dwconvk_wgrad, (sv.dsrc.data_ptr(), dzd.data_ptr(), dpart.data_ptr(), b.dw_g.data_ptr(), did, Ne, He, We, Ch,
                                                 b.K, b.stride, 2 if dc else 0, dc.scale.data_ptr() if dc else 0,
                                                 dc.shift.data_ptr() if dc else 0, 0.0, 0))), dzd)
            dae = G(sv.eshape)
            bwd.append((lib.pfr_dwconvk_dgrad, (dzd.data_ptr(), b.dw_w.data_ptr(), dae.data_ptr(), did, Ne, He, We, Ch, b.K, b.stride)))
            release(dzd)
            rows_e = Ne * He * We
            if b.expand is not None:     # (materialised or fused into the depthwise prologue: the backward is the same BN + SiLU step)
                dze = bn_bwd(dae, sv.ze, sv.ce, rows_e, "silu")
                release(dae)
                wgrad(sv.xin, sv.in_shape, dze, sv.eshape, 1, 1, 0, b.expand.g)
                dxin = G(sv.in_shape)
                dgrad_pw(dze, rows_e, b.expand, dxin, residual=dout if b.res else None)
                release(dze)
            elif b.res:
                dxin = G(sv.in_shape)
                bwd.append((lib.pfr_add, (dae.data_ptr(), dout.data_ptr(), dxin.data_ptr(), did, rows_e * Ch)))
                release(dae)
            else:
                dxin = dae
            release(dout)
            dout = dxin
            if sv.in_c is not None:     # the block input was silu(bn(raw)) of the layer before (the stem): its BatchNorm step
                dz = bn_bwd(dout, sv.in_raw, sv.in_c, rows_e, "silu")
                release(dout)
                dout = dz
            if b.stride == 2 and b is not self.blocks[0]:
                mark(b.off)
        if not self.blocks:
            dz = bn_bwd(dout, z0, c0, shape[0] * shape[1] * shape[2], "silu")
            release(dout)
            dout = dz
        # ---- stem (no data gradient)
        wgrad(x_nhwc, (N, H, W, self.cp), dout, (N,) + tuple(z0.shape[1:]), 3, 2, 1, st.g_conv)
        side((SIDE, (lib.pfr_nhwc_to_nchw_f32, (st.g_conv.data_ptr(), st.g.data_ptr(), st.out, st.cin, 9, st.cinp, 0))))
        mark(0, last=True)
        return pb.finish(self)

    def forward(self, x, sd, train, with_backward, ticket=None):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise PfrError(f"expected NCHW input with {self.in_channels} channels, got {tuple(x.shape)}")
        if train and any(d.p > 0 for d in self._dropouts):
            raise PfrError("HIP EfficientNet path: Dropout with p > 0 does not run on the device in training mode; use the reference's "
                           "classifier form, `m.classifier = torch.nn.Linear(m.classifier[1].in_features, 512)`, or build the "
                           "model with dropout=0")
        if with_backward and not train:
            raise PfrError("HIP EfficientNet path: a backward pass needs training mode (eval-mode BatchNorm has no backward here)")
        x = x.float().contiguous()
        N, _, H, W = x.shape
        if tuple(sd.shape) != (self.n_blocks, N):
            raise PfrError(f"stochastic-depth draw of shape {tuple(sd.shape)}, expected {(self.n_blocks, N)}")
        fill = (lambda plan: plan.meta["sd"].copy_(sd, non_blocking=True)) if self.n_blocks else None
        emb = self._forward_plan(x, N, H, W, train, with_backward, with_backward=with_backward, ticket=ticket, fill=fill)
        if train:
            self.nbt.add_(1)
        return emb


def efficientnet_forward(model, x, sd):
    """training mode: forward under autograd; eval mode: the inference plan (running statistics, no autograd graph)"""
    if model.training:
        return engine_forward(model, x, sd, True)
    with torch.no_grad():
        return engine_forward(model, x, sd, False)
