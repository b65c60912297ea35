"""MobileNetV2Engine — executes the MobileNetV2 feature extractor (forward, backward) on the gfx950 kernels.

Same design as models/_convnext_engine.ConvNeXtEngine: flat fp32 master / gradient buffers (the module's nn.Parameters become views,
torchvision's state-dict names unchanged), compute-dtype shadow, activations NHWC end to end, one pre-built plan of C-ABI calls per
input shape; the plan runtime and the PlanBuilder that build_plan emits through are models/_plan_engine.py, the BatchNorm emitters
models/_plan_layers.BatchNormLayers.  The BatchNorm buffers live in one flat `stats` tensor as in models/_fe_engine.FEEngine
(running_mean / running_var / num_batches_tracked of the modules become views: PlanEngine._adopt_batchnorms).

Mapping (models/mobilenet.py):
  stem 3x3 stride 2, expand / project / last 1x1 → pfr_conv2d_fwd with the BatchNorm partials in its epilogue (stats_part), pfr_conv2d_wgrad
  BatchNorm (train)                               → pfr_bn_finalize from the partials; eval: pfr_bn_eval_coeff, no statistics
  expand BN + ReLU6 → depthwise 3x3               → prologue of pfr_dwconv3_fwd: the activated expand tensor is never stored; its
                                                    weight gradient recomputes the operand (pfr_dwconv3_wgrad), pfr_dwconv3_dgrad
  depthwise BN + ReLU6 → project, last BN + ReLU6 → pfr_bn_act_clamp (materialised)
  project BN (linear) + residual                  → pfr_bn_act(relu = 0) with the residual operand
  BatchNorm (+ ReLU6) backward                    → pfr_bn_bwd_reduce_clamp / pfr_bn_bwd_finalize / pfr_bn_bwd_apply_clamp, the ReLU6
                                                    mask recomputed from the convolution output
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


class MobileNetV2Engine(PlanEngine):
    max_plans = 6

    def __init__(self, model, device, compute_dtype=None):
        super().__init__(model, device, compute_dtype)
        # False: a materialising pfr_bn_act_clamp before each depthwise conv (tools/mobilenet_bench.py's A/B).  Read when a plan is built
        # and not part of the plan key: set it before the first forward, plans that exist keep the form they were built with
        self.fuse_prologue = True
        self._adopt(model)

    # ------------------------------------------------------------------------------------------ parameters
    def _adopt(self, model):
        from .mobilenet import InvertedResidual
        dev, what = self.device, "MobileNetV2"
        lins = [(i, m) for i, m in enumerate(model.classifier) if not isinstance(m, nn.Dropout)]
        if len(lins) != 1 or not isinstance(lins[0][1], nn.Linear):
            raise PfrError("HIP MobileNetV2 path needs a classifier of exactly one Linear (plus Dropout layers)")
        self._dropouts = [m for m in model.classifier if isinstance(m, nn.Dropout)]
        named = list(model.named_parameters())
        if not all(p.requires_grad for _, p in named):
            raise PfrError("HIP MobileNetV2 path trains every parameter (no frozen layers)")
        offs = self._adopt_flat(named)
        bn_of = self._adopt_batchnorms(model, what)     # BatchNorm buffers → flat
        plain, chunked = self._plain, self._chunked

        def pw(prefix, m, bias=False):
            return self._pw(what, prefix, m, bias)

        feats = model.features
        self._adopt_stem(what, feats[0][0], bn_of[id(feats[0][1])])
        self.blocks = []
        for fi in range(1, len(feats) - 1):
            blk = feats[fi]
            if not isinstance(blk, InvertedResidual):
                raise PfrError(f"features.{fi}: the HIP MobileNetV2 path expects InvertedResidual blocks between the stem and the last conv")
            b = _Rec()
            b.off = offs[f"features.{fi}.conv.0.0.weight"]
            b.stride, b.res = blk.stride, blk.use_res_connect
            seq = list(blk.conv)
            j = 0
            b.expand = None
            if len(seq) == 4:
                if not plain(seq[0][0], 1, 1, 1):
                    raise PfrError(f"features.{fi}: unexpected expand convolution")
                b.expand = pw(f"features.{fi}.conv.0.0", seq[0][0])
                b.expand.bn = bn_of[id(seq[0][1])]
                j = 1
            dwc = seq[j][0]
            b.C = dwc.out_channels
            if not plain(dwc, 3, b.stride, b.C) or dwc.in_channels != b.C:
                raise PfrError(f"features.{fi}: the depthwise convolution is 3x3, padding 1, stride 1 or 2, bias-free")
            chunked(what, f"features.{fi}.conv.{j}.0", b.C)
            b.dw_off = offs[f"features.{fi}.conv.{j}.0.weight"]
            b.dw_g = self.grad[b.dw_off:b.dw_off + 9 * b.C]
            b.dw_w = torch.zeros(9 * b.C, dtype=self.dtype, device=dev)     # tap-major [9][C]
            b.dw_bn = bn_of[id(seq[j][1])]
            if not plain(seq[j + 1], 1, 1, 1):
                raise PfrError(f"features.{fi}: unexpected project convolution")
            b.project = pw(f"features.{fi}.conv.{j + 1}", seq[j + 1])
            b.project.bn = bn_of[id(seq[j + 2])]
            self.blocks.append(b)
        li = len(feats) - 1
        if not plain(feats[li][0], 1, 1, 1):
            raise PfrError("HIP MobileNetV2 path: the last feature layer is a bias-free 1x1 convolution")
        self.last = pw(f"features.{li}.0", feats[li][0])
        self.last.bn = bn_of[id(feats[li][1])]
        self.last_off = offs[f"features.{li}.0.weight"]
        ci, cm = lins[0]
        if cm.bias is None:
            raise PfrError("HIP MobileNetV2 path: the embedding Linear has a bias")
        self.head_fc = pw(f"classifier.{ci}", cm, bias=True)
        self.head_off = offs[f"classifier.{ci}.weight"]
        self.head_id = id(cm)
        self.emb_dim = self.head_fc.out
        torch.cuda.synchronize(dev)

    def matches(self, model):
        lin = [m for m in model.classifier if isinstance(m, nn.Linear)]
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
        for b in self.blocks:   # [C][9] → [9][C]
            lib.pfr_nchw_to_nhwc(self.master.data_ptr() + 4 * b.dw_off, b.dw_w.data_ptr(), self.did, 1, b.C, 9, 1, b.C, stream)
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

        def act6(z, shape, c):
            """materialised relu6(bn(z))"""
            a = A(shape)
            fwd.append((lib.pfr_bn_act_clamp, (z.data_ptr(), c.scale.data_ptr(), c.shift.data_ptr(), a.data_ptr(), 6.0, did,
                                               shape[0] * shape[1] * shape[2], shape[3])))
            return a

        st = self.stem
        x_nhwc = A((N, H, W, self.cp))
        z0, shape, c0 = conv_bn(x_nhwc, (N, H, W, self.cp), st.w, st.out, 3, 2, 1, st.bn)
        # `cur`: the running tensor; `cur_c`: the BatchNorm + ReLU6 still to be applied to it (None: cur is the activation itself)
        cur, cur_c = z0, c0
        saved = []
        for b in self.blocks:
            sv = _Rec()
            sv.in_raw, sv.in_c, sv.in_shape = cur, cur_c, shape
            # a block without an expand conv leaves the BatchNorm + ReLU6 of its input to the depthwise prologue, unless it adds
            # that input back: the residual operand is the activation itself and has to exist
            if b.expand is not None or b.res or not self.fuse_prologue:
                if cur_c is not None:
                    cur, cur_c = act6(cur, shape, cur_c), None
            sv.xin = cur
            if b.expand is not None:
                sv.ze, eshape, sv.ce = conv_bn(cur, shape, b.expand.w, b.expand.out, 1, 1, 0, b.expand.bn)
                dsrc, dc = sv.ze, sv.ce
                if not self.fuse_prologue:
                    dsrc, dc = act6(sv.ze, eshape, sv.ce), None
            else:
                eshape, dsrc, dc = shape, cur, cur_c
            sv.dsrc, sv.dc, sv.eshape = dsrc, dc, eshape
            Nq, Hq, Wq, Ch = eshape
            OH, OW = (Hq - 1) // b.stride + 1, (Wq - 1) // b.stride + 1
            M = Nq * OH * OW
            sv.zd, sv.dshape = A((Nq, OH, OW, Ch)), (Nq, OH, OW, Ch)
            rpp, nparts, part = 0, 0, None
            if train:
                rpp = lib.pfr_dwconv3_rows_per_part(did, Nq, Hq, Wq, Ch, b.stride)
                nparts = (M + rpp - 1) // rpp
                part = A((nparts, 2, Ch), torch.float32)
            fwd.append((lib.pfr_dwconv3_fwd, (dsrc.data_ptr(), b.dw_w.data_ptr(), sv.zd.data_ptr(), did, Nq, Hq, Wq, Ch, b.stride,
                                              dc.scale.data_ptr() if dc else 0, dc.shift.data_ptr() if dc else 0, 6.0,
                                              part.data_ptr() if train else 0)))
            sv.cd = coef(b.dw_bn)
            bn_fwd(sv.cd, part, nparts, rpp, M)
            sv.ad = act6(sv.zd, sv.dshape, sv.cd)
            sv.zp, pshape, sv.cp = conv_bn(sv.ad, sv.dshape, b.project.w, b.project.out, 1, 1, 0, b.project.bn)
            sv.out = A(pshape)
            fwd.append((lib.pfr_bn_act, (sv.zp.data_ptr(), sv.cp.scale.data_ptr(), sv.cp.shift.data_ptr(), sv.xin.data_ptr() if b.res else 0,
                                         0, 0, sv.out.data_ptr(), did, M, pshape[3], 0)))
            sv.pshape = pshape
            saved.append(sv)
            cur, cur_c, shape = sv.out, None, pshape
        if cur_c is not None:     # (a network without blocks)
            cur, cur_c = act6(cur, shape, cur_c), None
        last_in, last_inshape = cur, shape
        zl, lshape, cl = conv_bn(cur, shape, self.last.w, self.last.out, 1, 1, 0, self.last.bn)
        al = act6(zl, lshape, cl)
        Nn, Hh, Ww, Cf = lshape
        pooled = A((N, Cf))
        fwd.append((lib.pfr_avgpool_fwd, (al.data_ptr(), pooled.data_ptr(), did, N, Hh * Ww, Cf)))
        emb = A((N, self.emb_dim), torch.float32)
        hf = self.head_fc
        fwd.append((lib.pfr_conv2d_fwd, (pooled.data_ptr(), hf.w.data_ptr(), emb.data_ptr(), did, dtype_id(emb.dtype), N, 1, 1, Cf, hf.out,
                                         1, 1, 1, 0, 0, 1, 1, hf.out, hf.bias.data_ptr(), 0, 0, 0, 0, 0, 0, 0)))
        plan.ops = fwd
        plan.meta.update(x_nhwc=x_nhwc, emb=emb, n_fwd=len(fwd))
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
        dzl = bn_bwd(dal, zl, cl, rows_l, "clamp", 6.0)
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
            dzp = bn_bwd(dout, sv.zp, sv.cp, rows_o)
            wgrad(sv.ad, sv.dshape, dzp, sv.pshape, 1, 1, 0, b.project.g)
            dad = G(sv.dshape)
            dgrad_pw(dzp, rows_o, b.project, dad)
            release(dzp)
            # ---- depthwise BN + ReLU6, depthwise conv: weight gradient from the recomputed operand (side), gather data gradient
            dzd = bn_bwd(dad, sv.zd, sv.cd, rows_o, "clamp", 6.0)
            release(dad)
            Ne, He, We, _ = sv.eshape
            npart = lib.pfr_dwconv3_wgrad_parts(did, Ne, He, We, Ch, b.stride)
            dpart = A((npart, 9, Ch), torch.float32)
            dc = sv.dc
            side((SIDE, (lib.pfr_dwconv3_wgrad, (sv.dsrc.data_ptr(), dzd.data_ptr(), dpart.data_ptr(), b.dw_g.data_ptr(), did, Ne, He, We, Ch,
                                                 b.stride, dc.scale.data_ptr() if dc else 0, dc.shift.data_ptr() if dc else 0, 6.0, 0))), dzd)
            dae = G(sv.eshape)
            bwd.append((lib.pfr_dwconv3_dgrad, (dzd.data_ptr(), b.dw_w.data_ptr(), dae.data_ptr(), did, Ne, He, We, Ch, b.stride)))
            release(dzd)
            rows_e = Ne * He * We
            if b.expand is not None:     # (the unfused A/B form materialised the activation: its backward is the same BN + ReLU6 step)
                dze = bn_bwd(dae, sv.ze, sv.ce, rows_e, "clamp", 6.0)
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
            if sv.in_c is not None:     # the block input was relu6(bn(raw)) of the layer before (the stem): its BatchNorm step
                dz = bn_bwd(dout, sv.in_raw, sv.in_c, rows_e, "clamp", 6.0)
                release(dout)
                dout = dz
            if b.stride == 2 and b is not self.blocks[0]:
                mark(b.off)
        if not self.blocks:
            dz = bn_bwd(dout, z0, c0, shape[0] * shape[1] * shape[2], "clamp", 6.0)
            release(dout)
            dout = dz
        # ---- stem (no data gradient)
        wgrad(x_nhwc, (N, H, W, self.cp), dout, (N,) + tuple(z0.shape[1:]), 3, 2, 1, st.g_conv)
        side((SIDE, (lib.pfr_nhwc_to_nchw_f32, (st.g_conv.data_ptr(), st.g.data_ptr(), st.out, st.cin, 9, st.cinp, 0))))
        mark(0, last=True)
        return pb.finish(self)

    def forward(self, x, train, with_backward, ticket=None):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise PfrError(f"expected NCHW input with {self.in_channels} channels, got {tuple(x.shape)}")
        if train and any(d.p > 0 for d in self._dropouts):
            raise PfrError("HIP MobileNetV2 path: Dropout with p > 0 does not run on the device in training mode; use the reference's "
                           "classifier form, `m.classifier = torch.nn.Sequential(torch.nn.Linear(m.last_channel, 512))`, or build the "
                           "model with dropout=0")
        if with_backward and not train:
            raise PfrError("HIP MobileNetV2 path: a backward pass needs training mode (eval-mode BatchNorm has no backward here)")
        x = x.float().contiguous()
        N, _, H, W = x.shape
        emb = self._forward_plan(x, N, H, W, train, with_backward, with_backward=with_backward, ticket=ticket)
        if train:
            self.nbt.add_(1)
        return emb


def mobilenet_forward(model, x):
    """training mode: forward under autograd; eval mode: the inference plan (running statistics, no autograd graph)"""
    if model.training:
        return engine_forward(model, x, True)
    with torch.no_grad():
        return engine_forward(model, x, False)
