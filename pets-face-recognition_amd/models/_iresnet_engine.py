"""IResNetEngine — executes the IResNet feature extractor (forward, backward) on the gfx950 kernels.

Same design as models/_mobilenet_engine.MobileNetV2Engine: flat fp32 master / gradient buffers (the module's nn.Parameters become
views, the insightface state-dict names unchanged), compute-dtype shadow, activations NHWC end to end, one pre-built plan of C-ABI
calls per input shape through models/_plan_engine.PlanBuilder and models/_plan_layers.BatchNormLayers, BatchNorm buffers in one flat
`stats` tensor.  `features.weight` (frozen at 1 by the model) is not adopted: the engine reads it where it stands.

Mapping (models/iresnet.py):
  stem 3x3 stride 1, conv1 / conv2 3x3, 1x1 shortcut → pfr_conv2d_fwd with the BatchNorm partials in its epilogue (stats_part), pfr_conv2d_wgrad,
                                                    the data gradient pfr_conv2d_fwd over the pfr_weight_dgrad_layout weights
  stem bn1 + PReLU, block bn2 + PReLU              → pfr_bn_act_prelu (materialised); backward pfr_bn_bwd_reduce_prelu / pfr_bn_bwd_finalize /
                                                    pfr_prelu_slope_finalize / pfr_bn_bwd_apply_prelu, the mask recomputed from the conv output
  block bn1 (on the block input)                   → pfr_bn_stats + pfr_bn_finalize, pfr_bn_act(relu = 0) MATERIALISED: conv1 pads the
                                                    normalised tensor with zeros, which a BatchNorm prologue of the convolution (padding
                                                    the raw tensor, i.e. shift[c] after the affine map) would not reproduce
  bn3(conv2) + shortcut, no activation             → pfr_bn_act(relu = 0) with the second operand: the block input, or bn_d(conv_d(x))
  neck bn2 → flatten → fc → features               → pfr_bn_act(relu = 0), a 1x1 convolution over [N][1][1][s*s*512] whose weight copy is
                                                    permuted to the NHWC flatten order ([F][C][s*s] → [F][s*s][C]), BatchNorm over the
                                                    [N][F] fp32 rows (pfr_bn_stats / pfr_bn_finalize, rows = N)
"""
import torch
import torch.nn as nn

from .._hip import lib, dtype_id, PfrError, PFR_F32
from .._hip.cplan import SIDE
from ._plan_engine import PlanEngine, PlanBuilder, Plan, engine_forward
from ._plan_layers import BatchNormLayers


class _Rec:
    pass


class IResNetEngine(PlanEngine):
    max_plans = 6

    def __init__(self, model, device, compute_dtype=None):
        super().__init__(model, device, compute_dtype)
        self._adopt(model)

    # ------------------------------------------------------------------------------------------ parameters
    def _adopt(self, model):
        from .iresnet import IBasicBlock
        dev, what = self.device, "IResNet"
        named = []
        for n, p in model.named_parameters():
            if p.requires_grad:
                named.append((n, p))
            elif n == "features.weight":
                p.data = p.data.to(dev).float().contiguous()      # read where it stands (1.0, or what a checkpoint holds)
            else:
                raise PfrError(f"HIP IResNet path trains every parameter but features.weight ({n} is frozen)")
        if not isinstance(model.features, nn.BatchNorm1d) or model.features.weight.requires_grad:
            raise PfrError("HIP IResNet path: `features` is a BatchNorm1d whose weight is frozen")
        offs = self._adopt_flat(named)
        bn_of = self._adopt_batchnorms(model, what, kinds=(nn.BatchNorm2d, nn.BatchNorm1d))
        self._dropout = model.dropout
        self.input_size = int(model.input_size)
        self._adopt_stem(what, model.conv1, bn_of[id(model.bn1)], stride=1, name="conv1")
        self.stem_slope = self._slope("prelu", model.prelu, self.stem.out)
        self.blocks = []
        for li in range(1, 5):
            for bi, blk in enumerate(getattr(model, f"layer{li}")):
                pre = f"layer{li}.{bi}"
                if not isinstance(blk, IBasicBlock):
                    raise PfrError(f"{pre}: the HIP IResNet path expects IBasicBlock blocks")
                b = _Rec()
                b.off = offs[pre + ".bn1.weight"]
                b.first = bi == 0
                b.stride = blk.conv2.stride[0]
                b.conv1 = self._conv3(what, pre + ".conv1", blk.conv1, 1)
                b.conv2 = self._conv3(what, pre + ".conv2", blk.conv2, b.stride)
                b.bn1, b.bn2, b.bn3 = bn_of[id(blk.bn1)], bn_of[id(blk.bn2)], bn_of[id(blk.bn3)]
                b.slope = self._slope(pre + ".prelu", blk.prelu, b.conv1.out)
                b.down = None
                if blk.downsample is not None:
                    dc, dbn = blk.downsample[0], blk.downsample[1]
                    if not self._plain(dc, 1, b.stride, 1) or not isinstance(dbn, nn.BatchNorm2d):
                        raise PfrError(f"{pre}: the shortcut is a bias-free 1x1 convolution of the block's stride and a BatchNorm2d")
                    b.down = self._pw(what, pre + ".downsample.0", dc)
                    b.down.bn = bn_of[id(dbn)]
                elif b.stride != 1 or b.conv1.cin != b.conv2.out:
                    raise PfrError(f"{pre}: a block that changes the shape needs a downsample branch")
                self.blocks.append(b)
        self.neck_bn = bn_of[id(model.bn2)]
        fm = model.fc
        if fm.bias is None:
            raise PfrError("HIP IResNet path: the embedding Linear has a bias")
        C = self.blocks[-1].conv2.out
        fc = _Rec()
        fc.out, fc.inp, fc.C = fm.out_features, fm.in_features, C
        if fc.inp % C:
            raise PfrError(f"HIP IResNet path: fc.in_features {fc.inp} is not a multiple of the {C} channels of layer4")
        fc.hw = fc.inp // C
        self._chunked(what, "fc", fc.out)
        fc.off = offs["fc.weight"]
        n = fc.out * fc.inp
        fc.g = self.grad[fc.off:fc.off + n]
        fc.w = torch.zeros(n, dtype=self.dtype, device=dev)          # [F][s*s][C]: the NHWC flatten order
        fc.wt = torch.zeros(n, dtype=self.dtype, device=dev)         # [s*s*C][F]
        fc.g_conv = torch.zeros(n, dtype=torch.float32, device=dev)
        bo = offs["fc.bias"]
        fc.bias, fc.dbias = self.master[bo:bo + fc.out], self.grad[bo:bo + fc.out]
        self.fc = fc
        self.feat_bn = bn_of[id(model.features)]
        self.emb_dim = fc.out
        torch.cuda.synchronize(dev)

    def _slope(self, prefix, m, C):
        if not isinstance(m, nn.PReLU) or m.weight.numel() != C:
            raise PfrError(f"{prefix}: the HIP IResNet path expects nn.PReLU({C}), one slope per channel")
        s = _Rec()
        o = self.offs[prefix + ".weight"]
        s.w, s.g = self.master[o:o + C], self.grad[o:o + C]
        return s

    def _conv3(self, what, prefix, m, stride):
        """bias-free 3x3 convolution, padding 1: [O][I][3][3] parameter ↔ [O][9][I] conv layout (weights and gradient)"""
        if not self._plain(m, 3, stride, 1) or stride not in (1, 2):
            raise PfrError(f"{prefix}: the HIP {what} path expects a bias-free 3x3 convolution, padding 1, stride {stride}")
        c = _Rec()
        c.out, c.cin = m.out_channels, m.in_channels
        self._chunked(what, prefix, c.out)
        self._chunked(what, prefix, c.cin)
        c.off = self.offs[prefix + ".weight"]
        n = c.out * c.cin * 9
        c.g = self.grad[c.off:c.off + n]
        c.w = torch.zeros(n, dtype=self.dtype, device=self.device)
        c.wt = torch.zeros(n, dtype=self.dtype, device=self.device)     # [I][9 flipped][O]
        c.g_conv = torch.zeros(n, dtype=torch.float32, device=self.device)
        return c

    def _conv3s(self):
        for b in self.blocks:
            yield b.conv1
            yield b.conv2

    def refresh_weights(self, stream, for_backward=True):
        """compute-dtype shadow and the conv layouts of the 3x3 weights and of fc.weight from the fp32 master — on every forward pass,
        so an optimizer step, swap_averaged() or a loaded checkpoint needs no call of its own"""
        mp = self.master.data_ptr()
        if self.dtype != torch.float32:
            lib.pfr_cast(mp, 0, self.shadow.data_ptr(), self.did, self.n_flat, stream)
        st = self.stem     # [O][I][9] → [O][9][I padded]
        lib.pfr_nchw_to_nhwc(mp + 4 * st.off, st.w.data_ptr(), self.did, st.out, st.cin, 9, 1, st.cinp, stream)
        for c in self._conv3s():
            lib.pfr_nchw_to_nhwc(mp + 4 * c.off, c.w.data_ptr(), self.did, c.out, c.cin, 9, 1, c.cin, stream)
        fc = self.fc       # [F][C][s*s] → [F][s*s][C]
        lib.pfr_nchw_to_nhwc(mp + 4 * fc.off, fc.w.data_ptr(), self.did, fc.out, fc.C, fc.hw, 1, fc.C, stream)
        if for_backward:
            self._refresh_dgrad_layouts(stream)

    def _wt_records(self):
        for c in self._conv3s():
            yield (c.w.data_ptr(), c.wt.data_ptr(), c.out, 3, 3, c.cin)
        for b in self.blocks:
            if b.down is not None:
                yield (b.down.w.data_ptr(), b.down.wt.data_ptr(), b.down.out, 1, 1, b.down.inp)
        yield (self.fc.w.data_ptr(), self.fc.wt.data_ptr(), self.fc.out, 1, 1, self.fc.inp)

    # ------------------------------------------------------------------------------------------ plan
    def build_plan(self, N, H, W, train, with_backward):
        T, dev, did = self.dtype, self.device, self.did
        plan = Plan()
        pb = PlanBuilder(plan, T, dev, did, self.pool_depth)
        A, fwd, bwd = pb.A, pb.fwd, pb.bwd
        bn = BatchNormLayers(pb, train, self.bn_ws)
        coef, bn_fwd, conv_bn = bn.coef, bn.bn_fwd, bn.conv_bn

        def prelu_act(z, shape, c, slope):
            """materialised prelu(bn(z))"""
            a = A(shape)
            fwd.append((lib.pfr_bn_act_prelu, (z.data_ptr(), c.scale.data_ptr(), c.shift.data_ptr(), slope.w.data_ptr(), a.data_ptr(), did,
                                               shape[0] * shape[1] * shape[2], shape[3])))
            return a

        def bn_of_tensor(x, rows, C, rec, dt=did, out_dtype=None):
            """BatchNorm (no activation) of a stored tensor: statistics of x itself in training mode → (materialised output, coefficients)"""
            c = coef(rec)
            part, nb, rpp = None, 0, 0
            if train:
                nb = lib.pfr_colreduce_blocks(C, dt, rows)
                rpp = lib.pfr_bn_stats_rows_per_part(C, dt, rows)
                part = A((nb, 2, C), torch.float32)
                fwd.append((lib.pfr_bn_stats, (x.data_ptr(), dt, rows, C, part.data_ptr())))
            bn_fwd(c, part, nb, rpp, rows)
            y = A(tuple(x.shape), out_dtype)
            fwd.append((lib.pfr_bn_act, (x.data_ptr(), c.scale.data_ptr(), c.shift.data_ptr(), 0, 0, 0, y.data_ptr(), dt, rows, C, 0)))
            return y, c

        st = self.stem
        x_nhwc = A((N, H, W, self.cp))
        z0, shape, c0 = conv_bn(x_nhwc, (N, H, W, self.cp), st.w, st.out, 3, 1, 1, st.bn)
        cur = prelu_act(z0, shape, c0, self.stem_slope)
        saved = []
        for b in self.blocks:
            sv = _Rec()
            sv.xin, sv.in_shape = cur, shape
            rows_in = shape[0] * shape[1] * shape[2]
            sv.a1, sv.c1 = bn_of_tensor(cur, rows_in, shape[3], b.bn1)
            sv.z1, sv.s1, sv.c2 = conv_bn(sv.a1, shape, b.conv1.w, b.conv1.out, 3, 1, 1, b.bn2)
            sv.a2 = prelu_act(sv.z1, sv.s1, sv.c2, b.slope)
            sv.z2, sv.s2, sv.c3 = conv_bn(sv.a2, sv.s1, b.conv2.w, b.conv2.out, 3, b.stride, 1, b.bn3)
            M = sv.s2[0] * sv.s2[1] * sv.s2[2]
            sv.out = A(sv.s2)
            if b.down is not None:
                sv.zd, dshape, sv.cd = conv_bn(cur, shape, b.down.w, b.down.out, 1, b.stride, 0, b.down.bn)
                assert dshape == sv.s2
                fwd.append((lib.pfr_bn_act, (sv.z2.data_ptr(), sv.c3.scale.data_ptr(), sv.c3.shift.data_ptr(), sv.zd.data_ptr(),
                                             sv.cd.scale.data_ptr(), sv.cd.shift.data_ptr(), sv.out.data_ptr(), did, M, sv.s2[3], 0)))
            else:
                fwd.append((lib.pfr_bn_act, (sv.z2.data_ptr(), sv.c3.scale.data_ptr(), sv.c3.shift.data_ptr(), cur.data_ptr(), 0, 0,
                                             sv.out.data_ptr(), did, M, sv.s2[3], 0)))
            saved.append(sv)
            cur, shape = sv.out, sv.s2
        fc = self.fc
        Nn, Hh, Ww, Cf = shape
        if Hh * Ww != fc.hw or Cf != fc.C:
            raise PfrError(f"HIP IResNet path: layer4 leaves a {Hh}x{Ww}x{Cf} map, fc expects {fc.hw} pixels of {fc.C} channels")
        rows_n = N * Hh * Ww
        neck_in = cur
        an, cn = bn_of_tensor(cur, rows_n, Cf, self.neck_bn)
        zf = A((N, fc.out), torch.float32)
        fwd.append((lib.pfr_conv2d_fwd, (an.data_ptr(), fc.w.data_ptr(), zf.data_ptr(), did, PFR_F32, N, 1, 1, fc.inp, fc.out,
                                         1, 1, 1, 0, 0, 1, 1, fc.out, fc.bias.data_ptr(), 0, 0, 0, 0, 0, 0, 0)))
        emb, cf = bn_of_tensor(zf, N, fc.out, self.feat_bn, dt=PFR_F32, out_dtype=torch.float32)
        plan.ops = fwd
        plan.meta.update(x_nhwc=x_nhwc, emb=emb, n_fwd=len(fwd))
        if not with_backward:
            return plan

        # ================================================================= backward (stream roles, buffer pool: PlanBuilder)
        G, release, side, wgrad, mark = pb.G, pb.release, pb.side, pb.wgrad, pb.mark
        dgrad_pw, bn_bwd = bn.dgrad_pw, bn.bn_bwd

        def dgrad(dy, dyshape, cout, wt, cin, R, stride, dx, dxshape, accumulate=0):
            """data gradient of a padding-(R // 2) convolution: pfr_conv2d_fwd over dy, dilated by the stride, with the flipped weights"""
            Nq, OH, OW, _ = dyshape
            bwd.append((lib.pfr_conv2d_fwd, (dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), did, did, Nq, OH, OW, cout, cin, R, R, 1,
                                             R - 1 - R // 2, {1: 0, 2: 1}[stride], dxshape[1], dxshape[2], cin, 0, 0, accumulate, 0, 0, 0, 0, 0)))

        def wgrad3(x, xshape, dy, dyshape, stride, c):
            wgrad(x, xshape, dy, dyshape, 3, stride, 1, c.g_conv)
            side((SIDE, (lib.pfr_nhwc_to_nchw_f32, (c.g_conv.data_ptr(), c.g.data_ptr(), c.out, c.cin, 9, c.cin, 0))))

        # ---- features: BatchNorm over the fp32 [N][F] rows (its weight is frozen: dgamma goes to scratch), then fc
        demb = A((N, fc.out))
        plan.meta["demb"] = demb
        F = fc.out
        demb32, dzf32, dzf = A((N, F), torch.float32), A((N, F), torch.float32), A((N, F))
        fb = self.feat_bn
        nbf = lib.pfr_colreduce_blocks(F, PFR_F32, N)
        partf = A((nbf, 2, F), torch.float32)
        bwd.append((lib.pfr_cast, (demb.data_ptr(), did, demb32.data_ptr(), PFR_F32, N * F)))
        bwd.append((lib.pfr_bn_bwd_reduce_clamp, (demb32.data_ptr(), zf.data_ptr(), cf.f[0].data_ptr(), cf.f[1].data_ptr(), cf.scale.data_ptr(),
                                                  cf.shift.data_ptr(), 0.0, 0, PFR_F32, N, F, partf.data_ptr())))
        bwd.append((lib.pfr_bn_bwd_finalize, (partf.data_ptr(), nbf, F, float(N), fb.gamma.data_ptr(), cf.f[0].data_ptr(), cf.f[1].data_ptr(),
                                              fb.dgamma.data_ptr(), fb.dbeta.data_ptr(), cf.b.data_ptr(), 0)))
        bwd.append((lib.pfr_bn_bwd_apply_clamp, (demb32.data_ptr(), zf.data_ptr(), cf.b.data_ptr(), cf.scale.data_ptr(), cf.shift.data_ptr(),
                                                 0.0, 0, dzf32.data_ptr(), PFR_F32, N, F)))
        bwd.append((lib.pfr_cast, (dzf32.data_ptr(), PFR_F32, dzf.data_ptr(), did, N * F)))
        side((SIDE, (lib.pfr_colsum, (dzf.data_ptr(), did, N, F, fc.dbias.data_ptr(), 0, 0))), dzf)
        wgrad(an, (N, 1, 1, fc.inp), dzf, (N, 1, 1, F), 1, 1, 0, fc.g_conv)
        side((SIDE, (lib.pfr_nhwc_to_nchw_f32, (fc.g_conv.data_ptr(), fc.g.data_ptr(), F, fc.C, fc.hw, fc.C, 0))))
        dan = G(shape)
        dgrad_pw(dzf, N, fc, dan)
        mark(fc.off)
        dout = bn_bwd(dan, neck_in, cn, rows_n)
        release(dan)
        for b, sv in zip(reversed(self.blocks), reversed(saved)):
            s1, s2, sin = sv.s1, sv.s2, sv.in_shape
            rows_o, rows_1, rows_in = s2[0] * s2[1] * s2[2], s1[0] * s1[1] * s1[2], sin[0] * sin[1] * sin[2]
            # ---- the block output gradient feeds bn3 and the shortcut's BatchNorm, both linear
            dz2 = bn_bwd(dout, sv.z2, sv.c3, rows_o)
            dzd = bn_bwd(dout, sv.zd, sv.cd, rows_o) if b.down is not None else None
            wgrad3(sv.a2, s1, dz2, s2, b.stride, b.conv2)
            da2 = G(s1)
            dgrad(dz2, s2, b.conv2.out, b.conv2.wt, b.conv2.cin, 3, b.stride, da2, s1)
            release(dz2)
            dz1 = bn_bwd(da2, sv.z1, sv.c2, rows_1, "prelu", slope=b.slope)
            release(da2)
            wgrad3(sv.a1, sin, dz1, s1, 1, b.conv1)
            da1 = G(sin)
            dgrad(dz1, s1, b.conv1.out, b.conv1.wt, b.conv1.cin, 3, 1, da1, sin)
            release(dz1)
            dxin = bn_bwd(da1, sv.xin, sv.c1, rows_in)
            release(da1)
            if b.down is not None:     # the main branch wrote all of dxin; the strided 1x1 shortcut adds at the pixels it read
                wgrad(sv.xin, sin, dzd, s2, 1, b.stride, 0, b.down.g)
                dgrad(dzd, s2, b.down.out, b.down.wt, b.down.inp, 1, b.stride, dxin, sin, accumulate=1)
                release(dzd)
            else:
                bwd.append((lib.pfr_add, (dxin.data_ptr(), dout.data_ptr(), dxin.data_ptr(), did, rows_in * sin[3])))
            release(dout)
            dout = dxin
            if b.first and b is not self.blocks[0]:
                mark(b.off)
        # ---- stem (no data gradient)
        s0 = (N,) + tuple(z0.shape[1:])
        dz0 = bn_bwd(dout, z0, c0, s0[0] * s0[1] * s0[2], "prelu", slope=self.stem_slope)
        release(dout)
        wgrad(x_nhwc, (N, H, W, self.cp), dz0, s0, 3, 1, 1, st.g_conv)
        side((SIDE, (lib.pfr_nhwc_to_nchw_f32, (st.g_conv.data_ptr(), st.g.data_ptr(), st.out, st.cin, 9, st.cinp, 0))))
        mark(0, last=True)
        return pb.finish(self)

    def forward(self, x, train, with_backward, ticket=None):
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise PfrError(f"expected NCHW input with {self.in_channels} channels, got {tuple(x.shape)}")
        if x.shape[2] != self.input_size or x.shape[3] != self.input_size:
            raise PfrError(f"HIP IResNet path: the model was built for {self.input_size}x{self.input_size} input (fc.in_features depends "
                           f"on it), got {x.shape[2]}x{x.shape[3]}; build it with input_size={x.shape[2]}")
        if train and self._dropout.p > 0:
            raise PfrError("HIP IResNet path: Dropout with p > 0 does not run on the device in training mode; build the model with "
                           "dropout=0 (the default), or set model.dropout.p = 0")
        if with_backward and not train:
            raise PfrError("HIP IResNet path: a backward pass needs training mode (eval-mode BatchNorm has no backward here)")
        x = x.float().contiguous()
        N, _, H, W = x.shape
        emb = self._forward_plan(x, N, H, W, train, with_backward, with_backward=with_backward, ticket=ticket)
        if train:
            self.nbt.add_(1)
        return emb


def iresnet_forward(model, x):
    """training mode: forward under autograd; eval mode: the inference plan (running statistics, no autograd graph)"""
    if model.training:
        return engine_forward(model, x, True)
    with torch.no_grad():
        return engine_forward(model, x, False)
