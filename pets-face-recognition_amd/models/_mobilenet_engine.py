"""MobileNetV2Engine — executes the MobileNetV2 feature extractor (forward, backward) on the gfx950 kernels.

Same design as models/_convnext_engine.ConvNeXtEngine: flat fp32 master / gradient buffers (the module's nn.Parameters become views,
torchvision's state-dict names unchanged), compute-dtype shadow, activations NHWC end to end, one pre-built plan of C-ABI calls per
input shape; the plan runtime is models/_plan_engine.PlanEngine.  The BatchNorm buffers live in one flat `stats` tensor as in
models/_fe_engine.FEEngine (running_mean / running_var / num_batches_tracked of the modules become views).

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
import struct

import torch
import torch.nn as nn

from .._hip import lib, dtype_id, PfrError
from .._hip.cplan import SIDE, FORK, SREC, WAIT, MWAIT
from ._plan_engine import PlanEngine, Plan, engine_forward, flat_offsets


class _Rec:
    pass


class MobileNetV2Engine(PlanEngine):
    max_plans = 6

    def __init__(self, model, device, compute_dtype=None):
        super().__init__(model, device, compute_dtype)
        self.pool_depth = 48   # see SwinEngine: backward buffers per class before one a side-stream op still reads is re-used
        # False: a materialising pfr_bn_act_clamp before each depthwise conv (tools/mobilenet_bench.py's A/B).  Read when a plan is built
        # and not part of the plan key: set it before the first forward, plans that exist keep the form they were built with
        self.fuse_prologue = True
        self._adopt(model)

    # ------------------------------------------------------------------------------------------ parameters
    def _adopt(self, model):
        from .mobilenet import InvertedResidual
        dev = self.device
        lins = [(i, m) for i, m in enumerate(model.classifier) if not isinstance(m, nn.Dropout)]
        if len(lins) != 1 or not isinstance(lins[0][1], nn.Linear):
            raise PfrError("HIP MobileNetV2 path needs a classifier of exactly one Linear (plus Dropout layers)")
        self._dropouts = [m for m in model.classifier if isinstance(m, nn.Dropout)]
        named = list(model.named_parameters())
        if not all(p.requires_grad for _, p in named):
            raise PfrError("HIP MobileNetV2 path trains every parameter (no frozen layers)")
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

        # BatchNorm buffers → flat (running means, then running variances), as FEEngine
        bns = [(n, m) for n, m in model.named_modules() if isinstance(m, nn.BatchNorm2d)]
        nstat = sum(m.num_features for _, m in bns)
        self.stats = torch.zeros(2 * nstat, dtype=torch.float32, device=dev)
        self.nbt = torch.zeros(len(bns), dtype=torch.int64, device=dev)
        bn_of = {}
        so = 0
        for i, (n, m) in enumerate(bns):
            if m.momentum is None or not m.affine or not m.track_running_stats:
                raise PfrError(f"{n}: the HIP MobileNetV2 path needs an affine BatchNorm2d with running statistics and a momentum")
            C = m.num_features
            b = _Rec()
            b.C, b.eps, b.momentum = C, float(m.eps), float(m.momentum)
            b.rm, b.rv = self.stats[so:so + C], self.stats[nstat + so:nstat + so + C]
            b.rm.copy_(m.running_mean.detach().to(dev))
            b.rv.copy_(m.running_var.detach().to(dev))
            self.nbt[i] = int(m.num_batches_tracked.item())
            m.running_mean, m.running_var, m.num_batches_tracked = b.rm, b.rv, self.nbt[i]
            so += C
            ow, ob = offs[n + ".weight"], offs[n + ".bias"]
            b.gamma, b.dgamma = self.master[ow:ow + C], self.grad[ow:ow + C]
            b.beta, b.dbeta = self.master[ob:ob + C], self.grad[ob:ob + C]
            bn_of[id(m)] = b
        maxc = max(m.num_features for _, m in bns)
        self.bn_ws = torch.empty(max(1, lib.pfr_bn_finalize_ws_floats(1 << 20, maxc)), dtype=torch.float32, device=dev)

        def chunked(name, c):
            if c % self.kp:
                raise PfrError(f"HIP MobileNetV2 path: {name} has {c} channels, not a multiple of {self.kp} in {self.dtype}")

        def pw(prefix, m, bias=False):
            """1x1 convolution / Linear: the [O][I](x1x1) parameter is the kernel's [O][1][1][I] layout as it stands"""
            r = _Rec()
            r.out, r.inp = m.weight.shape[0], m.weight.shape[1]
            chunked(prefix, r.inp)
            chunked(prefix, r.out)
            r.off = offs[prefix + ".weight"]
            n = r.out * r.inp
            r.w, r.g = self.shadow[r.off:r.off + n], self.grad[r.off:r.off + n]
            r.wt = torch.zeros(n, dtype=self.dtype, device=dev)     # [I][1][1][O]
            if bias:
                bo = offs[prefix + ".bias"]
                r.bias, r.dbias = self.master[bo:bo + r.out], self.grad[bo:bo + r.out]
            return r

        def plain(m, k, stride, groups):
            return (m.kernel_size == (k, k) and m.stride == (stride, stride) and m.padding == ((k - 1) // 2,) * 2 and m.groups == groups
                    and m.dilation == (1, 1) and m.bias is None)

        feats = model.features
        # stem: [O][3][3][3] parameter ↔ [O][9][I padded] conv layout
        sc = feats[0][0]
        if not plain(sc, 3, 2, 1):
            raise PfrError("HIP MobileNetV2 path: the stem is a bias-free 3x3 stride-2 convolution")
        st = _Rec()
        st.out, st.cin = sc.out_channels, sc.in_channels
        chunked("features.0.0", st.out)
        st.cinp = (st.cin + self.kp - 1) // self.kp * self.kp
        st.off = offs["features.0.0.weight"]
        st.g = self.grad[st.off:st.off + st.out * st.cin * 9]
        st.w = torch.zeros(st.out * 9 * st.cinp, dtype=self.dtype, device=dev)
        st.g_conv = torch.zeros(st.out * 9 * st.cinp, dtype=torch.float32, device=dev)
        st.bn = bn_of[id(feats[0][1])]
        self.stem = st
        self.in_channels, self.cp = st.cin, st.cinp
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
            chunked(f"features.{fi}.conv.{j}.0", b.C)
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
        fwd, bwd = [], []

        def A(shape, dtype=None):
            return plan.keep(torch.empty(shape, dtype=dtype or T, device=dev))

        def coef(bn):
            """this plan's (mean, invstd, scale, shift) and backward coefficients of a BatchNorm"""
            c = _Rec()
            c.bn = bn
            c.f = plan.keep(torch.zeros((4, bn.C), dtype=torch.float32, device=dev))
            c.b = plan.keep(torch.zeros((3, bn.C), dtype=torch.float32, device=dev))
            c.scale, c.shift = c.f[2], c.f[3]
            return c

        def bn_fwd(c, part, nparts, rpp, count):
            bn = c.bn
            if train:
                nws = lib.pfr_bn_finalize_ws_floats(nparts, bn.C)
                assert nws <= self.bn_ws.numel()
                fwd.append((lib.pfr_bn_finalize, (part.data_ptr(), nparts, rpp, bn.C, float(count), bn.gamma.data_ptr(), bn.beta.data_ptr(),
                                                  bn.eps, bn.momentum, bn.rm.data_ptr(), bn.rv.data_ptr(), c.f[0].data_ptr(),
                                                  c.f[1].data_ptr(), c.f[2].data_ptr(), c.f[3].data_ptr(),
                                                  self.bn_ws.data_ptr() if nws else 0)))
            else:
                fwd.append((lib.pfr_bn_eval_coeff, (bn.C, bn.gamma.data_ptr(), bn.beta.data_ptr(), bn.rm.data_ptr(), bn.rv.data_ptr(),
                                                    bn.eps, c.f[2].data_ptr(), c.f[3].data_ptr())))

        def conv_bn(x, xshape, w, cout, R, stride, pad, bn):
            """dense convolution + the BatchNorm coefficients of its output → (raw output, its shape, coefficients)"""
            Nq, Hq, Wq, Cq = xshape
            OH, OW = (Hq + 2 * pad - R) // stride + 1, (Wq + 2 * pad - R) // stride + 1
            M = Nq * OH * OW
            z = A((Nq, OH, OW, cout))
            part, nt, mt = None, 0, 0
            if train:
                mt = lib.pfr_conv2d_mtile(Nq, Hq, Wq, Cq, cout, R, R, stride, pad, OH, OW, did, did, 0)
                nt = (M + mt - 1) // mt
                part = A((nt, 2, cout), torch.float32)
            fwd.append((lib.pfr_conv2d_fwd, (x.data_ptr(), w.data_ptr(), z.data_ptr(), did, did, Nq, Hq, Wq, Cq, cout, R, R, stride, pad, 0,
                                             OH, OW, cout, 0, 0, 0, 0, 0, 0, 0, part.data_ptr() if train else 0)))
            c = coef(bn)
            bn_fwd(c, part, nt, mt, M)
            return z, (Nq, OH, OW, cout), c

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

        # ================================================================= backward
        # Weight gradients (dense and depthwise) and the bias column sum feed nothing before the optimizer: they run on the SIDE stream
        # with the FORK / SREC / WAIT roles of _hip/cplan.py, exactly as in ConvNeXtEngine.build_plan (see the comments there).
        pool = {}
        nalloc = {}
        pending = {}      # data_ptr of a pooled buffer -> last side op that reads it
        side_reads = []   # (k, data_ptr) of every side-op input
        nside = [0]
        ws_need = [0]

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

        def side(op, *reads):
            if bwd and bwd[-1][0] == SREC:
                k = bwd.pop()[1]
            else:
                k = nside[0]
                nside[0] += 1
                bwd.append((FORK, k))
            bwd.append(op)
            bwd.append((SREC, k))
            for r in reads:
                side_reads.append((k, r.data_ptr()))

        def wgrad(x, xshape, dy, dyshape, R, stride, pad, out):
            Nq, Hq, Wq, Cq = xshape
            _, OH, OW, Co = dyshape
            KK = R * R * Cq
            splits = lib.pfr_conv2d_wgrad_splits(Nq * OH * OW, Co, KK)
            ws_need[0] = max(ws_need[0], splits * Co * KK)
            side(("wgrad", (x.data_ptr(), dy.data_ptr(), out.data_ptr(), None, did, Nq, Hq, Wq, Cq, Co, R, R, stride, pad, OH, OW, Co,
                            0, 0, 0, 1.0, 0)), dy)

        def dgrad_pw(dy, rows, r, dx, residual=None):
            bwd.append((lib.pfr_conv2d_fwd, (dy.data_ptr(), r.wt.data_ptr(), dx.data_ptr(), did, did, rows, 1, 1, r.out, r.inp, 1, 1, 1, 0, 0,
                                             1, 1, r.inp, 0, 0 if residual is None else residual.data_ptr(), 0, 0, 0, 0, 0, 0)))

        def bn_bwd(dout, z, c, rows, relu6):
            """dz of z from the gradient of relu6?(bn(z)), in place of a fresh buffer; dgamma / dbeta into the flat gradient"""
            bn = c.bn
            nb = lib.pfr_colreduce_blocks(bn.C, did, rows)
            part = A((nb, 2, bn.C), torch.float32)
            mode, hi = (2, 6.0) if relu6 else (0, 0.0)
            bwd.append((lib.pfr_bn_bwd_reduce_clamp, (dout.data_ptr(), z.data_ptr(), c.f[0].data_ptr(), c.f[1].data_ptr(), c.scale.data_ptr(),
                                                      c.shift.data_ptr(), hi, mode, did, rows, bn.C, part.data_ptr())))
            bwd.append((lib.pfr_bn_bwd_finalize, (part.data_ptr(), nb, bn.C, float(rows), bn.gamma.data_ptr(), c.f[0].data_ptr(),
                                                  c.f[1].data_ptr(), bn.dgamma.data_ptr(), bn.dbeta.data_ptr(), c.b.data_ptr(), 0)))
            dz = G(tuple(z.shape))
            bwd.append((lib.pfr_bn_bwd_apply_clamp, (dout.data_ptr(), z.data_ptr(), c.b.data_ptr(), c.scale.data_ptr(), c.shift.data_ptr(),
                                                     hi, mode, dz.data_ptr(), did, rows, bn.C)))
            return dz

        def stop(final, off):
            bwd.append((WAIT if final else MWAIT, nside[0] - 1))
            bwd.append((None, (off,)))

        demb = A((N, self.emb_dim))
        plan.meta["demb"] = demb
        side((SIDE, (lib.pfr_colsum, (demb.data_ptr(), did, N, hf.out, hf.dbias.data_ptr(), 0, 0))), demb)
        wgrad(pooled, (N, 1, 1, Cf), demb, (N, 1, 1, hf.out), 1, 1, 0, hf.g)
        dpooled = G((N, Cf))
        dgrad_pw(demb, N, hf, dpooled)
        dal = G(lshape)
        bwd.append((lib.pfr_avgpool_bwd, (dpooled.data_ptr(), dal.data_ptr(), did, N, Hh * Ww, Cf)))
        release(dpooled)
        stop(False, self.head_off)
        rows_l = N * Hh * Ww
        dzl = bn_bwd(dal, zl, cl, rows_l, True)
        release(dal)
        wgrad(last_in, last_inshape, dzl, lshape, 1, 1, 0, self.last.g)
        dout = G(last_inshape)
        dgrad_pw(dzl, rows_l, self.last, dout)
        release(dzl)
        stop(False, self.last_off)
        for b, sv in zip(reversed(self.blocks), reversed(saved)):
            Nq, OH, OW, Ch = sv.dshape
            rows_o = Nq * OH * OW
            # ---- project BN (linear) and conv
            dzp = bn_bwd(dout, sv.zp, sv.cp, rows_o, False)
            wgrad(sv.ad, sv.dshape, dzp, sv.pshape, 1, 1, 0, b.project.g)
            dad = G(sv.dshape)
            dgrad_pw(dzp, rows_o, b.project, dad)
            release(dzp)
            # ---- depthwise BN + ReLU6, depthwise conv: weight gradient from the recomputed operand (side), gather data gradient
            dzd = bn_bwd(dad, sv.zd, sv.cd, rows_o, True)
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
                dze = bn_bwd(dae, sv.ze, sv.ce, rows_e, True)
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
                dz = bn_bwd(dout, sv.in_raw, sv.in_c, rows_e, True)
                release(dout)
                dout = dz
            if b.stride == 2 and b is not self.blocks[0]:
                stop(False, b.off)
        if not self.blocks:
            dz = bn_bwd(dout, z0, c0, shape[0] * shape[1] * shape[2], True)
            release(dout)
            dout = dz
        # ---- stem (no data gradient)
        wgrad(x_nhwc, (N, H, W, self.cp), dout, (N,) + tuple(z0.shape[1:]), 3, 2, 1, st.g_conv)
        side((SIDE, (lib.pfr_nhwc_to_nchw_f32, (st.g_conv.data_ptr(), st.g.data_ptr(), st.out, st.cin, 9, st.cinp, 0))))
        stop(True, 0)
        plan.meta["n_side"] = nside[0]
        if self.ws is None or self.ws.numel() < ws_need[0]:
            self.ws = torch.empty(ws_need[0], dtype=torch.float32, device=dev)
        plan.ops = fwd + bwd
        return plan

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
        plan = self.acquire_plan(N, H, W, train, with_backward, ticket=ticket if with_backward else None)
        if with_backward:
            self._fresh(plan)
        stream = torch.cuda.current_stream().cuda_stream
        self.refresh_weights(stream, for_backward=with_backward)
        lib.pfr_nchw_to_nhwc(x.data_ptr(), plan.meta["x_nhwc"].data_ptr(), self.did, N, x.shape[1], H, W, self.cp, stream)
        self._run_fwd(plan, stream)
        if train:
            self.nbt.add_(1)
        self._last_plan = plan
        return plan.meta["emb"]

    def backward(self, demb, plan=None):
        plan = plan if plan is not None else self._last_plan
        self._begin_backward(plan, demb)
        # As in ConvNeXtEngine: the plan's gradient launches overwrite their slices; a second backward before zero_grad sets the
        # previous sum aside and adds it back (the accumulate forms of pfr_dwconv3_wgrad / pfr_bn_bwd_finalize serve hosts without it)
        prev = self.grad.clone() if self.first_param.grad is not None else None
        hook = self.grad_ready_hook
        if prev is not None or any(self._plan_busy(q) for q in self.plans.values()):
            hook = None
        self._run_bwd(plan, "bwd", hook, hook)
        if prev is not None:
            self.grad.add_(prev)
        self.attach_grads()


def mobilenet_forward(model, x):
    """training mode: forward under autograd; eval mode: the inference plan (running statistics, no autograd graph)"""
    if model.training:
        return engine_forward(model, x, True)
    with torch.no_grad():
        return engine_forward(model, x, False)
