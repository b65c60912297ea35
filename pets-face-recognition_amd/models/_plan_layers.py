"""Layer emitters on a models/_plan_engine.PlanBuilder `pb`: the launches of one layer appended to pb.fwd or pb.bwd.

  Linear / LayerNorm family (Swin, ConvNeXt, ViT): gemm, dgrad_lin, ln_fwd, ln_bwd, bias_grad
  BatchNorm family (MobileNetV2, EfficientNet, IResNet):    BatchNormLayers — coef, bn_fwd, conv_bn, dgrad_pw, bn_bwd

A Linear record `r` has out, inp, w ([out][in]), wt ([in][out]) and bias (or None); a LayerNorm record gamma, beta, dgamma, dbeta,
eps; a BatchNorm record is what PlanEngine._adopt_batchnorms returns."""
import torch

from .._hip import lib, dtype_id
from .._hip.cplan import SIDE
from ._plan_engine import _Rec


# ---------------------------------------------------------------------------------------------- Linear / LayerNorm
def gemm(pb, x, rows, cin, r, y, residual=None):
    """y = x · r.wᵀ (+ bias) (+ residual): the GEMM as a 1x1 convolution, bias and residual-add in its epilogue"""
    pb.fwd.append((lib.pfr_conv2d_fwd, (x.data_ptr(), r.w.data_ptr(), y.data_ptr(), pb.did, dtype_id(y.dtype), rows, 1, 1, cin, r.out,
                                        1, 1, 1, 0, 0, 1, 1, r.out, r.bias.data_ptr() if r.bias is not None else 0,
                                        0 if residual is None else residual.data_ptr(), 0, 0, 0, 0, 0, 0)))


def dgrad_lin(pb, dy, rows, r, dx):
    did = pb.did
    pb.bwd.append((lib.pfr_conv2d_fwd, (dy.data_ptr(), r.wt.data_ptr(), dx.data_ptr(), did, did, rows, 1, 1, r.out, r.inp, 1,
                                        1, 1, 0, 0, 1, 1, r.inp, 0, 0, 0, 0, 0, 0, 0, 0)))


def ln_fwd(pb, x, lnrec, rows, C):
    """→ (normalised rows, their means, their reciprocal standard deviations)"""
    y = pb.A((rows, C)); mu = pb.A((rows,), torch.float32); rs = pb.A((rows,), torch.float32)
    pb.fwd.append((lib.pfr_layernorm_fwd, (x.data_ptr(), lnrec.gamma.data_ptr(), lnrec.beta.data_ptr(), y.data_ptr(), mu.data_ptr(),
                                           rs.data_ptr(), pb.did, rows, C, float(lnrec.eps))))
    return y, mu, rs


def ln_bwd(pb, dy, xin, mu, rs, lnrec, dres, dx, rows, C, want_sum=False, dxsum=True):
    """→ (partials, rows of partials) of the column sums of dx when want_sum (and `dxsum`, the engine's switch) and the kernel can
    emit them, else None"""
    did = pb.did
    nb = lib.pfr_layernorm_bwd_blocks(rows)
    # the kernel's per-workgroup partials ARE the partial sets of the deferred final merge (own buffer per LayerNorm: they
    # must survive until the batched merge at the next bucket boundary)
    part = pb.A((2, nb, C), torch.float32)
    dsum = pb.A((nb, C), torch.float32) if (want_sum and dxsum and lib.pfr_layernorm_bwd_dxsum_ok(did, C)) else None
    pb.bwd.append((lib.pfr_layernorm_bwd_dxsum, (dy.data_ptr(), xin.data_ptr(), mu.data_ptr(), rs.data_ptr(), lnrec.gamma.data_ptr(),
                                                 0 if dres is None else dres.data_ptr(), dx.data_ptr(), part.data_ptr(),
                                                 0 if dsum is None else dsum.data_ptr(), did, rows, C)))
    pb.pend_cs.append((part[0], lnrec.dgamma, nb, C, 0, 0))
    pb.pend_cs.append((part[1], lnrec.dbeta, nb, C, 0, 0))
    return None if dsum is None else (dsum, nb)


def bias_grad(pb, g, rows, C, dbias, gsum):
    """bias gradient = column sum of g: from the LayerNorm-backward pass that produced g when it left the sums (gsum), else
    a column-sum pass of its own on the side stream"""
    if gsum is not None:
        pb.pend_cs.append((gsum[0], dbias, gsum[1], C, 0, 0))
    else:
        pb.colsum(g, rows, C, dbias)


# ---------------------------------------------------------------------------------------------- BatchNorm
class BatchNormLayers:
    """`train`: batch statistics from the partials the producing convolution leaves (pfr_bn_finalize; its workspace `bn_ws` is the
    engine's), else the running ones (pfr_bn_eval_coeff)"""

    def __init__(self, pb, train, bn_ws):
        self.pb, self.train, self.bn_ws = pb, train, bn_ws

    def coef(self, bn):
        """this plan's (mean, invstd, scale, shift) and backward coefficients of a BatchNorm"""
        pb = self.pb
        c = _Rec()
        c.bn = bn
        c.f = pb.plan.keep(torch.zeros((4, bn.C), dtype=torch.float32, device=pb.device))
        c.b = pb.plan.keep(torch.zeros((3, bn.C), dtype=torch.float32, device=pb.device))
        c.scale, c.shift = c.f[2], c.f[3]
        return c

    def bn_fwd(self, c, part, nparts, rpp, count):
        bn, fwd = c.bn, self.pb.fwd
        if self.train:
            nws = lib.pfr_bn_finalize_ws_floats(nparts, bn.C)
            assert nws <= self.bn_ws.numel()
            fwd.append((lib.pfr_bn_finalize, (part.data_ptr(), nparts, rpp, bn.C, float(count), bn.gamma.data_ptr(), bn.beta.data_ptr(),
                                              bn.eps, bn.momentum, bn.rm.data_ptr(), bn.rv.data_ptr(), c.f[0].data_ptr(),
                                              c.f[1].data_ptr(), c.f[2].data_ptr(), c.f[3].data_ptr(),
                                              self.bn_ws.data_ptr() if nws else 0)))
        else:
            fwd.append((lib.pfr_bn_eval_coeff, (bn.C, bn.gamma.data_ptr(), bn.beta.data_ptr(), bn.rm.data_ptr(), bn.rv.data_ptr(),
                                                bn.eps, c.f[2].data_ptr(), c.f[3].data_ptr())))

    def conv_bn(self, x, xshape, w, cout, R, stride, pad, bn):
        """dense convolution + the BatchNorm coefficients of its output → (raw output, its shape, coefficients)"""
        pb, train, did = self.pb, self.train, self.pb.did
        Nq, Hq, Wq, Cq = xshape
        OH, OW = (Hq + 2 * pad - R) // stride + 1, (Wq + 2 * pad - R) // stride + 1
        M = Nq * OH * OW
        z = pb.A((Nq, OH, OW, cout))
        part, nt, mt = None, 0, 0
        if train:
            mt = lib.pfr_conv2d_mtile(Nq, Hq, Wq, Cq, cout, R, R, stride, pad, OH, OW, did, did, 0)
            nt = (M + mt - 1) // mt
            part = pb.A((nt, 2, cout), torch.float32)
        pb.fwd.append((lib.pfr_conv2d_fwd, (x.data_ptr(), w.data_ptr(), z.data_ptr(), did, did, Nq, Hq, Wq, Cq, cout, R, R, stride, pad, 0,
                                            OH, OW, cout, 0, 0, 0, 0, 0, 0, 0, part.data_ptr() if train else 0)))
        c = self.coef(bn)
        self.bn_fwd(c, part, nt, mt, M)
        return z, (Nq, OH, OW, cout), c

    def dgrad_pw(self, dy, rows, r, dx, residual=None):
        did = self.pb.did
        self.pb.bwd.append((lib.pfr_conv2d_fwd, (dy.data_ptr(), r.wt.data_ptr(), dx.data_ptr(), did, did, rows, 1, 1, r.out, r.inp, 1, 1, 1,
                                                 0, 0, 1, 1, r.inp, 0, 0 if residual is None else residual.data_ptr(), 0, 0, 0, 0, 0, 0)))

    def bn_bwd(self, dout, z, c, rows, act=None, hi=0.0, slope=None):
        """dz of z from the gradient of act(bn(z)) — `act` None (linear), "clamp" (to [0, hi]: ReLU6 with hi = 6), "silu" or "prelu"
        (`slope`: the record of the nn.PReLU weight, w and g [C] fp32; its gradient is finalised on the side stream), the
        derivative recomputed from z — into a pooled buffer; dgamma / dbeta into the flat gradient"""
        pb, did, bn = self.pb, self.pb.did, c.bn
        bwd = pb.bwd
        nb = lib.pfr_colreduce_blocks(bn.C, did, rows)
        part = pb.A((nb, 3 if act == "prelu" else 2, bn.C), torch.float32)
        mode, hi = (2, hi) if act == "clamp" else (0, 0.0)
        if act == "prelu":
            bwd.append((lib.pfr_bn_bwd_reduce_prelu, (dout.data_ptr(), z.data_ptr(), c.f[0].data_ptr(), c.f[1].data_ptr(), c.scale.data_ptr(),
                                                      c.shift.data_ptr(), slope.w.data_ptr(), did, rows, bn.C, part.data_ptr())))
        elif act == "silu":
            bwd.append((lib.pfr_bn_bwd_reduce_silu, (dout.data_ptr(), z.data_ptr(), c.f[0].data_ptr(), c.f[1].data_ptr(),
                                                     c.scale.data_ptr(), c.shift.data_ptr(), did, rows, bn.C, part.data_ptr())))
        else:
            bwd.append((lib.pfr_bn_bwd_reduce_clamp, (dout.data_ptr(), z.data_ptr(), c.f[0].data_ptr(), c.f[1].data_ptr(),
                                                      c.scale.data_ptr(), c.shift.data_ptr(), hi, mode, did, rows, bn.C, part.data_ptr())))
        bwd.append((lib.pfr_bn_bwd_finalize, (part.data_ptr(), nb, bn.C, float(rows), bn.gamma.data_ptr(), c.f[0].data_ptr(),
                                              c.f[1].data_ptr(), bn.dgamma.data_ptr(), bn.dbeta.data_ptr(), c.b.data_ptr(), 0)))
        dz = pb.G(tuple(z.shape))
        if act == "prelu":
            pb.side((SIDE, (lib.pfr_prelu_slope_finalize, (part.data_ptr(), nb, bn.C, slope.g.data_ptr(), 0))))
            bwd.append((lib.pfr_bn_bwd_apply_prelu, (dout.data_ptr(), z.data_ptr(), c.b.data_ptr(), c.scale.data_ptr(), c.shift.data_ptr(),
                                                     slope.w.data_ptr(), dz.data_ptr(), did, rows, bn.C)))
        elif act == "silu":
            bwd.append((lib.pfr_bn_bwd_apply_silu, (dout.data_ptr(), z.data_ptr(), c.b.data_ptr(), c.scale.data_ptr(), c.shift.data_ptr(),
                                                    dz.data_ptr(), did, rows, bn.C)))
        else:
            bwd.append((lib.pfr_bn_bwd_apply_clamp, (dout.data_ptr(), z.data_ptr(), c.b.data_ptr(), c.scale.data_ptr(), c.shift.data_ptr(),
                                                     hi, mode, dz.data_ptr(), did, rows, bn.C)))
        return dz
