"""Tensor-level wrappers over the C-ABI (include/pfr_hip.h).  Tensors are torch CUDA tensors used purely as
device-memory handles: `.data_ptr()` goes straight into libpfr_hip.so, launches go on torch's current stream.
Nothing here computes with torch."""
import torch

from .lib import lib, dtype_id, PFR_F32, PFR_BF16, PfrError


def _p(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, name):
    if t is not None:
        if not t.is_cuda:
            raise PfrError(f"{name}: expected a CUDA (HIP) tensor — the HIP path has no CPU fallback")
        if not t.is_contiguous():
            raise PfrError(f"{name}: tensor must be contiguous")


def kpack(dtype):
    return 8 if dtype == torch.bfloat16 else 4


# ------------------------------------------------------------------------------------------------ conv / linear
def conv_out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def conv2d_fwd(x, w, stride=1, pad=0, idil_log2=0, out_hw=None, out=None, out_dtype=None, bias=None, accumulate=False,
               out_relu=False, pro=None, stats=False, stats_buf=None, residual=None):
    """x [N,H,W,C] NHWC, w [Cout,R,S,C].  Returns (y [N,OH,OW,Cout], stats_part or None)."""
    _chk(x, "x"); _chk(w, "w")
    N, H, W, C = x.shape
    Cout, R, S, Cw = w.shape
    assert Cw == C, (Cw, C)
    if out_hw is None:
        OH, OW = conv_out_hw(H, W, R, S, stride, pad)
    else:
        OH, OW = out_hw
    odt = out_dtype or x.dtype
    if out is None:
        out = torch.empty((N, OH, OW, Cout), dtype=odt, device=x.device)
    ldy = out.shape[-1]
    M = N * OH * OW
    part = None
    if stats:
        mt = lib.pfr_conv2d_mtile(N, H, W, C, Cout, R, S, stride, pad, OH, OW, dtype_id(x.dtype), dtype_id(out.dtype), int(pro is not None))
        nt = (M + mt - 1) // mt
        conv2d_fwd.last_mt = mt     # (rows per statistics partial of this launch: what pfr_bn_finalize needs as rows_per_part)
        part = stats_buf if stats_buf is not None else torch.empty((nt, 2, Cout), dtype=torch.float32, device=x.device)
        assert part.numel() >= nt * 2 * Cout
    ps = psh = None
    prelu = 0
    if pro is not None:
        ps, psh, prelu = pro
    lib.pfr_conv2d_fwd(_p(x), _p(w), _p(out), dtype_id(x.dtype), dtype_id(out.dtype), N, H, W, C, Cout, R, S, stride, pad,
                       idil_log2, OH, OW, ldy, _p(bias), _p(residual), int(accumulate), int(out_relu), _p(ps), _p(psh), int(prelu),
                       _p(part), _stream())
    return out, part


def conv2d_dgrad(dy, wt, in_hw, stride, pad, R, S, out=None, accumulate=False, out_dtype=None):
    """dy [N,OH,OW,Cout]; wt [Cin,R,S,Cout] = dgrad layout of the weights (weight_dgrad_layout).  → dx [N,H,W,Cin]"""
    H, W = in_hw
    log2 = {1: 0, 2: 1, 4: 2}[stride]
    y, _ = conv2d_fwd(dy, wt, stride=1, pad=R - 1 - pad, idil_log2=log2, out_hw=(H, W), out=out, accumulate=accumulate,
                      out_dtype=out_dtype)
    return y


def _conv2d_dgrad_geom_check(dy, in_hw, stride, pad, R):
    # the dilated-input gather computes ih = (h - (R-1-pad) + r') which must equal h + pad - r with r' = R-1-r
    return True


def weight_dgrad_layout(w, out=None):
    O, R, S, I = w.shape
    if out is None:
        out = torch.empty((I, R, S, O), dtype=w.dtype, device=w.device)
    lib.pfr_weight_dgrad_layout(_p(w), _p(out), dtype_id(w.dtype), O, R, S, I, _stream())
    return out


def conv2d_wgrad(x, dy, R, S, stride, pad, out=None, pro=None, scale=1.0, accumulate=False, workspace=None):
    """x [N,H,W,C], dy [N,OH,OW,Cout] → dw fp32 [Cout,R,S,C]"""
    _chk(x, "x"); _chk(dy, "dy")
    N, H, W, C = x.shape
    _, OH, OW, Cout = dy.shape
    if out is None:
        out = torch.empty((Cout, R, S, C), dtype=torch.float32, device=x.device)
    KK = R * S * C
    splits = lib.pfr_conv2d_wgrad_splits(N * OH * OW, Cout, KK)
    need = splits * Cout * KK
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.float32, device=x.device)
    ps = psh = None
    prelu = 0
    if pro is not None:
        ps, psh, prelu = pro
    lib.pfr_conv2d_wgrad(_p(x), _p(dy), _p(out), _p(workspace), dtype_id(x.dtype), N, H, W, C, Cout, R, S, stride, pad, OH,
                         OW, Cout, _p(ps), _p(psh), int(prelu), float(scale), int(accumulate), _stream())
    return out


# ------------------------------------------------------------------------------------------------ layout
def nchw_to_nhwc(x, dtype, cpad):
    N, C, H, W = x.shape
    assert x.dtype == torch.float32
    _chk(x, "x")
    y = torch.empty((N, H, W, cpad), dtype=dtype, device=x.device)
    lib.pfr_nchw_to_nhwc(_p(x), _p(y), dtype_id(dtype), N, C, H, W, cpad, _stream())
    return y


def cast(x, dtype, out=None):
    if out is None:
        out = torch.empty(x.shape, dtype=dtype, device=x.device)
    lib.pfr_cast(_p(x), dtype_id(x.dtype), _p(out), dtype_id(dtype), x.numel(), _stream())
    return out


def add(a, b, out=None):
    if out is None:
        out = torch.empty_like(a)
    lib.pfr_add(_p(a), _p(b), _p(out), dtype_id(a.dtype), a.numel(), _stream())
    return out


def colsum(x, out=None, accumulate=False):
    rows, C = x.shape
    if out is None:
        out = torch.empty(C, dtype=torch.float32, device=x.device)
    nws = lib.pfr_colsum_ws_floats(rows, C)
    ws = torch.empty(nws, dtype=torch.float32, device=x.device) if nws else None
    lib.pfr_colsum(_p(x), dtype_id(x.dtype), rows, C, _p(out), int(accumulate), _p(ws), _stream())
    return out


# ------------------------------------------------------------------------------------------------ batch norm
def bn_stats(x):
    C = x.shape[-1]
    rows = x.numel() // C
    nb = lib.pfr_colreduce_blocks(C, dtype_id(x.dtype), rows)
    part = torch.empty((nb, 2, C), dtype=torch.float32, device=x.device)
    lib.pfr_bn_stats(_p(x), dtype_id(x.dtype), rows, C, _p(part), _stream())
    return part, lib.pfr_bn_stats_rows_per_part(C, dtype_id(x.dtype), rows)


def bn_finalize(part, rows_per_part, count, gamma, beta, eps, momentum, running_mean, running_var, out=None):
    """→ (mean, invstd, scale, shift) rows of a [4,C] fp32 tensor"""
    C = part.shape[-1]
    nparts = part.numel() // (2 * C)
    if out is None:
        out = torch.empty((4, C), dtype=torch.float32, device=part.device)
    nws = lib.pfr_bn_finalize_ws_floats(nparts, C)
    ws = torch.empty(nws, dtype=torch.float32, device=part.device) if nws else None
    lib.pfr_bn_finalize(_p(part), nparts, int(rows_per_part), C, float(count), _p(gamma), _p(beta), float(eps), float(momentum),
                        _p(running_mean), _p(running_var), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _p(ws), _stream())
    return out


def bn_eval_coeff(gamma, beta, running_mean, running_var, eps, out=None):
    C = running_mean.numel()
    if out is None:
        out = torch.empty((2, C), dtype=torch.float32, device=running_mean.device)
    lib.pfr_bn_eval_coeff(C, _p(gamma), _p(beta), _p(running_mean), _p(running_var), float(eps), _p(out[0]), _p(out[1]), _stream())
    return out


def bn_act(x1, a1, b1, x2=None, a2=None, b2=None, relu=True, out=None, want_mask=False):
    """-> out, or (out, mask) with the ReLU bit mask ([rows][C / KPACK] bytes) that bn_bwd(mask_mode=3) consumes."""
    C = x1.shape[-1]
    rows = x1.numel() // C
    if out is None:
        out = torch.empty_like(x1)
    if want_mask:
        kp = 8 if x1.dtype == torch.bfloat16 else 4
        mask = torch.empty((rows, C // kp), dtype=torch.uint8, device=x1.device)
        lib.pfr_bn_act_mask(_p(x1), _p(a1), _p(b1), _p(x2), _p(a2), _p(b2), _p(out), _p(mask), dtype_id(x1.dtype), rows, C,
                            int(relu), _stream())
        return out, mask
    lib.pfr_bn_act(_p(x1), _p(a1), _p(b1), _p(x2), _p(a2), _p(b2), _p(out), dtype_id(x1.dtype), rows, C, int(relu), _stream())
    return out


def bn_bwd(dout, x, mean, invstd, gamma, count, mask_mode=0, out_act=None, scale=None, shift=None, dgamma=None,
           dbeta=None, want_gres=False, dx=None, gres=None, accumulate_param_grads=False):
    """Full BN(+ReLU mask) backward.  Returns (dx, gres or None, dgamma, dbeta)."""
    C = x.shape[-1]
    rows = x.numel() // C
    did = dtype_id(x.dtype)
    nb = lib.pfr_colreduce_blocks(C, did, rows)
    part = torch.empty((nb, 2, C), dtype=torch.float32, device=x.device)
    lib.pfr_bn_bwd_reduce(_p(dout), _p(out_act), _p(x), _p(mean), _p(invstd), _p(scale), _p(shift), mask_mode, did, rows, C,
                          _p(part), _stream())
    coef = torch.empty((3, C), dtype=torch.float32, device=x.device)
    if dgamma is None:
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
    if dbeta is None:
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
    lib.pfr_bn_bwd_finalize(_p(part), nb, C, float(count), _p(gamma), _p(mean), _p(invstd), _p(dgamma), _p(dbeta), _p(coef),
                            int(accumulate_param_grads), _stream())
    if dx is None:
        dx = torch.empty_like(x)
    if want_gres and gres is None:
        gres = torch.empty_like(x)
    lib.pfr_bn_bwd_apply(_p(dout), _p(out_act), _p(x), _p(coef), _p(scale), _p(shift), mask_mode, _p(dx), _p(gres), did, rows,
                         C, _stream())
    return dx, gres, dgamma, dbeta


# ------------------------------------------------------------------------------------------------ pooling
def bn_relu_maxpool_fwd(x, scale, shift, relu=True, want_idx=True):
    N, H, W, C = x.shape
    OH, OW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((N, OH, OW, C), dtype=x.dtype, device=x.device)
    idx = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=x.device) if want_idx else None
    lib.pfr_bn_relu_maxpool_fwd(_p(x), _p(scale), _p(shift), _p(y), _p(idx), dtype_id(x.dtype), N, H, W, C, int(relu), _stream())
    return y, idx


def maxpool_bwd(dy, idx, in_hw):
    N, OH, OW, C = dy.shape
    H, W = in_hw
    dz = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    lib.pfr_maxpool_bwd(_p(dy), _p(idx), _p(dz), dtype_id(dy.dtype), N, H, W, C, _stream())
    return dz


def avgpool_fwd(x):
    N, H, W, C = x.shape
    y = torch.empty((N, C), dtype=x.dtype, device=x.device)
    lib.pfr_avgpool_fwd(_p(x), _p(y), dtype_id(x.dtype), N, H * W, C, _stream())
    return y


def avgpool_bwd(dy, hw):
    N, C = dy.shape
    H, W = hw
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    lib.pfr_avgpool_bwd(_p(dy), _p(dx), dtype_id(dy.dtype), N, H * W, C, _stream())
    return dx


# ------------------------------------------------------------------------------------------------ head
def l2norm_fwd(x, out_dtype, want_t=False, ldt=None, xn=None, xnT=None, inv=None):
    rows, D = x.shape
    if xn is None:
        xn = torch.empty((rows, D), dtype=out_dtype, device=x.device)
    if want_t and xnT is None:
        xnT = torch.zeros((D, ldt or rows), dtype=out_dtype, device=x.device)
    if inv is None:
        inv = torch.empty(rows, dtype=torch.float32, device=x.device)
    lib.pfr_l2norm_fwd(_p(x), dtype_id(x.dtype), _p(xn), _p(xnT), dtype_id(out_dtype), _p(inv), rows, D,
                       0 if xnT is None else xnT.shape[1], 1e-12, _stream())
    return xn, xnT, inv


def l2norm_bwd(x, inv, dxn, out_dtype, out=None, accumulate=False):
    rows, D = x.shape
    assert dxn.dtype == torch.float32
    if out is None:
        out = torch.empty((rows, D), dtype=out_dtype, device=x.device)
    lib.pfr_l2norm_bwd(_p(x), dtype_id(x.dtype), _p(inv), _p(dxn), _p(out), dtype_id(out.dtype), rows, D, int(accumulate), _stream())
    return out


MARGIN_MODES = {"arc": 0, "arc_easy": 1, "cos": 2, "none": 3}


def margin_ce(cosv, label, C, mode, s, m, gamma=0.0, grad_scale=1.0, grad_scale_dev=None, want_logits=True, dcos_dtype=None, dcos=None,
              logits=None, loss_rows=None):
    B, ldc = cosv.shape
    assert cosv.dtype == torch.float32 and label.dtype == torch.int64
    if want_logits and logits is None:
        logits = torch.empty((B, C), dtype=torch.float32, device=cosv.device)
    if loss_rows is None:
        loss_rows = torch.empty(B, dtype=torch.float32, device=cosv.device)
    if dcos_dtype is not None and dcos is None:
        dcos = torch.zeros((B, ldc), dtype=dcos_dtype, device=cosv.device)
    lib.pfr_margin_ce(_p(cosv), _p(label), B, C, ldc, MARGIN_MODES[mode], float(s), float(m), float(gamma), float(grad_scale),
                      _p(grad_scale_dev), _p(logits), _p(loss_rows), _p(dcos), PFR_F32 if dcos is None else dtype_id(dcos.dtype), _stream())
    return logits, loss_rows, dcos


def mean(x, out=None):
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=x.device)
    lib.pfr_mean(_p(x), _p(out), x.numel(), _stream())
    return out


def _chk_class_vector(v, C, device, name):
    if v is not None and (v.dtype != torch.float32 or v.shape != (C,) or v.device != device or not v.is_contiguous()):
        raise PfrError(f"{name}: expected a contiguous fp32 [{C}] tensor on {device}")


def margin_ce_ex(cosv, label, C, mode, s, m, gamma=0.0, alpha=None, class_weight=None, label_smoothing=0.0, grad_scale=1.0,
                 grad_scale_dev=None, grad_scale_dev2=None, want_logits=True, want_stats=True, dcos_dtype=None):
    """margin_ce with the criterion options of pfr_margin_ce_ex -> (logits, loss_rows, row_stats [B, 4], dcos)"""
    B, ldc = cosv.shape
    assert cosv.dtype == torch.float32 and label.dtype == torch.int64
    _chk_class_vector(alpha, C, cosv.device, "margin_ce_ex: alpha")
    _chk_class_vector(class_weight, C, cosv.device, "margin_ce_ex: class_weight")
    logits = torch.empty((B, C), dtype=torch.float32, device=cosv.device) if want_logits else None
    loss_rows = torch.empty(B, dtype=torch.float32, device=cosv.device)
    stats = torch.empty((B, 4), dtype=torch.float32, device=cosv.device) if want_stats else None
    dcos = None if dcos_dtype is None else torch.zeros((B, ldc), dtype=dcos_dtype, device=cosv.device)
    lib.pfr_margin_ce_ex(_p(cosv), _p(label), B, C, ldc, MARGIN_MODES[mode], float(s), float(m), float(gamma), _p(alpha), _p(class_weight),
                         float(label_smoothing), float(grad_scale), _p(grad_scale_dev), _p(grad_scale_dev2), _p(logits), _p(loss_rows),
                         _p(stats), _p(dcos), PFR_F32 if dcos is None else dtype_id(dcos.dtype), _stream())
    return logits, loss_rows, stats, dcos


def alpha_grad(cosv, label, alpha, row_stats, C, s, grad_scale=1.0, grad_scale_dev=None):
    """d loss / d alpha [C] of the adaptive-alpha focal criterion from cos, alpha and margin_ce_ex's row statistics"""
    B, ldc = cosv.shape
    _chk_class_vector(alpha, C, cosv.device, "alpha_grad: alpha")
    assert row_stats.shape == (B, 4) and row_stats.dtype == torch.float32 and row_stats.is_contiguous()
    dalpha = torch.empty(C, dtype=torch.float32, device=cosv.device)
    lib.pfr_alpha_grad(_p(cosv), _p(label), _p(alpha), _p(row_stats), B, C, ldc, float(s), float(grad_scale), _p(grad_scale_dev),
                       _p(dalpha), _stream())
    return dalpha


LOSS_REDUCTIONS = {"mean": 0, "sum": 1, "weighted_mean": 2}


def loss_reduce(loss_rows, row_stats, reduction):
    """-> (loss, 1 / denominator), both device scalars"""
    out = torch.empty((), dtype=torch.float32, device=loss_rows.device)
    inv = torch.empty((), dtype=torch.float32, device=loss_rows.device)
    lib.pfr_loss_reduce(_p(loss_rows), _p(row_stats), loss_rows.numel(), LOSS_REDUCTIONS[reduction], _p(out), _p(inv), _stream())
    return out, inv


def _chk_sub(ok, what):
    if not ok:
        raise PfrError(what)


def subcenter_pool(cos_sub, C, K, ldc=None, label=None, count=None, cos=None, arg=None):
    """cos_sub [B, ld_sub] f32 (class-major sub-cosines, c*K + k) -> (cos [B, ldc] f32 = max over k with columns C.. zeroed,
    arg [B, C] uint8 = the lowest k attaining it); with `count` ([C*K] or [C, K] int32) the histogram of the label's sub-centre is added"""
    _chk(cos_sub, "subcenter_pool: cos_sub")
    _chk_sub(cos_sub.dim() == 2 and cos_sub.dtype == torch.float32, "subcenter_pool: cos_sub must be a 2-d fp32 tensor")
    B, ld_sub = cos_sub.shape
    _chk_sub(1 <= K <= 16 and C >= 1 and ld_sub >= C * K, f"subcenter_pool: {ld_sub} columns do not hold C={C} classes of K={K} (1..16) sub-centres")
    _chk_sub((count is None) == (label is None), "subcenter_pool: label and count go together")
    if count is not None:
        _chk(count, "subcenter_pool: count")
        _chk(label, "subcenter_pool: label")
        _chk_sub(count.dtype == torch.int32 and count.numel() == C * K and label.dtype == torch.int64 and label.numel() == B,
                 f"subcenter_pool: expected an int32 [{C * K}] count and an int64 [{B}] label")
    if cos is None:
        cos = torch.empty((B, C if ldc is None else ldc), dtype=torch.float32, device=cos_sub.device)
    if arg is None:
        arg = torch.empty((B, C), dtype=torch.uint8, device=cos_sub.device)
    _chk(cos, "subcenter_pool: cos")
    _chk(arg, "subcenter_pool: arg")
    _chk_sub(cos.dtype == torch.float32 and cos.dim() == 2 and cos.shape[0] == B and cos.shape[1] >= C,
             f"subcenter_pool: cos must be fp32 [{B}, >= {C}]")
    _chk_sub(arg.dtype == torch.uint8 and arg.shape == (B, C), f"subcenter_pool: arg must be uint8 [{B}, {C}]")
    lib.pfr_subcenter_pool(_p(cos_sub), B, C, K, ld_sub, _p(cos), cos.shape[1], _p(arg), _p(label), _p(count), _stream())
    return cos, arg


def subcenter_scatter(dcos, arg, K, ld_sub=None, out=None):
    """dcos [B, ldc], arg [B, C] uint8 -> dcos_sub [B, ld_sub] (dtype of dcos): dcos on each class's selected sub-centre, 0 elsewhere,
    pad columns included (the buffer needs no clearing)"""
    _chk(dcos, "subcenter_scatter: dcos")
    _chk(arg, "subcenter_scatter: arg")
    _chk_sub(dcos.dim() == 2 and arg.dim() == 2 and arg.dtype == torch.uint8 and arg.shape[0] == dcos.shape[0],
             "subcenter_scatter: expected dcos [B, ldc] and a uint8 arg [B, C]")
    B, ldc = dcos.shape
    C = arg.shape[1]
    _chk_sub(1 <= K <= 16 and ldc >= C, f"subcenter_scatter: K={K} outside 1..16 or dcos has {ldc} < C={C} columns")
    if out is None:
        out = torch.empty((B, C * K if ld_sub is None else ld_sub), dtype=dcos.dtype, device=dcos.device)
    _chk(out, "subcenter_scatter: out")
    _chk_sub(out.dtype == dcos.dtype and out.dim() == 2 and out.shape[0] == B and out.shape[1] >= C * K,
             f"subcenter_scatter: out must be {dcos.dtype} [{B}, >= {C * K}]")
    lib.pfr_subcenter_scatter(_p(dcos), dtype_id(dcos.dtype), _p(arg), B, C, K, ldc, _p(out), out.shape[1], _stream())
    return out


MARGIN_KINDS = {"adaface": 0, "curricular": 1}


def _margin_kind(kind, who):
    if kind not in MARGIN_KINDS:
        raise PfrError(f"{who}: margin kind must be one of {sorted(MARGIN_KINDS)}, got {kind!r}")
    return MARGIN_KINDS[kind]


def _chk_f32(t, shape, device, name):
    _chk(t, name)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or t.device != device:
        raise PfrError(f"{name}: expected a contiguous fp32 {list(shape)} tensor on {device}")


def _chk_cos_label(cosv, label, C, who):
    _chk(cosv, f"{who}: cos")
    _chk(label, f"{who}: label")
    if cosv.dim() != 2 or cosv.dtype != torch.float32 or cosv.shape[1] < C or C < 1:
        raise PfrError(f"{who}: cos must be fp32 [B, >= C={C}]")
    if label.dtype != torch.int64 or label.shape != (cosv.shape[0],) or label.device != cosv.device:
        raise PfrError(f"{who}: label must be int64 [{cosv.shape[0]}] on {cosv.device}")


def margin_prepare(kind, state, B, inv_norm=None, cosv=None, label=None, m=0.0, h=0.0, momentum=0.01, eps=1e-3, update=True):
    """The per-step state of an adaptive margin in one launch -> (row_margin [B, 2] or None, state_used [2]).
    'adaface': state = (batch_mean, batch_std), one-element fp32 tensors updated in place when `update`; reads inv_norm [B].
    'curricular': state = (t,); reads the target cosines of cosv [B, ldc] / label [B]."""
    k = _margin_kind(kind, "margin_prepare")
    if len(state) != (2 if kind == "adaface" else 1):
        raise PfrError(f"margin_prepare: '{kind}' takes {2 if kind == 'adaface' else 1} state buffer(s), got {len(state)}")
    dev = state[0].device
    for i, t in enumerate(state):
        _chk_f32(t.view(-1), (1,), dev, f"margin_prepare: state[{i}]")
    if not 0.0 <= momentum <= 1.0:
        raise PfrError(f"margin_prepare: momentum {momentum} outside [0, 1]")
    row_margin = None
    ldc = 0
    if kind == "adaface":
        if inv_norm is None:
            raise PfrError("margin_prepare: 'adaface' needs inv_norm")
        _chk_f32(inv_norm, (B,), dev, "margin_prepare: inv_norm")
        row_margin = torch.empty((B, 2), dtype=torch.float32, device=dev)
    else:
        if cosv is None or label is None:
            raise PfrError("margin_prepare: 'curricular' needs the cosines and the labels")
        _chk_cos_label(cosv, label, 1, "margin_prepare")
        if cosv.shape[0] != B or cosv.device != dev:
            raise PfrError(f"margin_prepare: cos must have {B} rows on {dev}")
        ldc = cosv.shape[1]
    state_used = torch.empty(2, dtype=torch.float32, device=dev)
    lib.pfr_margin_prepare(k, _p(inv_norm), _p(cosv), _p(label), B, ldc, float(m), float(h), float(momentum), float(eps), int(bool(update)),
                           _p(state[0]), _p(state[1]) if len(state) > 1 else 0, _p(row_margin), _p(state_used), _stream())
    return row_margin, state_used


def _chk_adaptive_state(kind, B, row_margin, state_used, device, who):
    if kind == "adaface":
        if row_margin is None:
            raise PfrError(f"{who}: 'adaface' needs margin_prepare's row_margin")
        _chk_f32(row_margin, (B, 2), device, f"{who}: row_margin")
    if state_used is None:
        raise PfrError(f"{who}: needs margin_prepare's state_used")
    _chk_f32(state_used, (2,), device, f"{who}: state_used")


def margin_ce_adaptive(cosv, label, C, kind, s, m, eps, row_margin, state_used, gamma=0.0, class_weight=None, label_smoothing=0.0,
                       grad_scale=1.0, grad_scale_dev=None, grad_scale_dev2=None, want_logits=True, want_stats=True, dcos_dtype=None):
    """margin_ce_ex for the adaptive margins ('adaface' / 'curricular') -> (logits, loss_rows, row_stats [B, 4], dcos)"""
    k = _margin_kind(kind, "margin_ce_adaptive")
    _chk_cos_label(cosv, label, C, "margin_ce_adaptive")
    B, ldc = cosv.shape
    _chk_adaptive_state(kind, B, row_margin, state_used, cosv.device, "margin_ce_adaptive")
    _chk_class_vector(class_weight, C, cosv.device, "margin_ce_adaptive: class_weight")
    if dcos_dtype not in (None, torch.float32, torch.bfloat16):
        raise PfrError(f"margin_ce_adaptive: dcos dtype must be fp32 or bf16, got {dcos_dtype}")
    logits = torch.empty((B, C), dtype=torch.float32, device=cosv.device) if want_logits else None
    loss_rows = torch.empty(B, dtype=torch.float32, device=cosv.device)
    stats = torch.empty((B, 4), dtype=torch.float32, device=cosv.device) if want_stats else None
    dcos = None if dcos_dtype is None else torch.zeros((B, ldc), dtype=dcos_dtype, device=cosv.device)
    lib.pfr_margin_ce_adaptive(_p(cosv), _p(label), B, C, ldc, k, float(s), float(m), float(eps), float(gamma), _p(class_weight),
                               float(label_smoothing), _p(row_margin), _p(state_used), float(grad_scale), _p(grad_scale_dev),
                               _p(grad_scale_dev2), _p(logits), _p(loss_rows), _p(stats), _p(dcos),
                               PFR_F32 if dcos is None else dtype_id(dcos.dtype), _stream())
    return logits, loss_rows, stats, dcos


def margin_bwd_adaptive(cosv, label, C, kind, s, m, eps, row_margin, state_used, dlogits, dcos_dtype):
    """dlogits [B, C] fp32 -> dcos [B, ldc] (pad columns 0) through the adaptive margin"""
    k = _margin_kind(kind, "margin_bwd_adaptive")
    _chk_cos_label(cosv, label, C, "margin_bwd_adaptive")
    B, ldc = cosv.shape
    _chk_adaptive_state(kind, B, row_margin, state_used, cosv.device, "margin_bwd_adaptive")
    _chk_f32(dlogits, (B, C), cosv.device, "margin_bwd_adaptive: dlogits")
    if dcos_dtype not in (torch.float32, torch.bfloat16):
        raise PfrError(f"margin_bwd_adaptive: dcos dtype must be fp32 or bf16, got {dcos_dtype}")
    dcos = torch.zeros((B, ldc), dtype=dcos_dtype, device=cosv.device)
    lib.pfr_margin_bwd_adaptive(_p(cosv), _p(label), B, C, ldc, k, float(s), float(m), float(eps), _p(row_margin), _p(state_used),
                                _p(dlogits), _p(dcos), dtype_id(dcos_dtype), _stream())
    return dcos


def magface_prepare(inv_norm, l_a, u_a, l_m, u_m):
    """inv_norm [B] (l2norm_fwd) -> (row_margin [B, 2] = {m, dm/d|x|}, row_reg [B, 2] = {g(a), dg/d|x|}); the derivatives are 0 where
    |x| lies outside [l_a, u_a]"""
    if not 0.0 < l_a < u_a:
        raise PfrError(f"magface_prepare: need 0 < l_a < u_a, got {l_a}, {u_a}")
    _chk(inv_norm, "magface_prepare: inv_norm")
    if inv_norm.dim() != 1 or inv_norm.dtype != torch.float32:
        raise PfrError("magface_prepare: inv_norm must be an fp32 [B] tensor")
    B = inv_norm.numel()
    row_margin = torch.empty((B, 2), dtype=torch.float32, device=inv_norm.device)
    row_reg = torch.empty((B, 2), dtype=torch.float32, device=inv_norm.device)
    lib.pfr_magface_prepare(_p(inv_norm), B, float(l_a), float(u_a), float(l_m), float(u_m), _p(row_margin), _p(row_reg), _stream())
    return row_margin, row_reg


def margin_ce_magface(cosv, label, C, easy_margin, s, row_margin, row_reg, reg_scale=0.0, gamma=0.0, class_weight=None, label_smoothing=0.0,
                      grad_scale=1.0, grad_scale_dev=None, grad_scale_dev2=None, want_logits=True, want_stats=True, dcos_dtype=None):
    """margin_ce_adaptive for MagFace -> (logits, loss_rows, row_stats [B, 4], dcos, dnorm [B]); dnorm (with dcos only) is
    d loss / d |x| at dcos's gradient scale, the regulariser's reg_scale * grad_scale_dev * dg/d|x| included"""
    _chk_cos_label(cosv, label, C, "margin_ce_magface")
    B, ldc = cosv.shape
    _chk_f32(row_margin, (B, 2), cosv.device, "margin_ce_magface: row_margin")
    if row_reg is not None:
        _chk_f32(row_reg, (B, 2), cosv.device, "margin_ce_magface: row_reg")
    _chk_class_vector(class_weight, C, cosv.device, "margin_ce_magface: class_weight")
    if dcos_dtype not in (None, torch.float32, torch.bfloat16):
        raise PfrError(f"margin_ce_magface: dcos dtype must be fp32 or bf16, got {dcos_dtype}")
    logits = torch.empty((B, C), dtype=torch.float32, device=cosv.device) if want_logits else None
    loss_rows = torch.empty(B, dtype=torch.float32, device=cosv.device)
    stats = torch.empty((B, 4), dtype=torch.float32, device=cosv.device) if want_stats else None
    dcos = None if dcos_dtype is None else torch.zeros((B, ldc), dtype=dcos_dtype, device=cosv.device)
    dnorm = None if dcos_dtype is None else torch.empty(B, dtype=torch.float32, device=cosv.device)
    lib.pfr_margin_ce_magface(_p(cosv), _p(label), B, C, ldc, int(bool(easy_margin)), float(s), float(gamma), _p(class_weight),
                              float(label_smoothing), _p(row_margin), _p(row_reg), float(reg_scale), float(grad_scale), _p(grad_scale_dev),
                              _p(grad_scale_dev2), _p(logits), _p(loss_rows), _p(stats), _p(dcos),
                              PFR_F32 if dcos is None else dtype_id(dcos.dtype), _p(dnorm), _stream())
    return logits, loss_rows, stats, dcos, dnorm


def margin_bwd_magface(cosv, label, C, easy_margin, s, row_margin, row_reg, reg_scale, reg_scale_dev, dlogits, dcos_dtype):
    """dlogits [B, C] fp32 -> (dcos [B, ldc] (pad columns 0), dnorm [B]) through the MagFace margin; dnorm also carries
    reg_scale * reg_scale_dev * dg/d|x| (reg_scale_dev: the regulariser's incoming gradient, a device scalar, or None = 1)"""
    _chk_cos_label(cosv, label, C, "margin_bwd_magface")
    B, ldc = cosv.shape
    _chk_f32(row_margin, (B, 2), cosv.device, "margin_bwd_magface: row_margin")
    if row_reg is not None:
        _chk_f32(row_reg, (B, 2), cosv.device, "margin_bwd_magface: row_reg")
    _chk_f32(dlogits, (B, C), cosv.device, "margin_bwd_magface: dlogits")
    if dcos_dtype not in (torch.float32, torch.bfloat16):
        raise PfrError(f"margin_bwd_magface: dcos dtype must be fp32 or bf16, got {dcos_dtype}")
    dcos = torch.zeros((B, ldc), dtype=dcos_dtype, device=cosv.device)
    dnorm = torch.empty(B, dtype=torch.float32, device=cosv.device)
    lib.pfr_margin_bwd_magface(_p(cosv), _p(label), B, C, ldc, int(bool(easy_margin)), float(s), _p(row_margin), _p(row_reg),
                               float(reg_scale), _p(reg_scale_dev), _p(dlogits), _p(dcos), dtype_id(dcos_dtype), _p(dnorm), _stream())
    return dcos, dnorm


def magface_loss(loss_rows, row_stats, row_reg, reduction, lambda_g):
    """loss_reduce with MagFace's regulariser -> (loss incl. the regulariser, 1 / denominator, regulariser), device scalars;
    loss_rows None -> (None, None, regulariser)"""
    n = row_reg.shape[0]
    dev = row_reg.device
    reg = torch.empty((), dtype=torch.float32, device=dev)
    out = inv = None
    if loss_rows is not None:
        out = torch.empty((), dtype=torch.float32, device=dev)
        inv = torch.empty((), dtype=torch.float32, device=dev)
    lib.pfr_magface_loss(_p(loss_rows), _p(row_stats), _p(row_reg), n, LOSS_REDUCTIONS[reduction], float(lambda_g), _p(out), _p(inv), _p(reg),
                         _stream())
    return out, inv, reg


def l2norm_bwd_radial(x, inv, dxn, dnorm, out_dtype, out=None, accumulate=False):
    """l2norm_bwd plus dnorm[row] * x[row] / |x[row]| in the same pass; dnorm None is l2norm_bwd itself"""
    rows, D = x.shape
    assert dxn.dtype == torch.float32
    if dnorm is not None:
        _chk_f32(dnorm, (rows,), x.device, "l2norm_bwd_radial: dnorm")
    if out is None:
        out = torch.empty((rows, D), dtype=out_dtype, device=x.device)
    lib.pfr_l2norm_bwd_radial(_p(x), dtype_id(x.dtype), _p(inv), _p(dxn), _p(dnorm), _p(out), dtype_id(out.dtype), rows, D, int(accumulate),
                              _stream())
    return out


# ------------------------------------------------------------------------------------------------ pair losses
PAIR_KINDS = {"supcon": 0, "circle": 1}
_PAIR_TICKETS = {}


def pair_params(kind, tau=0.1, m=0.25, gamma=64.0):
    """-> (kind id, p0, p1) of pfr_pair_loss_fwd / _bwd: supcon (tau, 0), circle (m, gamma)"""
    if kind not in PAIR_KINDS:
        raise ValueError(f"pair loss kind must be one of {sorted(PAIR_KINDS)}, got {kind!r}")
    return (0, float(tau), 0.0) if kind == "supcon" else (1, float(m), float(gamma))


def _pair_ticket(device):
    """the zeroed int32 the forward's last-workgroup reduction counts on and leaves at 0: one per (device, stream)"""
    key = (device.index, _stream())
    t = _PAIR_TICKETS.get(key)
    if t is None:
        t = _PAIR_TICKETS[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return t


def _pair_chk(xn, label):
    _chk(xn, "pair_loss: xn"); _chk(label, "pair_loss: label")
    if xn.dim() != 2 or xn.dtype not in (torch.float32, torch.bfloat16):
        raise PfrError(f"pair_loss: xn must be a [B, D] fp32 or bf16 tensor (int8 is not supported), got {xn.dtype} {tuple(xn.shape)}")
    if label.dtype != torch.int64 or label.shape != (xn.shape[0],):
        raise PfrError(f"pair_loss: label must be int64 [{xn.shape[0]}], got {label.dtype} {tuple(label.shape)}")


def pair_loss_fwd(xn, label, kind, **params):
    """normalised rows xn [B, D] (l2norm_fwd) -> (out fp32 [3] = {loss, 1 / A, A}, stats fp32 [B, 4], ell fp32 [B]); one launch"""
    _pair_chk(xn, label)
    B, D = xn.shape
    k, p0, p1 = pair_params(kind, **params)
    out = torch.empty(3, dtype=torch.float32, device=xn.device)
    stats = torch.empty((B, 4), dtype=torch.float32, device=xn.device)
    ell = torch.empty(B, dtype=torch.float32, device=xn.device)
    lib.pfr_pair_loss_fwd(_p(xn), dtype_id(xn.dtype), _p(label), B, D, k, p0, p1, _p(stats), _p(ell), _p(out), _p(_pair_ticket(xn.device)),
                          _stream())
    return out, stats, ell


def pair_loss_bwd(xn, xnT, label, stats, out, kind, grad_scale=1.0, grad_scale_dev=None, dxn=None, **params):
    """-> dxn fp32 [B, D] = grad_scale * (*grad_scale_dev) * d loss / d xn; xnT [D, ldt] is l2norm_fwd's transposed copy, ldt a multiple
    of 32 >= B with zero pad columns; one launch"""
    _pair_chk(xn, label)
    B, D = xn.shape
    k, p0, p1 = pair_params(kind, **params)
    _chk(xnT, "pair_loss_bwd: xnT")
    if xnT.dtype != xn.dtype or xnT.dim() != 2 or xnT.shape[0] != D:
        raise PfrError(f"pair_loss_bwd: xnT must be {xn.dtype} [{D}, ldt], got {xnT.dtype} {tuple(xnT.shape)}")
    _chk_f32(stats, (B, 4), xn.device, "pair_loss_bwd: stats")
    _chk_f32(out, (3,), xn.device, "pair_loss_bwd: out")
    if grad_scale_dev is not None:
        _chk_f32(grad_scale_dev, grad_scale_dev.shape, xn.device, "pair_loss_bwd: grad_scale_dev")
    if dxn is None:
        dxn = torch.empty((B, D), dtype=torch.float32, device=xn.device)
    lib.pfr_pair_loss_bwd(_p(xn), _p(xnT), dtype_id(xn.dtype), xnT.shape[1], _p(label), B, D, k, p0, p1, _p(stats), _p(out), float(grad_scale),
                          _p(grad_scale_dev), _p(dxn), _stream())
    return dxn


# ------------------------------------------------------------------------------------------------ pair losses with a cross-batch memory
def _pair_mem_chk(xn, label, mem, mem_label, count, who):
    _pair_chk(xn, label)
    _chk(mem, f"{who}: mem"); _chk(mem_label, f"{who}: mem_label")
    D = xn.shape[1]
    if mem.dim() != 2 or mem.dtype != xn.dtype or mem.shape[1] != D or mem.device != xn.device:
        raise PfrError(f"{who}: mem must be {xn.dtype} [M, {D}] on {xn.device}, got {mem.dtype} {tuple(mem.shape)} on {mem.device}")
    M = mem.shape[0]
    if mem_label.dtype != torch.int64 or mem_label.shape != (M,):
        raise PfrError(f"{who}: mem_label must be int64 [{M}], got {mem_label.dtype} {tuple(mem_label.shape)}")
    if not 0 <= int(count) <= M:
        raise PfrError(f"{who}: need 0 <= count <= M = {M}, got {count}")
    return M


def pair_mem_splits(B, count, D):
    """the number of partner-range splits that splits=0 stands for (host arithmetic); the workspaces hold [S, B, 8] (forward) and [S, B, D]
    (backward) floats"""
    return lib.pfr_pair_mem_splits(int(B), int(count), int(D))


def pair_mem_loss_fwd(xn, label, mem, mem_label, count, kind, splits=0, **params):
    """pair_loss_fwd with the live slots 0 .. count-1 of the ring (mem [M, D], mem_label [M]) as further partners -> (out, stats, ell);
    one launch.  splits: 0 = pair_mem_splits, or an explicit number of partner-range splits (the tests)"""
    M = _pair_mem_chk(xn, label, mem, mem_label, count, "pair_mem_loss_fwd")
    B, D = xn.shape
    k, p0, p1 = pair_params(kind, **params)
    S = int(splits) or pair_mem_splits(B, count, D)
    ws = torch.empty((S, B, 8), dtype=torch.float32, device=xn.device) if S > 1 else None
    out = torch.empty(3, dtype=torch.float32, device=xn.device)
    stats = torch.empty((B, 4), dtype=torch.float32, device=xn.device)
    ell = torch.empty(B, dtype=torch.float32, device=xn.device)
    lib.pfr_pair_mem_loss_fwd(_p(xn), dtype_id(xn.dtype), _p(label), B, D, _p(mem), _p(mem_label), M, int(count), k, p0, p1, S, _p(ws),
                              _p(stats), _p(ell), _p(out), _p(_pair_ticket(xn.device)), _stream())
    return out, stats, ell


def pair_mem_loss_bwd(xn, xnT, label, mem, memT, mem_label, count, stats, out, kind, grad_scale=1.0, grad_scale_dev=None, dxn=None, splits=0,
                      **params):
    """-> dxn fp32 [B, D]; memT [D, ldm] is the ring transposed, ldm a multiple of 32 >= M and zero at columns >= count (pair_mem_push keeps
    it so).  Nothing flows to the ring.  One launch, plus the slab sum when there is more than one split"""
    M = _pair_mem_chk(xn, label, mem, mem_label, count, "pair_mem_loss_bwd")
    B, D = xn.shape
    k, p0, p1 = pair_params(kind, **params)
    _chk(xnT, "pair_mem_loss_bwd: xnT"); _chk(memT, "pair_mem_loss_bwd: memT")
    if xnT.dtype != xn.dtype or xnT.dim() != 2 or xnT.shape[0] != D:
        raise PfrError(f"pair_mem_loss_bwd: xnT must be {xn.dtype} [{D}, ldt], got {xnT.dtype} {tuple(xnT.shape)}")
    if memT.dtype != xn.dtype or memT.dim() != 2 or memT.shape[0] != D:
        raise PfrError(f"pair_mem_loss_bwd: memT must be {xn.dtype} [{D}, ldm], got {memT.dtype} {tuple(memT.shape)}")
    _chk_f32(stats, (B, 4), xn.device, "pair_mem_loss_bwd: stats")
    _chk_f32(out, (3,), xn.device, "pair_mem_loss_bwd: out")
    if grad_scale_dev is not None:
        _chk_f32(grad_scale_dev, grad_scale_dev.shape, xn.device, "pair_mem_loss_bwd: grad_scale_dev")
    if dxn is None:
        dxn = torch.empty((B, D), dtype=torch.float32, device=xn.device)
    S = int(splits) or pair_mem_splits(B, count, D)
    ws = torch.empty((S, B, D), dtype=torch.float32, device=xn.device) if S > 1 else None
    lib.pfr_pair_mem_loss_bwd(_p(xn), _p(xnT), dtype_id(xn.dtype), xnT.shape[1], _p(label), B, D, _p(mem), _p(memT), memT.shape[1], _p(mem_label),
                              M, int(count), k, p0, p1, _p(stats), _p(out), float(grad_scale), _p(grad_scale_dev), S, _p(ws), _p(dxn), _stream())
    return dxn


def pair_mem_push(xn, label, mem, memT, mem_label, head):
    """rows, transposed columns and labels of the batch into the ring slots (head + r) mod M; the caller keeps head and count"""
    M = _pair_mem_chk(xn, label, mem, mem_label, 0, "pair_mem_push")
    B, D = xn.shape
    _chk(memT, "pair_mem_push: memT")
    if memT.dtype != xn.dtype or memT.dim() != 2 or memT.shape[0] != D:
        raise PfrError(f"pair_mem_push: memT must be {xn.dtype} [{D}, ldm], got {memT.dtype} {tuple(memT.shape)}")
    lib.pfr_pair_mem_push(_p(xn), _p(label), B, D, dtype_id(xn.dtype), _p(mem), _p(memT), memT.shape[1], _p(mem_label), M, int(head), _stream())


# ------------------------------------------------------------------------------------------------ mined pair losses
PAIR_MINED_KINDS = {"batch_hard": 2, "multi_similarity": 3}


def pair_mined_params(kind, m=0.3, gamma=0.0, alpha=2.0, beta=50.0, base=0.5, epsilon=0.1):
    """-> (kind id, the four host floats of pfr_pair_mined_fwd / _bwd): batch_hard (m, gamma, 0, 0), multi_similarity (alpha, beta,
    base, epsilon)"""
    import ctypes
    if kind not in PAIR_MINED_KINDS:
        raise ValueError(f"mined pair loss kind must be one of {sorted(PAIR_MINED_KINDS)}, got {kind!r}")
    vals = (m, gamma, 0.0, 0.0) if kind == "batch_hard" else (alpha, beta, base, epsilon)
    return PAIR_MINED_KINDS[kind], (ctypes.c_float * 4)(*[float(v) for v in vals])


def _pair_mined_chk(xn, label, mem, mem_label, count, who):
    """-> M; mem = None: the batch alone (M = count = 0)"""
    if mem is None:
        _pair_chk(xn, label)
        if mem_label is not None or int(count) != 0:
            raise PfrError(f"{who}: without a ring (mem=None) there is no mem_label and count is 0, got count={count}")
        return 0
    return _pair_mem_chk(xn, label, mem, mem_label, count, who)


def pair_mined_splits(B, count, D):
    """the number of partner-range splits that splits=0 stands for (host arithmetic; = pair_mem_splits); the workspaces hold [S, B, 8]
    (forward) and [S, B, D] (backward of multi_similarity) floats"""
    return lib.pfr_pair_mined_splits(int(B), int(count), int(D))


def pair_mined_fwd(xn, label, kind, mem=None, mem_label=None, count=0, splits=0, **params):
    """normalised rows xn [B, D] (l2norm_fwd), optionally the live slots 0 .. count-1 of a ring -> (out fp32 [3] = {loss, 1 / A, A},
    stats fp32 [B, 8], ell fp32 [B]).  stats[:, 2:4] hold partner numbers as int32 bits (stats.view(torch.int32)).  batch_hard: one
    launch; multi_similarity: two (the extremes, then the gated log-sum-exps)"""
    M = _pair_mined_chk(xn, label, mem, mem_label, count, "pair_mined_fwd")
    B, D = xn.shape
    k, p4 = pair_mined_params(kind, **params)
    S = int(splits) or pair_mined_splits(B, count, D)
    ws = torch.empty((S, B, 8), dtype=torch.float32, device=xn.device) if S > 1 else None
    out = torch.empty(3, dtype=torch.float32, device=xn.device)
    stats = torch.empty((B, 8), dtype=torch.float32, device=xn.device)
    ell = torch.empty(B, dtype=torch.float32, device=xn.device)
    lib.pfr_pair_mined_fwd(_p(xn), dtype_id(xn.dtype), _p(label), B, D, _p(mem), _p(mem_label), M, int(count), k, p4, S, _p(ws), _p(stats),
                           _p(ell), _p(out), _p(_pair_ticket(xn.device)), _stream())
    return out, stats, ell


def pair_mined_bwd(xn, xnT, label, stats, out, kind, mem=None, memT=None, mem_label=None, count=0, grad_scale=1.0, grad_scale_dev=None,
                   dxn=None, splits=0, **params):
    """-> dxn fp32 [B, D] = grad_scale * (*grad_scale_dev) * d loss / d xn.  multi_similarity: xnT [D, ldt] and memT [D, ldm] as for
    pair_mem_loss_bwd, one launch plus the slab sum when there is more than one split.  batch_hard: one sparse launch (xnT and memT are
    not read).  Nothing flows to the ring"""
    M = _pair_mined_chk(xn, label, mem, mem_label, count, "pair_mined_bwd")
    B, D = xn.shape
    k, p4 = pair_mined_params(kind, **params)
    _chk(xnT, "pair_mined_bwd: xnT"); _chk(memT, "pair_mined_bwd: memT")
    if xnT is None or xnT.dtype != xn.dtype or xnT.dim() != 2 or xnT.shape[0] != D:
        raise PfrError(f"pair_mined_bwd: xnT must be {xn.dtype} [{D}, ldt]")
    if (mem is None) != (memT is None) or (memT is not None and (memT.dtype != xn.dtype or memT.dim() != 2 or memT.shape[0] != D)):
        raise PfrError(f"pair_mined_bwd: memT must be {xn.dtype} [{D}, ldm] when there is a ring, and None without one")
    _chk_f32(stats, (B, 8), xn.device, "pair_mined_bwd: stats")
    _chk_f32(out, (3,), xn.device, "pair_mined_bwd: out")
    if grad_scale_dev is not None:
        _chk_f32(grad_scale_dev, grad_scale_dev.shape, xn.device, "pair_mined_bwd: grad_scale_dev")
    if dxn is None:
        dxn = torch.empty((B, D), dtype=torch.float32, device=xn.device)
    S = int(splits) or pair_mined_splits(B, count, D)
    ws = torch.empty((S, B, D), dtype=torch.float32, device=xn.device) if S > 1 and kind == "multi_similarity" else None
    lib.pfr_pair_mined_bwd(_p(xn), _p(xnT), dtype_id(xn.dtype), xnT.shape[1], _p(label), B, D, _p(mem), _p(memT),
                           0 if memT is None else memT.shape[1], _p(mem_label), M, int(count), k, p4, _p(stats), _p(out), float(grad_scale),
                           _p(grad_scale_dev), S, _p(ws), _p(dxn), _stream())
    return dxn


# ------------------------------------------------------------------------------------------------ optimisers
def sgd_step(p, g, mom, shadow, lr, momentum, weight_decay, grad_scale=1.0, first_step=False):
    lib.pfr_sgd_step(_p(p), _p(g), _p(mom), _p(shadow), PFR_F32 if shadow is None else dtype_id(shadow.dtype), p.numel(),
                     float(lr), float(momentum), float(weight_decay), float(grad_scale), int(first_step), _stream())


def adamw_step(p, g, m, v, shadow, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    lib.pfr_adamw_step(_p(p), _p(g), _p(m), _p(v), _p(shadow), PFR_F32 if shadow is None else dtype_id(shadow.dtype), p.numel(),
                       float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step), float(grad_scale),
                       _stream())


def sgd_step_clip(p, g, mom, shadow, lr, momentum, weight_decay, clip_coef, clip_value, grad_scale=1.0, first_step=False):
    """sgd_step on clamp(g * grad_scale * clip_coef, ±clip_value): clip_coef a 1-element fp32 CUDA tensor or None, clip_value 0 = no clamp"""
    lib.pfr_sgd_step_clip(_p(p), _p(g), _p(mom), _p(shadow), PFR_F32 if shadow is None else dtype_id(shadow.dtype), p.numel(),
                          float(lr), float(momentum), float(weight_decay), float(grad_scale), int(first_step), _p(clip_coef),
                          float(clip_value), _stream())


def adamw_step_clip(p, g, m, v, shadow, lr, beta1, beta2, eps, weight_decay, step, clip_coef, clip_value, grad_scale=1.0):
    lib.pfr_adamw_step_clip(_p(p), _p(g), _p(m), _p(v), _p(shadow), PFR_F32 if shadow is None else dtype_id(shadow.dtype),
                            p.numel(), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                            float(grad_scale), _p(clip_coef), float(clip_value), _stream())


def grad_norm(segs, chunk_seg, nseg, nchunks, norm_p, max_norm, ws, out):
    """pfr_grad_norm: segs / chunk_seg = the device tables of optim.fused.SegmentNorm, norm_p > 0 (math.inf: max norm),
    ws fp64 [nchunks + nseg], out fp32 [nseg + 2] (segment norms, total, clip coefficient)"""
    assert ws.dtype == torch.float64 and ws.numel() >= nchunks + nseg and out.dtype == torch.float32 and out.numel() >= nseg + 2
    lib.pfr_grad_norm(_p(segs), _p(chunk_seg), int(nseg), int(nchunks), float(norm_p), float(max_norm), _p(ws), _p(out), _stream())


def grad_norm_chunk_elems():
    return lib.pfr_grad_norm_chunk_elems()


# ------------------------------------------------------------------------------------------------ weight averaging (EMA / SWA)
def sgd_step_avg(p, g, mom, shadow, lr, momentum, weight_decay, clip_coef, clip_value, avg, avg_weight, grad_scale=1.0,
                 first_step=False):
    """sgd_step_clip (clip_coef None and clip_value 0: no clipping) + avg <- lerp(avg, p_new, avg_weight) in the same pass"""
    lib.pfr_sgd_step_avg(_p(p), _p(g), _p(mom), _p(shadow), PFR_F32 if shadow is None else dtype_id(shadow.dtype), p.numel(),
                         float(lr), float(momentum), float(weight_decay), float(grad_scale), int(first_step), _p(clip_coef),
                         float(clip_value), _p(avg), float(avg_weight), _stream())


def adamw_step_avg(p, g, m, v, shadow, lr, beta1, beta2, eps, weight_decay, step, clip_coef, clip_value, avg, avg_weight,
                   grad_scale=1.0):
    lib.pfr_adamw_step_avg(_p(p), _p(g), _p(m), _p(v), _p(shadow), PFR_F32 if shadow is None else dtype_id(shadow.dtype),
                           p.numel(), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                           float(grad_scale), _p(clip_coef), float(clip_value), _p(avg), float(avg_weight), _stream())


def weight_avg(avg, p, weight):
    """avg <- lerp(avg, p, weight) in place: dense fp32 CUDA tensors of one size (any offset into their storage)"""
    if avg.dtype != torch.float32 or p.dtype != torch.float32 or avg.numel() != p.numel():
        raise PfrError("weight_avg: fp32 tensors of one size expected")
    _chk(avg, "avg"); _chk(p, "p")
    lib.pfr_weight_avg(_p(avg), _p(p), avg.numel(), float(weight), _stream())


# ------------------------------------------------------------------------------------------------ Partial FC (csrc/pfr_pfc.hip)
def _chk_t(t, name, dtype, shape=None):
    _chk(t, name)
    if t.dtype != dtype or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise PfrError(f"{name}: expected a contiguous {dtype} tensor" + (f" of shape {tuple(shape)}" if shape is not None else "")
                       + f", got {t.dtype} {tuple(t.shape)}")


def pfc_sample(label, score, S, index=None, local_label=None):
    """label int64 [B], score fp32 [C] in [0, 1) -> (index int32 [S], local_label int64 [B]): the S classes with the largest key
    (2.0 for a class of the batch, else its score), ties towards the lower class id, ascending, and every label's position among them.
    Queued on the current stream, no host read-back."""
    _chk_t(label, "label", torch.int64)
    _chk_t(score, "score", torch.float32)
    B, C, S = label.numel(), score.numel(), int(S)
    if index is None:
        index = torch.empty(S, dtype=torch.int32, device=score.device)
    if local_label is None:
        local_label = torch.empty(B, dtype=torch.int64, device=score.device)
    ws = torch.empty(max(lib.pfr_pfc_sample_ws_bytes(C), 4), dtype=torch.uint8, device=score.device)
    lib.pfr_pfc_sample(_p(label), B, _p(score), C, S, _p(index), _p(local_label), _p(ws), _stream())
    return index, local_label


def l2norm_gather_fwd(w, index, out_dtype, spad=None, want_t=False):
    """w fp32 [C, D], index int32 [S] -> (wn [Spad, D] out_dtype with rows S.. zero, wnT [D, Spad] or None, inv fp32 [S]):
    row s is row index[s] of l2norm_fwd(w, out_dtype, want_t) bit for bit"""
    _chk_t(w, "w", torch.float32)
    _chk_t(index, "index", torch.int32)
    C, D = w.shape
    S = index.numel()
    spad = S if spad is None else int(spad)
    wn = torch.empty((spad, D), dtype=out_dtype, device=w.device)
    wnT = torch.empty((D, spad), dtype=out_dtype, device=w.device) if want_t else None
    inv = torch.empty(S, dtype=torch.float32, device=w.device)
    lib.pfr_l2norm_gather_fwd(_p(w), _p(index), _p(wn), _p(wnT), dtype_id(out_dtype), _p(inv), S, spad, C, D, spad, 1e-12, _stream())
    return wn, wnT, inv


def l2norm_gather_bwd(w, index, inv, dwn, dense_out=None, prev_index=None):
    """l2norm_bwd on the gathered rows: dwn fp32 [>= S, D] -> rows fp32 [S, D]; with `dense_out` (fp32 [C, D], zeroed once by the caller) the
    rows go to dense_out[index] instead and the rows of `prev_index` (the index of the call that last wrote it) outside index are re-zeroed"""
    _chk_t(w, "w", torch.float32)
    _chk_t(index, "index", torch.int32)
    C, D = w.shape
    S = index.numel()
    _chk_t(inv, "inv", torch.float32, (S,))
    _chk(dwn, "dwn")
    if dwn.dtype != torch.float32 or dwn.dim() != 2 or dwn.shape[0] < S or dwn.shape[1] != D:
        raise PfrError(f"l2norm_gather_bwd: dwn must be fp32 [>= {S}, {D}], got {dwn.dtype} {tuple(dwn.shape)}")
    if dense_out is None:
        if prev_index is not None:
            raise PfrError("l2norm_gather_bwd: prev_index belongs to the dense mode")
        out = torch.empty((S, D), dtype=torch.float32, device=w.device)
    else:
        _chk_t(dense_out, "dense_out", torch.float32, (C, D))
        out = dense_out
        if prev_index is not None:
            _chk_t(prev_index, "prev_index", torch.int32)
    lib.pfr_l2norm_gather_bwd(_p(w), _p(index), _p(inv), _p(dwn), _p(out), S, C, D, int(dense_out is not None), _p(prev_index),
                              0 if prev_index is None else prev_index.numel(), _stream())
    return out


def sgd_step_rows(p, index, rows, mom, lr, momentum, weight_decay, clip_coef=None, clip_value=0.0, grad_scale=1.0):
    """SGD on the rows p[index] only (p, mom fp32 [C, D]; rows fp32 [S, D]; mom zero-initialised, None when momentum == 0):
    g = clamp(rows * grad_scale * clip_coef, ±clip_value) + weight_decay * p[r]; mom[r] = momentum * mom[r] + g; p[r] -= lr * mom[r]"""
    _chk_t(p, "p", torch.float32)
    _chk_t(index, "index", torch.int32)
    C, D = p.shape
    S = index.numel()
    _chk_t(rows, "rows", torch.float32, (S, D))
    if mom is not None:
        _chk_t(mom, "mom", torch.float32, (C, D))
    lib.pfr_sgd_step_rows(_p(p), _p(index), _p(rows), _p(mom), S, C, D, float(lr), float(momentum), float(weight_decay), float(grad_scale),
                          _p(clip_coef), float(clip_value), _stream())
