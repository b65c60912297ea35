"""AdaFace and CurricularFace in the fused head, on the device.

Kernel level, through the C-ABI: the cosine matrices, the inverse norms and the state are given directly as fp32 inputs and the reference
is an fp64 restatement, written here from the definitions, of the same fp32 inputs.  Tolerances are those tests/test_head_criterion_gpu.py
uses for this row kernel: logits rtol 1e-5 / atol 1e-4, loss 1e-4 * max(1, |loss|), dcos relative L2 < 1e-4, and the bf16 dcos is the
fp32 dcos rounded to nearest even.  Shapes: B in {1, 2, 67} x C in {1037, 4099} (256- and 1024-thread rows, ldc 1040 / 4104 padded for
both dtypes); pfr_margin_prepare alone also at B = 1025 (more rows than its 256 threads, four and a bit strides).

Branch decisions of fp32 and fp64 can differ only within rounding distance of a threshold (a negative against cos(theta_t + m), the
target against cos(pi - m), AdaFace's clamp and clip edges): rows with an entry within 1e-6 of one are dropped, at most 2 % of a case's
rows and none when B <= 8 (asserted).  Checked on the CPU for SEED below: 0 rows in the band and 0 logits of an fp32 restatement outside
the tolerance in all 24 cases; at B = 67 62-66 % of the uniform set's negatives are hard for CurricularFace and 26-27 % of the peaked
set's, so both branches are exercised.

pfr_margin_prepare's statistics and margins against fp64: the bound is four times what torch's own float32 ops on the CPU differ from
fp64 on the same inputs.  Measured on the CPU over the four B of `test_prepare_vs_fp64` with its seeds, the worst case each:
mean() of the norms 2.5e-8 relative (B = 1), std() 8.5e-8 relative (B = 2), mean() of the target cosines 2.5e-7 relative (B = 1025),
the margins {g_ang, g_add} computed from those float32 ops 1.3e-7 absolute (B = 1025); hence the four *_BOUND constants.
Module level: against the CPU module in fp64, 1e-4 on the loss and 1e-3 relative on the gradients."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic")
S, EPS = 64.0, 1e-3
M = {"adaface": 0.4, "curricular": 0.5}
MEAN_BOUND, STD_BOUND, TARGET_MEAN_BOUND = 4 * 2.5e-8, 4 * 8.5e-8, 4 * 2.5e-7       # relative
MARGIN_BOUND = 4 * 1.3e-7                                                         # absolute
SEED = 103
LDC = {1037: 1040, 4099: 4104}
CRITERIA = {
    "ce": dict(),
    "focal_g2": dict(gamma=2.0),
    "weight": dict(weight=True),
    "smooth": dict(smoothing=0.1),
    "weight_smooth_sum": dict(weight=True, smoothing=0.1, reduction="sum"),
    "sum": dict(reduction="sum"),
}


def ops():
    from pets_face_recognition_amd._hip import ops as o
    return o


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------------------------------------ the definitions (dtype of the inputs)
def prepare_ref(kind, inv_norm, cos, label, state, m, h=0.333, momentum=0.01, eps=EPS, update=True):
    """-> (row_margin [B, 2] or None, state after the call)"""
    if kind == "curricular":
        t = state[0]
        if update:
            t = momentum * cos[torch.arange(len(label)), label].clamp(-1.0, 1.0).mean() + (1.0 - momentum) * t
        return None, (t,)
    bm, bs = state
    a = (1.0 / inv_norm).clip(1e-3, 100.0)
    if update:
        bm = momentum * a.mean() + (1.0 - momentum) * bm
        if a.numel() > 1:
            bs = momentum * a.std(unbiased=True) + (1.0 - momentum) * bs
    k = (h * (a - bm) / (bs + eps)).clip(-1.0, 1.0)
    return torch.stack([-m * k, m + m * k], 1), (bm, bs)


def logits_ref(kind, cos, label, row_margin, t, m, s=S, eps=EPS):
    rows = torch.arange(len(label))
    hot = F.one_hot(label, cos.shape[1]).bool()
    if kind == "adaface":
        c = cos.clamp(-1.0 + eps, 1.0 - eps)
        theta = torch.acos(c[rows, label])
        phi = torch.cos((theta + row_margin[:, 0]).clip(eps, math.pi - eps)) - row_margin[:, 1]
        return s * torch.where(hot, phi[:, None], c)
    c = cos.clamp(-1.0, 1.0)
    ct = c[rows, label]
    phi = ct * math.cos(m) - torch.sqrt((1.0 - ct * ct).clamp_min(0.0)) * math.sin(m)
    target = torch.where(ct > math.cos(math.pi - m), phi, ct - m * math.sin(math.pi - m))
    neg = torch.where(c.detach() > phi.detach()[:, None], c * (t + c), c)
    return s * torch.where(hot, target[:, None], neg)


def rows_near_a_threshold(kind, cos, label, row_margin, m, eps=EPS, band=1e-6):
    """bool [B]: the row holds an entry within `band` of a branch threshold (fp64 arithmetic on the fp32 inputs)"""
    cos = cos.double()
    rows = torch.arange(len(label))
    ct = cos[rows, label]
    if kind == "adaface":
        near = ((cos.abs() - (1.0 - eps)).abs() < band).any(1)
        tp = torch.acos(ct.clamp(-1.0 + eps, 1.0 - eps)) + row_margin.double()[:, 0]
        return near | ((tp - eps).abs() < band) | ((tp - (math.pi - eps)).abs() < band)
    phi = ct * math.cos(m) - torch.sqrt(1.0 - ct * ct) * math.sin(m)
    d = (cos - phi[:, None]).abs()
    d[rows, label] = 1.0
    return (d < band).any(1) | ((ct - math.cos(math.pi - m)).abs() < band)


def criterion_ref(logits, label, gamma=0.0, weight=None, smoothing=0.0, reduction="mean"):
    if weight is None and smoothing == 0.0 and reduction == "mean":
        logp = F.cross_entropy(logits, label, reduction="none")
        return (((1.0 - torch.exp(-logp)) ** gamma) * logp).mean()
    return F.cross_entropy(logits, label, weight=weight, label_smoothing=smoothing, reduction=reduction)


# ------------------------------------------------------------------------------------------------ inputs
def make_case(kind, B, C, dist, seed):
    """fp32 inputs of one case: cosines ('uniform' in (-0.99, 0.99), or 'peaked': sigma 0.05 around 0 with targets in (0.3, 0.9)), labels,
    inverse norms of norms in (5, 40), class weights.  At B = 67 rows 0-3 exercise AdaFace's edges: targets beyond the clamp with norms
    that saturate k (with the state (22, 5): both clips active), and negatives at and beyond +-1."""
    g = torch.Generator().manual_seed(seed)
    label = torch.randint(0, C, (B,), generator=g)
    if dist == "uniform":
        cos = 1.98 * torch.rand(B, C, generator=g) - 0.99
    else:
        cos = 0.05 * torch.randn(B, C, generator=g)
        cos[torch.arange(B), label] = 0.3 + 0.6 * torch.rand(B, generator=g)
    norm = 5.0 + 35.0 * torch.rand(B, generator=g)
    if B >= 8:
        cos[0, label[0]], norm[0] = 0.9995, 39.0
        cos[1, label[1]], norm[1] = -0.9995, 5.5
        cos[2, (label[2] + 1) % C] = 1.0
        cos[3, (label[3] + 1) % C] = -0.9996
    weight = 0.25 + 2.0 * torch.rand(C, generator=g)
    return cos, label, 1.0 / norm, weight


def initial_state(kind, dist):
    if kind == "adaface":
        return (22.0, 5.0) if dist == "uniform" else (20.0, 100.0)      # k saturates on many rows / on none
    return (0.35,) if dist == "uniform" else (0.0,)


def _padded(cos, ldc, fill=0.0):
    out = torch.full((cos.shape[0], ldc), fill)
    out[:, :cos.shape[1]] = cos
    return out


def _state_dev(state):
    return tuple(torch.tensor([v], dtype=torch.float32, device=DEV) for v in state)


def _ce_raw(kind, cosd, labeld, C, m, rm, su, gamma=0.0, weight=None, smoothing=0.0, gs=1.0, gs_dev=None, gs_dev2=None, dcos_dtype=None):
    """pfr_margin_ce_adaptive into NaN-filled outputs (the wrappers of _hip/ops.py allocate their own) -> (logits, rows, stats, dcos)"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    B, ldc = cosd.shape
    nan = lambda *shape, dt=torch.float32: torch.full(shape, float("nan"), dtype=dt, device=DEV)
    logits, rows, stats = nan(B, C), nan(B), nan(B, 4)
    dcos = None if dcos_dtype is None else nan(B, ldc, dt=dcos_dtype)
    p = lambda t: 0 if t is None else t.data_ptr()
    lib.pfr_margin_ce_adaptive(p(cosd), p(labeld), B, C, ldc, ops().MARGIN_KINDS[kind], S, m, EPS, gamma, p(weight), smoothing, p(rm), p(su), gs,
                               p(gs_dev), p(gs_dev2), p(logits), p(rows), p(stats), p(dcos), 0 if dcos is None else dtype_id(dcos_dtype),
                               torch.cuda.current_stream().cuda_stream)
    return logits, rows, stats, dcos


def _device_criterion(kind, cosd, labeld, C, m, rm, su, crit, weightd, dcos_dtype):
    """forward + backward as losses/_head_hip.py:MarginCEFunction chains them"""
    o = ops()
    B = cosd.shape[0]
    gamma, smoothing, reduction = crit.get("gamma", 0.0), crit.get("smoothing", 0.0), crit.get("reduction", "mean")
    w = weightd if crit.get("weight") else None
    logits, rows, stats, _ = _ce_raw(kind, cosd, labeld, C, m, rm, su, gamma, w, smoothing)
    plain = w is None and smoothing == 0.0 and reduction == "mean"
    inv = None
    if plain:
        loss, gs = o.mean(rows), 1.0 / B
    elif reduction == "sum":
        (loss, _), gs = o.loss_reduce(rows, None, "sum"), 1.0
    else:
        (loss, inv), gs = o.loss_reduce(rows, stats, "weighted_mean"), 1.0
    one = torch.ones((), device=DEV)
    wce = w is not None or smoothing != 0.0
    _, _, _, dcos = _ce_raw(kind, cosd, labeld, C, m, rm, su, gamma, w, smoothing, gs, one, inv if wce else None, dcos_dtype)
    torch.cuda.synchronize()
    return logits, rows, loss, dcos


@pytest.mark.parametrize("dist", ["uniform", "peaked"])
@pytest.mark.parametrize("C", [1037, 4099])
@pytest.mark.parametrize("B", [1, 2, 67])
@pytest.mark.parametrize("kind", ["adaface", "curricular"])
def test_row_kernel_vs_fp64(kind, B, C, dist):
    """every criterion the entry point accepts, fp32 and bf16 dcos, NaN-filled outputs, pad columns left alone"""
    o = ops()
    m, ldc = M[kind], LDC[C]
    cos, label, inv_norm, weight = make_case(kind, B, C, dist, seed=SEED + B + C)
    cosd, labeld, weightd = _padded(cos, ldc, float("nan")).to(DEV), label.to(DEV), weight.to(DEV)
    state = _state_dev(initial_state(kind, dist))
    rm, su = o.margin_prepare(kind, state, B, inv_norm=inv_norm.to(DEV), cosv=cosd, label=labeld, m=m, h=0.333, momentum=0.01, eps=EPS)
    torch.cuda.synchronize()
    rm64 = None if rm is None else rm.cpu().double()
    t64 = su.cpu().double()[0]
    keep = ~rows_near_a_threshold(kind, cos, label, rm64, m)
    dropped = B - int(keep.sum())
    assert dropped <= (0 if B <= 8 else int(0.02 * B)), f"{dropped} of {B} rows within 1e-6 of a threshold"
    if kind == "adaface" and B >= 8:
        k = -rm64[:, 0] / m
        assert (abs(k[0] - 1.0) < 1e-6 and abs(k[1] + 1.0) < 1e-6) == (dist == "uniform")      # the rows built for the clips
    for name, crit in CRITERIA.items():
        w64 = weight.double() if crit.get("weight") else None
        cos64 = cos.double().requires_grad_(True)
        logits_r = logits_ref(kind, cos64, label, rm64, t64, m)
        # the loss over the kept rows only is not the kernel's loss: rows in the band are compared nowhere, the scalar needs them all
        loss_r = criterion_ref(logits_r, label, crit.get("gamma", 0.0), w64, crit.get("smoothing", 0.0), crit.get("reduction", "mean"))
        loss_r.backward()
        logits, rows, loss, dcos = _device_criterion(kind, cosd, labeld, C, m, rm, su, crit, weightd, torch.float32)
        _, _, _, dcos16 = _device_criterion(kind, cosd, labeld, C, m, rm, su, crit, weightd, torch.bfloat16)
        figs = dict(loss=loss.item(), loss_ref=loss_r.item(), dcos=rel_err(dcos[:, :C][keep], cos64.grad[keep]), dropped=dropped)
        print(f"adaptive margin {kind} {dist} B={B} C={C} {name}: {figs}")
        assert torch.allclose(logits.cpu().double()[keep], logits_r.detach()[keep], rtol=1e-5, atol=1e-4)
        assert torch.isfinite(rows).all()
        if dropped == 0:
            assert abs(loss.item() - loss_r.item()) < 1e-4 * max(1.0, abs(loss_r.item()))
        assert figs["dcos"] < 1e-4
        assert torch.isfinite(dcos[:, :C]).all() and torch.isnan(dcos[:, C:]).all()       # every class written, no pad column touched
        assert torch.isnan(dcos16[:, C:]).all()
        assert torch.equal(dcos16[:, :C], dcos[:, :C].bfloat16())
    # the wrapper zero-fills the pad columns the GEMMs of the backward read
    _, _, _, dz = o.margin_ce_adaptive(cosd, labeld, C, kind, S, m, EPS, rm, su, grad_scale=1.0 / B, dcos_dtype=torch.bfloat16)
    assert torch.count_nonzero(dz[:, C:]).item() == 0
    if kind == "curricular":
        hard = cos > (cos[torch.arange(B), label].double() * math.cos(m)
                      - torch.sqrt(1 - cos[torch.arange(B), label].double() ** 2) * math.sin(m))[:, None]
        hard[torch.arange(B), label] = False
        frac = hard.sum().item() / (B * (C - 1))
        print(f"  hard negatives: {frac:.3f}")
        if B == 67:
            assert 0.0 < frac < 1.0


@pytest.mark.parametrize("kind", ["adaface", "curricular"])
def test_standalone_backward_vs_fp64(kind):
    o = ops()
    B, C, m = 67, 1037, M[kind]
    cos, label, inv_norm, _ = make_case(kind, B, C, "uniform", seed=7)
    cosd, labeld = _padded(cos, LDC[C]).to(DEV), label.to(DEV)
    rm, su = o.margin_prepare(kind, _state_dev(initial_state(kind, "uniform")), B, inv_norm=inv_norm.to(DEV), cosv=cosd, label=labeld, m=m,
                              h=0.333)
    dlogits = torch.randn(B, C, generator=torch.Generator().manual_seed(8))
    cos64 = cos.double().requires_grad_(True)
    logits_ref(kind, cos64, label, None if rm is None else rm.cpu().double(), su.cpu().double()[0], m).backward(dlogits.double())
    keep = ~rows_near_a_threshold(kind, cos, label, None if rm is None else rm.cpu().double(), m)
    assert keep.sum().item() >= B - 1
    d32 = o.margin_bwd_adaptive(cosd, labeld, C, kind, S, m, EPS, rm, su, dlogits.to(DEV), torch.float32)
    d16 = o.margin_bwd_adaptive(cosd, labeld, C, kind, S, m, EPS, rm, su, dlogits.to(DEV), torch.bfloat16)
    torch.cuda.synchronize()
    assert rel_err(d32[:, :C][keep], cos64.grad[keep]) < 1e-4
    assert torch.equal(d16, d32.bfloat16()) and torch.count_nonzero(d32[:, C:]).item() == 0


@pytest.mark.parametrize("B", [1, 2, 67, 1025])
@pytest.mark.parametrize("kind", ["adaface", "curricular"])
def test_prepare_vs_fp64(kind, B):
    """the batch statistics themselves (momentum 1 makes the buffers the statistics), the EMA step, the margins and state_used; two
    launches from the same state give the same bits; update = 0 leaves the state alone"""
    o = ops()
    C, m = 1037, M[kind]
    cos, label, inv_norm, _ = make_case(kind, B, C, "uniform", seed=300 + B)
    cosd, labeld, invd = _padded(cos, LDC[C]).to(DEV), label.to(DEV), inv_norm.to(DEV)
    s0 = initial_state(kind, "uniform")
    for momentum in (1.0, 0.01):
        runs = []
        for _ in range(2):
            state = _state_dev(s0)
            rm, su = o.margin_prepare(kind, state, B, inv_norm=invd, cosv=cosd, label=labeld, m=m, h=0.333, momentum=momentum, eps=EPS)
            torch.cuda.synchronize()
            runs.append((rm, su, state))
        for a, b in zip(runs[0][2] + (runs[0][1],), runs[1][2] + (runs[1][1],)):
            assert torch.equal(a, b)
        assert rm is None or torch.equal(runs[0][0], runs[1][0])
        rm_r, state_r = prepare_ref(kind, inv_norm.double(), cos.double(), label, tuple(torch.tensor(v, dtype=torch.float64) for v in s0), m,
                                    momentum=momentum)
        errs = [abs(d.item() - r.item()) / abs(r.item()) for d, r in zip(state, state_r)]
        print(f"prepare {kind} B={B} momentum={momentum}: state {[d.item() for d in state]} rel err {errs}")
        assert all(e <= b for e, b in zip(errs, (MEAN_BOUND, STD_BOUND) if kind == "adaface" else (TARGET_MEAN_BOUND,)))
        assert all(su[i].item() == state[i].item() for i in range(len(state)))         # the step used the buffers after the update
        if kind == "adaface":
            if B == 1:
                assert state[1].item() == s0[1]                                         # the deviation of one sample: the buffer stays
            # the margins follow from the fp32 buffers the kernel stored: restate them from those
            rm_r, _ = prepare_ref(kind, inv_norm.double(), None, None, tuple(d.cpu().double()[0] for d in state), m, update=False)
            err = (rm.cpu().double() - rm_r).abs().max().item()
            print(f"  row_margin max abs err {err:.3e}")
            assert rm.shape == (B, 2) and err <= MARGIN_BOUND
        else:
            assert su[1].item() == 0.0
    state = _state_dev(s0)
    rm2, su2 = o.margin_prepare(kind, state, B, inv_norm=invd, cosv=cosd, label=labeld, m=m, h=0.333, update=False)
    torch.cuda.synchronize()
    assert [d.item() for d in state] == [torch.tensor(v).item() for v in s0] and su2[0].item() == state[0].item()


def test_existing_entry_points_keep_their_bits():
    """pfr_margin_ce against pfr_margin_ce_ex with every option off and pfr_margin_bwd against the row kernel's dcos of a unit loss
    gradient, as before this change (tests/test_head_criterion_gpu.py::test_default_path_untouched), and against fp64"""
    o = ops()
    from pets_face_recognition_amd._hip import lib, dtype_id
    for B, C in ((67, 1037), (2, 4099)):
        cos, label, _, _ = make_case("curricular", B, C, "uniform", seed=9)
        cosd, labeld = _padded(cos, LDC[C]).to(DEV), label.to(DEV)
        for dt in (torch.float32, torch.bfloat16):
            for gamma in (0.0, 2.0):
                lg0, rows0, dc0 = o.margin_ce(cosd, labeld, C, "arc", S, 0.5, gamma=gamma, grad_scale=1.0 / B, dcos_dtype=dt)
                lg1, rows1, _, dc1 = o.margin_ce_ex(cosd, labeld, C, "arc", S, 0.5, gamma=gamma, grad_scale=1.0 / B, dcos_dtype=dt)
                torch.cuda.synchronize()
                assert torch.equal(lg0, lg1) and torch.equal(rows0, rows1) and torch.equal(dc0, dc1)
        c64 = cos.double()
        ct = c64[torch.arange(B), label]
        phi = ct * math.cos(0.5) - torch.sqrt(1 - ct * ct) * math.sin(0.5)
        want = S * torch.where(F.one_hot(label, C).bool(), torch.where(ct > math.cos(math.pi - 0.5), phi, ct - 0.5 * math.sin(math.pi - 0.5))[:, None], c64)
        assert torch.allclose(lg0.cpu().double(), want, rtol=1e-5, atol=1e-4)
        # pfr_margin_bwd of a unit gradient: s on the negatives, s * d phi / d cos on the target
        dl = torch.ones(B, C, device=DEV)
        dcb = torch.zeros(B, LDC[C], device=DEV)
        lib.pfr_margin_bwd(cosd.data_ptr(), labeld.data_ptr(), B, C, LDC[C], 0, S, 0.5, dl.data_ptr(), dcb.data_ptr(), dtype_id(torch.float32),
                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        dphi = torch.where(ct > math.cos(math.pi - 0.5), math.cos(0.5) + math.sin(0.5) * ct / torch.sqrt(1 - ct * ct), torch.ones_like(ct))
        want_d = S * torch.where(F.one_hot(label, C).bool(), dphi[:, None], torch.ones_like(c64))
        assert rel_err(dcb[:, :C], want_d) < 1e-6


# ------------------------------------------------------------------------------------------------ module level
def _forbid_fallback(monkeypatch, wrap):
    def boom(*a, **k):
        raise AssertionError("the fused head fell back to the unfused criterion")
    monkeypatch.setattr(F, "cross_entropy", boom)
    monkeypatch.setattr(torch, "log_softmax", boom)
    monkeypatch.setattr(F, "log_softmax", boom)
    monkeypatch.setattr(wrap, "_unfused", boom, raising=False)
    monkeypatch.setattr(wrap.focal_loss, "forward", boom)


def _build_pair(margin, C, K, g, is_focal=False, loss_kwargs=None, state=None):
    """the same head on the CPU in fp64 and on the device with fp32 compute"""
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    w0 = torch.randn(C * K, 512, generator=g) * 0.05
    wraps = []
    for device in ("cpu", DEV):
        wrap = SoftmaxBasedMetricLearning(nn.Identity(), C, 512, is_focal=is_focal, loss_kwargs=dict(loss_kwargs or {}), margin=margin,
                                          sub_centers=K)
        with torch.no_grad():
            wrap.add_margin.weight.copy_(w0)
            for name, v in (state or {}).items():
                getattr(wrap.add_margin, name).fill_(v)
        if device == "cpu":
            wrap = wrap.double()
        else:
            wrap.add_margin.compute_dtype = torch.float32
            wrap = wrap.to(DEV)
        wraps.append(wrap.train())
    return wraps


def _buffers(wrap):
    h = wrap.add_margin
    return [h.batch_mean, h.batch_std] if hasattr(h, "batch_mean") else [h.t]


def _inputs(B, C, g, w=None, K=1):
    label = torch.randint(0, C, (B,), generator=g)
    x = torch.randn(B, 512, generator=g)
    if w is not None:       # pulled towards the class centre: target cosines around 0.5, hard and easy negatives
        x = F.normalize(x) + 0.6 * F.normalize(w[label * K])
    return x * (5.0 + 35.0 * torch.rand(B, 1, generator=g)) / x.norm(dim=1, keepdim=True), label


MODULE_STATE = {"adaface": dict(batch_mean=22.0, batch_std=5.0), "curricular": dict(t=0.3)}


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("loss_kwargs", [dict(), dict(label_smoothing=0.1)], ids=["ce", "smooth"])
@pytest.mark.parametrize("margin", ["adaface", "curricular"])
def test_module_vs_cpu_fp64_without_fallback(margin, loss_kwargs, K, monkeypatch):
    B, C = 32, 300
    g = torch.Generator().manual_seed(41)
    ref, wrap = _build_pair(margin, C, K, g, loss_kwargs=loss_kwargs, state=MODULE_STATE[margin])
    x, label = _inputs(B, C, g, ref.add_margin.weight.detach().float(), K)
    x64 = x.double().requires_grad_(True)
    r64 = ref(x64, label)
    r64["loss"].backward()
    assert wrap._fusable(x.to(DEV)) is not None
    _forbid_fallback(monkeypatch, wrap)
    xd = x.to(DEV).requires_grad_(True)
    r = wrap(xd, label.to(DEV))
    r["loss"].backward()
    torch.cuda.synchronize()
    figs = dict(loss=r["loss"].item(), loss_ref=r64["loss"].item(), logits=rel_err(r["logits"], r64["logits"]), dx=rel_err(xd.grad, x64.grad),
                dw=rel_err(wrap.add_margin.weight.grad, ref.add_margin.weight.grad))
    print(f"adaptive module {margin} K={K} {loss_kwargs}: {figs}")
    assert r["loss"].is_cuda and r["logits"].shape == (B, C)
    assert figs["logits"] < 1e-3
    assert abs(figs["loss"] - figs["loss_ref"]) < 1e-4 * max(1.0, abs(figs["loss_ref"]))
    assert figs["dx"] < 1e-3 and figs["dw"] < 1e-3
    for b, b64 in zip(_buffers(wrap), _buffers(ref)):
        assert b.dtype == torch.float32 and abs(b.item() - b64.item()) < 1e-5 * abs(b64.item())
    if K > 1:
        assert torch.equal(wrap.add_margin.sub_center_count.cpu(), ref.add_margin.sub_center_count)


@pytest.mark.parametrize("margin", ["adaface", "curricular"])
def test_learnable_alpha_takes_the_unfused_path(margin):
    B, C = 32, 300
    g = torch.Generator().manual_seed(43)
    ref, wrap = _build_pair(margin, C, 1, g, is_focal=True, loss_kwargs=dict(gamma=2, alpha=True), state=MODULE_STATE[margin])
    a0 = 0.5 + torch.rand(C, generator=g)
    with torch.no_grad():
        ref.focal_loss.alpha.copy_(a0)
        wrap.focal_loss.alpha.copy_(a0)
    x, label = _inputs(B, C, g, ref.add_margin.weight.detach().float())
    x64 = x.double().requires_grad_(True)
    r64 = ref(x64, label)
    r64["loss"].backward()
    xd = x.to(DEV).requires_grad_(True)
    assert wrap._fusable(xd) is None
    r = wrap(xd, label.to(DEV))
    r["loss"].backward()
    torch.cuda.synchronize()
    assert abs(r["loss"].item() - r64["loss"].item()) < 1e-4 * max(1.0, abs(r64["loss"].item()))
    assert rel_err(r["logits"], r64["logits"]) < 1e-3 and rel_err(xd.grad, x64.grad) < 1e-3
    assert rel_err(wrap.add_margin.weight.grad, ref.add_margin.weight.grad) < 1e-3
    assert rel_err(wrap.focal_loss.alpha.grad, ref.focal_loss.alpha.grad) < 1e-3


@pytest.mark.parametrize("margin", ["adaface", "curricular"])
def test_head_only_training_follows_cpu_fp64(margin):
    """five SGD steps on an embedding table and the head weight: device fp32 against the CPU in fp64, buffers included"""
    N, C = 64, 40
    g = torch.Generator().manual_seed(47)
    ref, wrap = _build_pair(margin, C, 1, g, loss_kwargs=dict(label_smoothing=0.1))
    t0, label = _inputs(N, C, g)
    traces, bufs = [], []
    for w, device, dt in ((ref, "cpu", torch.float64), (wrap, DEV, torch.float32)):
        table = t0.to(device, dt).requires_grad_(True)
        opt = torch.optim.SGD([table] + list(w.parameters()), lr=0.05, momentum=0.9)
        losses, trace = [], []
        for _ in range(5):
            opt.zero_grad()
            r = w(table, label.to(device))
            r["loss"].backward()
            opt.step()
            losses.append(r["loss"].item())
            trace.append([b.item() for b in _buffers(w)])
        traces.append(losses)
        bufs.append(trace)
    print(f"head-only training {margin}: cpu fp64 {traces[0]}\n device {traces[1]}\n buffers {bufs[0][-1]} / {bufs[1][-1]}")
    for a, b in zip(traces[1], traces[0]):
        assert abs(a - b) <= 1e-3 * abs(b), (traces[1], traces[0])
    for ta, tb in zip(bufs[1], bufs[0]):
        for a, b in zip(ta, tb):
            assert abs(a - b) <= 1e-5 * max(abs(b), 1e-2), (bufs[1], bufs[0])
    assert bufs[0][-1] != bufs[0][0]


@pytest.mark.parametrize("margin", ["adaface", "curricular"])
def test_two_forwards_then_two_backwards(margin):
    """state_used / row_margin are saved per call: the second forward moves the buffers, the first backward still differentiates the first
    forward.  The momentum is large so that the two steps' states differ by far more than any tolerance."""
    B, C = 32, 300
    g = torch.Generator().manual_seed(53)
    kw = dict(t_alpha=0.9) if margin == "adaface" else dict(momentum=0.9)
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    wrap = SoftmaxBasedMetricLearning(nn.Identity(), C, 512, margin=margin, margin_kwargs=kw)
    wrap.add_margin.compute_dtype = torch.float32
    wrap = wrap.to(DEV).train()
    if margin == "adaface":
        wrap.add_margin.batch_std.fill_(5.0)
    w = wrap.add_margin.weight.detach().cpu()
    (x1, l1), (x2, l2) = _inputs(B, C, g, w), _inputs(B, C, g, w)
    x2 = x2 * 0.5                                                      # other norms, hence another batch_mean
    start = [b.clone() for b in _buffers(wrap)]

    def run(interleaved):
        for b, v in zip(_buffers(wrap), start):
            b.copy_(v)
        xs = [x.to(DEV).requires_grad_(True) for x in (x1, x2)]
        grads = []
        if interleaved:
            losses = [wrap(x, l.to(DEV))["loss"] for x, l in zip(xs, (l1, l2))]
            for loss in losses:
                wrap.add_margin.weight.grad = None
                loss.backward()
                grads.append(wrap.add_margin.weight.grad.clone())
        else:
            for x, l in zip(xs, (l1, l2)):
                wrap.add_margin.weight.grad = None
                wrap(x, l.to(DEV))["loss"].backward()
                grads.append(wrap.add_margin.weight.grad.clone())
        torch.cuda.synchronize()
        return grads + [x.grad for x in xs], [b.clone() for b in _buffers(wrap)]

    sep, buf_sep = run(False)
    mid = [b.clone() for b in _buffers(wrap)]
    inter, buf_inter = run(True)
    assert all(torch.equal(a, b) for a, b in zip(sep, inter))
    assert all(torch.equal(a, b) for a, b in zip(buf_sep, buf_inter))
    assert all(abs(a.item() - b.item()) > 1e-2 for a, b in zip(start, mid))                      # the buffers did move between the steps


@pytest.mark.parametrize("name", ["fe_r18_mi355x_adaface.py", "fe_r18_mi355x_curricular.py"])
def test_main_with_new_configs(name, tmp_path):
    env = dict(os.environ, PFR_LIMIT_TRAIN_BATCHES="8")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--config", os.path.join(SYNTH, name)], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Completed!" in r.stdout
    losses = [float(l.split("loss")[1]) for l in r.stdout.splitlines() if l.startswith("epoch") and "loss" in l]
    assert losses and all(math.isfinite(l) for l in losses)
