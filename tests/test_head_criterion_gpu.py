"""The criterion-general fused head on the device: adaptive-alpha focal loss, class weights, label smoothing and reduction='sum' inside
the margin + cross-entropy row kernel, and the column kernel of d loss / d alpha.

References are computed here, on the CPU in fp64, from the formulas of the reference's classes (ArcMarginProduct / AddMarginProduct,
FocalLoss with `input = alpha * input`) and torch's own F.cross_entropy(weight=, label_smoothing=, reduction=).
Tolerances at kernel level are those of tests/test_kernels_gpu.py::test_margin_ce_and_l2norm for this kernel: logits rtol 1e-5 / atol 1e-4,
loss 1e-4 * max(1, |loss|), gradients relative L2 error < 1e-4; at module level 1e-3 (the bound of the adaptive-alpha golden test)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SYNTH = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic")

CRITERIA = {
    "alpha_g0": dict(alpha=True, gamma=0.0),
    "alpha_g2": dict(alpha=True, gamma=2.0),
    "weight": dict(weight=True),
    "smooth": dict(smoothing=0.1),
    "weight_smooth": dict(weight=True, smoothing=0.1),
    "weight_sum": dict(weight=True, reduction="sum"),
}


def ops():
    from pets_face_recognition_amd._hip import ops as o
    return o


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _margin_logits64(cos, label, mode, s, m):
    """s * (onehot * phi + (1 - onehot) * cos) in the dtype of `cos` (fp64 here)"""
    if mode == "cos":
        phi = cos - m
    else:
        sine = torch.sqrt((1.0 - cos * cos).clamp_min(0.0))
        phi = cos * math.cos(m) - sine * math.sin(m)
        if mode == "arc_easy":
            phi = torch.where(cos > 0, phi, cos)
        else:
            phi = torch.where(cos > math.cos(math.pi - m), phi, cos - math.sin(math.pi - m) * m)
    oh = F.one_hot(label, cos.shape[1]).to(cos.dtype)
    return s * (oh * phi + (1.0 - oh) * cos)


def _criterion64(logits, label, gamma=0.0, alpha=None, weight=None, smoothing=0.0, reduction="mean"):
    if alpha is not None:
        logp = F.cross_entropy(alpha * logits, label, reduction="none")
        p = torch.exp(-logp)
        return ((1.0 - p) ** gamma * logp).mean()
    if weight is None and smoothing == 0.0 and reduction == "mean":
        logp = F.cross_entropy(logits, label, reduction="none")
        p = torch.exp(-logp)
        return ((1.0 - p) ** gamma * logp).mean()
    return F.cross_entropy(logits, label, weight=weight, label_smoothing=smoothing, reduction=reduction)


def _case(B, C, D, seed, crit):
    """cosines of random embeddings / class centres (fp32 values, the kernel's input), labels, and the criterion's tensors"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g, dtype=torch.float64)
    w = torch.randn(C, D, generator=g, dtype=torch.float64) * 0.05
    label = torch.randint(0, C, (B,), generator=g)
    # push every sample along its class centre by k in [-3, 2] row norms: target cosines from -0.95 to 0.89, on both sides of the easy
    # margin's 0 and of the hard margin's cos(pi - m) = -0.88
    k = 5.0 * torch.rand(B, 1, generator=g, dtype=torch.float64) - 3.0
    x = x + k * F.normalize(w[label]) * x.norm(dim=1, keepdim=True)
    cos = (F.normalize(x) @ F.normalize(w).t()).float()
    alpha = (0.5 + torch.rand(C, generator=g)) if crit.get("alpha") else None
    weight = (0.25 + 2.0 * torch.rand(C, generator=g)) if crit.get("weight") else None
    return cos, label, alpha, weight


def _reference(cos, label, mode, s, m, gamma, alpha, weight, smoothing, reduction):
    cos64 = cos.double().requires_grad_(True)
    a64 = None if alpha is None else alpha.double().requires_grad_(True)
    w64 = None if weight is None else weight.double()
    logits = _margin_logits64(cos64, label, mode, s, m)
    loss = _criterion64(logits, label, gamma, a64, w64, smoothing, reduction)
    loss.backward()
    return logits.detach(), loss.detach(), cos64.grad, None if a64 is None else a64.grad


def _device_head(cosd, labeld, C, mode, s, m, gamma, alpha, weight, smoothing, reduction, dcos_dtype=torch.float32, want_logits=True):
    """forward + backward of the criterion through the C-ABI wrappers, as losses/_head_hip.py:MarginCEFunction chains them"""
    o = ops()
    B = cosd.shape[0]
    logits, rows, stats, _ = o.margin_ce_ex(cosd, labeld, C, mode, s, m, gamma=gamma, alpha=alpha, class_weight=weight,
                                            label_smoothing=smoothing, want_logits=want_logits)
    wce = weight is not None or smoothing != 0.0
    inv = None
    if wce and reduction == "mean":
        loss, inv = o.loss_reduce(rows, stats, "weighted_mean")
        gs = 1.0
    elif reduction == "sum":
        loss, _ = o.loss_reduce(rows, None, "sum")
        gs = 1.0
    else:
        loss = o.mean(rows)
        gs = 1.0 / B
    one = torch.ones((), device=cosd.device)
    _, _, _, dcos = o.margin_ce_ex(cosd, labeld, C, mode, s, m, gamma=gamma, alpha=alpha, class_weight=weight, label_smoothing=smoothing,
                                   grad_scale=gs, grad_scale_dev=one, grad_scale_dev2=inv, want_logits=False, want_stats=False,
                                   dcos_dtype=dcos_dtype)
    dalpha = None if alpha is None else o.alpha_grad(cosd, labeld, alpha, stats, C, s, grad_scale=gs, grad_scale_dev=one)
    torch.cuda.synchronize()
    return logits, loss, dcos, dalpha


def _padded(cos, ldc):
    B, C = cos.shape
    out = torch.zeros(B, ldc)
    out[:, :C] = cos
    return out


def _check_kernels(B, C, ldc, mode, name, seed):
    crit = CRITERIA[name]
    s, m = 64.0, (0.4 if mode == "cos" else 0.5)
    cos, label, alpha, weight = _case(B, C, 512, seed, crit)
    gamma, smoothing, reduction = crit.get("gamma", 0.0), crit.get("smoothing", 0.0), crit.get("reduction", "mean")
    logits_r, loss_r, dcos_r, dalpha_r = _reference(cos, label, mode, s, m, gamma, alpha, weight, smoothing, reduction)
    dev = lambda t: None if t is None else t.to(DEV)
    logits, loss, dcos, dalpha = _device_head(_padded(cos, ldc).to(DEV), label.to(DEV), C, mode, s, m, gamma, dev(alpha), dev(weight),
                                              smoothing, reduction)
    figs = dict(loss=loss.item(), loss_ref=loss_r.item(), dcos=rel_err(dcos[:, :C], dcos_r),
                dalpha=None if dalpha is None else rel_err(dalpha, dalpha_r))
    print(f"head criterion {name} {mode} B={B} C={C} ldc={ldc}: {figs}")
    assert logits.shape == (B, C)
    assert torch.allclose(logits.cpu().double(), logits_r, rtol=1e-5, atol=1e-4)
    assert abs(loss.item() - loss_r.item()) < 1e-4 * max(1.0, abs(loss_r.item()))
    assert figs["dcos"] < 1e-4
    assert torch.count_nonzero(dcos[:, C:]).item() == 0      # padded columns: zero gradient, never a class
    if dalpha is not None:
        assert dalpha.shape == (C,)
        assert figs["dalpha"] < 1e-4


@pytest.mark.parametrize("name", list(CRITERIA))
@pytest.mark.parametrize("mode", ["arc", "arc_easy", "cos"])
def test_criterion_kernels_vs_fp64(mode, name):
    """B = 33, C = 1000: odd sizes, 256-thread rows, 256-thread column blocks"""
    _check_kernels(33, 1000, 1000, mode, name, seed=31)


@pytest.mark.parametrize("name", list(CRITERIA))
def test_criterion_kernels_headline_shape_padded(name):
    """B = 256, C = 10 000 with the cosine operand padded (ldc = 10 008): 1024-thread rows, 1024-thread column blocks"""
    _check_kernels(256, 10000, 10008, "arc", name, seed=32)


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_default_path_untouched(gamma):
    """all options off: the new entry point is pfr_margin_ce, bit for bit (logits, loss rows, fp32 and bf16 dcos)"""
    o = ops()
    for B, C, ldc in ((33, 1000, 1000), (64, 5000, 5008)):
        cos, label, _, _ = _case(B, C, 512, 33, {})
        cosd, labeld = _padded(cos, ldc).to(DEV), label.to(DEV)
        for dt in (torch.float32, torch.bfloat16):
            lg0, rows0, dc0 = o.margin_ce(cosd, labeld, C, "arc", 64.0, 0.5, gamma=gamma, grad_scale=1.0 / B, dcos_dtype=dt)
            lg1, rows1, stats, dc1 = o.margin_ce_ex(cosd, labeld, C, "arc", 64.0, 0.5, gamma=gamma, grad_scale=1.0 / B, dcos_dtype=dt)
            torch.cuda.synchronize()
            assert torch.equal(lg0, lg1) and torch.equal(rows0, rows1) and torch.equal(dc0, dc1)
            assert dc1.dtype == dt
        loss_sum, inv = o.loss_reduce(rows1, None, "mean")
        torch.cuda.synchronize()
        assert torch.equal(loss_sum, o.mean(rows0)) and inv.item() == pytest.approx(1.0 / B, rel=1e-7)


@pytest.mark.parametrize("mode", ["arc", "cos"])
def test_degenerate_options_agree_with_default(mode):
    """alpha = 1 (focal, gamma 0 and 2) and weight = 1 / e = 0 (cross-entropy) give the default criterion's loss and gradients"""
    o = ops()
    B, C = 33, 1000
    m = 0.4 if mode == "cos" else 0.5
    cos, label, _, _ = _case(B, C, 512, 34, {})
    cosd, labeld = cos.to(DEV), label.to(DEV)
    ones = torch.ones(C, device=DEV)
    for gamma, kw in ((0.0, dict(alpha=ones)), (2.0, dict(alpha=ones)), (0.0, dict(weight=ones))):
        lg0, rows0, dc0 = o.margin_ce(cosd, labeld, C, mode, 64.0, m, gamma=gamma, grad_scale=1.0 / B, dcos_dtype=torch.float32)
        loss0 = o.mean(rows0)
        lg1, loss1, dc1, dalpha = _device_head(cosd, labeld, C, mode, 64.0, m, gamma, kw.get("alpha"), kw.get("weight"), 0.0, "mean")
        assert torch.allclose(lg1, lg0, rtol=1e-5, atol=1e-4)
        assert abs(loss1.item() - loss0.item()) < 1e-4 * max(1.0, abs(loss0.item()))
        assert rel_err(dc1, dc0) < 1e-4


def test_alpha_backward_is_deterministic():
    B, C, ldc = 256, 10000, 10008
    cos, label, alpha, _ = _case(B, C, 512, 35, dict(alpha=True))
    cosd, labeld, alphad = _padded(cos, ldc).to(DEV), label.to(DEV), alpha.to(DEV)
    runs = [_device_head(cosd, labeld, C, "arc", 64.0, 0.5, 2.0, alphad, None, 0.0, "mean", want_logits=False) for _ in range(2)]
    assert torch.equal(runs[0][3], runs[1][3]) and torch.equal(runs[0][2], runs[1][2])
    assert torch.isfinite(runs[0][3]).all() and runs[0][3].abs().max().item() > 0


@pytest.mark.parametrize("name", ["alpha_g2", "weight_smooth"])
def test_bf16_dcos_is_the_rounded_fp32_dcos(name):
    crit = CRITERIA[name]
    B, C = 33, 1000
    cos, label, alpha, weight = _case(B, C, 512, 36, crit)
    dev = lambda t: None if t is None else t.to(DEV)
    args = (cos.to(DEV), label.to(DEV), C, "arc", 64.0, 0.5, crit.get("gamma", 0.0), dev(alpha), dev(weight), crit.get("smoothing", 0.0), "mean")
    d32 = _device_head(*args, dcos_dtype=torch.float32)[2]
    d16 = _device_head(*args, dcos_dtype=torch.bfloat16)[2]
    assert d16.dtype == torch.bfloat16
    normal = d32.abs() >= 2.0 ** -126
    err = ((d16.float() - d32).abs() / d32.abs().clamp_min(2.0 ** -126))[normal]
    print(f"bf16 dcos {name}: max rel err {err.max().item():.3e}, bit-equal to the rounded fp32: {torch.equal(d16, d32.bfloat16())}")
    assert err.max().item() <= 2.0 ** -8
    assert (d16.float()[~normal].abs() <= 2.0 ** -125).all()


# ------------------------------------------------------------------------------------------------ module level
MODULE_CASES = {
    "alpha_g0": (True, dict(gamma=0, alpha=True)),
    "alpha_g2": (True, dict(gamma=2, alpha=True)),
    "weight": (False, dict(weight=True)),
    "smooth": (False, dict(label_smoothing=0.1)),
    "weight_smooth": (False, dict(weight=True, label_smoothing=0.1)),
    "weight_sum": (False, dict(weight=True, reduction="sum")),
    "sum": (False, dict(reduction="sum")),
}


def _forbid_fallback(monkeypatch, wrap):
    """a silent fall-back to the unfused head (margin kernels, then torch ops / the criterion module over the B x C logits) raises"""
    def boom(*a, **k):
        raise AssertionError("the fused head fell back to the unfused criterion")
    monkeypatch.setattr(F, "cross_entropy", boom)
    monkeypatch.setattr(torch, "log_softmax", boom)
    monkeypatch.setattr(F, "log_softmax", boom)
    monkeypatch.setattr(wrap, "_unfused", boom, raising=False)
    monkeypatch.setattr(wrap.focal_loss, "forward", boom)      # the criterion module itself only ever runs on the unfused branch


def _build_pair(C, is_focal, kw, arc, g):
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    kw = dict(kw)
    if kw.get("weight"):
        kw["weight"] = 0.25 + 2.0 * torch.rand(C, generator=g)
    w0 = torch.randn(C, 512, generator=g) * 0.05
    a0 = 0.5 + torch.rand(C, generator=g)
    wraps = []
    for device in ("cpu", DEV):
        wrap = SoftmaxBasedMetricLearning(nn.Identity(), C, 512, is_focal=is_focal, loss_kwargs=dict(kw), arc_margin=arc)
        with torch.no_grad():
            wrap.add_margin.weight.copy_(w0)
            if kw.get("alpha"):
                wrap.focal_loss.alpha.copy_(a0)
        if device == "cpu":
            wrap = wrap.double()
        else:
            wrap.add_margin.compute_dtype = torch.float32
            wrap = wrap.to(DEV)
        wraps.append(wrap)
    return wraps


@pytest.mark.parametrize("arc", [True, False])
@pytest.mark.parametrize("name", list(MODULE_CASES))
def test_module_vs_cpu_fp64_without_fallback(name, arc, monkeypatch):
    is_focal, kw = MODULE_CASES[name]
    B, C = 32, 300
    g = torch.Generator().manual_seed(41)
    ref, wrap = _build_pair(C, is_focal, kw, arc, g)
    x = torch.randn(B, 512, generator=g)
    label = torch.randint(0, C, (B,), generator=g)
    x64 = x.double().requires_grad_(True)
    r64 = ref(x64, label)
    r64["loss"].backward()
    _forbid_fallback(monkeypatch, wrap)
    xd = x.to(DEV).requires_grad_(True)
    r = wrap(xd, label.to(DEV))
    r["loss"].backward()
    torch.cuda.synchronize()
    assert r["loss"].is_cuda and r["logits"].shape == (B, C)
    assert rel_err(r["logits"], r64["logits"]) < 1e-3        # the margin output, not alpha * logits
    assert abs(r["loss"].item() - r64["loss"].item()) < 1e-3 * abs(r64["loss"].item())
    assert rel_err(xd.grad, x64.grad) < 1e-3
    assert rel_err(wrap.add_margin.weight.grad, ref.add_margin.weight.grad) < 1e-3
    if kw.get("alpha"):
        assert rel_err(wrap.focal_loss.alpha.grad, ref.focal_loss.alpha.grad) < 1e-3


def test_alpha_golden_cases_without_fallback(monkeypatch):
    """the two adaptive-alpha vectors of the reference's own classes (tests/golden/arcface_alpha.npz) through the fused head"""
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    G = np.load(os.path.join(GOLD, "arcface_alpha.npz"))
    for name in ("arc_hard_alpha", "cosface_alpha"):
        C = G[name + "_w"].shape[0]
        wrap = SoftmaxBasedMetricLearning(nn.Identity(), C, 512, is_focal=True, loss_kwargs=dict(gamma=float(G[name + "_gamma"]), alpha=True),
                                          arc_margin=name.startswith("arc"))
        wrap.add_margin.compute_dtype = torch.float32
        wrap = wrap.to(DEV)
        with torch.no_grad():
            wrap.add_margin.weight.copy_(torch.tensor(G[name + "_w"]))
            wrap.focal_loss.alpha.copy_(torch.tensor(G[name + "_alpha"]))
        x = torch.tensor(G[name + "_x"]).to(DEV).requires_grad_(True)
        assert wrap._fusable(x).alpha is wrap.focal_loss.alpha
        with monkeypatch.context() as mp:
            _forbid_fallback(mp, wrap)
            r = wrap(x, torch.tensor(G[name + "_label"]).to(DEV))
            r["loss"].backward()
            torch.cuda.synchronize()
        assert torch.allclose(r["logits"].cpu(), torch.tensor(G[name + "_logits"]), rtol=1e-4, atol=2e-3), name
        assert abs(r["loss"].item() - float(G[name + "_loss"])) < 1e-4 * max(1, abs(float(G[name + "_loss"]))), name
        assert rel_err(x.grad, torch.tensor(G[name + "_dx"])) < 1e-3, name
        assert rel_err(wrap.add_margin.weight.grad, torch.tensor(G[name + "_dw"])) < 1e-3, name
        assert rel_err(wrap.focal_loss.alpha.grad, torch.tensor(G[name + "_dalpha"])) < 1e-3, name


def test_standalone_focal_loss_with_alpha_vs_fp64():
    """FocalLoss(alpha=True) on CUDA logits: alpha goes into the row kernel and its gradient comes from the column kernel"""
    from pets_face_recognition_amd.losses import FocalLoss
    B, C = 33, 257
    g = torch.Generator().manual_seed(43)
    logits = torch.randn(B, C, generator=g) * 8.0
    label = torch.randint(0, C, (B,), generator=g)
    a0 = 0.5 + torch.rand(C, generator=g)
    l64 = logits.double().requires_grad_(True)
    a64 = a0.double().requires_grad_(True)
    _criterion64(l64, label, 2.0, a64).backward()
    fl = FocalLoss(C, gamma=2, alpha=True).to(DEV)
    with torch.no_grad():
        fl.alpha.copy_(a0)
    ld = logits.to(DEV).requires_grad_(True)
    loss = fl(ld, label.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - _criterion64(l64, label, 2.0, a64).item()) < 1e-4
    assert rel_err(ld.grad, l64.grad) < 1e-4
    assert rel_err(fl.alpha.grad, a64.grad) < 1e-4


@pytest.mark.parametrize("name", ["smooth", "alpha_g2"])
def test_head_only_training_follows_cpu_fp64(name):
    """20 SGD steps on an embedding table, the head weight and (adaptive focal) alpha: device fp32 against the CPU in fp64"""
    is_focal, kw = MODULE_CASES[name]
    N, C = 64, 40
    g = torch.Generator().manual_seed(47)
    ref, wrap = _build_pair(C, is_focal, kw, True, g)
    t0 = torch.randn(N, 512, generator=g)
    label = torch.randint(0, C, (N,), generator=g)
    traces, alphas = [], []
    for w, device, dt in ((ref, "cpu", torch.float64), (wrap, DEV, torch.float32)):
        table = t0.to(device, dt).requires_grad_(True)
        params = [table] + list(w.parameters())
        assert len(params) == (3 if kw.get("alpha") else 2)
        opt = torch.optim.SGD(params, lr=0.05, momentum=0.9)
        losses = []
        for _ in range(20):
            opt.zero_grad()
            r = w(table, label.to(device))
            r["loss"].backward()
            opt.step()
            losses.append(r["loss"].item())
        traces.append(losses)
        alphas.append(w.focal_loss.alpha.detach().cpu().double() if kw.get("alpha") else None)
    print(f"head-only training {name}: cpu fp64 {traces[0]}\n device {traces[1]}")
    assert traces[0][-1] < 0.9 * traces[0][0]          # it trains
    for a, b in zip(traces[1], traces[0]):
        assert abs(a - b) <= 1e-3 * abs(b), (traces[1], traces[0])
    if kw.get("alpha"):
        assert (alphas[0] - 1.0).abs().max().item() > 1e-3       # alpha moved
        assert (alphas[1] - alphas[0]).abs().max().item() < 1e-3


def test_main_with_smooth_config(tmp_path):
    """python main.py --config fe_r18_mi355x_smooth.py trains end to end (nn.CrossEntropyLoss(label_smoothing=0.1) in the fused head)"""
    cfg = os.path.join(SYNTH, "fe_r18_mi355x_smooth.py")
    env = dict(os.environ, PFR_LIMIT_TRAIN_BATCHES="8")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--config", cfg], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Completed!" in r.stdout
    losses = [float(l.split("loss")[1]) for l in r.stdout.splitlines() if l.startswith("epoch") and "loss" in l]
    assert losses and all(math.isfinite(l) for l in losses)
