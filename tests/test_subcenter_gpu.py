"""The sub-centre head (K centres per class) on the device: the pooling and scatter kernels against torch on the same values, K = 1 as
the path it was, the chain pool -> row kernel -> scatter against fp64 on the CPU from the device's own sub-cosines (free of GEMM
rounding), and the module end to end against the CPU module in fp64.

Selection (which sub-centre is the maximum) is a discontinuous function of the cosines: wherever a device result is compared with an
fp64 one computed from OTHER cosines, the test first asserts that no (row, class) pair has its two best sub-cosines closer than 1e-4
in fp64, 100 times the fp32 cosine error, so that both sides select alike.  Tolerances are those of tests/test_head_criterion_gpu.py:
kernel level loss 1e-4 * max(1, |loss|), gradients relative L2 < 1e-4; module level 1e-3; bf16 loss 2e-2 (tests/test_model_gpu.py)."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_head_criterion_gpu import _criterion64, _forbid_fallback, _margin_logits64, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic")
SHAPES = [(1, 2), (37, 3), (130, 4), (64, 16), (4100, 2), (37, 1)]      # (C, K): vector paths (K 2, 4), K = 3, run-time K, > 1 chunk of classes
NAN = float("nan")


def ops():
    from pets_face_recognition_amd._hip import ops as o
    return o


def _up8(n):
    return (n + 7) // 8 * 8


def _first_argmax(v):
    """[B, C, K] -> (max, lowest index attaining it)"""
    K = v.shape[2]
    mx = v.amax(2)
    idx = torch.where(v == mx[..., None], torch.arange(K), torch.full((), K)).amin(2)
    return mx, idx


def _sub_cosines(B, C, K, seed):
    """fp32 [B, ld_sub] with NaN pad columns and exact ties: class c has sub-centre 1 equal to sub-centre 0 when c is even, and its last
    sub-centre equal to sub-centre 0 when c % 3 == 0"""
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(B, C, K, generator=g) * 2.0 - 1.0
    if K > 1:
        v[:, 0::2, 1] = v[:, 0::2, 0]
        v[:, 0::3, K - 1] = v[:, 0::3, 0]
    full = torch.full((B, _up8(C * K)), NAN)
    full[:, :C * K] = v.reshape(B, C * K)
    return v, full, g


@pytest.mark.parametrize("C,K", SHAPES)
@pytest.mark.parametrize("B", [1, 5, 8])
def test_pool_kernel_vs_torch(B, C, K):
    o = ops()
    v, full, g = _sub_cosines(B, C, K, 100 + B)
    mx, idx = _first_argmax(v)
    if K > 1:
        assert (v[:, 0, 0] == v[:, 0, 1]).all() and ((v == mx[..., None]).sum(2) > 1).any()      # exact ties do occur
    label = torch.randint(0, C, (B,), generator=g)
    want = torch.bincount(label * K + idx[torch.arange(B), label], minlength=C * K)
    ldc = _up8(C)
    cos = torch.full((B, ldc), NAN, device=DEV)
    count = torch.zeros(C * K, dtype=torch.int32, device=DEV)
    fd, ld = full.to(DEV), label.to(DEV)
    cos, arg = o.subcenter_pool(fd, C, K, label=ld, count=count, cos=cos)
    torch.cuda.synchronize()
    assert cos.shape == (B, ldc) and arg.shape == (B, C) and arg.dtype == torch.uint8
    assert torch.equal(cos[:, :C].cpu().view(torch.int32), mx.view(torch.int32))       # bit-equal to amax
    assert torch.count_nonzero(cos[:, C:]).item() == 0 and not torch.isnan(cos).any()
    assert torch.equal(arg.cpu().long(), idx)
    assert torch.equal(count.cpu().long(), want)
    _, arg2 = o.subcenter_pool(fd, C, K, label=ld, count=count)                         # the histogram accumulates
    cos3, arg3 = o.subcenter_pool(fd, C, K, ldc=ldc)                                    # and is optional
    torch.cuda.synchronize()
    assert torch.equal(count.cpu().long(), 2 * want)
    assert torch.equal(arg2, arg) and torch.equal(arg3, arg) and torch.equal(cos3, cos)


def test_pool_kernel_unaligned_rows_take_the_scalar_path():
    """K = 2 and 4 with an odd leading dimension: the 8- / 16-byte loads do not apply"""
    o = ops()
    for C, K in ((37, 2), (37, 4)):
        B = 5
        v, _, _ = _sub_cosines(B, C, K, 7)
        full = torch.full((B, C * K + 3), NAN)
        full[:, :C * K] = v.reshape(B, C * K)
        mx, idx = _first_argmax(v)
        cos, arg = o.subcenter_pool(full.to(DEV), C, K)
        torch.cuda.synchronize()
        assert torch.equal(cos.cpu(), mx) and torch.equal(arg.cpu().long(), idx)
        d = torch.randn(B, C)
        out = o.subcenter_scatter(d.to(DEV), arg, K, out=torch.full((B, C * K + 3), NAN, device=DEV))
        torch.cuda.synchronize()
        ref = torch.zeros(B, C * K + 3)
        ref[:, :C * K] = torch.zeros(B, C, K).scatter_(2, idx[..., None], d[..., None]).reshape(B, C * K)
        assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,K", SHAPES)
@pytest.mark.parametrize("B", [1, 5, 8])
def test_scatter_kernel_vs_torch(B, C, K, dtype):
    o = ops()
    g = torch.Generator().manual_seed(200 + B)
    ldc, ld_sub = _up8(C), _up8(C * K)
    dcos = torch.randn(B, ldc, generator=g).to(dtype)                 # the pad columns hold values that must not travel
    arg = torch.randint(0, K, (B, C), generator=g).to(torch.uint8)
    ref = torch.zeros(B, ld_sub, dtype=dtype)
    ref[:, :C * K] = torch.zeros(B, C, K, dtype=dtype).scatter_(2, arg.long()[..., None], dcos[:, :C, None]).reshape(B, C * K)
    out = torch.full((B, ld_sub), NAN, dtype=dtype, device=DEV)
    got = o.subcenter_scatter(dcos.to(DEV), arg.to(DEV), K, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and got.dtype == dtype
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got.cpu().view(bits), ref.view(bits))          # bit-equal everywhere, zeros and pad included


def _crit(C, kind, dev):
    from pets_face_recognition_amd.losses.losses import Criterion
    if kind == "focal_g2":
        return Criterion(2.0, None, None, 0.0, "mean")
    if kind == "alpha_g2":
        return Criterion(2.0, (0.5 + torch.rand(C, generator=torch.Generator().manual_seed(1))).to(dev), None, 0.0, "mean")
    return Criterion(0.0, None, (0.25 + 2.0 * torch.rand(C, generator=torch.Generator().manual_seed(2))).to(dev), 0.1, "mean")


@pytest.mark.parametrize("kind", ["focal_g2", "weight_smooth"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_sub_center_is_the_path_it_was(kind, dtype, monkeypatch):
    from pets_face_recognition_amd.losses._head_hip import MarginCEFunction, MarginFunction
    o = ops()

    def boom(*a, **k):
        raise AssertionError("K = 1 launched a sub-centre kernel")
    monkeypatch.setattr(o, "subcenter_pool", boom)
    monkeypatch.setattr(o, "subcenter_scatter", boom)
    B, C, D = 8, 37, 32
    g = torch.Generator().manual_seed(9)
    x, w = torch.randn(B, D, generator=g).to(DEV), torch.randn(C, D, generator=g).to(DEV)
    label = torch.randint(0, C, (B,), generator=g).to(DEV)
    crit = _crit(C, kind, DEV)
    res = []
    for extra in ((), (1, None)):
        xe, we = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        loss, logits = MarginCEFunction.apply(xe, we, label, "arc", 64.0, 0.5, crit, dtype, True, None, *extra)
        loss.backward()
        xm, wm = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        lg = MarginFunction.apply(xm, wm, label, "cos", 64.0, 0.4, dtype, *extra)
        lg.square().mean().backward()
        torch.cuda.synchronize()
        res.append((loss.detach(), logits, xe.grad, we.grad, lg.detach(), xm.grad, wm.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def _device_chain(cos_sub, label, C, K, mode, s, m, crit, T):
    """pool -> margin_ce / margin_ce_ex -> scatter, as MarginCEFunction chains them"""
    o = ops()
    B = cos_sub.shape[0]
    ldc = _up8(C) if T == torch.bfloat16 else (C + 3) // 4 * 4
    cos, arg = o.subcenter_pool(cos_sub, C, K, ldc=ldc)
    one = torch.ones((), device=cos_sub.device)
    if crit.is_plain:
        _, rows, _ = o.margin_ce(cos, label, C, mode, s, m, gamma=crit.gamma, want_logits=False)
        loss = o.mean(rows)
        _, _, dcos = o.margin_ce(cos, label, C, mode, s, m, gamma=crit.gamma, grad_scale=1.0 / B, grad_scale_dev=one, want_logits=False, dcos_dtype=T)
    else:
        kw = dict(gamma=crit.gamma, alpha=crit.alpha, class_weight=crit.weight, label_smoothing=crit.smoothing)
        _, rows, stats, _ = o.margin_ce_ex(cos, label, C, mode, s, m, want_logits=False, **kw)
        inv = None
        if crit.alpha is not None:
            loss, gs = o.mean(rows), 1.0 / B
        else:
            (loss, inv), gs = o.loss_reduce(rows, stats, "weighted_mean"), 1.0
        _, _, _, dcos = o.margin_ce_ex(cos, label, C, mode, s, m, grad_scale=gs, grad_scale_dev=one, grad_scale_dev2=inv, want_logits=False,
                                       want_stats=False, dcos_dtype=T, **kw)
    dsub = o.subcenter_scatter(dcos, arg, K, ld_sub=cos_sub.shape[1])
    torch.cuda.synchronize()
    return loss, dsub, arg


@pytest.mark.parametrize("kind", ["focal_g2", "alpha_g2", "weight_smooth"])
@pytest.mark.parametrize("mode", ["arc", "cos"])
def test_composition_vs_fp64_from_the_device_cosines(mode, kind):
    """cos_sub from the head's own cosine GEMM; pooled -> margin -> criterion -> d loss / d cos_sub in fp64 on the CPU from THOSE fp32 values
    (both sides pool the same floats: ties cannot differ), against the device chain in both compute dtypes"""
    from pets_face_recognition_amd.losses._head_hip import _cosine_fwd
    B, C, K, D = 8, 37, 3, 32
    s, m = 64.0, (0.4 if mode == "cos" else 0.5)
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(B, D, generator=g), torch.randn(C * K, D, generator=g)
    label = torch.randint(0, C, (B,), generator=g)
    crit = _crit(C, kind, DEV)
    d32 = None
    for T in (torch.float32, torch.bfloat16):
        cos_sub, _ = _cosine_fwd(x.to(DEV), w.to(DEV), T)
        assert cos_sub.dtype == torch.float32 and cos_sub.shape[1] >= C * K
        c64 = cos_sub[:, :C * K].cpu().double().requires_grad_(True)
        pooled = c64.view(B, C, K).max(2).values
        logits = _margin_logits64(pooled, label, mode, s, m)
        cpu = lambda t: None if t is None else t.cpu().double()
        loss_r = _criterion64(logits, label, crit.gamma, cpu(crit.alpha), cpu(crit.weight), crit.smoothing, crit.reduction)
        loss_r.backward()
        loss, dsub32, arg = _device_chain(cos_sub, label.to(DEV), C, K, mode, s, m, crit, torch.float32)
        figs = dict(loss=loss.item(), loss_ref=loss_r.item(), dcos_sub=rel_err(dsub32[:, :C * K], c64.grad))
        print(f"sub-centre chain {mode} {kind} cosines of the {T} GEMM: {figs}")
        assert abs(figs["loss"] - figs["loss_ref"]) < 1e-4 * max(1.0, abs(figs["loss_ref"]))
        assert figs["dcos_sub"] < 1e-4
        assert torch.count_nonzero(dsub32[:, C * K:]).item() == 0
        # bf16 gradient dtype: the rounded fp32 result, bit for bit (the scatter moves values, it does not compute)
        loss16, dsub16, arg16 = _device_chain(cos_sub, label.to(DEV), C, K, mode, s, m, crit, torch.bfloat16)
        assert dsub16.dtype == torch.bfloat16 and torch.equal(arg16, arg) and torch.equal(loss16, loss)
        assert torch.equal(dsub16.view(torch.int16), dsub32.bfloat16().view(torch.int16))


def _module_pair(mode="arc", is_focal=False, kw=None):
    """the draw of the module tests: torch.Generator().manual_seed(3), x then w as float64 randn; B = 8, C = 37, K = 3, D = 32"""
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    B, C, K, D = 8, 37, 3, 32
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, D, generator=g, dtype=torch.float64)
    w = torch.randn(C * K, D, generator=g, dtype=torch.float64)
    label = torch.randint(0, C, (B,), generator=g)
    wraps = []
    for device in ("cpu", DEV):
        wrap = SoftmaxBasedMetricLearning(nn.Identity(), C, D, is_focal=is_focal, loss_kwargs=dict(kw or {}), arc_margin=mode != "cos",
                                          sub_centers=K)
        with torch.no_grad():
            wrap.add_margin.weight.copy_(w)                    # the fp32 values both sides start from
        wrap = wrap.double() if device == "cpu" else wrap.to(DEV)
        wraps.append(wrap.train())
    return wraps[0], wraps[1], x.float(), label


def _gap64(emb64, w64, C, K):
    """smallest difference between the two best sub-cosines over all (row, class) pairs, and the fp64 selection"""
    cs = (F.normalize(emb64.detach()) @ F.normalize(w64.detach()).t()).view(emb64.shape[0], C, K)
    top2 = cs.topk(2, dim=2).values
    return (top2[..., 0] - top2[..., 1]).min().item(), cs.argmax(2)


@pytest.mark.parametrize("mode,is_focal,kw", [("arc", False, {}), ("cos", True, dict(gamma=2, alpha=True)),
                                              ("arc", False, dict(label_smoothing=0.1))], ids=["arc_ce", "cos_alpha_g2", "arc_smooth"])
def test_module_vs_cpu_fp64_without_fallback(mode, is_focal, kw, monkeypatch):
    ref, wrap, x, label = _module_pair(mode, is_focal, kw)
    B, C, K = 8, 37, 3
    wrap.add_margin.compute_dtype = torch.float32
    x64 = x.double().requires_grad_(True)
    gap, arg64 = _gap64(x64, ref.add_margin.weight, C, K)
    print(f"sub-centre module {mode}: smallest top-2 sub-cosine gap {gap:.3e}")
    assert gap > 1e-4
    r64 = ref(x64, label)
    r64["loss"].backward()
    _forbid_fallback(monkeypatch, wrap)
    xd = x.to(DEV).requires_grad_(True)
    r = wrap(xd, label.to(DEV))
    r["loss"].backward()
    torch.cuda.synchronize()
    figs = dict(loss=r["loss"].item(), loss_ref=r64["loss"].item(), logits=rel_err(r["logits"], r64["logits"]), dx=rel_err(xd.grad, x64.grad),
                dw=rel_err(wrap.add_margin.weight.grad, ref.add_margin.weight.grad))
    print(f"sub-centre module {mode} {kw}: {figs}")
    assert r["logits"].shape == (B, C)
    assert figs["logits"] < 1e-3
    assert abs(figs["loss"] - figs["loss_ref"]) < 1e-3 * abs(figs["loss_ref"])
    assert figs["dx"] < 1e-3 and figs["dw"] < 1e-3
    want = torch.bincount(label * K + arg64[torch.arange(B), label], minlength=C * K).view(C, K)
    assert torch.equal(wrap.add_margin.sub_center_count.cpu().long(), want)
    assert torch.equal(ref.add_margin.sub_center_count.long(), want)
    wrap.eval()
    wrap(xd, label.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(wrap.add_margin.sub_center_count.cpu().long(), want)     # evaluation does not count


def test_standalone_head_vs_cpu_fp64():
    """ArcMarginProduct(sub_centers=3) on its own (MarginFunction): logits and gradients of a downstream loss"""
    ref, wrap, x, label = _module_pair("arc")
    wrap.add_margin.compute_dtype = torch.float32
    x64 = x.double().requires_grad_(True)
    assert _gap64(x64, ref.add_margin.weight, 37, 3)[0] > 1e-4
    F.cross_entropy(ref.add_margin(x64, label), label).backward()
    xd = x.to(DEV).requires_grad_(True)
    logits = wrap.add_margin(xd, label.to(DEV))
    F.cross_entropy(logits, label.to(DEV)).backward()
    torch.cuda.synchronize()
    assert rel_err(logits, ref.add_margin(x64, label)) < 1e-3
    assert rel_err(xd.grad, x64.grad) < 1e-3
    assert rel_err(wrap.add_margin.weight.grad, ref.add_margin.weight.grad) < 1e-3
    assert wrap.add_margin.sub_center_count.sum().item() == 8


def test_module_bf16_routing(monkeypatch):
    """bf16 compute dtype: the loss within the bf16 bound, and the routing invariant: a weight row c*K + k that no sample selected
    (arg[b][c] != k for every b, arg from the pooling kernel on this forward's own sub-cosines) gets an exactly zero gradient, every
    selected row a non-zero one.  No comparison with an fp64 argmax: pairs with gaps under the bf16 cosine error may flip."""
    from pets_face_recognition_amd.losses import _head_hip
    ref, wrap, x, label = _module_pair("arc")
    B, C, K, D = 8, 37, 3, 32
    wrap.add_margin.compute_dtype = torch.bfloat16
    r64 = ref(x.double(), label)
    seen = []
    pool = _head_hip.ops.subcenter_pool

    def spy(*a, **k):
        out = pool(*a, **k)
        seen.append(out[1])
        return out
    monkeypatch.setattr(_head_hip.ops, "subcenter_pool", spy)
    _forbid_fallback(monkeypatch, wrap)
    xd = x.to(DEV).requires_grad_(True)
    r = wrap(xd, label.to(DEV))
    r["loss"].backward()
    torch.cuda.synchronize()
    print(f"sub-centre module bf16: loss {r['loss'].item()} vs fp64 {r64['loss'].item()}")
    assert abs(r["loss"].item() - r64["loss"].item()) < 2e-2 * abs(r64["loss"].item())
    assert len(seen) == 1 and seen[0].shape == (B, C)
    sel = torch.zeros(C, K, dtype=torch.bool)
    sel[torch.arange(C).expand(B, C), seen[0].cpu().long()] = True
    gw = wrap.add_margin.weight.grad.cpu().view(C, K, D)
    assert torch.isfinite(gw).all()
    assert gw[~sel].abs().max().item() == 0.0
    assert (gw[sel].abs().amax(1) > 0).all()
    assert (~sel).any() and sel.any()


def test_head_only_training_follows_cpu_fp64():
    """5 steps on an embedding table and the sub-centre head weight: FusedSGD on the device in fp32 against torch.optim.SGD on the CPU
    in fp64, the selection gap asserted at every step (on the CPU in fp64 the gaps of this draw are 2.9e-4, 2.7e-3, 8.0e-4, 1.8e-3, 5.5e-4;
    the sixth step would start from 2.4e-5, too close to a tie to compare selections across precisions)"""
    from pets_face_recognition_amd.optim import FusedSGD
    ref, wrap, x, label = _module_pair("arc", False, dict(label_smoothing=0.1))
    C, K = 37, 3
    wrap.add_margin.compute_dtype = torch.float32
    traces, counts = [], []
    for w, device, dt in ((ref, "cpu", torch.float64), (wrap, DEV, torch.float32)):
        counts.append([])
        table = x.to(device, dt).requires_grad_(True)
        params = [table] + list(w.parameters())
        assert len(params) == 2
        opt = (torch.optim.SGD if device == "cpu" else FusedSGD)(params, lr=0.05, momentum=0.9)
        losses = []
        for _ in range(5):
            if device == "cpu":
                gap, _ = _gap64(table, w.add_margin.weight, C, K)
                assert gap > 1e-4, gap
            opt.zero_grad()
            r = w(table, label.to(device))
            r["loss"].backward()
            opt.step()
            losses.append(r["loss"].item())
            counts[-1].append(w.add_margin.sub_center_count.cpu().clone())
        traces.append(losses)
    for step, (a, b) in enumerate(zip(counts[1], counts[0])):
        assert torch.equal(a, b), f"the selected sub-centres differ from step {step} on"
    print(f"sub-centre head-only training: cpu fp64 {traces[0]}\n device {traces[1]}")
    assert traces[0][-1] < 0.9 * traces[0][0]          # it trains
    for a, b in zip(traces[1], traces[0]):
        assert abs(a - b) <= 1e-3 * abs(b), (traces[1], traces[0])
    assert wrap.add_margin.sub_center_count.sum().item() == 5 * 8
    assert torch.equal(wrap.add_margin.sub_center_count.cpu(), ref.add_margin.sub_center_count)
    dom = wrap.add_margin.dominant_sub_centers()
    old = wrap.add_margin.weight.detach().clone()
    wrap.add_margin.prune_sub_centers()
    assert torch.equal(wrap.add_margin.weight.detach(), old[torch.arange(C, device=DEV) * K + dom])
    out = wrap(x.to(DEV), label.to(DEV))                # a one-centre head from here on
    torch.cuda.synchronize()
    assert out["logits"].shape == (8, C) and math.isfinite(out["loss"].item())


def test_integration_md_sub_centre_stubs_run():
    """the two stubs INTEGRATION.md §2 documents, executed as written, against the package's wrappers"""
    import re
    o = ops()
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = md.split("## 2. Binding the C-ABI directly")[1].split("\n## ")[0]
    block = re.findall(r"```python\n(.*?)```", sec, flags=re.S)[0]
    so = os.path.join(ROOT, "pets-face-recognition_amd", "csrc", "libpfr_hip.so")
    ns = {}
    exec(block.replace('"libpfr_hip.so"', repr(so)), ns)
    B, C, K = 5, 37, 3
    g = torch.Generator().manual_seed(4)
    cs = torch.randn(B, C * K, generator=g).to(DEV)
    label = torch.randint(0, C, (B,), generator=g).to(DEV)
    c1, c2 = torch.zeros(C * K, dtype=torch.int32, device=DEV), torch.zeros(C * K, dtype=torch.int32, device=DEV)
    cos, arg = ns["subcenter_pool"](cs, C, K, label, c1)
    cos2, arg2 = o.subcenter_pool(cs, C, K, label=label, count=c2)
    d = torch.randn(B, C, generator=g).to(DEV).bfloat16()
    ds = ns["subcenter_scatter"](d, arg, K)
    torch.cuda.synchronize()
    assert torch.equal(cos, cos2) and torch.equal(arg, arg2) and torch.equal(c1, c2) and c1.sum().item() == B
    assert torch.equal(ds, o.subcenter_scatter(d, arg, K))


def test_main_with_subcenter_config(tmp_path):
    """python main.py --config fe_r18_mi355x_subcenter.py trains end to end (three centres per identity in the fused head)"""
    cfg = os.path.join(SYNTH, "fe_r18_mi355x_subcenter.py")
    env = dict(os.environ, PFR_LIMIT_TRAIN_BATCHES="8")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--config", cfg], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Completed!" in r.stdout
    losses = [float(l.split("loss")[1]) for l in r.stdout.splitlines() if l.startswith("epoch") and "loss" in l]
    assert losses and all(math.isfinite(l) for l in losses)
