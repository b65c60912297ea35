"""Device-side gradient clipping: the segmented norm (pfr_grad_norm), the clip-aware optimizer steps (pfr_sgd_step_clip /
pfr_adamw_step_clip) behind FusedSGD / FusedAdamW.clip_grad_norm_ / clip_grad_value_, and Trainer(gradient_clip_val=,
track_grad_norm=) on the HIP path, against torch.nn.utils.clip_grad_norm_ / clip_grad_value_ + torch.optim."""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic")


def _segments():
    """> 300 views of one buffer: sizes that are not multiples of 4, starts at every 4-byte offset, one-element segments and one
    20 M-element segment, with gaps between them"""
    g = torch.Generator().manual_seed(7)
    sizes = [1, 1, 3, 5, 7, 1, 20_000_001] + [int(v) for v in torch.randint(1, 70_000, (310,), generator=g)]
    sizes[20] = 1
    offs, o = [], 0
    for i, n in enumerate(sizes):
        o += 1 + (i % 7)          # a gap of 1..7 floats: every alignment of the start
        offs.append(o)
        o += n
    buf = torch.randn(o + 8, generator=g)
    buf *= torch.rand(o + 8, generator=g) * 3       # (magnitudes spread a little)
    return buf.to(DEV), sizes, offs


def _views(buf, sizes, offs):
    return [buf[o:o + n] for n, o in zip(sizes, offs)]


@pytest.mark.parametrize("norm_type", [2.0, 1.0, math.inf, 3.0])
def test_segment_norm_against_fp64(norm_type):
    from pets_face_recognition_amd.optim.fused import SegmentNorm
    buf, sizes, offs = _segments()
    segs = _views(buf, sizes, offs)
    sn = SegmentNorm()
    outs = [sn.compute(segs, norm_type, 0.5).clone() for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])     # bitwise reproducible
    ref = torch.stack([torch.linalg.vector_norm(s.double(), norm_type) for s in segs])
    got = outs[0].double()
    n = len(segs)
    rel = ((got[:n] - ref).abs() / ref).max().item()
    assert rel <= 1e-6, rel
    total = torch.linalg.vector_norm(ref, norm_type)
    assert abs(got[n].item() - total.item()) / total.item() <= 1e-6
    # torch's fp32 coefficient from that total
    t = outs[0][n:n + 1]
    assert torch.equal(outs[0][n + 1:], torch.clamp(0.5 / (t + 1e-6), max=1.0))
    # garbage in the gaps between segments must not enter
    mask = torch.ones_like(buf, dtype=torch.bool)
    for s_, o in zip(sizes, offs):
        mask[o:o + s_] = False
    buf[mask] = float("nan")
    again = sn.compute(segs, norm_type, 0.5)
    assert torch.equal(again, outs[0])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_gradients_propagate_like_torch(bad):
    from pets_face_recognition_amd.optim import FusedSGD
    g = torch.Generator().manual_seed(3)
    w0 = [torch.randn(1000, generator=g), torch.randn(37, 5, generator=g), torch.randn(3, generator=g)]
    gr = [torch.randn_like(w, ) for w in w0]
    gr[1][4, 2] = bad
    pf = [w.clone().to(DEV).requires_grad_(True) for w in w0]
    pt = [w.clone().to(DEV).requires_grad_(True) for w in w0]
    for a, b, x in zip(pf, pt, gr):
        a.grad, b.grad = x.to(DEV), x.to(DEV)
    opt = FusedSGD(pf, 0.1, momentum=0.9)
    ropt = torch.optim.SGD(pt, 0.1, momentum=0.9)
    total = opt.clip_grad_norm_(1.0)
    coef = opt._clip_coef.clone()
    opt.step()
    rtotal = torch.nn.utils.clip_grad_norm_(pt, 1.0)
    ropt.step()
    rcoef = torch.clamp(1.0 / (rtotal + 1e-6), max=1.0)
    assert total.dim() == 0 and total.is_cuda
    if bad != bad:
        assert math.isnan(total.item()) and math.isnan(rtotal.item()) and math.isnan(coef.item())
    else:
        assert total.item() == rtotal.item() == math.inf and coef.item() == rcoef.item() == 0.0
    for a, b in zip(pf, pt):
        assert torch.equal(torch.isfinite(a), torch.isfinite(b))
        fin = torch.isfinite(b)
        assert torch.allclose(a[fin], b[fin], rtol=1e-6, atol=1e-7)


def _engine_setup(optname, seed=3):
    """ResNet-18 in an FEEngine flat buffer + a separate ArcFace-style head weight, in the reference's three groups
    (fe_dogs_config.py:123-133)"""
    import pets_face_recognition_amd.models as M
    from pets_face_recognition_amd.optim import FusedSGD, FusedAdamW
    torch.manual_seed(seed)
    m = M.resnet18(compute_dtype=torch.float32)
    m.fc = torch.nn.Linear(512, 512)
    m = m.to(DEV).train()
    m.hip_engine()
    head = torch.nn.Parameter(torch.randn(300, 512, device=DEV) * 0.05)
    p1 = [p for n, p in m.named_parameters() if "fc" not in n]
    p2 = [p for n, p in m.named_parameters() if "fc" in n]
    groups = [{"lr": 5e-3, "params": p1}, {"lr": 1e-2, "params": p2}, {"lr": 1e-2, "params": [head], "weight_decay": 1e-4}]
    if optname == "sgd":
        return m, head, groups, FusedSGD, torch.optim.SGD, dict(momentum=0.9)
    return m, head, groups, FusedAdamW, torch.optim.AdamW, {}


def _clone_groups(groups, src):
    return [dict({k: v for k, v in g.items() if k != "params"}, params=[src[id(p)] for p in g["params"]]) for g in groups]


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("optname", ["sgd", "adamw"])
@pytest.mark.parametrize("mode", ["norm", "value"])
def test_fused_optimizer_clipping_against_torch(optname, mode):
    m, head, groups, fcls, tcls, kw = _engine_setup(optname)
    opt = fcls(groups, 0.01, **kw)
    allp = [p for g in groups for p in g["params"]]
    # torch reference (clip_grad_norm_ / clip_grad_value_ + torch.optim) and the restatement (the clip applied by torch to the
    # gradients, then the plain fused step) on private copies of the same parameters
    ref = {id(p): torch.nn.Parameter(p.detach().clone()) for p in allp}
    rst = {id(p): torch.nn.Parameter(p.detach().clone()) for p in allp}
    ropt = tcls(_clone_groups(groups, ref), 0.01, **kw)
    sopt = fcls(_clone_groups(groups, rst), 0.01, **kw)
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    max_norm = clip_value = None
    for it in range(3):
        opt.zero_grad()
        (m(x) @ head.t()).square().mean().backward()
        grads = [p.grad.detach().clone() for p in allp]
        if it == 0:   # thresholds that bite: half the first step's total norm / a tenth of its largest gradient magnitude
            max_norm = 0.5 * torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(gr) for gr in grads])).item()
            clip_value = 0.1 * max(gr.abs().max().item() for gr in grads)
        if mode == "norm":
            total = opt.clip_grad_norm_(max_norm)
            coef = opt._clip_coef.clone()
        else:
            opt.clip_grad_value_(clip_value)
        opt.step()
        assert opt._clip_coef is None and opt._clip_value == 0.0      # consumed by the step
        for p, gr in zip(allp, grads):
            assert torch.equal(p.grad, gr)                             # the gradients are not rewritten
            ref[id(p)].grad = gr.clone()
            rst[id(p)].grad = gr * coef if mode == "norm" else gr.clamp(-clip_value, clip_value)
        rp = [ref[id(p)] for p in allp]
        if mode == "norm":
            rtotal = torch.nn.utils.clip_grad_norm_(rp, max_norm)
            assert abs(total.item() - rtotal.item()) <= 1e-6 * rtotal.item()
            assert total.item() > max_norm                              # the clip is active
        else:
            torch.nn.utils.clip_grad_value_(rp, clip_value)
            assert it > 0 or any(bool((gr.abs() > clip_value).any()) for gr in grads)
        ropt.step()
        sopt.step()
        for p in allp:
            assert torch.equal(p.detach(), rst[id(p)].detach()), (mode, it)       # bit-identical to the restatement
            # (AdamW: the fused update's own rounding against torch.optim.AdamW, with or without clipping — the parameters move by
            # ~lr per step and a bias of 64 elements is of that size — is ~1e-6; the clip itself is exact, see the line above)
            tol = 1e-6 if optname == "sgd" else 1e-5
            assert _rel(p.detach(), ref[id(p)].detach()) <= tol, (mode, it, _rel(p.detach(), ref[id(p)].detach()))


def test_no_clip_step_issues_the_plain_kernels(monkeypatch):
    """without clipping the step is the existing launch sequence: pfr_sgd_step only, no norm kernel"""
    from pets_face_recognition_amd._hip import ops
    m, head, groups, fcls, _, kw = _engine_setup("sgd")
    opt = fcls(groups, 0.01, **kw)
    calls = []
    for name in ("sgd_step", "sgd_step_clip", "grad_norm"):
        f = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _f=f, _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    x = torch.rand(2, 3, 64, 64, device=DEV)
    opt.zero_grad()
    (m(x) @ head.t()).square().mean().backward()
    opt.step()
    assert calls and set(calls) == {"sgd_step"}
    calls.clear()
    opt.clip_grad_norm_(1.0)
    opt.step()
    assert calls[0] == "grad_norm" and calls.count("grad_norm") == 1 and set(calls[1:]) == {"sgd_step_clip"}


def _r18_hip_namespace(tmp_path, monkeypatch, fused):
    import pets_face_recognition_amd as pfr
    pfr.install_reference_aliases()
    monkeypatch.chdir(tmp_path)
    if SYNTH not in sys.path:
        sys.path.insert(0, SYNTH)
    from _common import make
    ns = {}
    make(ns, arch='resnet18', n_train_ids=12, n_val_ids=4, photos=4, image_size=64, train_bs=8, test_bs=8, device='cuda:0',
         limit_train_batches=3, n_pairs=10, compute_dtype=torch.float32, fused_optimizer=fused)
    torch.manual_seed(5)
    batches = [b for _, b in zip(range(3), ns['train_dataloader']())]
    ns['train_dataloader'] = lambda: batches

    class Cfg(dict):
        __getattr__ = dict.get

    return Cfg(ns), batches


def test_trainer_clips_and_tracks_on_hip(tmp_path, monkeypatch):
    from pets_face_recognition_amd.engine import Trainer
    from pets_face_recognition_amd.engine.controller import Controller
    from pets_face_recognition_amd.engine.trainer import _to_device
    from pets_face_recognition_amd.optim import FusedSGD
    cfg, batches = _r18_hip_namespace(tmp_path, monkeypatch, fused=True)
    torch.manual_seed(11)
    a = Controller(cfg)

    class Logger:
        calls = []

        def log_metrics(self, metrics, step=None):
            exp = {f"grad_2.0_norm_{n}": torch.linalg.vector_norm(q.grad.double()).item()
                   for n, q in a.named_parameters() if q.grad is not None}
            exp["grad_2.0_norm_total"] = torch.linalg.vector_norm(torch.tensor(list(exp.values()), dtype=torch.float64)).item()
            self.calls.append((dict(metrics), exp))

    t = Trainer(gpus=[0], max_epochs=1, check_val_every_n_epoch=100, prefetch_batches=0, limit_train_batches=3,
                gradient_clip_val=0.05, track_grad_norm=2, log_every_n_steps=1, logger=Logger())
    t.fit(a)
    assert isinstance(a.configure_optimizers()[0][0], FusedSGD)
    assert len(t.grad_norm_history) == 3 and len(Logger.calls) == 3
    for got, exp in Logger.calls:
        assert set(got) == set(exp) and "grad_2.0_norm_total" in got
        for k, v in exp.items():       # every parameter's norm and the device total
            assert abs(got[k] - round(v, 4)) <= max(1e-4, 1e-5 * v), k
    assert Logger.calls[0][0]["grad_2.0_norm_total"] > 0.05           # the clip is active
    # the same model stepped by hand with torch.optim.SGD and torch's clip_grad_norm_
    cfg2, _ = _r18_hip_namespace(tmp_path, monkeypatch, fused=False)
    cfg2['train_dataloader'] = lambda: batches
    torch.manual_seed(11)
    b = Controller(cfg2)
    b.to(torch.device(DEV))
    opt = b.configure_optimizers()[0][0]
    assert type(opt) is torch.optim.SGD
    params = [p for g in opt.param_groups for p in g['params']]
    for bi, batch in enumerate(batches):
        b.train()
        opt.zero_grad()
        b.training_step(_to_device(batch, torch.device(DEV)), bi).backward()
        torch.nn.utils.clip_grad_norm_(params, 0.05)
        opt.step()
    for (k, va), (_, vb) in zip(a.named_parameters(), b.named_parameters()):
        assert _rel(va.detach(), vb.detach()) <= 1e-5, k


@pytest.mark.parametrize("norm", [3, 1.5, "inf"])
def test_trainer_tracks_any_norm_on_hip(tmp_path, monkeypatch, norm):
    """track_grad_norm accepts any positive p (PL 1.5): the device norm takes it, including p outside {1, 2, inf}"""
    from pets_face_recognition_amd.engine import Trainer
    from pets_face_recognition_amd.engine.controller import Controller
    cfg, _ = _r18_hip_namespace(tmp_path, monkeypatch, fused=True)
    torch.manual_seed(11)
    a = Controller(cfg)
    p = float(norm)

    class Logger:
        calls = []

        def log_metrics(self, metrics, step=None):
            exp = {f"grad_{p}_norm_{n}": torch.linalg.vector_norm(q.grad.double(), p).item()
                   for n, q in a.named_parameters() if q.grad is not None}
            exp[f"grad_{p}_norm_total"] = torch.linalg.vector_norm(torch.tensor(list(exp.values()), dtype=torch.float64), p).item()
            self.calls.append((dict(metrics), exp))

    t = Trainer(gpus=[0], max_epochs=1, check_val_every_n_epoch=100, prefetch_batches=0, limit_train_batches=2,
                track_grad_norm=norm, log_every_n_steps=1, logger=Logger())
    t.fit(a)
    assert len(Logger.calls) == 2 and t.grad_norm_history == [c[0] for c in Logger.calls]
    for got, exp in Logger.calls:
        assert set(got) == set(exp) and len(got) > 40
        for k, v in exp.items():
            assert abs(got[k] - round(v, 4)) <= max(1e-4, 1e-5 * v), (k, got[k], v)


def test_main_with_clip_config(tmp_path):
    """python main.py --config fe_r18_mi355x_clip.py trains end to end (gradient_clip_val=1, 'norm' in its trainer_kwargs)"""
    cfg = os.path.join(SYNTH, "fe_r18_mi355x_clip.py")
    env = dict(os.environ, PFR_LIMIT_TRAIN_BATCHES="3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--config", cfg], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Completed!" in r.stdout
    losses = [float(l.split("loss")[1]) for l in r.stdout.splitlines() if l.startswith("epoch") and "loss" in l]
    assert losses and all(l == l for l in losses)
