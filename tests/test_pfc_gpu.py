"""Partial FC on the MI355X: the sampler bit-exact against the torch definition, the gathered normalisation against the full one, the
fused head against fp64 on the CPU, the row-wise SGD step against a torch loop, and an end-to-end run against the CPU module."""
import math
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_pfc_host import _margin_logits64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic")
DEV = "cuda:0"


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _definition(label, score, S):
    key = score.clone()
    key[label] = 2.0
    index = torch.sort(key, descending=True, stable=True).indices[:S].sort().values
    return index.to(torch.int32), torch.searchsorted(index, label)


# ------------------------------------------------------------------------------------------------ sampler
def _sampler_cases():
    cases = []
    for C in (9, 130, 4100, 70001):
        for B in (1, 5, 64):
            for S in sorted({1, B, C // 10, C - 1}):
                if 1 <= S <= C and B <= S:
                    cases.append((C, B, S))
    return cases


@pytest.mark.parametrize("C,B,S", _sampler_cases())
def test_sampler_equals_the_definition(C, B, S):
    from pets_face_recognition_amd._hip import ops
    g = torch.Generator().manual_seed(C * 131 + B * 7 + S)
    label = torch.randint(0, C, (B,), generator=g)
    if B > 1:
        label[B // 2] = label[0]                          # duplicates
    scores = {"random": torch.rand(C, generator=g),
              "quantised": torch.randint(0, 64, (C,), generator=g).float() / 64,      # the threshold key is tied many times
              "equal": torch.full((C,), 0.25)}
    for name, score in scores.items():
        want_i, want_l = _definition(label, score, S)
        got_i, got_l = ops.pfc_sample(label.to(DEV), score.to(DEV), S)
        again_i, again_l = ops.pfc_sample(label.to(DEV), score.to(DEV), S)
        assert got_i.dtype == torch.int32 and got_l.dtype == torch.int64
        assert torch.equal(got_i.cpu(), want_i), name
        assert torch.equal(got_l.cpu(), want_l), name
        assert torch.equal(got_i, again_i) and torch.equal(got_l, again_l), name


@pytest.mark.parametrize("C", [130, 70001])
def test_sampler_with_as_many_samples_as_distinct_positives(C):
    from pets_face_recognition_amd._hip import ops
    g = torch.Generator().manual_seed(C)
    label = torch.randperm(C, generator=g)[:40]
    score = torch.rand(C, generator=g)
    want_i, want_l = _definition(label, score, 40)
    got_i, got_l = ops.pfc_sample(label.to(DEV), score.to(DEV), 40)
    assert torch.equal(got_i.cpu(), want_i) and torch.equal(got_l.cpu(), want_l)
    assert torch.equal(got_i.cpu().long(), label.sort().values)


def test_head_sample_on_the_device_is_the_cpu_sample():
    from pets_face_recognition_amd.losses.large_margin import ArcMarginProduct
    h = ArcMarginProduct(16, 4100, sample_rate=0.1)
    g = torch.Generator().manual_seed(1)
    label, score = torch.randint(0, 4100, (8,), generator=g), torch.rand(4100, generator=g)
    ci, cl = h.sample(label, score)
    gi, gl = h.sample(label.to(DEV), score.to(DEV))
    assert gi.is_cuda and torch.equal(gi.cpu(), ci) and torch.equal(gl.cpu(), cl) and h.last_index is gi


def test_argument_errors_launch_nothing():
    from pets_face_recognition_amd._hip import lib, PfrError
    label = torch.zeros(4, dtype=torch.int64, device=DEV)
    score = torch.rand(16, device=DEV)
    index = torch.full((16,), -7, dtype=torch.int32, device=DEV)
    local = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.pfr_pfc_sample_ws_bytes(16), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    args = lambda **k: [k.get("label", label.data_ptr()), k.get("B", 4), k.get("score", score.data_ptr()), 16, k.get("S", 8),
                        k.get("index", index.data_ptr()), local.data_ptr(), k.get("ws", ws.data_ptr()), st]
    for bad in (dict(S=17), dict(S=0), dict(B=9), dict(label=0), dict(score=0), dict(index=0), dict(ws=0)):
        with pytest.raises(PfrError):
            lib.pfr_pfc_sample(*args(**bad))
    w = torch.randn(16, 8, device=DEV)
    with pytest.raises(PfrError):
        lib.pfr_l2norm_gather_fwd(0, index.data_ptr(), w.data_ptr(), 0, 0, score.data_ptr(), 8, 8, 16, 8, 8, 1e-12, st)
    with pytest.raises(PfrError):
        lib.pfr_l2norm_gather_fwd(w.data_ptr(), index.data_ptr(), w.data_ptr(), 0, 0, score.data_ptr(), 17, 20, 16, 8, 20, 1e-12, st)
    with pytest.raises(PfrError):
        lib.pfr_l2norm_gather_bwd(w.data_ptr(), 0, score.data_ptr(), w.data_ptr(), w.data_ptr(), 8, 16, 8, 0, 0, 0, st)
    with pytest.raises(PfrError):
        lib.pfr_sgd_step_rows(w.data_ptr(), index.data_ptr(), 0, w.data_ptr(), 8, 16, 8, 0.1, 0.9, 0.0, 1.0, 0, 0.0, st)
    with pytest.raises(PfrError):
        lib.pfr_sgd_step_rows(w.data_ptr(), index.data_ptr(), w.data_ptr(), w.data_ptr(), 17, 16, 8, 0.1, 0.9, 0.0, 1.0, 0, 0.0, st)
    torch.cuda.synchronize()
    assert (index == -7).all() and (local == -7).all()


# ------------------------------------------------------------------------------------------------ gathered normalisation
@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [8, 512])
@pytest.mark.parametrize("want_t", [False, True])
def test_gathered_normalisation_has_the_bits_of_the_full_one(T, D, want_t):
    from pets_face_recognition_amd._hip import ops
    C, S, Sp = 301, 45, 48                                   # S no multiple of 8
    g = torch.Generator().manual_seed(D)
    w = (torch.randn(C, D, generator=g) * 0.1).to(DEV)
    index = torch.randperm(C, generator=g)[:S].sort().values.to(torch.int32).to(DEV)
    full, fullT, inv_full = ops.l2norm_fwd(w, T, want_t=want_t, ldt=C)
    wn, wnT, inv = ops.l2norm_gather_fwd(w, index, T, spad=Sp, want_t=want_t)
    assert wn.shape == (Sp, D) and wn.dtype == T
    assert torch.equal(wn[:S], full[index.long()])
    assert torch.equal(inv, inv_full[index.long()])
    assert (wn[S:] == 0).all()
    if want_t:
        assert torch.equal(wnT[:, :S], fullT[:, index.long()]) and (wnT[:, S:] == 0).all()
    else:
        assert wnT is None
    # backward: pfr_l2norm_bwd on the gathered rows
    dwn = torch.randn(Sp, D, generator=g).to(DEV)
    want = ops.l2norm_bwd(w[index.long()].contiguous(), inv, dwn[:S].contiguous(), torch.float32)
    rows = ops.l2norm_gather_bwd(w, index, inv, dwn)
    assert rows.shape == (S, D) and torch.equal(rows, want)


def test_dense_mode_rezeroes_the_previous_rows():
    from pets_face_recognition_amd._hip import ops
    C, D, S = 301, 24, 45
    g = torch.Generator().manual_seed(9)
    w = torch.randn(C, D, generator=g).to(DEV)
    dense = torch.zeros(C, D, device=DEV)
    prev = None
    for step in range(3):
        index = torch.randperm(C, generator=g)[:S].sort().values.to(torch.int32).to(DEV)
        _, _, inv = ops.l2norm_gather_fwd(w, index, torch.float32)
        dwn = torch.randn(S, D, generator=g).to(DEV)
        rows = ops.l2norm_gather_bwd(w, index, inv, dwn)
        out = ops.l2norm_gather_bwd(w, index, inv, dwn, dense_out=dense, prev_index=prev)
        assert out is dense
        mask = torch.ones(C, dtype=torch.bool, device=DEV)
        mask[index.long()] = False
        assert (dense[mask] == 0).all(), step                  # unsampled rows exactly 0, the previous step's included
        assert torch.equal(dense[index.long()], rows)
        prev = index


# ------------------------------------------------------------------------------------------------ head
HEADS = [("arc", dict(arc_margin=True), False), ("cos", {}, False), ("arc", dict(arc_margin=True), True), ("adaface", dict(margin="adaface"), False),
         ("curricular", dict(margin="curricular"), False)]


@pytest.mark.parametrize("kind,kw,focal", HEADS, ids=["arc", "cos", "arc-focal2", "adaface", "curricular"])
def test_head_against_fp64(kind, kw, focal):
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    C, D, B = 4100, 64, 8
    g = torch.Generator().manual_seed(17)
    emb0 = torch.randn(B, D, generator=g)
    label = torch.randint(0, C, (B,), generator=g)
    label[3] = label[1]
    score = torch.rand(C, generator=g)
    results = {}
    for sparse in (False, True):
        torch.manual_seed(5)
        ml = SoftmaxBasedMetricLearning(nn.Identity(), C, D, is_focal=focal, loss_kwargs=dict(gamma=2) if focal else None, sample_rate=0.1,
                                        sparse_grad=sparse, **kw)
        head = ml.add_margin
        head.compute_dtype = torch.float32
        state = {k: v.double().clone() for k, v in head.named_buffers()}
        w0 = head.weight.detach().clone()
        ml = ml.to(DEV).train()
        head.sample = lambda lab, sc=None, _f=head.sample: _f(lab, score.to(DEV))
        emb = emb0.to(DEV).requires_grad_(True)
        out = ml(emb, label.to(DEV))
        out["loss"].backward()
        index = out["classes"].cpu().long()
        assert out["logits"].shape == (B, 410) and index.numel() == 410
        if sparse:
            assert head.weight.grad is None
            ridx, rows = head.weight.row_grad
            assert ridx is out["classes"] and rows.shape == (410, D)
            rows = rows.cpu()
        else:
            assert getattr(head.weight, "row_grad", None) is None
            mask = torch.ones(C, dtype=torch.bool)
            mask[index] = False
            assert (head.weight.grad.cpu()[mask] == 0).all()
            rows = head.weight.grad.cpu()[index]
        results[sparse] = (out["loss"].item(), emb.grad.cpu(), rows)

    e64 = emb0.double().requires_grad_(True)
    w64 = w0.double().requires_grad_(True)
    local = out["local_label"].cpu()
    logits = _margin_logits64(kind, head, e64, w64[index], local, state)
    ce = F.cross_entropy(logits, local, reduction="none")
    loss = ((1 - torch.exp(-ce)) ** 2 * ce).mean() if focal else ce.mean()
    loss.backward()
    for sparse, (l, demb, rows) in results.items():
        print(f"{kind} sparse={sparse}: loss {l:.6f} vs {loss.item():.6f}, demb {rel(demb, e64.grad):.2e}, rows {rel(rows, w64.grad[index]):.2e}")
        assert abs(l - loss.item()) <= 1e-4 * max(1.0, abs(loss.item()))
        assert rel(demb, e64.grad) < 1e-4
        assert rel(rows, w64.grad[index]) < 1e-4
    assert torch.equal(results[False][2], results[True][2])          # dense and sparse modes give the same rows


def test_head_in_bf16_and_the_second_backward():
    from pets_face_recognition_amd._hip import PfrError
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    C, D, B = 4100, 64, 8
    g = torch.Generator().manual_seed(3)
    emb0, label, score = torch.randn(B, D, generator=g), torch.randint(0, C, (B,), generator=g), torch.rand(C, generator=g)
    torch.manual_seed(5)
    ml = SoftmaxBasedMetricLearning(nn.Identity(), C, D, arc_margin=True, sample_rate=0.1, sparse_grad=True)
    cpu_loss = None
    head = ml.add_margin
    head.sample = lambda lab, sc=None, _f=head.sample: _f(lab, score.to(lab.device))
    cpu_loss = ml.train()(emb0, label)["loss"].item()
    ml = ml.to(DEV)
    head.compute_dtype = torch.bfloat16
    emb = emb0.to(DEV).requires_grad_(True)
    out = ml(emb, label.to(DEV))
    assert abs(out["loss"].item() - cpu_loss) <= 2e-2 * max(1.0, abs(cpu_loss))
    out["loss"].backward(retain_graph=True)
    rows1 = head.weight.row_grad[1].clone()
    out["loss"].backward()                                  # the same index tensor: the rows accumulate
    assert torch.allclose(head.weight.row_grad[1], 2 * rows1, rtol=1e-6, atol=0)
    out2 = ml(emb, label.to(DEV))                           # another draw (another index tensor) before the rows were consumed
    with pytest.raises((PfrError, RuntimeError), match="zero_grad"):
        out2["loss"].backward()


# ------------------------------------------------------------------------------------------------ pfr_sgd_step_rows through FusedSGD
@pytest.mark.parametrize("clip", [False, True])
def test_row_step_against_a_torch_loop(clip):
    from pets_face_recognition_amd.optim import FusedSGD
    C, D, S = 203, 24, 31
    lr, mu, wd, max_norm = 0.1, 0.9, 1e-4, 0.5
    g = torch.Generator().manual_seed(23)
    w0 = torch.randn(C, D, generator=g)
    p = nn.Parameter(w0.clone().to(DEV))
    other = nn.Parameter(torch.randn(40, generator=g).to(DEV))          # a dense parameter in the same optimizer
    opt = FusedSGD([{"params": [other]}, {"params": [p], "weight_decay": wd}], lr, momentum=mu)
    w, mom = w0.double().clone(), torch.zeros(C, D, dtype=torch.float64)
    ow, omom = other.detach().cpu().double().clone(), torch.zeros(40, dtype=torch.float64)
    touched = torch.zeros(C, dtype=torch.bool)
    steps = []
    for step in range(5):
        if step == 3:       # state_dict() -> fresh optimiser -> load_state_dict() continues identically
            sd = opt.state_dict()
            opt = FusedSGD([{"params": [other]}, {"params": [p], "weight_decay": wd}], lr, momentum=mu)
            opt.load_state_dict(sd)
        index = torch.randperm(C, generator=g)[:S].sort().values
        rows = torch.randn(S, D, generator=g)
        og = torch.randn(40, generator=g)
        opt.zero_grad()
        assert getattr(p, "row_grad", None) is None
        p.row_grad = (index.to(torch.int32).to(DEV), rows.to(DEV))
        other.grad = og.to(DEV)
        coef = 1.0
        if clip:
            total = opt.clip_grad_norm_(max_norm)
            want_total = math.sqrt(rows.double().pow(2).sum().item() + og.double().pow(2).sum().item())      # the norm includes the rows
            assert abs(total.item() - want_total) <= 1e-5 * want_total
            coef = min(1.0, max_norm / (want_total + 1e-6))
        opt.step()
        for s, r in enumerate(index.tolist()):                # the torch loop over the rows
            gr = rows[s].double() * coef + wd * w[r]
            mom[r] = mu * mom[r] + gr
            w[r] -= lr * mom[r]
        omom = mu * omom + og.double() * coef
        ow -= lr * omom
        touched[index] = True
        steps.append(index)
    assert p.grad is None
    buf = opt.state[p]["momentum_buffer"]
    assert buf.shape == (C, D)
    assert rel(p, w) < 1e-6 and rel(buf, mom) < 1e-6 and rel(other, ow) < 1e-6
    assert not touched.all()
    assert torch.equal(p.detach().cpu()[~touched], w0[~touched])          # never sampled: weight and momentum bits untouched
    assert (buf.cpu()[~touched] == 0).all()


def test_row_step_with_a_value_clip():
    from pets_face_recognition_amd._hip import ops
    C, D, S = 50, 6, 7                                    # D no multiple of 4: the element-wise kernel
    g = torch.Generator().manual_seed(2)
    w0, rows = torch.randn(C, D, generator=g), torch.randn(S, D, generator=g)
    index = torch.randperm(C, generator=g)[:S].sort().values
    p, mom = w0.clone().to(DEV), torch.zeros(C, D, device=DEV)
    ops.sgd_step_rows(p, index.to(torch.int32).to(DEV), rows.to(DEV), mom, 0.1, 0.9, 0.01, clip_value=0.3, grad_scale=0.5)
    want, wmom = w0.double().clone(), torch.zeros(C, D, dtype=torch.float64)
    gr = (rows.double() * 0.5).clamp(-0.3, 0.3) + 0.01 * want[index]
    wmom[index] = gr
    want[index] -= 0.1 * gr
    assert rel(p, want) < 1e-6 and rel(mom, wmom) < 1e-6
    mask = torch.ones(C, dtype=torch.bool)
    mask[index] = False
    assert torch.equal(p.cpu()[mask], w0[mask])


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("sparse", [False, True])
def test_resnet18_three_steps_against_the_cpu_module(sparse):
    """The reference of the dense mode is the CPU module under torch.optim.SGD.  sparse_grad=True defines another update of the head
    weight (lazy momentum: rows outside the step's index keep weight and momentum, no decay), so there the CPU module's head weight is
    stepped by that rule, written as a torch loop over its dense gradient's sampled rows; the backbone stays under torch.optim.SGD."""
    import pets_face_recognition_amd.models as M
    from oracle import resnet_ref
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    from pets_face_recognition_amd.optim import FusedSGD
    C, B, HW = 300, 8, 32
    sd = resnet_ref.init_state_dict("resnet18", 512, seed=1)
    g = torch.Generator().manual_seed(4)
    xs = [torch.rand(B, 3, HW, HW, generator=g) for _ in range(3)]
    ys = [torch.randint(0, C, (B,), generator=g) for _ in range(3)]
    scores = [torch.rand(C, generator=g) for _ in range(3)]
    w = torch.randn(C, 512, generator=g) * 0.05
    losses = {}
    for dev in ("cpu", DEV):
        m = M.resnet18(compute_dtype=torch.float32) if dev != "cpu" else M.resnet18()
        m.fc = torch.nn.Linear(512, 512)
        m.load_state_dict(sd)
        ml = SoftmaxBasedMetricLearning(m, C, 512, arc_margin=True, sample_rate=0.2, sparse_grad=sparse and dev != "cpu")
        head = ml.add_margin
        head.compute_dtype = torch.float32
        with torch.no_grad():
            head.weight.copy_(w)
        ml = ml.to(dev).train()
        it = iter(scores)
        head.sample = lambda lab, sc=None, _f=head.sample: _f(lab, next(it).to(lab.device))
        lr, mu, wd = 0.01, 0.9, 1e-4
        lazy = sparse and dev == "cpu"
        opt = (torch.optim.SGD if dev == "cpu" else FusedSGD)(ml.module.parameters() if lazy else ml.parameters(), lr, momentum=mu,
                                                              weight_decay=wd)
        mom = torch.zeros(C, 512)
        ls = []
        for x, y in zip(xs, ys):
            opt.zero_grad()
            head.weight.grad = None
            out = ml(x.to(dev), y.to(dev))
            assert out["logits"].shape == (B, 60)
            out["loss"].backward()
            opt.step()
            if lazy:
                with torch.no_grad():
                    for r in out["classes"].tolist():
                        gr = head.weight.grad[r] + wd * head.weight[r]
                        mom[r] = mu * mom[r] + gr
                        head.weight[r] -= lr * mom[r]
            ls.append(out["loss"].item())
        losses[dev] = (ls, head.weight.detach().cpu().clone())
    print("losses", losses["cpu"][0], losses[DEV][0], "head weight rel", rel(losses[DEV][1], losses["cpu"][1]))
    for a, b in zip(losses["cpu"][0], losses[DEV][0]):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(a))
    assert rel(losses[DEV][1], losses["cpu"][1]) < 1e-3


def test_main_with_pfc_config(tmp_path):
    """python main.py --config fe_r18_mi355x_pfc.py trains end to end: sample_rate=0.1, sparse_grad=True, FusedSGD"""
    import subprocess
    cfg = os.path.join(SYNTH, "fe_r18_mi355x_pfc.py")
    env = dict(os.environ, PFR_LIMIT_TRAIN_BATCHES="4")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--config", cfg], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Completed!" in r.stdout
    losses = [float(l.split("loss")[1]) for l in r.stdout.splitlines() if l.startswith("epoch") and "loss" in l]
    assert losses and all(math.isfinite(l) for l in losses)
