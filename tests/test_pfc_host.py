"""Partial FC (sample_rate < 1) without a GPU: constructor validation, the sampling definition, the CPU module against an fp64 oracle
that is the full reference formula restricted to the sampled classes, the unchanged default path, and every refused combination."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

C, D, B = 50, 16, 6


def _heads():
    from pets_face_recognition_amd.losses.large_margin import AddMarginProduct, ArcMarginProduct, AdaFaceProduct, CurricularFaceProduct
    return {"arc": ArcMarginProduct, "cos": AddMarginProduct, "adaface": AdaFaceProduct, "curricular": CurricularFaceProduct}


def _sample_definition(label, score, C, S):
    """the issue's definition, written out element by element (no torch.sort): S largest keys, ties to the lower class id, ascending"""
    pos = set(int(v) for v in label.tolist())
    key = [2.0 if c in pos else float(score[c]) for c in range(C)]
    order = sorted(range(C), key=lambda c: (-key[c], c))
    index = sorted(order[:S])
    where = {c: i for i, c in enumerate(index)}
    return index, [where[int(v)] for v in label.tolist()]


def _batch(seed=0, n=B):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(n, D, generator=g)
    label = torch.randint(0, C, (n,), generator=g)
    label[-1] = label[0]                      # a duplicate
    score = torch.rand(C, generator=g)
    return emb, label, score


# ------------------------------------------------------------------------------------------------ constructor
@pytest.mark.parametrize("rate", [0.0, -0.1, 1.5, float("nan")])
def test_sample_rate_out_of_range(rate):
    with pytest.raises(ValueError, match="sample_rate"):
        _heads()["arc"](D, C, sample_rate=rate)


def test_sample_rate_that_samples_nothing():
    with pytest.raises(ValueError, match="samples no class"):
        _heads()["arc"](D, C, sample_rate=0.01)          # int(0.01 * 50) = 0


def test_constructor_attributes_and_defaults():
    for cls in _heads().values():
        h = cls(D, C)
        assert h.sample_rate == 1.0 and h.sparse_grad is False and h.num_sample == C and h.sample_generator is None
        assert h.last_index is None
        h = cls(D, C, sample_rate=0.3, sparse_grad=True)
        assert h.num_sample == int(0.3 * C) == 15 and h.sparse_grad is True
        assert list(h.state_dict()) == list(cls(D, C).state_dict())      # no new state-dict keys


def test_wrapper_passes_the_arguments_through():
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    for kw in (dict(arc_margin=True), dict(), dict(margin="adaface"), dict(margin="curricular")):
        ml = SoftmaxBasedMetricLearning(nn.Identity(), C, D, sample_rate=0.2, sparse_grad=True, **kw)
        assert ml.add_margin.sample_rate == 0.2 and ml.add_margin.sparse_grad and ml.add_margin.num_sample == 10
        assert SoftmaxBasedMetricLearning(nn.Identity(), C, D, **kw).add_margin.num_sample == C


# ------------------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize("rate,seed", [(0.2, 0), (0.5, 1), (0.98, 2), (6 / 50 + 1e-9, 3)])
def test_sample_equals_the_definition(rate, seed):
    h = _heads()["arc"](D, C, sample_rate=rate)
    _, label, score = _batch(seed)
    index, local = h.sample(label, score)
    want_index, want_local = _sample_definition(label, score, C, h.num_sample)
    assert index.dtype == torch.int32 and local.dtype == torch.int64
    assert index.tolist() == want_index and local.tolist() == want_local
    assert h.last_index is index
    assert set(label.tolist()) <= set(index.tolist())
    assert torch.equal(index.long()[local], label)


def test_sample_ties_go_to_the_lower_class():
    h = _heads()["arc"](D, C, sample_rate=0.4)          # S = 20
    label = torch.tensor([49, 3, 3, 17])
    for score in (torch.zeros(C), torch.full((C,), 0.5), (torch.arange(C) % 4).float() / 64):
        index, local = h.sample(label, score)
        want_index, want_local = _sample_definition(label, score, C, 20)
        assert index.tolist() == want_index and local.tolist() == want_local
    # S equal to the number of distinct positives: the index is exactly the positives
    h3 = _heads()["arc"](D, C, sample_rate=3 / 50 + 1e-9)
    assert h3.num_sample == 3
    index, local = h3.sample(torch.tensor([49, 3, 17]), torch.rand(C))
    assert index.tolist() == [3, 17, 49] and local.tolist() == [2, 0, 1]


def test_sample_draws_with_the_generator():
    h = _heads()["arc"](D, C, sample_rate=0.3)
    label = torch.tensor([1, 2, 3])
    h.sample_generator = torch.Generator().manual_seed(11)
    a, _ = h.sample(label)
    h.sample_generator = torch.Generator().manual_seed(11)
    b, _ = h.sample(label)
    score = torch.rand(C, generator=torch.Generator().manual_seed(11))
    assert torch.equal(a, b) and a.tolist() == _sample_definition(label, score, C, 15)[0]


def test_batch_larger_than_the_sample_is_refused():
    h = _heads()["arc"](D, C, sample_rate=0.1).train()          # S = 5 < B = 6
    emb, label, _ = _batch()
    with pytest.raises(ValueError, match="does not fit"):
        h(emb, label)


# ------------------------------------------------------------------------------------------------ CPU module against fp64
def _margin_logits64(kind, head, emb, w, label, state):
    """the full formulas of the heads in fp64 on the given centres (the same as scoring all classes, restricted to them)"""
    cos = F.normalize(emb) @ F.normalize(w).t()
    hot = F.one_hot(label, w.shape[0]).bool()
    s, m = head.s, head.m
    if kind == "cos":
        return s * torch.where(hot, cos - m, cos)
    if kind == "arc":
        phi = cos * math.cos(m) - torch.sqrt(1 - cos * cos) * math.sin(m)
        phi = torch.where(cos > math.cos(math.pi - m), phi, cos - math.sin(math.pi - m) * m)
        return s * torch.where(hot, phi, cos)
    if kind == "adaface":
        eps = head.eps
        c = cos.clamp(-1 + eps, 1 - eps)
        a = emb.detach().norm(dim=1).clip(1e-3, 100.0)
        mean = head.t_alpha * a.mean() + (1 - head.t_alpha) * state["batch_mean"]
        std = head.t_alpha * a.std() + (1 - head.t_alpha) * state["batch_std"]
        k = (head.h * (a - mean) / (std + eps)).clip(-1, 1)
        theta = torch.acos(c.gather(1, label[:, None]).squeeze(1))
        phi = torch.cos((theta - m * k).clip(eps, math.pi - eps)) - (m + m * k)
        return s * torch.where(hot, phi[:, None], c)
    c = cos.clamp(-1, 1)
    ct = c.gather(1, label[:, None]).squeeze(1)
    phi = ct * math.cos(m) - torch.sqrt((1 - ct * ct).clamp_min(0)) * math.sin(m)
    t = head.momentum * ct.detach().mean() + (1 - head.momentum) * state["t"]
    target = torch.where(ct > math.cos(math.pi - m), phi, ct - math.sin(math.pi - m) * m)
    neg = torch.where(c.detach() > phi.detach()[:, None], c * (t + c), c)
    return s * torch.where(hot, target[:, None], neg)


@pytest.mark.parametrize("kind", ["arc", "cos", "adaface", "curricular"])
@pytest.mark.parametrize("focal", [False, True])
def test_cpu_module_equals_the_restricted_fp64_oracle(kind, focal):
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    torch.manual_seed(3)
    kw = dict(arc_margin=True) if kind == "arc" else ({} if kind == "cos" else dict(margin=kind))
    ml = SoftmaxBasedMetricLearning(nn.Identity(), C, D, is_focal=focal, loss_kwargs=dict(gamma=2) if focal else None, sample_rate=0.3,
                                    **kw).train()
    head = ml.add_margin
    state = {k: v.double().clone() for k, v in head.named_buffers()}
    emb, label, score = _batch(4)
    emb.requires_grad_(True)
    index, local = head.sample(label, score)
    # pin the draw: the forward's torch.rand returns this score
    head.sample = lambda lab, sc=None, _f=head.sample: _f(lab, score)
    out = ml(emb, label)
    out["loss"].backward()
    assert torch.equal(out["classes"], index) and torch.equal(out["local_label"], local)
    assert out["logits"].shape == (B, head.num_sample)
    assert set(label.tolist()) <= set(index.tolist())

    e64 = emb.detach().double().requires_grad_(True)
    w64 = head.weight.detach().double().requires_grad_(True)
    logits = _margin_logits64(kind, head, e64, w64[index.long()], local, state)
    ce = F.cross_entropy(logits, local, reduction="none")
    loss = ((1 - torch.exp(-ce)) ** 2 * ce).mean() if focal else ce.mean()
    loss.backward()
    assert abs(out["loss"].item() - loss.item()) <= 1e-4 * max(1.0, abs(loss.item()))
    assert (out["logits"].double() - logits).abs().max() <= 1e-3

    def rel(a, b):
        return ((a.double() - b).norm() / b.norm().clamp_min(1e-30)).item()
    assert rel(emb.grad, e64.grad) < 1e-4
    assert rel(head.weight.grad, w64.grad) < 1e-4
    unsampled = torch.ones(C, dtype=torch.bool)
    unsampled[index.long()] = False
    assert unsampled.sum() == C - head.num_sample
    assert (head.weight.grad[unsampled] == 0).all()            # exactly zero, not merely small


# ------------------------------------------------------------------------------------------------ the default path is the head as it was
@pytest.mark.parametrize("kind", ["arc", "cos", "adaface", "curricular"])
def test_eval_and_full_rate_give_the_bits_of_a_plain_head(kind):
    cls = _heads()[kind]
    emb, label, _ = _batch(5)
    for make, mode in ((lambda: cls(D, C, sample_rate=1.0), "train"), (lambda: cls(D, C, sample_rate=0.3), "eval")):
        torch.manual_seed(1)
        plain = cls(D, C)           # (a fresh one each time: the adaptive heads move their buffers in training mode)
        torch.manual_seed(1)
        h = make()
        assert torch.equal(h.weight, plain.weight)
        getattr(plain, mode)()
        getattr(h, mode)()
        assert not h.sampling(label)
        a, b = plain(emb, label), h(emb, label)
        assert a.shape == (B, C) and torch.equal(a, b)


def test_wrapper_in_eval_mode_scores_all_classes():
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    emb, label, _ = _batch(6)
    torch.manual_seed(2)
    a = SoftmaxBasedMetricLearning(nn.Identity(), C, D, arc_margin=True).eval()
    torch.manual_seed(2)
    b = SoftmaxBasedMetricLearning(nn.Identity(), C, D, arc_margin=True, sample_rate=0.3).eval()
    oa, ob = a(emb, label), b(emb, label)
    assert torch.equal(oa["loss"], ob["loss"]) and torch.equal(oa["logits"], ob["logits"]) and "classes" not in ob
    assert torch.equal(b(emb), emb)                   # label is None: the embedding, no sampling


# ------------------------------------------------------------------------------------------------ refusals
def test_sub_centers_are_refused():
    for cls in _heads().values():
        with pytest.raises(ValueError, match="sub_centers"):
            cls(D, C, sub_centers=2, sample_rate=0.5)


def test_learnable_alpha_and_class_weight_are_refused():
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    with pytest.raises(ValueError, match="learnable focal alpha"):
        SoftmaxBasedMetricLearning(nn.Identity(), C, D, is_focal=True, loss_kwargs=dict(alpha=True), sample_rate=0.5)
    with pytest.raises(ValueError, match="class weight"):
        SoftmaxBasedMetricLearning(nn.Identity(), C, D, loss_kwargs=dict(weight=torch.ones(C)), sample_rate=0.5)
    # both stay available when every class is scored
    SoftmaxBasedMetricLearning(nn.Identity(), C, D, is_focal=True, loss_kwargs=dict(alpha=True))
    SoftmaxBasedMetricLearning(nn.Identity(), C, D, loss_kwargs=dict(weight=torch.ones(C)), sparse_grad=True)


def _row_grad_param():
    p = nn.Parameter(torch.zeros(8, 4))
    p.row_grad = (torch.tensor([1, 5], dtype=torch.int32), torch.ones(2, 4))
    return p


def test_adamw_refuses_a_row_gradient():
    from pets_face_recognition_amd._hip import PfrError
    from pets_face_recognition_amd.optim.fused import FusedAdamW
    opt = FusedAdamW([_row_grad_param()])
    with pytest.raises(PfrError, match="sparse_grad=False"):
        opt.step()


def test_an_attached_average_refuses_a_row_gradient():
    from pets_face_recognition_amd._hip import PfrError
    from pets_face_recognition_amd.optim.fused import FusedSGD
    for kind, decay in (("ema", 0.9), ("swa", None)):
        opt = FusedSGD([_row_grad_param()], 0.1, momentum=0.9)
        opt.attach_average(kind, decay)
        with pytest.raises(PfrError, match="sparse_grad=False"):
            opt.step()


def test_a_distributed_run_refuses_sparse_grad(monkeypatch):
    from pets_face_recognition_amd._hip import PfrError
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    h = _heads()["arc"](D, C, sample_rate=0.3, sparse_grad=True).train()
    _, label, _ = _batch()

    class _OnDevice:                 # the refusal is the CUDA path's (the CPU path has no row gradient): a label that says it is there
        is_cuda = True
    monkeypatch.setattr(type(h), "sample", lambda self, lab, score=None: (torch.zeros(15, dtype=torch.int32), torch.zeros(B, dtype=torch.int64)))
    with pytest.raises(PfrError, match="sparse_grad=False"):
        h._partial(_OnDevice())
    # sparse_grad=False trains on
    h.sparse_grad = False
    assert h._partial(_OnDevice()) is not None


def test_zero_grad_clears_the_row_gradient_and_clipping_sees_the_rows():
    from pets_face_recognition_amd.optim.fused import FusedSGD
    p = _row_grad_param()
    opt = FusedSGD([p], 0.1, momentum=0.9)
    assert len(opt._grads()) == 1 and opt._grads()[0] is p.row_grad[1]
    opt.zero_grad()
    assert p.row_grad is None and opt._grads() == []
