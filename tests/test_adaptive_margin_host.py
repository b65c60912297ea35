"""Host-side contract of the adaptive-margin heads, AdaFace (Kim et al., CVPR 2022) and CurricularFace (Huang et al., CVPR 2020); no GPU.

The CPU formulation of both heads (losses/large_margin.py) against an fp64 restatement written here from the definitions: forward
logits, loss, d emb and d weight to 1e-5 relative with the module in float32; the buffers over five training steps, eval mode, B = 1;
the two degenerate cases (AdaFace with h = 0 is CosFace on the clamped cosines, CurricularFace without a hard negative is ArcFace);
state dicts; `margin=None` builds what it built; the configs; the C-ABI declarations and the argument checks of the three new entry points."""
import ctypes
import math
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic")
B, C, D = 8, 37, 32
NEW_SYMBOLS = ("pfr_margin_prepare", "pfr_margin_ce_adaptive", "pfr_margin_bwd_adaptive")


# ------------------------------------------------------------------------------------------------ the definitions, in the dtype of `cos`
def ada_prepare(norm, state, m=0.4, h=0.333, t_alpha=0.01, eps=1e-3, train=True):
    """norms [B], state (batch_mean, batch_std) -> (g_ang [B], g_add [B], new state)"""
    bm, bs = state
    a = norm.clamp_min(1e-12).clip(1e-3, 100.0)
    if train:
        bm = t_alpha * a.mean() + (1.0 - t_alpha) * bm
        if a.numel() > 1:
            bs = t_alpha * a.std(unbiased=True) + (1.0 - t_alpha) * bs
    k = (h * (a - bm) / (bs + eps)).clip(-1.0, 1.0)
    return -m * k, m + m * k, (bm, bs)


def ada_logits(cos, label, g_ang, g_add, s=64.0, eps=1e-3):
    c = cos.clamp(-1.0 + eps, 1.0 - eps)
    theta = torch.acos(c[torch.arange(len(label)), label])
    phi = torch.cos((theta + g_ang.detach()).clip(eps, math.pi - eps)) - g_add.detach()
    hot = F.one_hot(label, cos.shape[1]).bool()
    return s * torch.where(hot, phi[:, None], c)


def cur_logits(cos, label, t, m=0.5, s=64.0, momentum=0.01, train=True):
    """-> (logits, the t this step used)"""
    c = cos.clamp(-1.0, 1.0)
    ct = c[torch.arange(len(label)), label]
    phi = ct * math.cos(m) - torch.sqrt(1.0 - ct * ct) * math.sin(m)
    if train:
        t = momentum * ct.detach().mean() + (1.0 - momentum) * t
    target = torch.where(ct > math.cos(math.pi - m), phi, ct - m * math.sin(math.pi - m))
    hard = c.detach() > phi.detach()[:, None]
    neg = torch.where(hard, c * (t + c), c)
    hot = F.one_hot(label, cos.shape[1]).bool()
    return s * torch.where(hot, target[:, None], neg), t


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _wrap(margin, seed=0, **kw):
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    torch.manual_seed(seed)
    return SoftmaxBasedMetricLearning(nn.Identity(), C, embedding_size=D, margin=margin, **kw)


def _draw(seed=3, K=1, b=B):
    """embeddings with norms between 5 and 40 (AdaFace's k takes both signs), pulled towards their class centre"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(C * K, D, generator=g)
    label = torch.randint(0, C, (b,), generator=g)
    x = F.normalize(torch.randn(b, D, generator=g) + 6.0 * F.normalize(w[label * K]))
    x = x * (5.0 + 35.0 * torch.rand(b, 1, generator=g))
    return x, w, label


def _reference(margin, x, w, label, state, K=1, train=True, **kw):
    """fp64 restatement of the whole head on the fp32 values of x and w -> (logits, loss, dx, dw, new state)"""
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    cos = F.normalize(x64) @ F.normalize(w64).t()
    if K > 1:
        cos = cos.view(len(label), C, K).max(2).values
    if margin == "adaface":
        g_ang, g_add, state = ada_prepare(x64.detach().norm(dim=1), state, train=train, **kw)
        logits = ada_logits(cos, label, g_ang, g_add)
    else:
        logits, t = cur_logits(cos, label, state[0], train=train, **kw)
        state = (t,)
    loss = F.cross_entropy(logits, label)
    loss.backward()
    return logits.detach(), loss.detach(), x64.grad, w64.grad, state


def _state_of(head):
    return (head.batch_mean, head.batch_std) if hasattr(head, "batch_mean") else (head.t,)


CASES = {
    "adaface": ("adaface", (20.0, 100.0), 1),
    "adaface_clipped_k": ("adaface", (22.0, 5.0), 1),      # |h (a - mean) / std| > 1 on several rows
    "adaface_k3": ("adaface", (20.0, 100.0), 3),
    "curricular": ("curricular", (0.0,), 1),
    "curricular_t": ("curricular", (0.6,), 1),
    "curricular_k3": ("curricular", (0.3,), 3),
}


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_module_vs_fp64_restatement(name):
    margin, state0, K = CASES[name]
    x, w, label = _draw(K=K)
    wrap = _wrap(margin, sub_centers=K).train()
    head = wrap.add_margin
    with torch.no_grad():
        head.weight.copy_(w)
        for buf, v in zip(_state_of(head), state0):
            buf.fill_(v)
    x32 = x.clone().requires_grad_(True)
    r = wrap(x32, label)
    r["loss"].backward()
    logits, loss, dx, dw, state = _reference(margin, x, w, label, tuple(torch.tensor(v, dtype=torch.float64) for v in state0), K=K)
    figs = dict(logits=_rel(r["logits"], logits), loss=abs(r["loss"].item() - loss.item()) / abs(loss.item()), dx=_rel(x32.grad, dx),
                dw=_rel(head.weight.grad, dw), state=[abs(b.item() - v.item()) / max(abs(v.item()), 1e-30) for b, v in zip(_state_of(head), state)])
    print(f"adaptive margin cpu module {name}: {figs}")
    assert r["logits"].shape == (B, C) and r["logits"].dtype == torch.float32
    assert figs["logits"] < 1e-5 and figs["loss"] < 1e-5 and figs["dx"] < 1e-5 and figs["dw"] < 1e-5
    assert all(e < 1e-5 for e in figs["state"])
    if margin == "adaface":
        g_ang = ada_prepare(x.double().norm(dim=1), tuple(torch.tensor(v, dtype=torch.float64) for v in state0))[0]
        saturated = (g_ang.abs() == 0.4).sum().item()
        assert (saturated > 0) == (name == "adaface_clipped_k") and saturated < B
    else:
        cos = F.normalize(x.double()) @ F.normalize(w.double()).t()
        if K > 1:
            cos = cos.view(B, C, K).max(2).values
        ct = cos[torch.arange(B), label]
        hard = cos > (ct * math.cos(0.5) - torch.sqrt(1 - ct * ct) * math.sin(0.5))[:, None]
        hard[torch.arange(B), label] = False
        print(f"  hard negatives: {hard.sum().item()} of {B * (C - 1)}")
        assert 0 < hard.sum().item() < B * (C - 1)          # both kinds of negative occur


@pytest.mark.parametrize("margin", ["adaface", "curricular"])
def test_buffers_follow_the_definitions_over_five_steps(margin):
    wrap = _wrap(margin).train()
    head = wrap.add_margin
    _, w, _ = _draw()
    with torch.no_grad():
        head.weight.copy_(w)
    state = tuple(b.double().squeeze(0).clone() for b in _state_of(head))
    assert [v.item() for v in state] == ([20.0, 100.0] if margin == "adaface" else [0.0])
    for step in range(5):
        x, _, label = _draw(seed=10 + step)
        wrap(x, label)
        *_, state = _reference(margin, x, w, label, state)
        for b, v in zip(_state_of(head), state):
            assert b.dtype == torch.float32 and b.shape == (1,)
            assert abs(b.item() - v.item()) <= 1e-5 * abs(v.item()), (step, b.item(), v.item())
    assert all(abs(b.item() - v0) > 1e-4 for b, v0 in zip(_state_of(head), (20.0, 100.0)))      # they moved
    wrap.eval()
    before = [b.clone() for b in _state_of(head)]
    r_eval = wrap(x, label)
    assert all(torch.equal(a, b) for a, b in zip(before, _state_of(head)))
    # eval uses the buffers as they are
    logits, *_ = _reference(margin, x, w, label, tuple(b.double().squeeze(0) for b in before), train=False)
    assert _rel(r_eval["logits"], logits) < 1e-5


@pytest.mark.parametrize("margin", ["adaface", "curricular"])
def test_batch_of_one(margin):
    wrap = _wrap(margin).train()
    head = wrap.add_margin
    x, _, label = _draw(b=1)
    x.requires_grad_(True)
    r = wrap(x, label)
    r["loss"].backward()
    assert torch.isfinite(r["logits"]).all() and torch.isfinite(r["loss"]) and torch.isfinite(x.grad).all()
    assert torch.isfinite(head.weight.grad).all()
    assert all(torch.isfinite(b).all() for b in _state_of(head))
    if margin == "adaface":
        assert head.batch_std.item() == 100.0                                   # the deviation of one sample is undefined
        assert head.batch_mean.item() == pytest.approx(0.01 * x.detach().norm().item() + 0.99 * 20.0, rel=1e-6)


def test_adaface_without_h_is_cosface_on_the_clamped_cosines():
    wrap = _wrap("adaface", margin_kwargs=dict(h=0.0, m=0.35)).train()
    head = wrap.add_margin
    x, _, label = _draw()
    with torch.no_grad():
        head.weight[label[0]] = x[0]           # a cosine of 1: the clamp is active
    logits = wrap(x, label)["logits"]
    c = (F.normalize(x.double()) @ F.normalize(head.weight.detach().double()).t()).clamp(-1 + 1e-3, 1 - 1e-3)
    assert c.max().item() == 1 - 1e-3
    hot = F.one_hot(label, C).double()
    want = 64.0 * (hot * (c - 0.35) + (1.0 - hot) * c)
    assert _rel(logits, want) < 1e-5


def test_curricular_without_hard_negatives_is_arcface():
    from pets_face_recognition_amd.losses import ArcMarginProduct, CurricularFaceProduct
    g = torch.Generator().manual_seed(7)
    cos = -0.5 - 0.49 * torch.rand(B, C, generator=g)                  # negatives <= -0.5
    label = torch.randint(0, C, (B,), generator=g)
    cos[torch.arange(B), label] = 0.3 + 0.6 * torch.rand(B, generator=g)   # targets >= 0.3: cos(theta + 0.5) >= -0.2
    cur = CurricularFaceProduct(D, C, s=64.0, m=0.5).train()
    cur.t.fill_(0.7)
    arc = ArcMarginProduct(D, C, s=64.0, m=0.5)
    hot = F.one_hot(label, C).to(cos.dtype)
    want = arc.s * (hot * arc._target_logit(cos) + (1.0 - hot) * cos)
    got = cur._adaptive_logits(torch.zeros(B, D), cos, label)
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-5)
    assert cur.t.item() != pytest.approx(0.7)                           # t moved all the same


def test_state_dict_round_trip():
    for margin, keys in (("adaface", {"add_margin.weight", "add_margin.batch_mean", "add_margin.batch_std"}),
                         ("curricular", {"add_margin.weight", "add_margin.t"})):
        a = _wrap(margin, seed=1).train()
        x, _, label = _draw()
        a(x, label)
        sd = a.state_dict()
        assert set(sd) == keys
        assert all(sd[k].dtype == torch.float32 and sd[k].shape == (1,) for k in keys if k != "add_margin.weight")
        b = _wrap(margin, seed=2)
        b.load_state_dict(sd)
        assert all(torch.equal(p, q) for p, q in zip(_state_of(a.add_margin), _state_of(b.add_margin)))
        a.eval(), b.eval()
        assert torch.equal(a(x, label)["logits"], b(x, label)["logits"])


def test_margin_none_builds_what_it_built():
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning, ArcMarginProduct, AddMarginProduct
    for kw, cls in ((dict(arc_margin=True), ArcMarginProduct), (dict(arc_margin=True, easy_margin=True), ArcMarginProduct),
                    (dict(), AddMarginProduct), (dict(arc_margin=True, sub_centers=2), ArcMarginProduct)):
        torch.manual_seed(4)
        old = SoftmaxBasedMetricLearning(nn.Identity(), C, embedding_size=D, **kw)
        torch.manual_seed(4)
        new = SoftmaxBasedMetricLearning(nn.Identity(), C, embedding_size=D, margin=None, margin_kwargs=None, **kw)
        assert type(new.add_margin) is cls and type(old.add_margin) is cls
        assert list(new.state_dict()) == list(old.state_dict()) == ["add_margin.weight"]
        assert torch.equal(new.add_margin.weight, old.add_margin.weight)
        assert new.add_margin.hip_adaptive() is None
        assert new.add_margin.easy_margin == kw.get("easy_margin", False) if cls is ArcMarginProduct else True


def test_margin_selects_the_new_heads_and_rejects_the_rest():
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    from pets_face_recognition_amd.losses.large_margin import AdaFaceProduct, CurricularFaceProduct, _MarginHead
    ada = _wrap("adaface", sub_centers=2).add_margin
    assert type(ada) is AdaFaceProduct and isinstance(ada, _MarginHead)
    assert (ada.s, ada.m, ada.h, ada.t_alpha, ada.sub_centers) == (64.0, 0.4, 0.333, 0.01, 2) and tuple(ada.weight.shape) == (2 * C, D)
    cur = _wrap("curricular", margin_kwargs=dict(m=0.45, momentum=0.02)).add_margin
    assert type(cur) is CurricularFaceProduct and (cur.s, cur.m, cur.momentum) == (64.0, 0.45, 0.02)
    for bad in ("arcface", "AdaFace", "", 0):
        with pytest.raises(ValueError, match="margin"):
            SoftmaxBasedMetricLearning(nn.Identity(), C, embedding_size=D, margin=bad)


def test_sub_centres_count_and_prune():
    wrap = _wrap("adaface", sub_centers=3).train()
    head = wrap.add_margin
    x, _, label = _draw()
    wrap(x, label)
    assert head.sub_center_count.sum().item() == B
    head.prune_sub_centers()
    assert head.sub_centers == 1 and tuple(head.weight.shape) == (C, D)
    assert wrap(x, label)["logits"].shape == (B, C)


@pytest.mark.parametrize("name", ["fe_r18_mi355x_adaface.py", "fe_r18_mi355x_curricular.py"])
def test_new_configs_load_without_a_gpu(name, tmp_path, monkeypatch):
    import pets_face_recognition_amd as pfr
    from pets_face_recognition_amd.losses.large_margin import AdaFaceProduct, CurricularFaceProduct
    pfr.install_reference_aliases()
    monkeypatch.chdir(tmp_path)
    from pets_face_recognition_amd.utils import get_dict_wrapper
    ns = dict(get_dict_wrapper(os.path.join(SYNTH, name)).__dict__)
    assert ns["device"] == "cuda:0" and ns["n_epochs"] == 1
    wrap = ns["loss"](None, nn.Identity())
    assert type(wrap.add_margin) is (AdaFaceProduct if "adaface" in name else CurricularFaceProduct)
    assert wrap.add_margin.out_features == 100


def test_config_builder_passes_the_margin_only_when_set():
    src = open(os.path.join(SYNTH, "_common.py")).read()
    sig = src[src.index("def make("):src.index("torch.manual_seed(seed)")]
    assert "margin=None" in sig and "margin_kwargs=None" in sig
    assert "**margin_args" in src and "if margin is not None" in src and "if margin_kwargs is not None" in src


# ------------------------------------------------------------------------------------------------ C-ABI
def test_new_entry_points_declared_and_exported():
    from pets_face_recognition_amd._hip.lib import LIB_PATH, parse_header
    protos = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos, f"{name} not declared in include/pfr_hip.h"
        assert hasattr(dll, name), f"{name} not exported by libpfr_hip.so"
    inc = open(os.path.join(os.path.dirname(LIB_PATH), "pfr_thunks_gen.inc")).read()
    for name in NEW_SYMBOLS:
        assert f'{{"{name}", th_{name}}}' in inc
    # the existing entry points keep their prototypes
    assert protos["pfr_margin_ce"][2] == ["cosv", "label", "B", "C", "ldc", "mode", "s", "m", "gamma", "grad_scale", "grad_scale_dev", "logits",
                                          "loss_rows", "dcos", "dcos_dtype", "stream"]
    assert protos["pfr_margin_bwd"][2] == ["cosv", "label", "B", "C", "ldc", "mode", "s", "m", "dlogits", "dcos", "dcos_dtype", "stream"]
    assert len(protos["pfr_margin_ce_ex"][2]) == 21 and len(protos["pfr_alpha_grad"][2]) == 12


def _prep(lib, kind=0, inv=16, cos=16, label=16, B_=2, ldc=8, mom=0.01, s0=16, s1=16, rm=16, su=16):
    # pointers are never dereferenced on the host: every call below must fail its argument check before any launch
    return lib.pfr_margin_prepare(kind, inv, cos, label, B_, ldc, 0.4, 0.333, mom, 1e-3, 1, s0, s1, rm, su, 0)


def _ce(lib, cos=16, label=16, B_=2, C_=8, ldc=8, kind=0, eps=1e-3, gamma=0.0, weight=0, e=0.0, rm=16, su=16, dev2=0, dtype=0):
    return lib.pfr_margin_ce_adaptive(cos, label, B_, C_, ldc, kind, 64.0, 0.4, eps, gamma, weight, e, rm, su, 1.0, 0, dev2, 0, 0, 0, 0, dtype, 0)


def _bwd(lib, cos=16, label=16, B_=2, C_=8, ldc=8, kind=0, eps=1e-3, rm=16, su=16, dl=16, dcos=16, dtype=0):
    return lib.pfr_margin_bwd_adaptive(cos, label, B_, C_, ldc, kind, 64.0, 0.4, eps, rm, su, dl, dcos, dtype, 0)


def test_new_entry_points_reject_bad_arguments():
    from pets_face_recognition_amd._hip import lib, PfrError
    for kw, msg in ((dict(kind=2), "bad margin kind"), (dict(B_=0), "bad shape"), (dict(s0=0), "null pointer"), (dict(su=0), "null pointer"),
                    (dict(inv=0), "null pointer"), (dict(s1=0), "null pointer"), (dict(rm=0), "null pointer"), (dict(mom=1.5), "momentum"),
                    (dict(kind=1, cos=0), "null pointer"), (dict(kind=1, label=0), "null pointer")):
        with pytest.raises(PfrError, match=msg):
            _prep(lib, **kw)
    for call in (_ce, _bwd):
        for kw, msg in ((dict(cos=0), "null pointer"), (dict(label=0), "null pointer"), (dict(B_=0), "bad shape"), (dict(ldc=4), "bad shape"),
                        (dict(kind=-1), "bad margin kind"), (dict(rm=0), "null pointer"), (dict(kind=1, su=0), "null pointer"),
                        (dict(eps=0.0), "eps"), (dict(dtype=2), "dcos dtype")):
            with pytest.raises(PfrError, match=msg):
                call(lib, **kw)
    for e in (-0.1, 1.5, float("nan")):
        with pytest.raises(PfrError, match="label_smoothing"):
            _ce(lib, e=e)
    with pytest.raises(PfrError, match="gamma excludes"):
        _ce(lib, gamma=2.0, e=0.1)
    with pytest.raises(PfrError, match="grad_scale_dev2"):
        _ce(lib, dev2=16)
    with pytest.raises(PfrError, match="null pointer"):
        _bwd(lib, dl=0)


def test_wrappers_refuse_cpu_tensors_and_bad_kinds():
    from pets_face_recognition_amd._hip import ops, PfrError
    cos, label = torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64)
    one = torch.zeros(1)
    with pytest.raises(PfrError, match="margin kind"):
        ops.margin_prepare("arc", (one,), 2, cosv=cos, label=label)
    with pytest.raises(PfrError, match="no CPU fallback"):
        ops.margin_prepare("curricular", (one,), 2, cosv=cos, label=label)
    with pytest.raises(PfrError, match="state buffer"):
        ops.margin_prepare("adaface", (one,), 2, inv_norm=torch.ones(2))
    with pytest.raises(PfrError, match="no CPU fallback"):
        ops.margin_ce_adaptive(cos, label, 8, "adaface", 64.0, 0.4, 1e-3, torch.zeros(2, 2), torch.zeros(2))
    with pytest.raises(PfrError, match="margin kind"):
        ops.margin_bwd_adaptive(cos, label, 8, "cos", 64.0, 0.4, 1e-3, None, torch.zeros(2), torch.zeros(2, 8), torch.float32)
