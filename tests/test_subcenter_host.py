"""Host-side contract of the sub-centre head (K centres per class, Sub-center ArcFace / CosFace; no GPU): constructors and state dict,
`sub_centers=1` is the head as it was, the CPU path against an fp64 formulation written here, the sub-centre histogram and the pruning
step, and the two new C-ABI entry points' declarations and argument checks.

The fp64 formulation: normalise, matmul, `view(B, C, K).max(2)`, the margin of losses/large_margin.py, cross-entropy.  Bounds are the
module-free ones tests/test_head_criterion_gpu.py states for this head: logits rtol 1e-5 / atol 1e-4, gradients relative L2 < 1e-4."""
import ctypes
import math
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

B, C, K, D = 8, 37, 3, 32
NEW_SYMBOLS = ("pfr_subcenter_pool", "pfr_subcenter_scatter")


def _wrap(mode="arc", seed=0, **kw):
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    torch.manual_seed(seed)
    return SoftmaxBasedMetricLearning(nn.Identity(), C, embedding_size=D, arc_margin=mode != "cos", easy_margin=mode == "arc_easy", **kw)


def _draw(seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g, dtype=torch.float64)
    w = torch.randn(C * K, D, generator=g, dtype=torch.float64)
    label = torch.randint(0, C, (B,), generator=g)
    return x, w, label


def _margin64(cos, label, mode, s, m):
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


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def test_constructs_with_sub_centers():
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    model = nn.Identity()
    wrap = SoftmaxBasedMetricLearning(model, 37, embedding_size=32, arc_margin=True, sub_centers=3)
    assert tuple(wrap.add_margin.weight.shape) == (111, 32)
    assert wrap.add_margin.out_features == 37 and wrap.add_margin.sub_centers == 3
    assert tuple(wrap.add_margin.sub_center_count.shape) == (37, 3) and wrap.add_margin.sub_center_count.dtype == torch.int32
    assert set(wrap.state_dict()) == {"add_margin.weight"}            # the histogram is not persistent
    cosf = SoftmaxBasedMetricLearning(model, 37, embedding_size=32, sub_centers=2)
    assert tuple(cosf.add_margin.weight.shape) == (74, 32)
    bound = math.sqrt(6.0 / (111 + 32))                              # Xavier-uniform over the [C*K, D] matrix
    assert wrap.add_margin.weight.abs().max().item() <= bound
    for bad in (0, 17):
        with pytest.raises(ValueError):
            SoftmaxBasedMetricLearning(model, 37, embedding_size=32, sub_centers=bad)


@pytest.mark.parametrize("mode", ["arc", "arc_easy", "cos"])
def test_one_sub_center_is_the_head_as_it_was(mode):
    a, b = _wrap(mode, seed=11), _wrap(mode, seed=11, sub_centers=1)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(sa[k].shape == sb[k].shape for k in sa)
    assert torch.equal(a.add_margin.weight, b.add_margin.weight)
    assert not any("sub_center_count" in k for k in sb)
    assert not hasattr(b.add_margin, "sub_center_count")
    x, _, label = _draw()
    ra, rb = a(x.float(), label), b(x.float(), label)
    assert torch.equal(ra["logits"], rb["logits"]) and torch.equal(ra["loss"], rb["loss"])
    # today's arithmetic, restated: s * (onehot * phi + (1 - onehot) * cos) of F.normalize(x) @ F.normalize(w).t()
    head = a.add_margin
    cos = F.normalize(x.float()) @ F.normalize(head.weight).t()
    hot = F.one_hot(label, C).to(cos.dtype)
    assert torch.equal(rb["logits"], head.s * (hot * head._target_logit(cos) + (1.0 - hot) * cos))
    assert torch.equal(b.add_margin.dominant_sub_centers(), torch.zeros(C, dtype=torch.long))


@pytest.mark.parametrize("mode", ["arc", "arc_easy", "cos"])
def test_cpu_module_vs_fp64_formulation(mode):
    x, w, label = _draw()
    wrap = _wrap(mode, sub_centers=K)
    with torch.no_grad():
        wrap.add_margin.weight.copy_(w)
    x32 = x.float().requires_grad_(True)
    r = wrap(x32, label)
    r["loss"].backward()
    assert r["logits"].shape == (B, C)
    x64 = x.float().double().requires_grad_(True)
    w64 = wrap.add_margin.weight.detach().double().requires_grad_(True)
    cos_sub = F.normalize(x64) @ F.normalize(w64).t()
    top2 = cos_sub.view(B, C, K).topk(2, dim=2).values
    assert (top2[..., 0] - top2[..., 1]).min().item() > 1e-4          # no (row, class) pair near a tie: fp32 and fp64 select alike
    cos = cos_sub.view(B, C, K).max(2).values
    logits = _margin64(cos, label, mode, wrap.add_margin.s, wrap.add_margin.m)
    loss = F.cross_entropy(logits, label)
    loss.backward()
    figs = dict(loss=r["loss"].item(), loss_ref=loss.item(), dx=_rel(x32.grad, x64.grad), dw=_rel(wrap.add_margin.weight.grad, w64.grad))
    print(f"sub-centre cpu module {mode}: {figs}")
    assert torch.allclose(r["logits"].double(), logits.detach(), rtol=1e-5, atol=1e-4)
    assert abs(figs["loss"] - figs["loss_ref"]) < 1e-4 * max(1.0, abs(figs["loss_ref"]))
    assert figs["dx"] < 1e-4 and figs["dw"] < 1e-4
    # routing: a sub-centre that no row selected gets exactly no gradient
    arg = cos_sub.view(B, C, K).argmax(2)
    sel = torch.zeros(C, K, dtype=torch.bool)
    sel[torch.arange(C).expand(B, C), arg] = True
    assert wrap.add_margin.weight.grad.view(C, K, D)[~sel].abs().max().item() == 0.0


def test_histogram_dominant_and_prune():
    from pets_face_recognition_amd.losses import ArcMarginProduct
    _, w, _ = _draw()
    wrap = _wrap("arc", sub_centers=K)
    head = wrap.add_margin
    with torch.no_grad():
        head.weight.copy_(w)
    g = torch.Generator().manual_seed(5)
    want = torch.zeros(C * K, dtype=torch.long)
    wrap.train()
    for _ in range(4):
        x = torch.randn(B, D, generator=g)
        label = torch.randint(0, C, (B,), generator=g)
        wrap(x, label)
        arg = (F.normalize(x) @ F.normalize(head.weight).t()).view(B, C, K).argmax(2)
        want += torch.bincount(label * K + arg[torch.arange(B), label], minlength=C * K)
    assert head.sub_center_count.sum().item() == 4 * B
    assert torch.equal(head.sub_center_count.view(-1).long(), want)
    wrap.eval()
    wrap(x, label)
    assert torch.equal(head.sub_center_count.view(-1).long(), want)          # evaluation does not count
    wrap.train()
    # dominant: the argmax of the count, the lowest index on ties
    cnt = want.view(C, K)
    dom = head.dominant_sub_centers()
    assert dom.dtype == torch.long and dom.shape == (C,)
    for c in range(C):
        assert dom[c].item() == min(k for k in range(K) if cnt[c, k] == cnt[c].max())
    assert (cnt.max(1).values == 0).any() and (cnt.max(1).values > 0).any()    # both the tie (unseen class) and the counted case occur
    # prune: row c*K + dominant[c] survives, the head is a one-centre head from then on
    old = head.weight.detach().clone()
    kept = head.prune_sub_centers()
    assert torch.equal(kept, dom)
    assert head.sub_centers == 1 and tuple(head.weight.shape) == (C, D)
    assert torch.equal(head.weight.detach(), old[torch.arange(C) * K + dom])
    assert not hasattr(head, "sub_center_count") and set(wrap.state_dict()) == {"add_margin.weight"}
    plain = ArcMarginProduct(D, C, s=head.s, m=head.m)
    plain.load_state_dict(head.state_dict())
    x = torch.randn(B, D, generator=g).requires_grad_(True)
    out = head(x, label)
    assert torch.equal(out, plain(x, label))
    out.sum().backward()
    assert tuple(head.weight.grad.shape) == (C, D)
    fresh = _wrap("arc")
    fresh.load_state_dict(wrap.state_dict())
    assert torch.equal(fresh(x, label)["logits"], wrap(x, label)["logits"])
    head.reset_sub_center_count()                                              # nothing left to reset: a no-op


def test_reset_sub_center_count():
    wrap = _wrap("cos", sub_centers=2).train()
    x, _, label = _draw()
    wrap(x.float(), label)
    assert wrap.add_margin.sub_center_count.sum().item() == B
    wrap.add_margin.reset_sub_center_count()
    assert wrap.add_margin.sub_center_count.sum().item() == 0


def test_new_entry_points_declared_and_exported():
    from pets_face_recognition_amd._hip.lib import LIB_PATH, parse_header
    protos = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos, f"{name} not declared in include/pfr_hip.h"
        assert hasattr(dll, name), f"{name} not exported by libpfr_hip.so"
    assert protos["pfr_subcenter_pool"][2] == ["cos_sub", "B", "C", "K", "ld_sub", "cos", "ldc", "arg", "label", "count", "stream"]
    assert protos["pfr_subcenter_scatter"][2] == ["dcos", "dtype", "arg", "B", "C", "K", "ldc", "dcos_sub", "ld_sub", "stream"]
    inc = open(os.path.join(os.path.dirname(LIB_PATH), "pfr_thunks_gen.inc")).read()
    for name in NEW_SYMBOLS:
        assert f'{{"{name}", th_{name}}}' in inc


def _pool(lib, cos_sub=16, Kk=3, ld_sub=24, cos=16, ldc=8, arg=16, label=0, count=0):
    # pointers are never dereferenced on the host: every call below must fail its argument check before any launch
    return lib.pfr_subcenter_pool(cos_sub, 2, 8, Kk, ld_sub, cos, ldc, arg, label, count, 0)


def _scatter(lib, dcos=16, dtype=0, arg=16, Kk=3, ldc=8, out=16, ld_sub=24):
    return lib.pfr_subcenter_scatter(dcos, dtype, arg, 2, 8, Kk, ldc, out, ld_sub, 0)


@pytest.mark.parametrize("call", [_pool, _scatter], ids=["pool", "scatter"])
def test_new_entry_points_reject_bad_arguments(call):
    from pets_face_recognition_amd._hip import lib, PfrError
    for kw, msg in ((dict(Kk=0), "outside 1..16"), (dict(Kk=17), "outside 1..16"), (dict(ldc=7), "bad shape"), (dict(ld_sub=23), "bad shape"),
                    (dict(arg=0), "null pointer")):
        with pytest.raises(PfrError, match=msg) as e:
            call(lib, **kw)
        assert "rc=-1" in str(e.value) and call.__name__.strip("_") in str(e.value)


def test_pool_specific_argument_errors():
    from pets_face_recognition_amd._hip import lib, PfrError
    with pytest.raises(PfrError, match="null pointer"):
        _pool(lib, cos_sub=0)
    with pytest.raises(PfrError, match="go together"):
        _pool(lib, label=16)
    with pytest.raises(PfrError, match="go together"):
        _pool(lib, count=16)
    with pytest.raises(PfrError, match="bad dtype"):
        _scatter(lib, dtype=2)
