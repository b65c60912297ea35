"""Host-side contract of the criterion-general fused head (no GPU): the new C-ABI entry points exist and check their arguments before
they touch the device, and `SoftmaxBasedMetricLearning._fusable` describes exactly the supported `loss_kwargs` sets."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn

NEW_SYMBOLS = ("pfr_margin_ce_ex", "pfr_alpha_grad", "pfr_loss_reduce")


def test_new_entry_points_declared_and_exported():
    from pets_face_recognition_amd._hip.lib import LIB_PATH, parse_header
    protos = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos, f"{name} not declared in include/pfr_hip.h"
        assert hasattr(dll, name), f"{name} not exported by libpfr_hip.so"
    # the existing entry point keeps its prototype
    assert protos["pfr_margin_ce"][2] == ["cosv", "label", "B", "C", "ldc", "mode", "s", "m", "gamma", "grad_scale", "grad_scale_dev", "logits",
                                          "loss_rows", "dcos", "dcos_dtype", "stream"]
    names = protos["pfr_margin_ce_ex"][2]
    for a in ("alpha", "class_weight", "label_smoothing", "row_stats"):
        assert a in names
    # and the plan executor's thunk table knows them
    inc = open(os.path.join(os.path.dirname(LIB_PATH), "pfr_thunks_gen.inc")).read()
    for name in NEW_SYMBOLS:
        assert f'{{"{name}", th_{name}}}' in inc


def _ex(lib, cosv=16, label=16, B=2, C=8, ldc=8, mode=0, gamma=0.0, alpha=0, weight=0, e=0.0, dev2=0, dtype=0):
    # pointers are never dereferenced on the host: every call below must fail its argument check before any launch
    return lib.pfr_margin_ce_ex(cosv, label, B, C, ldc, mode, 64.0, 0.5, gamma, alpha, weight, e, 1.0, 0, dev2, 0, 0, 0, 0, dtype, 0)


def test_new_entry_points_reject_bad_arguments():
    from pets_face_recognition_amd._hip import lib, PfrError
    with pytest.raises(PfrError, match="null pointer"):
        _ex(lib, cosv=0)
    with pytest.raises(PfrError, match="null pointer"):
        _ex(lib, label=0)
    with pytest.raises(PfrError, match="bad shape"):
        _ex(lib, B=0)
    with pytest.raises(PfrError, match="bad shape"):
        _ex(lib, C=8, ldc=4)
    with pytest.raises(PfrError, match="bad margin mode"):
        _ex(lib, mode=4)
    for e in (-0.1, 1.5, float("nan")):
        with pytest.raises(PfrError, match="label_smoothing"):
            _ex(lib, e=e)
    with pytest.raises(PfrError, match="dcos dtype"):
        _ex(lib, dtype=2)
    with pytest.raises(PfrError, match="alpha excludes"):
        _ex(lib, alpha=16, weight=16)
    with pytest.raises(PfrError, match="alpha excludes"):
        _ex(lib, alpha=16, e=0.1)
    with pytest.raises(PfrError, match="gamma excludes"):
        _ex(lib, gamma=2.0, e=0.1)
    with pytest.raises(PfrError, match="grad_scale_dev2"):
        _ex(lib, dev2=16)
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_alpha_grad(16, 16, 0, 16, 2, 8, 8, 64.0, 1.0, 0, 16, 0)
    with pytest.raises(PfrError, match="null pointer"):
        lib.pfr_alpha_grad(16, 16, 16, 0, 2, 8, 8, 64.0, 1.0, 0, 16, 0)
    with pytest.raises(PfrError, match="bad shape"):
        lib.pfr_alpha_grad(16, 16, 16, 16, 2, 8, 7, 64.0, 1.0, 0, 16, 0)
    with pytest.raises(PfrError, match="bad args"):
        lib.pfr_loss_reduce(0, 0, 4, 0, 16, 0, 0)
    with pytest.raises(PfrError, match="bad reduction"):
        lib.pfr_loss_reduce(16, 0, 4, 3, 16, 0, 0)
    with pytest.raises(PfrError, match="row_stats"):
        lib.pfr_loss_reduce(16, 0, 4, 2, 16, 0, 0)


class _DeviceEmb:
    """stand-in for a [B, 512] embedding that lives on a device (`_fusable` only looks at these attributes); its 'device' is the CPU so
    that the criterion's tensors count as being on the embedding's device"""
    is_cuda = True
    device = torch.device("cpu")
    shape = (4, 512)

    def dim(self):
        return 2


C = 10


def _wrap(is_focal, **loss_kwargs):
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    return SoftmaxBasedMetricLearning(nn.Identity(), C, 512, is_focal=is_focal, loss_kwargs=loss_kwargs, arc_margin=True)


def test_fusable_is_none_on_cpu_tensors():
    for wrap in (_wrap(True), _wrap(True, alpha=True), _wrap(False, label_smoothing=0.1)):
        assert wrap._fusable(torch.zeros(4, 512)) is None


def test_fusable_describes_each_supported_criterion():
    emb = _DeviceEmb()
    w = torch.rand(C) + 0.5
    d = _wrap(True)._fusable(emb)
    assert (d.gamma, d.alpha, d.weight, d.smoothing, d.reduction) == (0.0, None, None, 0.0, "mean") and d.is_plain
    d = _wrap(True, gamma=2)._fusable(emb)
    assert d.gamma == 2.0 and d.is_plain
    wrap = _wrap(True, gamma=2, alpha=True)
    d = wrap._fusable(emb)
    assert d.gamma == 2.0 and d.alpha is wrap.focal_loss.alpha and d.weight is None and d.reduction == "mean" and not d.is_plain
    d = _wrap(False)._fusable(emb)
    assert d.is_plain and d.gamma == 0.0
    d = _wrap(False, label_smoothing=0.1)._fusable(emb)
    assert (d.gamma, d.alpha, d.weight, d.smoothing, d.reduction) == (0.0, None, None, 0.1, "mean") and not d.is_plain
    d = _wrap(False, weight=w)._fusable(emb)
    assert torch.equal(d.weight, w) and d.smoothing == 0.0 and d.reduction == "mean" and not d.is_plain
    d = _wrap(False, weight=w, label_smoothing=0.1, reduction="sum")._fusable(emb)
    assert torch.equal(d.weight, w) and d.smoothing == 0.1 and d.reduction == "sum"
    d = _wrap(False, reduction="sum")._fusable(emb)
    assert d.weight is None and d.reduction == "sum" and not d.is_plain


def test_fusable_is_none_for_each_excluded_criterion():
    emb = _DeviceEmb()
    assert _wrap(False, reduction="none")._fusable(emb) is None
    assert _wrap(False, ignore_index=3)._fusable(emb) is None
    assert _wrap(False, weight=torch.ones(C, dtype=torch.float64))._fusable(emb) is None
    assert _wrap(False, weight=torch.ones(C + 1))._fusable(emb) is None
    assert _wrap(True, alpha=True).double()._fusable(emb) is None

    class Sub(nn.CrossEntropyLoss):
        pass

    wrap = _wrap(False)
    wrap.focal_loss = Sub()
    assert wrap._fusable(emb) is None
    # not a [B, in_features] embedding
    bad = _DeviceEmb()
    bad.shape = (4, 256)
    assert _wrap(True)._fusable(bad) is None


def test_state_dict_keys_unchanged():
    assert "focal_loss.alpha" in _wrap(True, alpha=True).state_dict()
    assert "focal_loss.weight" in _wrap(False, weight=torch.ones(C)).state_dict()
    assert set(_wrap(True).state_dict()) == {"add_margin.weight"}


def test_synthetic_config_builder_passes_the_criterion_through():
    synth = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pets-face-recognition_amd", "configs", "synthetic")
    src = open(os.path.join(synth, "_common.py")).read()
    sig = src[src.index("def make("):src.index("torch.manual_seed(seed)")]
    assert "loss_kwargs=None" in sig and "is_focal=True" in sig
    assert "is_focal=is_focal" in src and "loss_kwargs=loss_kwargs" in src
    cfg = open(os.path.join(synth, "fe_r18_mi355x_smooth.py")).read()
    assert "is_focal=False" in cfg and "label_smoothing=0.1" in cfg
