"""Trainer(ema_decay=) / Trainer(stochastic_weight_avg=, swa_epoch_start=, swa_lrs=, annealing_epochs=, annealing_strategy=) on the CPU
path against torch.optim.swa_utils (AveragedModel, SWALR, update_bn) driven by hand on the same seed, the checkpoint's
`averaged_state_dict`, resuming an average, and the argument checks."""
import os
import sys

import pytest
import torch
from torch.optim import swa_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic")


class _Cfg(dict):
    __getattr__ = dict.get


def _fixed_batches(ns, n=3):
    torch.manual_seed(5)
    batches = [b for _, b in zip(range(n), ns['train_dataloader']())]
    ns['train_dataloader'] = lambda: batches
    return batches


def _small_config(tmp_path, monkeypatch):
    """a fe_r18_cpu-style namespace (ResNet-18 + ArcFace, torch.optim.SGD with the reference's three groups) at 64x64, with three
    fixed training batches"""
    import pets_face_recognition_amd as pfr
    pfr.install_reference_aliases()
    monkeypatch.chdir(tmp_path)
    if SYNTH not in sys.path:
        sys.path.insert(0, SYNTH)
    from _common import make
    ns = {}
    make(ns, arch='resnet18', n_train_ids=12, n_val_ids=4, photos=4, image_size=64, train_bs=8, test_bs=8, device='cpu',
         limit_train_batches=3, n_pairs=10)
    batches = _fixed_batches(ns)
    return _Cfg(ns), batches


def _fe_r18_cpu_config(tmp_path, monkeypatch):
    """configs/synthetic/fe_r18_cpu.py itself, with its first three training batches fixed"""
    import pets_face_recognition_amd as pfr
    pfr.install_reference_aliases()
    monkeypatch.chdir(tmp_path)
    from pets_face_recognition_amd.utils import get_dict_wrapper
    ns = dict(get_dict_wrapper(os.path.join(SYNTH, "fe_r18_cpu.py")).__dict__)
    batches = _fixed_batches(ns)
    return _Cfg(ns), batches


def _controller(cfg, seed=11):
    from pets_face_recognition_amd.engine.controller import Controller
    torch.manual_seed(seed)
    return Controller(cfg)


def _assert_state_close(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.allclose(sa[k].float(), sb[k].float()), k


def test_swa_run_matches_swa_utils(tmp_path, monkeypatch):
    from pets_face_recognition_amd.engine import Trainer
    cfg, batches = _fe_r18_cpu_config(tmp_path, monkeypatch)
    E, start = 5, 3                      # int(0.6 * 5)
    a = _controller(cfg)
    t = Trainer(gpus=0, max_epochs=E, check_val_every_n_epoch=100, prefetch_batches=0, limit_train_batches=3,
                stochastic_weight_avg=True, swa_epoch_start=0.6, swa_lrs=0.02, annealing_epochs=2)
    t.fit(a)
    # by hand: the same loop with torch.optim.swa_utils
    b = _controller(cfg)
    (opt,), (sched,) = b.configure_optimizers()
    assert isinstance(opt, torch.optim.SGD)
    params = [p for g in opt.param_groups for p in g['params']]
    holder = torch.nn.ParameterList(params)      # AveragedModel averages a module's parameters
    # (torch's lerp form of the running mean, what AveragedModel itself picks on a GPU; its CPU default divides instead, 1 ulp apart)
    swa_model = swa_utils.AveragedModel(holder, multi_avg_fn=swa_utils.get_swa_multi_avg_fn())
    swalr, lrs = None, []
    for epoch in range(E):
        b.train()
        if epoch >= start and swalr is None:
            swalr = swa_utils.SWALR(opt, swa_lr=0.02, anneal_epochs=2, anneal_strategy='cos')
        lrs.append([g['lr'] for g in opt.param_groups])
        for bi, batch in enumerate(batches):
            opt.zero_grad()
            b.training_step(batch, bi).backward()
            opt.step()
        if swalr is not None:
            swa_model.update_parameters(holder)
            swalr.step()
        else:
            sched.step()
    with torch.no_grad():
        for p, q in zip(params, swa_model.module.parameters()):
            p.copy_(q)
    swa_utils.update_bn((x['x'] for x in batches), b.model_loss)
    assert t.lr_history == lrs
    assert lrs[start] == lrs[0] and lrs[-1] != lrs[start]        # SWALR took over and its anneal moved the rates
    assert int(swa_model.n_averaged) == E - start
    _assert_state_close(a, b)
    # the averaged model is not the last iterate: the check above is not vacuous
    c = _controller(cfg)
    assert not torch.allclose(a.state_dict()['model_loss.module.fc.weight'], c.state_dict()['model_loss.module.fc.weight'])


class _Recorder:
    """records a checksum of the backbone's parameters whenever the trainer validates"""
    def __init__(self, controller):
        self.c, self.sums = controller, []
        controller.validation_step = self.step
        controller.validation_epoch_end = lambda outputs: {}

    def step(self, batch, bi=0, di=0):
        self.sums.append(float(sum(p.double().sum() for p in self.c.model_loss.module.parameters())))
        return {}


def _ema_by_hand(cfg, batches, epochs, decay):
    b = _controller(cfg)
    (opt,), _ = b.configure_optimizers()
    params = [p for g in opt.param_groups for p in g['params']]
    holder = torch.nn.ParameterList(params)
    ema = swa_utils.AveragedModel(holder, multi_avg_fn=swa_utils.get_ema_multi_avg_fn(decay))
    for epoch in range(epochs):
        b.train()
        for bi, batch in enumerate(batches):
            opt.zero_grad()
            b.training_step(batch, bi).backward()
            opt.step()
            ema.update_parameters(holder)
    return b, params, list(ema.module.parameters())


def test_ema_run_validates_and_saves_the_average(tmp_path, monkeypatch):
    from pets_face_recognition_amd.engine import Trainer
    cfg, batches = _small_config(tmp_path, monkeypatch)
    a = _controller(cfg)
    rec = _Recorder(a)
    t = Trainer(gpus=0, max_epochs=2, prefetch_batches=0, limit_train_batches=3, limit_val_batches=1, ema_decay=0.9,
                enable_checkpointing=True, default_root_dir=str(tmp_path / 'ckpt'))
    t.fit(a)
    b, params, avg = _ema_by_hand(cfg, batches, 2, 0.9)
    # the live weights are the plain run's, the average is AveragedModel's
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(va, vb), k
    names = {id(p): n for n, p in b.named_parameters()}
    loop = torch.load(str(tmp_path / 'ckpt' / 'epoch=1.ckpt.trainer'), map_location='cpu', weights_only=True)
    asd = loop['averaged_state_dict']
    live = torch.load(str(tmp_path / 'ckpt' / 'epoch=1.ckpt'), map_location='cpu', weights_only=True)
    assert list(asd) == list(live) == list(b.state_dict())         # the reference's key set
    for p, q in zip(params, avg):
        assert torch.allclose(asd[names[id(p)]], q.detach()), names[id(p)]
        assert not torch.equal(asd[names[id(p)]], live[names[id(p)]])
    for k, v in b.state_dict().items():
        if 'running_' in k or 'num_batches' in k:
            assert torch.equal(asd[k], v), k                           # live buffers
    # validation after the last epoch saw the averaged backbone, not the live one
    backbone = {id(p) for p in b.model_loss.module.parameters()}
    want = float(sum(q.detach().double().sum() for p, q in zip(params, avg) if id(p) in backbone))
    live_sum = float(sum(p.detach().double().sum() for p in b.model_loss.module.parameters()))
    assert len(rec.sums) == 2
    assert abs(rec.sums[-1] - want) <= 1e-6 * max(1.0, abs(want)) and abs(want - live_sum) > 1e-4
    # validate() outside fit() also runs on the average, and leaves the live weights in place
    t.validate(a)
    assert abs(rec.sums[-1] - want) <= 1e-6 * max(1.0, abs(want))
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(va, vb), k


@pytest.mark.parametrize("mode", ["ema", "swa"])
def test_resume_continues_the_average(tmp_path, monkeypatch, mode):
    from pets_face_recognition_amd.engine import Trainer
    cfg, batches = _small_config(tmp_path, monkeypatch)
    kw = dict(ema_decay=0.9) if mode == "ema" else dict(stochastic_weight_avg=True, swa_epoch_start=1, annealing_epochs=2, swa_lrs=0.02)
    common = dict(gpus=0, max_epochs=4, check_val_every_n_epoch=100, prefetch_batches=0, limit_train_batches=3,
                  enable_checkpointing=True, **kw)
    a = _controller(cfg)
    ta = Trainer(default_root_dir=str(tmp_path / 'a'), **common)
    ta.fit(a)
    b = _controller(cfg, seed=12)        # other initial weights: everything must come from the checkpoint
    tb = Trainer(default_root_dir=str(tmp_path / 'b'), resume_from_checkpoint=str(tmp_path / 'a' / 'epoch=1.ckpt'), **common)
    tb.fit(b)
    assert tb._averager.n_averaged == ta._averager.n_averaged > 0
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.allclose(va.float(), vb.float()), k
    for x, y in zip(ta._averager.avg, tb._averager.avg):
        assert torch.allclose(x, y)
    assert tb.lr_history == ta.lr_history[2:]


def test_weight_average_arguments_are_validated():
    from pets_face_recognition_amd.engine import Trainer
    from pets_face_recognition_amd.optim import WeightAverage
    for bad in (0, 1, 1.5, -0.1, "0.9", True):
        with pytest.raises(ValueError):
            Trainer(ema_decay=bad)
    with pytest.raises(ValueError):
        Trainer(ema_decay=0.9, stochastic_weight_avg=True)
    with pytest.raises(ValueError):
        Trainer(stochastic_weight_avg=True, swa_epoch_start=1.5)
    with pytest.raises(ValueError):
        Trainer(stochastic_weight_avg=True, annealing_strategy='exp')
    t = Trainer(stochastic_weight_avg=True)
    assert (t.swa_epoch_start, t.swa_lrs, t.annealing_epochs, t.annealing_strategy) == (0.8, None, 10, 'cos')
    t = Trainer()
    assert t.ema_decay is None and t.stochastic_weight_avg is False
    p = [torch.nn.Parameter(torch.ones(3))]
    with pytest.raises(ValueError):
        WeightAverage(p, 'ema')
    with pytest.raises(ValueError):
        WeightAverage(p, 'mean')
    with pytest.raises(ValueError):
        WeightAverage(p, 'swa', 0.9)


def test_weight_average_helper_matches_averaged_model():
    """optim.WeightAverage (the CPU path's averager): update / swap / state round trip"""
    from pets_face_recognition_amd.optim import WeightAverage
    g = torch.Generator().manual_seed(0)
    for kind, decay, ref_kw in (("ema", 0.9, dict(multi_avg_fn=swa_utils.get_ema_multi_avg_fn(0.9))), ("swa", None, dict(multi_avg_fn=swa_utils.get_swa_multi_avg_fn()))):
        ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(5, 3, generator=g)), torch.nn.Parameter(torch.randn(7, generator=g))])
        wa = WeightAverage(list(ps), kind, decay)
        ref = swa_utils.AveragedModel(ps, **ref_kw)
        for _ in range(4):
            with torch.no_grad():
                for p in ps:
                    p.add_(torch.randn(p.shape, generator=g))
            wa.update_average()
            ref.update_parameters(ps)
        for a, r in zip(wa.avg, ref.module.parameters()):
            assert torch.allclose(a, r.detach())
        live = [p.detach().clone() for p in ps]
        with wa.swap_averaged():
            for p, r in zip(ps, ref.module.parameters()):
                assert torch.allclose(p.detach(), r.detach())
        for p, l_ in zip(ps, live):
            assert torch.equal(p.detach(), l_)
        wb = WeightAverage(list(ps), kind, decay)
        wb.load_state_dict(wa.state_dict())
        assert wb.n_averaged == 4 and all(torch.equal(x, y) for x, y in zip(wa.avg, wb.avg))
