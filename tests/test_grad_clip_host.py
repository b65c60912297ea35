"""Trainer(gradient_clip_val=, gradient_clip_algorithm=, track_grad_norm=) on the CPU path (PL 1.5 semantics,
reference engine/trainer.py:73-74,87,481-505): torch.nn.utils clipping of the optimizer's parameters between backward and step,
PL's argument checks, and PL's grad_norm dictionary."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic")


class _Cfg(dict):
    __getattr__ = dict.get


def _r18_cpu_config(tmp_path, monkeypatch, **clip):
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
         limit_train_batches=3, n_pairs=10, **clip)
    torch.manual_seed(5)
    batches = [b for _, b in zip(range(3), ns['train_dataloader']())]
    ns['train_dataloader'] = lambda: batches
    return _Cfg(ns), batches


def _controller(cfg, seed=11):
    from pets_face_recognition_amd.engine.controller import Controller
    torch.manual_seed(seed)
    return Controller(cfg)


@pytest.mark.parametrize("algorithm", ["norm", "value"])
def test_cpu_trainer_clips_like_torch(tmp_path, monkeypatch, algorithm):
    from pets_face_recognition_amd.engine import Trainer
    cfg, batches = _r18_cpu_config(tmp_path, monkeypatch, gradient_clip_val=0.05, gradient_clip_algorithm=algorithm)
    assert cfg.trainer_kwargs['gradient_clip_val'] == 0.05 and cfg.trainer_kwargs['gradient_clip_algorithm'] == algorithm
    a = _controller(cfg)
    Trainer(gpus=0, max_epochs=1, check_val_every_n_epoch=100, prefetch_batches=0, **cfg.trainer_kwargs).fit(a)
    # the same model stepped by hand: backward -> torch.nn.utils clipping of the optimizer's parameters -> SGD step
    b = _controller(cfg)
    opt = b.configure_optimizers()[0][0]
    assert isinstance(opt, torch.optim.SGD)
    params = [p for g in opt.param_groups for p in g['params']]
    clipped = []
    for bi, batch in enumerate(batches):
        b.train()
        opt.zero_grad()
        b.training_step(batch, bi).backward()
        if algorithm == 'norm':
            clipped.append(float(torch.nn.utils.clip_grad_norm_(params, 0.05)) > 0.05)
        else:
            clipped.append(any(bool((p.grad.abs() >= 0.05).any()) for p in params))
            torch.nn.utils.clip_grad_value_(params, 0.05)
        opt.step()
    assert all(clipped)     # the clip is active on every step: an unclipped run would end elsewhere
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(va, vb), k


def test_clip_arguments_are_validated_like_pl():
    from pets_face_recognition_amd.engine import Trainer
    with pytest.raises(TypeError):
        Trainer(gradient_clip_val="1.0")
    with pytest.raises(TypeError):
        Trainer(gradient_clip_val=[1.0])
    with pytest.raises(ValueError):
        Trainer(gradient_clip_val=1.0, gradient_clip_algorithm="l2")
    for bad in (0, -2, "two", "-inf", [2]):
        with pytest.raises(ValueError):
            Trainer(track_grad_norm=bad)
    t = Trainer(gradient_clip_val=1, gradient_clip_algorithm="VALUE", track_grad_norm="inf")
    assert t.gradient_clip_algorithm == "value" and t.track_grad_norm == float("inf")
    t = Trainer(gradient_clip_val=0.5)
    assert t.gradient_clip_algorithm == "norm" and t.track_grad_norm == -1.0
    Trainer(track_grad_norm=-1)
    Trainer(track_grad_norm=1)
    Trainer(track_grad_norm=2.5)


def _tiny_config():
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    g = torch.Generator().manual_seed(0)
    xs = torch.rand(24, 3, 8, 8, generator=g)
    ys = torch.randint(0, 6, (24,), generator=g)
    data = [{"x": xs[i:i + 8], "label": ys[i:i + 8], "index": torch.arange(i, i + 8)} for i in range(0, 24, 8)]

    def optimizer(ml):
        return [torch.optim.SGD(ml.parameters(), 0.05, momentum=0.9)], []

    return _Cfg(model=lambda: torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(192, 512)),
                loss=lambda config, m: SoftmaxBasedMetricLearning(m, 6, 512, is_focal=True, arc_margin=True),
                optimizer=optimizer, train_dataloader=lambda: data, val_dataloader=lambda: data, n_epochs=1)


@pytest.mark.parametrize("norm", [2, 1, "inf", 3])
def test_track_grad_norm_dictionary(norm):
    """PL 1.5 grad_norm(): 'grad_{float(p)}_norm_{name}' over named parameters with a gradient plus '..._total', rounded to 4
    digits, on the steps where (global_step + 1) % log_every_n_steps == 0, handed to logger.log_metrics"""
    from pets_face_recognition_amd.engine import Trainer

    class Logger:
        def __init__(self):
            self.calls = []

        def log_metrics(self, metrics, step=None):
            # called before the optimizer step: the gradients the dictionary was made from are still in place
            p = float(norm)
            exp = {f"grad_{p}_norm_{n}": torch.linalg.vector_norm(q.grad, p).item()
                   for n, q in ctrl.named_parameters() if q.grad is not None}
            exp[f"grad_{p}_norm_total"] = torch.linalg.vector_norm(torch.tensor(list(exp.values())), p).item()
            self.calls.append((step, dict(metrics), {k: round(v, 4) for k, v in exp.items()}))

    torch.manual_seed(0)
    from pets_face_recognition_amd.engine.controller import Controller
    ctrl = Controller(_tiny_config())
    log = Logger()
    t = Trainer(gpus=0, max_epochs=1, check_val_every_n_epoch=100, prefetch_batches=0, logger=log, log_every_n_steps=2,
                track_grad_norm=norm)
    t.fit(ctrl)
    assert [c[0] for c in log.calls] == [1]          # global_step 1 is the step with (global_step + 1) % 2 == 0
    step, got, exp = log.calls[0]
    assert got == exp
    p = float(norm)
    assert set(got) == {f"grad_{p}_norm_model_loss.module.1.weight", f"grad_{p}_norm_model_loss.module.1.bias",
                        f"grad_{p}_norm_model_loss.add_margin.weight", f"grad_{p}_norm_total"}
    assert all(v == round(v, 4) for v in got.values()) and got[f"grad_{p}_norm_total"] > 0
    assert t.grad_norm_history == [got]
