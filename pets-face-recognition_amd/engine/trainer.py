"""`Trainer` — a plain training / evaluation driver with the call surface the reference uses
(`Trainer(gpus=…, max_epochs=…, strategy=…, default_root_dir=…, logger=…, enable_checkpointing=…, callbacks=…,
**trainer_kwargs)`, `.fit(controller)`, `.test(controller)`), replacing the copy of PyTorch-Lightning's Trainer in
/root/reference/engine/trainer.py:66-652 and the custom loops of engine/loops/*.py.  Order of operations kept from the
reference: per batch zero_grad → training_step → backward → optimizer.step (PL automatic optimisation,
trainer.py:403-413); validation at the end of every epoch, then a barrier when distributed, then the LR-scheduler
step (loops/train_loop.py:13-38); evaluation outputs are handed over as List[dataloader][batch]
(loops/eval_loop.py:30-51); no sanity-validation steps, no sampler replacement, private BN statistics per rank
(trainer.py:105,110,118); one checkpoint (bare state_dict, reference key names) per epoch plus a `.trainer` sidecar
(epoch, global_step, optimizer_states, lr_schedulers — PL's checkpoint keys) that `resume_from_checkpoint=` /
`fit(ckpt_path=)` restart from (trainer.py:111,399; a PL-format checkpoint holding the same keys is read too).
`gradient_clip_val` / `gradient_clip_algorithm` / `track_grad_norm` as in PL 1.5 (trainer.py:73-74,87,481-505), in the order of
its OptimizerLoop._track_and_norm_grad: backward -> gradient all-reduce -> track -> clip -> optimizer.step.

Weight averaging (off by default; the two modes exclude each other; both average the parameters of `optims[0]`):

`ema_decay=d`, 0 < d < 1: avg <- d * avg + (1 - d) * p after every optimizer step (the first step copies), inside the fused
optimizer's update kernel on the HIP path, `torch._foreach_lerp_` on the CPU path.  Validation and `test()` run on the averaged
parameters (inside `swap_averaged()`) with the LIVE BatchNorm running statistics, the usual EMA practice: an EMA follows the live
weights closely enough for their statistics.  The checkpoint holds the live weights as before; its `.trainer` sidecar also holds
`averaged_state_dict`, a state dict with the reference's key names made of the averaged parameters and the live buffers
(`eval_fe.py --averaged` loads it).

`stochastic_weight_avg=True` with `swa_epoch_start=0.8`, `swa_lrs=None`, `annealing_epochs=10`, `annealing_strategy='cos'`
(PL 1.5's names and defaults).  The contract is torch.optim.swa_utils' own:
  1. from epoch s = int(swa_epoch_start * max_epochs) on (an int swa_epoch_start is s itself) the config's schedulers no longer
     step; a `SWALR(optims[0], swa_lr, anneal_epochs=annealing_epochs, anneal_strategy=annealing_strategy)` is built at the start of
     epoch s and steps at the end of every epoch from s on; swa_lr per group is `swa_lrs` (a float or one per group) or the group's
     lr at that moment;
  2. `update_average()` (running mean, AveragedModel's default) runs at the end of every epoch from s on, before SWALR's step;
  3. after the last epoch the average is swapped in, `utils.update_bn` re-estimates the BatchNorm statistics over the train
     loader (limit_train_batches applies) and the result stays as the model's weights (and is what the last checkpoint holds).
Where this may differ from PL's StochasticWeightAveraging callback: the epoch bookkeeping around s (PL starts its SWALR and takes
its first average one epoch apart, and skips the BatchNorm pass's batches differently); the arithmetic of each piece is torch's.
The per-epoch learning rates of the last fit() are kept in `lr_history`.
Resume: `n_averaged` and the average travel in the optimizer's state dict (fused) or the sidecar's `weight_average` (torch
optimizers), SWALR's state in the sidecar's `swa_lr`; `resume_from_checkpoint` continues the average.  Under DDP every rank
averages its own, identical weights: no collective for the average.  SWA's final BatchNorm pass runs on each rank's shard of the
train loader; the buffers are then synchronised once (rank 0's statistics, as before every evaluation).

Distributed = one process per GPU started by torchrun (RANK / LOCAL_RANK / WORLD_SIZE), RCCL all-reduce of the flat
gradient buffer in buckets overlapped with backward (engine/ddp.py)."""
import os
import time
from pathlib import Path

import torch


def _to_device(batch, device):
    if isinstance(batch, dict):
        return {k: _to_device(v, device) for k, v in batch.items()}
    if isinstance(batch, (list, tuple)):
        return type(batch)(_to_device(v, device) for v in batch)
    if torch.is_tensor(batch):
        return batch.to(device, non_blocking=True)
    return batch


def _batch_size(batch):
    if isinstance(batch, dict):
        for v in batch.values():
            if torch.is_tensor(v) and v.dim() > 0:
                return int(v.shape[0])
    if isinstance(batch, (list, tuple)) and batch and torch.is_tensor(batch[0]):
        return int(batch[0].shape[0])
    return 0


class Trainer:
    def __init__(self, gpus=0, default_root_dir=None, strategy=None, max_epochs=1, logger=False, enable_checkpointing=False,
                 callbacks=None, num_sanity_val_steps=0, limit_train_batches=None, limit_val_batches=None,
                 check_val_every_n_epoch=1, log_every_n_steps=50, benchmark=None, fast_dev_run=False, prefetch_batches=2,
                 resume_from_checkpoint=None, resume_weights_only=False, gradient_clip_val=None, gradient_clip_algorithm=None,
                 track_grad_norm=-1, ema_decay=None, stochastic_weight_avg=False, swa_epoch_start=0.8, swa_lrs=None,
                 annealing_epochs=10, annealing_strategy='cos', **_ignored):
        # PL 1.5's checks (reference engine/trainer.py:481-505; its MisconfigurationException is a ValueError here)
        if gradient_clip_val is not None and not isinstance(gradient_clip_val, (int, float)):
            raise TypeError(f"`gradient_clip_val` should be an int or a float. Got {gradient_clip_val}.")
        if gradient_clip_algorithm is not None:
            if not isinstance(gradient_clip_algorithm, str):
                raise TypeError(f"`gradient_clip_algorithm` should be a str. Got {gradient_clip_algorithm}.")
            if gradient_clip_algorithm.lower() not in ('norm', 'value'):
                raise ValueError(f"`gradient_clip_algorithm` {gradient_clip_algorithm} is invalid. Allowed algorithms: ['value', 'norm'].")
        if track_grad_norm != -1 and not ((isinstance(track_grad_norm, (int, float)) or track_grad_norm == 'inf')
                                          and float(track_grad_norm) > 0):
            raise ValueError(f"`track_grad_norm` must be a positive number or 'inf' (infinity norm). Got {track_grad_norm}.")
        if ema_decay is not None and not (isinstance(ema_decay, (int, float)) and not isinstance(ema_decay, bool)
                                          and 0.0 < float(ema_decay) < 1.0):
            raise ValueError(f"`ema_decay` must be a float in (0, 1). Got {ema_decay}.")
        if ema_decay is not None and stochastic_weight_avg:
            raise ValueError("`ema_decay` and `stochastic_weight_avg` are two weight averages of the same parameters: set one of them.")
        if stochastic_weight_avg:
            if isinstance(swa_epoch_start, bool) or not ((isinstance(swa_epoch_start, int) and swa_epoch_start >= 1)
                                                         or (isinstance(swa_epoch_start, float) and 0.0 <= swa_epoch_start <= 1.0)):
                raise ValueError(f"`swa_epoch_start` should be a positive integer or a float between 0 and 1. Got {swa_epoch_start}.")
            if annealing_strategy not in ('cos', 'linear'):
                raise ValueError(f"`annealing_strategy` should be 'cos' or 'linear'. Got {annealing_strategy}.")
            if not (isinstance(annealing_epochs, int) and annealing_epochs >= 0):
                raise ValueError(f"`annealing_epochs` should be a non-negative integer. Got {annealing_epochs}.")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.stochastic_weight_avg = bool(stochastic_weight_avg)
        self.swa_epoch_start, self.swa_lrs = swa_epoch_start, swa_lrs
        self.annealing_epochs, self.annealing_strategy = annealing_epochs, annealing_strategy
        self.lr_history = []          # [lr of every param group of optims[0]] during each epoch of the last fit()
        self._averager = None         # the fused optimizer itself or an optim.WeightAverage (set by fit())
        self._loop_state = {}
        self.gradient_clip_val = gradient_clip_val
        self.gradient_clip_algorithm = 'norm' if gradient_clip_algorithm is None else gradient_clip_algorithm.lower()
        self.track_grad_norm = float(track_grad_norm)
        self.grad_norm_history = []   # the grad_norm dictionaries of the logging steps of the last fit()
        self._track_norm = None       # optim.fused.SegmentNorm of the tracked gradients (CUDA)
        self.gpus, self.root, self.strategy = gpus, default_root_dir, strategy
        self.max_epochs = 1 if fast_dev_run else max_epochs
        self.logger = logger if logger else None
        self.enable_checkpointing = enable_checkpointing
        self.callbacks = callbacks or []
        self.limit_train_batches = 1 if fast_dev_run else limit_train_batches
        self.limit_val_batches = 1 if fast_dev_run else limit_val_batches
        self.check_val_every_n_epoch = check_val_every_n_epoch
        self.log_every_n_steps = log_every_n_steps
        self.world = int(os.environ.get('WORLD_SIZE', '1'))
        self.rank = int(os.environ.get('RANK', '0'))
        self.local_rank = int(os.environ.get('LOCAL_RANK', '0'))
        self.global_step = 0
        self.ddp = None
        self.resume_from_checkpoint = resume_from_checkpoint
        self.resume_weights_only = resume_weights_only   # a bare state dict without its .trainer sidecar restarts at epoch 0 instead of raising
        # batches copied to the device ahead of the step on a copy stream (data_loading/prefetch.py); 0: plain .to() per batch
        self.prefetch_batches = int(prefetch_batches)
        self.train_img_s = None      # end-to-end images/s of the last fit() (loader + copy + step), first 5 steps excluded

    # ------------------------------------------------------------------
    @property
    def is_distributed_run(self):
        return self.strategy is not None and self.world > 1

    def _device(self):
        if not self.gpus:
            return torch.device('cpu')
        if self.is_distributed_run:
            return torch.device('cuda', self.local_rank)
        return torch.device('cuda', self.gpus[0] if isinstance(self.gpus, (list, tuple)) else 0)

    def _setup(self, controller):
        device = self._device()
        if device.type == 'cuda':
            torch.cuda.set_device(device)
        p0 = next(controller.parameters(), None)
        if p0 is None or p0.device != device:
            controller.to(device)      # (a redundant .to() would make the HIP models drop and rebuild their engines)
        controller.logger = self.logger
        if self.is_distributed_run:
            import torch.distributed as dist
            if not dist.is_initialized():
                os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
                dist.init_process_group('nccl' if device.type == 'cuda' else 'gloo')
            if device.type == 'cuda':
                from .ddp import FlatDDP
                eng = controller.model_loss.module.hip_engine(device)
                if self.ddp is None or self.ddp.eng is not eng:
                    # (re)bind: a new engine means new flat gradient buffers — the old reducer would all-reduce stale memory
                    if self.ddp is not None:
                        self.ddp.detach()
                    self.ddp = FlatDDP(controller.model_loss, bucket_mb=self.strategy.get('bucket_mb', 25))
            elif self.ddp is None or self.ddp.module is not controller.model_loss:
                # (re)bind: main.py builds a fresh Controller after the batch-size / lr finders — a reducer kept from the discarded
                # one would neither broadcast rank 0's new parameters nor all-reduce the new model's gradients
                from .ddp import GenericDDP
                self.ddp = GenericDDP(controller.model_loss)
        return device

    # ------------------------------------------------------------------ checkpoint / resume
    def _save_checkpoint(self, controller, optims, scheds, epoch, swalr=None):
        root = Path(self.root)
        root.mkdir(parents=True, exist_ok=True)
        torch.save(controller.state_dict(), root / f'epoch={epoch}.ckpt')
        loop = {'epoch': epoch + 1, 'global_step': self.global_step,
                'optimizer_states': [o.state_dict() for o in optims],
                'lr_schedulers': [s.state_dict() for s in scheds]}
        avg = self._averager
        if avg is not None:
            from ..optim.fused import WeightAverage
            if isinstance(avg, WeightAverage):
                loop['weight_average'] = avg.state_dict()
            loop['swa_lr'] = None if swalr is None else swalr.state_dict()
            if self.ema_decay is not None and avg.n_averaged > 0:
                with avg.swap_averaged():
                    loop['averaged_state_dict'] = {k: v.detach().cpu().clone() for k, v in controller.state_dict().items()}
        torch.save(loop, root / f'epoch={epoch}.ckpt.trainer')

    def _attach_average(self, optim):
        """-> the object that averages optims[0]'s parameters (the fused optimizer itself, or an optim.WeightAverage), or None"""
        if self.ema_decay is None and not self.stochastic_weight_avg:
            return None
        from ..optim.fused import _FusedBase, WeightAverage
        kind, decay = ('ema', self.ema_decay) if self.ema_decay is not None else ('swa', None)
        if isinstance(optim, _FusedBase):
            optim.attach_average(kind, decay)
            return optim
        return WeightAverage([p for g in optim.param_groups for p in g['params']], kind, decay)

    def _swa_start(self):
        s = self.swa_epoch_start
        return int(s * self.max_epochs) if isinstance(s, float) else int(s)

    def _make_swalr(self, optim, resumed=False):
        from torch.optim.swa_utils import SWALR
        groups = optim.param_groups
        if resumed:      # the groups' swa_lr came back with the optimizer state
            lrs = [g['swa_lr'] for g in groups]
        elif self.swa_lrs is None:
            lrs = [g['lr'] for g in groups]
        else:
            lrs = list(self.swa_lrs) if isinstance(self.swa_lrs, (list, tuple)) else [self.swa_lrs] * len(groups)
        return SWALR(optim, swa_lr=lrs if len(lrs) > 1 else lrs[0], anneal_epochs=self.annealing_epochs,
                     anneal_strategy=self.annealing_strategy)

    def _finish_swa(self, controller, device):
        """contract step 3: the average becomes the model, with BatchNorm statistics of its own"""
        from ..utils import update_bn
        self._averager.swap_averaged_()

        def images():
            for bi, batch in enumerate(controller.train_dataloader()):
                if self.limit_train_batches is not None and bi >= self.limit_train_batches:
                    break
                yield controller._images(_to_device(batch, device), True)      # the batch itself: a device_align config needs its 'pts'
        update_bn(images(), controller.model_loss)
        if self.ddp is not None:
            self.ddp.sync_buffers()   # each rank saw its own shard: every rank keeps rank 0's statistics

    def _resume(self, controller, optims, scheds, path, device):
        """→ first epoch to run.  `path`: an `epoch=N.ckpt` of this trainer (state dict; loop state in its `.trainer` sidecar) or a
        pytorch-lightning checkpoint ({'state_dict', 'epoch', 'global_step', 'optimizer_states', 'lr_schedulers'}).  Like PL
        (trainer.py:306-308) a missing file raises, and training continues at the beginning of the next epoch."""
        path = Path(path)
        if not path.is_file():
            raise FileNotFoundError(f"resume_from_checkpoint: no checkpoint at {path}")
        # torch >= 2.6 unpickles with weights_only=True by default: fine for this trainer's own files (tensors, dicts, lists, numbers),
        # not for a pytorch-lightning checkpoint (callbacks, AttributeDict hyper-parameters, ...).  The checkpoint is the user's own file,
        # as it is for PL's `resume_from_checkpoint`: try the safe load first, fall back to the full unpickler and say so.
        def load(p_):
            import pickle
            try:
                return torch.load(str(p_), map_location='cpu', weights_only=True)
            except pickle.UnpicklingError as e:   # a global the safe unpickler does not allow; truncated files, I/O errors etc. propagate
                print(f'resume_from_checkpoint: {Path(p_).name} holds more than tensors ({e.__class__.__name__}: {str(e)[:120]}); '
                      f'loading it with the full unpickler (it can run code: only resume from files you wrote)')
                return torch.load(str(p_), map_location='cpu', weights_only=False)
        ckpt = load(path)
        if isinstance(ckpt, dict) and 'state_dict' in ckpt:
            sd, loop = ckpt['state_dict'], ckpt
            if 'optimizer_states' not in ckpt and 'epoch' not in ckpt:
                # {'state_dict': ...} alone / a PL `save_weights_only` file: the same policy as a bare state dict
                if not self.resume_weights_only:
                    raise ValueError(f"resume_from_checkpoint: {path.name} holds a state_dict but no loop state (epoch, optimizer, LR "
                                     f"schedule); pass Trainer(resume_weights_only=True) to restart at epoch 0 from these weights")
                loop = {}
        else:
            sd = ckpt
            side = Path(str(path) + '.trainer')
            if side.is_file():
                loop = load(side)
            elif self.resume_weights_only:
                loop = {}
            else:
                raise FileNotFoundError(f"resume_from_checkpoint: {path.name} is a bare state dict and its loop state {side.name} is missing "
                                        f"(epoch, optimizer, LR schedule); pass Trainer(resume_weights_only=True) to restart at epoch 0 from these weights")
        controller.load_state_dict(sd, strict=True)
        if loop and ('optimizer_states' in loop or 'lr_schedulers' in loop):
            ost, lst = loop.get('optimizer_states', []), loop.get('lr_schedulers', [])
            if len(ost) != len(optims) or len(lst) != len(scheds):
                raise ValueError(f"resume_from_checkpoint: the checkpoint holds {len(ost)} optimizer / {len(lst)} scheduler states, "
                                 f"configure_optimizers() built {len(optims)} / {len(scheds)}")
            for o, st in zip(optims, ost):
                o.load_state_dict(st)
            for s_, st in zip(scheds, lst):
                s_.load_state_dict(st)
        self.global_step = int(loop.get('global_step', 0))
        self._loop_state = {k: loop[k] for k in ('weight_average', 'swa_lr') if k in loop}   # what fit() still reads
        if 'epoch' not in loop:
            print(f'resume_from_checkpoint: {path.name} carries no loop state — weights only, starting at epoch 0')
        return int(loop.get('epoch', 0))

    # ------------------------------------------------------------------
    def fit(self, controller, ckpt_path=None):
        device = self._setup(controller)
        opt = controller.configure_optimizers()
        optims, scheds = (opt if isinstance(opt, (tuple, list)) and len(opt) == 2 and isinstance(opt[0], (list, tuple))
                          else ([opt], []))
        optim = optims[0]
        averager = self._averager = self._attach_average(optim)
        ema = averager if self.ema_decay is not None else None
        ema_by_hand = ema is not None and ema is not optim     # a torch optimizer: the average is updated after its step
        swa = averager if self.stochastic_weight_avg else None
        swa_start = self._swa_start() if swa is not None else None
        swalr = None
        self._loop_state = {}
        lr_history = []
        history = []
        reg_history = []     # a MagFace head's regulariser at the steps of `history`
        pair_history = []    # the pair term (losses/pair.py) at the steps of `history`
        gn_history = []
        first_epoch = 0
        ckpt_path = ckpt_path or self.resume_from_checkpoint
        if ckpt_path is not None:
            first_epoch = self._resume(controller, optims, scheds, ckpt_path, device)
            if averager is not None and 'weight_average' in self._loop_state and averager is not optim:
                averager.load_state_dict(self._loop_state['weight_average'])
            if swa is not None and self._loop_state.get('swa_lr') is not None:
                swalr = self._make_swalr(optim, resumed=True)
                swalr.load_state_dict(self._loop_state['swa_lr'])
            if self.ddp is not None and hasattr(self.ddp, 'broadcast_parameters'):
                self.ddp.broadcast_parameters()
        for epoch in range(first_epoch, self.max_epochs):
            controller.current_epoch = epoch
            controller.train()
            if swa is not None and epoch >= swa_start and swalr is None:
                swalr = self._make_swalr(optim)
            lr_history.append([g['lr'] for g in optim.param_groups])
            loader = controller.train_dataloader()
            if device.type == 'cuda' and self.prefetch_batches > 0:
                from ..data_loading.prefetch import DevicePrefetcher
                loader = DevicePrefetcher(loader, device, self.prefetch_batches, self.limit_train_batches)
            t_mark, n_mark = None, 0
            for bi, batch in enumerate(loader):
                if self.limit_train_batches is not None and bi >= self.limit_train_batches:
                    break
                if bi == 5:      # throughput clock: after the first steps (plan build, allocator warm-up)
                    if device.type == 'cuda':
                        torch.cuda.synchronize(device)
                    t_mark, n_mark = time.perf_counter(), 0
                batch = _to_device(batch, device)
                n_mark += _batch_size(batch)
                optim.zero_grad()
                loss = controller.training_step(batch, bi)
                loss.backward()
                if self.ddp is not None:
                    self.ddp.finish_backward()
                if self.track_grad_norm > 0 and (self.global_step + 1) % self.log_every_n_steps == 0:
                    norms = self._grad_norm_dict(controller)
                    gn_history.append(norms)
                    if norms and self.logger is not None and self.rank == 0 and hasattr(self.logger, 'log_metrics'):
                        self.logger.log_metrics(norms, step=self.global_step)
                self._clip_gradients(optim)
                optim.step()
                if ema_by_hand:
                    ema.update_average()
                self.global_step += 1
                if self.global_step % self.log_every_n_steps == 0 or bi == 0:
                    lv = float(loss.detach())
                    history.append(lv)
                    reg = getattr(controller, 'last_regulariser', None)
                    if reg is not None:
                        reg_history.append(float(reg.detach()))
                    pair = getattr(controller, 'last_pair_loss', None)
                    if pair is not None:
                        pair_history.append(float(pair.detach()))
                    if self.rank == 0:
                        print(f'epoch {epoch} step {self.global_step} loss {lv:.5f}' + (f' loss_g {reg_history[-1]:.5f}' if reg is not None else '')
                              + (f' loss_pair {pair_history[-1]:.5f}' if pair is not None else ''))
            if t_mark is not None and n_mark:
                if device.type == 'cuda':
                    torch.cuda.synchronize(device)
                self.train_img_s = n_mark * self.world / (time.perf_counter() - t_mark)
                if self.rank == 0:
                    print(f'epoch {epoch} train throughput {self.train_img_s:.1f} img/s (loader + copy + step, {self.world} process(es))')
            if (epoch + 1) % self.check_val_every_n_epoch == 0:
                self._run_eval(controller, device, 'val')
            if self.is_distributed_run:
                import torch.distributed as dist
                dist.barrier()
            if swalr is not None:
                swa.update_average()
                swalr.step()
                if epoch == self.max_epochs - 1:
                    self._finish_swa(controller, device)
            else:
                for s in scheds:
                    s.step()
            if self.enable_checkpointing and self.root is not None and self.rank == 0:
                self._save_checkpoint(controller, optims, scheds, epoch, swalr)
        self.lr_history = lr_history
        self.loss_history = history
        self.regulariser_history = reg_history
        self.pair_loss_history = pair_history
        self.grad_norm_history = gn_history
        return controller

    # ------------------------------------------------------------------ gradient clipping / norm tracking
    def _clip_gradients(self, optim):
        """PL 1.5 clip_gradients over the optimizer's own parameters (PL's main_params(optimizer)); a value <= 0 / None: no clipping.
        A fused optimizer folds the clip into its next step (device norm, no host sync); any other optimizer goes through
        torch.nn.utils."""
        clip_val = self.gradient_clip_val
        if clip_val is None or float(clip_val) <= 0:
            return
        clip_val = float(clip_val)
        from ..optim.fused import _FusedBase
        if isinstance(optim, _FusedBase):
            if self.gradient_clip_algorithm == 'value':
                optim.clip_grad_value_(clip_val)
            else:
                optim.clip_grad_norm_(clip_val, 2.0)
            return
        params = [p for group in optim.param_groups for p in group['params']]
        if self.gradient_clip_algorithm == 'value':
            torch.nn.utils.clip_grad_value_(params, clip_val)
        else:
            torch.nn.utils.clip_grad_norm_(params, clip_val)

    def _grad_norm_dict(self, controller):
        """PL 1.5's grad_norm(lightning_module, track_grad_norm): {'grad_{p}_norm_{name}': norm} over the parameters with a gradient,
        plus 'grad_{p}_norm_total', rounded to 4 digits.  CUDA gradients: one pfr_grad_norm call and one device-to-host copy
        (PL syncs once per parameter)."""
        p = self.track_grad_norm
        # (a Partial FC head with sparse_grad=True has no dense gradient: its norm is that of the sampled rows, weight.row_grad[1])
        named = [(n, q.grad if q.grad is not None else q.row_grad[1]) for n, q in controller.named_parameters()
                 if q.grad is not None or getattr(q, 'row_grad', None) is not None]
        if not named:
            return {}
        if named[0][1].is_cuda:
            from ..optim.fused import SegmentNorm
            if self._track_norm is None:
                self._track_norm = SegmentNorm()
            vals = self._track_norm.compute([g for _, g in named], p, copy_other=True).cpu().tolist()
            norms = {f'grad_{p}_norm_{n}': v for (n, _), v in zip(named, vals)}
            norms[f'grad_{p}_norm_total'] = vals[len(named)]
        else:
            norms = {f'grad_{p}_norm_{n}': g.norm(p).item() for n, g in named}
            norms[f'grad_{p}_norm_total'] = torch.tensor(list(norms.values())).norm(p).item()
        return {k: round(v, 4) for k, v in norms.items()}

    def _run_eval(self, controller, device, kind):
        avg = self._averager
        if self.ema_decay is not None and avg is not None and avg.n_averaged > 0:
            with avg.swap_averaged():      # EMA: evaluate the averaged parameters (live BatchNorm statistics)
                return self._eval_loop(controller, device, kind)
        return self._eval_loop(controller, device, kind)

    def _eval_loop(self, controller, device, kind):
        if self.ddp is not None:
            self.ddp.sync_buffers()   # every rank evaluates with rank 0's BN statistics (torch DDP's broadcast_buffers)
        controller.eval()
        loaders = controller.val_dataloader() if kind == 'val' else controller.test_dataloader()
        if not isinstance(loaders, (list, tuple)):
            loaders = [loaders]
        outputs = []
        with torch.no_grad():
            for di, loader in enumerate(loaders):
                outs = []
                for bi, batch in enumerate(loader):
                    if self.limit_val_batches is not None and bi >= self.limit_val_batches:
                        break
                    batch = _to_device(batch, device)
                    step = controller.validation_step if kind == 'val' else controller.test_step
                    outs.append(step(batch, bi, di))
                outputs.append(outs)
            res = controller.validation_epoch_end(outputs) if kind == 'val' else controller.test_epoch_end(outputs)
        controller.train()
        return res

    def test(self, controller):
        device = self._setup(controller)
        return self._run_eval(controller, device, 'test')

    def validate(self, controller):
        device = self._setup(controller)
        return self._run_eval(controller, device, 'val')
